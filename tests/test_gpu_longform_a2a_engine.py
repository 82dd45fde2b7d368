"""GPU: WindowedAudioToAudioEngine (engine.py) on the tiny UNet, W = 16 -- graph replay against eager launches for the four samplers
on a suffix of the schedule, masked and unmasked; a plan of one window against DenoiseEngine(begin_index, masked); the loop at
strength 0.5 against the restatement's windowed loop on the oracle UNet (tests/longform_a2a_restatement.py); the kept region; and
set_inpaint's shape errors.  Plans, window and overlap are those of tests/test_gpu_longform_engine.py."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_a2a_restatement as A  # noqa: E402
import longform_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

W, HW, OV = 16, 32, 8
# name -> (clips, rows, looped): windows of 32 rows, overlap 8
PLANS = {"b1_k3": (1, 72, False), "b2_k2": (2, 56, False), "b1_k3_looped": (1, 72, True)}
SOLVERS = ["ddim", "dpm", "unipc", "euler_a"]


@functools.lru_cache(maxsize=None)
def _models():
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from oracle import configs
    from oracle.unet import UNet2DConditionModel as OUNet
    cfg = configs.tiny_unet()
    torch.manual_seed(5)
    ref = OUNet(**cfg).eval()
    mine = UNet2DConditionModel(**cfg)
    mine.load_state_dict(ref.state_dict())
    return ref, mine.cuda()


def _scheduler(solver):
    from audioldm_with_lora_amd.scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,
                                                  UniPCMultistepScheduler)
    if solver == "ddim":
        return DDIMScheduler()
    cls = {"dpm": DPMSolverMultistepScheduler, "unipc": UniPCMultistepScheduler, "euler_a": EulerAncestralDiscreteScheduler}[solver]
    return cls.from_config(DDIMScheduler().config)


def _inputs(B, rows):
    """(the clip's latents x0, the noise, prompt and negative embeddings, a mask [B, rows, W] that keeps the first 20 rows and a band,
    with one fractional stripe)"""
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(B, 8, rows, W, generator=g)
    eps = torch.randn(B, 8, rows, W, generator=g)
    pe = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=-1)
    m = torch.ones(B, rows, W)
    m[:, :20] = 0.0
    m[:, 40:50, :4] = 0.0
    m[:, 30:34] = 0.25
    return x0, eps, pe, ne, m


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _start(s, x0, eps, begin):
    a, sg = s.add_noise_coefficients(begin)
    return float(a) * x0 + float(sg) * eps


@functools.lru_cache(maxsize=None)
def _run(plan_name, solver, steps, begin, masked, use_graph):
    """the engine's final long latents (NCHW, CPU), its last UNet input and the counter after the suffix"""
    from audioldm_with_lora_amd.engine import WindowedAudioToAudioEngine
    from audioldm_with_lora_amd.longform import WindowPlan
    B, rows, loop = PLANS[plan_name]
    plan = WindowPlan(rows, HW, OV, loop)
    x0, eps, pe, ne, m = _inputs(B, rows)
    s = _scheduler(solver)
    eng = WindowedAudioToAudioEngine(_models()[1], s, B, plan, W, steps, 2.5, use_graph=use_graph, begin_index=begin, masked=masked)
    assert eng.x.shape == (B, rows, W, 8) and eng.x_in[0].shape == (2 * B * plan.K, HW, W, 8) and eng.n_steps == steps - begin
    eng.set_condition(pe, ne)
    if solver == "euler_a":
        eng.set_seed(1234)
    s.set_timesteps(steps)
    eng.set_latents(_start(s, x0, eps, begin))
    if masked:
        eng.set_inpaint(x0, eps, m)
    eng.capture()
    assert (eng.graph is not None) == use_graph
    eng.run()
    return eng.latents_nchw().cpu(), eng.x_in[0].cpu(), int(eng.step_idx.item())


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_graph_replay_equals_eager_bitwise(solver, masked):
    """6 steps from index 2 over three windows with a shifted last one: the replayed graph and eager launches agree bit for bit, the
    counter wraps to 0 after the suffix"""
    a, ain, ca = _run("b1_k3", solver, 6, 2, masked, False)
    b, bin_, cb = _run("b1_k3", solver, 6, 2, masked, True)
    assert torch.equal(a, b) and torch.equal(ain.view(torch.int16), bin_.view(torch.int16)) and ca == cb == 0 and torch.isfinite(a).all()


@pytest.mark.parametrize("plan_name", ["b2_k2", "b1_k3_looped"])
def test_graph_replay_equals_eager_on_the_other_plans(plan_name):
    a, _, ca = _run(plan_name, "ddim", 10, 5, True, False)
    b, _, cb = _run(plan_name, "ddim", 10, 5, True, True)
    assert torch.equal(a, b) and ca == cb == 0


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_single_window_equals_the_plain_engine_bitwise(solver, masked):
    """K = 1 (rows == window): DenoiseEngine(begin_index, masked) bit for bit -- latents, the first and the last UNet input and, for
    Euler-ancestral with the same seed, the noise stream's state"""
    from audioldm_with_lora_amd.engine import DenoiseEngine, WindowedAudioToAudioEngine
    from audioldm_with_lora_amd.longform import WindowPlan
    x0, eps, pe, ne, m = _inputs(2, HW)
    out = []
    for windowed in (False, True):
        s = _scheduler(solver)
        if windowed:
            eng = WindowedAudioToAudioEngine(_models()[1], s, 2, WindowPlan(HW, HW, OV), W, 6, 2.5, begin_index=2, masked=masked)
            assert eng.K == 1
        else:
            eng = DenoiseEngine(_models()[1], s, 2, HW, W, 6, 2.5, begin_index=2, masked=masked)
        eng.set_condition(pe, ne)
        if solver == "euler_a":
            eng.set_seed(77)
        s.set_timesteps(6)
        eng.set_latents(_start(s, x0, eps, 2))
        if masked:
            eng.set_inpaint(x0, eps, m)
        first_in = eng.x_in[0].clone()
        eng.capture()
        eng.run()
        out.append((eng.latents_nchw().cpu(), first_in.cpu(), eng.x_in[0].cpu(), None if eng.rng is None else eng.rng.cpu()))
    for a, b in zip(*out):
        assert (a is None and b is None) or torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                                                        b.view(torch.int16) if b.dtype == torch.bfloat16 else b)
    assert torch.isfinite(out[0][0]).all()


@functools.lru_cache(maxsize=None)
def _oracle(plan_name, solver, masked):
    B, rows, loop = PLANS[plan_name]
    x0, eps, pe, ne, m = _inputs(B, rows)
    with torch.no_grad():
        return A.windowed_a2a_loop(_models()[0], R.make_restatement(solver), solver, x0, eps, pe, ne, 10, 5, 2.5,
                                   R.tables_of(rows, HW, OV, loop), mask=m if masked else None)


@pytest.mark.parametrize("plan_name", list(PLANS))
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("solver", ["ddim", "dpm"])
def test_engine_matches_the_restatement_loop_on_the_oracle_unet(solver, masked, plan_name):
    """A 10-step schedule at strength 0.5 (5 steps from index 5), g = 2.5.  The bound is tests/test_gpu_longform_engine.py's for this
    UNet and step count.  The plain engine's distance from the restatement on one 32-row window of the same inputs is recorded
    beside it.  Masked: the rows the mask keeps end on x0 bit for bit."""
    import conftest
    from audioldm_with_lora_amd.engine import DenoiseEngine
    got, _, counter = _run(plan_name, solver, 10, 5, masked, True)
    want = _oracle(plan_name, solver, masked)
    rel = _rel(got, want)
    conftest.record(rel, "windowed_a2a_rel_l2")
    B, rows, _ = PLANS[plan_name]
    x0, eps, pe, ne, m = _inputs(B, rows)
    cut = lambda t: t[:, :, :HW].contiguous()
    s = _scheduler(solver)
    eng = DenoiseEngine(_models()[1], s, B, HW, W, 10, 2.5, begin_index=5, masked=masked)
    eng.set_condition(pe, ne)
    s.set_timesteps(10)
    eng.set_latents(_start(s, cut(x0), cut(eps), 5))
    if masked:
        eng.set_inpaint(cut(x0), cut(eps), m[:, :HW].contiguous())
    eng.capture()
    eng.run()
    with torch.no_grad():
        one = A.windowed_a2a_loop(_models()[0], R.make_restatement(solver), solver, cut(x0), cut(eps), pe, ne, 10, 5, 2.5,
                                  R.tables_of(HW, HW, OV), mask=m[:, :HW] if masked else None)
    plain = _rel(eng.latents_nchw().cpu(), one)
    conftest.record(plain, "plain_engine_one_window_rel_l2")
    print(f"{solver} {plan_name} masked={masked}: windowed {rel:.3e}, plain engine on one window {plain:.3e}")
    assert got.shape == want.shape == (B, 8, rows, W) and torch.isfinite(got).all() and rel < 5e-2, rel
    assert counter == 0                                    # wrapped after exactly the suffix
    if masked:
        keep = (m == 0)[:, None].expand_as(got)
        assert keep.any() and (~keep).any() and torch.equal(got[keep], x0[keep])


def test_set_inpaint_shape_errors():
    from audioldm_with_lora_amd.engine import WindowedAudioToAudioEngine
    from audioldm_with_lora_amd.longform import WindowPlan
    plan = WindowPlan(72, HW, OV)
    x0, eps, pe, ne, m = _inputs(1, 72)
    eng = WindowedAudioToAudioEngine(_models()[1], _scheduler("ddim"), 1, plan, W, 6, 2.5, use_graph=False, begin_index=2, masked=True)
    eng.set_inpaint(x0, eps, m)
    assert torch.equal(eng.mask.cpu(), m) and eng.x0.shape == (1, 72, W, 8)
    for bad in ((x0[:, :, :HW], eps, m), (x0, eps[:, :, :HW], m), (x0, eps, m[:, :HW]), (x0, eps, m[0]),
                (x0.expand(2, -1, -1, -1), eps, m)):
        with pytest.raises(ValueError):
            eng.set_inpaint(*bad)
    un = WindowedAudioToAudioEngine(_models()[1], _scheduler("ddim"), 1, plan, W, 6, 2.5, use_graph=False, begin_index=2)
    with pytest.raises(ValueError):
        un.set_inpaint(x0, eps, m)
    with pytest.raises(NotImplementedError):
        WindowedAudioToAudioEngine(_models()[1], _scheduler("ddim"), 2, plan, W, 6, 2.5, chains=2, masked=True)
