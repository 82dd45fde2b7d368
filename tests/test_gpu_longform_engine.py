"""GPU: WindowedDenoiseEngine (engine.py) on the tiny UNet, W = 16 -- against the restatement's windowed loop over the oracle UNet
(tests/longform_restatement.py), graph replay against eager launches, a plan of one window against DenoiseEngine, the other
samplers, one prompt per window, and the options it does not take."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

W, HW, OV = 16, 32, 8
# name -> (clips, rows, looped): windows of 32 rows, overlap 8
PLANS = {"b1_k3": (1, 72, False),          # offsets 0, 24, 40: the last window is shifted
         "b2_k2": (2, 56, False),          # offsets 0, 24
         "b1_k3_looped": (1, 72, True)}    # offsets 0, 24, 48: the last window wraps over the seam


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
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(B, 8, rows, W, generator=g)
    pe = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=-1)
    return lat, pe, ne


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@functools.lru_cache(maxsize=None)
def _run(plan_name, solver, steps, use_graph, per_window_prompts=False):
    """the windowed engine's final latents (NCHW, CPU) and the counter after n_steps"""
    from audioldm_with_lora_amd.engine import WindowedDenoiseEngine
    from audioldm_with_lora_amd.longform import WindowPlan
    B, rows, loop = PLANS[plan_name]
    plan = WindowPlan(rows, HW, OV, loop)
    lat, pe, ne = _inputs(B, rows)
    s = _scheduler(solver)
    eng = WindowedDenoiseEngine(_models()[1], s, B, plan, W, steps, 2.5, use_graph=use_graph)
    assert eng.x.shape == (B, rows, W, 8) and eng.x_in[0].shape == (2 * B * plan.K, HW, W, 8) and eng.n_steps == steps
    if per_window_prompts:
        eng.set_condition(pe[:, None, :].expand(B, plan.K, 64).contiguous(), ne[:, None, :].expand(B, plan.K, 64).contiguous())
    else:
        eng.set_condition(pe, ne)
    if solver == "euler_a":
        eng.set_seed(1234)
    s.set_timesteps(steps)
    eng.set_latents(lat * s.init_noise_sigma)
    eng.capture()
    assert (eng.graph is not None) == use_graph
    eng.run()
    return eng.latents_nchw().cpu(), int(eng.step_idx.item())


@functools.lru_cache(maxsize=None)
def _oracle(plan_name, steps):
    from oracle.ddim import DDIMScheduler as ODDIM
    B, rows, loop = PLANS[plan_name]
    lat, pe, ne = _inputs(B, rows)
    with torch.no_grad():
        return R.windowed_loop(_models()[0], ODDIM(), lat, pe, ne, steps, 2.5, R.tables_of(rows, HW, OV, loop))


@pytest.mark.parametrize("plan_name", list(PLANS))
def test_windowed_engine_matches_the_restatement_loop_on_the_oracle_unet(plan_name):
    """10 DDIM steps, g = 2.5: the bound is tests/test_gpu_engine.py's for this UNet and step count.  The plain engine's distance
    from the oracle on one 32-row window of the same inputs is recorded beside it."""
    import conftest
    from audioldm_with_lora_amd.engine import DenoiseEngine
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from oracle.ddim import DDIMScheduler as ODDIM
    from oracle.pipeline import denoise_loop
    got, counter = _run(plan_name, "ddim", 10, True)
    want = _oracle(plan_name, 10)
    rel = _rel(got, want)
    conftest.record(rel, "windowed_rel_l2")
    B, rows, _ = PLANS[plan_name]
    lat, pe, ne = _inputs(B, rows)
    eng = DenoiseEngine(_models()[1], DDIMScheduler(), B, HW, W, 10, 2.5)
    eng.set_condition(pe, ne)
    eng.set_latents(lat[:, :, :HW].contiguous())
    eng.capture()
    eng.run()
    with torch.no_grad():
        plain = _rel(eng.latents_nchw().cpu(), denoise_loop(_models()[0], ODDIM(), lat[:, :, :HW].contiguous(), pe, ne, 10, 2.5))
    conftest.record(plain, "plain_engine_one_window_rel_l2")
    print(f"{plan_name}: windowed {rel:.3e}, plain engine on one window {plain:.3e}")
    assert got.shape == want.shape == (B, 8, rows, W) and torch.isfinite(got).all() and rel < 5e-2, rel
    assert counter == 0                                    # wrapped after exactly n_steps


@pytest.mark.parametrize("plan_name", list(PLANS))
def test_graph_replay_equals_eager_bitwise(plan_name):
    a, ca = _run(plan_name, "ddim", 10, False)
    b, cb = _run(plan_name, "ddim", 10, True)
    assert torch.equal(a, b) and ca == cb == 0


@pytest.mark.parametrize("solver", ["ddim", "euler_a"])
def test_single_window_equals_the_plain_engine_bitwise(solver):
    """K = 1 (rows == window): the windowed engine is DenoiseEngine bit for bit -- latents, the next UNet input and, for
    Euler-ancestral with the same seed, the noise stream's state"""
    from audioldm_with_lora_amd.engine import DenoiseEngine, WindowedDenoiseEngine
    from audioldm_with_lora_amd.longform import WindowPlan
    lat, pe, ne = _inputs(2, HW)
    out = []
    for windowed in (False, True):
        s = _scheduler(solver)
        if windowed:
            eng = WindowedDenoiseEngine(_models()[1], s, 2, WindowPlan(HW, HW, OV), W, 6, 2.5)
            assert eng.K == 1
        else:
            eng = DenoiseEngine(_models()[1], s, 2, HW, W, 6, 2.5)
        eng.set_condition(pe, ne)
        if solver == "euler_a":
            eng.set_seed(77)
        s.set_timesteps(6)
        eng.set_latents(lat * s.init_noise_sigma)
        first_in = eng.x_in[0].clone()
        eng.capture()
        eng.run()
        out.append((eng.latents_nchw().cpu(), first_in.cpu(), eng.x_in[0].cpu(), None if eng.rng is None else eng.rng.cpu()))
    for a, b in zip(*out):
        assert (a is None and b is None) or torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                                                        b.view(torch.int16) if b.dtype == torch.bfloat16 else b)
    assert torch.isfinite(out[0][0]).all()


@pytest.mark.parametrize("solver", ["dpm", "unipc", "euler_a"])
def test_other_samplers_replay_equals_eager(solver):
    """DPM-Solver++, UniPC and Euler-ancestral (fixed seed) at 6 steps over three windows: eager and replayed runs agree bit for bit,
    the counter wraps to 0, everything is finite"""
    a, ca = _run("b1_k3", solver, 6, False)
    b, cb = _run("b1_k3", solver, 6, True)
    assert torch.equal(a, b) and ca == cb == 0 and torch.isfinite(a).all()
    assert not torch.equal(a, _run("b1_k3", "ddim", 10, True)[0])


def test_equal_per_window_prompts_are_the_per_clip_prompt():
    a, _ = _run("b2_k2", "ddim", 10, True)
    b, _ = _run("b2_k2", "ddim", 10, True, True)
    assert torch.equal(a, b)


def test_a_prompt_per_window_changes_its_window_and_bad_shapes_raise():
    from audioldm_with_lora_amd.engine import WindowedDenoiseEngine
    from audioldm_with_lora_amd.longform import WindowPlan
    lat, pe, ne = _inputs(1, 72)
    plan = WindowPlan(72, HW, OV)
    eng = WindowedDenoiseEngine(_models()[1], _scheduler("ddim"), 1, plan, W, 4, 2.5, use_graph=False)
    sched = pe[:, None, :].repeat(1, plan.K, 1)
    sched[:, 2] = -sched[:, 2]                                       # another prompt for the last window (rows 40 .. 71)
    outs = []
    for cond in (pe, sched):
        eng.set_condition(cond, ne)
        eng.set_latents(lat)
        eng.run()
        outs.append(eng.latents_nchw().cpu())
    assert torch.isfinite(outs[1]).all() and not torch.equal(outs[0][:, :, 40:], outs[1][:, :, 40:])
    with pytest.raises(ValueError):
        eng.set_condition(pe[:, None, :].repeat(1, 2, 1), ne)        # K = 3
    with pytest.raises(ValueError):
        eng.set_adapters(["__base__", "__base__"])                   # neither 1 nor 3 entries


def test_unsupported_options_raise():
    from audioldm_with_lora_amd.engine import WindowedDenoiseEngine
    from audioldm_with_lora_amd.longform import WindowPlan
    plan = WindowPlan(72, HW, OV)
    for kw in (dict(masked=True), dict(chains=2), dict(begin_index=1)):
        with pytest.raises(NotImplementedError):
            WindowedDenoiseEngine(_models()[1], _scheduler("ddim"), 2, plan, W, 6, 2.5, **kw)
