"""GPU: UniPCMultistepScheduler + aldm_unipc_step_fused[_masked] against the restatement (tests/unipc_restatement.py) -- the eager step
and the fused kernel on an analytic model (with the wrap to row 0 and the ring's parity), the scalar / vector kernel paths, the
corrector-off launch against aldm_dpm_step_fused, the masked launch, the replayed engine on the tiny UNet (full, begun, masked), the
pipelines with the scheduler swapped (and swapped back), one full-width run and the inference script.

The bound of the kernel tests is measured, not chosen: the restatement is run twice on the same inputs, in fp32 (diffusers' own
arithmetic) and in float64, and the worst per-step relative L2 between the two is the rounding noise of the fp32 statement itself.  The
kernel folds the same sums into six coefficients and associates them differently, so it may sit up to 4 x that noise from the fp32
restatement (and never has to be closer than 1e-6, a few fp32 ulps of a relative L2)."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dpm_restatement import DPMSolverRestatement  # noqa: E402
from unipc_restatement import UniPCRestatement  # noqa: E402

pytestmark = pytest.mark.gpu

_NP = dict(predict_x0=False, final_sigmas_type="sigma_min")
VARIANTS = [dict(), dict(solver_type="bh1"), dict(solver_order=1), dict(solver_order=1, solver_type="bh1"),
            dict(_NP), dict(_NP, solver_type="bh1"), dict(_NP, solver_order=1), dict(_NP, solver_order=1, solver_type="bh1")]
IDS = ["x0-bh2-o2", "x0-bh1-o2", "x0-bh2-o1", "x0-bh1-o1", "eps-bh2-o2", "eps-bh1-o2", "eps-bh2-o1", "eps-bh1-o1"]


def _unipc(**kw):
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, UniPCMultistepScheduler
    return UniPCMultistepScheduler.from_config(DDIMScheduler().config, **kw)


def _dpm(**kw):
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(DDIMScheduler().config, **kw)


def _analytic_eps(x, t, mu, s, ac):
    """exact eps-prediction for data ~ N(mu, s^2) per element at timestep t"""
    a = float(ac[int(t)])
    return math.sqrt(1 - a) * (x - math.sqrt(a) * mu) / (a * s * s + 1 - a)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _bound(spread):
    return max(4.0 * spread, 1e-6)


def _model_eps(x, t, ac, cfg, g_scale):
    """the analytic model(s) of the fused tests: one model, or two as the unconditional / text halves"""
    eu = _analytic_eps(x, t, 0.4, 1.5, ac)
    if not cfg:
        return eu, eu
    et = _analytic_eps(x, t, -0.3, 0.8, ac)
    return torch.cat([eu, et]).contiguous(), eu + g_scale * (et - eu)


def _restatement_runs(make, x0, n, cfg=False, g_scale=1.0):
    """The restatement over n steps from x0, closed loop on the analytic model, in fp32 and in float64.  Returns the fp32 states after
    every step and the spread: the worst per-step relative L2 between the two runs."""
    runs = {}
    for dt in (torch.float32, torch.float64):
        r = make(dt)
        r.set_timesteps(n)
        x, out = x0.to(dt), []
        for k, t in enumerate(r.timesteps):
            _, e = _model_eps(x, t, r.alphas_cumprod.to(dt), cfg, g_scale)
            x = r.step(e, t, x).prev_sample
            out.append(x)
        runs[dt] = out
    spread = max(_rel(a, b) for a, b in zip(runs[torch.float32], runs[torch.float64]))
    return runs[torch.float32], spread


class _DPMRestatement64(DPMSolverRestatement):
    """DPMSolverRestatement with a dtype switch (its own step() pins the sample to fp32): the same statements in float64"""

    def __init__(self, dtype=torch.float32, **kw):
        super().__init__(**kw)
        self.dtype = dtype

    def set_timesteps(self, n, device=None):
        super().set_timesteps(n)
        self.sigmas = self.sigmas.to(self.dtype)

    def step(self, model_output, timestep, sample, eta=0.0, **kw):
        if self.step_index is None:
            self.step_index = int((self.timesteps == int(timestep)).nonzero()[0])
        model_output, sample = model_output.to(self.dtype), sample.to(self.dtype)
        m = self.convert_model_output(model_output, sample)
        self.model_outputs = self.model_outputs[1:] + [m]
        first = self.order_of(self.step_index, self.lower_order_nums) == 1
        prev = self.first_order(m, sample) if first else self.second_order(self.model_outputs, sample)
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return SimpleNamespace(prev_sample=prev)


@pytest.mark.parametrize("kw", VARIANTS, ids=IDS)
def test_eager_step_follows_restatement_on_analytic_model(kw):
    import conftest
    s = _unipc(**kw)
    s.set_timesteps(20)
    x0 = torch.randn(2, 8, 7, 5, generator=torch.Generator().manual_seed(3))
    want, spread = _restatement_runs(lambda dt: UniPCRestatement(dtype=dt, **kw), x0, 20)
    xg, worst = x0.cuda(), 0.0
    for k, t in enumerate(s.timesteps):
        xg = s.step(_analytic_eps(xg, t, 0.4, 1.5, s.alphas_cumprod), t, xg).prev_sample
        worst = max(worst, _rel(xg.cpu(), want[k]))
    conftest.record(worst, "max_step_rel")
    conftest.record(spread, "restatement_fp32_fp64_spread")
    assert xg.shape == x0.shape and xg.is_cuda and torch.isfinite(xg).all() and worst <= _bound(spread), (worst, spread)
    assert s.step_index == 20


def _fused_pass(ops, s, x, st, cfg, g_scale, want=None):
    """one whole loop of the engine's launch from the latents in x; returns the worst per-step rel against `want`"""
    n = len(s.timesteps)
    B = x.shape[0]
    worst = 0.0
    for i, t in enumerate(s.timesteps):
        eps, _ = _model_eps(x, t, s.alphas_cumprod, cfg, g_scale)
        ops.unipc_step_fused(eps, x, cfg, g_scale, st.coef, st.step_idx, st.x_in, st.state, None, None, st.ts, st.t_out, st.ticket)
        if want is not None:
            worst = max(worst, _rel(x.cpu(), want[i]))
        nxt = (i + 1) % n
        assert int(st.step_idx.item()) == nxt and float(st.t_out.item()) == float(s.timesteps[nxt]) and int(st.ticket.item()) == 0
        xb = x.to(torch.bfloat16)
        assert torch.equal(st.x_in[:B], xb) and (not cfg or torch.equal(st.x_in[B:], xb))
    return worst


@pytest.mark.parametrize("kw", VARIANTS, ids=IDS)
@pytest.mark.parametrize("g_scale", [3.0, 1.0])
@pytest.mark.parametrize("n", [20, 9])
def test_fused_kernel_cfg_counter_ring_and_wrap(kw, g_scale, n):
    """The engine's launch (device coefficient table, counter + ticket, bf16 UNet input) over a whole loop: two analytic models as the
    unconditional / text halves, combined with g.  [3, 9, 8, 8] is 1728 elements: two workgroups at VEC = 4.  state starts as NaN, so a
    row that loads what its flags do not ask for poisons the result.  Then a second pass over the wrapped schedule WITHOUT resetting
    state must give the first pass's bits: row 0 reads nothing, whatever the ring holds (odd n: the last step and row 0 share a slot)."""
    import conftest
    from audioldm_with_lora_amd import ops
    s = _unipc(**kw)
    s.set_timesteps(n)
    cfg = g_scale > 1.0
    x0 = torch.randn(3, 9, 8, 8, generator=torch.Generator().manual_seed(4))
    want, spread = _restatement_runs(lambda dt: UniPCRestatement(dtype=dt, **kw), x0, n, cfg, g_scale)
    x = x0.cuda()
    st = SimpleNamespace(coef=s.coefficient_table().cuda(), ts=s.timesteps.float().cuda(),
                         step_idx=torch.zeros(1, dtype=torch.int32, device="cuda"), ticket=torch.zeros(1, dtype=torch.int32, device="cuda"),
                         t_out=torch.zeros(1, device="cuda"), state=torch.full((3,) + tuple(x.shape), float("nan"), device="cuda"),
                         x_in=torch.zeros((6 if cfg else 3,) + tuple(x.shape[1:]), dtype=torch.bfloat16, device="cuda"))
    worst = _fused_pass(ops, s, x, st, cfg, g_scale, want)
    conftest.record(worst, "max_step_rel")
    conftest.record(spread, "restatement_fp32_fp64_spread")
    assert torch.isfinite(x).all() and torch.isfinite(st.state).all() and worst <= _bound(spread), (worst, spread)
    first, first_state = x.clone(), st.state.clone()
    x.copy_(x0.cuda())
    _fused_pass(ops, s, x, st, cfg, g_scale)
    assert torch.equal(x, first) and torch.equal(st.state, first_state)


@pytest.mark.parametrize("n_vec", [1000, 4004])
def test_scalar_and_vector_paths_bitwise_equal(n_vec):
    """VEC = 4 (B * n % 4 == 0) at n_vec elements and VEC = 1 at n_vec + 3 give the same bits on the n_vec elements they share, through
    three rows: no corrector + first-order predictor, first-order corrector + second-order predictor, second-order corrector."""
    from audioldm_with_lora_amd import ops
    s = _unipc()
    s.set_timesteps(8)
    coef = s.coefficient_table().cuda()
    assert coef[:3, 10:13].tolist() == [[0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [1.0, 1.0, 1.0]]
    ts = s.timesteps.float().cuda()
    g = torch.Generator().manual_seed(6)
    x0 = torch.randn(n_vec + 3, generator=g)
    e = [torch.randn(2, n_vec + 3, generator=g) for _ in range(3)]
    res = {}
    for n in (n_vec, n_vec + 3):
        x = x0[:n].clone().view(1, n).cuda()
        state = torch.zeros(3, 1, n, device="cuda")
        x_in = torch.zeros(2, n, dtype=torch.bfloat16, device="cuda")
        step_idx = torch.zeros(1, dtype=torch.int32, device="cuda")
        ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
        t_out = torch.zeros(1, device="cuda")
        for k in range(3):
            ops.unipc_step_fused(e[k][:, :n].contiguous().cuda(), x, True, 2.5, coef, step_idx, x_in, state, None, None, ts, t_out, ticket)
        res[n] = (x[0, :n_vec].cpu(), state[:, 0, :n_vec].cpu(), x_in[:, :n_vec].cpu())
    assert n_vec % 4 == 0 and (n_vec + 3) % 4 != 0
    for a, b in zip(res[n_vec], res[n_vec + 3]):
        assert torch.equal(a, b) and torch.isfinite(a.float()).all()
    assert all(float(plane.abs().max()) > 0 for plane in res[n_vec][1])          # last and both slots were written


def test_corrector_off_is_the_dpm_launch():
    """disable_corrector on every step: ops.unipc_step_fused and ops.dpm_step_fused (DPM-Solver++ 2M midpoint, merged code) over N = 10
    from the same latents on the same analytic model.  Bound: the larger of the two restatements' own fp32 / float64 spreads."""
    import conftest
    from audioldm_with_lora_amd import ops
    n = 10
    u, d = _unipc(disable_corrector=list(range(n))), _dpm()
    u.set_timesteps(n)
    d.set_timesteps(n)
    x0 = torch.randn(3, 9, 8, 8, generator=torch.Generator().manual_seed(7))
    _, spread_u = _restatement_runs(lambda dt: UniPCRestatement(dtype=dt, disable_corrector=list(range(n))), x0, n, True, 3.0)
    _, spread_d = _restatement_runs(lambda dt: _DPMRestatement64(dtype=dt), x0, n, True, 3.0)
    spread = max(spread_u, spread_d)
    ts = u.timesteps.float().cuda()
    xu, xd = x0.cuda(), x0.cuda()
    cu, cd = u.coefficient_table().cuda(), d.coefficient_table().cuda()
    state, hist = torch.full((3,) + tuple(xu.shape), float("nan"), device="cuda"), torch.full_like(xd, float("nan"))
    iu, idd = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    tu, td = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    t_out = torch.zeros(1, device="cuda")
    worst = 0.0
    for t in u.timesteps:
        eu, _ = _model_eps(xu, t, u.alphas_cumprod, True, 3.0)
        ed, _ = _model_eps(xd, t, d.alphas_cumprod, True, 3.0)
        ops.unipc_step_fused(eu, xu, True, 3.0, cu, iu, None, state, None, None, ts, t_out, tu)
        ops.dpm_step_fused(ed, xd, True, 3.0, cd, idd, None, hist, None, None, ts, t_out, td)
        worst = max(worst, _rel(xu, xd))
    conftest.record(worst, "max_step_rel")
    conftest.record(spread, "restatement_fp32_fp64_spread")
    assert torch.isfinite(xu).all() and worst <= _bound(spread), (worst, spread_u, spread_d)
    assert torch.isnan(state[0]).sum() == 0 and int(iu.item()) == 0          # `last` is stored (x itself) though no row reads it


# ---- the masked launch ----------------------------------------------------------------------------------------------------------
from test_gpu_audio2audio import _a2a, _blend_ref, _inputs, _ops_case, _tiny  # noqa: E402


@pytest.mark.parametrize("kw", [dict(), dict(solver_type="bh1")], ids=["bh2", "bh1"])
@pytest.mark.parametrize("g_scale", [2.5, 1.0])
def test_masked_kernel_matches_restatement_and_blend(kw, g_scale):
    """Five steps of the masked launch on a begun schedule (counter, ticket, next time-embedding row) against the restatement's step()
    followed by the blend in fp32 torch; state keeps unblended values (equal to the unmasked launch's from the same inputs)."""
    import conftest
    from audioldm_with_lora_amd import ops
    s = _unipc(**kw)
    _, begin = s.get_timesteps(10, 0.5)
    coef = s.coefficient_table(begin_index=begin).cuda()
    ts = s.timesteps[begin:].float().cuda()
    blend = s.blend_table(begin).cuda()
    cfg = g_scale > 1.0
    x, x0, nz, m, e = _ops_case(3)
    B, n = x.shape[0], len(ts)
    e = e + [torch.randn(e[0].shape, generator=torch.Generator().manual_seed(30 + k)) for k in range(n - len(e))]
    table = torch.randn(n, 2 * B, 12, generator=torch.Generator().manual_seed(1)).cuda()
    runs = {}
    for dt in (torch.float32, torch.float64):
        r = UniPCRestatement(dtype=dt, **kw)
        r.set_timesteps(10)
        r.set_begin_index(begin)
        xc, out = x.to(dt), []
        for k in range(n):
            eu, et = e[k][:B].to(dt), e[k][B:].to(dt)
            xc = r.step(eu + g_scale * (et - eu) if cfg else eu, r.timesteps[begin + k], xc).prev_sample
            xc = _blend_ref(xc, x0.to(dt), nz.to(dt), m.to(dt), blend[k, 0].item(), blend[k, 1].item())
            out.append(xc)
        runs[dt] = out
    spread = max(_rel(a, b) for a, b in zip(runs[torch.float32], runs[torch.float64]))
    st = {}
    for name in ("masked", "plain"):
        st[name] = dict(x=x.clone().cuda(), state=torch.full((3,) + tuple(x.shape), float("nan"), device="cuda"),
                        x_in=torch.zeros((2 * B if cfg else B,) + x.shape[1:], dtype=torch.bfloat16, device="cuda"),
                        idx=torch.zeros(1, dtype=torch.int32, device="cuda"), ticket=torch.zeros(1, dtype=torch.int32, device="cuda"),
                        t=torch.zeros(1, device="cuda"), row=torch.zeros(2 * B, 12, device="cuda"))
    x0g, nzg, mg = x0.cuda(), nz.cuda(), m.cuda()
    worst = 0.0
    for k in range(n):
        eps = (e[k] if cfg else e[k][:B]).contiguous().cuda()
        p, q = st["masked"], st["plain"]
        ops.unipc_step_fused_masked(eps, p["x"], cfg, g_scale, coef, p["idx"], p["x_in"], p["state"], table, p["row"], ts, p["t"],
                                    p["ticket"], x0g, nzg, mg, blend)
        ops.unipc_step_fused(eps, q["x"], cfg, g_scale, coef, q["idx"], q["x_in"], q["state"], table, q["row"], ts, q["t"], q["ticket"])
        assert torch.equal(p["state"].nan_to_num(nan=7.0), q["state"].nan_to_num(nan=7.0))     # state: unblended values
        assert bool(torch.isnan(p["state"][2]).all()) == (k == 0)          # (the second slot is first written by step 1)
        worst = max(worst, _rel(p["x"].cpu(), runs[torch.float32][k]))
        q["x"].copy_(p["x"])                                 # the plain chain follows the blended trajectory
        xb = p["x"].to(torch.bfloat16)
        assert torch.equal(p["x_in"][:B], xb) and (not cfg or torch.equal(p["x_in"][B:], xb))
        nxt = (k + 1) % n
        assert int(p["idx"].item()) == nxt and int(p["ticket"].item()) == 0 and float(p["t"].item()) == float(ts[nxt])
        assert torch.equal(p["row"], table[nxt])
    conftest.record(worst, "max_step_rel")
    conftest.record(spread, "restatement_fp32_fp64_spread")
    assert worst <= _bound(spread), (worst, spread)


@pytest.mark.parametrize("g_scale", [2.5, 1.0])
def test_all_ones_mask_is_the_unmasked_kernel_and_ends_are_exact(g_scale):
    from audioldm_with_lora_amd import ops
    s = _unipc()
    _, begin = s.get_timesteps(8, 0.5)
    coef = s.coefficient_table(begin_index=begin).cuda()
    ts = s.timesteps[begin:].float().cuda()
    blend = s.blend_table(begin).cuda()
    n = len(ts)
    cfg = g_scale > 1.0
    x, x0, nz, _, e = _ops_case(9)
    B = x.shape[0]
    table = torch.randn(n, 2 * B, 12, generator=torch.Generator().manual_seed(2)).cuda()

    def run(mask):
        st = dict(x=x.clone().cuda(), state=torch.zeros((3,) + tuple(x.shape), device="cuda"),
                  x_in=torch.zeros((2 * B if cfg else B,) + x.shape[1:], dtype=torch.bfloat16, device="cuda"),
                  idx=torch.zeros(1, dtype=torch.int32, device="cuda"), ticket=torch.zeros(1, dtype=torch.int32, device="cuda"),
                  t=torch.zeros(1, device="cuda"), row=torch.zeros(2 * B, 12, device="cuda"))
        for k in range(n):
            eps = (e[k % 3] if cfg else e[k % 3][:B]).contiguous().cuda()
            a = (eps, st["x"], cfg, g_scale, coef, st["idx"], st["x_in"], st["state"], table, st["row"], ts, st["t"], st["ticket"])
            if mask is None:
                ops.unipc_step_fused(*a)
            else:
                ops.unipc_step_fused_masked(*a, x0.cuda(), nz.cuda(), mask.cuda(), blend)
        return {k: v.cpu() for k, v in st.items()}

    plain, ones, zeros = run(None), run(torch.ones(B, *x.shape[1:3])), run(torch.zeros(B, *x.shape[1:3]))
    for k in plain:
        assert torch.equal(plain[k], ones[k]), k
    assert torch.equal(zeros["x"], x0)                     # the last row (1, 0): known == x0, bitwise


def test_ops_check_the_state_operand():
    from audioldm_with_lora_amd import ops
    s = _unipc()
    s.set_timesteps(5)
    coef = s.coefficient_table().cuda()
    x = torch.zeros(2, 4, 4, 8, device="cuda")
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    for bad in (torch.zeros(2, *x.shape, device="cuda"), torch.zeros(3, *x.shape, device="cuda", dtype=torch.float64),
                torch.zeros(3, x.numel() + 4, device="cuda")):
        with pytest.raises(AssertionError):
            ops.unipc_step_fused(torch.zeros_like(x), x, False, 1.0, coef, idx, None, bad)


# ---- the engine on the tiny UNet ------------------------------------------------------------------------------------------
def _setup(steps, g_scale, use_graph, kw=None):
    from audioldm_with_lora_amd.engine import DenoiseEngine
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from oracle import configs
    from oracle.pipeline import denoise_loop
    from oracle.unet import UNet2DConditionModel as OUNet
    kw = kw or {}
    cfg = configs.tiny_unet()
    torch.manual_seed(5)
    ref = OUNet(**cfg).eval()
    mine = UNet2DConditionModel(**cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(2, 8, 31, 16, generator=g)
    pe = torch.nn.functional.normalize(torch.randn(2, 64, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(2, 64, generator=g), dim=-1)
    with torch.no_grad():
        want = denoise_loop(ref, UniPCRestatement(**kw), lat, pe, ne, steps, g_scale)
    eng = DenoiseEngine(mine, _unipc(**kw), 2, 31, 16, steps, g_scale, use_graph=use_graph)
    assert eng.unipc and not eng.dpm and not eng.euler and eng.state.shape == (3, 2, 31, 16, 8)
    eng.set_condition(pe, ne)
    eng.set_latents(lat)
    eng.capture()
    eng.run()
    return eng.latents_nchw().cpu(), want, eng, lat


@pytest.mark.parametrize("steps", [8, 9])
@pytest.mark.parametrize("g_scale", [2.5, 1.0])
def test_engine_matches_oracle_loop(steps, g_scale):
    got, want, eng, lat = _setup(steps, g_scale, True)
    rel = _rel(got, want)
    import conftest
    conftest.record(rel)
    assert torch.isfinite(got).all() and rel < 5e-2, rel
    assert eng.n_steps == steps and int(eng.step_idx.item()) == 0          # wrapped after exactly n_steps
    # a second run from the same latents reproduces the first bit for bit: no state leaks from one run into the next
    eng.set_latents(lat)
    eng.run()
    assert torch.equal(eng.latents_nchw().cpu(), got)


@pytest.mark.parametrize("steps", [8, 9])
def test_engine_graph_replay_equals_eager_bitwise(steps):
    a, _, _, _ = _setup(steps, 2.5, False)
    b, _, _, _ = _setup(steps, 2.5, True)
    assert torch.equal(a, b)


@pytest.mark.parametrize("begin", [4, 5])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_engine_begun_graph_replay_equals_eager(begin, masked):
    from audioldm_with_lora_amd.engine import DenoiseEngine
    pipe, _ = _tiny()
    g = torch.Generator().manual_seed(4)
    lat, x0 = torch.randn(2, 8, 16, 16, generator=g), torch.randn(2, 8, 16, 16, generator=g)
    m = (torch.rand(2, 16, 16, generator=g) > 0.5).float()
    pe, ne, _ = _inputs()
    out = []
    for use_graph in (False, True):
        eng = DenoiseEngine(pipe._unet, _unipc(), 2, 16, 16, 12, 2.5, use_graph=use_graph, begin_index=begin, masked=masked)
        assert eng.n_steps == 12 - begin and eng.coef.shape == (12 - begin, 16)
        eng.set_condition(pe, ne)
        eng.set_latents(lat)
        if masked:
            eng.set_inpaint(x0, lat, m)
        eng.capture()
        eng.run()
        assert int(eng.step_idx.item()) == 0 and eng.temb[0].shape[0] == 12 - begin
        out.append(eng.latents_nchw().cpu())
    assert torch.equal(out[0], out[1]) and torch.isfinite(out[0]).all()


def test_engine_chains_not_implemented():
    from audioldm_with_lora_amd.engine import DenoiseEngine
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from oracle import configs
    u = UNet2DConditionModel(**configs.tiny_unet()).cuda()
    with pytest.raises(NotImplementedError):
        DenoiseEngine(u, _unipc(), 2, 8, 16, 5, 2.5, chains=2)


# ---- the pipelines on tiny models -----------------------------------------------------------------------------------------
def test_pipeline_scheduler_swap_matches_oracle_and_rekeys_the_engine():
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, UniPCMultistepScheduler
    from oracle.pipeline import AudioLDMPipeline as OPipe
    pipe, (ou, ov, oh) = _tiny()
    g = torch.Generator().manual_seed(19)
    pe = torch.nn.functional.normalize(torch.randn(2, 64, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(2, 64, generator=g), dim=-1)
    lat = torch.randn(2, 8, 16, 16, generator=g)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio_length_in_s=0.64, num_inference_steps=8, guidance_scale=2.5)
    ddim = pipe.scheduler
    a = pipe(latents=lat.clone(), **call).audios
    pipe.scheduler = UniPCMultistepScheduler.from_config(pipe.scheduler.config)
    b = pipe(latents=lat.clone(), generator=torch.Generator().manual_seed(1), **call).audios    # (_seed_engine: a no-op here)
    pipe.scheduler = DDIMScheduler.from_config(pipe.scheduler.config)       # a NEW DDIM object with the same configuration
    c = pipe(latents=lat.clone(), **call).audios
    assert np.array_equal(a, c) and not np.allclose(a, b)
    assert any(e.scheduler is pipe.scheduler for e in pipe._engines.values())
    assert not any(e.scheduler is ddim for e in pipe._engines.values())            # the first DDIM object's engine was dropped
    assert any(e.unipc for e in pipe._engines.values())
    want = OPipe(ou, ov, oh, UniPCRestatement())(pe, ne, audio_length_in_s=0.64, num_inference_steps=8, guidance_scale=2.5,
                                                 latents=lat.clone()).audios
    got = torch.from_numpy(b)
    rel = _rel(got, torch.from_numpy(want))
    import conftest
    conftest.record(rel)
    assert got.shape == (2, 10240) and torch.isfinite(got).all() and rel < 8e-2, rel


def _restate(models, audio, pe, ne, strength, mask_mel, N, g_scale, seed):
    """CPU restatement, built as test_gpu_audio2audio._restate is for DPM: oracle log-mel -> oracle VAE encode + the same posterior
    noise -> add_noise at begin -> UniPCRestatement over the suffix with the legacy inpaint blend -> oracle decode + vocoder."""
    from oracle.mel import DSP, log_mel_spec
    from oracle.pipeline import cfg_combine
    ou, ov, oh = models
    B = pe.shape[0]
    mel = log_mel_spec(audio, dict(DSP, target_length=128))
    gen = torch.Generator().manual_seed(seed)
    dist = ov.encode(mel).latent_dist
    post = torch.randn(dist.mean.shape, generator=gen)
    x0 = (dist.mean + dist.std * post) * ov.config.scaling_factor
    eps = torch.randn(x0.shape, generator=gen)
    begin = max(N - min(int(N * strength), N), 0)
    s = UniPCRestatement()
    s.set_timesteps(N)
    s.set_begin_index(begin)

    def noise_to(i):
        a, sg = s._sigma_to_alpha_sigma_t(s.sigmas[i])
        return a * x0 + sg * eps
    m = None
    if mask_mel is not None:
        m = torch.nn.functional.max_pool2d(mask_mel.expand(B, -1, -1)[:, None].float(), 4)
    x = noise_to(begin)
    emb = torch.cat([ne, pe])
    ts = s.timesteps[begin:]
    for k, t in enumerate(ts):
        e = ou(torch.cat([x, x]), t, encoder_hidden_states=None, class_labels=emb)[0]
        x = s.step(cfg_combine(e, g_scale), t, x).prev_sample
        if m is not None:
            known = noise_to(begin + k + 1) if k + 1 < len(ts) else x0
            x = (1 - m) * known + m * x
    wav = oh(ov.decode(x / ov.config.scaling_factor).sample.squeeze(1)).float()[:, :20480]
    return x, wav, x0, m


@pytest.mark.parametrize("masked", [False, True], ids=["style", "inpaint"])
def test_audio_to_audio_parity_with_cpu_restatement(masked):
    from audioldm_with_lora_amd.audio2audio import regeneration_mask
    from audioldm_with_lora_amd.scheduler import UniPCMultistepScheduler
    pipe, models = _tiny()
    pipe.scheduler = UniPCMultistepScheduler.from_config(pipe.scheduler.config)
    a2a = _a2a(pipe)
    pe, ne, audio = _inputs()
    mask = regeneration_mask(128, 64, seconds=(0.4, 0.8)) if masked else None
    N = 9
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, strength=0.5, mask=mask, num_inference_steps=N, guidance_scale=2.5)
    lat = a2a(generator=torch.Generator().manual_seed(8), output_type="latent", **call).audios.cpu()
    wav = torch.from_numpy(a2a(generator=torch.Generator().manual_seed(8), **call).audios)
    with torch.no_grad():
        x_ref, wav_ref, x0_ref, m = _restate(models, audio, pe, ne, 0.5, mask, N, 2.5, 8)
    r_lat, r_wav = _rel(lat, x_ref), _rel(wav, wav_ref)
    import conftest
    conftest.record(r_lat, "latents_rel")
    conftest.record(r_wav, "audio_rel")
    assert wav.shape == (2, 20480) and torch.isfinite(wav).all()
    assert r_lat < 8e-2 and r_wav < 8e-2, (r_lat, r_wav)
    if masked:
        keep = (m == 0).expand_as(lat)
        assert keep.any() and (~keep).any()
        r_keep = _rel(lat[keep], x_ref[keep])
        conftest.record(r_keep, "kept_rel")
        assert r_keep < 4e-2, r_keep


# ---- full width ---------------------------------------------------------------------------------------------------------------
def test_full_width_unet_three_unipc_steps_finite():
    """configs.UNET at the config-2 shape: batch 4 x 10 s (latents [4, 8, 250, 16]) with CFG, random weights, 3 UniPC steps."""
    from audioldm_with_lora_amd.engine import DenoiseEngine
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    torch.manual_seed(1234)
    unet = UNet2DConditionModel().cuda()
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(4, 8, 250, 16, generator=g)
    pe = torch.nn.functional.normalize(torch.randn(4, 512, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(4, 512, generator=g), dim=-1)
    eng = DenoiseEngine(unet, _unipc(), 4, 250, 16, 3, 2.5)
    eng.set_condition(pe, ne)
    eng.set_latents(lat)
    eng.capture()
    out = eng.run()
    torch.cuda.synchronize()
    assert out.shape == (4, 250, 16, 8) and torch.isfinite(out).all() and int(eng.step_idx.item()) == 0
    assert torch.isfinite(eng.state).all() and not torch.equal(eng.latents_nchw().cpu(), lat)


# ---- the script -----------------------------------------------------------------------------------------------------------------
def test_inference_script_unipc(tmp_path):
    from scipy.io import wavfile
    import synth_checkpoint
    from audioldm_with_lora_amd.script import inference
    root = str(tmp_path / "m")
    synth_checkpoint.write_model_dir(root)
    wavs = []
    for i, extra in enumerate((["--scheduler", "unipc"], ["--scheduler", "unipc", "--solver-order", "1"], [])):
        out = str(tmp_path / f"out_{i}.wav")
        inference.main(["--model-dir", root, "--no-lora", "--steps", "5", "--audio-length", "1.28", "--guidance-scale", "2.5",
                        "--output", out, "--seed", "1"] + extra)
        sr, wav = wavfile.read(out)
        assert sr == 16000 and wav.shape == (20480,) and wav.dtype == np.float32 and np.isfinite(wav).all()
        wavs.append(wav)
    assert not np.array_equal(wavs[0], wavs[1]) and not np.array_equal(wavs[0], wavs[2])
