"""GPU: the kernels of windowed denoising (csrc/elementwise.hip: aldm_window_gather, aldm_window_blend and the four
aldm_*_step_fused_windowed) -- a plan of one window against the plain launches bit for bit, the windowed step against the
restatement (tests/longform_restatement.py: blend the windows' eps, then the existing restatement's step), the next UNet input in
every window, gather and blend on their own, and what the launchers reject.

The bound of the comparisons with the restatement is measured as in tests/test_gpu_unipc.py: the restatement runs twice on the same
inputs, in fp32 and in float64, the worst per-step relative L2 between the two is the rounding noise of the fp32 statement itself,
and the kernel -- which associates the same sums differently -- may sit up to 4 x that noise from the fp32 run (never closer than
1e-6, a few fp32 ulps of a relative L2)."""
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

SOLVERS = ["ddim", "dpm", "unipc", "euler_a"]
# latents [B, rows, W, C], window rows, overlap rows, looped: the smallest shapes at which the frame can go wrong
SHAPES = {
    "vec4_two_workgroups_shifted_last": ((2, 44, 3, 4), 16, 4, False),     # 1056 elements: VEC = 4, 264 threads; offsets 0, 12, 24, 28
    "vec1_odd_total": ((1, 11, 5, 3), 5, 2, False),                        # 165 elements, C = 3: VEC = 1
    "cover_3": ((2, 21, 3, 4), 8, 2, False),                               # offsets 0, 6, 12, 13: row 13 lies under three windows
    "looped_wrap": ((2, 18, 3, 4), 8, 2, True),                            # offsets 0, 6, 12: the last window wraps over the seam
}
N_STEPS = 4
ROW = 8                                                                    # floats per row of the time-embedding table


def _scheduler(solver):
    from audioldm_with_lora_amd.scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,
                                                  UniPCMultistepScheduler)
    if solver == "ddim":
        return DDIMScheduler()
    cls = {"dpm": DPMSolverMultistepScheduler, "unipc": UniPCMultistepScheduler, "euler_a": EulerAncestralDiscreteScheduler}[solver]
    return cls.from_config(DDIMScheduler().config)


def _plan(name):
    from audioldm_with_lora_amd.longform import WindowPlan
    dims, hw, ov, loop = SHAPES[name]
    return WindowPlan(dims[1], hw, ov, loop), dims


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _bound(spread):
    return max(4.0 * spread, 1e-6)


def _state(ops, solver, dims, n_win, cfg, x_start):
    """the buffers of one run: long x and solver state, per-window x_in (NaN: every element must be written)"""
    halves = 2 if cfg else 1
    st = dict(x=x_start.clone().cuda(),
              x_in=torch.full((halves * n_win[0],) + n_win[1:], float("nan"), dtype=torch.bfloat16, device="cuda"),
              idx=torch.zeros(1, dtype=torch.int32, device="cuda"), t=torch.zeros(1, device="cuda"), rowbias=torch.zeros(ROW, device="cuda"))
    if solver == "dpm":
        st["op"] = torch.zeros(dims, device="cuda")
    if solver == "unipc":
        st["op"] = torch.zeros((3,) + tuple(dims), device="cuda")
    if solver == "euler_a":
        st["op"] = ops.philox_state(2025, 0xFFFFFFFE)                       # the ordinal's low word carries within the run
    return st


# ---- 1. one window is the plain launch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(2, 44, 3, 4), (1, 11, 5, 3)], ids=["vec4", "vec1"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_single_window_equals_the_plain_launch_bitwise(solver, dims):
    """rows == hw, K = 1, weight 1.0, under CFG, over 2 n_steps + 1 launches (the counter wraps twice): x, x_in (both halves), rowbias,
    the counter, t_out, hist / state / the Philox state bit for bit after every launch; the ticket rests at 0."""
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.longform import WindowPlan
    plan = WindowPlan(dims[1], dims[1], 0)
    assert plan.K == plan.KC == 1 and float(plan.weight.min()) == 1.0
    win = plan.device("cuda")
    s = _scheduler(solver)
    s.set_timesteps(N_STEPS)
    coef, ts = s.coefficient_table().cuda(), s.timesteps.float().cuda()
    g = torch.Generator().manual_seed(7)
    table = torch.randn(N_STEPS, ROW, generator=g).cuda()
    x_start = torch.randn(dims, generator=g)
    got, want = (_state(ops, solver, dims, tuple(dims), True, x_start) for _ in range(2))
    tickets = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]
    for k in range(2 * N_STEPS + 1):
        eps = torch.randn((2 * dims[0],) + tuple(dims[1:]), generator=g).cuda()
        for st, ticket, suffix, tail in ((got, tickets[0], "_windowed", (win,)), (want, tickets[1], "", ())):
            operand = (st["op"],) if "op" in st else ()
            getattr(ops, f"{solver}_step_fused{suffix}")(eps, st["x"], True, 2.5, coef, st["idx"], st["x_in"], *operand, table, st["rowbias"], ts,
                                                         st["t"], ticket, *tail)
        for name in got:
            assert torch.equal(_bits(got[name]), _bits(want[name])), (k, name)
        assert int(got["idx"]) == (k + 1) % N_STEPS and int(tickets[0]) == 0 and int(tickets[1]) == 0, k


# ---- 2. and 3. the windowed step against the restatement; the next UNet input -----------------------------------------------------
def _windowed_run(ops, solver, shape, cfg, g_scale=2.5, check_x_in=False):
    """N_STEPS launches of the windowed step from random latents with random eps per window; the restatement in fp32 and float64 on
    the same numbers (Euler-ancestral: fed the device's own noise).  Returns (worst per-step rel of the kernel against the fp32
    restatement, the fp32 / float64 spread)."""
    plan, dims = _plan(shape)
    win = plan.device("cuda")
    tables = R.tables_of(dims[1], SHAPES[shape][1], SHAPES[shape][2], SHAPES[shape][3])
    n_win = (dims[0] * plan.K, plan.window_rows) + tuple(dims[2:])
    halves = 2 if cfg else 1
    s = _scheduler(solver)
    s.set_timesteps(N_STEPS)
    coef, ts = s.coefficient_table().cuda(), s.timesteps.float().cuda()
    g = torch.Generator().manual_seed(11)
    table = torch.randn(N_STEPS, ROW, generator=g).cuda()
    x0 = torch.randn(dims, generator=g) * float(s.init_noise_sigma)
    eps = [torch.randn((halves * n_win[0],) + n_win[1:], generator=g) for _ in range(N_STEPS)]
    st = _state(ops, solver, dims, n_win, cfg, x0)
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    operand = (st["op"],) if "op" in st else ()
    got, zs = [], []
    for i in range(N_STEPS):
        if solver == "euler_a":
            zs.append(ops.randn(tuple(dims), st["op"], advance=False).cpu())
        getattr(ops, f"{solver}_step_fused_windowed")(eps[i].cuda(), st["x"], cfg, g_scale, coef, st["idx"], st["x_in"], *operand, table,
                                                      st["rowbias"], ts, st["t"], ticket, win)
        got.append(st["x"].cpu())
        nxt = (i + 1) % N_STEPS
        assert int(st["idx"]) == nxt and float(st["t"]) == float(s.timesteps[nxt]) and int(ticket) == 0
        assert torch.equal(st["rowbias"], table[nxt])
        if check_x_in:
            # every window holds the bf16 of its rows of the new long latent (Euler-ancestral: times the next row's input scale)
            scale = coef[i, 2] if solver == "euler_a" else None
            xs = st["x"] * scale if scale is not None else st["x"]
            want = R.gather(xs.cpu(), tables[0], tables[1]).to(torch.bfloat16)
            for h in range(halves):
                assert torch.equal(_bits(st["x_in"][h * n_win[0]:(h + 1) * n_win[0]].cpu()), _bits(want)), (i, h)
            assert torch.equal(_bits(ops.window_gather(st["x"], win, float(scale) if scale is not None else 1.0)), _bits(st["x_in"][:n_win[0]]))
    runs = {}
    for dt in (torch.float32, torch.float64):
        r = R.set_timesteps_typed(R.make_restatement(solver, dt), N_STEPS, dt)
        x, out = x0.to(dt), []
        for i, t in enumerate(r.timesteps):
            e = eps[i].to(dt)
            eu, et = e.chunk(2) if cfg else (e, None)
            kw = dict(noise=zs[i]) if solver == "euler_a" else {}
            x = R.windowed_step(r, t, x, eu, et, g_scale, tables, dim=1, **kw)
            out.append(x)
        runs[dt] = out
    spread = max(_rel(a, b) for a, b in zip(runs[torch.float32], runs[torch.float64]))
    worst = max(_rel(a, b) for a, b in zip(got, runs[torch.float32]))
    return worst, spread, got[-1]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_windowed_step_follows_the_restatement(solver, cfg, shape):
    import conftest
    from audioldm_with_lora_amd import ops
    worst, spread, last = _windowed_run(ops, solver, shape, cfg, 2.5 if cfg else 1.0)
    conftest.record(worst, "max_step_rel")
    conftest.record(spread, "restatement_fp32_fp64_spread")
    print(f"{solver} {shape} cfg={cfg}: max_step_rel {worst:.3e}, spread {spread:.3e}, bound {_bound(spread):.3e}")
    assert torch.isfinite(last).all() and worst <= _bound(spread), (worst, spread)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("solver", SOLVERS)
def test_next_unet_input_lands_in_every_covering_window(solver, shape):
    from audioldm_with_lora_amd import ops
    _windowed_run(ops, solver, shape, True, check_x_in=True)
    _windowed_run(ops, solver, shape, False, 1.0, check_x_in=True)


# ---- 4. gather and blend ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_window_gather_and_blend(shape):
    import conftest
    from audioldm_with_lora_amd import ops
    plan, dims = _plan(shape)
    win = plan.device("cuda")
    offs, hw, cover, weight = R.tables_of(dims[1], *SHAPES[shape][1:])
    g = torch.Generator().manual_seed(13)
    x = torch.randn(dims, generator=g)
    # gather: indexing, bit for bit -- fp32, bf16 and bf16 with a scale
    want = R.gather(x, offs, hw)
    got32 = ops.window_gather(x.cuda(), win, out_f32=True)
    assert got32.shape == want.shape == (dims[0] * plan.K, hw) + tuple(dims[2:]) and torch.equal(got32.cpu(), want)
    assert torch.equal(_bits(ops.window_gather(x.cuda(), win).cpu()), _bits(want.to(torch.bfloat16)))
    assert torch.equal(_bits(ops.window_gather(x.cuda(), win, 0.37).cpu()), _bits((want * torch.tensor(0.37)).to(torch.bfloat16)))
    assert torch.equal(_bits(ops.window_gather(x.cuda(), win, 0.37)), _bits(ops.f32_to_bf16(got32, 0.37)))
    # blend of independent windows against the restatement in float64; the restatement's own fp32 run gives the bound
    w = torch.randn(want.shape, generator=g)
    b32, b64 = R.blend(w, offs, hw, dims[1], cover, weight), R.blend(w.double(), offs, hw, dims[1], cover, weight)
    spread = _rel(b32, b64)
    got = ops.window_blend(w.cuda(), win).cpu()
    rel = _rel(got, b64)
    conftest.record(rel, "blend_rel")
    conftest.record(spread, "restatement_fp32_fp64_spread")
    assert got.shape == tuple(dims) and rel <= _bound(spread), (rel, spread)
    # windows cut out of one tensor blend back into it (the weights of a row sum to 1)
    back = ops.window_blend(got32, win).cpu()
    rel = _rel(back, x)
    conftest.record(rel, "blend_of_gather_rel")
    assert rel <= _bound(spread), (rel, spread)


# ---- 5. what the launchers reject -----------------------------------------------------------------------------------------------
def test_launchers_reject_bad_plans_and_launch_nothing():
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd._lib import AldmError
    plan, dims = _plan("cover_3")
    win = plan.device("cuda")
    n_win = (dims[0] * plan.K, plan.window_rows) + tuple(dims[2:])
    s = _scheduler("ddim")
    s.set_timesteps(N_STEPS)
    coef, ts = s.coefficient_table().cuda(), s.timesteps.float().cuda()
    x = torch.randn(dims, generator=torch.Generator().manual_seed(1)).cuda()
    x_before = x.clone()
    eps = torch.ones((2 * n_win[0],) + n_win[1:], device="cuda")
    x_in = torch.zeros(eps.shape, dtype=torch.bfloat16, device="cuda")
    idx, t, ticket = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    table, rowbias = torch.ones(N_STEPS, ROW, device="cuda"), torch.zeros(ROW, device="cuda")

    def bad(**over):
        d = dict(vars(win))
        d.update(over)
        return SimpleNamespace(**d)

    wide = bad(KC=5, cover=torch.full((dims[1], 5), -1, dtype=torch.int32, device="cuda"), weight=torch.zeros(dims[1], 5, device="cuda"))
    plans = {"KC > 4": (wide, "at most 4"), "cover rows": (bad(cover=win.cover[:-1].contiguous()), "rows * KC"),
             "weight rows": (bad(weight=win.weight[:-1].contiguous()), "rows * KC"), "offset count": (bad(offset=win.offset[:-1].contiguous()), "K ="),
             "rows": (bad(rows=dims[1] - 1), ""), "hw > rows": (bad(hw=dims[1] + 1), "")}
    for what, (p, msg) in plans.items():
        with pytest.raises((AldmError, AssertionError), match=re.escape(msg)):
            ops.ddim_step_fused_windowed(eps, x, True, 2.5, coef, idx, x_in, table, rowbias, ts, t, ticket, p)
        if what in ("KC > 4", "cover rows", "weight rows"):
            with pytest.raises((AldmError, AssertionError), match=re.escape(msg)):
                ops.window_blend(eps[:n_win[0]].contiguous(), p)
    with pytest.raises(AldmError, match="rc=-3"):                        # ALDM_E_UNSUPPORTED, from the launcher itself
        ops.ddim_step_fused_windowed(eps, x, True, 2.5, coef, idx, x_in, table, rowbias, ts, t, ticket, wide)
    with pytest.raises(AldmError, match="rc=-1"):                        # ALDM_E_ARG
        ops.ddim_step_fused_windowed(eps, x, True, 2.5, coef, idx, x_in, table, rowbias, ts, t, ticket, plans["cover rows"][0])
    with pytest.raises(AldmError, match="rc=-1"):
        ops.window_gather(x, plans["offset count"][0])
    torch.cuda.synchronize()
    assert torch.equal(x, x_before) and int(idx) == 0 and int(ticket) == 0 and not x_in.any() and not rowbias.any()
    # the plan itself still launches
    ops.ddim_step_fused_windowed(eps, x, True, 2.5, coef, idx, x_in, table, rowbias, ts, t, ticket, win)
    assert int(idx) == 1 and not torch.equal(x, x_before)
