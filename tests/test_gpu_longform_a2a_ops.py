"""GPU: the four masked windowed fused steps (csrc/elementwise.hip: aldm_{ddim,dpm,euler_a,unipc}_step_fused_windowed_masked) -- against
the restatement (tests/longform_a2a_restatement.py: the windowed step, then the legacy inpaint blend), the bitwise identities with
the launches they join (an all-ones mask is the unmasked windowed launch, a plan of one window is the plain masked launch, the
VEC 1 and VEC 4 paths agree), the exact ends of the blend, and what the launcher rejects.

Shapes and the bound are those of tests/test_gpu_longform_ops.py: the restatement runs in fp32 and in float64 on the same numbers,
the worst per-step relative L2 between the two is the rounding noise of the fp32 statement, and the kernel may sit up to 4 x that
noise from the fp32 run (never closer than 1e-6)."""
import ctypes as C
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_a2a_restatement as A  # noqa: E402
import longform_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

SOLVERS = ["ddim", "dpm", "unipc", "euler_a"]
# latents [B, rows, W, C], window rows, overlap rows, looped (tests/test_gpu_longform_ops.py)
SHAPES = {
    "vec4_two_workgroups_shifted_last": ((2, 44, 3, 4), 16, 4, False),
    "vec1_odd_total": ((1, 11, 5, 3), 5, 2, False),
    "cover_3": ((2, 21, 3, 4), 8, 2, False),
    "looped_wrap": ((2, 18, 3, 4), 8, 2, True),
}
N_STEPS = 4
ROW = 8


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


def _mask(dims, g):
    """one value per pixel out of {0, 0.25, 1}"""
    return torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, tuple(dims[:3]), generator=g)]


def _state(ops, solver, dims, n_win, cfg, x_start):
    """the buffers of one run: long x and solver state, per-window x_in (NaN: every element must be written), counter, ticket"""
    halves = 2 if cfg else 1
    st = dict(x=x_start.clone().cuda(),
              x_in=torch.full((halves * n_win[0],) + tuple(n_win[1:]), float("nan"), dtype=torch.bfloat16, device="cuda"),
              idx=torch.zeros(1, dtype=torch.int32, device="cuda"), t=torch.zeros(1, device="cuda"), rowbias=torch.zeros(ROW, device="cuda"),
              ticket=torch.zeros(1, dtype=torch.int32, device="cuda"))
    if solver == "dpm":
        st["op"] = torch.zeros(tuple(dims), device="cuda")
    if solver == "unipc":
        st["op"] = torch.zeros((3,) + tuple(dims), device="cuda")
    if solver == "euler_a":
        st["op"] = ops.philox_state(2025, 0xFFFFFFFE)                       # the ordinal's low word carries within the run
    return st


def _launch(ops, name, eps, st, cfg, g_scale, coef, table, ts, *tail):
    operand = (st["op"],) if "op" in st else ()
    getattr(ops, name)(eps, st["x"], cfg, g_scale, coef, st["idx"], st["x_in"], *operand, table, st["rowbias"], ts, st["t"], st["ticket"], *tail)


def _schedule(solver):
    s = _scheduler(solver)
    s.set_timesteps(N_STEPS)
    return s, s.coefficient_table().cuda(), s.timesteps.float().cuda(), s.blend_table(0).cuda()


def _same(got, want, where):
    for name in got:
        assert torch.equal(_bits(got[name]), _bits(want[name])), (where, name)


# ---- 1. against the restatement; the exact ends -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_masked_windowed_step_follows_the_restatement(solver, cfg, shape):
    """4 steps from random latents with random eps per window and a mask out of {0, 0.25, 1} per pixel.  Euler-ancestral: the
    restatement is fed the device's own draw.  After the last step the rows the mask keeps hold x0 exactly, and every window holds
    the bf16 of the BLENDED long latent."""
    import conftest
    from audioldm_with_lora_amd import ops
    g_scale = 2.5 if cfg else 1.0
    plan, dims = _plan(shape)
    win = plan.device("cuda")
    tables = R.tables_of(dims[1], *SHAPES[shape][1:])
    n_win = (dims[0] * plan.K, plan.window_rows) + tuple(dims[2:])
    halves = 2 if cfg else 1
    s, coef, ts, blend = _schedule(solver)
    g = torch.Generator().manual_seed(11)
    table = torch.randn(N_STEPS, ROW, generator=g).cuda()
    x_start = torch.randn(dims, generator=g) * float(s.init_noise_sigma)
    x0, nz, m = torch.randn(dims, generator=g), torch.randn(dims, generator=g), _mask(dims, g)
    assert {0.0, 0.25, 1.0} == set(m.unique().tolist())
    eps = [torch.randn((halves * n_win[0],) + n_win[1:], generator=g) for _ in range(N_STEPS)]
    st = _state(ops, solver, dims, n_win, cfg, x_start)
    inpaint = (x0.cuda(), nz.cuda(), m.cuda(), blend)
    got, zs = [], []
    for i in range(N_STEPS):
        if solver == "euler_a":
            zs.append(ops.randn(tuple(dims), st["op"], advance=False).cpu())
        st["x_in"].fill_(float("nan"))
        _launch(ops, f"{solver}_step_fused_windowed_masked", eps[i].cuda(), st, cfg, g_scale, coef, table, ts, win, *inpaint)
        got.append(st["x"].cpu())
        nxt = (i + 1) % N_STEPS
        assert int(st["idx"]) == nxt and float(st["t"]) == float(s.timesteps[nxt]) and int(st["ticket"]) == 0
        assert torch.equal(st["rowbias"], table[nxt])
        scale = float(coef[i, 2]) if solver == "euler_a" else 1.0
        want_in = ops.window_gather(st["x"], win, scale)
        for h in range(halves):
            assert torch.equal(_bits(st["x_in"][h * n_win[0]:(h + 1) * n_win[0]]), _bits(want_in)), (i, h)
    keep = (m == 0)[..., None].expand(dims)
    assert keep.any() and torch.equal(got[-1][keep], x0[keep])                # the last row (1, 0): known == x0, bitwise
    runs = {}
    for dt in (torch.float32, torch.float64):
        r = R.set_timesteps_typed(R.make_restatement(solver, dt), N_STEPS, dt)
        x, out = x_start.to(dt), []
        for i in range(N_STEPS):
            e = eps[i].to(dt)
            eu, et = e.chunk(2) if cfg else (e, None)
            kw = dict(noise=zs[i]) if solver == "euler_a" else {}
            x = A.masked_windowed_step(r, solver, i, N_STEPS, x, eu, et, g_scale, tables, x0.to(dt), nz.to(dt), m, dim=1, **kw)
            out.append(x)
        runs[dt] = out
    spread = max(_rel(a, b) for a, b in zip(runs[torch.float32], runs[torch.float64]))
    worst = max(_rel(a, b) for a, b in zip(got, runs[torch.float32]))
    conftest.record(worst, "max_step_rel")
    conftest.record(spread, "restatement_fp32_fp64_spread")
    print(f"{solver} {shape} cfg={cfg}: max_step_rel {worst:.3e}, spread {spread:.3e}, bound {_bound(spread):.3e}")
    assert torch.isfinite(got[-1]).all() and worst <= _bound(spread), (worst, spread)


# ---- 2. the bitwise identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("solver", SOLVERS)
def test_all_ones_mask_is_the_unmasked_windowed_launch_bitwise(solver, shape):
    from audioldm_with_lora_amd import ops
    plan, dims = _plan(shape)
    win = plan.device("cuda")
    n_win = (dims[0] * plan.K, plan.window_rows) + tuple(dims[2:])
    s, coef, ts, blend = _schedule(solver)
    g = torch.Generator().manual_seed(5)
    table = torch.randn(N_STEPS, ROW, generator=g).cuda()
    x_start = torch.randn(dims, generator=g) * float(s.init_noise_sigma)
    inpaint = (torch.randn(dims, generator=g).cuda(), torch.randn(dims, generator=g).cuda(), torch.ones(dims[:3], device="cuda"), blend)
    got, want = (_state(ops, solver, dims, n_win, True, x_start) for _ in range(2))
    for k in range(N_STEPS + 1):
        eps = torch.randn((2 * n_win[0],) + n_win[1:], generator=g).cuda()
        for st in (got, want):
            st["x_in"].fill_(float("nan"))
        _launch(ops, f"{solver}_step_fused_windowed_masked", eps, got, True, 2.5, coef, table, ts, win, *inpaint)
        _launch(ops, f"{solver}_step_fused_windowed", eps, want, True, 2.5, coef, table, ts, win)
        _same(got, want, k)
        assert not torch.isnan(got["x_in"].float()).any() and int(got["idx"]) == (k + 1) % N_STEPS and int(got["ticket"]) == 0


@pytest.mark.parametrize("dims", [(2, 44, 3, 4), (1, 11, 5, 3)], ids=["vec4", "vec1"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_single_window_equals_the_plain_masked_launch_bitwise(solver, dims):
    """rows == hw, K = 1, weight 1.0, under CFG, over 2 n_steps + 1 launches (the counter wraps twice)"""
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.longform import WindowPlan
    plan = WindowPlan(dims[1], dims[1], 0)
    assert plan.K == plan.KC == 1 and float(plan.weight.min()) == 1.0
    win = plan.device("cuda")
    s, coef, ts, blend = _schedule(solver)
    g = torch.Generator().manual_seed(7)
    table = torch.randn(N_STEPS, ROW, generator=g).cuda()
    x_start = torch.randn(dims, generator=g)
    inpaint = (torch.randn(dims, generator=g).cuda(), torch.randn(dims, generator=g).cuda(), _mask(dims, g).cuda(), blend)
    got, want = (_state(ops, solver, dims, tuple(dims), True, x_start) for _ in range(2))
    for k in range(2 * N_STEPS + 1):
        eps = torch.randn((2 * dims[0],) + tuple(dims[1:]), generator=g).cuda()
        for st in (got, want):
            st["x_in"].fill_(float("nan"))
        _launch(ops, f"{solver}_step_fused_windowed_masked", eps, got, True, 2.5, coef, table, ts, win, *inpaint)
        _launch(ops, f"{solver}_step_fused_masked", eps, want, True, 2.5, coef, table, ts, *inpaint)
        _same(got, want, k)
        assert int(got["idx"]) == (k + 1) % N_STEPS and int(got["ticket"]) == 0 and int(want["ticket"]) == 0, k


@pytest.mark.parametrize("solver", ["ddim", "dpm", "unipc"])
def test_scalar_and_vector_paths_bitwise_equal(solver):
    """The same numbers in rows of 4 floats (VEC = 4) and in the first 4 of rows of 5 (VEC = 1), C = 1 so that the mask covers both,
    three windows with a shifted last one: x, the solver's state and every window's x_in agree on the shared columns after every
    launch.  (Euler-ancestral draws element i of the LONG latent from its stream, and the two widths number the elements differently;
    its two paths meet the plain launches' in test_single_window_equals_the_plain_masked_launch_bitwise.)"""
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.longform import WindowPlan
    B, rows, hw, ov = 2, 21, 8, 2
    plan = WindowPlan(rows, hw, ov)
    win = plan.device("cuda")
    s, coef, ts, blend = _schedule(solver)
    g = torch.Generator().manual_seed(6)
    table = torch.randn(N_STEPS, ROW, generator=g).cuda()
    full = lambda *lead: torch.randn(*lead, 5, 1, generator=g)
    x_start, x0, nz = full(B, rows), full(B, rows), full(B, rows)
    m = _mask((B, rows, 5), g)
    eps = [full(2 * B * plan.K, hw) for _ in range(N_STEPS)]
    res = {}
    for w in (4, 5):
        cut = lambda t: t[..., :w, :].contiguous()
        st = _state(ops, solver, (B, rows, w, 1), (B * plan.K, hw, w, 1), True, cut(x_start))
        inpaint = (cut(x0).cuda(), cut(nz).cuda(), m[..., :w].contiguous().cuda(), blend)
        out = []
        for k in range(N_STEPS):
            st["x_in"].fill_(float("nan"))
            _launch(ops, f"{solver}_step_fused_windowed_masked", cut(eps[k]).cuda(), st, True, 2.5, coef, table, ts, win, *inpaint)
            out.append({n: (v[..., :4, :] if n in ("x", "x_in", "op") else v).clone() for n, v in st.items()})
        res[w] = out
    for k, (a, b) in enumerate(zip(res[4], res[5])):
        _same(a, b, k)


# ---- 3. what the launcher rejects -------------------------------------------------------------------------------------------------
def test_launcher_rejects_and_launches_nothing():
    from audioldm_with_lora_amd import _lib, ops
    from audioldm_with_lora_amd._lib import AldmError
    plan, dims = _plan("cover_3")
    win = plan.device("cuda")
    n_win = (dims[0] * plan.K, plan.window_rows) + tuple(dims[2:])
    s, coef, ts, blend = _schedule("ddim")
    x = torch.randn(dims, generator=torch.Generator().manual_seed(1)).cuda()
    x_before = x.clone()
    eps = torch.ones((2 * n_win[0],) + n_win[1:], device="cuda")
    x_in = torch.zeros(eps.shape, dtype=torch.bfloat16, device="cuda")
    idx, t, ticket = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    table, rowbias = torch.ones(N_STEPS, ROW, device="cuda"), torch.zeros(ROW, device="cuda")
    x0, nz, m = torch.ones(dims, device="cuda"), torch.ones(dims, device="cuda"), torch.zeros(dims[:3], device="cuda")
    p = ops._p

    def raw(solver, operand, x0_, nz_, m_, blend_, channels, plan_=win):
        """the C entry point itself, past the Python wrapper's own checks"""
        args = ops._window_plan(plan_)
        fn = getattr(_lib.load(), f"aldm_{solver}_step_fused_windowed_masked")
        return fn(p(eps), p(x), dims[0], x.numel() // dims[0], 1, 2.5, p(coef), p(idx), p(x_in), *map(p, operand), p(table), ROW, p(rowbias),
                  p(ts), N_STEPS, p(t), p(ticket), C.byref(args), p(x0_), p(nz_), p(m_), p(blend_), channels, ops._stream())

    # null inpainting operands, one at a time, for every solver's entry point
    operands = {"ddim": (), "dpm": (torch.zeros_like(x),), "unipc": (torch.zeros(3, *dims, device="cuda"),), "euler_a": (ops.philox_state(1, 0),)}
    sched_coef = {k: _schedule(k)[1] for k in operands}
    for solver, operand in operands.items():
        coef = sched_coef[solver]
        for hole in range(4):
            a = [x0, nz, m, blend]
            a[hole] = None
            assert raw(solver, operand, *a, dims[3]) == -1, (solver, hole)
        assert raw(solver, operand, x0, nz, m, blend, 0) == -1                       # channels
        assert raw(solver, operand, x0, nz, m, blend, 5) == -1                       # n % C != 0  (252 floats per clip)
    coef = sched_coef["ddim"]
    assert "inpainting" in _lib.load().aldm_last_error().decode()

    def bad(**over):
        d = dict(vars(win))
        d.update(over)
        return SimpleNamespace(**d)

    wide = bad(KC=5, cover=torch.full((dims[1], 5), -1, dtype=torch.int32, device="cuda"), weight=torch.zeros(dims[1], 5, device="cuda"))
    plans = {"KC > 4": (wide, "at most 4"), "cover rows": (bad(cover=win.cover[:-1].contiguous()), "rows * KC"),
             "weight rows": (bad(weight=win.weight[:-1].contiguous()), "rows * KC"), "offset count": (bad(offset=win.offset[:-1].contiguous()), "K ="),
             "rows": (bad(rows=dims[1] - 1), ""), "hw > rows": (bad(hw=dims[1] + 1), "")}
    for what, (pl, msg) in plans.items():
        with pytest.raises((AldmError, AssertionError), match=re.escape(msg)):
            ops.ddim_step_fused_windowed_masked(eps, x, True, 2.5, coef, idx, x_in, table, rowbias, ts, t, ticket, pl, x0, nz, m, blend)
    with pytest.raises(AldmError, match="rc=-3"):                        # ALDM_E_UNSUPPORTED, from the launcher itself
        ops.ddim_step_fused_windowed_masked(eps, x, True, 2.5, coef, idx, x_in, table, rowbias, ts, t, ticket, wide, x0, nz, m, blend)
    assert raw("ddim", (), x0, nz, m, blend, dims[3], wide) == -3
    with pytest.raises(AldmError, match="rc=-1"):                        # ALDM_E_ARG
        ops.ddim_step_fused_windowed_masked(eps, x, True, 2.5, coef, idx, x_in, table, rowbias, ts, t, ticket, plans["cover rows"][0], x0,
                                            nz, m, blend)
    # the Python wrapper's own checks: mask / x0 geometry, blend rows
    for over in (dict(m=torch.zeros(dims[0], dims[1], dims[2] + 1, device="cuda")), dict(x0=torch.ones(dims[0], dims[1] + 1, *dims[2:], device="cuda")),
                 dict(blend=blend[:-1].contiguous())):
        a = dict(x0=x0, nz=nz, m=m, blend=blend)
        a.update(over)
        with pytest.raises(AssertionError):
            ops.ddim_step_fused_windowed_masked(eps, x, True, 2.5, coef, idx, x_in, table, rowbias, ts, t, ticket, win, a["x0"], a["nz"], a["m"],
                                                a["blend"])
    torch.cuda.synchronize()
    assert torch.equal(x, x_before) and int(idx) == 0 and int(ticket) == 0 and not x_in.any() and not rowbias.any()
    # the plan itself still launches; m == 0 with the first blend row: x = a x0 + s noise
    ops.ddim_step_fused_windowed_masked(eps, x, True, 2.5, coef, idx, x_in, table, rowbias, ts, t, ticket, win, x0, nz, m, blend)
    assert int(idx) == 1 and int(ticket) == 0 and torch.equal(x, torch.full_like(x, 1.0) * blend[0, 0] + blend[0, 1] * 1.0)
