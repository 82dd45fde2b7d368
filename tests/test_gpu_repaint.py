"""GPU: RePaintScheduler + aldm_repaint_step_fused[_windowed]_masked against tests/repaint_restatement.py fed with the device's own
noise -- the scalar / vector kernel paths, the noise identities of the draw contract, the reduction to the DDIM masked launch, a whole
folded loop on an analytic model, the ends of the mask, the Gaussian property through the kernel, the replayed engines on the tiny
UNet, the 10-call loop against the oracle UNet, and the audio-to-audio pipeline and script with the scheduler swapped in."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repaint_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 2025
N, JL, JS, L = 6, 2, 2, 10          # the pinned schedule of the issue: 10 UNet calls, jumps behind calls 3 and 7


def _repaint(**kw):
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, RePaintScheduler
    kw = dict(dict(jump_length=JL, jump_n_sample=JS), **kw)
    return RePaintScheduler.from_config(DDIMScheduler().config, **kw)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _record(v, what):
    import conftest
    return conftest.record(v, what)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _bufs(x_in_shape):
    return dict(x_in=torch.full(x_in_shape, float("nan"), dtype=torch.bfloat16, device="cuda"),
                idx=torch.zeros(1, dtype=torch.int32, device="cuda"), ticket=torch.zeros(1, dtype=torch.int32, device="cuda"),
                t=torch.zeros(1, device="cuda"))


def _schedule(**kw):
    s = _repaint(**kw)
    s.set_timesteps(N)
    return s, s.coefficient_table().cuda(), s.timesteps.float().cuda(), s.blend_table().cuda()


def _mask(shape, g):
    """one value per pixel out of {0, 0.25, 1}"""
    return torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, tuple(shape), generator=g)]


# ---- the op ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start_row", [0, 3])
def test_scalar_and_vector_paths_bitwise_equal(start_row):
    """n = 1000 C elements (VEC = 4) and three more pixels (VEC = 1), C = 2: the shared elements agree bit for bit after two launches
    under CFG, from a row without a jump and from row 3 (J = 2); the ordinal moves by 2 per launch"""
    from audioldm_with_lora_amd import ops
    s, coef, ts, blend = _schedule()
    assert float(coef[3, 5]) > 0 and float(coef[0, 5]) == 0
    g = torch.Generator().manual_seed(6)
    C, n_vec = 2, 2000
    n_odd = n_vec + 3 * C
    x0 = torch.randn(n_odd, generator=g)
    e = [torch.randn(2, n_odd, generator=g) for _ in range(2)]
    k0, m = torch.randn(n_odd, generator=g), _mask((n_odd // C,), g)
    res = {}
    for n in (n_vec, n_odd):
        x = x0[:n].clone().view(1, n // C, 1, C).cuda()
        b = _bufs((2, n // C, 1, C))
        b["idx"].fill_(start_row)
        st = ops.philox_state(SEED, 50)
        for k in range(2):
            ops.repaint_step_fused_masked(e[k][:, :n].contiguous().cuda(), x, True, 2.5, coef, b["idx"], b["x_in"], st, None, None, ts, b["t"],
                                          b["ticket"], k0[:n].view(1, n // C, 1, C).contiguous().cuda(), None,
                                          m[:n // C].view(1, n // C, 1).contiguous().cuda(), blend)
            assert ops.philox_state_values(st) == (SEED, 50 + 2 * (k + 1)) and int(b["idx"]) == start_row + k + 1
        res[n] = (x.view(-1)[:n_vec].cpu(), b["x_in"].view(2, -1)[:, :n_vec].cpu())
    assert n_vec % 4 == 0 and n_odd % 4 != 0
    for a, bb in zip(res[n_vec], res[n_odd]):
        assert torch.equal(_bits(a), _bits(bb)) and torch.isfinite(a.float()).all()


@pytest.mark.parametrize("n", [4096, 1001])
def test_in_kernel_noises_are_randn_of_draws_d_and_d_plus_1(n):
    """the draw contract, bitwise, on the vector and the scalar kernel: the jump's noise is draw d + 1, the known part's draw d; without
    a ticket the ordinal stays; `noise` is not read (None)"""
    from audioldm_with_lora_amd import ops
    zeros = lambda *s: torch.zeros(*s, device="cuda")
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = ops.philox_state(SEED, 6)
    want_k, want_j = ops.randn((n,), ops.philox_state(SEED, 6), advance=False), ops.randn((n,), ops.philox_state(SEED, 7), advance=False)
    # {1, 0, 1, 0, c1 = 0, c2 = 1} on zeros with mask 1: x' = zj
    x = zeros(1, n, 1)
    ops.repaint_step_fused_masked(zeros(1, n, 1), x, False, 0.0, torch.tensor([[1.0, 0, 1, 0, 0, 1, 0, 0]], device="cuda"), idx, None, st, None, None,
                                  None, None, None, zeros(1, n, 1), None, torch.ones(1, n, device="cuda"), torch.tensor([[1.0, 0.0]], device="cuda"))
    assert torch.equal(_bits(x.view(-1)), _bits(want_j)) and ops.philox_state_values(st) == (SEED, 6)
    # blend row (a, s) = (0, 1), mask 0, jump (1, 0): x' = zk, whatever x, eps and x0 hold
    x = torch.full((1, n, 1), 3.0, device="cuda")
    ops.repaint_step_fused_masked(torch.full((1, n, 1), -2.0, device="cuda"), x, False, 0.0, torch.tensor([[0.5, 0.5, 0.5, 0.5, 1, 0, 0, 0]], device="cuda"),
                                  idx, None, st, None, None, None, None, None, torch.full((1, n, 1), 7.0, device="cuda"), None, zeros(1, n),
                                  torch.tensor([[0.0, 1.0]], device="cuda"))
    assert torch.equal(_bits(x.view(-1)), _bits(want_k)) and ops.philox_state_values(st) == (SEED, 6)
    assert not torch.equal(want_k, want_j)


def test_mask_one_without_jumps_is_the_ddim_masked_launch_bitwise():
    """mask == 1 and (1, 0) jumps: x and x_in equal ops.ddim_step_fused_masked on the same inputs bit for bit, plain (VEC 4 and 1)
    and windowed with a plan of 2 overlapping windows, over n_steps + 1 launches (the counter wraps)"""
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.longform import WindowPlan
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    s, coef, ts, blend = _schedule(jump_n_sample=1)
    d = DDIMScheduler()
    d.set_timesteps(N)
    dcoef = d.coefficient_table().cuda()
    assert torch.equal(coef[:, :4], dcoef) and len(ts) == N
    g = torch.Generator().manual_seed(7)
    plan = WindowPlan(12, 8, 4)
    assert plan.K == 2 and plan.KC == 2
    cases = [((2, 11, 3, 4), None), ((1, 11, 5, 3), None), ((2, 12, 3, 4), plan), ((1, 12, 5, 3), plan)]
    for dims, pl in cases:
        n_win = dims if pl is None else (dims[0] * pl.K, pl.window_rows) + dims[2:]
        tail = () if pl is None else (pl.device("cuda"),)
        name = "_step_fused_masked" if pl is None else "_step_fused_windowed_masked"
        x_start = torch.randn(dims, generator=g)
        x0, nz = torch.randn(dims, generator=g).cuda(), torch.randn(dims, generator=g).cuda()
        ones = torch.ones(dims[:3], device="cuda")
        got, want = ({**_bufs((2 * n_win[0],) + tuple(n_win[1:])), "x": x_start.clone().cuda()} for _ in range(2))
        st = ops.philox_state(SEED, 0)
        for k in range(N + 1):
            eps = torch.randn((2 * n_win[0],) + tuple(n_win[1:]), generator=g).cuda()
            getattr(ops, "repaint" + name)(eps, got["x"], True, 2.5, coef, got["idx"], got["x_in"], st, None, None, ts, got["t"], got["ticket"], *tail,
                                           x0, None, ones, blend)
            getattr(ops, "ddim" + name)(eps, want["x"], True, 2.5, dcoef, want["idx"], want["x_in"], None, None, ts, want["t"], want["ticket"], *tail,
                                        x0, nz, ones, blend)
            for key in got:
                assert torch.equal(_bits(got[key]), _bits(want[key])), (dims, pl is not None, k, key)
            assert int(got["idx"]) == (k + 1) % N and not torch.isnan(got["x_in"].float()).any()
        assert ops.philox_state_values(st) == (SEED, 2 * (N + 1))


def _analytic_eps(x, abar, mu, sd):
    """exact eps-prediction for data ~ N(mu, sd^2) per element: x = sqrt(abar) x0 + sqrt(1 - abar) eps"""
    return (1 - abar) ** 0.5 * (x - abar ** 0.5 * mu) / (abar * sd * sd + 1 - abar)


@pytest.mark.parametrize("g_scale", [3.0, 1.0])
def test_fused_kernel_against_restatement_with_device_noise(g_scale):
    """The engine's launch over the whole folded loop (N = 6, 2, 2: 10 launches, two of them with a jump) on an analytic model (two of
    them as the CFG halves) with a mask out of {0, 0.25, 1}: per-step relative error <= 1e-5 (the Euler-ancestral op test's bound)
    against the float64 restatement fed the device's own zk, zj; counter, timestep, ticket and ordinal every step; the bf16 UNet input."""
    from audioldm_with_lora_amd import ops
    s, coef, ts, blend = _schedule()
    r = R.RePaintRestatement(JL, JS)
    r.set_timesteps(N)
    cfg = g_scale > 1.0
    g = torch.Generator().manual_seed(4)
    dims = (3, 9, 8, 8)
    xc = torch.randn(dims, generator=g, dtype=torch.float64)
    x0c, m = torch.randn(dims, generator=g, dtype=torch.float64), _mask(dims[:3], g)
    x, x0, md = xc.float().cuda(), x0c.float().cuda(), m.cuda()
    xc, x0c = x.double().cpu(), x0.double().cpu()
    b = _bufs(((2 if cfg else 1) * dims[0],) + dims[1:])
    d0 = 0xFFFFFFFA                                                  # the ordinal's low word carries within the run
    st = ops.philox_state(SEED, d0)
    worst = 0.0
    for i, (level, J) in enumerate(r.folded):
        a = r.abar(level)
        zk = ops.randn(dims, ops.philox_state(SEED, d0 + 2 * i), advance=False).double().cpu()
        zj = ops.randn(dims, ops.philox_state(SEED, d0 + 2 * i + 1), advance=False).double().cpu()
        eu, et = _analytic_eps(x, a, 0.4, 1.5), _analytic_eps(x, a, -0.3, 0.8)
        eps = torch.cat([eu, et]).contiguous() if cfg else eu.contiguous()
        ops.repaint_step_fused_masked(eps, x, cfg, g_scale, coef, b["idx"], b["x_in"], st, None, None, ts, b["t"], b["ticket"], x0, None, md, blend)
        cu, ct = _analytic_eps(xc, a, 0.4, 1.5), _analytic_eps(xc, a, -0.3, 0.8)
        xc = r.step(i, cu + g_scale * (ct - cu) if cfg else cu, xc, x0c, m.double()[..., None], zk, zj)
        worst = max(worst, _rel(x.cpu(), xc))
        nxt = (i + 1) % L
        assert int(b["idx"]) == nxt and float(b["t"]) == float(s.timesteps[nxt]) and int(b["ticket"]) == 0
        assert ops.philox_state_values(st) == (SEED, d0 + 2 * (i + 1))
        xb = x.to(torch.bfloat16)
        assert torch.equal(_bits(b["x_in"][:3]), _bits(xb)) and (not cfg or torch.equal(_bits(b["x_in"][3:]), _bits(xb)))
    keep = (m == 0)[..., None].expand(dims)
    assert torch.equal(x.cpu()[keep], x0.cpu()[keep])                 # the last row (1, 0): the kept pixels are x0, bitwise
    _record(worst, "max_step_rel")
    print(f"g = {g_scale}: max per-step rel {worst:.3e}")
    assert torch.isfinite(x).all() and worst <= 1e-5, worst


def test_ends_of_the_mask():
    """mask 0 ends on x0 bit for bit after the whole loop; on the last row a fractional mask lies between the mask-0 and the mask-1
    results element by element (to two roundings of the larger one) and is finite"""
    from audioldm_with_lora_amd import ops
    s, coef, ts, blend = _schedule()
    g = torch.Generator().manual_seed(12)
    dims = (2, 7, 5, 4)
    x0 = torch.randn(dims, generator=g).cuda()
    x = torch.randn(dims, generator=g).cuda()
    b = _bufs(dims)
    st = ops.philox_state(SEED, 0)
    for i in range(L):
        ops.repaint_step_fused_masked(torch.randn(dims, generator=g).cuda(), x, False, 0.0, coef, b["idx"], b["x_in"], st, None, None, ts, b["t"],
                                      b["ticket"], x0, None, torch.zeros(dims[:3], device="cuda"), blend)
    assert torch.equal(x, x0) and int(b["idx"]) == 0
    start, eps = torch.randn(dims, generator=g).cuda(), torch.randn(dims, generator=g).cuda()
    out = {}
    for mv in (0.0, 0.25, 1.0):
        x = start.clone()
        b["idx"].fill_(L - 1)
        ops.repaint_step_fused_masked(eps, x, False, 0.0, coef, b["idx"], b["x_in"], ops.philox_state(SEED, 9), None, None, ts, b["t"], b["ticket"],
                                      x0, None, torch.full(dims[:3], mv, device="cuda"), blend)
        out[mv] = x
    lo, hi = torch.minimum(out[0.0], out[1.0]), torch.maximum(out[0.0], out[1.0])
    tol = 2.0 ** -22 * torch.maximum(lo.abs(), hi.abs())
    assert torch.equal(out[0.0], x0) and not torch.equal(out[1.0], x0) and torch.isfinite(out[0.25]).all()
    assert bool(((out[0.25] >= lo - tol) & (out[0.25] <= hi + tol)).all())
    assert not torch.equal(out[0.25], out[0.0]) and not torch.equal(out[0.25], out[1.0])


@functools.lru_cache(maxsize=None)
def _kernel_slope(jump_n_sample):
    """tests/repaint_restatement.py gaussian_slope through the kernel: [B = 2, H = 625, W = 2, C = 16] latents are 20 000 two-pixel
    problems along W, pixel 0 kept and pixel 1 regenerated; eps is computed by torch on the device at every call"""
    from audioldm_with_lora_amd import ops
    s = _repaint(jump_length=2, jump_n_sample=jump_n_sample)
    s.set_timesteps(10)
    r = R.RePaintRestatement(2, jump_n_sample)
    r.set_timesteps(10)
    coef, ts, blend = s.coefficient_table().cuda(), s.timesteps.float().cuda(), s.blend_table().cuda()
    n_calls = len(ts)
    g = torch.Generator().manual_seed(3)
    dims = (2, 625, 2, 16)
    x0 = torch.zeros(dims)
    x0[:, :, 0] = torch.randn(2, 625, 16, generator=g)
    x0, x = x0.cuda(), torch.randn(dims, generator=g).cuda()
    mask = torch.zeros(dims[:3], device="cuda")
    mask[..., 1] = 1.0
    sigma = torch.tensor([[1.0, 0.9], [0.9, 1.0]], dtype=torch.float64)
    b = _bufs(dims)
    st = ops.philox_state(SEED + jump_n_sample, 0)
    for k, (level, _) in enumerate(r.folded):
        a = r.abar(level)
        s_inv = (np.sqrt(1 - a) * torch.linalg.inv(a * sigma + (1 - a) * torch.eye(2, dtype=torch.float64))).float().cuda()
        eps = torch.einsum("bhwc,wv->bhvc", x, s_inv).contiguous()
        ops.repaint_step_fused_masked(eps, x, False, 0.0, coef, b["idx"], b["x_in"], st, None, None, ts, b["t"], b["ticket"], x0, None, mask, blend)
    assert int(b["idx"]) == 0 and ops.philox_state_values(st) == (SEED + jump_n_sample, 2 * n_calls)
    assert torch.equal(x[:, :, 0], x0[:, :, 0]) and torch.isfinite(x).all()
    u, v = x[:, :, 0].double().flatten(), x[:, :, 1].double().flatten()
    return float((u * v).sum() / (u * u).sum()), n_calls


def test_gaussian_property_through_the_kernel():
    """the two slope intervals of tests/test_repaint_host.py, on the device: [0.38, 0.47] without resampling (10 launches), [0.64, 0.73]
    at jump_n_sample = 4 (34 launches); the true conditional slope is 0.9"""
    (plain, n1), (resampled, n4) = _kernel_slope(1), _kernel_slope(4)
    _record(plain, "slope_jump_n_sample_1")
    _record(resampled, "slope_jump_n_sample_4")
    print(f"slope {plain:.4f} over {n1} launches without jumps, {resampled:.4f} over {n4} at jump_n_sample = 4")
    assert (n1, n4) == (10, 34)
    assert 0.38 <= plain <= 0.47, plain
    assert 0.64 <= resampled <= 0.73, resampled


def test_eager_scheduler_step_and_undo_step():
    """RePaintScheduler.step is one row without a jump through the kernel, on a sample of any layout with a mask that broadcasts;
    undo_step is the closed-form jump up one level.  Both against the restatement with the device's noise, rel <= 1e-5."""
    from audioldm_with_lora_amd import ops
    s = _repaint()
    s.set_timesteps(N)
    r = R.RePaintRestatement(JL, JS)
    r.set_timesteps(N)
    g = torch.Generator().manual_seed(3)
    shape = (2, 8, 7, 5)                                             # NCHW, 560 elements
    x, e, x0 = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    m = (torch.rand(2, 1, 7, 5, generator=g) > 0.5).float()
    state = ops.philox_state(11, 4)
    zk = ops.randn(shape, ops.philox_state(11, 4), advance=False).double().cpu()
    got = s.step(e, 333, x, x0, m, generator=state).prev_sample
    assert ops.philox_state_values(state) == (11, 6) and got.shape == shape and got.is_cuda
    want = r.step(5, e.double().cpu(), x.double().cpu(), x0.double().cpu(), m.double(), zk, torch.zeros(shape, dtype=torch.float64))
    assert r.folded[5] == (2, 0) and int(r.timesteps[5]) == 333
    rel = _rel(got.cpu(), want)
    keep = (m == 0).expand(shape)
    a = float(s.alphas_cumprod[167])
    torch.testing.assert_close(got.cpu()[keep].double(), (a ** 0.5 * x0.double().cpu() + (1 - a) ** 0.5 * zk)[keep], rtol=1e-5, atol=1e-6)
    # an int seed and a torch.Generator name the same stream; it is kept from draw 0 on until the next set_timesteps
    outs = [s.step(e, 333, x, x0, m, generator=gen).prev_sample for gen in (torch.Generator().manual_seed(11), ops.philox_state(11))]
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], got)
    # undo_step from t = 167 (level 1) to t = 333 (level 2)
    state = ops.philox_state(11, 8)
    z = ops.randn(shape, ops.philox_state(11, 8), advance=False).double().cpu()
    up = s.undo_step(x, 167, generator=state)
    ratio = r.abar(2) / r.abar(1)
    rel = max(rel, _rel(up.cpu(), ratio ** 0.5 * x.double().cpu() + (1 - ratio) ** 0.5 * z))
    assert ops.philox_state_values(state) == (11, 9)
    _record(rel, "max_rel")
    assert rel <= 1e-5, rel
    with pytest.raises(ValueError):
        s.undo_step(x, 999)


# ---- the engines on the tiny UNet -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_unets():
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from oracle import configs
    from oracle.unet import UNet2DConditionModel as OUNet
    cfg = configs.tiny_unet()
    torch.manual_seed(5)
    ref = OUNet(**cfg).eval()
    mine = UNet2DConditionModel(**cfg)
    mine.load_state_dict(ref.state_dict())
    return mine.cuda(), ref


def _cond(B=2, h=16, w=16):
    g = torch.Generator().manual_seed(0)
    lat, x0 = torch.randn(B, 8, h, w, generator=g), torch.randn(B, 8, h, w, generator=g)
    pe = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=-1)
    m = torch.ones(B, h, w)
    m[:, : h // 2] = 0.0                                             # half the rows are kept
    return lat, x0, pe, ne, m


def _engine(use_graph, seed, h=16, plan=None):
    from audioldm_with_lora_amd.engine import DenoiseEngine, WindowedAudioToAudioEngine
    unet, _ = _tiny_unets()
    lat, x0, pe, ne, m = _cond(h=h)
    s = _repaint()
    if plan is None:
        eng = DenoiseEngine(unet, s, 2, h, 16, N, 2.5, use_graph=use_graph, masked=True)
    else:
        eng = WindowedAudioToAudioEngine(unet, s, 2, plan, 16, N, 2.5, use_graph=use_graph, masked=True)
    assert eng.repaint and eng.n_steps == L
    eng.set_condition(pe, ne)
    eng.set_seed(seed)
    eng.set_latents(lat)
    eng.set_inpaint(x0, torch.zeros_like(x0), m)                     # (the loop's eps is not read by this solver)
    return eng, lat, x0, m


def test_engine_replay_equals_eager_and_seeds():
    from audioldm_with_lora_amd import ops
    outs = {}
    for use_graph in (False, True):
        eng, lat, x0, m = _engine(use_graph, 41)
        before = (eng.x.clone(), eng.x_in[0].clone(), eng.step_idx.clone(), eng.t_buf.clone())
        eng.capture()
        assert (eng.graph is not None) == use_graph
        assert ops.philox_state_values(eng.rng) == (41, 0)                    # capture() leaves the state as it found it
        for a, bb in zip(before, (eng.x, eng.x_in[0], eng.step_idx, eng.t_buf)):
            assert torch.equal(_bits(a) if a.dtype != torch.int32 else a, _bits(bb) if bb.dtype != torch.int32 else bb)
        eng.run()
        outs[use_graph] = eng.latents_nchw().cpu()
        assert int(eng.step_idx.item()) == 0 and int(eng.ticket.item()) == 0 and ops.philox_state_values(eng.rng) == (41, 2 * L)
    assert torch.equal(outs[False], outs[True]) and torch.isfinite(outs[True]).all()
    keep = (m == 0)[:, None].expand_as(x0)
    assert torch.equal(outs[True][keep], x0[keep]) and not torch.equal(outs[True][~keep], x0[~keep])
    eng.set_latents(lat)                                                      # the same seed and latents again: identical
    assert ops.philox_state_values(eng.rng) == (41, 0)
    eng.run()
    assert torch.equal(eng.latents_nchw().cpu(), outs[True])
    eng.set_seed(42)                                                          # another seed: the regenerated region differs, the kept one is x0
    eng.set_latents(lat)
    eng.run()
    other = eng.latents_nchw().cpu()
    assert torch.equal(other[keep], x0[keep]) and not torch.equal(other[~keep], outs[True][~keep]) and torch.isfinite(other).all()
    assert ops.philox_state_values(eng.rng) == (42, 2 * L)


def test_engine_refusals():
    from audioldm_with_lora_amd.engine import DenoiseEngine, WindowedAudioToAudioEngine, WindowedDenoiseEngine
    from audioldm_with_lora_amd.longform import WindowPlan
    unet, _ = _tiny_unets()
    with pytest.raises(ValueError, match="mask"):
        DenoiseEngine(unet, _repaint(), 2, 16, 16, N, 2.5)
    with pytest.raises(ValueError, match="mask"):
        WindowedDenoiseEngine(unet, _repaint(), 2, WindowPlan(56, 32, 8), 16, N, 2.5)
    with pytest.raises(NotImplementedError, match="begin_index"):
        DenoiseEngine(unet, _repaint(), 2, 16, 16, N, 2.5, masked=True, begin_index=2)
    with pytest.raises(NotImplementedError, match="begin_index"):
        WindowedAudioToAudioEngine(unet, _repaint(), 2, WindowPlan(56, 32, 8), 16, N, 2.5, masked=True, begin_index=2)
    with pytest.raises(NotImplementedError, match="chains"):
        DenoiseEngine(unet, _repaint(), 2, 16, 16, N, 2.5, masked=True, chains=2)


def test_ten_call_cfg_loop_against_oracle_unet():
    """10 UNet calls (N = 6, 2, 2), CFG 2.5, half the rows kept: the oracle UNet driven by the float64 restatement with the device's own
    zk, zj.  Relative L2 <= 5e-2, the bound of the project's other 10-call loops."""
    from audioldm_with_lora_amd import ops
    from oracle.pipeline import cfg_combine
    _, ref = _tiny_unets()
    lat, x0, pe, ne, m = _cond()
    r = R.RePaintRestatement(JL, JS)
    r.set_timesteps(N)

    def draw(d):                                                     # the engine's draw d, element order NHWC
        B, C, H, W = lat.shape
        return ops.randn((B, H, W, C), ops.philox_state(77, d), advance=False).cpu().permute(0, 3, 1, 2).double()

    x, emb = lat.double(), torch.cat([ne, pe])
    with torch.no_grad():
        for k, t in enumerate(r.timesteps.tolist()):
            eps = cfg_combine(ref(torch.cat([x, x]).float(), torch.tensor(t), encoder_hidden_states=None, class_labels=emb)[0], 2.5)
            x = r.step(k, eps.double(), x, x0.double(), m.double()[:, None], draw(2 * k), draw(2 * k + 1))
    eng, _, _, _ = _engine(True, 77)
    eng.capture()
    eng.run()
    got = eng.latents_nchw().cpu()
    rel = _rel(got, x)
    _record(rel, "rel_l2")
    print(f"10-call RePaint loop vs the oracle UNet: rel L2 {rel:.3e}")
    assert torch.isfinite(got).all() and rel <= 5e-2, rel


def test_windowed_engine_one_window_is_the_plain_engine_and_two_windows_keep_x0():
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.longform import WindowPlan
    out = []
    for plan in (None, WindowPlan(32, 32, 8)):
        eng, _, _, _ = _engine(True, 77, h=32, plan=plan)
        assert plan is None or eng.K == 1
        eng.capture()
        eng.run()
        out.append((eng.latents_nchw().cpu(), eng.x_in[0].cpu(), eng.rng.cpu()))
    for a, bb in zip(*out):
        assert torch.equal(_bits(a) if a.dtype != torch.int32 else a, _bits(bb) if bb.dtype != torch.int32 else bb)
    plan = WindowPlan(56, 32, 8)
    eng, _, x0, m = _engine(True, 77, h=56, plan=plan)
    assert eng.K == 2 and eng.x_in[0].shape == (2 * 2 * 2, 32, 16, 8)
    eng.capture()
    eng.run()
    got = eng.latents_nchw().cpu()
    keep = (m == 0)[:, None].expand_as(x0)
    assert torch.isfinite(got).all() and torch.equal(got[keep], x0[keep]) and not torch.equal(got[~keep], x0[~keep])
    assert int(eng.step_idx.item()) == 0 and ops.philox_state_values(eng.rng) == (77, 2 * L)


# ---- the pipeline and the script on tiny models ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    import synth_checkpoint
    from audioldm_with_lora_amd.pipeline import AudioLDMPipeline
    root = str(tmp_path_factory.mktemp("model"))
    synth_checkpoint.write_model_dir(root)
    return root, AudioLDMPipeline.from_pretrained(root).to("cuda")


def test_audio_to_audio_pipeline_with_the_scheduler_swapped(tiny):
    from audioldm_with_lora_amd.audio2audio import AudioLDMAudioToAudioPipeline, regeneration_mask
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, RePaintScheduler
    _, pipe = tiny
    a2a = AudioLDMAudioToAudioPipeline.from_pipe(pipe)
    g = torch.Generator().manual_seed(21)
    pe = torch.nn.functional.normalize(torch.randn(1, 64, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(1, 64, generator=g), dim=-1)
    n = int(1.28 * 16000)
    t = torch.arange(n) / 16000.0
    audio = (0.3 * torch.sin(2 * np.pi * 220 * t) + 0.05 * torch.randn(n, generator=g))[None]
    mask = regeneration_mask(128, 64, seconds=(0.4, 0.96))
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, mask=mask, strength=1.0, num_inference_steps=N, guidance_scale=2.5,
                output_type="latent")
    gen = lambda s: torch.Generator().manual_seed(s)
    ddim = a2a(generator=gen(6), **call).audios
    n_engines = len(a2a._engines)
    a2a.scheduler = RePaintScheduler.from_config(pipe.scheduler.config, jump_length=JL, jump_n_sample=JS)
    r1 = a2a(generator=gen(6), **call).audios
    r2 = a2a(generator=gen(6), **call).audios
    r3 = a2a(generator=gen(7), **call).audios
    assert len(a2a._engines) == n_engines + 1 and any(e.repaint and e.n_steps == L for e in a2a._engines.values())
    assert r1.shape == (1, 8, 32, 16) and torch.isfinite(r1).all() and torch.equal(r1, r2) and not torch.equal(r1, r3)
    assert torch.equal(r1[:, :, :10], ddim[:, :, :10]) and torch.equal(r1[:, :, 24:], ddim[:, :, 24:])      # the kept rows: the same x0
    assert not torch.equal(r1[:, :, 10:24], ddim[:, :, 10:24])
    # other jump parameters are another engine
    a2a.scheduler = RePaintScheduler.from_config(pipe.scheduler.config, jump_length=JL, jump_n_sample=3)
    assert torch.isfinite(a2a(generator=gen(6), **call).audios).all() and len(a2a._engines) == n_engines + 2
    # what RePaint cannot do is refused before any device work
    with pytest.raises(ValueError, match="mask"):
        a2a(generator=gen(6), **dict(call, mask=None))
    with pytest.raises(ValueError, match="strength"):
        a2a(generator=gen(6), **dict(call, strength=0.5))
    assert len(a2a._engines) == n_engines + 2
    t2a = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio_length_in_s=1.28, num_inference_steps=N, guidance_scale=2.5)
    saved = pipe.scheduler
    try:
        pipe.scheduler = a2a.scheduler
        with pytest.raises(ValueError, match="mask"):
            pipe(**t2a)
    finally:
        pipe.scheduler = saved
    # back: a NEW DDIM object with the same configuration reproduces the first output bit for bit
    a2a.scheduler = DDIMScheduler.from_config(pipe.scheduler.config)
    assert torch.equal(a2a(generator=gen(6), **call).audios, ddim)
    assert any(e.scheduler is a2a.scheduler for e in a2a._engines.values())


def test_inference_script_repaint(tiny, tmp_path):
    from scipy.io import wavfile
    from audioldm_with_lora_amd.script import inference
    root, _ = tiny
    src = str(tmp_path / "in.wav")
    n = 46080
    wavfile.write(src, 16000, (0.3 * np.sin(2 * np.pi * 330 * np.arange(n) / 16000)).astype(np.float32))
    base = ["--model-dir", root, "--no-lora", "--steps", str(N), "--guidance-scale", "2.5", "--seed", "1", "--init-audio", src, "--repaint", "2,2"]
    windows = ["--window-seconds", "1.28", "--window-overlap-seconds", "0.32"]
    for name, extra in (("plain", ["--regenerate-seconds", "0.9,2.0"]), ("windowed", ["--regenerate-seconds", "0.9,2.0"] + windows)):
        out = str(tmp_path / f"{name}.wav")
        inference.main(base + extra + ["--output", out])
        sr, wav = wavfile.read(out)
        assert sr == 16000 and wav.shape == (n,) and wav.dtype == np.float32 and np.isfinite(wav).all(), name
    args = inference.parse_args(base + ["--regenerate-bands", "0.5,1.0"])
    assert args.repaint == (2, 2) and args.strength == 1.0
    assert inference.parse_args(["--model-dir", root]).strength == 0.5 and inference.parse_args(["--model-dir", root]).repaint is None
    for bad in (base + ["--regenerate-seconds", "0.9,2.0", "--strength", "0.5"],      # RePaint runs from noise
                base,                                                                  # no mask
                ["--model-dir", root, "--repaint", "2,2", "--regenerate-seconds", "0.9,2.0"],      # no --init-audio
                base[:-1] + ["2", "--regenerate-seconds", "0.9,2.0"],                  # not two numbers
                base[:-1] + ["0,2", "--regenerate-seconds", "0.9,2.0"],
                base + ["--regenerate-seconds", "0.9,2.0", "--scheduler", "euler-a"]):
        with pytest.raises(SystemExit):
            inference.parse_args(bad)
