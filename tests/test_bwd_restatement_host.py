"""CPU checks of tests/bwd_restatement.py: (1) every `exact` restatement equals float64 torch autograd, (2) the comparator
`check` -- not the kernels -- is proven sharp: every listed mutant of every op, computed in float64 and rounded the way `rounded`
rounds, is rejected at the shapes tests/test_gpu_bwd_edges.py runs, while the comparator the op tests used before (`old_close`,
tests/test_gpu_train_ops.py's `close`) accepts it at one of the shapes and input draws those tests use."""
import math

import pytest
import torch
import torch.nn.functional as F

import bwd_restatement as R

F64 = torch.float64


def same(a, b, tol=1e-9):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# formula check: exact == float64 autograd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", [0, 1])
def test_groupnorm_exact_is_autograd(silu):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 24, 5, 7, generator=g, dtype=F64).requires_grad_()
    gm, bt = torch.randn(24, generator=g, dtype=F64), torch.randn(24, generator=g, dtype=F64)
    dy = torch.randn(2, 24, 5, 7, generator=g, dtype=F64)
    y = F.group_norm(x, 2, gm, bt, 1e-5)
    (F.silu(y) if silu else y).backward(dy)
    same(R.groupnorm_bwd(x.detach(), dy, gm, bt, 2, 1e-5, silu), x.grad)
    prior = torch.randn(2, 24, 5, 7, generator=g, dtype=F64)
    same(R.groupnorm_bwd(x.detach(), dy, gm, bt, 2, 1e-5, silu, prior=prior), x.grad + prior)


def test_layernorm_exact_is_autograd():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(9, 264, generator=g, dtype=F64).requires_grad_()
    gm, bt = torch.randn(264, generator=g, dtype=F64), torch.randn(264, generator=g, dtype=F64)
    dy = torch.randn(9, 264, generator=g, dtype=F64)
    F.layer_norm(x, (264,), gm, bt, 1e-5).backward(dy)
    same(R.layernorm_bwd(x.detach(), dy, gm, 1e-5), x.grad)


def test_geglu_exact_is_autograd():
    g = torch.Generator().manual_seed(2)
    h = torch.randn(7, 64, generator=g, dtype=F64).requires_grad_()
    dout = torch.randn(7, 32, generator=g, dtype=F64)
    y = h[:, :32] * F.gelu(h[:, 32:])
    y.backward(dout)
    same(R.geglu_fwd(h.detach()), y.detach())
    same(R.geglu_bwd(h.detach(), dout), h.grad)
    order = R.geglu_pack_order(32)                      # 16 value | 16 gate interleaving: a permutation of the 2I columns
    assert sorted(order.tolist()) == list(range(64)) and order[:32].tolist() == list(range(16)) + list(range(32, 48))


@pytest.mark.parametrize("B,N,H,d", [(2, 37, 3, 8), (1, 70, 2, 40)])
def test_attention_exact_is_autograd(B, N, H, d):
    g = torch.Generator().manual_seed(3)
    C = H * d
    qkv = torch.randn(B * N, 3 * C, generator=g, dtype=F64).requires_grad_()
    dO = torch.randn(B * N, C, generator=g, dtype=F64)
    sp = lambda z: z.reshape(B, N, H, d).transpose(1, 2)
    o = F.scaled_dot_product_attention(sp(qkv[:, :C]), sp(qkv[:, C:2 * C]), sp(qkv[:, 2 * C:])).transpose(1, 2).reshape(B * N, C)
    o.backward(dO)
    o_e, lse = R.attention_fwd(qkv.detach(), B, N, H, d)
    same(o_e, o.detach())
    s = (sp(qkv[:, :C]) @ sp(qkv[:, C:2 * C]).transpose(-1, -2)).detach() / math.sqrt(d)
    same(lse, torch.logsumexp(s, -1) * R.LOG2E)
    same(R.attention_bwd(qkv.detach(), dO, o_e, lse, B, N, H, d), qkv.grad)


@pytest.mark.parametrize("ih,iw,oh,ow", [(32, 2, 63, 4), (63, 4, 125, 8), (8, 4, 16, 8)])
def test_upsample_exact_is_interpolate_adjoint(ih, iw, oh, ow):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, ih, iw, generator=g, dtype=F64).requires_grad_()
    dy = torch.randn(2, 3, oh, ow, generator=g, dtype=F64)
    up = F.interpolate(x, size=(oh, ow), mode="nearest")
    # the source map src = floor(dst * I / O) is F.interpolate's own
    assert torch.equal(up.detach(), x.detach()[:, :, R._nearest_src(oh, ih)][:, :, :, R._nearest_src(ow, iw)])
    (up * dy).sum().backward()
    same(R.upsample_nearest_bwd(dy, ih, iw), x.grad)


def test_lora_site_exact_is_autograd():
    x, W, bias, parts, dy, rs = R.site_draw(37, 64, 192, (16, 16, 16), res=True)
    xv = x.clone().requires_grad_()
    As = [p[2].to(F64).requires_grad_() for p in parts]
    Bs = [p[3].to(F64).requires_grad_() for p in parts]
    y = xv @ W.t() + bias + rs + torch.cat([s * (xv @ A.t()) @ Bm.t() for (_, _, _, _, s), A, Bm in zip(parts, As, Bs)], 1)
    y.backward(dy)
    ref = R.lora_site(x, W, bias, parts, dy, res=rs)
    same(ref["y"], y.detach())
    same(ref["dx"], xv.grad)
    for i in range(3):
        same(ref["dA"][i], As[i].grad)
        same(ref["dB"][i], Bs[i].grad)
    # the rounded form's T / U are what the rank-r gradient products read: dA = U^T x, dB = s dy^T T
    for i, (row0, nrows, A, Bm, s) in enumerate(parts):
        same(s * R.tn_exact(dy[:, row0:row0 + nrows], ref["T"][i])[0], ref["dB"][i])
        same(R.tn_exact(ref["U"][i], x)[0], ref["dA"][i])


# ---------------------------------------------------------------------------------------------------------------------------------
# mutant check
# ---------------------------------------------------------------------------------------------------------------------------------
NORM_MUTANTS = ("no_s1", "no_s2", "neither", "n")
# A miscount of the strip length by n_extra perturbs xhat by (n_extra / n) * |mean| / std and s1, s2 by n_extra / n.  Below the
# bf16 rounding of the output (2^-8 relative) no parity test can see it; it must be rejected from four times that on.
N_MUTANT_VISIBLE = 2.0 ** -6


def _n_mutant_size(xrows, n_extra):
    n = xrows.shape[1]
    return n_extra / n * max(1.0, float((xrows.mean(1).abs() / xrows.std(1)).max()))


@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_groupnorm_mutants_rejected_at_every_new_shape(case):
    G = case[1]
    for variant in R.GN_VARIANTS:
        for pivot in ((False, True) if case in R.GN_PIVOT_CASES and variant == "plain" else (False,)):
            x, dy, gm, bt, act, C1, prior = R.gn_draw(case, variant, pivot)
            exact = R.groupnorm_bwd(x, dy, gm, bt, G, 1e-5, act, prior)
            rounded = R.groupnorm_bwd(x, dy, gm, bt, G, 1e-5, act, prior, rounded=True)
            assert R.accepts(rounded, exact, rounded)
            for m in NORM_MUTANTS:
                if m == "n" and _n_mutant_size(R.gn_rows(x, G), x.shape[1] // G) < N_MUTANT_VISIBLE:
                    continue
                mut = R.groupnorm_bwd(x, dy, gm, bt, G, 1e-5, act, prior, rounded=True, mutant=m)
                e_l2, f_l2, _, _ = R.floor_ratios(mut, exact, rounded)
                assert e_l2 > R.L2_MARGIN * f_l2, (variant, pivot, m, e_l2 / f_l2)      # the L2 condition alone catches it


def test_groupnorm_n_mutant_is_visible_on_the_pivot_cases():
    for case in R.GN_PIVOT_CASES:
        x = R.gn_draw(case, "plain", True)[0]
        assert _n_mutant_size(R.gn_rows(x, case[1]), x.shape[1] // case[1]) >= N_MUTANT_VISIBLE


def _old_gn_draw(B, G, C, H, W):
    g = torch.Generator().manual_seed(0)                                 # test_groupnorm_bwd's draw
    x = R.bf16_input(torch.randn(B, C, H, W, generator=g) * 2 + 0.3)
    gm, bt = torch.randn(C, generator=g).to(F64), torch.randn(C, generator=g).to(F64)
    return x, R.bf16_input(torch.randn(B, C, H, W, generator=g)), gm, bt


@pytest.mark.parametrize("m", NORM_MUTANTS)
def test_groupnorm_mutants_passed_the_old_comparator(m):
    ok = []
    for (B, G, C, H, W, act) in R.GN_OLD_CASES:
        x, dy, gm, bt = _old_gn_draw(B, G, C, H, W)
        want = R.groupnorm_bwd(x, dy, gm, bt, G, 1e-5, act)
        ok.append(R.old_close(R.groupnorm_bwd(x, dy, gm, bt, G, 1e-5, act, rounded=True, mutant=m), want))
    assert any(ok), ok
    if m in ("no_s1", "n"):
        assert all(ok), ok                                               # these passed every case the suite had


@pytest.mark.parametrize("Cc", R.LN_CS)
def test_layernorm_mutants_rejected_at_every_new_shape(Cc):
    for M in R.LN_MS:
        x, dy, gm, prior = R.ln_draw(M, Cc)
        for pr in (None, prior):
            exact = R.layernorm_bwd(x, dy, gm, 1e-5, pr)
            rounded = R.layernorm_bwd(x, dy, gm, 1e-5, pr, rounded=True)
            assert R.accepts(rounded, exact, rounded)
            for m in NORM_MUTANTS:
                if m == "n" and _n_mutant_size(x, 8) < N_MUTANT_VISIBLE:
                    continue
                mut = R.layernorm_bwd(x, dy, gm, 1e-5, pr, rounded=True, mutant=m)
                e_l2, f_l2, _, _ = R.floor_ratios(mut, exact, rounded)
                assert e_l2 > R.L2_MARGIN * f_l2, (M, pr is not None, m, e_l2 / f_l2)


def test_layernorm_mutants_and_the_old_comparator():
    """test_layernorm_and_geglu_bwd's draws (one generator, C = 64, 256, 640 in turn).  Recorded as found: with 64 to 640 elements
    per row the old tolerance did see a missing `xh * s2` term; it let the missing `s1` and the miscounted n through."""
    g = torch.Generator().manual_seed(1)
    ok = {m: [] for m in NORM_MUTANTS}
    for Cc in (64, 256, 640):
        x = R.bf16_input(torch.randn(50, Cc, generator=g) * 2 + 1)
        gm, _ = torch.randn(Cc, generator=g).to(F64), torch.randn(Cc, generator=g)
        dy = R.bf16_input(torch.randn(50, Cc, generator=g))
        want = R.layernorm_bwd(x, dy, gm, 1e-5)
        for m in NORM_MUTANTS:
            ok[m].append(R.old_close(R.layernorm_bwd(x, dy, gm, 1e-5, rounded=True, mutant=m), want))
        torch.randn(50, Cc, generator=g)                                 # (the test's `prev` draw)
    assert any(ok["no_s1"]) and any(ok["n"]), ok
    assert not any(ok["no_s2"]) and not any(ok["neither"]), ok


def test_geglu_mutant():
    for (M, I) in R.GEGLU_CASES:
        h, dout = R.geglu_draw(M, I)
        assert set(R.GEGLU_EDGE_GATES) <= set(h[:, I:].reshape(-1).tolist()) or M * I < len(R.GEGLU_EDGE_GATES)
        exact, rounded = R.geglu_bwd(h, dout), R.geglu_bwd(h, dout, rounded=True)
        assert R.accepts(rounded, exact, rounded)
        assert not R.accepts(R.geglu_bwd(h, dout, rounded=True, mutant="no_pdf"), exact, rounded), (M, I)
    # the old case: M = 40, I = 64, one generator after the three layer-norm cases
    g = torch.Generator().manual_seed(1)
    for Cc in (64, 256, 640):
        for shape in ((50, Cc), (Cc,), (Cc,), (50, Cc), (50, Cc)):
            torch.randn(*shape, generator=g)
    h = R.bf16_input(torch.randn(40, 128, generator=g))
    dout = R.bf16_input(torch.randn(40, 64, generator=g))
    ok = R.old_close(R.geglu_bwd(h, dout, rounded=True, mutant="no_pdf"), R.geglu_bwd(h, dout))
    assert not ok                                   # recorded as found: the old tolerance did see this one


def test_upsample_mutant():
    for (B, C) in R.UPS_BC:
        for (ih, iw, oh, ow) in R.UPS_SIZES:
            g = torch.Generator().manual_seed(ih + oh)
            dy = R.bf16_input(torch.randn(B, C, oh, ow, generator=g, dtype=F64))
            exact, rounded = R.upsample_nearest_bwd(dy, ih, iw), R.upsample_nearest_bwd(dy, ih, iw, rounded=True)
            assert R.accepts(rounded, exact, rounded)
            mut = R.upsample_nearest_bwd(dy, ih, iw, rounded=True, mutant="shift")
            if oh % ih or ow % iw:
                assert not R.accepts(mut, exact, rounded), (ih, iw, oh, ow)
            else:
                assert torch.equal(mut, rounded)        # integer ratios: the mutant is the operation itself (the old test's 8x4 -> 16x8)


ATTN_MUTANTS = ("last_query", "delta8", "noscale")
ATTN_NEW = ([(1, 100, 2, d, False) for d in R.ATTN_DS] + [(1, N, 2, 32, False) for N in R.ATTN_NS] +
            [(B, 200, H, 32, False) for (B, H) in R.ATTN_PAIRS] + [(1, N, 2, d, True) for (N, d) in R.ATTN_PEAKED])


@pytest.mark.parametrize("B,N,H,d,peaked", ATTN_NEW)
def test_attention_mutants_rejected_at_every_new_shape(B, N, H, d, peaked):
    qkv, dO = R.attn_draw(B, N, H, d, peaked)
    o_e, o_r, lse, g_e, g_r = R.attention_pair(qkv, dO, B, N, H, d)
    C = H * d
    parts = lambda t: [t[:, i * C:(i + 1) * C] for i in range(3)]
    assert R.accepts(o_r, o_e, o_r) and all(R.accepts(r, e, r) for r, e in zip(parts(g_r), parts(g_e)))
    for m in ATTN_MUTANTS:
        if m == "noscale" and N == 1:
            continue                                    # one token: dS = 0, dK is zero with or without the scale
        mut = R.attention_bwd(qkv, dO, o_r, lse, B, N, H, d, rounded=True, mutant=m)
        seen = [not (R.floor_ratios(a, e, r)[0] <= R.L2_MARGIN * R.floor_ratios(a, e, r)[1]) for a, e, r in zip(parts(mut), parts(g_e), parts(g_r))]
        assert any(seen), (m, seen)                     # per tensor, by the L2 condition alone
    # A P for dV recomputed from lse + 2^-8 scales dV by 0.9973: inside the bf16 floor, so `check` on dV cannot see it (measured
    # 1.5x the L2 floor) -- which is why lse has a bound of its own, 16 times tighter than this mutant.
    mut = R.attention_bwd(qkv, dO, o_r, lse, B, N, H, d, rounded=True, mutant="lse_ulp")
    if N > 1:
        assert R.accepts(parts(mut)[2], parts(g_e)[2], parts(g_r)[2]) and 2.0 ** -8 > R.LSE_BOUND


def test_attention_mutants_and_the_old_comparator():
    """test_attention_fwd_lse_and_bwd's draws at its five smaller shapes.  Recorded as found: the pooled dQ | dK | dV comparison did
    see these three mutants wherever it ran (by 6x to 180x its tolerance) -- the attention gap was in the arms that never ran, not in
    the tolerance -- and it let a P recomputed from a shifted lse through, at a tenth of its tolerance."""
    for (B, N, H, d) in R.ATTN_OLD:
        g = torch.Generator().manual_seed(3)
        C = H * d
        qkv = R.bf16_input(torch.randn(B * N, 3 * C, generator=g))
        dO = R.bf16_input(torch.randn(B * N, C, generator=g))
        o_e, o_r, lse, g_e, _ = R.attention_pair(qkv, dO, B, N, H, d)
        for m in ATTN_MUTANTS:
            assert not R.old_close(R.attention_bwd(qkv, dO, o_r, lse, B, N, H, d, rounded=True, mutant=m), g_e, rtol=3e-2), (m, N, d)
        assert R.old_close(R.attention_bwd(qkv, dO, o_r, lse, B, N, H, d, rounded=True, mutant="lse_ulp"), g_e, rtol=3e-2)
        lse_mut = lse + 2.0 ** -8                                        # ... and the old lse check (rtol 1e-2 on ~8) passes it too
        assert bool(((lse_mut - lse).abs() <= 1.5e-2 * float(lse.abs().max()) + 1e-2 * lse.abs()).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp32 bound of the rank-r gradient products
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SITE_CASES))
def test_tn_bound_sees_one_missing_row(name):
    """Per part of every LoRA-site case of the GPU test, with the operands the restatement gives the two products (T, dy) and (U, x):
    the bound c |P|^T |Q| holds for a float32 matmul with room to spare and is violated at >= 99 % of the elements by a product
    that misses any ONE of the M rows."""
    M, K, N, ranks, res = R.SITE_CASES[name]
    x, W, bias, parts, dy, rs = R.site_draw(M, K, N, ranks, res=res)
    ref = R.lora_site(x, W, bias, parts, dy, res=rs, rounded=True)
    for i, (row0, nrows, A, Bm, s) in enumerate(parts):
        for P, Q in ((ref["T"][i], dy[:, row0:row0 + nrows]), (ref["U"][i], x)):
            want, mag = R.tn_exact(P, Q)
            unit = R.tn_unit(P, Q)
            assert 0.0 < unit < M * 2.0 ** -24, unit                     # fp32 summation of M terms: at most (M - 1) half-ulps of sum |p q|
            c = R.TN_MARGIN * unit
            for mrow in range(M):
                gone = torch.outer(P[mrow], Q[mrow])                     # what the product loses with row mrow
                assert float((gone.abs() > c * mag).double().mean()) >= 0.99, (name, i, mrow)
