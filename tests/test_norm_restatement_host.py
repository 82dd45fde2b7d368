"""CPU checks of tests/norm_restatement.py: (1) every `exact` restatement equals float64 torch, (2) the comparator `check` is proven
sharp at every shape tests/test_gpu_norm_edges.py runs: every listed mutant, computed in float64 and rounded the way `rounded` rounds,
is rejected, while `rounded` itself and the float32 restatement of the handed-over design (`onepass_f32`) are accepted -- which is
what fixes the top rung of the mean ladder on the reference, never on the GPU; (3) the comparator the forward norm tests used before
(tests/test_gpu_ops.py's `close`) accepts the first three mutants on the inputs those tests draw: data about the past."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_restatement as R

F64 = torch.float64


def same(a, b, tol=1e-9):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def nchw(t, H, W):
    return t.view(t.shape[0], H, W, -1).permute(0, 3, 1, 2)


def rejected(fn, mutant, exact, rounded, **kw):
    got = fn(rounded=True, mutant=mutant, **kw)
    return not R.accepts(got, exact, rounded)


# ---------------------------------------------------------------------------------------------------------------------------------
# formula checks
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
def test_groupnorm_exact_is_torch(act):
    x, gm, bt = R.gn_draw(2, 35, 24, 2)
    want = F.group_norm(nchw(x, 5, 7), 2, gm, bt, 1e-5)
    want = F.silu(want) if act else want
    same(nchw(R.groupnorm(x, gm, bt, 2, 1e-5, act), 5, 7), want)
    # the table fold (float64) of any tiling is the same statistics
    for tl in (R.Tiling(16, 0, 0), R.Tiling(0, 3, 14)):
        a = R._image_quad_sums(x, tl)
        same(a[..., 0], x.view(2, 35, 6, 4).sum((1, 3)))
        same(a[..., 1], (x * x).view(2, 35, 6, 4).sum((1, 3)))


def test_layernorm_and_embedding_exact_is_torch():
    x, gm, bt = R.ln_draw(9, 264)
    same(R.layernorm(x, gm, bt, 1e-5), F.layer_norm(x, (264,), gm, bt, 1e-5))
    ids, word, pos, type0, gm, bt = R.embed_draw(3, 20, 64)
    pid = R.position_ids(ids, 1)
    assert pid[0, :4].tolist() == [2, 3, 1, 4] and pid[2].tolist() == [1] * 20 and pid[1].tolist() == list(range(2, 22))
    want = F.layer_norm(F.embedding(ids, word) + type0 + F.embedding(pid, pos), (64,), gm, bt, 1e-5)
    same(R.embed_layernorm(ids, word, pos, type0, gm, bt, 1e-5, 1), want.view(60, 64))


def test_ln_linear_exact_is_torch_and_fold_is_the_same_algebra():
    x, W, bias, gm, bt, parts = R.ln_linear_draw(19, 128, 96, 4)
    xn = F.layer_norm(x, (128,), gm, bt, 1e-5)
    want = xn @ W.t() + bias
    for row0, nrows, A, Bm, s in parts:
        want[:, row0:row0 + nrows] += s * (xn @ A.to(F64).t()) @ Bm.to(F64).t()
    same(R.ln_linear(x, W, bias, gm, bt, 1e-5, parts), want)
    # the fold with nothing rounded is the same function: r16 = identity
    keep = R.r16, R.pack_round
    R.r16, R.pack_round = (lambda t: t), (lambda b, s: s * b.to(F64))
    try:
        same(R.ln_linear(x, W, bias, gm, bt, 1e-5, parts, rounded=True), want, tol=1e-8)
    finally:
        R.r16, R.pack_round = keep


def test_gn_conv_exact_is_torch():
    x, gm, bt = R.gn_draw(2, 5 * 16, 8, 2)
    g = torch.Generator().manual_seed(0)
    w, b = torch.randn(3, 8, 3, 3, generator=g, dtype=F64), torch.randn(3, generator=g, dtype=F64)
    want = F.conv2d(F.silu(F.group_norm(nchw(x, 5, 16), 2, gm, bt, 1e-5)), w, b, padding=1)
    same(nchw(R.gn_conv(x, gm, bt, 2, 1e-5, 5, 16, w, b), 5, 16), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants at the GPU shapes
# ---------------------------------------------------------------------------------------------------------------------------------
# A mutant that changes the result by less than the bf16 rounding of the output cannot be seen by ANY parity test of a bf16 tensor:
#   unbiased variance scales xhat by 1 - 1 / (2 n): from n = 32 down it is 2^-6, four times the rounding (the same rule as
#   tests/test_bwd_restatement_host.py's strip-length mutant) -- of the GPU shapes that is LayerNorm at C = 8;
#   an eps outside the root or dropped is eps / (2 var) = 8e-5 at eps = 1e-5 and the smallest ladder variance 0.0625: the cases that
#   run at EPS_BIG = 0.1 are there for it;
#   a padded strip length is a mutant only where the padding is not empty.
def gn_mutants(B, HW, C, groups, C1, act, eps, straddles=False):
    m = ["neighbour", "gamma_in_group"] if groups > 1 else ["neighbour"]
    if act:
        m.append("silu_first")
    if C1 < C and C1 % (C // groups):
        m.append("quad_off")
    if eps == R.EPS_BIG:
        m += ["eps_out", "eps_drop"]
    if straddles:
        m.append("straddle_first")
    return m


@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: f"HW{c[1]}C{c[2]}s{c[4]}")
def test_groupnorm_arm_shapes_reject_every_mutant(case):
    B, HW, C, groups, C1, act, eps, arm = case
    assert R.gn_arm(HW, C, groups) == arm
    x, gm, bt = R.gn_draw(B, HW, C, groups)
    fn = lambda **kw: R.groupnorm(x, gm, bt, groups, eps, act, C1=C1, **kw)
    exact, rounded = fn(), fn(rounded=True)
    assert R.accepts(rounded, exact, rounded)
    muts = gn_mutants(B, HW, C, groups, C1, act, eps)
    n_pad = R.gn_n_pad(HW, C // groups)
    if n_pad != HW * (C // groups):
        assert not R.accepts(fn(rounded=True, mutant="n_pad", n_pad=n_pad), exact, rounded), "n_pad"
    for m in muts:
        assert rejected(fn, m, exact, rounded), m


@pytest.mark.parametrize("C", R.LN_CS)
def test_layernorm_shapes_reject_every_mutant(C):
    for M in R.LN_MS:
        for eps in (R.EPS, R.EPS_BIG):
            x, gm, bt = R.ln_draw(M, C)
            fn = lambda **kw: R.layernorm(x, gm, bt, eps, **kw)
            exact, rounded = fn(), fn(rounded=True)
            assert R.accepts(rounded, exact, rounded)
            muts = (["neighbour"] if M > 1 else []) + (["unbiased"] if C <= 32 else []) + (["eps_out", "eps_drop"] if eps == R.EPS_BIG else [])
            # eps mutants show on the rows of scale 0.25 only: M = 1 is a row of scale 0.25 (ladder(., 1): scale rung o % 3)
            for m in muts:
                assert rejected(fn, m, exact, rounded), (M, eps, m)
            if R.ln_n_pad(C) != C:
                assert not R.accepts(fn(rounded=True, mutant="n_pad", n_pad=R.ln_n_pad(C)), exact, rounded), (M, "n_pad")


@pytest.mark.parametrize("case", R.EMBED_CASES)
def test_embed_layernorm_shapes_reject_every_mutant(case):
    B, L, C = case
    ids, word, pos, type0, gm, bt = R.embed_draw(B, L, C)
    fn = lambda **kw: R.embed_layernorm(ids, word, pos, type0, gm, bt, 1e-5, 1, **kw)
    exact, rounded = fn(), fn(rounded=True)
    assert R.accepts(rounded, exact, rounded)
    for m in ("neighbour", "pos_plain"):
        assert rejected(fn, m, exact, rounded), m


def apply_n_pad(case, tilings):
    """the strip of a generic producer padded to whole M-tiles (a halo producer: to whole tiles of its image)"""
    name, B, H, W, C1, C2, groups = case[:7]
    t = tilings[0]
    rows = -(-H * W // t.bm) * t.bm if t.tpi == 0 else t.tpi * t.pix
    return rows * ((C1 + C2) // groups)


@pytest.mark.parametrize("case", R.APPLY_CASES, ids=lambda c: c[0])
def test_groupnorm_apply_shapes_reject_every_mutant_and_accept_the_design(case):
    name, B, H, W, C1, C2, groups, t1, t2, act, eps = case
    HW, C = H * W, C1 + C2
    x, gm, bt, tilings = R.apply_draw(case)
    fn = lambda **kw: R.groupnorm(x, gm, bt, groups, eps, act, C1=C1, tilings=tilings, **kw)
    exact, rounded = fn(), fn(rounded=True)
    assert R.accepts(rounded, exact, rounded)
    # the contract ceiling of the mean ladder: the documented float32 one-pass fold is within the floor at the top rung
    assert R.accepts(fn(rounded=True, design="onepass_f32"), exact, rounded), "the float32 one-pass design misses the floor at |mean| / std = 16"
    straddles = any(t.tpi == 0 and HW % t.bm for t in tilings) and B > 1
    if name in ("straddle", "concat", "g1"):
        assert straddles
    for m in gn_mutants(B, HW, C, groups, C1, act, eps, straddles):
        assert rejected(fn, m, exact, rounded), m
    n_pad = apply_n_pad(case, tilings)
    if n_pad != HW * (C // groups):
        assert not R.accepts(fn(rounded=True, mutant="n_pad", n_pad=n_pad), exact, rounded), "n_pad"


@pytest.mark.parametrize("hw", R.PARTIALS_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_groupnorm_partials_shapes_reject_every_mutant(hw):
    H, W = hw
    d = R.partials_draw(H, W)
    gm, bt = d["gamma"], d["beta"]
    for h, C, groups, eps, act in ((d["h_rowbias"], 64, 16, R.EPS, 1), (d["h_res"], 64, 16, R.EPS_BIG, 0), (d["h_cat"], 128, 32, R.EPS_BIG, 1)):
        fn = lambda **kw: R.groupnorm(h, gm[:C], bt[:C], groups, eps, act, C1=64, **kw)
        exact, rounded = fn(), fn(rounded=True)
        assert R.accepts(rounded, exact, rounded)
        muts = ["neighbour", "gamma_in_group"] + (["silu_first"] if act else []) + (["eps_out", "eps_drop"] if eps == R.EPS_BIG else [])
        for m in muts:
            assert rejected(fn, m, exact, rounded), m
        n_pad = R.gn_n_pad(H * W, 4)
        if n_pad != H * W * 4:
            assert not R.accepts(fn(rounded=True, mutant="n_pad", n_pad=n_pad), exact, rounded), "n_pad"


@pytest.mark.parametrize("case", R.LNLIN_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_folded_layernorm_shapes_reject_every_mutant_and_accept_the_design(case):
    route, M, K, N, r = case
    x, W, bias, gm, bt, parts = R.ln_linear_draw(M, K, N, r)
    for eps in (R.EPS, R.EPS_BIG):
        fn = lambda **kw: R.ln_linear(x, W, bias, gm, bt, eps, parts, **kw)
        exact, rounded = fn(), fn(rounded=True)
        assert R.accepts(rounded, exact, rounded)
        assert R.accepts(fn(rounded=True, design="onepass_f32", nparts=K // 64), exact, rounded), "one-pass design at the top rung"
        muts = ["neighbour", "s_unrounded"] + (["t_round_first"] if r else []) + (["eps_out", "eps_drop"] if eps == R.EPS_BIG else [])
        for m in muts:
            assert rejected(fn, m, exact, rounded), (eps, m)


@pytest.mark.parametrize("kind,N", [(64, n) for n in R.ATTN64_NS] + [(256, n) for n in R.ATTN256_NS])
def test_attn_block_shapes_reject_projection_mutants_and_accept_the_design(kind, N):
    """the fused block's output still shows a wrong folded LayerNorm: mutants enter through ln_linear, the attention is the float64 one"""
    H, d, B = 8, (80 if kind == 64 else 48), 2
    C = H * d
    x, W, _, gm, bt, parts = R.ln_linear_draw(B * N, C, 3 * C, 4)
    fn = lambda **kw: R.attn_block(x, W, gm, bt, 1e-5, parts, B, N, H, d, **kw)
    exact, rounded = fn(), fn(rounded=True)
    assert R.accepts(rounded, exact, rounded)
    # both blocks are one-pass sites: statistics from C / 64 partial pairs per row (10 at C = 640, 6 at C = 384)
    assert R.accepts(fn(rounded=True, design="onepass_f32", nparts=C // 64), exact, rounded), "one-pass design at the top rung"
    for m in ("neighbour", "s_unrounded", "t_round_first"):
        assert rejected(fn, m, exact, rounded), m


@pytest.mark.parametrize("ptile", R.CONSUMER_PTILES)
def test_gn_conv_consumer_shapes_reject_statistics_mutants_and_accept_the_design(ptile):
    d = R.consumer_draw()
    B, H, W, x, gm, bt = d["B"], d["H"], d["W"], d["x"], d["gamma"], d["beta"]
    tl = [R.tiling_for(ptile, B, H, W)]
    straddles = tl[0].tpi == 0 and (H * W) % tl[0].bm
    assert straddles or ptile == 7
    forms = (("gn_silu_conv_out", d["w8"], d["b8"].to(F64), None, False), ("conv gn_in", d["w"], d["b"].to(F64), d["extra"], True))
    for what, w, b, extra, out_bf16 in forms:
        fn = lambda **kw: R.gn_conv(x, gm, bt, d["groups"], R.EPS, H, W, w, b, extra, out_bf16=out_bf16, tilings=tl, **kw)
        exact, rounded = fn(), fn(rounded=True)
        assert R.accepts(rounded, exact, rounded)
        assert R.accepts(fn(rounded=True, design="onepass_f32"), exact, rounded), what
        for m in ["neighbour", "gamma_in_group", "silu_first"] + (["straddle_first"] if straddles else []):
            assert rejected(fn, m, exact, rounded), (what, m)


@pytest.mark.parametrize("tile", R.RANDOM_PRODUCER_TILES)
def test_random_weight_producer_shape_rejects_statistics_mutants_and_accepts_the_design(tile):
    """the GPU case judges the consumer against the float64 GroupNorm of the STORED tensor; here that tensor is the bf16-rounded float64
    convolution (the kernel's may differ from it in a last bit here and there, which changes nothing about what the comparator sees)"""
    d = R.random_producer_draw()
    B, H, W, groups, gm, bt = d["B"], d["H"], d["W"], d["groups"], d["gamma"], d["beta"]
    stored = R.r16(R.conv3x3(d["xin"], H, W, d["w"], d["bias"].to(F64)))
    tl = [R.tiling_for(tile, B, H, W)]
    straddles = tl[0].tpi == 0 and (H * W) % tl[0].bm
    fn = lambda **kw: R.groupnorm(stored, gm, bt, groups, R.EPS, 1, tilings=tl, **kw)
    exact, rounded = fn(), fn(rounded=True)
    assert R.accepts(fn(rounded=True, design="onepass_f32"), exact, rounded)
    for m in ["neighbour", "gamma_in_group", "silu_first"] + (["straddle_first"] if straddles else []):
        assert rejected(fn, m, exact, rounded), m


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables: the per-entry fp32 summation bound accepts float32 sums in any order and rejects one missing or foreign pixel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [2, 1, 9, 7, 8])
def test_table_bound_is_sharp(tile):
    B, H, W, C = 3, 130, 16, 128
    x, _, _ = R.gn_draw(B, H * W, C, 32, seed=11)
    tl = R.tiling_for(tile, B, H, W)
    want, mag, cnt = R.qstat_entries(x, tl)
    read = cnt > 0
    crossed = sum(1 for b in range(1, B) if (b * H * W) % tl.bm) if tl.tpi == 0 else 0
    assert int(read.sum()) == want.shape[0] + crossed       # every tile's slot 0 + one slot 1 per image boundary inside a tile
    n = cnt.view(-1, 2, 1, 1)
    # float32 sums in two different orders
    idx, T = tl.entry_of_rows(B, H * W)
    xq = x.reshape(B * H * W, C // 4, 4).numpy().astype(np.float32)
    for order in (np.arange(B * H * W), np.arange(B * H * W)[::-1]):
        tab = np.zeros((T * 2, C // 4, 2), np.float32)
        v = np.stack([xq[order].sum(-1, dtype=np.float32), (xq[order] ** 2).sum(-1, dtype=np.float32)], -1)
        np.add.at(tab, idx.numpy()[order], v)
        ok, worst = R.table_ok(torch.from_numpy(tab).view(T, 2, C // 4, 2), want, mag, n, read)
        assert ok, worst
    # one pixel missing from its entry; one pixel of the next tile counted into it
    for pixel, sign in ((H * W - 1, -1.0), (H * W + 5, -1.0), (2 * H * W, 1.0)):
        bad = want.clone()
        e = int(idx[pixel if sign < 0 else pixel - 1])
        px = x.reshape(B * H * W, C // 4, 4)[pixel]
        bad.view(T * 2, C // 4, 2)[e, :, 0] += sign * px.sum(-1)
        bad.view(T * 2, C // 4, 2)[e, :, 1] += sign * (px * px).sum(-1)
        assert not R.table_ok(bad, want, mag, n, read)[0]
    # rowstats: the same bound over the BN columns of a row
    y = x[0, :70]
    want, mag = R.rowstat_entries(y, 64)
    f32 = np.stack([y.numpy().astype(np.float32).reshape(70, 2, 64).sum(-1, dtype=np.float32),
                    (y.numpy().astype(np.float32).reshape(70, 2, 64) ** 2).sum(-1, dtype=np.float32)], -1)
    assert R.table_ok(torch.from_numpy(f32), want, mag, 64)[0]
    bad = want.clone()
    bad[3, 1, 0] -= y[3, 127]
    bad[3, 1, 1] -= y[3, 127] ** 2
    assert not R.table_ok(bad, want, mag, 64)[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# data about the past: the comparator and the draws of tests/test_gpu_ops.py accept the first three mutants
# ---------------------------------------------------------------------------------------------------------------------------------
def old_close(got, want, rtol=1.2e-2, atol=None):
    """tests/test_gpu_ops.py `close` as it stood when these tests were written"""
    want, got = want.float(), got.float()
    atol = atol if atol is not None else 8e-3 * float(want.abs().max()) + 1e-6
    return not bool((~((got - want).abs() <= atol + rtol * want.abs())).any())


def _old_apply_inputs(B, H, W, C1, C2):
    """test_groupnorm_apply_from_conv_statistics' draws: the bf16 outputs of its two producers, channels-last float64"""
    bf = lambda t: t.to(torch.bfloat16).float()
    g = torch.Generator().manual_seed(31)
    x = bf(torch.randn(B, 64, H, W, generator=g))
    w1 = bf(torch.randn(C1, 64, 3, 3, generator=g) * 0.06)
    b1 = torch.randn(C1, generator=g)
    ys = [bf(F.conv2d(x, w1, b1, padding=1))]
    if C2:
        w2 = bf(torch.randn(C2, 64, 1, 1, generator=g) * 0.2)
        ys.append(bf(F.conv2d(x, w2)))
    gm, bt = torch.randn(C1 + C2, generator=g), torch.randn(C1 + C2, generator=g)
    cl = torch.cat(ys, 1).permute(0, 2, 3, 1).reshape(B, H * W, C1 + C2).to(F64)
    return cl, gm.to(F64), bt.to(F64)


@pytest.mark.parametrize("mutant,shape", [("neighbour", (3, 130, 16, 128, 0)), ("straddle_first", (3, 130, 16, 128, 0)),
                                          ("quad_off", (2, 250, 16, 256, 128))])
def test_old_close_accepted_the_first_three_mutants_on_its_own_inputs(mutant, shape):
    B, H, W, C1, C2 = shape
    x, gm, bt = _old_apply_inputs(*shape)
    tl = [R.Tiling(64, 0, 0), R.Tiling(64, 0, 0)]
    fn = lambda **kw: R.groupnorm(x, gm, bt, 32, 1e-5, 1, C1=C1, tilings=tl, **kw)
    exact, rounded = fn(), fn(rounded=True)
    got = fn(rounded=True, mutant=mutant)
    assert old_close(got, exact, rtol=2e-2), "the old comparator saw this mutant on its own inputs after all"
    # (on these draws all channels share one distribution, so a quad taken from the neighbouring group changes the statistics by less
    #  than the output's rounding and NO comparator can see it: the ladder draws are what makes it visible, see the tests above)
    if mutant != "quad_off":
        assert not R.accepts(got, exact, rounded)             # the floor comparator sees these two even there
