"""GPU parity of the forward normalisations against the float64 restatements of tests/norm_restatement.py, per output tensor, with
the one floor-based comparator `check` (twice the L2 floor, four times the max floor; tests/bwd_restatement.py), at every dispatch
arm: each case asserts the arithmetic that puts it on its arm.  Every strip (image x group, or row) is drawn with its own mean and
scale, and the kernels that read a producer's statistics table get it from an IDENTITY convolution, so that the stored tensor is the
drawn tensor bit for bit and every table entry has an exact float64 expectation.  tests/test_norm_restatement_host.py proves on
the CPU that `check` rejects every listed mutant at exactly these shapes."""
import pytest
import torch

import norm_restatement as R
from norm_restatement import EPS, EPS_BIG, check, check_table

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    return o


def dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV)


def nhwc(x, H, W):
    """[B, HW, C] float64 (bf16-representable) -> bf16 [B, H, W, C] on the device"""
    return x.reshape(x.shape[0], H, W, x.shape[2]).to(torch.bfloat16).to(DEV).contiguous()


def host(y):
    """device [B, H, W, C] -> [B, HW, C] float64"""
    return y.detach().to("cpu").to(F64).reshape(y.shape[0], -1, y.shape[-1])


class launches:
    """the labels of the launches made inside the block"""

    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        self.before, self.ops.PROFILE = self.ops.PROFILE, []
        self.labels = []
        return self

    def __exit__(self, *exc):
        self.labels += [r[0] for r in self.ops.PROFILE]
        self.ops.PROFILE = self.before


def produce(ops, xs, H, W, tile, k, epi=None):
    """identity convolution (centre tap, no bias) over xs [B, HW, C]: the stored tensor IS xs, with the statistics table next to it"""
    C = xs.shape[2]
    pw = ops.pack_conv(R.identity_weight(C, k).to(DEV), None)
    xd = nhwc(xs, H, W)
    y = ops.conv(xd, pw, pad=(k // 2, k // 2), tile=tile, splits=1, qstats=True, epi=epi)
    assert getattr(y, "qstats", None) is not None, "the convolution left no statistics"
    assert torch.equal(y, xd), "the identity producer did not store its input bit for bit"
    want = R.tiling_for(tile, xs.shape[0], H, W)
    assert (y.qstats.bm, y.qstats.tpi) == (want.bm, want.tpi), "QStats tiling differs from the documented one"
    return y


def check_qstats(y, xs, tile, H, W, what):
    """every entry of the table a consumer reads, against the float64 sums, within the any-order fp32 summation bound"""
    tl = R.tiling_for(tile, xs.shape[0], H, W)
    want, mag, cnt = R.qstat_entries(xs, tl)
    assert tuple(y.qstats.table.shape) == tuple(want.shape)
    assert float(cnt.max()) <= 4.0 * R.TILE_ROWS[tile]
    check_table(y.qstats.table, want, mag, cnt.view(-1, 2, 1, 1), what, read=cnt > 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# aldm_groupnorm: every register-strip template from both sides of its boundary, the LDS-cached and the streaming groupnorm_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: f"{c[7]}-HW{c[1]}C{c[2]}s{c[4]}")
def test_groupnorm_arms(ops, case):
    B, HW, C, groups, C1, act, eps, arm = case
    assert R.gn_arm(HW, C, groups) == arm
    assert C1 == C or C1 % (C // groups), "the split of a two-source case falls inside a group"
    x, gm, bt = R.gn_draw(B, HW, C, groups)
    x1 = nhwc(x[..., :C1], HW, 1)
    x2 = nhwc(x[..., C1:], HW, 1) if C1 < C else None
    with launches(ops) as L:
        y = ops.groupnorm(x1, dev(gm), dev(bt), groups, eps, act, x2=x2)
    assert L.labels and L.labels[0].startswith("groupnorm|"), L.labels
    fn = lambda **kw: R.groupnorm(x, gm, bt, groups, eps, act, C1=C1, **kw)
    check(host(y), fn(), fn(rounded=True), f"groupnorm {arm}")


# ---------------------------------------------------------------------------------------------------------------------------------
# aldm_layernorm, aldm_embed_layernorm
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.LN_CS)
def test_layernorm_widths_and_ragged_rows(ops, C):
    assert (C <= 256) == (C in (8, 248, 256))                 # 32 lanes per row up to 256 channels, a whole wave beyond
    for M in R.LN_MS:                                         # 8 (4) rows per workgroup: one row, one short, exact, one over, several
        for eps in (EPS, EPS_BIG):
            x, gm, bt = R.ln_draw(M, C)
            y = ops.layernorm(dev(x, torch.bfloat16), dev(gm), dev(bt), eps)
            fn = lambda **kw: R.layernorm(x, gm, bt, eps, **kw)
            check(y, fn(), fn(rounded=True), f"layernorm C{C} M{M} eps{eps:g}")


@pytest.mark.parametrize("C", R.LN_BAD_CS)
def test_layernorm_rejects_unsupported_widths(ops, C):
    from audioldm_with_lora_amd._lib import AldmError
    x = torch.zeros(4, C, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(AldmError):
        ops.layernorm(x, torch.ones(C, device=DEV), torch.zeros(C, device=DEV))


@pytest.mark.parametrize("case", R.EMBED_CASES, ids=lambda c: f"B{c[0]}L{c[1]}C{c[2]}")
def test_embed_layernorm_position_rule(ops, case):
    B, L, C = case
    ids, word, pos, type0, gm, bt = R.embed_draw(B, L, C)
    assert bool((ids[0, 2:L - 3] == 1).any()) and bool((ids[0, 3:L - 3] != 1).any()) and bool((ids[B - 1] == 1).all())   # pads inside, an all-pad row
    y = ops.embed_layernorm(ids.to(DEV), dev(word), dev(pos), dev(type0), dev(gm), dev(bt), EPS, 1)
    fn = lambda **kw: R.embed_layernorm(ids, word, pos, type0, gm, bt, EPS, 1, **kw)
    check(y, fn(), fn(rounded=True), f"embed_layernorm L{L}")


# ---------------------------------------------------------------------------------------------------------------------------------
# aldm_groupnorm_partials through conv(gn=) and conv(defer=)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["rowmajor", "planar"])
@pytest.mark.parametrize("hw,arm", list(zip(R.PARTIALS_HW, (1, 2, 2, 4, 4, 8, 8))), ids=lambda v: str(v).replace(" ", ""))
def test_groupnorm_over_split_partials(ops, monkeypatch, hw, arm, layout):
    from audioldm_with_lora_amd import _lib
    H, W = hw
    HW, B, C = H * W, 2, 64
    lay = _lib.SLAB_PLANAR if layout == "planar" else _lib.SLAB_ROWMAJOR
    monkeypatch.setattr(ops, "SLAB_LAYOUT", lay)               # conv(gn=) writes the layout its own consumer reads
    assert R.partials_arm(HW, C, 16) == arm == R.partials_arm(HW, 2 * C, 32)
    d = R.partials_draw(H, W)
    xc, skip, bias, rb, res, gm, bt = (d[k] for k in ("xc", "skip", "bias", "rb", "res", "gamma", "beta"))
    pw = ops.pack_conv(R.identity_weight(C, 3).to(DEV), bias.to(DEV))
    xd = nhwc(xc, H, W)
    # (a) two splits, row bias, SiLU
    h = d["h_rowbias"]
    with launches(ops) as L:
        y = ops.conv(xd, pw, pad=(1, 1), rowbias=rb.to(DEV)[:, 8:], rowbias_ld=C + 8, splits=2, gn=(dev(gm[:C]), dev(bt[:C]), 16, EPS, 1))
    assert any(l.startswith("groupnorm_partials") for l in L.labels), L.labels
    fn = lambda **kw: R.groupnorm(h, gm[:C], bt[:C], 16, EPS, 1, **kw)
    check(host(y), fn(), fn(rounded=True), f"partials rowbias S2 {layout}")
    # (b) five splits, residual, the sum kept next to its norm
    h = d["h_res"]
    with launches(ops) as L:
        hk, y = ops.conv(xd, pw, pad=(1, 1), res=nhwc(res, H, W), splits=5, gn=(dev(gm[:C]), dev(bt[:C]), 16, EPS_BIG, 0), gn_keep=True)
    assert any(l.startswith("groupnorm_partials") for l in L.labels), L.labels
    fn = lambda **kw: R.groupnorm(h, gm[:C], bt[:C], 16, EPS_BIG, 0, **kw)
    check(host(y), fn(), fn(rounded=True), f"partials res S5 {layout}")
    check(host(hk), h, R.r16(h), f"partials kept sum {layout}")      # groupnorm_partials_kernel: `o[k] = (bf16)v[i][k]` into sum_out
    # (c) deferred, consumed by the next groupnorm() over cat(h, skip)
    h, hc = d["h_plain"], d["h_cat"]
    df = ops.conv(xd, pw, pad=(1, 1), splits=(5 if arm in (2, 8) else 2), defer=(2 * C, 32), slab_layout=lay)
    assert isinstance(df, ops.Deferred) and df.eff > 1 and df.layout == lay
    y = ops.groupnorm(df, dev(gm), dev(bt), 32, EPS_BIG, 1, x2=nhwc(skip, H, W))
    fn = lambda **kw: R.groupnorm(hc, gm, bt, 32, EPS_BIG, 1, C1=C, **kw)
    check(host(y), fn(), fn(rounded=True), f"partials deferred x2 {layout}")
    check(host(ops.tensor_of(df)), h, R.r16(h), f"partials deferred sum {layout}")


# ---------------------------------------------------------------------------------------------------------------------------------
# aldm_groupnorm_apply over identity producers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.APPLY_CASES, ids=lambda c: c[0])
def test_groupnorm_apply_from_identity_producers(ops, case):
    name, B, H, W, C1, C2, groups, t1, t2, act, eps = case
    HW, C = H * W, C1 + C2
    x, gm, bt, tilings = R.apply_draw(case)
    # the arithmetic that puts the case on its arm
    assert HW >= ops.QSTATS_MIN_HW
    arm = dict(straddle=lambda: HW % 64 and B > 2, halo7=lambda: tilings[0].tpi > 0 and HW % tilings[0].pix, halo8=lambda: tilings[0].tpi > 0,
               concat=lambda: C1 % (C // groups), tiles95=lambda: R.apply_tiles(HW, tilings) == ops.GN_FINALIZE_MIN_TILES - 1,
               tiles96=lambda: R.apply_tiles(HW, tilings) == ops.GN_FINALIZE_MIN_TILES,
               tiles95x2=lambda: R.apply_tiles(HW, tilings) == 95 and C2, tiles96x2=lambda: R.apply_tiles(HW, tilings) == 96 and C2,
               g64=lambda: R.apply_lpg(groups) == 4, g1=lambda: R.apply_lpg(groups) == 64 and R.apply_pxb(C) == 256 and HW % 256,
               c2048=lambda: R.apply_pxb(C) == 16 and HW % 16 and C // 8 == 256)[name]
    assert arm(), name
    assert {R.apply_lpg(g_) for g_ in (64, 32, 8, 1)} == {4, 8, 32, 64}
    k1 = 1 if name == "c2048" else 3
    y1 = produce(ops, x[..., :C1].contiguous(), H, W, t1, k1)
    check_qstats(y1, x[..., :C1].contiguous(), t1, H, W, f"qstats {name} src1")
    y2 = None
    if C2:
        y2 = produce(ops, x[..., C1:].contiguous(), H, W, t2, 1)
        check_qstats(y2, x[..., C1:].contiguous(), t2, H, W, f"qstats {name} src2")
    with launches(ops) as L:
        got = ops.groupnorm(y1, dev(gm), dev(bt), groups, eps, act, x2=y2)
    assert L.labels and L.labels[0].startswith("groupnorm_apply"), L.labels
    fn = lambda **kw: R.groupnorm(x, gm, bt, groups, eps, act, C1=C1, **kw)
    check(host(got), fn(), fn(rounded=True), f"groupnorm_apply {name}")


@pytest.mark.parametrize("tile", R.RANDOM_PRODUCER_TILES)
def test_groupnorm_apply_from_random_weight_producer(ops, tile):
    """One random-weight producer per tile family: the reference is the float64 GroupNorm of the STORED bf16 tensor, and the table is
    checked against the float64 sums of that tensor."""
    d = R.random_producer_draw()
    B, H, W, groups, gm, bt = d["B"], d["H"], d["W"], d["groups"], d["gamma"], d["beta"]
    pw = ops.pack_conv(dev(d["w"], torch.bfloat16), d["bias"].to(DEV))
    y1 = ops.conv(nhwc(d["xin"], H, W), pw, pad=(1, 1), tile=tile, splits=1, qstats=True)
    stored = host(y1)
    check(stored, R.conv3x3(d["xin"], H, W, d["w"], d["bias"].to(F64)), R.r16(R.conv3x3(d["xin"], H, W, d["w"], d["bias"].to(F64))),
          f"random producer tile {tile} output")
    check_qstats(y1, stored, tile, H, W, f"qstats random producer tile {tile}")
    got = ops.groupnorm(y1, dev(gm), dev(bt), groups, EPS, 1)
    fn = lambda **kw: R.groupnorm(stored, gm, bt, groups, EPS, 1, **kw)
    check(host(got), fn(), fn(rounded=True), f"groupnorm_apply random producer tile {tile}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the other consumers of a producer's table
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptile", R.CONSUMER_PTILES)
def test_gn_silu_conv_out_from_identity_producer(ops, ptile):
    d = R.consumer_draw()
    H, W, groups, x, gm, bt, w, b = (d[k] for k in ("H", "W", "groups", "x", "gamma", "beta", "w8", "b8"))
    y1 = produce(ops, x, H, W, ptile, 3)
    pw = ops.pack_conv(w.to(DEV), b.to(DEV))
    assert ops.gn_silu_conv_out_ok(y1, pw, groups)
    got = ops.gn_silu_conv_out(y1, dev(gm), dev(bt), groups, EPS, pw)
    assert got.dtype == torch.float32
    fn = lambda **kw: R.gn_conv(x, gm, bt, groups, EPS, H, W, w, b.to(F64), out_bf16=False, **kw)
    check(host(got), fn(), fn(rounded=True), f"gn_silu_conv_out producer tile {ptile}")


@pytest.mark.parametrize("tile", [7, 8, 15, 16])
@pytest.mark.parametrize("ptile", R.CONSUMER_PTILES)
def test_conv_applies_groupnorm_of_identity_producer(ops, ptile, tile):
    d = R.consumer_draw()
    H, W, groups, N, x, gm, bt, w, b, rb, res = (d[k] for k in ("H", "W", "groups", "N", "x", "gamma", "beta", "w", "b", "rb", "res"))
    y1 = produce(ops, x, H, W, ptile, 3)
    pw = ops.pack_conv(w.to(DEV), b.to(DEV))
    assert ops.gn_in_ok(y1, None, pw)
    with launches(ops) as L:
        got = ops.conv(y1, pw, pad=(1, 1), gn_in=(dev(gm), dev(bt), groups, EPS, 1), tile=tile, rowbias=rb.to(DEV), rowbias_ld=N,
                       res=nhwc(res, H, W))
    assert L.labels and L.labels[0].startswith(f"igemm_{ops.TILE_NAMES[tile]}_r"), L.labels
    fn = lambda **kw: R.gn_conv(x, gm, bt, groups, EPS, H, W, w, b.to(F64), d["extra"], **kw)
    check(host(got), fn(), fn(rounded=True), f"conv gn_in tile {tile} producer tile {ptile}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables themselves: every tile family that conv() lets produce them, both epilogue forms
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["lds", "auto"])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 6, 9, 10, 11, 12, 13, 14, 7, 8, 15, 16])
def test_qstat_table_entries(ops, monkeypatch, tile, epi):
    from audioldm_with_lora_amd import _lib
    B, H, W, C = 3, 130, 16, 128
    x, _, _ = R.gn_draw(B, H * W, C, 32, seed=11)             # one group per quad: every entry has its own mean and scale
    trace = []
    monkeypatch.setattr(ops, "EPI_TRACE", trace)
    y = produce(ops, x, H, W, tile, 3, epi=(_lib.EPI_LDS if epi == "lds" else _lib.EPI_AUTO))
    assert trace == [0 if (epi == "lds" or tile in (1, 9, 12)) else 1], "the epilogue form this case is there for"
    check_qstats(y, x, tile, H, W, f"qstats tile {tile} {epi}")


@pytest.mark.parametrize("route,tile,K", [("igemm", 2, 128), ("igemm", 1, 128), ("igemm", 3, 128), ("igemm", 4, 128), ("igemm", 6, 128),
                                            ("igemm", 9, 128), ("igemm", 10, 128), ("igemm", 11, 128), ("igemm", 12, 128), ("igemm", 13, 128), ("igemm", 14, 128),
                                            ("pgemm", 0, 256), ("pgemm", 0, 640)])
def test_rowstat_table_entries(ops, route, tile, K):
    M = 130
    x, _, _ = R.ln_draw(M, K)
    xd = dev(x, torch.bfloat16)
    with launches(ops) as L:
        y, stats = ops.linear(xd, ops.pack_linear(torch.eye(K, device=DEV), None), rowstats=True, tile=tile)
    assert L.labels and L.labels[0].startswith(route), L.labels
    assert torch.equal(y, xd)
    BN = K // stats.shape[1]
    assert route == "pgemm" or BN == ops.TILE_DIMS[tile][1]
    want, mag = R.rowstat_entries(x, BN)
    check_table(stats, want, mag, BN, f"rowstats {route} tile {tile} K{K}")


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm folded into the GEMMs and the attention blocks
# ---------------------------------------------------------------------------------------------------------------------------------
def pack_ln(ops, W, bias, gm, bt, eps, parts):
    pw = ops.pack_linear_ln(dev(W), None if bias is None else dev(bias), dev(gm), dev(bt), eps)
    if parts:
        ops.attach_lora(pw, [(r0, nr, A.to(DEV), Bm.to(DEV), s) for r0, nr, A, Bm, s in parts])
    return pw


@pytest.mark.parametrize("eps", [EPS, EPS_BIG])
@pytest.mark.parametrize("case", R.LNLIN_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_layernorm_folded_into_gemm_on_ladder_rows(ops, case, eps):
    route, M, K, N, r = case
    assert M % 64 and M % 16                                  # ragged against every tile
    x, W, bias, gm, bt, parts = R.ln_linear_draw(M, K, N, r)
    pw = pack_ln(ops, W, bias, gm, bt, eps, parts)
    xd = dev(x, torch.bfloat16)
    kw = {}
    if route != "igemm_own":                                  # the statistics come from a producer's rowstat table
        _, stats = ops.linear(xd, ops.pack_linear(torch.eye(K, device=DEV), None), rowstats=True)
        kw = dict(ln_parts=stats)
    with launches(ops) as L:
        if route == "pgemm_vt":                               # columns >= 2 K leave token-major, as the attention kernel reads V^T
            Bt, Nt = 2, M // 2
            npad = (Nt + 7) // 8 * 8
            vt = torch.zeros(Bt, K, npad, dtype=torch.bfloat16, device=DEV)
            qk = ops.conv(xd.view(Bt, 1, Nt, K), pw, vt=vt, vt_col0=2 * K, vt_ld=npad, vt_batch_stride=K * npad, **kw)
            got = torch.cat([qk.view(M, 2 * K), vt[:, :, :Nt].permute(0, 2, 1).reshape(M, K)], 1)
        else:
            got = ops.linear(xd, pw, **kw)
    assert L.labels and L.labels[0].startswith("pgemm" if route == "pgemm_vt" else "igemm"), L.labels
    fn = lambda **k_: R.ln_linear(x, W, bias, gm, bt, eps, parts, **k_)
    check(got, fn(), fn(rounded=True), f"ln_linear {route} M{M} K{K} eps{eps:g}")


def slab_parts(xd, M, C):
    """row partials as a producer epilogue leaves them: [M][C / 64][2] = (sum, sum of squares) per 64-column slab"""
    xs = xd.float().view(M, C // 64, 64)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).contiguous()


@pytest.mark.parametrize("kind,N", [(64, n) for n in R.ATTN64_NS] + [(256, n) for n in R.ATTN256_NS])
def test_attn_block_on_ladder_rows(ops, monkeypatch, kind, N):
    H, d, B = 8, (80 if kind == 64 else 48), 2
    C = H * d
    x, W, _, gm, bt, parts = R.ln_linear_draw(B * N, C, 3 * C, 4)
    pw = pack_ln(ops, W, None, gm, bt, EPS, parts)
    xd = dev(x, torch.bfloat16)
    lp = slab_parts(xd, B * N, C)
    monkeypatch.setattr(ops, "ATTN_BLOCK256", True)
    assert ops.attn_block_ok(pw, N, H, d, lp) == kind
    got = ops.attn_block(xd, pw, lp, B, N, H, d)
    exact = R.attn_block(x, W, gm, bt, EPS, parts, B, N, H, d)
    rounded = R.attn_block(x, W, gm, bt, EPS, parts, B, N, H, d, rounded=True)
    check(got, exact, rounded, f"attn_block{kind} N{N}")
