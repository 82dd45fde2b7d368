"""The forward 2-D forms of ops.conv (csrc/igemm_core.h, igemm_halo.hip, igemm_ws.hip, the igemm_t*.hip instantiations behind the dispatcher in
igemm.hip) against the float64 restatement of tests/conv_restatement.py, per element, under a bound made of the number formats alone
(`b32 = (n + 1) 2^-24 mag`, plus one bf16 half-ulp for a bf16 output), and for bf16 outputs also under the floor rule of
tests/bwd_restatement.py.  tests/test_conv_restatement_host.py proves on the CPU that the bound rejects the listed mutants at exactly
these shapes.

Every launch names tile=, ring= and splits=, so neither the tuned table nor the heuristics play a part; every case asserts the arithmetic
that puts it on its arm; every input is a contiguous slice out of the middle of a NaN-filled arena with an image of guard on each side;
every output goes into a NaN-filled buffer with out_ld = N + 8 and a guard image behind the last one, which must still be NaN afterwards;
every case runs with an fp32 and with a bf16 output; the bf16 run records ops.EPI_TRACE and asserts the epilogue form the host rule
gives (register-direct or LDS walk), and a direct launch is repeated under the LDS walk and must come out bit-equal.

A. generic tiles x geometry   B. halo tiles at their capacity edges   C. split-K (the plan_splits rule)   D. epilogue forms.
Not here (covered elsewhere): gn= / defer= / gn_in= / qstats (test_gpu_norm_edges.py), LoRA / V^T / GEGLU / folded LayerNorm
(test_gpu_pgemm.py, test_gpu_multi_adapter.py), 1-D and transposed convolutions (test_gpu_vocoder_edges.py)."""
import ctypes
from functools import lru_cache

import pytest
import torch

import conv_restatement as R
from bwd_restatement import F64

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GENERIC_ANY = (1, 2, 3, 4)                                       # reg_staged rows of IGEMM_TILES: any input
GENERIC_DMA = (6, 9, 10, 11, 12, 13, 14)                         # LDS-DMA path only: every source a multiple of 64 channels, no gather activation


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    return o


WORST = {}


@pytest.fixture(autouse=True)
def _record_worst():
    """One log line per kind of output (`what`) and test: the largest ratio to the bound / to the floor (DESIGN.md's tables)."""
    WORST.clear()
    yield
    import conftest
    for what, v in sorted(WORST.items()):
        conftest.record(v, what)


def _note(v, what):
    WORST[what] = max(WORST.get(what, 0.0), v)


# ---------------------------------------------------------------------------------------------------------------------------------
# arenas, the launch, the guards
# ---------------------------------------------------------------------------------------------------------------------------------
def arena(t, dtype=torch.bfloat16):
    """[B, ...] float64 -> the contiguous slice [1 : B + 1] of a NaN-filled device arena with one item of guard on each side."""
    a = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), NAN, dtype=dtype)
    a[1:-1] = t.to(dtype)
    s = a.to(DEV)[1:-1]
    assert s.is_contiguous()
    return s


def rows_arena(t, ld, ps, po):
    """[B, OH, OW, N] -> [B, OH * OW * ps, ld] laid out like the output (row pix * ps + po, columns 0 .. N - 1), NaN everywhere else."""
    B, OH, OW, N = t.shape
    a = torch.full((B, OH * OW * ps, ld), NAN, dtype=F64)
    a[:, po::ps, :N] = t.reshape(B, OH * OW, N)
    return arena(a)


@lru_cache(maxsize=None)
def pack(c):
    from audioldm_with_lora_amd import ops
    t = R.draw(c)
    w, b = t["w"].float().to(DEV), (t["bias"].float().to(DEV) if t["bias"] is not None else None)
    if t["w_sc"] is not None:
        return ops.pack_conv_shortcut(w, b, t["w_sc"].float()[:, :, None, None].to(DEV), torch.zeros_like(b))
    return ops.pack_conv(w, b)


def direct_expected(c, tile, eff, f32, rb_ld, ld, obs):
    """The host rule of the register-direct epilogue (igemm.hip epilogue_direct), restated."""
    d = dict(c)
    OH, OW = R.out_hw(c)
    fast = d["C1"] % 64 == 0 and d["C2"] % 64 == 0 and not d["in_act"]
    plain = d["out_act"] is None and d["post_act"] is None and not d["out2"] and not d["res2"] and not f32
    rb_ok = not d["rowbias"] or (rb_ld % 4 == 0 and (tile in R.HALO or OH * OW >= R.TILE_BM[tile]))
    return int(fast and eff <= 1 and plain and d["N"] % 8 == 0 and ld % 4 == 0 and obs % 4 == 0 and rb_ok and tile not in R.NO_DIRECT)


def lib_eff_splits(ops, c, tile, want):
    d = dict(c)
    a = ops._lib.IgemmArgs()
    a.KH, a.KW = d["k"]
    a.Cin, a.Cin2, a.Cin3, a.Cin4, a.splits, a.tile = d["C1"], d["C2"], d["C3"], d["C4"], want, tile
    a.x3, a.x4 = (1 if d["C3"] else None), (1 if d["C4"] else None)           # (only tested for null)
    return ops._lib.load().aldm_igemm_effective_splits(ctypes.byref(a))


def launch(ops, c, tile, ring, splits, f32, rb_pad=0, pix=(1, 0), epi=None, trace=None):
    """One ops.conv launch of case c -> (out [B, OH, OW, N] float64, out2 or None, the raw output buffer, the traced epilogue form)."""
    d, t = dict(c), R.draw(c)
    B, N = d["B"], d["N"]
    OH, OW = R.out_hw(c)
    ld, (ps, po) = N + 8, pix
    rows = OH * OW * ps
    dt = torch.float32 if f32 else torch.bfloat16
    buf = torch.full((B + 1, rows, ld), NAN, dtype=dt, device=DEV)
    buf2 = torch.full((B + 1, rows, ld), NAN, dtype=torch.bfloat16, device=DEV) if d["out2"] else None
    acts = {None: ops.ACT_NONE, "silu": ops.ACT_SILU, "lrelu": ops.ACT_LRELU}
    kw = dict(stride=d["stride"], pad=d["pad"], dil=d["dil"], up_size=d["up"], alpha=d["alpha"], out_act=acts[d["out_act"]], out_slope=0.1,
              post_act=acts[d["post_act"]], post_slope=0.1, out=buf[:B], out_ld=ld, out_batch_stride=rows * ld, out_pix_stride=ps,
              out_pix_offset=po, tile=tile, ring=ring, splits=splits, epi=epi)
    if d["in_act"]:
        kw.update(in_act=ops.ACT_LRELU, in_slope=R.IN_SLOPE)
    for k in ("x2", "x3", "x4"):
        if t[k] is not None:
            kw[k] = arena(t[k])
    for k in ("res", "res2"):
        if t[k] is not None:
            kw[k] = rows_arena(t[k], ld, ps, po)
    if t["rowbias"] is not None:
        rb = torch.full((B, N + rb_pad), NAN, dtype=F64)
        rb[:, :N] = t["rowbias"]
        kw.update(rowbias=arena(rb, torch.float32), rowbias_ld=N + rb_pad)
    if buf2 is not None:
        kw["out2"] = buf2[:B]
    n0 = len(trace) if trace is not None else 0
    ops.conv(arena(t["x"]), pack(c), **kw)
    torch.cuda.synchronize()
    form = None
    if trace is not None:
        assert len(trace) == n0 + 1
        form = trace[-1]
    outs = []
    for b_ in (buf, buf2):
        if b_ is None:
            outs.append(None)
            continue
        h = b_.cpu()
        nan = torch.isnan(h)
        assert bool(nan[B].all()), f"{d['name']}: the guard image behind the output was written"
        assert bool(nan[:B, :, N:].all()), f"{d['name']}: columns N .. out_ld - 1 were written"
        if ps > 1:                                                   # the other phase, bit for bit what it was
            other = torch.ones(rows, dtype=torch.bool)
            other[po::ps] = False
            fill = torch.full((1,), NAN, dtype=h.dtype)
            iv = torch.int32 if h.dtype == torch.float32 else torch.int16
            assert bool((h[:B][:, other].view(iv) == fill.view(iv)).all()), f"{d['name']}: rows of the other output phase were written"
        outs.append(h[:B, po::ps, :N].reshape(B, OH, OW, N).to(F64))
    return outs[0], outs[1], buf, form


def run_case(ops, monkeypatch, c, tile, ring, splits, what, forms=None, **kw):
    """fp32 output against the fp32 bound, bf16 output against the bf16 bound and the floor rule; the bf16 run's epilogue form is asserted
    against the host rule, and a register-direct launch is repeated under the LDS walk, bit-equal."""
    d = dict(c)
    ref = R.cached_reference(c)
    where = f"{what} [{d['name']} tile {tile} ring {ring} splits {splits}]"
    eff = lib_eff_splits(ops, c, tile, splits)
    assert eff == R.eff_splits(c, tile, splits), (where, eff)
    trace = []
    monkeypatch.setattr(ops, "EPI_TRACE", trace)
    got, got2, _, form = launch(ops, c, tile, ring, splits, True, trace=trace, **kw)
    assert form == 0, where                                          # an fp32 output always walks the LDS image
    R.check_elem(got, ref, what + " f32", True, record=_note)
    if got2 is not None:
        R.check_both(got2, ref, what + " out2 (beside f32)", False, True, record=_note)
    got, got2, buf, form = launch(ops, c, tile, ring, splits, False, trace=trace, **kw)
    OH, OW = R.out_hw(c)
    ld, ps = d["N"] + 8, kw.get("pix", (1, 0))[0]
    want_form = direct_expected(c, tile, eff, False, d["N"] + kw.get("rb_pad", 0), ld, OH * OW * ps * ld)
    assert form == want_form, (where, form, want_form)
    try:
        R.check_both(got, ref, what + " bf16", False, record=_note)
        if got2 is not None:
            R.check_both(got2, ref, what + " out2", False, True, record=_note)
    except AssertionError as err:
        raise AssertionError(f"{where}: {err}") from None
    if form == 1:
        _, _, buf_lds, form_lds = launch(ops, c, tile, ring, splits, False, epi=ops._lib.EPI_LDS, trace=trace, **kw)
        assert form_lds == 0
        assert torch.equal(buf.view(torch.int16), buf_lds.view(torch.int16)), f"{where}: the direct epilogue differs from the LDS walk"
    if forms is not None:
        forms.add(form)


def generic_ok(c, tile):
    d = dict(c)
    return tile in GENERIC_ANY or (d["C1"] % 64 == 0 and d["C2"] % 64 == 0 and not d["in_act"])


# ---------------------------------------------------------------------------------------------------------------------------------
# A. generic tiles x geometry
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 6, 9, 10, 11, 12, 13, 14])
def test_generic_tile_channel_edges(ops, monkeypatch, tile):
    """Three images of 11 x 7 (M = 231: less than a 256-row tile, ragged under 64 and 128, tiles over both image boundaries) at the channel
    edges: 8 -> 136, 72 -> 40 (the generic gather: K-tiles straddle taps), 64 -> 72 (with and without a row bias), 128 + 64 -> 136 (two
    sources), 64 -> 8."""
    bm, forms, ran = R.TILE_BM[tile], set(), 0
    for c in R.A_BASE:
        d = dict(c)
        M = d["B"] * 77
        assert R.out_hw(c) == (11, 7) and M == 231 and M % bm != 0 and R.straddles(c, bm)
        assert (9 * d["C1"]) % 64 != 0 or d["C1"] % 64 == 0          # 72: a K-tile holds parts of two taps; 8: one ragged K-tile after the first
        if not generic_ok(c, tile):
            assert tile in GENERIC_DMA and d["C1"] in (8, 72)
            continue
        run_case(ops, monkeypatch, c, tile, 2 if tile in (6, 9) else 3, 1, f"A tile {tile}", forms)
        ran += 1
    assert ran == (6 if tile in GENERIC_ANY else 4)
    # the register-direct epilogue was seen on every tile that has it (and run_case repeated those launches under the LDS walk); the LDS
    # walk as dispatched on every tile that meets a gather-path input or, at 128 / 256 rows, a row bias with 77 pixels an image
    assert (1 in forms) == (tile not in R.NO_DIRECT) and (0 in forms) == (tile in GENERIC_ANY or bm > 64)


@pytest.mark.parametrize("tile", [9, 12])
def test_generic_256_row_tiles(ops, monkeypatch, tile):
    for c in R.A_BIG:
        M = dict(c)["B"] * 37 * 7
        assert M == 518 and M > 2 * 256 and M % 256 == 6 and R.straddles(c, 256)      # two whole tiles, a 6-row tail, image boundary at row 259
        run_case(ops, monkeypatch, c, tile, 2 if tile == 9 else 3, 1, f"A tile {tile}")


@pytest.mark.parametrize("c", R.A_GEOM, ids=lambda c: dict(c)["name"].replace(" ", "_"))
def test_generic_geometries(ops, monkeypatch, c):
    """stride 2 on odd and even extents, 1x1, dilation (2, 1), nearest up-sampling to exact 2x and to two other sizes (two sources): on
    tile 2 and on one tile of each LDS-DMA family (8-wave, loader-wave)."""
    d = dict(c)
    OH, OW = R.out_hw(c)
    if d["stride"] == (2, 2):
        assert (OH, OW) == (6, 4) and ((d["IH"] % 2, d["IW"] % 2) in ((1, 1), (0, 0)))
    if d["up"] is not None:
        assert (OH, OW) == d["up"] and d["C2"] == 64 and (d["up"] == (2 * d["IH"], 2 * d["IW"])) == (d["IH"] == 8)
    for tile in (2, 10, 14):
        assert generic_ok(c, tile) and ((d["B"] * OH * OW) % R.TILE_BM[tile] != 0) == (d["up"] != (16, 8))   # (two images of 16 x 8: whole tiles)
        run_case(ops, monkeypatch, c, tile, 3, 1, "A geometry")


# ---------------------------------------------------------------------------------------------------------------------------------
# B. halo tiles
# ---------------------------------------------------------------------------------------------------------------------------------
def halo_cap(ops, tile):
    return ops.HALO_ROWS[tile]


@pytest.mark.parametrize("tile", R.HALO)
def test_halo_capacity_edges(ops, monkeypatch, tile):
    """Every output width the tile takes: three and five DMA passes on the 128-row tiles (180 / 204 / 264 halo rows against 192 and 320),
    108 and 100 rows against 128 on the 64-row tiles; image heights with 0, 1 and rows_pt - 1 rows in the last tile; one, two
    (virtual concat) and three 64-channel chunks; every ring depth the launcher has."""
    bm, passes, chans, rings, forms = R.TILE_BM[tile], set(), set(), set(), set()
    for c, ring in R.b_cases(tile):
        d = dict(c)
        OH, OW = R.out_hw(c)
        need = R.halo_need(tile, OW)
        assert tile in ops.halo_tiles(OW, True) and bm % OW == 0 and need <= halo_cap(ops, tile)
        assert OH % (bm // OW) in (0, 1, bm // OW - 1)
        passes.add(5 if need > 192 else 3 if bm == 128 else 2)
        chans.add((d["C1"], d["C2"]))
        rings.add(ring)
        run_case(ops, monkeypatch, c, tile, ring, 1, f"B tile {tile}", forms)
    assert passes == ({3, 5} if bm == 128 else {2}) and chans == set(R.B_CH) and rings == set(R.B_RINGS[tile])
    run_case(ops, monkeypatch, R.B_ACT, tile, 3, 1, f"B silu tile {tile}", forms)
    assert forms == {0, 1}                                           # register-direct (bias + row bias + res) and the LDS walk (SiLU) as dispatched


@pytest.mark.parametrize("tile", R.HALO)
def test_halo_upsampling_sizes(ops, monkeypatch, tile):
    for c in R.B_UP:
        OH, OW = R.out_hw(c)
        assert OW in (8, 16) and tile in ops.halo_tiles(OW, True)
        run_case(ops, monkeypatch, c, tile, 3, 1, f"B up tile {tile}")


@pytest.mark.parametrize("tile", [15, 16])
def test_halo_fused_shortcut(ops, monkeypatch, tile):
    """conv2 + conv_shortcut as one GEMM (pack_conv_shortcut, x3 | x4 over the output pixels): C3 = 64 and C3 + C4 = 64 + 128."""
    for c in R.B_SHORTCUT:
        d = dict(c)
        OH, OW = R.out_hw(c)
        assert R.halo_need(tile, OW) <= (192 if tile == 15 else 128) and d["C3"] == 64 and d["C4"] in (0, 128)
        assert pack(c).Cext == d["C3"] + d["C4"] and R.nkt_of(c) == 9 + (d["C3"] + d["C4"]) // 64
        run_case(ops, monkeypatch, c, tile, 3, 1, f"B shortcut tile {tile}")


def ws_admits(c, tile):
    """`same` of select_halo (igemm_select.hip) for the wave-specialised tiles (no segment, no up-sampling): odd filter, 2 pad = (K - 1) dil, stride 1."""
    d = dict(c)
    (KH, KW), (ph, pw), (dh, dw) = d["k"], d["pad"], d["dil"]
    return KH % 2 == 1 and KW % 2 == 1 and 2 * ph == (KH - 1) * dh and 2 * pw == (KW - 1) * dw and d["stride"] == (1, 1)


@pytest.mark.parametrize("tile", [15, 16])
def test_halo_general_filters(ops, monkeypatch, tile):
    """The general-filter form of the wave-specialised halo tiles as a 2-D launch: exactly the forms the launcher admits (5x5 / pad 2,
    3x1 / pad (1, 0), 3x3 with dilation (2, 1) / pad (2, 1)) where the halo (BM / OW + (KH - 1) dh)(OW + (KW - 1) dw) fits."""
    ran = []
    for c in R.B_FILTER:
        d = dict(c)
        OH, OW = R.out_hw(c)
        assert ws_admits(c, tile) and (OH, OW) == (d["IH"], d["IW"])
        if R.halo_need(tile, OW, d["k"], d["dil"]) > halo_cap(ops, tile):
            assert tile == 16 and d["k"] == (5, 5)                   # 12 x 12 = 144 halo rows against 128
            continue
        run_case(ops, monkeypatch, c, tile, 3, 1, f"B filter tile {tile}")
        ran.append(d["name"])
    assert len(ran) == (4 if tile == 15 else 3)


@pytest.mark.parametrize("tile,c", R.B_REFUSED, ids=lambda v: dict(v)["name"].replace(" ", "_") if isinstance(v, tuple) else str(v))
def test_halo_refuses_what_does_not_fit(ops, tile, c):
    d = dict(c)
    OH, OW = R.out_hw(c)
    over = R.halo_need(tile, OW, d["k"], d["dil"]) > halo_cap(ops, tile)
    assert over or (tile in (7, 8) and d["dil"] != (1, 1))           # 136 / 144 halo rows against 128; the eight-wave halo tiles: 3x3 without dilation only
    if d["k"] == (3, 3) and d["dil"] == (1, 1):
        assert tile not in ops.halo_tiles(OW, True)
    with pytest.raises(ops._lib.AldmError):
        launch(ops, c, tile, 3, 1, False)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. split-K
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [2, 3, 13, 14])
def test_splitk_generic(ops, monkeypatch, tile):
    """nkt = 9: an effective count below the request (4 -> 3, 7 -> 5, 12 -> 9) and a one-K-tile tail (5: 2 + 2 + 2 + 2 + 1); bias + row
    bias + res through the reduce, N = 72 and 136."""
    for c in R.C_GENERIC:
        assert R.nkt_of(c) == 9
        assert [R.eff_splits(c, tile, s) for s in R.C_SPLITS] == [2, 3, 5, 5, 9, 9]
        for s in R.C_SPLITS:
            run_case(ops, monkeypatch, c, tile, 3, s, f"C tile {tile}")


def test_splitk_zero_padded_tail_ktile(ops, monkeypatch):
    """Cin = 72: K = 648 = 10 K-tiles + 8 elements; the last split's last K-tile is mostly padding."""
    for c in R.C_TAIL:
        assert R.nkt_of(c) == 11 and pack(c).Kpad == 704
        for s, eff in ((2, 2), (4, 4), (11, 11)):
            assert R.eff_splits(c, 2, s) == eff
            run_case(ops, monkeypatch, c, 2, 3, s, "C tail K-tile")


@pytest.mark.parametrize("tile", R.HALO)
def test_splitk_halo_by_chunks(ops, monkeypatch, tile):
    """Halo tiles split by whole 64-channel chunks: 3 chunks -> 2 + 1 and 1 + 1 + 1, 4 chunks asked 3 -> 2 + 2, more splits than chunks."""
    effs = {}
    for c in R.C_HALO:
        nch = (dict(c)["C1"] + dict(c)["C2"]) // 64
        for s in R.C_HALO_SPLITS:
            effs[(nch, s)] = R.eff_splits(c, tile, s)
            run_case(ops, monkeypatch, c, tile, 3, s, f"C halo tile {tile}")
    assert [effs[(3, s)] for s in R.C_HALO_SPLITS] == [2, 3, 3, 3] and [effs[(4, s)] for s in R.C_HALO_SPLITS] == [2, 2, 4, 4]


def test_splitk_fused_shortcut_segment(ops, monkeypatch):
    for c in R.C_SHORTCUT:
        d = dict(c)
        assert R.nkt_of(c) == 18 + (d["C3"] + d["C4"]) // 64
        for s in (2, 3):
            assert R.eff_splits(c, 16, s) == 2                        # two main chunks: at most two splits, each with its share of the segment
            run_case(ops, monkeypatch, c, 16, 3, s, "C shortcut segment")


# ---------------------------------------------------------------------------------------------------------------------------------
# D. epilogue forms
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [40, 72])
@pytest.mark.parametrize("tile", [2, 14, 16])
def test_epilogue_forms(ops, monkeypatch, tile, N):
    """Row bias with fewer and with at least BM pixels per image, res / res2 / alpha, out_act SiLU and leaky, out2 with and without post_act,
    at N = 40 and 72 (quads without whole 16-column blocks)."""
    forms, below = set(), set()
    for what, c in R.d_cases(tile, N):
        OH, OW = R.out_hw(c)
        below.add(OH * OW < R.TILE_BM[tile])
        assert tile != 16 or tile in ops.halo_tiles(OW, True)
        run_case(ops, monkeypatch, c, tile, 3, 1, f"D {what}", forms)
    assert below == {False, True} and forms == {0, 1}


@pytest.mark.parametrize("tile", [2, 14, 16])
def test_rowbias_stride_and_output_phase(ops, monkeypatch, tile):
    """rowbias_ld = N + 4, and out_pix_stride = 2 / out_pix_offset = 1 into a pre-filled buffer whose other phase stays as it was."""
    (_, small), (_, big) = [(w, c) for w, c in R.d_cases(tile, 72) if w == "rowbias"]
    for c in (small, big):
        run_case(ops, monkeypatch, c, tile, 3, 1, "D rowbias_ld N + 4", rb_pad=4)
        run_case(ops, monkeypatch, c, tile, 3, 1, "D rowbias_ld N + 2", rb_pad=2)      # no 16-byte row bias loads
    res = [c for w, c in R.d_cases(tile, 72) if w == "res res2 alpha"]
    for c in res:
        run_case(ops, monkeypatch, c, tile, 3, 1, "D output phase", pix=(2, 1))
    run_case(ops, monkeypatch, big, tile, 3, 1, "D output phase", pix=(2, 1))


@pytest.mark.parametrize("tile", GENERIC_ANY)
def test_input_activation_on_the_gather_path(ops, monkeypatch, tile):
    """in_act (leaky, slope 2^-2: the activated input stays bf16-representable) leaves the LDS-DMA path: tiles 1 - 4 only."""
    for c in R.D_IN_ACT:
        run_case(ops, monkeypatch, c, tile, 3, 1, "D in_act")
    with pytest.raises(ops._lib.AldmError):
        launch(ops, R.D_IN_ACT[0], 14, 3, 1, False)
