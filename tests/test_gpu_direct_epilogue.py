"""GPU: the register-direct standard epilogue of the implicit-GEMM family (igemm_epilogue_direct) against the LDS walk it replaces.

The same operands go through both forms (ops.conv(epi=EPI_LDS / EPI_DIRECT)).  EPI_DIRECT is an error for a launch that cannot take the
direct form, and every case also reads aldm_igemm_epilogue_form through ops.EPI_TRACE, so a case cannot pass by running the LDS walk twice.
  * `out` must be bit-identical (the direct form applies the same operations in the same order per element);
  * the GroupNorm hand-over table (qstat_out) is compared with a float64 sum of the stored bf16 values: every entry's error under the direct
    form is at most twice the LDS walk's largest error on the same case (per image slot and per sum | sum of squares), or 8 fp32 ulps of
    the entry if that is larger -- an entry-by-entry comparison of two rounding patterns would fail wherever the LDS walk happens to be
    exact;
  * launches the direct form does not take are run with EPI_AUTO, must report the LDS walk and come out bit-equal to the forced LDS walk
    (and, where they carry a table, a correct one): activation, out2 with and without activation, res2, fp32 output, V^T, GEGLU, LayerNorm
    row statistics, the folded LayerNorm, the LoRA side channel, the 128x128 / 256x128 tiles.
Shapes: two images of 19 x 7 pixels (M = 266; 37 x 7 under 256-row tiles): an image has at least one M-tile of rows -- what the row bias
and the statistics need -- an M-tile crosses the image boundary and the last one has an m < M tail.  Cin = 64, N = 64 and N = 192 under
out_ld = 256.  Two images of 9 x 7 (M = 126, less than a tile per image) for the cases without a row bias.  The halo tiles need OW >= 8: two
images of 16 x 8.  N = 72 (whole quads, no whole 16-column block at the end) is taken by the direct form and asserted bit-equal.
[REF script/train/train_audioldm_lora.py:539-546] (UNet2DConditionModel.forward)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
PIPE, WS, W8, HALO = (2, 3, 4), (14, 13), (6, 10, 11), (7, 8, 15, 16)      # tiles with the direct form
BIG = (1, 9, 12)                                                          # 128x128, 256x128 (8-wave, loader-wave): LDS walk only
BM = {1: 128, 2: 64, 3: 128, 4: 64, 6: 128, 9: 256, 10: 64, 11: 128, 12: 256, 13: 64, 14: 128, 7: 128, 8: 64, 15: 128, 16: 64}


def dv(t):
    return t.to(torch.bfloat16).to(DEV)


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    return o


@pytest.fixture()
def lib():
    from audioldm_with_lora_amd import _lib
    return _lib


def both(ops, lib, monkeypatch, run, direct=True):
    """run(epi) -> tensor(s).  direct: (LDS walk, forced direct form); else (LDS walk, EPI_AUTO), which must report the LDS walk."""
    trace = []
    monkeypatch.setattr(ops, "EPI_TRACE", trace)
    a = run(lib.EPI_LDS)
    del trace[:]
    b = run(lib.EPI_DIRECT if direct else lib.EPI_AUTO)
    torch.cuda.synchronize()
    assert trace and trace[-1] == (1 if direct else 0), trace
    return a, b


def problem(seed, B, H, W, N, k=3, Cin=64):
    g = torch.Generator().manual_seed(seed)
    x = dv(torch.randn(B, H, W, Cin, generator=g))
    w = (torch.randn(N, Cin, k, k, generator=g) / math.sqrt(k * k * Cin)).to(DEV)
    return g, x, w


def image(tile, small=False):
    if tile in HALO:
        return 2, 16, 8
    if small:
        return 2, 9, 7
    return (2, 37, 7) if BM[tile] == 256 else (2, 19, 7)


@pytest.mark.parametrize("tile", PIPE + WS + W8 + HALO + BIG)
@pytest.mark.parametrize("N,ld,full", [(64, 64, False), (192, 256, True), (192, 192, True), (192, 256, False)])
def test_out_is_bit_identical(ops, lib, monkeypatch, tile, N, ld, full):
    """bias / row bias / residual / alpha on and off, contiguous and strided (out_ld > N) output rows"""
    B, H, W = image(tile, small=not full)
    g, x, w = problem(10 * tile + N + ld, B, H, W, N)
    pw = ops.pack_conv(w, torch.randn(N, generator=g).to(DEV) if full else None)
    rb = torch.randn(B, N + 4, generator=g).to(DEV)
    res = dv(torch.randn(B, H, W, ld, generator=g))
    kw = dict(pad=(1, 1), tile=tile, splits=1, out_ld=ld, out_batch_stride=H * W * ld)
    if full:
        kw.update(rowbias=rb[:, 4:], rowbias_ld=N + 4, res=res, alpha=0.5)

    def run(epi):
        out = torch.full((B, H, W, ld), 7.0, dtype=torch.bfloat16, device=DEV)
        ops.conv(x, pw, out=out, epi=epi, **kw)
        return out
    a, b = both(ops, lib, monkeypatch, run, direct=tile not in BIG)
    assert torch.equal(a, b)
    assert torch.equal(b[..., N:], torch.full_like(b[..., N:], 7.0))       # the columns past N stay untouched
    assert float(b[..., :N].float().abs().max()) > 0.1


def table_ref(out, tile, OW):
    """float64 (sum, sum of squares) per M-tile, image slot and channel quad of the stored values: [tiles][2][N / 4][2]"""
    B, H, W, N = out.shape
    v = out.double().cpu().reshape(B, H * W, N // 4, 4)
    bm, HW = BM[tile], H * W
    if tile in HALO:
        tpi = math.ceil(H / (bm // OW))
        ref = torch.zeros(B * tpi, 2, N // 4, 2, dtype=torch.float64)
        for b in range(B):
            for t in range(tpi):
                blk = v[b, t * bm:(t + 1) * bm]
                ref[b * tpi + t, 0, :, 0] = blk.sum((0, 2))
                ref[b * tpi + t, 0, :, 1] = (blk * blk).sum((0, 2))
        return ref
    M = B * HW
    flat = v.reshape(M, N // 4, 4)
    ref = torch.zeros(math.ceil(M / bm), 2, N // 4, 2, dtype=torch.float64)
    for t in range(ref.shape[0]):
        b0 = (t * bm) // HW
        for m in range(t * bm, min(M, (t + 1) * bm)):
            s = int(m // HW != b0)
            ref[t, s, :, 0] += flat[m].sum(1)
            ref[t, s, :, 1] += (flat[m] * flat[m]).sum(1)
    return ref


def check_tables(tab_lds, tab_new, ref, what):
    e_lds, e_new = (tab_lds - ref).abs(), (tab_new - ref).abs()
    ulp = torch.ldexp(torch.ones_like(ref), torch.floor(torch.log2(ref.abs().clamp_min(1e-30))).int() - 23)
    # twice the LDS walk's error on this case -- its maximum per (image slot, sum | sum of squares): the entries of the two kinds are two
    # orders of magnitude apart, and slot 1 holds far fewer rows -- or 8 ulps of the entry
    bound = torch.maximum(2 * e_lds.amax(dim=(0, 2), keepdim=True), 8 * ulp)
    print(f"{what}: LDS walk max err {float(e_lds.max()):.3g}, direct {float(e_new.max()):.3g}, max |entry| {float(ref.abs().max()):.3g}, "
          f"worst direct err / bound {float((e_new / bound).max()):.3g}")
    assert bool((e_new <= bound).all()), float((e_new / bound).max())


@pytest.mark.parametrize("tile", PIPE + WS + W8 + HALO)
def test_groupnorm_statistics(ops, lib, monkeypatch, tile):
    monkeypatch.setattr(ops, "QSTATS_MIN_HW", 1)
    trace = []
    monkeypatch.setattr(ops, "EPI_TRACE", trace)
    B, H, W = image(tile)
    N = 128
    g, x, w = problem(500 + tile, B, H, W, N)
    pw = ops.pack_conv(w, torch.randn(N, generator=g).to(DEV))
    rb = torch.randn(B, N, generator=g).to(DEV)
    res = dv(torch.randn(B, H, W, N, generator=g))
    outs, tabs = [], []
    for epi in (lib.EPI_LDS, lib.EPI_DIRECT):
        y = ops.conv(x, pw, pad=(1, 1), tile=tile, splits=1, rowbias=rb, rowbias_ld=N, res=res, alpha=0.75, qstats=True, epi=epi)
        assert getattr(y, "qstats", None) is not None
        outs.append(y)
        tabs.append(y.qstats.table.double().cpu())
    assert trace == [0, 1]
    assert torch.equal(outs[0], outs[1])
    ref = table_ref(outs[0], tile, W)
    check_tables(tabs[0], tabs[1], ref, f"tile {tile}")
    assert float(ref[:, 0].abs().max()) > 1 and (tile in HALO or float(ref[:, 1].abs().max()) > 1)   # slot 1 is exercised


@pytest.mark.parametrize("tile", HALO)
def test_halo_groupnorm_of_the_input(ops, lib, monkeypatch, tile):
    """gn-in launches (the loader / compute waves normalise the halo) end in the same epilogue"""
    monkeypatch.setattr(ops, "QSTATS_MIN_HW", 1)
    B, H, W, C, N = 2, 16, 8, 128, 128
    g, x, w0 = problem(700 + tile, B, H, W, C, Cin=C)
    y = ops.conv(x, ops.pack_conv(w0, None), pad=(1, 1), splits=1, qstats=True)
    assert getattr(y, "qstats", None) is not None
    pw = ops.pack_conv((torch.randn(N, C, 3, 3, generator=g) / 30).to(DEV), torch.randn(N, generator=g).to(DEV))
    gm, bt = (torch.randn(C, generator=g) * 0.3 + 1).to(DEV), (torch.randn(C, generator=g) * 0.2).to(DEV)
    assert ops.gn_in_ok(y, None, pw, (1, 1), (1, 1), (1, 1), None, None)
    a, b = both(ops, lib, monkeypatch, lambda epi: ops.conv(y, pw, pad=(1, 1), tile=tile, gn_in=(gm, bt, 32, 1e-5, 1), epi=epi))
    assert torch.equal(a, b)


@pytest.mark.parametrize("tile", [15, 16])
def test_halo_fused_shortcut_segment(ops, lib, monkeypatch, tile):
    B, H, W, C, Ce, N = 2, 16, 8, 64, 128, 128
    g, h, w = problem(800 + tile, B, H, W, N, Cin=C)
    xa = dv(torch.randn(B, H, W, Ce, generator=g))
    pw = ops.pack_conv_shortcut(w, torch.randn(N, generator=g).to(DEV), (torch.randn(N, Ce, 1, 1, generator=g) / 12).to(DEV),
                                torch.randn(N, generator=g).to(DEV))
    a, b = both(ops, lib, monkeypatch, lambda epi: ops.conv(h, pw, pad=(1, 1), x3=xa, tile=tile, ring=3, splits=1, epi=epi))
    assert torch.equal(a, b)


@pytest.mark.parametrize("tile", [2, 3, 4, 1])
def test_lora_side_channel(ops, lib, monkeypatch, tile):
    """rank-4 adapter riding the K loop (Rp = 32).  LoRA launches keep the LDS walk (the direct form grew the larger tiles by 0.9 - 1.8k
    instructions and measured slower on the 64x64 tile's short-K projections): they must report and run it, and refuse EPI_DIRECT."""
    B, H, W, K, N, r = 2, 19, 7, 64, 192, 4
    g = torch.Generator().manual_seed(900 + tile)
    x = dv(torch.randn(B, H, W, K, generator=g))
    pw = ops.pack_linear((torch.randn(N, K, generator=g) / 8).to(DEV), torch.randn(N, generator=g).to(DEV))
    ops.attach_lora(pw, [(0, N, (torch.randn(r, K, generator=g) / r).to(DEV), (torch.randn(N, r, generator=g) * 0.05).to(DEV), 2.0)])
    res = dv(torch.randn(B, H, W, N, generator=g))
    rb = torch.randn(B, N, generator=g).to(DEV)
    a, b = both(ops, lib, monkeypatch, lambda epi: ops.conv(x, pw, tile=tile, splits=1, res=res, rowbias=rb, rowbias_ld=N, alpha=1.5, epi=epi),
                direct=False)
    assert torch.equal(a, b)
    with pytest.raises(lib.AldmError):
        ops.conv(x, pw, tile=tile, splits=1, res=res, epi=lib.EPI_DIRECT)


def test_n72_whole_quads(ops, lib, monkeypatch):
    B, H, W, K, N = 2, 9, 7, 64, 72
    g = torch.Generator().manual_seed(950)
    x = dv(torch.randn(B, H, W, K, generator=g))
    pw = ops.pack_linear((torch.randn(N, K, generator=g) / 8).to(DEV), torch.randn(N, generator=g).to(DEV))
    a, b = both(ops, lib, monkeypatch, lambda epi: ops.conv(x, pw, tile=2, splits=1, epi=epi))
    assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["act", "out2_act", "out2", "res2", "f32", "vt", "geglu", "rowstats", "ln", "rowbias_small_image"])
def test_fallbacks_take_the_lds_walk(ops, lib, monkeypatch, kind):
    """every term of the host rule: the launch reports the LDS walk under EPI_AUTO, refuses EPI_DIRECT, and equals the forced LDS walk;
    the ones whose work the direct form would drop are also checked against torch"""
    B, H, W, K = 2, 9, 7, 64
    M = B * H * W
    g = torch.Generator().manual_seed(1000)
    x = dv(torch.randn(B, H, W, K, generator=g))
    N = 128
    wt, bias = dv(torch.randn(N, K, generator=g) / 8).float(), torch.randn(N, generator=g).to(DEV)
    r2 = dv(torch.randn(B, H, W, N, generator=g))
    rb = torch.randn(B, N, generator=g).to(DEV)
    if kind == "geglu":
        pw = ops.pack_geglu(wt, bias)
    elif kind == "ln":
        pw = ops.pack_linear_ln(wt, bias, (torch.randn(K, generator=g) * 0.3 + 1).to(DEV), (torch.randn(K, generator=g) * 0.2).to(DEV))
    else:
        pw = ops.pack_linear(wt, bias)
    lin = x.float().reshape(M, K) @ wt.float().t() + bias                  # fp32 reference of the plain projection

    def run(epi):
        kw = dict(tile=2, splits=1, epi=epi)
        if kind == "act":
            return ops.conv(x, pw, out_act=ops.ACT_SILU, **kw)
        if kind in ("out2_act", "out2"):
            o2 = torch.zeros(B, H, W, N, dtype=torch.bfloat16, device=DEV)
            y = ops.conv(x, pw, out2=o2, post_act=(ops.ACT_SILU if kind == "out2_act" else ops.ACT_NONE), **kw)
            return torch.cat([y, o2], -1)
        if kind == "res2":
            return ops.conv(x, pw, res2=r2, alpha=0.5, **kw)
        if kind == "f32":
            return ops.conv(x, pw, out_f32=True, **kw)
        if kind == "vt":
            vt = torch.zeros(B, 64, 64, dtype=torch.bfloat16, device=DEV)
            y = ops.conv(x, pw, vt=vt, vt_col0=64, vt_ld=64, vt_batch_stride=64 * 64, **kw)
            return torch.cat([y.reshape(B, H * W, 64), vt[:, :, :H * W].transpose(1, 2)], -1)
        if kind == "rowstats":
            y, st = ops.conv(x, pw, rowstats=True, **kw)
            return torch.cat([y.reshape(M, N).float(), st.reshape(M, -1)], -1)
        if kind == "rowbias_small_image":                                   # 63 pixels an image < the tile's 64 rows: two boundaries in a tile
            return ops.conv(x, pw, rowbias=rb, rowbias_ld=N, **kw)
        return ops.conv(x, pw, **kw)
    a, b = both(ops, lib, monkeypatch, run, direct=False)
    assert torch.equal(a, b)
    assert float(a.float().abs().max()) > 0.1
    with pytest.raises(lib.AldmError):
        run(lib.EPI_DIRECT)
    tol = dict(rtol=2e-2, atol=3e-2)
    if kind == "out2":
        assert torch.equal(b[..., :N], b[..., N:])                          # out2 = post_act(out) with no activation: written, equal
        torch.testing.assert_close(b[..., :N].float().cpu().reshape(M, N), lin.cpu(), **tol)
    if kind == "res2":
        torch.testing.assert_close(b.float().cpu().reshape(M, N), (0.5 * lin + r2.float().reshape(M, N)).cpu(), **tol)
    if kind == "f32":
        assert b.dtype == torch.float32
        torch.testing.assert_close(b.cpu().reshape(M, N), lin.cpu(), **tol)
    if kind == "rowstats":
        y = b[:, :N].double()
        st = b[:, N:].double().reshape(M, -1, 2)
        parts = st.shape[1]
        yb = y.reshape(M, parts, N // parts)
        torch.testing.assert_close(st[..., 0], yb.sum(-1), rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(st[..., 1], (yb * yb).sum(-1), rtol=1e-5, atol=1e-4)
    if kind == "rowbias_small_image":
        torch.testing.assert_close(b.float().cpu().reshape(M, N), (lin.reshape(B, H * W, N) + rb[:, None, :]).reshape(M, N).cpu(), **tol)


def test_cold_launch_is_deterministic(ops, lib, monkeypatch):
    """the direct form with its statistics (the only part that touches LDS: the cross-wave table and its barrier) twice from fresh
    allocations on an idle GPU: output and table bit-equal"""
    monkeypatch.setattr(ops, "QSTATS_MIN_HW", 1)
    B, H, W, N = 2, 19, 7, 128
    g, x, w = problem(1100, B, H, W, N)
    pw = ops.pack_conv(w, torch.randn(N, generator=g).to(DEV))
    res = dv(torch.randn(B, H, W, N, generator=g))
    got = []
    for _ in range(2):
        torch.cuda.synchronize()
        y = ops.conv(x, pw, pad=(1, 1), tile=3, splits=1, res=res, qstats=True, epi=lib.EPI_DIRECT)
        torch.cuda.synchronize()
        got.append((y.clone(), y.qstats.table.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
