"""GPU parity of the nine entry points of csrc/clap_audio.hip and csrc/mel.hip against the float64 restatements of
tests/clap_audio_restatement.py at their pad, shift and arm edges: per element within a derived bound (`check_elem`), within twice the
L2 floor / four times the max floor of a float32 FFT and within the log-domain bound that follows from it for the two log-mels, bit for
bit where the contract is a copy or a single rounding.  Every input is a slice from the middle of a NaN arena, every output the middle
slice of a NaN arena whose guards must still be NaN.  tests/test_clap_audio_restatement_host.py proves on the CPU that these
comparators reject every listed mutant at exactly these shapes."""
import math

import numpy as np
import pytest
import torch

import clap_audio_restatement as R
import conftest

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256          # NaN elements either side of every operand (a multiple of 8: 16-byte alignment is kept)
DB = 10.0 / math.log(10.0)
E_ARG, E_ALIGN, E_UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from audioldm_with_lora_amd import _lib
    return _lib.load()


def P(t):
    from audioldm_with_lora_amd.ops import _p
    return _p(t)


def S():
    from audioldm_with_lora_amd.ops import _stream
    return _stream()


def arena(shape, dtype):
    """-> (whole NaN arena, its contiguous middle slice viewed as `shape`)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(shape)


def put(x, dtype):
    """a float64 numpy array (NaN allowed) as the middle slice of a NaN arena"""
    _, mid = arena(x.shape, dtype)
    mid.copy_(torch.from_numpy(np.ascontiguousarray(x)).to(dtype))
    return mid


def guards_ok(whole):
    torch.cuda.synchronize()
    assert bool(whole[:GUARD].isnan().all()) and bool(whole[-GUARD:].isnan().all()), "the kernel wrote outside its output"


def ok(rc, what):
    from audioldm_with_lora_amd._lib import check
    check(rc, what)


def ranges_of(basis):
    rng = np.zeros((basis.shape[0], 2), dtype=np.int32)
    for m, row in enumerate(basis):
        nz = np.nonzero(row)[0]
        rng[m] = (nz.min(), nz.max() + 1) if nz.size else (0, 0)
    return torch.from_numpy(rng).to(DEV)


def f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def banks():
    from audioldm_with_lora_amd import clap_audio as CA
    return {"htk": CA.mel_filter_bank(513, 64, 0, 14000, 48000, norm=None, mel_scale="htk").T.astype(np.float32).astype(np.float64),
            "slaney": CA.mel_filter_bank(513, 64, 0, 14000, 48000, norm="slaney", mel_scale="slaney").T.astype(np.float32).astype(np.float64)}


# ---- resampler -------------------------------------------------------------------------------------------------------------------
def test_resample_up3_lens_and_clamps(lib):
    from audioldm_with_lora_amd.clap_audio import resample_taps
    taps = resample_taps(3).astype(np.float32).astype(np.float64)
    x = R.resample_draw()
    B, Tin = x.shape
    assert (B, Tin) == (5, 300) and all(np.isnan(x[b, L:]).all() for b, L in enumerate(R.RESAMPLE_LENS))
    y, Sabs, Kn = R.resample_up3(x, R.RESAMPLE_LENS, taps)
    xd, td = put(x, torch.float32), f32(taps)
    lens = torch.tensor(R.RESAMPLE_LENS, dtype=torch.int32, device=DEV)
    whole, out = arena((B, 3 * Tin), torch.float32)
    ok(lib.aldm_resample_up3(P(xd), P(lens), B, Tin, P(td), 61, P(out), 3 * Tin, S()), "aldm_resample_up3")
    guards_ok(whole)
    R.check_elem(out, y, R.resample_bound(Sabs, Kn), "resample_up3")
    for b, L in enumerate(R.RESAMPLE_LENS):
        assert not bool(out[b, 3 * L:].ne(0).any()), f"clip {b}: the tail past 3 L is not exactly zero"


# ---- CLAP log-mel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", R.CLAP_LS)
@pytest.mark.parametrize("bank", ["htk", "slaney"])
def test_clap_log_mel_repeat_and_tail(lib, bank, L):
    basis, win = banks()[bank], R.periodic_hann()
    w = np.full((2, R.CLAP_MAX_LEN), np.nan)
    w[0, :L] = R.noise_tones(L, L, 48000)
    w[1, :L] = 0.0
    lens = [L, L]
    ex = R.clap_log_mel(w, lens, R.CLAP_MAX_LEN, R.CLAP_HOP, win, basis)
    ref = R.with_floor(ex, R.clap_log_mel(w, lens, R.CLAP_MAX_LEN, R.CLAP_HOP, win, basis, rounded=True), "db")
    wd, bd, wind = put(w, torch.float32), f32(basis), f32(win)
    whole, out = arena((2, 11, 64), torch.float32)
    ld, rg = torch.tensor(lens, dtype=torch.int32, device=DEV), ranges_of(basis)     # (every operand stays referenced until the sync)
    ok(lib.aldm_clap_log_mel(P(wd), P(ld), 2, R.CLAP_MAX_LEN, R.CLAP_MAX_LEN, 1024, R.CLAP_HOP, P(wind), P(bd), P(rg), 64, P(out), S()),
       "aldm_clap_log_mel")
    guards_ok(whole)
    got = out.double().cpu().numpy()
    assert np.isfinite(got).all()
    what = f"clap_log_mel {bank} L{L}"
    R.check_lin(got[0], ref, 0, what)
    R.check_log(got[0], ref, 0, DB, what, need_share=L not in R.CLAP_LINE_LS)
    assert (got[0][~ex["live"][0]] == -100.0).all(), "an all-zero frame of the zero tail is not exactly -100 dB"
    assert (got[1] == -100.0).all(), "the all-zero clip is not exactly -100 dB"
    if L == 2401:
        assert not ex["live"][0, 8:].any()                                  # rep_end = 2401: the zero tail, reflected at the right border


# ---- log_mel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_", R.LOG_MEL_TS)
def test_log_mel_frame_boundaries(lib, T_):
    from audioldm_with_lora_amd.mel import mel_filter_bank
    basis, win = mel_filter_bank(16000, 1024, 64, 0, 8000).astype(np.float64), R.periodic_hann()
    w = np.stack([R.noise_tones(T_, T_, 16000).astype(np.float64), np.zeros(T_)])
    ex = R.log_mel(w, R.LOG_MEL_HOP, R.LOG_MEL_TARGET, win, basis)
    ref = R.with_floor(ex, R.log_mel(w, R.LOG_MEL_HOP, R.LOG_MEL_TARGET, win, basis, rounded=True), "ln")
    n = ex["n_frames"]
    assert n == min(8, T_ // 160)
    wd, bd, wind = put(w, torch.float32), f32(basis), f32(win)
    whole, out = arena((2, 8, 64), torch.float32)
    rg = ranges_of(basis)
    ok(lib.aldm_log_mel(P(wd), 2, T_, 1024, R.LOG_MEL_HOP, P(wind), P(bd), P(rg), 64, R.LOG_MEL_TARGET, 1e-5, P(out), S()), "aldm_log_mel")
    guards_ok(whole)
    got = out.double().cpu().numpy()
    assert np.isfinite(got).all()
    assert not got[:, n:].any(), "frames past the clip are not exactly zero"
    what = f"log_mel T{T_}"
    R.check_lin(got[0], ref, 0, what)
    R.check_log(got[0], ref, 0, 1.0, what)
    assert (got[1, :n] == np.float64(np.float32(math.log(np.float32(1e-5))))).all(), "a silent frame is not exactly log(1e-5)"


# ---- input stage -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_", R.INPUT_TS)
@pytest.mark.parametrize("variant", ["distinct", "stride0", "absent"])
def test_clap_input(lib, variant, T_):
    B = 2
    C = 4 if variant == "distinct" else 1
    mel, sc, sh = R.input_draw(T_, C=C, B=B)
    pad = 3 * 64                                                            # NaN elements between the items: a batch stride past the tensor
    item = C * T_ * 64
    buf = np.full((B, item + pad), np.nan)
    buf[:, :item] = mel.reshape(B, item)
    md = put(buf, torch.float32)
    want_l = variant != "absent"
    ref = R.clap_input(np.repeat(mel, 4, axis=1) if variant == "stride0" else mel, sc, sh)
    gw, g = arena((B, 64, 64, 16), torch.bfloat16)
    lw, l = arena((B, 64, 64, 48), torch.bfloat16) if want_l else (None, None)
    scd, shd = f32(sc), f32(sh)
    ok(lib.aldm_clap_input(P(md), item + pad, 0 if variant == "stride0" else T_ * 64, B, T_, 64, P(scd), P(shd), P(g), P(l), S()),
       "aldm_clap_input")
    guards_ok(gw)
    R.check_elem(g, ref["g"], ref["g_bound"], f"clap_input g T{T_} {variant}")
    if want_l:
        guards_ok(lw)
        R.check_elem(l, ref["l"], ref["l_bound"], f"clap_input l T{T_} {variant}")
        assert not bool(l[:, :, 63].ne(0).any()), "token column 63 of the local rows is not zero"
        if variant == "distinct":                                           # the three local channels really differ in this draw
            assert np.abs(ref["l"][:, :, 0:21] - ref["l"][:, :, 21:42]).max() > 1.0


# ---- attentional feature fusion --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.AFF_CS)
def test_aff_sum_pool_and_combine(lib, C):
    B = 1 if C == 2048 else 3
    longer = [1] if B == 1 else [1, 0, 1]
    h, r, loc, glob = R.aff_draw(B, C)
    pool_ex, pool_rd = R.aff_sum_pool(h, r), R.aff_sum_pool(h, r, rounded=True)
    comb = R.aff_combine(h, r, loc, glob, longer)
    comb_rd = R.aff_combine(h, r, loc, glob, longer, rounded=True)
    rn = r.copy()
    rn.reshape(B, 64, 64, C)[:, :, 63] = np.nan                             # the local branch's padding column must never be read
    hd, rd_ = put(h, torch.bfloat16), put(rn, torch.bfloat16)
    aw, a = arena((B, 4096, C), torch.bfloat16)
    pw, pooled = arena((B, C), torch.bfloat16)
    ok(lib.aldm_aff_sum_pool(P(hd), P(rd_), B, C, P(a), P(pooled), S()), "aldm_aff_sum_pool")
    guards_ok(aw)
    guards_ok(pw)
    assert R.bits_equal(a, pool_rd["a"]), "a != bf16(h + r)"
    R.check_elem(pooled, pool_ex["pooled"], pool_ex["pooled_bound"], f"aff pooled C{C}")
    ow, out = arena((B, 4096, C), torch.bfloat16)
    lg = torch.tensor(longer, dtype=torch.int32, device=DEV)
    locd, globd = f32(loc), f32(glob)
    ok(lib.aldm_aff_combine(P(hd), P(rd_), P(locd), P(globd), P(lg), B, C, P(out), S()), "aldm_aff_combine")
    guards_ok(ow)
    got = out.double().cpu().numpy()
    fused = np.asarray(longer, dtype=bool)
    R.check_elem(got[fused], comb["out"][fused], comb["bound"][fused], f"aff combine C{C}")
    assert np.array_equal(got[~fused], h[~fused]), "a not-longer item is not its global branch bit for bit"
    e_l2, f_l2, e_max, f_max = R.floor_ratios(torch.from_numpy(got[fused]), torch.from_numpy(comb["out"][fused]), torch.from_numpy(comb_rd["out"][fused]))
    conftest.record(e_l2 / f_l2, f"aff combine C{C} l2/floor")


# ---- window attention ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,shift,draw,heads,B,padded", R.window_cases())
def test_window_attention(lib, H, W, shift, draw, heads, B, padded):
    C = heads * 24
    rows = B * H * W
    qkv, bias = R.window_draw(draw, B, H, W, heads, shift)
    ex = R.window_attention(qkv, B, H, W, heads, shift, bias)
    rd = R.window_attention(qkv, B, H, W, heads, shift, bias, rounded=True)
    ld, ld_out = (3 * C + 8, C + 8) if padded else (3 * C, C)
    full = np.full((rows, ld), np.nan)
    full[:, :3 * C] = qkv.numpy()
    qd = put(full, torch.bfloat16)
    ow, out = arena((rows, ld_out), torch.bfloat16)
    bd = f32(bias.numpy())
    ok(lib.aldm_window_attention(P(qd), ld, B, H, W, heads, 24, 8, shift, P(bd), 1.0 / math.sqrt(24), P(out), ld_out, S()),
       "aldm_window_attention")
    guards_ok(ow)
    if padded:
        assert bool(out[:, C:].isnan().all()), "the padding columns of the output rows were written"
    got = out[:, :C].double().cpu()
    what = f"window {H}x{W} s{shift} {draw} h{heads} B{B}" + (" padded" if padded else "")
    R.check_elem(got, ex["out"], ex["bound"], what)
    R.check(got, torch.from_numpy(ex["out"]), torch.from_numpy(rd["out"]), what)


# ---- merge and mean --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", R.MERGE_CASES)
def test_patch_merge_gather(lib, B, H, W, C):
    x = R.r16(np.random.default_rng(C).standard_normal((B * H * W, C)))
    xd = put(x, torch.bfloat16)
    ow, out = arena((B * (H // 2) * (W // 2), 4 * C), torch.bfloat16)
    ok(lib.aldm_patch_merge_gather(P(xd), B, H, W, C, P(out), S()), "aldm_patch_merge_gather")
    guards_ok(ow)
    assert R.bits_equal(out, R.patch_merge_gather(x, B, H, W, C))


@pytest.mark.parametrize("N", R.MEAN_NS)
@pytest.mark.parametrize("C", R.MEAN_CS)
def test_token_mean(lib, C, N):
    x = R.r16(1.0 + np.random.default_rng(C + N).standard_normal((2, N, C)))
    ref = R.token_mean(x)
    xd = put(x, torch.bfloat16)
    w32, o32 = arena((2, C), torch.float32)
    w16, o16 = arena((2, C), torch.bfloat16)
    ok(lib.aldm_token_mean(P(xd), 2, N, C, P(o32), P(o16), S()), "aldm_token_mean")
    guards_ok(w32)
    guards_ok(w16)
    R.check_elem(o32, ref["mean"], ref["bound"], f"token_mean C{C} N{N}")
    assert torch.equal(o16, o32.to(torch.bfloat16)), "out_bf16 != bf16(out_f32)"


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def test_rejections_return_their_rc(lib):
    z16 = torch.zeros(4 * 4096 * 64, dtype=torch.bfloat16, device=DEV)
    o16 = torch.zeros(64 * 64, dtype=torch.bfloat16, device=DEV)
    z32 = torch.zeros(2 * 1025 * 64, dtype=torch.float32, device=DEV)
    zi = torch.zeros(256, dtype=torch.int32, device=DEV)
    s = 1.0 / math.sqrt(24)
    wa = lambda **k: lib.aldm_window_attention(P(k.get("qkv", z16)), k.get("ld", 144), 1, k.get("H", 8), 8, 2, k.get("hd", 24), 8,
                                               k.get("shift", 0), P(z32), s, P(o16), k.get("ld_out", 48), S())
    assert wa() == 0
    assert wa(hd=32) == E_UNSUPPORTED
    assert wa(shift=8) == E_UNSUPPORTED
    assert wa(H=12) == E_UNSUPPORTED
    assert wa(ld=148) == E_ALIGN and wa(ld_out=52) == E_ALIGN
    assert wa(qkv=z16[4:]) == E_ALIGN                                       # rows 8 bytes off a 16-byte boundary
    assert wa(ld=136) == E_ARG                                              # narrower than Q | K | V
    assert lib.aldm_patch_merge_gather(P(z16), 1, 4, 4, 12, P(z16), S()) == E_UNSUPPORTED          # C % 8
    assert lib.aldm_patch_merge_gather(P(z16), 1, 3, 4, 8, P(z16), S()) == E_UNSUPPORTED
    assert lib.aldm_aff_sum_pool(P(z16), P(z16), 1, 12, P(z16), P(z16), S()) == E_UNSUPPORTED      # C % 8
    assert lib.aldm_aff_sum_pool(P(z16), P(z16), 1, 2056, P(z16), P(z16), S()) == E_UNSUPPORTED
    for T_ in (1, 1025):
        assert lib.aldm_clap_input(P(z32), 1025 * 64, 0, 1, T_, 64, P(z32), P(z32), P(z16), None, S()) == E_UNSUPPORTED
    assert lib.aldm_clap_input(P(z32), 1024 * 64, 0, 1, 1024, 80, P(z32), P(z32), P(z16), None, S()) == E_UNSUPPORTED
    assert lib.aldm_clap_log_mel(P(z32), P(zi), 1, 4800, 4800, 512, 480, P(z32), P(z32), P(zi), 64, P(z32), S()) == E_UNSUPPORTED
    assert lib.aldm_log_mel(P(z32), 1, 4800, 512, 160, P(z32), P(z32), P(zi), 64, 8, 1e-5, P(z32), S()) == E_ARG
    assert lib.aldm_log_mel(P(z32), 1, 432, 1024, 160, P(z32), P(z32), P(zi), 64, 8, 1e-5, P(z32), S()) == E_ARG    # too short to reflect
    torch.cuda.synchronize()
