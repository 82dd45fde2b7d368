"""CPU: the float64 restatements of tests/clap_audio_restatement.py equal independent float64 references to 1e-9, every draw is what
it claims to be, and the comparators of tests/test_gpu_clap_audio_edges.py accept `rounded` and reject every listed mutant at the
shapes that file uses.  Run with -s for the ratios."""
import math

import numpy as np
import pytest
import torch

import clap_audio_restatement as R
from audioldm_with_lora_amd import clap_audio as CA
from audioldm_with_lora_amd import mel as PM

F64 = torch.float64
TAPS32 = CA.resample_taps(3).astype(np.float32).astype(np.float64)
DB = 10.0 / math.log(10.0)


def close9(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max()) if a.size else 0.0
    assert err <= 1e-9 * max(1.0, float(np.abs(b).max())), (what, err)


def htk_bank():
    return CA.mel_filter_bank(513, 64, 0, 14000, 48000, norm=None, mel_scale="htk").T.astype(np.float32).astype(np.float64)


def slaney48_bank():
    return CA.mel_filter_bank(513, 64, 0, 14000, 48000, norm="slaney", mel_scale="slaney").T.astype(np.float32).astype(np.float64)


def slaney16_bank():
    return PM.mel_filter_bank(16000, 1024, 64, 0, 8000).astype(np.float64)


def clap_wave(L, kind, seed=0):
    if kind == "zero":
        return np.zeros((1, R.CLAP_MAX_LEN))
    w = np.full((1, R.CLAP_MAX_LEN), np.nan)
    w[0, :L] = R.noise_tones(L, seed + L, 48000)
    return w


# ---- the restatements against independent references ---------------------------------------------------------------------------
def test_resampler_equals_resample_poly():
    sig = pytest.importorskip("scipy.signal")
    x = R.resample_draw()
    h = CA.resample_taps(3)
    y, S, Kn = R.resample_up3(x, R.RESAMPLE_LENS, h)
    for b, L in enumerate(R.RESAMPLE_LENS):
        close9(y[b, :3 * L], sig.resample_poly(x[b, :L], 3, 1), f"clip {b}")
        assert not y[b, 3 * L:].any() and np.isfinite(y[b]).all()
        assert Kn[b, :3 * L].min() >= 1 and Kn[b, :3 * L].max() <= 21 and (S[b, :3 * L] >= np.abs(y[b, :3 * L]) - 1e-15).all()
    # the clamps at both ends are reached: the first outputs meet fewer taps than the middle, the last ones too, one sample meets <= 21
    assert Kn[0, 0] < Kn[0, 450] == 20 or Kn[0, 450] == 21
    assert Kn[0, 899] < Kn[0, 450] and Kn[2, :3].tolist() == [1, 1, 1]


def _clap_independent(w, L, max_len, hop, window, basis, pad_mode="reflect"):
    c = np.tile(w[:L], max_len // L)
    c = np.concatenate([c, np.zeros(max_len - c.size)])
    p = np.pad(c, (512, 512), mode=pad_mode)
    rows = []
    for f in range(1 + max_len // hop):
        X = np.fft.rfft(p[f * hop:f * hop + 1024] * window)
        rows.append(basis @ (np.abs(X) ** 2))
    lin = np.array(rows)
    return lin, 10.0 * np.log10(np.maximum(lin, 1e-10))


@pytest.mark.parametrize("L", R.CLAP_LS)
def test_clap_log_mel_equals_rfft(L):
    win = R.periodic_hann()
    for bank in (htk_bank(), slaney48_bank()):
        w = clap_wave(L, "noise")
        ref = R.clap_log_mel(w, [L], R.CLAP_MAX_LEN, R.CLAP_HOP, win, bank)
        lin, lg = _clap_independent(w[0], L, R.CLAP_MAX_LEN, R.CLAP_HOP, win, bank)
        close9(ref["lin"][0], lin, "lin")
        judged = lin > 1e-6 * lin.max()
        close9(ref["log"][0][judged], lg[judged], "log")                   # far below the peak the two rffts differ in the last bits
        assert ref["lin"].shape == (1, 11, 64)


def test_clap_log_mel_equals_feature_extractor():
    tr = pytest.importorskip("transformers")
    fe = tr.ClapFeatureExtractor(truncation="rand_trunc", padding="repeatpad")
    win64 = np.hanning(1025)[:-1]
    for L in (4800, 4799, 2401, 1600, 513, 7):
        w = clap_wave(L, "noise")
        f = fe(w[0, :L].astype(np.float32), sampling_rate=48000, max_length=R.CLAP_MAX_LEN, return_tensors="np")
        got = R.clap_log_mel(w, [L], R.CLAP_MAX_LEN, R.CLAP_HOP, win64, fe.mel_filters_slaney.T)
        want = np.asarray(f["input_features"], dtype=np.float64)[0, 0]
        assert want.shape == (11, 64)
        judged = got["lin"][0] > 1e-6 * got["lin"][0].max()
        assert np.abs(got["log"][0] - want)[judged].max() < 1e-4, L       # the extractor returns float32


@pytest.mark.parametrize("T_", R.LOG_MEL_TS)
def test_log_mel_equals_torch_stft_float64(T_):
    n = R.log_mel_frames(T_, R.LOG_MEL_HOP, R.LOG_MEL_TARGET)
    assert n == min(8, T_ // 160)
    assert {433: 2, 479: 2, 480: 3, 592: 3, 593: 3, 1279: 7, 1280: 8, 1439: 8, 1440: 8, 1552: 8, 1553: 8, 3000: 8}[T_] == n
    w = R.noise_tones(T_, T_, 16000).astype(np.float64)[None]
    win, bank = R.periodic_hann(), slaney16_bank()
    ref = R.log_mel(w, R.LOG_MEL_HOP, R.LOG_MEL_TARGET, win, bank)
    p = torch.nn.functional.pad(torch.from_numpy(w)[None], (432, 432), mode="reflect")[0]
    X = torch.stft(p, 1024, hop_length=160, win_length=1024, window=torch.from_numpy(win), center=False, onesided=True,
                   return_complex=True)[0]                                  # [513, frames]
    lin = (torch.from_numpy(bank) @ X.abs()).T.numpy()[:8]
    assert lin.shape[0] == n
    close9(ref["lin"][0, :n], lin, "lin")
    close9(ref["log"][0, :n], np.log(np.maximum(lin, np.float64(np.float32(1e-5)))), "log")
    assert not ref["lin"][0, n:].any() and not ref["log"][0, n:].any()


@pytest.mark.parametrize("T_", R.INPUT_TS)
def test_resize_equals_torch_bicubic(T_):
    mel, sc, sh = R.input_draw(T_)
    got = R.resize_1024(mel)
    want = torch.nn.functional.interpolate(torch.from_numpy(mel), size=(1024, 64), mode="bicubic", align_corners=True).numpy()
    close9(got, want, f"T {T_}")
    if T_ == 1024:
        assert np.array_equal(got, mel)


def ref_window_attention64(qkv, B, H, W, heads, shift, bias):
    """test_gpu_clap_audio.ref_window_attention in float64"""
    C = heads * 24
    x = qkv.double().view(B, H, W, 3 * C)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    win = x.view(B, H // 8, 8, W // 8, 8, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 64, 3 * C)
    q, k, v = (win[..., i * C:(i + 1) * C].reshape(-1, 64, heads, 24).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(24) + bias.double()[None]
    if shift:
        hr = (torch.arange(H) >= H - 8).long() + (torch.arange(H) >= H - shift).long()
        wr = (torch.arange(W) >= W - 8).long() + (torch.arange(W) >= W - shift).long()
        reg = (hr[:, None] * 3 + wr[None, :]).view(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64)
        m = torch.where(reg[:, None, :] != reg[:, :, None], -100.0, 0.0).double()
        s = (s.view(B, -1, heads, 64, 64) + m[None, :, None]).view(-1, heads, 64, 64)
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, H // 8, W // 8, 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(B * H * W, C)


@pytest.mark.parametrize("H,W", [(8, 16), (16, 8), (16, 24), (24, 16)])
@pytest.mark.parametrize("shift", range(8))
def test_window_attention_equals_float64_reference(H, W, shift):
    for draw in ("diffuse", "peaked"):
        qkv, bias = R.window_draw(draw, 2, H, W, 2, shift)
        got = R.window_attention(qkv, 2, H, W, 2, shift, bias)["out"]
        close9(got, ref_window_attention64(qkv, 2, H, W, 2, shift, bias).numpy(), f"{draw} {H}x{W} s{shift}")


def test_merge_is_transformers_order():
    x = np.arange(2 * 4 * 6 * 8, dtype=np.float64).reshape(2, 4, 6, 8)
    t = torch.from_numpy(x)
    want = torch.cat([t[:, 0::2, 0::2], t[:, 1::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 1::2]], -1).reshape(-1, 32).numpy()
    assert np.array_equal(R.patch_merge_gather(x, 2, 4, 6, 8), want)
    assert not np.array_equal(R.patch_merge_gather(x, 2, 4, 6, 8, mutant="swapped"), want)


def test_input_stage_chain_equals_transformers_patch_embed():
    """clap_input + the two patch GEMMs + aff_sum_pool + aff_combine, float64, against ClapAudioEncoder's batch_norm, reshape_mel2img and
    ClapAudioPatchEmbed with four distinct channels and is_longer = [True, False, True]: pins c * 21 + j, column 63 and the not-longer
    arm against the model itself."""
    tr = pytest.importorskip("transformers")
    from transformers.models.clap.modeling_clap import ClapAudioEncoder
    import clap_audio_weights as W
    cfg = tr.ClapAudioConfig(**dict(W.audio_config("narrow"), enable_patch_layer_norm=False, depths=[1, 1, 1, 1]))
    torch.manual_seed(3)
    enc = ClapAudioEncoder(cfg).double().eval()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for n_, p in enc.named_parameters():
            if "patch_embed" in n_ or n_.startswith("batch_norm"):
                p.copy_(torch.randn(p.shape, generator=g, dtype=F64) * (0.3 if p.dim() > 1 else 0.2) + (1.0 if "norm" in n_ and n_.endswith("weight") else 0.0))
        for n_, b in enc.named_buffers():
            if n_.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g, dtype=F64) * 0.2 + (-35.0 if n_.startswith("batch_norm") else 0.0))
            if n_.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g, dtype=F64) + (50.0 if n_.startswith("batch_norm") else 0.5))
    mel, _, _ = R.input_draw(1001, C=4, B=3)
    longer = [True, False, True]
    feats = torch.from_numpy(mel)
    with torch.no_grad():
        x = enc.batch_norm(feats.transpose(1, 3)).transpose(1, 3)
        want = enc.patch_embed(enc.reshape_mel2img(x), torch.where(torch.tensor(longer))[0]).numpy()      # [3, 4096, 48]
    bn = enc.batch_norm
    s = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach()
    sc, sh = s.numpy(), (bn.bias - bn.running_mean * s).detach().numpy()
    rows = R.clap_input(mel, sc, sh)
    assert not rows["l"][:, :, 63].any()
    pe = enc.patch_embed
    wp, wm = pe.proj.weight.detach().reshape(48, 16).numpy(), pe.mel_conv2d.weight.detach().reshape(48, 48).numpy()
    h = rows["g"].reshape(3, 4096, 16) @ wp.T + pe.proj.bias.detach().numpy()
    r = rows["l"].reshape(3, 4096, 48) @ wm.T + pe.mel_conv2d.bias.detach().numpy()              # column 63 holds the bare bias here
    sp = R.aff_sum_pool(h, r)
    fm = pe.fusion_model

    def branch(seq, t):                                                     # 1x1 conv, BatchNorm, ReLU, 1x1 conv, BatchNorm over [..., C]
        with torch.no_grad():
            y = seq(torch.from_numpy(t).reshape(-1, 48, 1, 1))
        return y.reshape(t.shape[:-1] + (48,)).numpy()
    loc = branch(fm.local_att, sp["a"])
    glob = branch(torch.nn.Sequential(*list(fm.global_att)[1:]), sp["pooled"])
    got = R.aff_combine(h, r, loc, glob, longer)["out"]
    close9(got, want, "patch embed")
    assert np.array_equal(got[1], h[1])
    for m in ("chan_perm", "col63", "khkw"):
        rm = R.clap_input(mel, sc, sh, mutant=m)
        assert np.abs(rm["l"] - rows["l"]).max() > 0.1, m


# ---- the float32 FFT and the floor's margin --------------------------------------------------------------------------------------
def test_float32_fft_is_a_dft_and_its_floor_is_a_float32_floor():
    """fft4_f32 against np.fft.fft; and the measured constant of the floor rule: a second float32 FFT (scipy.fft.rfft on float32 input)
    sits within the 2 x / 4 x of section 16 of the floor that fft4_f32 defines, on every log-mel draw (the spread is printed)."""
    sfft = pytest.importorskip("scipy.fft")
    g = np.random.default_rng(0)
    x = g.standard_normal((3, 1024))
    X = R.fft4_f32(x.astype(np.complex64))
    assert X.dtype == np.complex64
    ref = np.fft.fft(x.astype(np.float32).astype(np.float64))
    assert np.abs(X - ref).max() / np.abs(ref).max() < 2e-6
    win, spread = R.periodic_hann(), []
    for L in R.CLAP_LS:
        w = clap_wave(L, "noise")
        ex = R.clap_log_mel(w, [L], R.CLAP_MAX_LEN, R.CLAP_HOP, win, htk_bank())
        rd = R.clap_log_mel(w, [L], R.CLAP_MAX_LEN, R.CLAP_HOP, win, htk_bank(), rounded=True)
        c = np.tile(w[0, :L], R.CLAP_MAX_LEN // L)
        p = np.pad(np.concatenate([c, np.zeros(R.CLAP_MAX_LEN - c.size)]), 512, mode="reflect")
        fr = (R._frames(p, R.CLAP_HOP, 11).astype(np.float32) * win.astype(np.float32)).astype(np.float32)
        Y = sfft.rfft(fr, axis=-1)
        assert Y.dtype == np.complex64
        pw = (Y.real * Y.real + Y.imag * Y.imag).astype(np.float32)
        second = (pw @ htk_bank().astype(np.float32).T).astype(np.float64)
        e_l2, f_l2, e_max, f_max = R.floor_ratios(torch.from_numpy(second), torch.from_numpy(ex["lin"][0]), torch.from_numpy(rd["lin"][0]))
        spread.append((L, e_l2 / f_l2, e_max / f_max))
        assert R.accepts(torch.from_numpy(second), torch.from_numpy(ex["lin"][0]), torch.from_numpy(rd["lin"][0])), spread[-1]
    print("second float32 FFT / floor (L, l2, max):", [(L, round(a, 3), round(b, 3)) for L, a, b in spread])


# ---- draws -----------------------------------------------------------------------------------------------------------------------
def test_log_mel_draws_are_judged_on_the_reference_alone():
    win = R.periodic_hann()
    for bank in (htk_bank(), slaney48_bank()):
        for L in R.CLAP_LS:
            w = clap_wave(L, "noise")
            ref = R.with_floor(R.clap_log_mel(w, [L], R.CLAP_MAX_LEN, R.CLAP_HOP, win, bank),
                               R.clap_log_mel(w, [L], R.CLAP_MAX_LEN, R.CLAP_HOP, win, bank, rounded=True), "db")
            ratio, share = R.log_ratio(ref["rounded_log"][0], ref, 0, DB)
            assert ratio <= 1.0, (L, ratio)
            assert (share >= R.SHARE) == (L not in R.CLAP_LINE_LS), (L, share)
            if L == 2401:
                assert not ref["live"][0, 8:].any() and ref["live"][0, :6].all()       # the zero tail from rep_end on, reflected
                assert (ref["log"][0, 8:] == -100.0).all() and (ref["rounded_log"][0, 8:] == -100.0).all()
    for T_ in R.LOG_MEL_TS:
        w = R.noise_tones(T_, T_, 16000).astype(np.float64)[None]
        ref = R.with_floor(R.log_mel(w, 160, 8, win, slaney16_bank()), R.log_mel(w, 160, 8, win, slaney16_bank(), rounded=True), "ln")
        ratio, share = R.log_ratio(ref["rounded_log"][0], ref, 0, 1.0)
        assert ratio <= 1.0 and share >= R.SHARE, (T_, ratio, share)
    z = R.log_mel(np.zeros((1, 600)), 160, 8, win, slaney16_bank(), rounded=True)
    assert (z["log"][0, :3] == np.float64(np.float32(math.log(np.float32(1e-5))))).all() and not z["log"][0, 3:].any()
    z = R.clap_log_mel(np.zeros((1, 4800)), [4800], 4800, 480, win, htk_bank(), rounded=True)
    assert (z["log"] == -100.0).all()


@pytest.mark.parametrize("C", R.AFF_CS)
def test_aff_draw_ladder(C):
    B = 1 if C == 2048 else 3
    h, r, loc, glob = R.aff_draw(B, C)
    ref = R.aff_sum_pool(h, r)
    p = ref["pooled"]
    assert (np.abs(p) > 20 * ref["pooled_bound"]).all()                     # every channel mean far above its bound
    assert (np.abs(np.diff(p, axis=1)) > 20 * ref["pooled_bound"][:, 1:]).all()             # and distinct from its neighbour's
    if B > 1:
        assert (np.abs(p[0] - p[1]) > 20 * ref["pooled_bound"][0]).all()
    assert R.pool_chain(C) == {8: 272, 48: 140, 96: 217, 128: 272, 2048: 4097}[C]
    assert (256 % (C // 8) == 0) == (C in (8, 128, 2048))


@pytest.mark.parametrize("H,W,shift,draw,heads,B,padded", R.window_cases())
def test_window_draws(H, W, shift, draw, heads, B, padded):
    if draw == "diffuse":
        return
    qkv, bias = R.window_draw(draw, B, H, W, heads, shift)
    ref = R.window_attention(qkv, B, H, W, heads, shift, bias, want=("out", "weights"))
    wts, s0 = ref["weights"], ref["scores"]
    reg = ref["regions"].repeat(B, 1)
    if draw == "peaked":
        tgt = R.peaked_targets(H, W, shift).repeat(B, 1)
        w_t = torch.gather(wts, 3, tgt[:, None, :, None].expand(-1, heads, -1, 1))[..., 0]
        assert float(w_t.min()) >= 0.5                                      # every query's target is its dominant key
        assert bool((torch.gather(reg, 1, tgt) == reg).all())               # and lies in its region
        for w in range(reg.shape[0]):                                      # the targets cover every corner of every region
            r2 = reg[w].view(8, 8)
            hit = set(tgt[w].tolist())
            for rid in r2.unique().tolist():
                ys, xs = (r2 == rid).nonzero(as_tuple=True)
                for y in (int(ys.min()), int(ys.max())):
                    for x in (int(xs.min()), int(xs.max())):
                        assert y * 8 + x in hit
    else:
        other = reg != reg[:, 63:64]                                        # queries outside key 63's region
        assert bool(other.any()) == (reg.unique().numel() > 1)
        own = (reg[:, :, None] == reg[:, None, :])[:, None].expand_as(s0)
        lead = s0[..., 63] - torch.where(own, s0, torch.full_like(s0, -1e9)).max(-1)[0]
        o = other[:, None].expand_as(lead)
        if bool(o.any()):
            assert float(lead[o].min()) >= 85.0                             # it outweighs every true key before the mask
            w63 = wts[..., 63][o]
            assert float(w63.max()) < 0.05 and float(w63.min()) > 1e-5      # and is left a visible ~e^-5 after it


# ---- mutants ---------------------------------------------------------------------------------------------------------------------
def strongest(got, exact, bnd=None, rounded=None):
    r = []
    if bnd is not None:
        r.append(R.elem_ratio(got, exact, bnd))
    if rounded is not None:
        e_l2, f_l2, e_max, f_max = R.floor_ratios(torch.from_numpy(got), torch.from_numpy(exact), torch.from_numpy(rounded))
        r += [e_l2 / (2 * f_l2) if f_l2 else math.inf * (e_l2 > 0), e_max / (4 * f_max) if f_max else math.inf * (e_max > 0)]
    return max(x for x in r if x == x)


def lin_strongest(got_log, ref, b=0):
    r_l2, r_max = R.lin_ratios(got_log, ref, b)
    return max(r_l2 / 2.0, r_max / 4.0)


def test_resampler_mutants():
    x, xf = R.resample_draw(), R.resample_draw(finite_tail=True)
    y, S, Kn = R.resample_up3(x, R.RESAMPLE_LENS, TAPS32)
    bnd = R.resample_bound(S, Kn)
    y32 = np.zeros_like(y)                                                  # "rounded": the same sum in fp32, sample by sample
    for b, L in enumerate(R.RESAMPLE_LENS):
        u = np.zeros(3 * L, dtype=np.float32)
        u[::3] = x[b, :L].astype(np.float32)
        y32[b, :3 * L] = np.convolve(u, TAPS32.astype(np.float32))[30:30 + 3 * L]
    assert R.elem_ratio(y32, y, bnd) <= 1.0
    for m in R.RESAMPLE_MUTANTS:
        ym = R.resample_up3(xf, R.RESAMPLE_LENS, TAPS32, mutant=m)[0]
        ratio = R.elem_ratio(ym, y, bnd)
        print(f"resampler {m}: {ratio:.3g}")
        assert ratio > 1.0, m
        for b in range(1, 5):                                              # every clip shorter than the row rejects it on its own
            assert R.elem_ratio(ym[b:b + 1], y[b:b + 1], bnd[b:b + 1]) > 1.0, (m, b)


def tone_on_bin(L, k):
    t = np.arange(L)
    return (0.5 * np.sin(2 * np.pi * k * t / 1024.0)).astype(np.float32)


def test_clap_log_mel_mutants():
    win = R.periodic_hann()
    recorded = []
    for name, bank in (("htk", htk_bank()), ("slaney", slaney48_bank())):
        for L in R.CLAP_LS:
            w = clap_wave(L, "noise")
            args = (w, [L], R.CLAP_MAX_LEN, R.CLAP_HOP, win, bank)
            ex, rd = R.clap_log_mel(*args), R.clap_log_mel(*args, rounded=True)
            ref = R.with_floor(ex, rd, "db")
            assert lin_strongest(rd["log"][0], ref) <= 1.0
            for m in R.CLAP_MEL_MUTANTS:
                mu = R.clap_log_mel(*args, rounded=True, mutant=m)
                if np.array_equal(mu["lin"], rd["lin"]):
                    assert (m, L) in {("ceil_rep", 4800), ("ceil_rep", 2400), ("ceil_rep", 1600), ("ceil_rep", 1), ("tail_kept", 4800),
                                      ("tail_kept", 2400), ("tail_kept", 1600), ("tail_kept", 1), ("symmetric", 1)}, (m, L)
                    continue                                               # max_len is a whole number of clips (or the clip one sample): nothing to differ in
                ratio = max(lin_strongest(mu["log"][0], ref), R.log_ratio(mu["log"][0], ref, 0, DB)[0])
                if ratio <= 1.0:
                    recorded.append((name, L, m, ratio))
                else:
                    print(f"clap log-mel {name} L {L} {m}: {ratio:.3g}")
    # what the comparators cannot reject by construction: a one-sample clip is a constant, its spectrum is the window's (bins 0 and 1),
    # and no Slaney filter's top bin lies there.  Every other mutant must be rejected at every L where it differs.
    print("recorded (accepted) clap log-mel mutants:", recorded)
    assert all((L, m) == (1, "short_range") for _, L, m, _ in recorded), recorded
    # the short mel range: a tone centred on the bin a filter loses
    for name, bank in (("htk", htk_bank()), ("slaney", slaney48_bank())):
        top = int(np.nonzero(bank[40])[0].max())
        w = tone_on_bin(4800, top)[None].astype(np.float64)
        args = (w, [4800], R.CLAP_MAX_LEN, R.CLAP_HOP, win, bank)
        ex, rd, mu = R.clap_log_mel(*args), R.clap_log_mel(*args, rounded=True), R.clap_log_mel(*args, rounded=True, mutant="short_range")
        ref = R.with_floor(ex, rd, "db")
        ratio = max(lin_strongest(mu["log"][0], ref), R.log_ratio(mu["log"][0], ref, 0, DB)[0])
        print(f"clap log-mel {name} short_range on a tone at bin {top}: {ratio:.3g}")
        assert ratio > 1.0


def test_log_mel_mutants():
    win, bank = R.periodic_hann(), slaney16_bank()
    for T_ in R.LOG_MEL_TS:
        w = R.noise_tones(T_, T_, 16000).astype(np.float64)[None]
        ex, rd = R.log_mel(w, 160, 8, win, bank), R.log_mel(w, 160, 8, win, bank, rounded=True)
        ref = R.with_floor(ex, rd, "ln")
        for m in R.LOG_MEL_MUTANTS:
            mu = R.log_mel(w, 160, 8, win, bank, rounded=True, mutant=m)
            if m == "log_pad":
                differs = ex["n_frames"] < 8
                assert differs == (not np.array_equal(mu["log"], rd["log"]))
                if differs:
                    assert mu["log"][0, ex["n_frames"]:].any()              # the GPU file asserts exact zeros there
                continue
            if m == "pad512" and mu["n_frames"] != ex["n_frames"] and mu["n_frames"] < 8:
                continue                                                    # another frame count: the zero-frame assertion sees it
            ratio = max(lin_strongest(mu["log"][0], ref), R.log_ratio(mu["log"][0], ref, 0, 1.0)[0])
            print(f"log_mel T {T_} {m}: {ratio:.3g}")
            assert ratio > 1.0, (T_, m)


def test_input_mutants():
    recorded = []
    for T_ in R.INPUT_TS:
        mel, sc, sh = R.input_draw(T_)
        ex, rd = R.clap_input(mel, sc, sh), R.clap_input(mel, sc, sh, rounded=True)
        for k in ("g", "l"):
            assert R.elem_ratio(rd[k], ex[k], ex[k + "_bound"]) <= 1.0
        for m in R.INPUT_MUTANTS:
            mu = R.clap_input(mel, sc, sh, rounded=True, mutant=m)
            ratio = max(R.elem_ratio(mu[k], ex[k], ex[k + "_bound"]) for k in ("g", "l"))
            if np.array_equal(mu["g"], rd["g"]) and np.array_equal(mu["l"], rd["l"]):
                if T_ == 1023 and m == "no_clamp":
                    recorded.append((T_, m, 0.0))                           # under bf16's resolution altogether
                    continue
                assert T_ == 1024 and m in ("a_half", "no_align", "no_clamp"), (T_, m)          # the pass-through resizes nothing
                continue
            print(f"input T {T_} {m}: {ratio:.3g}")
            if ratio <= 1.0:
                recorded.append((T_, m, ratio))
    # no_clamp at T = 1001 / 1023: align_corners puts the only out-of-range taps beside frames 0 and T - 1 under coefficients of 4e-4
    print("recorded (accepted) input mutants:", recorded)
    assert all(m == "no_clamp" and T_ in (1001, 1023) for T_, m, _ in recorded), recorded


@pytest.mark.parametrize("C", R.AFF_CS)
def test_aff_mutants(C):
    B = 1 if C == 2048 else 3
    longer = [1] if B == 1 else [1, 0, 1]
    h, r, loc, glob = R.aff_draw(B, C)
    assert np.isfinite(r).all()                                             # (the GPU file puts NaN at column 63 of r)
    ex, rd = R.aff_sum_pool(h, r), R.aff_sum_pool(h, r, rounded=True)
    assert R.elem_ratio(rd["pooled"], ex["pooled"], ex["pooled_bound"]) <= 1.0
    for m in ("col63_used", "pool4095"):
        mu = R.aff_sum_pool(h, r, rounded=True, mutant=m)
        ratio = R.elem_ratio(mu["pooled"], ex["pooled"], ex["pooled_bound"])
        print(f"aff pool C {C} {m}: {ratio:.3g}")
        assert ratio > 1.0, m
        assert (m == "col63_used") == (not np.array_equal(mu["a"], rd["a"]))
    cx, cr = R.aff_combine(h, r, loc, glob, longer), R.aff_combine(h, r, loc, glob, longer, rounded=True)
    fused = np.asarray(longer, dtype=bool)
    assert R.elem_ratio(cr["out"][fused], cx["out"][fused], cx["bound"][fused]) <= 1.0
    assert np.array_equal(cr["out"][~fused], h[~fused])
    for m in ("col63_used", "fuse_all", "glob_wrong"):
        if B == 1 and m in ("fuse_all", "glob_wrong"):
            continue                                                        # one item, fused: nothing to differ in
        mu = R.aff_combine(h, r, loc, glob, longer, rounded=True, mutant=m)
        if m == "fuse_all":
            assert not np.array_equal(mu["out"][~fused], h[~fused])
            continue
        ratio = R.elem_ratio(mu["out"][fused], cx["out"][fused], cx["bound"][fused])
        print(f"aff combine C {C} {m}: {ratio:.3g}")
        assert ratio > 1.0, m


WINDOW_LOG = []


@pytest.mark.parametrize("H,W,shift,draw,heads,B,padded", R.window_cases())
def test_window_mutants(H, W, shift, draw, heads, B, padded):
    judge_window_case(H, W, shift, draw, heads, B, padded)


def judge_window_case(H, W, shift, draw, heads, B, padded):
    qkv, bias = R.window_draw(draw, B, H, W, heads, shift)
    ex = R.window_attention(qkv, B, H, W, heads, shift, bias)
    rd = R.window_attention(qkv, B, H, W, heads, shift, bias, rounded=True)
    assert strongest(rd["out"], ex["out"], ex["bound"], rd["out"]) <= 1.0
    for m in R.WINDOW_MUTANTS:
        mu = R.window_attention(qkv, B, H, W, heads, shift, bias, rounded=True, mutant=m)
        if np.array_equal(mu["out"], rd["out"]):
            assert shift == 0 or (m == "w_for_h" and H == W) or (m == "thr_m1" and shift == 7) or m == "mask_inf" or \
                (m in ("mask_unrolled", "roll_back_neg") and (H, W, shift) == (8, 8, 4)), (m, H, W, shift, draw)   # one window, halves exchanged: the same partition; -4 = +4 mod 8
            continue
        ratio = strongest(mu["out"], ex["out"], ex["bound"], rd["out"])
        old = R.old_window_close(torch.from_numpy(mu["out"]), torch.from_numpy(ex["out"]))
        WINDOW_LOG.append((m, (H, W, shift, draw), ratio, old))
        if m == "mask_inf" and draw != "cross":
            continue                                                        # e^-100 is not a visible weight: the cross draw is for this
        if m == "bias_T" and draw != "diffuse":
            continue                                                        # a peaked softmax hides a bias of 0.5: the diffuse draw is for this
        assert ratio > 1.0, (m, H, W, shift, draw, ratio)


def test_window_mutants_summary():
    """every window mutant is rejected at some GPU-file shape; the old comparator's verdicts are printed, not asserted"""
    if not WINDOW_LOG:                                                      # run on its own: judge the cases here
        for c in R.window_cases():
            judge_window_case(*c)
    for m in R.WINDOW_MUTANTS:
        rows = [r for r in WINDOW_LOG if r[0] == m]
        judged = [r for r in rows if not (m == "mask_inf" and r[1][3] != "cross") and not (m == "bias_T" and r[1][3] != "diffuse")]
        assert judged and min(r[2] for r in judged) > 1.0, m
        print(f"window {m}: rejected at {len(judged)} shapes, weakest ratio {min(r[2] for r in judged):.3g}; "
              f"old comparator accepts it at {sum(r[3] for r in rows)} of {len(rows)}")


def test_merge_and_mean_mutants():
    for (B, H, W, C) in R.MERGE_CASES:
        x = R.r16(np.random.default_rng(C).standard_normal((B * H * W, C)))
        assert not np.array_equal(R.patch_merge_gather(x, B, H, W, C, mutant="swapped"), R.patch_merge_gather(x, B, H, W, C))
    recorded = []
    for C in R.MEAN_CS:
        for N in R.MEAN_NS:
            x = R.r16(1.0 + np.random.default_rng(C + N).standard_normal((2, N, C)))
            ex, mu = R.token_mean(x), R.token_mean(x, mutant="n_minus_1")
            x32 = x.astype(np.float32)
            seq = np.zeros((2, C), dtype=np.float32)
            for t in range(N):
                seq = seq + x32[:, t]
            assert R.elem_ratio((seq / np.float32(N)).astype(np.float64), ex["mean"], ex["bound"]) <= 1.0
            if N == 1:
                assert np.array_equal(mu["mean"], ex["mean"])               # nothing to divide by: N - 1 is clamped to 1
                continue
            ratio = R.elem_ratio(mu["mean"], ex["mean"], ex["bound"])
            recorded.append((C, N, ratio))
            assert ratio > 1.0
    print("token mean n_minus_1 (C, N, ratio):", [(c, n, round(r, 1)) for c, n, r in recorded])
