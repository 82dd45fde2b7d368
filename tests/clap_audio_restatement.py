"""Test helper: float64 restatements of the nine kernels of csrc/clap_audio.hip and csrc/mel.hip, written from the formulas and the
docstrings of include/aldm_hip.h, transformers' ClapFeatureExtractor / ClapAudioEncoder and the reference's mel_spectrogram_train,
not from the kernels.

Every op comes as `exact` (float64, nothing rounded) and `rounded` (`rounded=True`: the same body with a rounding at the points where
the kernel's contract rounds); a `mutant=` argument computes a deliberately wrong variant (host test only).  Inputs are
bf16-representable where the kernel takes bf16 and fp32-representable where it takes fp32.

Comparators:
  check_elem   ops with a derived per-element bound: finite and max |got - exact| / bound <= 1
  check        section 16's floor rule (2 x the L2 floor, 4 x the max floor) against `rounded`: window attention
  check_lin    the same two conditions on the linear mel of the two log-mels, per clip, taken back from the fp32 logarithm the kernel
               writes; the floor is the float32 radix-4 FFT of `rounded` (measured on this reference) and the output format's
               rounding (with_floor)
  check_log    the log-domain rule of the two log-mels: where a bin's exact linear value is at least JUDGE x its clip's max floor,
               |got - exact| in dB / nepers stays under what 4 x the max floor can move the logarithm, plus the fp32 log itself
  bit equality aff a = bf16(h + r), the not-longer arm, the merge gather, token_mean's bf16 output
"""
import math

import numpy as np
import torch

from bwd_restatement import MAX_MARGIN, accepts, check, floor_ratios  # noqa: F401  (section 16's comparator, re-exported)

F64 = torch.float64
U = 2.0 ** -24                  # fp32 unit roundoff
NFFT, NBINS = 1024, 513


def r16(x):
    """numpy float64 -> nearest-even bf16 -> float64"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch.bfloat16).to(F64).numpy()


def half_ulp_bf16(t):
    """2^(floor(log2 t) - 8) per element, 0 at 0: the largest distance from a value of magnitude t to the nearest bf16"""
    t = np.asarray(t, dtype=np.float64)
    _, e = np.frexp(t)
    return np.where(t > 0, np.ldexp(1.0, e - 9), 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# comparators
# ---------------------------------------------------------------------------------------------------------------------------------
def _np(got):
    return got.detach().to("cpu").to(F64).numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)


def elem_ratio(got, exact, bnd):
    got = _np(got)
    assert got.shape == exact.shape == bnd.shape, (got.shape, exact.shape, bnd.shape)
    if not np.isfinite(got).all():
        return math.inf
    err = np.abs(got - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, math.inf))   # a bound of zero admits only equality
    return float(r.max()) if r.size else 0.0


def check_elem(got, exact, bnd, what, record=None):
    if record is None:
        import conftest
        record = conftest.record
    g = _np(got)
    assert np.isfinite(g).all(), f"{what}: non-finite values"
    ratio = elem_ratio(g, exact, bnd)
    record(ratio, what + " err/bound")
    if ratio > 1.0:
        with np.errstate(divide="ignore", invalid="ignore"):
            bad = np.argwhere(np.abs(g - exact) > bnd)
        raise AssertionError(f"{what}: error {ratio:.4g} x the bound; {len(bad)} elements, first {bad[:6].tolist()}")


def bits_equal(got, want):
    g, w = _np(got), np.asarray(want, dtype=np.float64)
    return g.shape == w.shape and bool(np.array_equal(g, w))


JUDGE = 1000.0                  # a bin is judged in the log domain where exact linear >= JUDGE x its clip's max floor
SHARE = 0.9                     # of the bins of the non-silent frames of every spectrally filled draw


def log_bound(lin_exact, log_exact, max_floor, k):
    """What section 16's max condition (|got - exact| <= 4 max floor, linear) lets the logarithm move at a judged bin, plus the fp32
    logarithm: 1 ulp of logf / log10f, the rounding of its argument's clamp (none) and, in dB, the product by 10 -- 4 units of the
    result.  k = 1 (nepers) or 10 / ln 10 (dB)."""
    rel = MAX_MARGIN * max_floor / np.maximum(lin_exact, 1e-300)
    return k * -np.log1p(-np.minimum(rel, 0.5)) + 4.0 * U * np.abs(log_exact) + 1e-30


def log_ratio(got_log, ref, b, k):
    """-> (largest |got - exact| / bound over the judged bins of clip b, judged share of the bins of its non-silent frames)"""
    lin, lg, fl = ref["lin"][b], ref["log"][b], ref["floor_max"][b]
    full = ref["full"][b]                                             # frames at least half filled with non-zero samples
    judged = lin >= JUDGE * fl
    share = float(judged[full].sum()) / max(1, int(full.sum()) * lin.shape[1])
    g = _np(got_log)
    if not np.isfinite(g).all():
        return math.inf, share
    if not judged.any():
        return 0.0, share
    r = np.abs(g - lg)[judged] / log_bound(lin, lg, fl, k)[judged]
    return float(r.max()), share


def check_log(got_log, ref, b, k, what, record=None, need_share=True):
    if record is None:
        import conftest
        record = conftest.record
    ratio, share = log_ratio(got_log, ref, b, k)
    record(ratio, what + " log err/bound")
    record(share, what + " judged share")
    assert ratio <= 1.0, f"{what}: log-domain error {ratio:.4g} x the bound"
    if need_share:
        assert share >= SHARE, f"{what}: only {share:.3f} of the bins are judged"


# the comparator of test_window_attention_matches_torch as it stands: data about the past, for the host test
def old_window_close(got, want):
    got, want = got.float(), want.float()
    return float((got - want).abs().max()) < 2e-2 and float((got - want).norm() / want.norm()) < 5e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# resample_up3
# ---------------------------------------------------------------------------------------------------------------------------------
RESAMPLE_MUTANTS = ("tap_off", "len_plus", "no_tail")


def resample_up3(x, lens, taps, mutant=None):
    """y[b][n] = sum_j x[b][j] h[n + half - 3 j] over j < lens[b], n < 3 lens[b]; exactly zero from 3 lens[b] on.
    x [B, T_in] (samples past lens[b] may be anything), taps [ntaps] odd.  -> (y, S, Kn) each [B, 3 T_in]: S = sum |x h| and Kn the
    number of taps that met a sample, the terms of resample_restatement.bound.
    mutants: tap_off (h[n + half + 1 - 3 j]), len_plus (lens[b] + 1 samples count), no_tail (the filter's tail past 3 lens[b] kept)."""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(taps, dtype=np.float64)
    B, Tin = x.shape
    half = (h.size - 1) // 2
    y, S, Kn = np.zeros((B, 3 * Tin)), np.zeros((B, 3 * Tin)), np.zeros((B, 3 * Tin), dtype=np.int64)
    for b in range(B):
        L = int(lens[b]) + (1 if mutant == "len_plus" else 0)
        L = min(L, Tin)
        u = np.zeros(3 * L)
        u[::3] = x[b, :L]
        off = half + (1 if mutant == "tap_off" else 0)
        full = np.concatenate([np.convolve(u, h), np.zeros(3 * Tin + 2)])          # full[m] = sum_j x[j] h[m - 3 j]
        fabs = np.concatenate([np.convolve(np.abs(u), np.abs(h)), np.zeros(3 * Tin + 2)])
        ind = np.zeros(3 * L)
        ind[::3] = 1.0
        cnt = np.concatenate([np.convolve(ind, np.ones(h.size)), np.zeros(3 * Tin + 2)])
        n_valid = 3 * Tin if mutant == "no_tail" else 3 * L
        y[b, :n_valid] = full[off:off + n_valid]
        S[b, :n_valid] = fabs[off:off + n_valid]
        Kn[b, :n_valid] = np.rint(cnt[off:off + n_valid]).astype(np.int64)
    return y, S, Kn


def resample_bound(S, Kn):
    """resample_restatement.bound: (terms + 2) 2^-24 sum |x h| -- a length-Kn fp32 sum in any order, fused or not"""
    return (Kn + 2) * U * S + 1e-30


# ---------------------------------------------------------------------------------------------------------------------------------
# a float32 FFT for the floor: radix-4 decimation in time, the textbook recurrence
#   X[k + q N/4] = sum_{r=0..3} (-i)^(q r) w_N^(r k) F_r[k],  F_r = FFT_{N/4}(x[r::4]),  w_N = exp(-2 pi i / N)
# in complex64 with twiddles rounded from float64
# ---------------------------------------------------------------------------------------------------------------------------------
def fft4_f32(x):
    """x complex64 [..., N], N a power of 4 -> its DFT, every operation in float32"""
    x = np.asarray(x, dtype=np.complex64)
    N = x.shape[-1]
    if N == 1:
        return x
    F = [fft4_f32(x[..., r::4]) for r in range(4)]
    k = np.arange(N // 4, dtype=np.float64)
    t = [F[0]] + [(np.exp(-2j * np.pi * r * k / N).astype(np.complex64) * F[r]).astype(np.complex64) for r in (1, 2, 3)]
    j = np.complex64(1j)
    a, b = t[0] + t[2], t[0] - t[2]
    c, d = t[1] + t[3], (t[1] - t[3]) * j
    return np.concatenate([a + c, b - d, a - c, b + d], axis=-1).astype(np.complex64)


def _spectra(frames, rounded):
    """frames [..., 1024] float64 (already windowed when exact) -> complex [..., 513]"""
    if rounded:
        return fft4_f32(frames.astype(np.float32).astype(np.complex64))[..., :NBINS]
    return np.fft.rfft(frames, axis=-1)


def periodic_hann():
    """transformers' window_function(1024, "hann") / torch.hann_window(periodic=True), as the fp32 table the kernels read"""
    return np.hanning(NFFT + 1)[:-1].astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# clap_log_mel
# ---------------------------------------------------------------------------------------------------------------------------------
CLAP_MEL_MUTANTS = ("symmetric", "ceil_rep", "tail_kept", "sym_hann", "short_range")


def _frames(padded, hop, n):
    idx = hop * np.arange(n)[:, None] + np.arange(NFFT)[None, :]
    return padded[idx]


def clap_log_mel(w, lens, max_len, hop, window, basis, rounded=False, mutant=None):
    """ClapFeatureExtractor._np_extract_fbank_features over a repeatpad'ed clip.
    w [B, T] (lens[b] samples count), window [1024], basis [n_mels, 513] (the fp32 bank taken as float64).
    -> dict(lin [B, frames, n_mels] mel power, log = 10 log10(max(lin, 1e-10)), live [B, frames] bool: the frame holds a non-zero
    sample).  rounded: fp32 window product, float32 FFT, fp32 power and bank, the float64 log10 rounded to fp32 once.
    mutants: symmetric (padding mirrors the border sample too), ceil_rep (one repeat more), tail_kept (the clip keeps repeating where
    zeros belong), sym_hann (np.hanning(1024)), short_range (every filter loses its top non-zero bin)."""
    w, basis = np.asarray(w, dtype=np.float64), np.asarray(basis, dtype=np.float64)
    if mutant == "sym_hann":
        window = np.hanning(NFFT).astype(np.float32).astype(np.float64)
    if mutant == "short_range":
        basis = basis.copy()
        for m in range(basis.shape[0]):
            nz = np.nonzero(basis[m])[0]
            if nz.size:
                basis[m, nz.max()] = 0.0
    n = 1 + max_len // hop
    lin, live, full = [], [], []
    for b in range(w.shape[0]):
        L = int(lens[b])
        clip = w[b, :L]
        reps = -(-max_len // L) if mutant == "ceil_rep" else max_len // L
        if mutant == "tail_kept":
            c = np.resize(clip, max_len)
        else:
            c = np.tile(clip, reps)[:max_len]
            c = np.concatenate([c, np.zeros(max_len - c.size)])
        p = np.pad(c, NFFT // 2, mode="symmetric" if mutant == "symmetric" else "reflect")
        fr = _frames(p, hop, n)
        live.append(np.abs(fr).max(1) > 0)
        full.append((fr != 0).mean(1) >= 0.5)
        if rounded:
            X = _spectra(fr.astype(np.float32) * window.astype(np.float32), True)
            pw = (X.real * X.real + X.imag * X.imag).astype(np.float32)
            lin.append((pw @ basis.astype(np.float32).T).astype(np.float64))
        else:
            X = _spectra(fr * window, False)
            lin.append((X.real ** 2 + X.imag ** 2) @ basis.T)
    lin = np.stack(lin)
    if rounded:
        arg = np.maximum(lin.astype(np.float32), np.float32(1e-10)).astype(np.float64)       # the float64 logarithm of the fp32 power,
        lg = (10.0 * np.log10(arg)).astype(np.float32).astype(np.float64)                     # rounded once (the extractor's astype)
    else:
        lg = 10.0 * np.log10(np.maximum(lin, 1e-10))
    return dict(lin=lin, log=lg, live=np.stack(live), full=np.stack(full))


# ---------------------------------------------------------------------------------------------------------------------------------
# log_mel (csrc/mel.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
LOG_MEL_MUTANTS = ("power", "log_pad", "pad512")
CLAMP = 1e-5


def log_mel_frames(T_, hop, target):
    """frames of torch.stft(center=False) over the reflect-padded clip, cropped by pad_spec"""
    return min(target, 1 + (T_ + 2 * ((NFFT - hop) // 2) - NFFT) // hop)


def log_mel(w, hop, target_frames, window, basis, rounded=False, mutant=None):
    """mel_spectrogram_train + pad_spec: reflect pad (1024 - hop) / 2, |STFT| (magnitude), Slaney bank, log(max(., 1e-5)); frames from
    n_frames on are exactly zero; cropped at target_frames.  w [B, T].  -> dict(lin, log [B, target, n_mels], live, n_frames).
    mutants: power (|X|^2), log_pad (padded frames hold log(1e-5)), pad512 (reflect pad 512, as the CLAP front end)."""
    w, basis = np.asarray(w, dtype=np.float64), np.asarray(basis, dtype=np.float64)
    B, T_ = w.shape
    pad = 512 if mutant == "pad512" else (NFFT - hop) // 2
    n = log_mel_frames(T_, hop, target_frames)
    nm = basis.shape[0]
    lin, lg, live = np.zeros((B, target_frames, nm)), np.zeros((B, target_frames, nm)), np.zeros((B, target_frames), dtype=bool)
    full = np.zeros((B, target_frames), dtype=bool)
    if mutant == "log_pad":
        lg[:] = math.log(CLAMP)
    for b in range(B):
        p = np.pad(w[b], pad, mode="reflect")
        fr = _frames(p, hop, n)
        live[b, :n] = np.abs(fr).max(1) > 0
        full[b, :n] = (fr != 0).mean(1) >= 0.5
        if rounded:
            X = _spectra(fr.astype(np.float32) * window.astype(np.float32), True)
            mag = np.sqrt((X.real * X.real + X.imag * X.imag).astype(np.float32)).astype(np.float32)
            mag = mag * mag if mutant == "power" else mag
            lin[b, :n] = (mag @ basis.astype(np.float32).T).astype(np.float64)
            lg[b, :n] = np.log(np.maximum(lin[b, :n].astype(np.float32), np.float32(CLAMP)).astype(np.float64)).astype(np.float32)
        else:
            X = _spectra(fr * window, False)
            mag = np.abs(X)
            mag = mag * mag if mutant == "power" else mag
            lin[b, :n] = mag @ basis.T
            lg[b, :n] = np.log(np.maximum(lin[b, :n], np.float64(np.float32(CLAMP))))
    return dict(lin=lin, log=lg, live=live, full=full, n_frames=n)


def to_lin(lg, kind, n_frames=None):
    """the linear mel a logarithm stands for: 10^(dB / 10) ("db") or e^x ("ln"; frames from n_frames on are pad_spec's zeros)"""
    lg = np.asarray(lg, dtype=np.float64)
    if kind == "db":
        return 10.0 ** (lg / 10.0)
    out = np.exp(lg)
    if n_frames is not None:
        out[..., n_frames:, :] = 0.0
    return out


def half_ulp_f32(t):
    t = np.asarray(t, dtype=np.float64)
    _, e = np.frexp(t)
    return np.where(t > 0, np.ldexp(1.0, e - 25), 0.0)


def with_floor(exact, rounded, kind):
    """adds the floor of the linear mel to an exact reference.  The kernels hand over the logarithm only, rounded to fp32, so the GPU
    test takes the linear mel back from it (to_lin) and the floor has two parts, per element:
        f = |rounded lin - exact lin|            the float32 FFT, power / magnitude and bank, measured on this reference
        q = lin c half_ulp_fp32(|log|)           what the output format's rounding moves the linear value by (c = ln 10 / 10 in dB, 1 in
                                                 nepers): precision of the number format, nothing measured
    L2 floor = sqrt(sum f^2 + sum q^2 / 3) / ||lin|| (a rounding error is uniform in +-q: rms q / sqrt 3), max floor = max (f + q), per
    clip; all on the clamped linear value, which is what the logarithm carries.  Section 16's margins (2 x, 4 x) apply to these."""
    out = dict(exact)
    clamp = 1e-10 if kind == "db" else np.float64(np.float32(CLAMP))
    c = math.log(10.0) / 10.0 if kind == "db" else 1.0
    lin = np.maximum(exact["lin"], clamp)
    f = np.abs(np.maximum(rounded["lin"], clamp) - lin)
    q = lin * c * half_ulp_f32(np.abs(exact["log"]))
    if kind == "ln":
        n = exact["n_frames"]
        lin[:, n:], f[:, n:], q[:, n:] = 0.0, 0.0, 0.0                      # pad_spec's zero frames: nothing to round
    B = lin.shape[0]
    flat = lambda t: t.reshape(B, -1)
    norm = np.sqrt((flat(lin) ** 2).sum(1))
    norm = np.where(norm > 0, norm, 1.0)
    out["lin_c"] = lin
    out["floor_l2"] = np.sqrt((flat(f) ** 2).sum(1) + (flat(q) ** 2).sum(1) / 3.0) / norm
    out["floor_max"] = flat(f + q).max(1)
    out["lin_norm"] = norm
    out["rounded_log"] = rounded["log"]
    out["kind"] = kind
    return out


def lin_ratios(got_log, ref, b):
    """-> (rel L2 error / L2 floor, max error / max floor) of clip b's linear mel, taken back from the logarithm the kernel wrote"""
    g = _np(got_log)
    if not np.isfinite(g).all():
        return math.inf, math.inf
    lin = to_lin(g, ref["kind"], ref.get("n_frames"))
    err = np.abs(lin - ref["lin_c"][b])
    rat = lambda e, f: e / f if f > 0 else (0.0 if e == 0 else math.inf)
    return rat(float(np.sqrt((err ** 2).sum())) / ref["lin_norm"][b], ref["floor_l2"][b]), rat(float(err.max()), ref["floor_max"][b])


def check_lin(got_log, ref, b, what, record=None):
    """section 16's two conditions on the linear mel of clip b: 2 x the L2 floor, 4 x the max floor"""
    if record is None:
        import conftest
        record = conftest.record
    assert np.isfinite(_np(got_log)).all(), f"{what}: non-finite values"
    r_l2, r_max = lin_ratios(got_log, ref, b)
    record(r_l2, what + " l2/floor")
    record(r_max, what + " max/floor")
    assert r_l2 <= 2.0, f"{what}: rel L2 error {r_l2:.4g} x the floor (limit 2)"
    assert r_max <= MAX_MARGIN, f"{what}: max error {r_max:.4g} x the floor (limit 4)"


def noise_tones(n, seed, rate):
    """white noise at 0.3 plus two tones, fp32: fills every mel bin far above the float32 FFT's floor"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / float(rate)
    f1, f2 = rate * 0.031, rate * 0.117
    x = 0.3 * g.standard_normal(n) + 0.25 * np.sin(2 * np.pi * f1 * t + 0.3) + 0.15 * np.sin(2 * np.pi * f2 * t + 1.1)
    return x.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# clap_input
# ---------------------------------------------------------------------------------------------------------------------------------
INPUT_MUTANTS = ("a_half", "no_align", "no_clamp", "chan_perm", "col63", "khkw")
D1_SUP, D2_SUP = 1.35, 0.75       # sup |c'| of the inner (|x| <= 1) and outer (1 <= |x| <= 2) cubic pieces at A = -0.75
DD_SUP = 15.0                     # sum over the four taps of sup |c''| (4.5, 4.5, 3, 3)
COEF_ERR = 8 * U * 16.0           # a tap coefficient in fp32: at most 8 roundings of intermediates no larger than 16 (5 |A| x^2 at x = 2)


def _cubic(x, A, d=0):
    """the cubic convolution kernel (d = 0) or its derivative (d = 1) at |x| <= 2, x >= 0"""
    x = np.asarray(x, dtype=np.float64)
    if d == 0:
        inner = ((A + 2) * x - (A + 3)) * x * x + 1
        outer = ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    else:
        inner = 3 * (A + 2) * x * x - 2 * (A + 3) * x
        outer = (3 * A * x - 10 * A) * x + 8 * A
    return np.where(x <= 1, inner, outer)


def resize_1024(v, mutant=None, want_bound=False):
    """v [..., T, F] float64 -> [..., 1024, F]: torch's upsample_bicubic2d along the time axis, align_corners=True, A = -0.75, taps
    clamped to [0, T - 1]; T = 1024 passes through.  want_bound -> (value, fp32 error term without the half-ulp)."""
    Tn = v.shape[-2]
    if Tn == 1024:
        return (v, U * np.abs(v)) if want_bound else v
    A = -0.5 if mutant == "a_half" else -0.75
    t = np.arange(1024, dtype=np.float64)
    real = (t + 0.5) * Tn / 1024.0 - 0.5 if mutant == "no_align" else t * (Tn - 1) / 1023.0
    i0 = np.floor(real)
    u = real - i0
    xs = [u + 1, u, 1 - u, 2 - u]
    sgn = [-1.0, -1.0, 1.0, 1.0]                                          # d|x_k| / du
    out, mag, dv, cerr, ymax = 0.0, 0.0, 0.0, 0.0, 0.0
    for k in range(4):
        ti = (i0 - 1 + k).astype(np.int64)
        inside = (ti >= 0) & (ti <= Tn - 1)
        y = v[..., np.clip(ti, 0, Tn - 1), :]
        if mutant == "no_clamp":
            y = y * inside[:, None]
        c = _cubic(xs[k], A)[:, None]
        out = out + c * y
        mag = mag + np.abs(c * y)
        dv = dv + (sgn[k] * _cubic(xs[k], A, 1))[:, None] * y
        cerr = cerr + np.abs(y)
        ymax = np.maximum(ymax, np.abs(y))
    if not want_bound:
        return out
    du = (2.0 * U * real)[:, None]                                        # tscale = fl((T-1)/1023), real = fl(tscale t): two roundings
    e32 = U * mag + COEF_ERR * cerr + 4 * U * mag + np.abs(dv) * du + 0.5 * DD_SUP * du * du * ymax
    return out, e32


def clap_input(mel, bn_scale, bn_shift, rounded=False, mutant=None):
    """BatchNorm per mel bin (y = mel scale + shift), bicubic resize of T frames to 1024, reshape_mel2img (image row k 64 + f, column
    t - 256 k for frame t in chunk k), then the im2col rows of the two patch convolutions:
        g[b, h, w, kh 4 + kw]  = img_0[4 h + kh, 4 w + kw]
        l[b, h, w, kh 12 + kw] = img_{1 + c}[4 h + kh, 12 j + kw]   at token column w = c 21 + j < 63;  column 63 is zero
    mel [B, C, T, 64], C = 1 or 4.  -> dict(g, l or None, g_bound, l_bound): bound = e32 + half_ulp_bf16(|exact| + e32).
    mutants: a_half, no_align, no_clamp (resize), chan_perm (local channel c reads image 1 + (c + 1) % 3), col63 (column 63 repeats
    column 62), khkw (kernel row and column exchanged in both im2col layouts)."""
    mel = np.asarray(mel, dtype=np.float64)
    B, C = mel.shape[:2]
    y = mel * np.asarray(bn_scale, dtype=np.float64) + np.asarray(bn_shift, dtype=np.float64)
    v, e32 = resize_1024(y, mutant, want_bound=True)                       # [B, C, 1024, 64]; the BatchNorm's fma is the U * mag term

    def img(a):                                                            # [B, C, 1024, 64] -> [B, C, 256 rows, 256 cols]
        return a.reshape(B, C, 4, 256, 64).transpose(0, 1, 2, 4, 3).reshape(B, C, 256, 256)

    def rows_g(a):
        p = a[:, 0].reshape(B, 64, 4, 64, 4)                               # [b, h, kh, w, kw]
        p = p.transpose(0, 1, 3, 4, 2) if mutant == "khkw" else p.transpose(0, 1, 3, 2, 4)
        return p.reshape(B, 64, 64, 16)

    def rows_l(a):
        out = np.zeros((B, 64, 64, 48))
        for c in range(3):
            src = 1 + ((c + 1) % 3 if mutant == "chan_perm" else c)
            p = a[:, src, :, :252].reshape(B, 64, 4, 21, 12)               # [b, h, kh, j, kw]
            p = p.transpose(0, 1, 3, 4, 2) if mutant == "khkw" else p.transpose(0, 1, 3, 2, 4)
            out[:, :, 21 * c:21 * c + 21] = p.reshape(B, 64, 21, 48)
        if mutant == "col63":
            out[:, :, 63] = out[:, :, 62]
        return out

    iv, ie = img(v), img(e32)
    res = {}
    for name, fn in (("g", rows_g), ("l", rows_l)):
        if name == "l" and C != 4:
            res["l"], res["l_bound"] = None, None
            continue
        val, err = fn(iv), fn(ie)
        res[name + "_bound"] = err + half_ulp_bf16(np.abs(val) + err)
        res[name] = r16(val) if rounded else val
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# attentional feature fusion
# ---------------------------------------------------------------------------------------------------------------------------------
AFF_MUTANTS = ("col63_used", "pool4095", "fuse_all", "glob_wrong")


def _r0(r, mutant=None):
    """the local branch as the fusion sees it: zero at token column 63 (the padding of the 63 local columns)"""
    r = np.array(r, dtype=np.float64)
    if mutant != "col63_used":
        r.reshape(r.shape[0], 64, 64, -1)[:, :, 63] = 0.0
    return r


def pool_chain(C):
    """the longest addition chain of aff_sum_pool's striped fp32 sum: 256 / (C / 8) stripes (whole part) of every stripes-th token,
    then the stripes in order"""
    stripes = 256 // (C // 8)
    return -(-4096 // stripes) + stripes


def aff_sum_pool(h, r, rounded=False, mutant=None):
    """a = h + r (r zero at column 63), pooled = mean over the 4096 tokens.  h, r [B, 4096, C] bf16-representable.
    -> dict(a, pooled, pooled_bound).  rounded: a = bf16(h + r) (the kernel must match it bit for bit), pooled = bf16(mean of the
    unrounded sums).  mutants: col63_used, pool4095 (the last token left out)."""
    h = np.asarray(h, dtype=np.float64)
    a = h + _r0(r, mutant)
    C = a.shape[2]
    if mutant == "pool4095":
        pooled = a[:, :4095].sum(1) / 4095.0
    else:
        pooled = a.sum(1) / 4096.0
    e32 = (pool_chain(C) + 1) * U * np.abs(a).sum(1) / 4096.0               # + 1: the fp32 sum h + r itself
    bnd = e32 + half_ulp_bf16(np.abs(pooled) + e32)
    return dict(a=r16(a) if rounded else a, pooled=r16(pooled) if rounded else pooled, pooled_bound=bnd)


def aff_combine(h, r, loc, glob, longer, rounded=False, mutant=None):
    """out = 2 h f + 2 r (1 - f), f = sigmoid(loc + glob[b]) where longer[b] (r zero at column 63); out = h otherwise (bit-exact).
    h, r [B, 4096, C]; loc fp32 [B, 4096, C]; glob fp32 [B, C].  -> dict(out, bound) (bound 0 where not longer).
    mutants: col63_used, fuse_all (not-longer items fused too), glob_wrong (glob of item b + 1)."""
    h, loc, glob = (np.asarray(t, dtype=np.float64) for t in (h, loc, glob))
    r0 = _r0(r, mutant)
    B = h.shape[0]
    gl = np.roll(glob, -1, axis=0) if mutant == "glob_wrong" else glob
    x = loc + gl[:, None, :]
    f = 1.0 / (1.0 + np.exp(-x))
    fused = 2.0 * h * f + 2.0 * r0 * (1.0 - f)
    # f in fp32: the argument's rounding moves it by f (1 - f) U |x|; expf (2 units), 1 + e, the division: 6 U f.  1 - f: U more.
    df = f * (1.0 - f) * U * np.abs(x) + 6 * U * f + U
    e32 = (2 * np.abs(h) + 2 * np.abs(r0)) * df + 4 * U * (np.abs(2 * h * f) + np.abs(2 * r0 * (1 - f)))
    bnd = e32 + half_ulp_bf16(np.abs(fused) + e32)
    lg = np.ones(B, dtype=bool) if mutant == "fuse_all" else np.asarray(longer).astype(bool).reshape(B)
    out = np.where(lg[:, None, None], r16(fused) if rounded else fused, h)
    return dict(out=out, bound=np.where(lg[:, None, None], bnd, 0.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# shifted-window attention
# ---------------------------------------------------------------------------------------------------------------------------------
WINDOW_MUTANTS = ("mask_inf", "mask_unrolled", "thr_m1", "roll_back_neg", "bias_T", "w_for_h")
WIN, HD = 8, 24
MASK = -100.0


def region_map(H, W, shift, mutant=None):
    """transformers' img_mask: a counter over the slices (0, -8), (-8, -shift), (-shift, None) of both axes of the rolled frame"""
    img = torch.zeros(H, W, dtype=torch.long)
    s1 = shift + 1 if mutant == "thr_m1" else shift
    Hh = W if mutant == "w_for_h" else H
    cnt = 0
    for hs in (slice(0, Hh - WIN), slice(Hh - WIN, Hh - s1), slice(Hh - s1, None)):
        for ws in (slice(0, W - WIN), slice(W - WIN, W - s1), slice(W - s1, None)):
            img[hs, ws] = cnt
            cnt += 1
    if mutant == "mask_unrolled":
        img = torch.roll(img, (shift, shift), (0, 1))                      # the regions of image coordinates, not of the rolled frame
    return img


def _partition(x, B, H, W):
    """[B, H, W, c] -> [B * windows, 64, c]"""
    c = x.shape[-1]
    return x.view(B, H // WIN, WIN, W // WIN, WIN, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, WIN * WIN, c)


def _reverse(w, B, H, W):
    c = w.shape[-1]
    return w.view(B, H // WIN, W // WIN, WIN, WIN, c).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, c)


def window_attention(qkv, B, H, W, heads, shift, bias, rounded=False, mutant=None, want=("out",)):
    """ClapAudioLayer's attention: roll(-shift), window partition, softmax(q k / sqrt(24) + bias + mask) v per head, window reverse,
    roll(+shift).  mask: -100 between tokens of different regions of the rolled frame (shift > 0 only).
    qkv [B * H * W, 3 C] float64 torch (Q | K | V), bias [heads, 64, 64].  -> dict(out [B * H * W, C], bound, weights [nW, heads, 64,
    64] and scores before the mask when asked).  rounded: out = bf16(sum p v / sum p).
        bound = (n 2^-24 + e_exp) A + half_ulp_bf16(|exact| + that),  A = sum p |v| / sum p,  n = 64 + 24 + 2
        e_exp = 28 2^-24 (max_k (sum_j |q_j k_j| / sqrt(24) + |bias| + |mask|) + |max score|) + 2^-23        per query
    (28: the 24 fmas of one score, q's product with the scale, the bias, the mask, the subtraction of the maximum.)"""
    C = heads * HD
    scale = 1.0 / math.sqrt(HD)
    x = qkv.to(F64).view(B, H, W, 3 * C)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    win = _partition(x, B, H, W)
    nW = win.shape[0]
    q, k, v = (win[..., i * C:(i + 1) * C].reshape(nW, 64, heads, HD).transpose(1, 2) for i in range(3))
    bs = bias.to(F64)
    bs = bs.transpose(-1, -2) if mutant == "bias_T" else bs
    s0 = q @ k.transpose(-1, -2) * scale + bs[None]
    sabs = q.abs() @ k.abs().transpose(-1, -2) * scale + bs.abs()[None]
    s = s0
    if shift:
        reg = _partition(region_map(H, W, shift, mutant)[None, :, :, None].to(F64), 1, H, W)[..., 0]      # [windows per image, 64]
        differ = reg[:, None, :] != reg[:, :, None]
        m = torch.where(differ, -math.inf if mutant == "mask_inf" else MASK, 0.0).to(F64)
        m = m.repeat(B, 1, 1)[:, None]
        s = s0 + m
        sabs = sabs + torch.where(differ, -MASK, 0.0).to(F64).repeat(B, 1, 1)[:, None]
    mx = s.max(-1, keepdim=True)[0]
    p = torch.exp(s - mx)
    l = p.sum(-1, keepdim=True)
    o = (p @ v) / l
    A = (p @ v.abs()) / l
    e_exp = 28 * U * (sabs.max(-1, keepdim=True)[0] + mx.abs()) + 2.0 ** -23
    b32 = ((64 + 24 + 2) * U + e_exp) * A

    def back(t):
        t = _reverse(t.transpose(1, 2).reshape(nW, 64, C), B, H, W)
        if shift:
            t = torch.roll(t, (-shift, -shift) if mutant == "roll_back_neg" else (shift, shift), (1, 2))
        return t.reshape(B * H * W, C)

    o, b32 = back(o).numpy(), back(b32).numpy()
    res = dict(out=r16(o) if rounded else o, bound=b32 + half_ulp_bf16(np.abs(o) + b32))
    if "weights" in want:
        res["weights"], res["scores"] = p / l, s0
        res["regions"] = _partition(region_map(H, W, shift)[None, :, :, None].to(F64), 1, H, W)[..., 0].long() if shift else \
            torch.zeros(nW // B, 64, dtype=torch.long)
    return res


# draws.  Control coordinates 18..23 of every head carry a +-1 code of the window-local key index (bit t of j -> coordinate 18 + t),
# the other 18 are noise: a query that carries the code of key j scores 6 a b / sqrt(24) on it and at most 4 a b / sqrt(24) elsewhere.
PEAK_Q, PEAK_K = 4.0, 3.75          # 15 / sqrt(24) = 3.06 per agreeing bit: the target key leads every other by >= 6.1
CROSS_Q, CROSS_K = 16.0, 29.0       # 464 / sqrt(24) = 94.7 on one coordinate


def _local_regions(H, W, shift):
    return _partition(region_map(H, W, shift)[None, :, :, None].to(F64), 1, H, W)[..., 0].long() if shift else \
        torch.zeros((H // WIN) * (W // WIN), 64, dtype=torch.long)


def peaked_targets(H, W, shift):
    """[windows, 64]: every query's dominant key -- its own position reflected through the centre of its region's part of the window,
    so the corners of every region (the window's corners, and both sides of every region border) are each some query's target."""
    reg = _local_regions(H, W, shift)
    tgt = torch.zeros_like(reg)
    for w in range(reg.shape[0]):
        r2 = reg[w].view(8, 8)
        for i in range(64):
            y, x = divmod(i, 8)
            rows = (r2[:, x] == r2[y, x]).nonzero().flatten()
            cols = (r2[y, :] == r2[y, x]).nonzero().flatten()
            tgt[w, i] = int(rows[0] + rows[-1] - y) * 8 + int(cols[0] + cols[-1] - x)
    return tgt


def _to_rows(t, B, H, W, shift):
    """[B * windows, 64, c] in the rolled frame -> token-major rows of the image"""
    t = _reverse(t, B, H, W)
    if shift:
        t = torch.roll(t, (shift, shift), (1, 2))
    return t.reshape(B * H * W, -1)


def window_draw(kind, B, H, W, heads, shift, seed=0):
    """-> (qkv [B * H * W, 3 C] bf16-representable float64, bias fp32-representable [heads, 64, 64]).
    diffuse: test_window_attention_matches_torch's draw.  peaked: one dominant key per query (peaked_targets).  cross: key 63 of every
    window scores CROSS_Q CROSS_K / sqrt(24) = 94.7 over the others for every query -- masked by -100 it keeps a weight of about e^-5
    beside the keys of the query's own region, and its V row is 16 x the others'."""
    g = torch.Generator().manual_seed(seed + 1000 * H + 10 * W + shift + 7 * heads + 100000 * B + {"diffuse": 0, "peaked": 1, "cross": 2}[kind])
    C = heads * HD
    nW = B * (H // WIN) * (W // WIN)
    bias = (torch.randn(heads, 64, 64, generator=g) * 0.5).to(torch.float32).to(F64)
    amp = 1.5 if kind == "diffuse" else 0.5
    q, k, v = (torch.randn(nW, 64, heads, HD, generator=g, dtype=F64) * amp for _ in range(3))
    if kind == "peaked":
        tgt = peaked_targets(H, W, shift).repeat(B, 1)                      # [nW, 64]
        bits = lambda idx: ((idx[..., None] >> torch.arange(6)) & 1).to(F64) * 2 - 1
        q[..., 18:] = (PEAK_Q * bits(tgt))[:, :, None, :]
        k[..., 18:] = (PEAK_K * bits(torch.arange(64)))[None, :, None, :]
    if kind == "cross":
        q[..., 18:], k[..., 18:] = 0.0, 0.0
        q[..., 23] = CROSS_Q
        k[:, 63, :, 23] = CROSS_K
        v[:, 63] *= 16.0
    rows = torch.cat([_to_rows(t.reshape(nW, 64, C), B, H, W, shift) for t in (q, k, v)], 1)
    return rows.to(torch.bfloat16).to(F64), bias


def window_cases():
    """(H, W, shift, draw, heads, B, padded): every image size x shift x draw, with heads (1, 2, 3), B (1, 3) and the padded strides
    (ld = 3 C + 8, ld_out = C + 8) rotating so that every value meets every size, shift and draw somewhere."""
    out, i = [], 0
    for (H, W) in WINDOW_HW:
        for shift in WINDOW_SHIFTS:
            for draw in ("diffuse", "peaked", "cross"):
                if draw == "cross" and shift == 0:
                    continue                                               # no mask to cross
                out.append((H, W, shift, draw, (1, 2, 3)[i % 3], (1, 3)[(i // 3) % 2], bool((i // 2) % 2)))
                i += 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_clap_audio_edges.py (the host test rejects every mutant at these)
# ---------------------------------------------------------------------------------------------------------------------------------
RESAMPLE_TIN, RESAMPLE_LENS = 300, (300, 299, 1, 20, 21)
CLAP_MAX_LEN, CLAP_HOP = 4800, 480
CLAP_LS = (4800, 4799, 2400, 2401, 1600, 513, 511, 7, 1)
CLAP_LINE_LS = (7, 1)             # a clip of 7 samples or 1, tiled, is a line spectrum: most mel bins hold nothing to judge
LOG_MEL_HOP, LOG_MEL_TARGET = 160, 8
# n_frames = 1 + (T + 864 - 1024) // 160 = T // 160: 433 is the shortest clip the reflect padding admits (2 frames; one frame cannot
# occur), 479 | 480 the 2 | 3 boundary, 1279 | 1280 the 7 | 8 boundary, 1440 the first cropped length (9 frames), 3000 far past it;
# 592, 593 (3 frames) and 1552, 1553 (9, cropped) are the lengths the issue names.
LOG_MEL_TS = (433, 479, 480, 592, 593, 1279, 1280, 1439, 1440, 1552, 1553, 3000)
INPUT_TS = (2, 3, 4, 1001, 1023, 1024)
AFF_CS = (8, 48, 96, 128, 2048)
WINDOW_HW = ((8, 8), (8, 16), (16, 8), (16, 24), (64, 64))
WINDOW_SHIFTS = (0, 1, 4, 7)
MERGE_CASES = ((2, 4, 6, 8), (1, 64, 64, 96))                              # (B, H, W, C)
MEAN_CS, MEAN_NS = (8, 40, 768), (1, 63, 64)


def resample_draw(finite_tail=False):
    """B = 5 clips of RESAMPLE_LENS samples in rows of 300; the samples past each length are NaN (finite_tail: 1.0, for the mutant that
    reads one of them)"""
    g = np.random.default_rng(5)
    x = np.clip(0.3 * g.standard_normal((len(RESAMPLE_LENS), RESAMPLE_TIN)), -1, 1).astype(np.float32).astype(np.float64)
    for b, L in enumerate(RESAMPLE_LENS):
        x[b, L:] = 1.0 if finite_tail else np.nan
    return x


def input_draw(T_, C=4, B=2, seed=0):
    """log-mel-like features [B, C, T, 64] with every (b, c, t, f) value distinct, fp32; BatchNorm scale / shift centred on them"""
    g = np.random.default_rng(seed + T_)
    n = B * C * T_ * 64
    mel = (-60.0 + 50.0 * g.permutation(n) / n).astype(np.float32).reshape(B, C, T_, 64)     # a shuffled ramp over -60 .. -10 dB
    assert np.unique(mel).size == n
    sc = (0.1 * (1.0 + 0.1 * g.standard_normal(64))).astype(np.float32)
    sh = (3.5 + 0.5 * g.standard_normal(64)).astype(np.float32)
    return mel.astype(np.float64), sc.astype(np.float64), sh.astype(np.float64)


def aff_draw(B, C, seed=0):
    """h, r [B, 4096, C] bf16-representable; the channel means of h + r form a ladder (+-(1 + c % 7) / 2 with an item-dependent start,
    noise 0.25) and the last token of h is 64 x its rung, so one token left out of the pool moves the mean by 1.5 %.  loc, glob fp32."""
    g = np.random.default_rng(seed + C + 10 * B)
    rung = ((1 + (np.arange(C)[None, :] + 3 * np.arange(B)[:, None]) % 7) / 2.0) * np.where(np.arange(C) % 2, -1.0, 1.0)[None, :]
    h = rung[:, None, :] * 0.5 + 0.25 * g.standard_normal((B, 4096, C))
    r = rung[:, None, :] * 0.5 + 0.25 * g.standard_normal((B, 4096, C))
    h[:, 4095] = 64.0 * rung
    loc = (1.5 * g.standard_normal((B, 4096, C))).astype(np.float32).astype(np.float64)
    glob = (1.0 * g.standard_normal((B, C))).astype(np.float32).astype(np.float64)
    return r16(h), r16(r), loc, glob


# ---------------------------------------------------------------------------------------------------------------------------------
# patch merging gather, token mean
# ---------------------------------------------------------------------------------------------------------------------------------
def patch_merge_gather(x, B, H, W, C, mutant=None):
    """ClapAudioPatchMerging's gather: [x0 | x1 | x2 | x3] = x[2i, 2j], x[2i+1, 2j], x[2i, 2j+1], x[2i+1, 2j+1].  Bit-exact.
    mutant swapped: [x0, x2, x1, x3]."""
    x = np.asarray(x, dtype=np.float64).reshape(B, H, W, C)
    parts = [x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]]
    if mutant == "swapped":
        parts = [parts[0], parts[2], parts[1], parts[3]]
    return np.concatenate(parts, -1).reshape(B * (H // 2) * (W // 2), 4 * C)


def token_mean(x, mutant=None):
    """x [B, N, C] -> dict(mean [B, C], bound): a sequential fp32 sum of N terms and one division, N + 1 roundings of partial sums no
    larger than sum |x|.  mutant n_minus_1: division by N - 1."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[1]
    den = float(max(N - 1, 1)) if mutant == "n_minus_1" else float(N)
    return dict(mean=x.sum(1) / den, bound=(N + 1) * U * np.abs(x).sum(1) / N + 1e-45)
