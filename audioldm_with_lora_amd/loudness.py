"""ITU-R BS.1770-4 integrated loudness (mono, channel weight 1) and loudness normalisation on the MI355X.

K-weighting at any rate fs is designed on the host in float64 the way libebur128 does it (De Man's derivation of the
recommendation's 48 kHz tables, bilinear transform with the warp K = tan(pi f0 / fs)); at 48 kHz it reproduces the printed
coefficients to better than 1e-8.  The measurement runs in csrc/loudness.hip:

    hop H = fs / 10;  e[j] = sum of y^2 over [j H, (j + 1) H), y the K-weighted signal from a zero state (complete hops only)
    block i = hops i .. i + 3:  z_i = (e_i + .. + e_{i+3}) / (4 H),  l_i = -0.691 + 10 log10 z_i
    absolute gate l_i > -70;  relative gate Gr = -0.691 + 10 log10(mean z of the absolutely gated) - 10
    L = -0.691 + 10 log10(mean of z_i with l_i > -70 and l_i > Gr),  -inf without a block above -70

    integrated_loudness(wav, 16000)                               float64 [B] in LUFS, on the device
    normalize_loudness(wav, 16000, target_lufs=-14.0)             (wav_out, {"lufs_in", "gain_db", "peak_in"})

Normalisation: gain = 10^((target - L) / 20), capped at 10^(ceiling / 20) / peak.  `peak` is an OVERSAMPLED-PEAK ESTIMATE: the
absolute maximum of the clip after `oversample`-fold interpolation through this project's own polyphase resampler (resample.py: a
Kaiser(5.0)-windowed sinc of 20 oversample + 1 taps), not the 48-tap filter of the recommendation's Annex 2; oversample=1 is the
sample peak.  The ceiling only caps the gain (no limiter); a clip of loudness -inf keeps gain 1.
"""
import math

import numpy as np
import torch

from . import _lib, ops
from . import resample as R

CHUNK = 1024              # samples per chunk of the chunked recurrence (= aldm_loudness_chunk of csrc/loudness.hip, checked at the launch)
SCAN_LEVELS = 6           # the kernel's scan over 64 chunks needs M^(2^k), k = 0 .. 5
MIN_RATE = 8000


def check_rate(fs):
    fs = R._rate(fs)
    if fs < MIN_RATE or fs % 10:
        raise ValueError(f"loudness: the sampling rate must be at least {MIN_RATE} Hz and a multiple of 10 (100 ms hops), got {fs}")
    return fs


def k_weighting(fs):
    """The two biquads of the K-weighting at fs Hz, float64: ((b, a) of the shelf, (b, a) of the high-pass), each [3] with a[0] = 1."""
    fs = check_rate(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0], dtype=np.float64)
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0], dtype=np.float64)
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)
    return (b1, a1), (b2, a2)


def state_transition(fs):
    """The 4x4 matrix A of the cascade's state (s1, s2 of the shelf, s1, s2 of the high-pass; transposed direct form II, as
    scipy.signal.lfilter keeps it) over one sample with input 0: state' = A state."""
    (b, a), (c, d) = k_weighting(fs)
    return np.array([[-a[1], 1.0, 0.0, 0.0],
                     [-a[2], 0.0, 0.0, 0.0],
                     [c[1] - d[1] * c[0], 0.0, -d[1], 1.0],
                     [c[2] - d[2] * c[0], 0.0, -d[2], 0.0]], dtype=np.float64)


_FIX = 4096               # fraction bits of the fixed-point matrix powers: A^(32 chunks) at 8 kHz is ~2^-1500, and keeps 2500 bits


def _fix_matmul(x, y):
    return [[sum(x[i][k] * y[k][j] for k in range(4)) >> _FIX for j in range(4)] for i in range(4)]


def chunk_powers(fs, chunk=CHUNK, levels=SCAN_LEVELS):
    """float64 [levels, 2, 4, 4]: M^(2^k), k = 0 .. levels - 1, with M = A^chunk the state transition over one chunk, each as a
    double-double (leading doubles, trailing doubles).  The powers are taken in integer fixed point with _FIX fraction bits, so
    every entry is the float64 A's exact power rounded once: A^chunk of the high-pass's nearly double pole is far from normal, and
    float64 repeated squaring leaves its entries with errors that are small against the matrix norm only (the kernel's hand-over
    of a decayed state needs them small against the entry)."""
    from fractions import Fraction
    one = 1 << _FIX
    a = [[int(Fraction(float(v)) * one) for v in row] for row in state_transition(fs)]      # exact: a float64 is a dyadic fraction
    n, power, base = int(chunk), None, a
    while n:
        if n & 1:
            power = base if power is None else _fix_matmul(power, base)
        n >>= 1
        if n:
            base = _fix_matmul(base, base)
    out = np.zeros((levels, 2, 4, 4), dtype=np.float64)
    for k in range(levels):
        for i in range(4):
            for j in range(4):
                v = Fraction(power[i][j], one)
                hi = float(v)
                out[k, 0, i, j], out[k, 1, i, j] = hi, float(v - Fraction(hi))
        power = _fix_matmul(power, power)
    return out


def coef_table(fs):
    """float64 [10]: {b0, b1, b2, a1, a2} of the shelf, then of the high-pass (the kernel's argument)"""
    (b, a), (c, d) = k_weighting(fs)
    return np.concatenate([b, a[1:], c, d[1:]])


class LoudnessMeter:
    """BS.1770 loudness at `rate` Hz on `device`; the coefficients and the chunk's state-transition powers stay on the device.

        m = LoudnessMeter(16000, "cuda")
        m.hop_energies(wav, lens)     float64 [B, T // H]
        m.measure(wav, lens)          float64 [B] LUFS
        m.peak(wav, lens, 4)          fp32 [B]
        m.normalize(wav, -14.0, -1.0, lens)   (wav_out, info)

    wav: fp32 [T] or [B, T] on the device.  lens: None (whole rows), a list / host tensor (checked and copied over), or an int32 device
    tensor [B] -- with the latter, or None, nothing is copied from the host and the chain can be captured in a graph."""

    def __init__(self, rate, device="cuda"):
        self.rate = check_rate(rate)
        self.hop = self.rate // 10
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AldmError("LoudnessMeter runs on the MI355X only (got a CPU device); there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.coef = torch.from_numpy(coef_table(self.rate)).to(self.device)
        self.mpow = torch.from_numpy(chunk_powers(self.rate)).contiguous().to(self.device)

    def _rows(self, wav, lens):
        if not torch.is_tensor(wav) or wav.dim() not in (1, 2) or wav.numel() == 0:
            raise ValueError("loudness: a non-empty tensor [T] or [B, T] is expected")
        ops._require_gpu(wav)
        if wav.device != self.device:
            raise ValueError(f"loudness: this meter lives on {self.device}, the waveform on {wav.device}")
        x = (wav[None] if wav.dim() == 1 else wav).to(torch.float32).contiguous()
        B, T = x.shape
        if lens is None:
            lens = torch.full((B,), T, dtype=torch.int32, device=x.device)
        elif torch.is_tensor(lens) and lens.is_cuda:
            lens = lens.to(torch.int32).reshape(-1).contiguous()
            if lens.numel() != B:
                raise ValueError(f"loudness: lens must hold {B} lengths")
        else:
            host = torch.as_tensor(lens).to("cpu", torch.int32).reshape(-1)
            if host.numel() != B or int(host.min()) < 0 or int(host.max()) > T:
                raise ValueError(f"loudness: lens must hold {B} lengths in [0, {T}], got {host.tolist()}")
            lens = ops._h2d(host, x.device)
        return x, lens

    def hop_energies(self, wav, lens=None):
        x, lens = self._rows(wav, lens)
        return ops.kweight_energy(x, lens, self.hop, self.coef, self.mpow, CHUNK)

    def _measure(self, x, lens):
        e = ops.kweight_energy(x, lens, self.hop, self.coef, self.mpow, CHUNK)
        return ops.loudness_gate(e, lens, x.shape[1], self.hop)

    def measure(self, wav, lens=None):
        """integrated loudness in LUFS: float64 [B] on the device, -inf for a clip without a 400 ms block above -70"""
        return self._measure(*self._rows(wav, lens))

    def _peak(self, x, lens, oversample):
        oversample = int(oversample)
        if oversample < 1:
            raise ValueError(f"loudness: oversample must be at least 1, got {oversample}")
        if oversample == 1:
            return ops.peak_abs(x, lens)
        R.check_ratio(oversample, 1)
        up = ops._resample_poly_rows(x, oversample, 1, lens, R.device_table(oversample, 1, x.device))
        return ops.peak_abs(up, lens, lens_ratio=(oversample, 1))

    def peak(self, wav, lens=None, oversample=4):
        """the oversampled-peak estimate (module docstring): fp32 [B] on the device"""
        return self._peak(*self._rows(wav, lens), oversample)

    def normalize(self, wav, target_lufs=-14.0, peak_ceiling_dbfs=-1.0, lens=None, oversample=4):
        """(wav_out, info): every clip brought to target_lufs, the gain capped so that its peak stays at or under peak_ceiling_dbfs
        (None: no cap).  wav_out fp32, shaped like wav, zero from lens[b] on; info = {"lufs_in" float64 [B], "gain_db" float64 [B]
        (the gain really applied), "peak_in" fp32 [B]}, all on the device."""
        x, lens = self._rows(wav, lens)
        lufs = self._measure(x, lens)
        peak = self._peak(x, lens, oversample)
        y, _, gain_db = ops.loudness_gain(x, lens, lufs, peak, target_lufs, peak_ceiling_dbfs)
        return (y[0] if wav.dim() == 1 else y), {"lufs_in": lufs, "gain_db": gain_db, "peak_in": peak}


_meters = {}


def meter(rate, device):
    """the LoudnessMeter of (rate, device), built once"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(rate), device)
    if key not in _meters:
        _meters[key] = LoudnessMeter(rate, device)
    return _meters[key]


def _on_gpu(wav):
    if not torch.is_tensor(wav):
        raise ValueError("loudness: a tensor [T] or [B, T] is expected")
    ops._require_gpu(wav)


def integrated_loudness(wav, rate, lens=None):
    """BS.1770-4 integrated loudness of wav ([T] or [B, T] on the GPU) at `rate` Hz: float64 [B] on the device."""
    check_rate(rate)
    _on_gpu(wav)
    return meter(rate, wav.device).measure(wav, lens)


def normalize_loudness(wav, rate, target_lufs=-14.0, peak_ceiling_dbfs=-1.0, lens=None, oversample=4):
    """LoudnessMeter.normalize in one call: (wav_out, info)."""
    check_rate(rate)
    _on_gpu(wav)
    return meter(rate, wav.device).normalize(wav, target_lufs, peak_ceiling_dbfs, lens, oversample)
