"""Rational polyphase FIR resampling on the MI355X: audio at any rate in, any rate out.

The arithmetic is scipy.signal.resample_poly(x, up, down) with its defaults -- a Kaiser(5.0)-windowed sinc of 20 max(up, down) + 1
taps, zero padding -- the definition clap_audio.resample_taps already uses for 3 : 1.  The host side (numpy, float64) builds the
filter and cuts it into its `up` phases; the sum runs in csrc/resample.hip (aldm_resample_poly, ops.resample_poly):

    m = n down + half,  p = m mod up,  j1 = m div up
    y[n] = sum_{k = 0 .. K-1} table[p][k] x[j1 - k]          (x[j] = 0 outside [0, len)),  n < ceil(len up / down)

    Resampler(44100, 16000, "cuda")(wav)      the table stays on the device; wav fp32 [T] or [B, T] on the GPU
    resample(wav, 44100, 16000)               the same in one call; equal rates hand the input back untouched
"""
import math
import sys

import numpy as np
import torch

from . import _lib, ops

MAX_RATIO = 2048          # cap of max(up, down): 40 961 taps.  Of the pairs among 8 / 11.025 / 16 / 22.05 / 32 / 44.1 / 48 / 96 / 192 kHz
                          # only 11.025 <-> 192 kHz (2560 : 147) is over it; the next largest is 1280 : 147


def _rate(r):
    ok = isinstance(r, (int, np.integer)) and not isinstance(r, bool)
    if not ok and isinstance(r, (float, np.floating)):
        ok = float(r).is_integer()
    if not ok or r <= 0:
        raise ValueError(f"a sampling rate must be a positive integer, got {r!r}")
    return int(r)


def ratio(rate_in, rate_out):
    """(up, down) of rate_in -> rate_out, reduced by the gcd: 44100 -> 16000 is (160, 441)."""
    rate_in, rate_out = _rate(rate_in), _rate(rate_out)
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    if max(up, down) > MAX_RATIO:
        raise ValueError(f"{rate_in} -> {rate_out} Hz reduces to {up} : {down}, over the cap of {MAX_RATIO} "
                         "(go through an intermediate rate)")
    return up, down


def check_ratio(up, down):
    ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= 1 for v in (up, down))
    if not ok:
        raise ValueError(f"up and down must be positive integers, got {up!r} : {down!r}")
    if max(up, down) > MAX_RATIO:
        raise ValueError(f"ratio {up} : {down} is over the cap of {MAX_RATIO}")
    return int(up), int(down)


def resample_filter(up, down):
    """The FIR of scipy.signal.resample_poly(x, up, down): firwin(2 half + 1, 1 / m, window=("kaiser", 5.0)) * up with
    m = max(up, down), half = 10 m, written out in numpy (float64).  resample_filter(3, 1) is clap_audio.resample_taps(3)."""
    up, down = check_ratio(up, down)
    m = max(up, down)
    half = 10 * m
    n = np.arange(2 * half + 1, dtype=np.float64) - half
    cutoff = 1.0 / m
    h = cutoff * np.sinc(cutoff * n) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def phase_table(up, down):
    """The filter cut into its phases: fp32 [up][K], K = ceil((2 half + 1) / up), table[p][k] = h[p + k up], zero behind the end."""
    h = resample_filter(up, down)
    K = -(-h.size // up)
    t = np.zeros(K * up, dtype=np.float64)
    t[:h.size] = h
    return np.ascontiguousarray(t.reshape(K, up).T).astype(np.float32)


def output_length(n, up, down):
    """ceil(n up / down): the number of samples resample_poly returns for n"""
    return -(-int(n) * int(up) // int(down))


_tables = {}


def device_table(up, down, device):
    """the phase table of up : down on `device`, built once per (ratio, device)"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(up), int(down), device)
    if key not in _tables:
        _tables[key] = torch.from_numpy(phase_table(up, down)).to(device)
    return _tables[key]


class Resampler:
    """rate_in -> rate_out on `device`, the phase table kept there.  `r(wav)`: fp32 [T] or [B, T] on the GPU -> the resampled tensor,
    ceil(T up / down) samples per row.  `r(wav, lens)` -> (tensor, out_lens) for rows that hold lens[b] samples (ops.resample_poly)."""

    def __init__(self, rate_in, rate_out, device="cuda"):
        self.rate_in, self.rate_out = _rate(rate_in), _rate(rate_out)
        self.up, self.down = ratio(rate_in, rate_out)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AldmError("Resampler runs on the MI355X only (got a CPU device); there is no CPU fallback")
        self.table = None if self.up == self.down else device_table(self.up, self.down, self.device)

    def output_length(self, n):
        return output_length(n, self.up, self.down)

    def __call__(self, wav, lens=None):
        if not torch.is_tensor(wav) or wav.dim() not in (1, 2):
            raise ValueError("Resampler: a tensor [T] or [B, T] is expected")
        ops._require_gpu(wav)
        if self.up == self.down:                                      # equal rates: the input itself, no launch
            return wav if lens is None else (wav, torch.as_tensor(lens).to("cpu", torch.int32))
        y, out_lens = ops.resample_poly(wav[None] if wav.dim() == 1 else wav, self.up, self.down, lens,
                                        table=self.table if self.table.device == wav.device else None)
        y = y[0] if wav.dim() == 1 else y
        return y if lens is None else (y, out_lens)


def resample(wav, rate_in, rate_out):
    """wav [T] or [B, T] on the GPU at rate_in -> the same at rate_out (ceil(T up / down) samples).  Equal rates return `wav` itself."""
    up, down = ratio(rate_in, rate_out)
    if up == down:
        return wav
    if not torch.is_tensor(wav):
        raise ValueError("resample: a tensor [T] or [B, T] is expected")
    ops._require_gpu(wav)
    return Resampler(rate_in, rate_out, wav.device)(wav)


class _CallableModule(type(math)):
    """The package exports the function `resample`, and this module has that name: importing it binds the package attribute to the
    module, so the module is made callable -- `from audioldm_with_lora_amd import resample; resample(wav, 44100, 16000)` is the
    function, `resample.Resampler` the class."""

    def __call__(self, wav, rate_in, rate_out):
        return resample(wav, rate_in, rate_out)


sys.modules[__name__].__class__ = _CallableModule
