"""float64 restatement of the polyphase resampler (audioldm_with_lora_amd/resample.py, csrc/resample.hip), for tests.

    m = n down + half,  p = m mod up,  j1 = m div up
    y[n] = sum_{k = 0 .. K-1} table[p][k] x[j1 - k]          (x[j] = 0 outside [0, len))

evaluated at a given set of output indices with Python-integer (unbounded) index arithmetic and the float64 filter
(table[p][k] = h[p + k up]: the value scipy.signal.resample_poly computes).  Besides y it returns, per output,
S[n] = sum |table[p][k] x[j1 - k]| and Kn, the number of taps that met a sample: the terms of the bound

    |got[n] - y[n]| <= (Kn + 2) 2^-24 S[n] + 1e-30

-- the running-error bound of a length-Kn fp32 sum in any order (Kn roundings of partial sums, each at most 2^-24 of a partial
sum of absolute value <= S, fused or not) plus one rounding of each float64 tap to the fp32 table the kernel reads.
"""
import numpy as np

from audioldm_with_lora_amd.resample import output_length, resample_filter

# the GPU parity list: (rate in, rate out, T_in)
PAIRS = [(16000, 44100, 3001), (44100, 16000, 5003), (48000, 16000, 4001), (16000, 48000, 1001), (22050, 16000, 3000),
         (16000, 22400, 777)]


def clip(T, seed):
    """the tests' input: a seeded 0.3 * randn clipped to [-1, 1], fp32"""
    return np.clip(0.3 * np.random.default_rng(seed).standard_normal(T), -1.0, 1.0).astype(np.float32)


def restate(x, up, down, idx=None, length=None):
    """x: 1-D array (its first `length` samples count, all when None); idx: output indices (all ceil(length up / down) when None).
    -> (y float64, S float64, Kn int64), each [len(idx)]."""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0] if length is None else int(length)
    half = 10 * max(up, down)
    h = resample_filter(up, down)
    K = -(-h.size // up)
    tab = np.zeros(K * up)
    tab[:h.size] = h
    tab = tab.reshape(K, up).T
    n_out = output_length(L, up, down)
    idx = range(n_out) if idx is None else [int(i) for i in idx]
    y, S, Kn = np.zeros(len(idx)), np.zeros(len(idx)), np.zeros(len(idx), dtype=np.int64)
    for i, n in enumerate(idx):
        assert 0 <= n < n_out
        m = n * down + half                                    # Python ints: no overflow
        p, j1 = m % up, m // up
        k0, k1 = max(0, j1 - (L - 1)), min((h.size - 1 - p) // up, j1)         # the taps of phase p that meet a sample
        if k1 < k0:
            continue
        terms = tab[p, k0:k1 + 1] * x[j1 - k1:j1 - k0 + 1][::-1]
        y[i], S[i], Kn[i] = terms.sum(), np.abs(terms).sum(), k1 - k0 + 1
    return y, S, Kn


def bound(S, Kn, factor=1.0):
    return factor * ((Kn + 2) * 2.0 ** -24 * S) + 1e-30
