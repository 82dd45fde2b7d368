"""Float64 CPU restatement of the BS.1770-4 loudness measurement and normalisation (mono, channel weight 1), written from the
definition and independent of audioldm_with_lora_amd/loudness.py: its own filter design, scipy.signal.lfilter for the recurrence.

    design(fs)                        the two biquads (libebur128's design: De Man's derivation of the 48 kHz tables)
    hop_energies(x, fs)               sum of y^2 per complete 100 ms hop, y = the K-weighted signal from a zero state
    hop_energies(x, fs, chunked=C)    the same arithmetic in the kernel's order: every chunk of C samples from a zero state, the
                                      states handed along the chunks with the 4x4 state-transition power, every chunk again from its
                                      true state
    loudness(e, H)                    both gates; loudness(e, H, relative_gate=False) the absolute gate alone
    gain(L, peak, target, ceiling)    the normalisation gain (linear)
"""
import math

import numpy as np
from scipy.signal import lfilter

ENERGY_FLOOR = 1e-290     # below this a float64 sum of squares no longer carries 53 bits (squares of y under 1e-154 are subnormal or
                          # zero): relative errors are taken against max(reference, ENERGY_FLOOR)


def design(fs):
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K]) / a0
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return (b1, a1), (b2, a2)


def hop(fs):
    if fs % 10 or fs < 8000:
        raise ValueError(f"rate {fs}")
    return fs // 10


def transition(fs):
    """state' = A state for input 0; state = lfilter's (transposed direct form II) delays of the shelf, then of the high-pass"""
    (b, a), (c, d) = design(fs)
    return np.array([[-a[1], 1.0, 0.0, 0.0], [-a[2], 0.0, 0.0, 0.0],
                     [c[1] - d[1] * c[0], 0.0, -d[1], 1.0], [c[2] - d[2] * c[0], 0.0, -d[2], 0.0]])


def k_weighted(x, fs, chunked=None):
    """the K-weighted signal of the float64 samples x from a zero state; chunked=C: in the kernel's order"""
    (b1, a1), (b2, a2) = design(fs)
    x = np.asarray(x, dtype=np.float64)
    if not chunked:
        return lfilter(b2, a2, lfilter(b1, a1, x))
    C = int(chunked)
    n_chunks = -(-x.size // C)
    M = np.linalg.matrix_power(transition(fs), C)
    ends = []
    for c in range(n_chunks - 1):                                    # 1. every chunk that has a successor, from a zero state
        seg = x[c * C:(c + 1) * C]
        y1, z1 = lfilter(b1, a1, seg, zi=np.zeros(2))
        _, z2 = lfilter(b2, a2, y1, zi=np.zeros(2))
        ends.append(np.concatenate([z1, z2]))
    starts = [np.zeros(4)]
    for z in ends:                                                   # 2. S_{c+1} = M S_c + z_c
        starts.append(M @ starts[-1] + z)
    out = np.empty_like(x)
    for c in range(n_chunks):                                        # 3. every chunk again, from its true state
        seg = x[c * C:(c + 1) * C]
        y1, _ = lfilter(b1, a1, seg, zi=starts[c][:2].copy())
        out[c * C:c * C + seg.size], _ = lfilter(b2, a2, y1, zi=starts[c][2:].copy())
    return out


def hop_energies(x, fs, chunked=None):
    """float64 [len(x) // H]: the complete hops; a trailing partial hop is dropped (and never filtered: it cannot reach a hop before it)"""
    H = hop(fs)
    n = len(x) // H
    y = k_weighted(np.asarray(x, dtype=np.float64)[:n * H], fs, chunked)
    return (y * y).reshape(n, H).sum(axis=1)


def block_powers(e, H):
    e = np.asarray(e, dtype=np.float64)
    if e.size < 4:
        return np.zeros(0)
    return (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * H)


def _lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def loudness(e, H, relative_gate=True):
    z = block_powers(e, H)
    l = _lufs(z) if z.size else z
    keep = l > -70.0
    if not keep.any():
        return -np.inf
    if relative_gate:
        gr = _lufs(z[keep].mean()) - 10.0
        keep = keep & (l > gr)
    return float(_lufs(z[keep].mean()))


def ungated(e, H):
    """the loudness of all blocks, no gate at all"""
    z = block_powers(e, H)
    return float(_lufs(z.mean())) if z.size else -np.inf


def integrated(x, fs, chunked=None, relative_gate=True):
    return loudness(hop_energies(x, fs, chunked), hop(fs), relative_gate)


def gain(L, peak, target, ceiling=None):
    """the linear gain: 10^((target - L) / 20), capped at 10^(ceiling / 20) / peak; 1 for a clip of loudness -inf"""
    if not np.isfinite(L):
        return 1.0
    g = 10.0 ** ((target - L) / 20.0)
    if ceiling is not None and peak > 0:
        g = min(g, 10.0 ** (ceiling / 20.0) / peak)
    return g


def rel_err(got, want):
    """worst relative hop-energy error against max(reference, ENERGY_FLOOR)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want) / np.maximum(want, ENERGY_FLOOR)))


# ---- the inputs the host and the device tests share -----------------------------------------------------------------------------
def sine(fs, seconds, freq=997.0, amp=1.0):
    return amp * np.sin(2.0 * np.pi * freq * np.arange(int(round(seconds * fs))) / fs)


def dc_case(n, fs, seed=0):
    """0.5 DC + 1e-3 of a 440 Hz tone + 1e-4 noise: the high-pass output is a small difference of large states"""
    r = np.random.RandomState(seed)
    t = np.arange(n)
    return 0.5 + 1e-3 * np.sin(2.0 * np.pi * 440.0 * t / fs) + 1e-4 * r.standard_normal(n)


def white(n, seed=1):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, n)


def impulse_at(n, pos):
    x = np.zeros(n)
    if 0 <= pos < n:
        x[pos] = 1.0
    return x


def two_level(fs, second_amp_db):
    """a 1 kHz sine at -20 dBFS for 3 s, then at second_amp_db dBFS (None: zeros) for 3 s"""
    a = sine(fs, 3.0, 1000.0, 10.0 ** (-20.0 / 20.0))
    if second_amp_db is None:
        return np.concatenate([a, np.zeros_like(a)])
    t = np.arange(a.size, 2 * a.size)
    return np.concatenate([a, 10.0 ** (second_amp_db / 20.0) * np.sin(2.0 * np.pi * 1000.0 * t / fs)])
