"""Test helper: a numpy restatement of the clip front end's two rules (csrc/clip_prep.hip), written from their description in
include/aldm_hip.h and csrc/philox.h, not from the kernels.

Segment rule (integers, on top of philox_restatement).  A recording of L samples, a segment of S:
  L <= S      the whole recording from 0 on, zeros behind it
  otherwise   R = L - S.  Candidate c = 0 .. 9 starts at (top 24 bits of word ordinal * 10 + c of the draw) * R // 2^24 -- the integer
              part of R * u for the 24-bit uniform u = (w >> 8) / 2^24, which is what `int(R * torch.rand(1))` computes.  The first
              candidate whose S samples hold one that is louder than fp32(1e-4) wins; when none does, the tenth.

Normalisation (float64).  Over the first m = min(n, target) samples: subtract their mean, divide by (largest magnitude + 1e-8), halve;
zeros from m to target.
"""
import numpy as np

import philox_restatement as PR

CANDIDATES = 10
SILENCE = np.float32(1e-4)


def candidate_starts(seed, draw, ordinal, R):
    """the ten candidate starts of the row with this ordinal, as Python ints"""
    w = PR.u32(seed, draw, (ordinal + 1) * CANDIDATES)[ordinal * CANDIDATES:]
    return [((int(v) >> 8) * int(R)) >> 24 for v in w]


def segment(x, S, seed, draw, ordinal):
    """x fp32 [L] -> (start, seg fp32 [S])"""
    x = np.asarray(x, dtype=np.float32)
    L = x.shape[0]
    seg = np.zeros(S, dtype=np.float32)
    if L <= S:
        seg[:L] = x
        return 0, seg
    start = None
    for start in candidate_starts(seed, draw, ordinal, L - S):
        if (np.abs(x[start:start + S]) > SILENCE).any():
            break
    seg[:] = x[start:start + S]
    return start, seg


def normalize(y, n, target):
    """y [T] (its first n samples count) -> float64 [target]"""
    m = min(int(n), int(target), len(y))
    out = np.zeros(target, dtype=np.float64)
    if m <= 0:
        return out
    v = np.asarray(y[:m], dtype=np.float64)
    d = v - v.mean()
    out[:m] = d / (np.abs(d).max() + 1e-8) * 0.5
    return out


def normalize_bound(x):
    """Per-sample bound of |kernel - normalize(x)| for the counted samples x (fp32 values), float64 [len(x)].

    With u = 2^-24 (fp32's unit roundoff), mean the exact mean, d = x - mean, peak = max |d| and ref = d / (peak + 1e-8) / 2, an fp32
    evaluation commits, to first order:
      the mean rounded to fp32                 |error of the mean| <= u |mean|.  It moves every d by that much, and the peak with it:
                                               sample term  u |mean| / (2 (peak + 1e-8)),
                                               peak term    |ref| u |mean| / (peak + 1e-8) <= u |mean| / (2 (peak + 1e-8))
      the subtraction x - mean rounded         <= u |d|: sample term u |d| / (2 (peak + 1e-8)) = u |ref|, and the same on the sample
                                               that is the peak: u |ref| more
      the division: the denominator's sum and the quotient, each rounded      2 u |ref|      (the halving is exact)
    Sum: u (4 |ref| + |mean| / (peak + 1e-8)).  The stated bound adds max|x| / (peak + 1e-8) >= 1 units of u on top, which covers the
    second-order terms and a mean that is rounded from a float64 sum rather than exactly:

        2^-24 (4 |ref| + (|mean| + max|x|) / (peak + 1e-8))
    """
    v = np.asarray(x, dtype=np.float64)
    mean = v.mean()
    d = v - mean
    peak = np.abs(d).max()
    ref = d / (peak + 1e-8) * 0.5
    return 2.0 ** -24 * (4.0 * np.abs(ref) + (abs(mean) + np.abs(v).max()) / (peak + 1e-8))
