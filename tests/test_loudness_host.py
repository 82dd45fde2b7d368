"""Host: the BS.1770 loudness arithmetic (audioldm_with_lora_amd/loudness.py's filter design and chunk tables, and the float64
restatement the device tests compare against) -- the recommendation's printed coefficients and its 997 Hz reading, both gates,
the chunked recurrence against the sequential one, and the edge rules of the hop / block grid."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loudness_restatement as LR  # noqa: E402
from audioldm_with_lora_amd import loudness as L  # noqa: E402

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0, b1, b2, a1, a2 of the shelf; a1, a2 of the high-pass (its b is 1, -2, 1)
PRINTED_SHELF = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
PRINTED_HIGHPASS = (-1.99004745483398, 0.99007225036621)


def test_k_weighting_reproduces_the_printed_48k_coefficients():
    (b1, a1), (b2, a2) = L.k_weighting(48000)
    got = np.concatenate([b1, a1[1:], a2[1:]])
    assert all(v.dtype == np.float64 for v in (b1, a1, b2, a2))
    assert a1[0] == 1.0 and a2[0] == 1.0 and b2.tolist() == [1.0, -2.0, 1.0]
    assert np.max(np.abs(got - np.array(PRINTED_SHELF + PRINTED_HIGHPASS))) <= 1e-7
    for fs in (16000, 44100, 48000):                                # the restatement designs its own filter: the two agree
        for (b, a), (rb, ra) in zip(L.k_weighting(fs), LR.design(fs)):
            assert np.array_equal(b, rb) and np.array_equal(a, ra)
        assert np.array_equal(L.state_transition(fs), LR.transition(fs))
        assert L.coef_table(fs).shape == (10,)


@pytest.mark.parametrize("fs,want", [(48000, -3.0103), (16000, -2.9700)])
def test_full_scale_997_hz_sine(fs, want):
    """the recommendation's calibration: a 0 dBFS 997 Hz sine reads -3.01 LKFS (at 16 kHz the bilinear warp moves it to -2.970)"""
    assert abs(LR.integrated(LR.sine(fs, 5.0), fs) - want) <= 1e-3


def test_both_gates():
    """-20 dBFS then -50 dBFS: the relative gate drops the quiet half (2.8 LU); -20 dBFS then zeros: the absolute gate drops the
    silence, the relative gate the blocks that straddle the edge"""
    fs, H = 16000, 1600
    e = LR.hop_energies(LR.two_level(fs, -50.0), fs)
    assert abs(LR.loudness(e, H) - (-23.186)) <= 1e-3
    assert abs(LR.loudness(e, H, relative_gate=False) - (-25.970)) <= 1e-3
    e = LR.hop_energies(LR.two_level(fs, None), fs)
    assert abs(LR.loudness(e, H) - (-23.186)) <= 1e-3
    assert abs(LR.loudness(e, H, relative_gate=False) - (-23.329)) <= 1e-3


def test_chunked_restatement_is_the_sequential_one():
    """Two float64 orderings of the same arithmetic (sequential; chunks from a zero state + state hand-over by the transition power +
    chunks again) on 0.5 DC + a small tone + noise, where the high-pass output is a small difference of large states.  The worst
    relative hop-energy difference is the float64 ordering floor (1.3e-12 at 16 kHz); the device bound of 1e-9 sits 1000 x above."""
    import conftest
    fs, C = 16000, L.CHUNK
    worst = 0.0
    for n in (3 * fs + 37, C - 1, C, C + 1, 2 * C + 1):
        x = LR.dc_case(n, fs)                                        # (the lengths under a hop have no hop energy: checked below)
        worst = max(worst, LR.rel_err(LR.hop_energies(x, fs, chunked=C), LR.hop_energies(x, fs)))
    for n in (C - 1, C, C + 1, 2 * C + 1):                           # the chunk edges themselves: the K-weighted samples
        x = LR.dc_case(n, fs)
        a, b = LR.k_weighted(x, fs), LR.k_weighted(x, fs, chunked=C)
        assert a.shape == b.shape == (n,)
        worst = max(worst, float(np.max(np.abs(a - b)) / np.max(np.abs(a))))
    conftest.record(worst, "float64_ordering_floor")
    assert worst <= 1e-9 / 100.0


def test_chunk_tables():
    """chunk_powers: exact powers of the float64 transition matrix as double-doubles; level k is the square of level k - 1"""
    from fractions import Fraction
    for fs in (16000, 48000):
        p = L.chunk_powers(fs)
        assert p.shape == (L.SCAN_LEVELS, 2, 4, 4) and p.dtype == np.float64
        A = [[Fraction(float(v)) for v in row] for row in LR.transition(fs)]
        P = A
        for _ in range(10):                                          # A^1024 by ten exact squarings (L.CHUNK = 2^10)
            P = [[sum(P[i][k] * P[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
        assert L.CHUNK == 1024
        for i in range(4):
            for j in range(4):
                hi, lo = float(p[0, 0, i, j]), float(p[0, 1, i, j])
                assert hi == float(P[i][j])                           # the leading double is the exact entry rounded once
                assert abs(Fraction(hi) + Fraction(lo) - P[i][j]) <= abs(P[i][j]) * Fraction(1, 2 ** 100)
        sq = (p[0, 0] + p[0, 1]) @ (p[0, 0] + p[0, 1])
        assert np.max(np.abs(sq - p[1, 0])) <= 1e-12 * np.max(np.abs(p[1, 0]))


def test_edge_rules():
    fs, H = 16000, 1600
    x = LR.white(4 * H + 700, seed=3)
    assert LR.integrated(x[:4 * H - 1], fs) == -np.inf                # three complete hops: no block
    assert LR.gain(-np.inf, 0.9, -14.0, -1.0) == 1.0
    e = LR.hop_energies(x[:4 * H], fs)
    assert e.shape == (4,) and LR.block_powers(e, H).shape == (1,)    # exactly one block
    assert LR.integrated(x[:4 * H], fs) == pytest.approx(-0.691 + 10.0 * np.log10(e.sum() / (4 * H)), abs=1e-12)
    assert np.array_equal(LR.hop_energies(x, fs), e)                   # the trailing partial hop is ignored
    assert LR.integrated(x, fs) == LR.integrated(x[:4 * H], fs)
    assert LR.integrated(np.zeros(8 * H), fs) == -np.inf              # silence
    for bad in (11025, 4000):
        with pytest.raises(ValueError):
            L.k_weighting(bad)
        with pytest.raises(ValueError):
            LR.hop(bad)
    # the gain: the target, capped by the ceiling over the peak
    assert LR.gain(-20.0, 0.1, -14.0, -1.0) == pytest.approx(10.0 ** (6.0 / 20.0))
    assert LR.gain(-20.0, 0.8, -14.0, -1.0) == pytest.approx(10.0 ** (-1.0 / 20.0) / 0.8)


def test_cpu_tensors_are_refused():
    import torch
    from audioldm_with_lora_amd._lib import AldmError
    with pytest.raises(AldmError, match="no CPU fallback"):
        L.integrated_loudness(torch.zeros(16000), 16000)
    with pytest.raises(AldmError, match="no CPU fallback"):
        L.normalize_loudness(torch.zeros(2, 16000), 16000)
    with pytest.raises(ValueError):
        L.integrated_loudness(torch.zeros(16000), 11025)
