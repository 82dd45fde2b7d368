"""Host: the window plan of long-form generation (audioldm_with_lora_amd/longform.py) against its rule and against the independent
restatement (tests/longform_restatement.py) -- offsets, coverage, weights, the cover count, rotation invariance of a looped plan,
smoothness along time, the scaled plan, the rejections and the pipeline's seconds-to-rows rounding."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_restatement as R  # noqa: E402

OPEN = [(20, 8, 2), (11, 5, 2), (21, 8, 2), (44, 16, 4), (72, 32, 8), (41, 16, 8), (1536, 256, 64), (8, 8, 0)]
LOOPED = [(18, 8, 2), (72, 32, 8), (1536, 256, 64)]
CASES = [(s, False) for s in OPEN] + [(s, True) for s in LOOPED]
IDS = ["x".join(map(str, s)) + ("-loop" if lp else "") for s, lp in CASES]
KC_THREE = {(21, 8, 2), (41, 16, 8)}


def _plan(shape, loop, f=1):
    from audioldm_with_lora_amd.longform import WindowPlan
    p = WindowPlan(*shape, loop=loop)
    return p.scaled(f) if f > 1 else p


def _dense(p):
    """[rows, K] float64: window k's weight at long row r (0 where it does not cover r)"""
    d = np.zeros((p.rows, p.K))
    for r in range(p.rows):
        for j in range(p.KC):
            if p.cover[r, j] >= 0:
                d[r, p.cover[r, j]] = p.weight64[r, j]
    return d


@pytest.mark.parametrize("f", [1, 4])
@pytest.mark.parametrize("shape,loop", CASES, ids=IDS)
def test_plan_follows_the_rule(shape, loop, f):
    p = _plan(shape, loop, f)
    rows, hw, ov = (v * f for v in shape)
    S = hw - ov
    # offsets
    if loop:
        want = list(range(0, rows, S))
    elif rows <= hw:
        want = [0]
    else:
        want = [o for o in range(0, rows, S) if o + hw < rows] + [rows - hw]
    assert p.offsets == want and p.offset.dtype == np.int32 and list(p.offset) == want and p.K == len(want)
    assert p.offsets == R.offsets_of(rows, hw, ov, loop)
    # coverage, order, weights
    assert p.cover.shape == p.weight.shape == p.weight64.shape == (rows, p.KC) and p.cover.dtype == np.int32 and p.weight.dtype == np.float32
    for r in range(rows):
        ks = [int(k) for k in p.cover[r] if k >= 0]
        assert len(ks) >= 1 and ks == sorted(set(ks)) and list(p.cover[r, :len(ks)]) == ks           # covered; ascending; -1 only behind
        assert ks == [k for k in range(p.K) if (r - p.offsets[k]) % rows < hw and (loop or r >= p.offsets[k])]
        w = p.weight64[r, :len(ks)]
        assert (w > 0).all() and abs(w.sum() - 1.0) <= 1e-12 and (p.weight64[r, len(ks):] == 0).all()
        assert (p.weight[r, :len(ks)] > 0).all()
    assert np.array_equal(p.weight, p.weight64.astype(np.float32))
    assert p.KC == (3 if shape in KC_THREE and not loop else 1 if p.K == 1 else 2) and p.KC <= 4
    # the restatement's tables, built row by row as differences of crossfades -- and, where at most two windows lie over a row, also
    # from min(1, (i + 1) / (L + 1), (hw - i) / (R + 1))
    forms = [False] + ([True] if p.KC <= 2 else [])
    for min_form in forms:
        _, rhw, rcover, rweight = R.tables_of(rows, hw, ov, loop, min_form=min_form)
        assert rhw == p.window_rows
        for r in range(rows):
            n = len(rcover[r])
            assert list(p.cover[r, :n]) == rcover[r] and np.allclose(p.weight64[r, :n], rweight[r], rtol=0, atol=1e-15), (min_form, r)


@pytest.mark.parametrize("f", [1, 4])
@pytest.mark.parametrize("shape,loop", CASES, ids=IDS)
def test_weights_have_no_jumps_along_time(shape, loop, f):
    """a window's weight moves by at most 1 / (overlap + 1) from one long row to the next (entering and leaving included).  The
    plans with three windows over a row are what this is about: with the profile taken as a plain min() of the two ramps they miss it
    ((21, 8, 2): 0.370 against 0.333), which is why the profile is the difference of the neighbouring crossfades (longform.py)."""
    p = _plan(shape, loop, f)
    d = _dense(p)
    step = np.abs(np.diff(np.concatenate([d, d[:1]]) if loop else d, axis=0))
    # (open plans: the clip's first and last row are ends, not jumps)
    print(f"{shape} x{f} loop={loop}: largest move {step.max(initial=0.0):.4f}, bound {1.0 / (p.overlap_rows + 1):.4f}")
    assert step.max(initial=0.0) <= 1.0 / (p.overlap_rows + 1) + 1e-12, (step.max(), 1.0 / (p.overlap_rows + 1))


@pytest.mark.parametrize("shape", LOOPED, ids=["x".join(map(str, s)) for s in LOOPED])
def test_looped_plan_is_invariant_under_a_rotation_by_the_stride(shape):
    p = _plan(shape, True)
    d = _dense(p)
    assert np.array_equal(np.roll(np.roll(d, p.stride, axis=0), 1, axis=1), d)
    assert (p.cover >= 0).sum(axis=1).min() >= 1


def test_rejections():
    from audioldm_with_lora_amd.longform import WindowPlan
    with pytest.raises(ValueError):
        WindowPlan(20, 8, 5)                      # overlap > hw // 2
    with pytest.raises(ValueError):
        WindowPlan(20, 8, -1)
    with pytest.raises(ValueError):
        WindowPlan(20, 8, 2, loop=True)           # 20 % 6 != 0
    with pytest.raises(ValueError):
        WindowPlan(0, 8, 2)
    assert WindowPlan(18, 8, 2, loop=True).K == 3 and WindowPlan(20, 8, 4).K == 4
    one = WindowPlan(5, 8, 2)                     # shorter than a window: one window of the clip's own length
    assert one.K == one.KC == 1 and one.window_rows == 5 and (one.weight == 1.0).all()
    assert WindowPlan(20, 8, 2).key != WindowPlan(20, 8, 2, loop=False).scaled(4).key and WindowPlan(18, 8, 2).key != WindowPlan(18, 8, 2, loop=True).key


def test_seconds_to_rows_at_25_rows_per_second():
    """the pipeline's rounding: 16 kHz, hop 160 (0.01 s per mel frame), VAE scale 4 -- 25 latent rows per second"""
    from audioldm_with_lora_amd.longform import plan_for_seconds, seconds_to_rows
    up = 160 / 16000
    assert [seconds_to_rows(s, up, 4) for s in (10.24, 2.56, 60.0, 2.88, 1.28, 1.3, 0.64, 0.01)] == [256, 64, 1500, 72, 32, 33, 16, 1]
    p = plan_for_seconds(60.0, 10.24, 2.56, up, 4)
    assert p.key == (1500, 256, 64, False) and p.offsets == [0, 192, 384, 576, 768, 960, 1152, 1244] and p.KC == 2
    p = plan_for_seconds(60.0, 10.24, 2.56, up, 4, loop=True)                  # rounded UP to 8 strides of 192 rows: 61.44 s
    assert p.key == (1536, 256, 64, True) and p.K == 8 and p.KC == 2
    p = plan_for_seconds(2.88, 1.28, 0.32, up, 4, loop=True)
    assert p.key == (72, 32, 8, True) and p.K == 3
    p = plan_for_seconds(2.0, 1.28, 0.32, up, 4, loop=True)                    # 50 rows -> 72
    assert p.key == (72, 32, 8, True)
    p = plan_for_seconds(0.64, 1.28, 0.32, up, 4)                              # shorter than a window
    assert p.key == (16, 16, 0, False) and p.K == 1
