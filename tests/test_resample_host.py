"""Host side of the polyphase resampler (resample.py): the filter and its phase table against scipy, the float64 restatement the GPU
tests compare with against scipy.signal.resample_poly, the ratio rules, and the no-CPU-fallback rule."""
import numpy as np
import pytest
import torch
from scipy import signal

import resample_restatement as RR
from audioldm_with_lora_amd import resample as R

RATIOS = [R.ratio(a, b) for a, b, _ in RR.PAIRS]


@pytest.mark.parametrize("up,down", RATIOS + [(1999, 2000), (2000, 1999), (1, 2048), (2048, 1)])
def test_filter_matches_scipy_firwin(up, down):
    m = max(up, down)
    half = 10 * m
    want = signal.firwin(2 * half + 1, 1.0 / m, window=("kaiser", 5.0)) * up
    h = R.resample_filter(up, down)
    assert h.dtype == np.float64 and h.shape == (2 * half + 1,)
    np.testing.assert_allclose(h, want, rtol=1e-12, atol=1e-18)


def test_filter_3_1_is_the_clap_front_ends():
    from audioldm_with_lora_amd.clap_audio import resample_taps
    assert np.array_equal(R.resample_filter(3, 1), resample_taps(3))


@pytest.mark.parametrize("up,down", RATIOS + [(1999, 2000)])
def test_phase_table_layout(up, down):
    h = R.resample_filter(up, down)
    t = R.phase_table(up, down)
    K = -(-h.size // up)
    assert t.dtype == np.float32 and t.shape == (up, K) and t.flags["C_CONTIGUOUS"]
    for p in range(up):
        for k in range(K):
            i = p + k * up
            assert t[p, k] == (np.float32(h[i]) if i < h.size else np.float32(0.0)), (p, k)
    if up * K > h.size:
        assert not t.reshape(-1, order="F")[h.size:].any()          # zeros behind the end of h


@pytest.mark.parametrize("rate_in,rate_out,T", RR.PAIRS)
def test_restatement_matches_scipy_resample_poly(rate_in, rate_out, T):
    up, down = R.ratio(rate_in, rate_out)
    for t_in in (T, 1, 7):
        x = RR.clip(t_in, 11).astype(np.float64)
        want = signal.resample_poly(x, up, down)
        y, S, Kn = RR.restate(x, up, down)
        assert y.shape == want.shape == (R.output_length(t_in, up, down),)
        assert np.abs(y - want).max() <= 1e-12
        assert (Kn >= 1).all() and Kn.max() <= -(-(20 * max(up, down) + 1) // up)
        assert (S >= np.abs(y) - 1e-15).all()


def test_restatement_ragged_length_and_index_subset():
    x = RR.clip(500, 3).astype(np.float64)
    full, _, _ = RR.restate(x[:123], 160, 441)
    part, _, _ = RR.restate(x, 160, 441, length=123)
    assert np.array_equal(full, part)
    some, _, _ = RR.restate(x, 160, 441, idx=[0, 7, 44], length=123)
    assert np.array_equal(some, full[[0, 7, 44]])


def test_restatement_past_2_pow_31():
    """the overflow case of the GPU suite: 1999 : 2000 on 1.1 M samples, where n down + half passes 2^31"""
    T = 1_100_000
    x = RR.clip(T, 5).astype(np.float64)
    n_out = R.output_length(T, 1999, 2000)
    assert (n_out - 1) * 2000 + 20000 == 2_198_918_000 > 2 ** 31
    want = signal.resample_poly(x, 1999, 2000)
    assert want.shape == (n_out,)
    idx = np.arange(n_out - 512, n_out)
    y, _, _ = RR.restate(x, 1999, 2000, idx=idx)
    assert np.abs(y - want[idx]).max() <= 1e-12


def test_ratio_rules():
    assert R.ratio(44100, 16000) == (160, 441)
    assert R.ratio(16000, 48000) == (3, 1)
    assert R.ratio(16000, 16000) == (1, 1)
    assert R.ratio(22050, 16000) == (320, 441)
    assert R.ratio(np.int64(48000), 16000.0) == (1, 3)
    for bad in ((0, 16000), (16000, -1), (44100.5, 16000), ("44100", 16000), (16000, None), (True, 16000)):
        with pytest.raises(ValueError):
            R.ratio(*bad)
    assert R.ratio(2048, 1) == (1, 2048)
    with pytest.raises(ValueError, match="2049"):
        R.ratio(2049, 1)
    with pytest.raises(ValueError, match="16000 : 16001|16001 : 16000"):
        R.ratio(16001, 16000)
    rates = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000)
    assert max(max(R.ratio(a, b)) for a in rates for b in rates) == 1280          # 11025 <-> 96000: 1280 : 147
    assert max(max(R.ratio(a, 192000)) for a in rates if a != 11025) == 1280      # 22050 -> 192000
    with pytest.raises(ValueError, match="2560 : 147"):                            # the one common pair over the cap
        R.ratio(11025, 192000)
    with pytest.raises(ValueError):
        R.resample_filter(1, 2049)
    with pytest.raises(ValueError):
        R.phase_table(0, 1)


def test_output_length_matches_scipy():
    for up, down in RATIOS:
        for T in (1, 2, 7, 160, 441, 1000):
            assert R.output_length(T, up, down) == signal.resample_poly(np.zeros(T), up, down).shape[0] == -(-T * up // down)


def test_equal_rates_are_the_identity():
    import audioldm_with_lora_amd as pkg
    x = torch.randn(2, 100)
    assert R.resample(x, 16000, 16000) is x
    assert R.resample(x, 48000, 48000) is x
    assert pkg.resample(x, 44100, 44100) is x                       # the package's export is the function
    assert pkg.Resampler is R.Resampler and pkg.resample.Resampler is R.Resampler


def test_no_cpu_fallback():
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd._lib import AldmError
    x = torch.zeros(1, 64)
    with pytest.raises(AldmError):
        ops.resample_poly(x, 3, 1)
    with pytest.raises(AldmError):
        R.resample(x, 44100, 16000)
    with pytest.raises(AldmError):
        R.Resampler(44100, 16000, "cpu")


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    """every ALDM_CHECK_ARG of aldm_resample_poly returns before anything is launched (the pointers are never followed)"""
    import ctypes
    from audioldm_with_lora_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    good = [p, p, 1, 100, p, 3, 1, 21, 30, p, 300, None]
    for pos, bad in ((0, None), (1, None), (4, None), (9, None), (2, 0), (2, 65536), (3, 0), (10, 299), (10, 0), (7, 20), (7, 22), (8, 31),
                     (5, 2049), (5, 0), (6, 0)):
        args = list(good)
        args[pos] = bad
        assert lib.aldm_resample_poly(*args) == -1, (pos, bad)
        assert b"resample_poly" in lib.aldm_last_error()
    assert lib.aldm_resample_poly(p, p, 1, 100, p, 1, 2049, 1, 20490, p, 1, None) == -1 and b"cap" in lib.aldm_last_error()
