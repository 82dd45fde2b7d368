"""Host side of the on-device training noise (no GPU): the restatement of the stream contract (tests/train_noise_restatement.py)
on its own, the trainer's argument validation and the per-rank ordinal base."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_restatement as P  # noqa: E402
import train_noise_restatement as N  # noqa: E402


def test_timesteps_lie_in_range_and_hit_every_decile():
    T = 1000
    w = P.u32(1234, 5, 2 ** 16)
    t = N.timesteps_of(w, T)
    assert t.dtype == np.int64 and t.min() >= 0 and t.max() < T
    hist = np.bincount(t // (T // 10), minlength=10)
    assert hist.shape == (10,) and (hist > 0).all(), hist
    # the extremes of the word map to the extremes of the range, and never to T
    assert N.timesteps_of(np.array([0, 2 ** 32 - 1], dtype=np.uint32), T).tolist() == [0, T - 1]


def test_the_four_draws_are_the_documented_ordinals():
    seed, d, shape, T = 77, 40, (3, 8, 5, 3), 1000
    B, C, H, W = shape
    n_el = B * C * H * W
    abar = np.linspace(0.999, 0.005, T)
    lat = P.randn(1, 0, n_el).reshape(shape)
    mom = P.randn(2, 0, 2 * n_el).reshape(B, H, W, 2 * C)
    assert N.draw_ordinals(d) == dict(t=d, e=d + 1, n=d + 2, o=d + 3, next=d + 4)
    outs = [N.step(seed, d, shape, abar, latents=lat), N.step(seed, d, shape, abar, noise_offset=0.1, latents=lat),
            N.step(seed, d, shape, abar, moments=mom, scaling_factor=0.9), N.step(seed, d, shape, abar, noise_offset=0.1, moments=mom)]
    for r in outs:                                            # the same four draws whatever the options: streams stay aligned
        assert np.array_equal(r["timesteps"], N.timesteps_of(P.u32(seed, d, B), T))
        assert np.array_equal(r["e"].reshape(-1), P.randn(seed, d + 1, n_el))
        assert np.array_equal(r["n"].reshape(-1), P.randn(seed, d + 2, n_el))
        assert np.array_equal(r["o"].reshape(-1), P.randn(seed, d + 3, B * C))
        assert r["next"] == d + 4
    # the target is the noise, channels-last, with the offset broadcast over H x W
    n, o = outs[0]["n"], outs[0]["o"]
    assert np.array_equal(outs[0]["target"], n.transpose(0, 2, 3, 1))
    assert np.array_equal(outs[1]["target"], (n + 0.1 * o[:, :, None, None]).transpose(0, 2, 3, 1))
    # the noisy latents, spelled out for one element of each source
    b, c, h, w = 2, 5, 4, 1
    t = outs[0]["timesteps"][b]
    want = np.sqrt(abar[t]) * lat[b, c, h, w] + np.sqrt(1 - abar[t]) * n[b, c, h, w]
    assert abs(outs[0]["noisy"][b, h, w, c] - want) < 1e-15
    z = (mom[b, h, w, c] + np.exp(0.5 * np.clip(mom[b, h, w, C + c], -30, 20)) * outs[2]["e"][b, c, h, w]) * 0.9
    want = np.sqrt(abar[t]) * z + np.sqrt(1 - abar[t]) * n[b, c, h, w]
    assert abs(outs[2]["noisy"][b, h, w, c] - want) < 1e-15
    # passing the normals in replaces the restated ones
    r = N.step(seed, d, shape, abar, latents=lat, n=np.zeros(shape), o=np.zeros((B, C)))
    assert np.array_equal(r["target"], np.zeros((B, H, W, C)))


def test_rank_ordinal_base_is_rank_times_2_to_the_48():
    from audioldm_with_lora_amd import training
    assert training.RANK_ORDINAL_STRIDE == 2 ** 48 == N.RANK_STRIDE
    for rank in (0, 1, 7, 255):
        assert training.noise_ordinal_base(rank) == rank * 2 ** 48 == N.rank_base(rank)
    # 2^46 steps of four draws fit under a rank's base before it reaches the next rank's
    assert training.noise_ordinal_base(1) - training.noise_ordinal_base(0) == 4 * 2 ** 46


def test_noise_argument_validation():
    import torch
    from audioldm_with_lora_amd import training
    from audioldm_with_lora_amd._lib import AldmError
    x = torch.zeros(1)
    chk = training.check_noise_args
    assert chk(None, 0.0, (x, x)) is False                       # today's call: tensors, no seed
    assert chk(3, 0.0, (x, x, x)) is False                       # a seeded trainer still takes host noise
    assert chk(3, 0.0, (None, None)) is True
    assert chk(3, 0.1, (None, None, None)) is True
    with pytest.raises(AldmError, match="noise_seed"):
        chk(None, 0.0, (None, None))                             # None without a seed
    with pytest.raises(AldmError, match="noise_offset"):
        chk(3, 0.1, (x, x))                                      # the offset with host noise
    with pytest.raises(AldmError, match="all together"):
        chk(3, 0.0, (x, None))


def test_cpu_tensors_are_refused():
    import torch
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd._lib import AldmError
    state = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(AldmError, match="CPU"):
        ops.train_noise_fused(state, torch.ones(10), latents=torch.zeros(1, 1, 2, 2))
    with pytest.raises(AldmError, match="CPU"):
        ops.philox_set(state, draw=4)


def test_train_driver_parses_the_device_noise_options():
    from audioldm_with_lora_amd.script import train
    a = train.build_parser().parse_args([])
    assert a.device_noise is False and a.noise_offset == 0.0
    a = train.build_parser().parse_args(["--device-noise", "--noise-offset", "0.1"])
    assert a.device_noise is True and a.noise_offset == 0.1
