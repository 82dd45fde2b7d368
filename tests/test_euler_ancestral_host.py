"""CPU: the Philox restatement against the published Random123 known answers and the statistical asserts of the GPU test, and
EulerAncestralDiscreteScheduler's host side -- timesteps, sigmas, init_noise_sigma and the coefficient / blend tables in closed form
and against tests/euler_a_restatement.py, the configuration round trip, the refused options, and no CPU fallback."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_restatement as P  # noqa: E402
from euler_a_restatement import EulerAncestralRestatement  # noqa: E402

from audioldm_with_lora_amd.scheduler import (DDIMScheduler, DPMSolverMultistepScheduler,  # noqa: E402
                                              EulerAncestralDiscreteScheduler)

SEED = 2025           # the seed of the GPU moment test; it and two others pass the same asserts on the restatement below

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_restatement_known_answers(counter, key, want):
    got = P.philox4x32_10(counter, key)
    assert " ".join(f"{int(w):08x}" for w in got) == want
    # the same vector through the stream addressing: seed = key, draw = counter words 2..3, block = counter words 0..1
    seed, draw, block = key[0] | key[1] << 32, counter[2] | counter[3] << 32, counter[0] | counter[1] << 32
    assert " ".join(f"{int(w):08x}" for w in P.blocks(seed, draw, 1, first_block=block)[0]) == want


def test_box_muller_inputs_are_fp32_and_in_range():
    w = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32)
    u, v = P.box_muller_inputs(w, w)
    assert u[0] == np.float32(2.0 ** -33) and u[-1] == np.float32(1.0) and (u > 0).all() and (u <= 1).all()
    assert v[0] == 0 and v[-1] <= np.float32(2 * math.pi) * np.float32(1.0000002)
    z = P.randn(3, 0, 4096)
    assert np.isfinite(z).all() and np.abs(z).max() <= math.sqrt(-2 * math.log(2.0 ** -33))


@pytest.mark.parametrize("seed", [SEED, 1, 987654321])
def test_restatement_passes_the_moment_asserts(seed):
    N = 1 << 22
    P.moment_checks(P.randn(seed, 0, N), P.randn(seed, 1, N))


def _euler(**kw):
    return EulerAncestralDiscreteScheduler.from_config(DDIMScheduler().config, **kw)


def _sigma_all():
    betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, dim=0)
    return (((1 - ac) / ac) ** 0.5).numpy()


@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
@pytest.mark.parametrize("N", [10, 20, 37])
def test_schedule_closed_form(spacing, N):
    s = _euler(timestep_spacing=spacing)
    s.set_timesteps(N)
    if spacing == "leading":
        want = np.array([(N - 1 - k) * (1000 // N) + 1 for k in range(N)], dtype=np.float32)
    elif spacing == "linspace":
        want = np.linspace(0, 999, N, dtype=np.float32)[::-1]
    else:
        want = np.array([round(1000 - k * 1000 / N) - 1 for k in range(N)], dtype=np.float32)
    assert s.timesteps.dtype == torch.float32 and np.array_equal(s.timesteps.numpy(), want)
    sa = _sigma_all()
    lo = np.floor(want).astype(np.int64)
    hi = np.minimum(lo + 1, 999)
    f = want.astype(np.float64) - lo
    sig = (sa[lo] * (1 - f) + sa[hi] * f).astype(np.float32)
    assert s.sigmas.dtype == torch.float32 and s.sigmas.shape == (N + 1,) and float(s.sigmas[-1]) == 0.0
    np.testing.assert_allclose(s.sigmas[:-1].numpy(), sig, rtol=2e-7, atol=0)
    m = float(s.sigmas.max())
    want_init = m if spacing != "leading" else math.sqrt(m * m + 1)
    assert abs(s.init_noise_sigma - want_init) <= 1e-6 * want_init
    # the restatement builds the same schedule
    r = EulerAncestralRestatement(timestep_spacing=spacing)
    r.set_timesteps(N)
    assert torch.equal(r.timesteps, s.timesteps) and torch.equal(r.sigmas, s.sigmas) and r.init_noise_sigma == s.init_noise_sigma


@pytest.mark.parametrize("spacing", ["leading", "linspace", "trailing"])
def test_tables_against_restatement(spacing):
    N = 20
    s, r = _euler(timestep_spacing=spacing), EulerAncestralRestatement(timestep_spacing=spacing)
    s.set_timesteps(N)
    r.set_timesteps(N)
    tab = s.coefficient_table()
    assert tab.dtype == torch.float32 and tab.shape == (N, 4)
    assert torch.equal(tab, torch.stack([r.row(i) for i in range(N)]))
    assert torch.equal(s.coefficient_table(begin_index=7), tab[7:])
    sig = s.sigmas.double()
    dt, up, scale, down = (tab[:, k].double() for k in range(4))
    # sigma_up^2 + sigma_down^2 == s_to^2 and dt == sigma_down - s_from, to fp32 rounding of quantities of size s_to^2 / s_from
    assert torch.all((up ** 2 + down ** 2 - sig[1:] ** 2).abs() <= 8 * 2.0 ** -24 * sig[1:] ** 2)
    assert torch.all((dt - (down - sig[:-1])).abs() <= 2.0 ** -23 * sig[:-1])
    assert torch.all((scale - 1 / (sig[1:] ** 2 + 1).sqrt()).abs() <= 4 * 2.0 ** -24)
    assert torch.all(up[:-1] > 0) and torch.all(down[:-1] > 0) and torch.all(dt < 0)
    # the last row: no noise, no scaling, x' = x - s_from e
    assert float(tab[-1, 1]) == 0.0 and float(tab[-1, 2]) == 1.0 and float(tab[-1, 3]) == 0.0 and float(tab[-1, 0]) == -float(s.sigmas[N - 1])
    # audio-to-audio pieces: (1, sigma_i), blend rows (1, sigma_{i + 1}) with the last exactly (1, 0)
    a, sg = s.add_noise_coefficients(5)
    assert float(a) == 1.0 and float(sg) == float(s.sigmas[5])
    bl = s.blend_table(7)
    assert bl.shape == (N - 7, 2) and torch.equal(bl[:, 0], torch.ones(N - 7)) and torch.equal(bl[:, 1], s.sigmas[8:])
    ts, begin = s.get_timesteps(N, 0.5)
    assert begin == 10 and torch.equal(ts, s.timesteps[10:])
    with pytest.raises(ValueError):
        s.coefficient_table(begin_index=N)


def test_restatement_step_is_the_documented_update():
    r = EulerAncestralRestatement()
    r.set_timesteps(10)
    g = torch.Generator().manual_seed(0)
    x, e, z = (torch.randn(2, 3, generator=g) for _ in range(3))
    up, down = r.sigma_up_down(0)
    got = r.step(e, r.timesteps[0], x, noise=z).prev_sample
    assert torch.equal(got, x + e * (down - r.sigmas[0]) + up * z) and r.step_index == 1
    r.step_index = 9
    assert torch.equal(r.step(e, r.timesteps[9], x, noise=z).prev_sample, x + e * (0 - r.sigmas[9]) + 0 * z)


def test_from_config_round_trip_and_surface():
    ddim = DDIMScheduler()
    s = EulerAncestralDiscreteScheduler.from_config(ddim.config)
    for k in ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "steps_offset", "timestep_spacing", "prediction_type"):
        assert getattr(s.config, k) == getattr(ddim.config, k)
    assert not hasattr(s.config, "clip_sample")                         # unknown keys are ignored
    back = DDIMScheduler.from_config(s.config)
    assert vars(back.config) == vars(ddim.config)
    dpm = DPMSolverMultistepScheduler.from_config(s.config)
    s2 = EulerAncestralDiscreteScheduler.from_config(dpm.config, timestep_spacing="trailing")
    assert s2.config.timestep_spacing == "trailing" and not hasattr(s2.config, "solver_order")
    assert vars(EulerAncestralDiscreteScheduler.from_config(vars(s.config)).config) == vars(s.config)
    assert s.config.num_train_timesteps == 1000 and s.step_index is None and len(s.timesteps) == 1000
    s.set_timesteps(10)
    s.set_begin_index(3)
    assert s.begin_index == 3 and s.num_inference_steps == 10
    import audioldm_with_lora_amd
    assert audioldm_with_lora_amd.EulerAncestralDiscreteScheduler is EulerAncestralDiscreteScheduler


def test_from_pretrained_reads_scheduler_config(tmp_path):
    import json
    d = tmp_path / "scheduler"
    d.mkdir()
    (d / "scheduler_config.json").write_text(json.dumps(dict(vars(DDIMScheduler().config), _class_name="DDIMScheduler")))
    s = EulerAncestralDiscreteScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    assert s.config.beta_end == 0.0195 and s.config.steps_offset == 1


@pytest.mark.parametrize("kw,name", [(dict(prediction_type="v_prediction"), "prediction_type"),
                                     (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"),
                                     (dict(beta_schedule="linear"), "beta_schedule"),
                                     (dict(use_karras_sigmas=True), "use_karras_sigmas"),
                                     (dict(timestep_spacing="quadratic"), "timestep_spacing")])
def test_unsupported_options_raise_and_name_the_option(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        EulerAncestralDiscreteScheduler(**kw)


def test_existing_refusals_are_untouched():
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    with pytest.raises(NotImplementedError):
        DDIMScheduler().step(torch.zeros(1), 1, torch.zeros(1), eta=0.5)


def test_no_cpu_fallback():
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd._lib import AldmError
    s = _euler()
    s.set_timesteps(5)
    with pytest.raises(ValueError):
        _euler().step(torch.zeros(1, 4), 801, torch.zeros(1, 4))          # no schedule yet
    with pytest.raises(AldmError):
        s.step(torch.zeros(1, 4), s.timesteps[0], torch.zeros(1, 4), generator=3)
    with pytest.raises(AldmError):
        s.add_noise(torch.zeros(1, 4), torch.zeros(1, 4), s.timesteps[:1])
    cpu_state = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(AldmError):
        ops.randn((8,), cpu_state)
    with pytest.raises(AldmError):
        ops.philox_u32(8, cpu_state)
    with pytest.raises(AldmError):
        ops.philox_state(1, device="cpu")
