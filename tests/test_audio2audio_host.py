"""Host-only pieces of audio-to-audio / inpainting (no GPU, no shared library): the strength -> suffix rule, the add_noise coefficients
and blend rows of both schedulers, the begun DPM-Solver table against tests/dpm_restatement.py, the mask reduction and
regeneration_mask, and the argument errors."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dpm_restatement import DPMSolverRestatement  # noqa: E402

from audioldm_with_lora_amd.audio2audio import regeneration_mask, reduce_mask  # noqa: E402
from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, strength_begin_index  # noqa: E402


def _diffusers_get_timesteps(N, strength):
    """diffusers' img2img / inpaint pipelines: get_timesteps(num_inference_steps, strength)"""
    init_timestep = min(int(N * strength), N)
    t_start = max(N - init_timestep, 0)
    return t_start, N - t_start


STRENGTHS = [0.01, 0.1, 0.25, 0.3, 0.5, 0.75, 0.9, 0.999, 1.0]


@pytest.mark.parametrize("N", [1, 10, 25, 50, 200])
@pytest.mark.parametrize("sched", [DDIMScheduler, DPMSolverMultistepScheduler])
def test_strength_to_suffix_matches_diffusers(N, sched):
    s = sched()
    for strength in STRENGTHS:
        t_start, n = _diffusers_get_timesteps(N, strength)
        if n == 0:
            with pytest.raises(ValueError):
                strength_begin_index(N, strength)
            with pytest.raises(ValueError):
                s.get_timesteps(N, strength)
            continue
        assert strength_begin_index(N, strength) == t_start
        ts, begin = s.get_timesteps(N, strength)
        s.set_timesteps(N)
        assert begin == t_start and len(ts) == n and torch.equal(ts, s.timesteps[t_start:])


def test_strength_errors():
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            strength_begin_index(10, bad)
    with pytest.raises(ValueError):
        strength_begin_index(0, 0.5)
    with pytest.raises(ValueError):
        strength_begin_index(10, 0.0)
    with pytest.raises(ValueError):
        strength_begin_index(10, 0.05)           # int(0.5) == 0: no step left
    assert strength_begin_index(10, 1.0) == 0


def test_ddim_add_noise_coefficients_are_add_noise():
    s = DDIMScheduler()
    s.set_timesteps(25)
    for i in (0, 7, 24):
        t = int(s.timesteps[i])
        a, sg = s.add_noise_coefficients(i)
        ac = s.alphas_cumprod[t]
        assert float(a) == float(ac ** 0.5) and float(sg) == float((1 - ac) ** 0.5)
        assert a.dtype == torch.float32 and sg.dtype == torch.float32


def test_dpm_add_noise_coefficients_are_alpha_sigma_of_sigma():
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(20)
    for i in (0, 5, 19):
        a, sg = s.add_noise_coefficients(i)
        sig = s.sigmas[i]
        alpha = 1 / ((sig ** 2 + 1) ** 0.5)
        assert float(a) == float(alpha) and float(sg) == float(sig * alpha)
        # the same (alpha, sigma) the restatement's step uses at that index
        r = DPMSolverRestatement()
        r.set_timesteps(20)
        ra, rs = r._alpha_sigma(r.sigmas[i])
        assert float(a) == float(ra) and float(sg) == float(rs)


@pytest.mark.parametrize("sched", [DDIMScheduler, DPMSolverMultistepScheduler])
@pytest.mark.parametrize("N,strength", [(10, 0.5), (25, 0.3), (50, 1.0), (1, 1.0), (200, 0.75)])
def test_blend_rows(sched, N, strength):
    s = sched()
    _, begin = s.get_timesteps(N, strength)
    tab = s.blend_table(begin)
    assert tab.dtype == torch.float32 and tab.shape == (N - begin, 2)
    assert tab[-1].tolist() == [1.0, 0.0]
    for k in range(N - begin - 1):
        a, sg = s.add_noise_coefficients(begin + k + 1)
        assert tab[k, 0].item() == float(a) and tab[k, 1].item() == float(sg)
    with pytest.raises(ValueError):
        s.blend_table(N)


def test_ddim_suffix_table_is_a_slice():
    s = DDIMScheduler()
    s.set_timesteps(50)
    full = s.coefficient_table()
    for begin in (0, 1, 25, 49):
        assert torch.equal(s.coefficient_table(begin_index=begin), full[begin:])


@pytest.mark.parametrize("kw", [dict(), dict(solver_type="heun"), dict(algorithm_type="dpmsolver", final_sigmas_type="sigma_min")],
                         ids=["dpmsolver++-midpoint", "dpmsolver++-heun", "dpmsolver-sigma_min"])
@pytest.mark.parametrize("N,strength", [(25, 0.5), (20, 0.3), (10, 0.7), (12, 1.0)])
def test_dpm_suffix_rows_follow_restatement_from_a_begun_schedule(kw, N, strength):
    """Rows of the begun table, applied as x' = A x + B m0 + C (m0 - m1), reproduce diffusers' loop started at begin with an empty
    history (step_index = begin, lower_order_nums = 0), on an analytic model."""
    s = DPMSolverMultistepScheduler.from_config(DDIMScheduler().config, **kw)
    _, begin = s.get_timesteps(N, strength)
    rows = s.coefficient_table(begin_index=begin)
    full = s.coefficient_table()
    assert rows.shape == (N - begin, 8)
    assert rows[0, 4].item() == 0.0 and rows[0, 6].item() == 0.0              # first row: first order
    assert torch.equal(rows[0, :4], full[begin, :4]) and torch.equal(rows[1:], full[begin + 1:])
    r = DPMSolverRestatement(**kw)
    r.set_timesteps(N)
    r.step_index = begin                                                       # set_begin_index(begin)
    g = torch.Generator().manual_seed(N)
    x = torch.randn(2, 8, 5, 4, generator=g, dtype=torch.float64)
    xr, m1 = x.float(), None
    xt = x.clone()
    for k, t in enumerate(s.timesteps[begin:]):
        e = torch.tanh(xr) * 0.7 + 0.1                                        # any smooth model
        xr_next = r.step(e, t, xr).prev_sample
        A, B, C, convert, reads = (rows[k, j].double() for j in (2, 3, 4, 5, 6))
        alpha_s, sig_s = rows[k, 0].double(), rows[k, 1].double()
        et = (torch.tanh(xt.float()) * 0.7 + 0.1).double()
        m0 = (xt - sig_s * et) / alpha_s if convert else et
        xt = A * xt + B * m0 + C * (m0 - (m1 if reads else m0))
        m1 = m0
        xr = xr_next
        rel = float((xt - xr.double()).norm() / xr.double().norm())
        assert rel < 1e-5, (k, rel)


def test_dpm_add_noise_with_begin_index_needs_the_device():
    """add_noise exists (diffusers' surface) and refuses host tensors rather than falling back to the CPU"""
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(10)
    s.set_begin_index(4)
    assert s.begin_index == 4
    from audioldm_with_lora_amd import _lib
    with pytest.raises(_lib.AldmError):
        s.add_noise(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4), s.timesteps[4:5])
    s.set_timesteps(10)
    assert s.begin_index is None


# ---- masks ------------------------------------------------------------------------------------------------------------------------
def test_reduce_mask_is_cell_max():
    g = torch.Generator().manual_seed(2)
    m = (torch.rand(3, 16, 8, generator=g) > 0.9).float()
    got = reduce_mask(m, 4)
    assert got.shape == (3, 4, 2)
    for b in range(3):
        for i in range(4):
            for j in range(2):
                assert got[b, i, j].item() == m[b, 4 * i:4 * i + 4, 4 * j:4 * j + 4].max().item()
    frac = torch.full((1, 8, 8), 0.25)
    frac[0, 1, 6] = 0.75
    assert reduce_mask(frac, 4).tolist() == [[[0.25, 0.75], [0.25, 0.25]]]
    with pytest.raises(ValueError):
        reduce_mask(torch.ones(1, 10, 8), 4)
    with pytest.raises(ValueError):
        reduce_mask(torch.ones(10, 8), 4)


def test_regeneration_mask_edges():
    assert torch.equal(regeneration_mask(128, 64), torch.ones(128, 64))
    m = regeneration_mask(128, 64, seconds=(0.32, 0.64))
    assert m[:, 0].nonzero().flatten().tolist() == list(range(32, 64)) and torch.equal(m[:, 0:1].expand(-1, 64), m)
    m = regeneration_mask(128, 64, seconds=(0.325, 0.641))                     # partial frames are included
    assert m[:, 0].nonzero().flatten().tolist() == list(range(32, 65))
    m = regeneration_mask(100, 64, seconds=(0.5, 5.0))                         # clipped at the clip's end
    assert m[:, 0].nonzero().flatten().tolist() == list(range(50, 100))
    assert regeneration_mask(100, 64, seconds=(2.0, 3.0)).sum().item() == 0.0  # wholly past the end
    m = regeneration_mask(128, 64, bands=(0.5, 1.0))
    assert m[0].nonzero().flatten().tolist() == list(range(32, 64)) and torch.equal(m[0:1].expand(128, -1), m)
    m = regeneration_mask(128, 64, seconds=(0.0, 0.1), bands=(0.0, 0.25))
    assert m.sum().item() == 10 * 16 and m[:10, :16].min().item() == 1.0
    # after the latent max-pool the regenerated region covers what was asked
    m = regeneration_mask(128, 64, seconds=(0.35, 0.37), bands=(0.3, 0.31))     # frames 35, 36: two latent rows
    lat = reduce_mask(m[None], 4)[0]
    up = lat.repeat_interleave(4, 0).repeat_interleave(4, 1)
    assert bool((up >= m).all()) and lat.sum().item() == 2.0
    for bad in [dict(seconds=(0.5, 0.5)), dict(seconds=(-1.0, 1.0)), dict(bands=(0.5, 1.5)), dict(bands=(0.6, 0.5))]:
        with pytest.raises(ValueError):
            regeneration_mask(128, 64, **bad)


def test_pipeline_argument_errors_before_any_device_work():
    """The package exports the pipeline, and the pipeline refuses a CPU device before any other work"""
    from audioldm_with_lora_amd import AudioLDMAudioToAudioPipeline, _lib
    from audioldm_with_lora_amd.audio2audio import AudioLDMAudioToAudioPipeline as P
    assert AudioLDMAudioToAudioPipeline is P
    pipe = P.__new__(P)
    pipe.device = torch.device("cpu")
    with pytest.raises(_lib.AldmError):
        pipe(prompt_embeds=torch.zeros(1, 64), audio=torch.zeros(16000))


# ---- add_noise's index rule (diffusers 0.32 DPMSolverMultistepScheduler.add_noise) ------------------------------------------------
def test_dpm_add_noise_indices_follow_diffusers_branch_order():
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(10)
    ts = s.timesteps
    # (1) no begin index: index_for_timestep, per sample; an unknown timestep falls back to the last index
    assert s.add_noise_indices(ts[[3, 7]]) == [3, 7]
    assert s.add_noise_indices(torch.tensor([12345])) == [9]
    s._step_index = 5                                           # a step index does not matter without a begin index
    assert s.add_noise_indices(ts[2:3]) == [2]
    # (3) begin index, no step yet: the begin index whatever the timesteps
    s.set_timesteps(10)
    s.set_begin_index(4)
    assert s.add_noise_indices(ts[[0, 8]]) == [4, 4]
    # (2) begin index and a step has run: the current step index (diffusers' legacy inpaint loop noises to timesteps[i + 1])
    s._init_step_index(ts[0])
    assert s.step_index == 4                                    # a begun schedule starts at its begin index
    s._step_index += 1
    assert s.add_noise_indices(ts[5:6]) == [5] and s.add_noise_indices(ts[0:1]) == [5]


def test_dpm_index_for_timestep_duplicates_take_the_second_match():
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(10)
    s.timesteps = torch.tensor([901, 801, 801, 601], dtype=torch.int64)
    assert s.index_for_timestep(801) == 2 and s.index_for_timestep(901) == 0 and s.index_for_timestep(5) == 3


@pytest.mark.parametrize("dtype", ["uint8", "int16", "int32", "float32"])
def test_inference_script_reads_pcm_wavs_into_unit_range(tmp_path, dtype):
    import numpy as np
    from scipy.io import wavfile
    from audioldm_with_lora_amd.script.inference import read_wav
    x = np.array([-1.0, -0.5, 0.0, 0.5, 0.25], dtype=np.float64)
    if dtype == "uint8":
        raw = np.round(x * 128 + 128).clip(0, 255).astype(np.uint8)
    elif dtype == "float32":
        raw = x.astype(np.float32)
    else:
        full = -np.iinfo(dtype).min
        raw = np.round(x * full).clip(-full, full - 1).astype(dtype)
    f = str(tmp_path / "a.wav")
    wavfile.write(f, 16000, raw)
    sr, got = read_wav(f)
    assert sr == 16000 and got.dtype == np.float32 and got.shape == (5,)
    np.testing.assert_allclose(got, x, atol=1e-6)
    wavfile.write(f, 16000, np.stack([raw, raw], axis=1))           # stereo -> mono
    np.testing.assert_allclose(read_wav(f)[1], x, atol=1e-6)
