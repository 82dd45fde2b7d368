"""CPU: RePaintScheduler's host side -- the walk, its folding and the timesteps against the pinned literal and
tests/repaint_restatement.py, the coefficient / blend tables against the float64 restatement, the reduction to DDIMScheduler without
jumps, the refused options, no CPU fallback, and the Gaussian property RePaint exists for, on the restatement."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repaint_restatement as R  # noqa: E402

from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, RePaintScheduler  # noqa: E402

TRIPLES = [(50, 10, 10), (20, 5, 3), (10, 2, 2), (12, 4, 3)]


def _repaint(**kw):
    return RePaintScheduler.from_config(DDIMScheduler().config, **kw)


def _record(v, what):
    import conftest
    return conftest.record(v, what)


def test_walk_fold_and_timesteps_pinned_literal():
    s = _repaint(jump_length=2, jump_n_sample=2)
    s.set_timesteps(6)
    assert s.walk == [5, 4, 3, 2, 3, 4, 3, 2, 1, 0, 1, 2, 1, 0]
    assert s.folded == [(5, 0), (4, 0), (3, 0), (2, 2), (3, 0), (2, 0), (1, 0), (0, 2), (1, 0), (0, 0)]
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == [831, 665, 499, 333, 499, 333, 167, 1, 167, 1]
    assert s.num_inference_steps == 6 and s.init_noise_sigma == 1.0
    x = torch.ones(3)
    assert s.scale_model_input(x, 831) is x


@pytest.mark.parametrize("N,jl,js,L", [t + (n,) for t, n in zip(TRIPLES, (410, 50, 18, 28))])
def test_walk_fold_and_timesteps_against_restatement(N, jl, js, L):
    s, r = _repaint(jump_length=jl, jump_n_sample=js), R.RePaintRestatement(jl, js)
    s.set_timesteps(N)
    r.set_timesteps(N)
    assert s.walk == r.walk and s.folded == r.folded and np.array_equal(s.timesteps.numpy(), r.timesteps)
    assert len(s.timesteps) == L == R.n_calls(N, jl, js)
    # the walk ends at level 0, never leaves the grid, and moves one level at a time
    assert s.walk[0] == N - 1 and s.walk[-1] == 0 and min(s.walk) == 0 and max(s.walk) == N - 1
    assert all(abs(a - b) == 1 for a, b in zip(s.walk, s.walk[1:]))
    # set_timesteps' own arguments override the configuration for that schedule
    s.set_timesteps(N, jump_length=1, jump_n_sample=1)
    assert len(s.timesteps) == N


def test_without_jumps_it_is_ddim():
    for N in (10, 37):
        s, d = _repaint(jump_n_sample=1), DDIMScheduler()
        s.set_timesteps(N)
        d.set_timesteps(N)
        tab = s.coefficient_table()
        assert torch.equal(s.timesteps, d.timesteps) and tab.dtype == torch.float32 and tab.shape == (N, 8)
        assert torch.equal(tab[:, :4], d.coefficient_table())
        assert torch.equal(tab[:, 4:6], torch.tensor([[1.0, 0.0]]).expand(N, 2)) and torch.equal(tab[:, 6:], torch.zeros(N, 2))
        # the blend rows are the legacy loop's (the noise differs, not the level)
        assert torch.equal(s.blend_table(), d.blend_table(0))
    # a jump longer than the schedule leaves nothing to jump from
    s = _repaint(jump_length=10, jump_n_sample=10)
    s.set_timesteps(10)
    d.set_timesteps(10)
    assert torch.equal(s.timesteps, d.timesteps)


@pytest.mark.parametrize("N,jl,js", TRIPLES)
def test_tables_against_restatement(N, jl, js):
    s, r = _repaint(jump_length=jl, jump_n_sample=js), R.RePaintRestatement(jl, js)
    s.set_timesteps(N)
    r.set_timesteps(N)
    tab, bl = s.coefficient_table(), s.blend_table()
    L = len(s.timesteps)
    assert tab.dtype == bl.dtype == torch.float32 and tab.shape == (L, 8) and bl.shape == (L, 2)
    want, wbl = r.table(), r.blend_table()
    # relative error per entry <= 1e-6 (the bound tests/test_dpm_solver_host.py holds its tables to); exact zeros stay zeros
    worst = 0.0
    for got, ref in ((tab.double().numpy(), want), (bl.double().numpy(), wbl)):
        assert np.array_equal(got == 0, ref == 0)
        nz = ref != 0
        worst = max(worst, float(np.abs(got[nz] / ref[nz] - 1).max()))
    _record(worst, "table_max_rel")
    assert worst <= 1e-6, worst
    J = np.array([j for _, j in s.folded])
    assert torch.equal(bl[-1], torch.tensor([1.0, 0.0]))
    assert torch.equal(tab[torch.from_numpy(J == 0)][:, 4:6], torch.tensor([[1.0, 0.0]]).expand(int((J == 0).sum()), 2))
    c1, c2 = tab[:, 4].double(), tab[:, 5].double()
    assert torch.all((c1 ** 2 + c2 ** 2 - 1).abs() <= 4 * 2.0 ** -24)
    assert torch.all(c2[torch.from_numpy(J > 0)] > 0) and torch.all(c1[torch.from_numpy(J > 0)] < 1)
    # an arrival at level -1 that is not the last row uses final_alpha_cumprod
    first0 = next(k for k, (l, _) in enumerate(s.folded) if l == 0)
    if first0 != L - 1:
        a = s.final_alpha_cumprod
        assert torch.equal(bl[first0], torch.stack([a ** 0.5, (1 - a) ** 0.5]))
    # add_noise_coefficients index the folded list
    a, sg = s.add_noise_coefficients(first0)
    ac = s.alphas_cumprod[int(s.timesteps[first0])]
    assert float(a) == float(ac ** 0.5) and float(sg) == float((1 - ac) ** 0.5)


def test_get_timesteps_accepts_strength_one_only():
    s = _repaint(jump_length=2, jump_n_sample=2)
    ts, begin = s.get_timesteps(6, 1.0)
    assert begin == 0 and len(ts) == 10 and torch.equal(ts, s.timesteps)
    with pytest.raises(ValueError, match="from noise"):
        s.get_timesteps(6, 0.5)
    with pytest.raises(NotImplementedError, match="begin_index"):
        s.coefficient_table(begin_index=2)
    with pytest.raises(NotImplementedError, match="begin_index"):
        s.blend_table(2)


@pytest.mark.parametrize("kw,name", [(dict(eta=0.5), "eta"), (dict(clip_sample=True), "clip_sample"),
                                     (dict(prediction_type="v_prediction"), "prediction_type"),
                                     (dict(beta_schedule="linear"), "beta_schedule"),
                                     (dict(timestep_spacing="trailing"), "timestep_spacing")])
def test_unsupported_options_raise_and_name_the_option(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        RePaintScheduler(**kw)


@pytest.mark.parametrize("kw,name", [(dict(jump_length=0), "jump_length"), (dict(jump_n_sample=0), "jump_n_sample")])
def test_bad_jump_parameters_raise(kw, name):
    with pytest.raises(ValueError, match=name):
        RePaintScheduler(**kw)
    s = RePaintScheduler()
    with pytest.raises(ValueError, match=name):
        s.set_timesteps(10, **kw)


def test_existing_refusals_still_raise():
    with pytest.raises(NotImplementedError):
        DDIMScheduler().step(torch.zeros(1), 1, torch.zeros(1), eta=0.5)
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")


def test_config_round_trip_and_surface(tmp_path):
    import json
    ddim = DDIMScheduler()
    s = RePaintScheduler.from_config(ddim.config, jump_length=5, jump_n_sample=3)
    for k, v in vars(ddim.config).items():
        assert getattr(s.config, k) == v
    assert (s.config.jump_length, s.config.jump_n_sample, s.config.eta) == (5, 3, 0.0)
    assert (RePaintScheduler().config.jump_length, RePaintScheduler().config.jump_n_sample) == (10, 10)
    assert vars(DDIMScheduler.from_config(s.config).config) == vars(ddim.config)
    assert vars(RePaintScheduler.from_config(vars(s.config)).config) == vars(s.config)
    # the pipelines key their engine cache by the frozen configuration: the jump parameters must be in it
    from audioldm_with_lora_amd.pipeline import _frozen_config
    assert _frozen_config(s) != _frozen_config(RePaintScheduler.from_config(ddim.config, jump_length=5, jump_n_sample=4))
    d = tmp_path / "scheduler"
    d.mkdir()
    (d / "scheduler_config.json").write_text(json.dumps(dict(vars(s.config), _class_name="RePaintScheduler")))
    p = RePaintScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    assert vars(p.config) == vars(s.config)
    import audioldm_with_lora_amd
    assert audioldm_with_lora_amd.RePaintScheduler is RePaintScheduler
    assert "1 = REGENERATE" in RePaintScheduler.__doc__ and "opposite" in RePaintScheduler.__doc__


def test_no_cpu_fallback():
    from audioldm_with_lora_amd._lib import AldmError
    s = _repaint(jump_length=2, jump_n_sample=2)
    z = torch.zeros(1, 4)
    with pytest.raises(ValueError):
        s.step(z, 831, z, z, torch.ones(1, 4))                              # no schedule yet
    s.set_timesteps(6)
    with pytest.raises(AldmError):
        s.step(z, 831, z, z, torch.ones(1, 4), generator=3)
    with pytest.raises(AldmError):
        s.undo_step(z, 333, generator=3)
    with pytest.raises(AldmError):
        s.add_noise(z, z, s.timesteps[:1])


def test_restatement_step_is_the_documented_update():
    r = R.RePaintRestatement(2, 2)
    r.set_timesteps(6)
    g = torch.Generator().manual_seed(0)
    x, e, x0, zk, zj = (torch.randn(2, 3, generator=g, dtype=torch.float64) for _ in range(5))
    m = torch.tensor([0.0, 1.0, 0.25], dtype=torch.float64)
    ac = r.alphas_cumprod
    # call 3 stands at level 2 (t = 333), lands on level 1 (t = 167) and jumps to level 3 (t = 499)
    a, ap, aj = ac[333], ac[167], ac[499]
    unknown = np.sqrt(ap) * (x - np.sqrt(1 - a) * e) / np.sqrt(a) + np.sqrt(1 - ap) * e
    xb = (1 - m) * (np.sqrt(ap) * x0 + np.sqrt(1 - ap) * zk) + m * unknown
    want = np.sqrt(aj / ap) * xb + np.sqrt(1 - aj / ap) * zj
    torch.testing.assert_close(r.step(3, e, x, x0, m, zk, zj), want, rtol=1e-14, atol=1e-14)
    # the last call: no jump, and the kept pixel is x0 itself
    out = r.step(9, e, x, x0, m, zk, zj)
    assert torch.equal(out[:, 0], x0[:, 0]) and not torch.equal(out[:, 1], x0[:, 1])
    # J single-beta steps compose to the closed form: prod(1 - beta) over the timesteps between two levels is the alpha-bar ratio
    betas = (torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float32) ** 2).double().numpy()
    prod = np.prod(1 - betas[168:500])
    assert abs(prod / (aj / ap) - 1) <= 1e-4                                # (the fp32 cumprod table against a float64 product)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gaussian_property_on_the_restatement(seed):
    """Two pixels with data correlation 0.9, one kept and one regenerated, exact eps, 20 000 problems, N = 10, jump_length = 2: the
    slope of the regenerated pixel on the kept one (0.9 for the true conditional) is in [0.38, 0.47] without resampling and in
    [0.64, 0.73] at jump_n_sample = 4.  Measured: 0.417 .. 0.423 and 0.684 .. 0.688 over these seeds."""
    plain, resampled = R.gaussian_slope(1, seed), R.gaussian_slope(4, seed)
    _record(plain, "slope_jump_n_sample_1")
    _record(resampled, "slope_jump_n_sample_4")
    print(f"seed {seed}: slope {plain:.4f} without jumps, {resampled:.4f} at jump_n_sample = 4 (true conditional 0.9)")
    assert 0.38 <= plain <= 0.47, plain
    assert 0.64 <= resampled <= 0.73, resampled
