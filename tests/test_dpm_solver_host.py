"""DPMSolverMultistepScheduler host logic (no GPU): timesteps and sigmas, the per-row order schedule, the coefficient table against
the restatement (tests/dpm_restatement.py), configuration round trips and errors, and the solver's order on an analytic model."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dpm_restatement import DPMSolverRestatement  # noqa: E402


def _dpm(**kw):
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(DDIMScheduler().config, **kw)


@pytest.mark.parametrize("n", [10, 20, 25, 50, 200])
def test_leading_timesteps_closed_form(n):
    s = _dpm()
    s.set_timesteps(n)
    ratio = 1000 // (n + 1)
    want = np.array([(n - k) * ratio + 1 for k in range(n)], dtype=np.int64)
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), want)
    if n == 25:
        assert int(s.timesteps[0]) == 951 and int(s.timesteps[-1]) == 39 and set(np.diff(want).tolist()) == {-38}


@pytest.mark.parametrize("n", [10, 25, 50])
def test_linspace_and_trailing_timesteps(n):
    s = _dpm(timestep_spacing="linspace")
    s.set_timesteps(n)
    want = np.array([round(999 * (n - k) / n) for k in range(n)], dtype=np.int64)   # linspace(0, 999, n+1)[::-1][:-1]
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), want)
    s = _dpm(timestep_spacing="trailing")
    s.set_timesteps(n)
    want = np.array([round(1000 - k * 1000 / n) - 1 for k in range(n)], dtype=np.int64)
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), want)
    assert int(s.timesteps[0]) == 999


@pytest.mark.parametrize("n", [10, 25])
def test_sigmas(n):
    s = _dpm()
    s.set_timesteps(n)
    ac = s.alphas_cumprod
    want = ((1 - ac) / ac) ** 0.5
    assert s.sigmas.dtype == torch.float32 and s.sigmas.numel() == n + 1 and float(s.sigmas[-1]) == 0.0
    assert torch.equal(s.sigmas[:-1], want[s.timesteps])
    s = _dpm(final_sigmas_type="sigma_min")
    s.set_timesteps(n)
    assert float(s.sigmas[-1]) == float(want[0])


def _orders(s):
    return [int(r) + 1 for r in s.coefficient_table()[:, 6].tolist()]


def test_row_order_schedule():
    for n in (15, 25, 50):
        s = _dpm()
        s.set_timesteps(n)
        assert _orders(s) == [1] + [2] * (n - 2) + [1]
        s = _dpm(final_sigmas_type="sigma_min")                   # N >= 15: no lower_order_final, the last row stays second order
        s.set_timesteps(n)
        assert _orders(s) == [1] + [2] * (n - 1)
        s = _dpm(final_sigmas_type="sigma_min", euler_at_final=True)
        s.set_timesteps(n)
        assert _orders(s) == [1] + [2] * (n - 2) + [1]
    s = _dpm(final_sigmas_type="sigma_min")
    s.set_timesteps(10)
    assert _orders(s) == [1] + [2] * 8 + [1]                      # N < 15: lower_order_final
    for n in (10, 25):
        s = _dpm(solver_order=1)
        s.set_timesteps(n)
        assert _orders(s) == [1] * n
        assert float(s.coefficient_table()[:, 4].abs().max()) == 0.0


CASES = [dict(), dict(solver_type="heun"), dict(solver_order=1), dict(final_sigmas_type="sigma_min"),
         dict(algorithm_type="dpmsolver", final_sigmas_type="sigma_min"),
         dict(algorithm_type="dpmsolver", final_sigmas_type="sigma_min", solver_type="heun"),
         dict(timestep_spacing="trailing"), dict(timestep_spacing="linspace", euler_at_final=True)]


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "default")
@pytest.mark.parametrize("n", [10, 25, 200])
def test_coefficient_table_matches_restatement(kw, n):
    s = _dpm(**kw)
    s.set_timesteps(n)
    r = DPMSolverRestatement(**kw)
    r.set_timesteps(n)
    got, want = s.coefficient_table(), r.coefficient_rows()
    assert torch.equal(s.timesteps, r.timesteps) and torch.equal(s.sigmas, r.sigmas)
    assert got.dtype == torch.float32 and got.shape == (n, 8) and torch.isfinite(got).all()
    torch.testing.assert_close(got, want, rtol=1e-6, atol=0)
    if kw.get("algorithm_type", "dpmsolver++") == "dpmsolver++" and kw.get("final_sigmas_type", "zero") == "zero":
        assert got[-1, 2:7].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0]          # final row: x' = m0 (A = 0, B = 1, C = 0)


def test_from_config_round_trips():
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    d = DDIMScheduler()
    s = DPMSolverMultistepScheduler.from_config(d.config)
    assert s.config.timestep_spacing == "leading" and s.config.steps_offset == 1
    assert torch.equal(s.betas, d.betas) and torch.equal(s.alphas_cumprod, d.alphas_cumprod)
    assert not hasattr(s.config, "clip_sample") and not hasattr(s.config, "set_alpha_to_one")
    assert vars(DDIMScheduler.from_config(s.config).config) == vars(d.config)
    assert vars(DPMSolverMultistepScheduler.from_config(DDIMScheduler.from_config(s.config).config).config) == vars(s.config)
    assert vars(DPMSolverMultistepScheduler.from_config(vars(s.config)).config) == vars(s.config)          # a plain dict
    h = DPMSolverMultistepScheduler.from_config(s.config, solver_type="heun", clip_sample=True)
    assert h.config.solver_type == "heun" and s.config.solver_type == "midpoint"
    assert s.init_noise_sigma == 1.0
    x = torch.randn(3)
    assert s.scale_model_input(x, 5) is x


def test_from_pretrained(tmp_path):
    import json
    from audioldm_with_lora_amd.scheduler import DPMSolverMultistepScheduler
    os.makedirs(tmp_path / "scheduler")
    cfg = {"_class_name": "DDIMScheduler", "num_train_timesteps": 1000, "beta_start": 0.0015, "beta_end": 0.0195,
           "beta_schedule": "scaled_linear", "clip_sample": False, "set_alpha_to_one": False, "steps_offset": 1,
           "prediction_type": "epsilon", "timestep_spacing": "leading"}
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    s = DPMSolverMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    s.set_timesteps(25)
    assert int(s.timesteps[0]) == 951
    with pytest.raises(FileNotFoundError):
        DPMSolverMultistepScheduler.from_pretrained(str(tmp_path), subfolder="nope")


@pytest.mark.parametrize("kw,exc,word", [
    (dict(algorithm_type="sde-dpmsolver++"), NotImplementedError, "sde-dpmsolver++"),
    (dict(algorithm_type="sde-dpmsolver", final_sigmas_type="sigma_min"), NotImplementedError, "sde-dpmsolver"),
    (dict(solver_order=3), NotImplementedError, "solver_order"),
    (dict(thresholding=True), NotImplementedError, "thresholding"),
    (dict(use_karras_sigmas=True), NotImplementedError, "use_karras_sigmas"),
    (dict(use_exponential_sigmas=True), NotImplementedError, "use_exponential_sigmas"),
    (dict(use_beta_sigmas=True), NotImplementedError, "use_beta_sigmas"),
    (dict(use_lu_lambdas=True), NotImplementedError, "use_lu_lambdas"),
    (dict(prediction_type="v_prediction"), NotImplementedError, "v_prediction"),
    (dict(beta_schedule="linear"), NotImplementedError, "beta_schedule"),
    (dict(algorithm_type="dpmsolver"), ValueError, "final_sigmas_type"),
])
def test_unsupported_options_raise(kw, exc, word):
    import re
    with pytest.raises(exc, match=re.escape(word)):
        _dpm(**kw)


def test_product_step_has_no_cpu_fallback():
    from audioldm_with_lora_amd._lib import AldmError
    s = _dpm()
    s.set_timesteps(10)
    with pytest.raises(AldmError):
        s.step(torch.zeros(2, 4), s.timesteps[0], torch.zeros(2, 4))


# ---- the solver's order on an analytic model -----------------------------------------------------------------------------
# Data x0 ~ N(mu, s^2) per element: the exact eps-prediction is sqrt(1-a)(x - sqrt(a) mu) / (a s^2 + 1 - a), and the exact
# probability-flow ODE keeps z = (x - sqrt(a) mu) / sqrt(a s^2 + 1 - a) constant, so every intermediate state is known.
MU = 0.4


def _eps(x, a, s):
    return math.sqrt(1 - a) * (x - math.sqrt(a) * MU) / (a * s * s + 1 - a)


def _flow_error(table, sigmas, s, mu=MU):
    """Largest deviation from the exact flow of the intermediate states (steps 0 .. N-2), x over [-2, 2], numpy loop over the rows."""
    tab = table.double().numpy()
    a_of = 1.0 / (1.0 + sigmas.double().numpy() ** 2)          # alpha^2 at every point of the schedule
    x = np.linspace(-2.0, 2.0, 81)
    z = (x - math.sqrt(a_of[0]) * mu) / math.sqrt(a_of[0] * s * s + 1 - a_of[0])
    m1 = np.zeros_like(x)
    err = 0.0
    for i in range(len(tab) - 1):
        alpha_s, sig_s, A, B, C, conv, second = tab[i, :7]
        e = _eps(x, a_of[i], s)
        m0 = (x - sig_s * e) / alpha_s if conv else e
        x = A * x + B * m0 + (C * (m0 - m1) if second else 0.0)
        m1 = m0
        a = a_of[i + 1]
        exact = math.sqrt(a) * mu + z * math.sqrt(a * s * s + 1 - a)
        err = max(err, float(np.abs(x - exact).max()))
    return err


def _err(order, n, s):
    sch = _dpm(solver_order=order)
    sch.set_timesteps(n)
    return _flow_error(sch.coefficient_table(), sch.sigmas, s)


@pytest.mark.parametrize("s", [0.5, 1.5, 3.0])
def test_second_order_converges_faster_on_analytic_model(s):
    for n in (10, 20, 40):
        e1, e2 = _err(1, n, s), _err(2, n, s)
        assert np.isfinite(e1) and np.isfinite(e2) and e2 * 4 <= e1, (n, e1, e2)
    assert _err(2, 20, s) < _err(1, 160, s)


def test_restatement_loop_follows_exact_flow():
    """The restatement's own step() (diffusers' form) tracks the table loop on the same analytic model."""
    r = DPMSolverRestatement()
    r.set_timesteps(20)
    s = _dpm()
    s.set_timesteps(20)
    x0 = torch.linspace(-2, 2, 81, dtype=torch.float32)
    x = x0.clone()
    tab = s.coefficient_table().double().numpy()
    xn, m1 = x0.double().numpy(), np.zeros(81)
    for i, t in enumerate(r.timesteps):
        a = float(s.alphas_cumprod[int(t)])
        a_sig = 1.0 / (1.0 + float(s.sigmas[i]) ** 2)
        x = r.step(torch.from_numpy(_eps(x.double().numpy(), a_sig, 1.5)).float(), t, x).prev_sample
        alpha_s, sig_s, A, B, C, conv, second = tab[i, :7]
        e = _eps(xn, a_sig, 1.5)
        m0 = (xn - sig_s * e) / alpha_s
        xn = A * xn + B * m0 + (C * (m0 - m1) if second else 0.0)
        m1 = m0
        assert abs(a - a_sig) < 1e-6
        np.testing.assert_allclose(x.double().numpy(), xn, rtol=1e-4, atol=1e-4)
