"""UniPCMultistepScheduler host logic (no GPU): the coefficient table against the restatement (tests/unipc_restatement.py) on an
analytic model, the pin of the predictor against DPMSolverMultistepScheduler's merged table, the accuracy against DPM-Solver++ 2M at
5 and 8 steps, exact entries of the table, configuration round trips and refusals."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from unipc_restatement import UniPCRestatement  # noqa: E402

# columns of a row (scheduler.py UniPCMultistepScheduler)
ALPHA, SIG, AC, BC, CC, DC, AP, BP, CP, CONVERT, CORR, CORR_M1, PRED_M0 = range(13)


def _unipc(**kw):
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, UniPCMultistepScheduler
    return UniPCMultistepScheduler.from_config(DDIMScheduler().config, **kw)


def _dpm(**kw):
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(DDIMScheduler().config, **kw)


# ---- the analytic model of tests/test_dpm_solver_host.py ------------------------------------------------------------------
# Data x0 ~ N(mu, s^2) per element: the exact eps-prediction is sqrt(1-a)(x - sqrt(a) mu) / (a s^2 + 1 - a), and the exact
# probability-flow ODE keeps z = (x - sqrt(a) mu) / sqrt(a s^2 + 1 - a) constant, so every intermediate state is known.
MU = 0.4


def _eps(x, a, s):
    return math.sqrt(1 - a) * (x - math.sqrt(a) * MU) / (a * s * s + 1 - a)


def apply_unipc_rows(table, sigmas, s, x, first=0):
    """The device update restated in numpy float64 over the rows of `table` (which starts at schedule index `first`); yields the
    state after every row.  m0 / m1 / last start as NaN: a row that reads what its flags do not ask for poisons the result."""
    tab = table.double().numpy()
    a_of = 1.0 / (1.0 + sigmas.double().numpy() ** 2)
    nan = np.full_like(x, np.nan)
    last, m0, m1 = nan, nan, nan
    for k in range(len(tab)):
        r = tab[k]
        e = _eps(x, a_of[first + k], s)
        mt = (x - r[SIG] * e) / r[ALPHA] if r[CONVERT] else e
        xc = x
        if r[CORR]:
            xc = r[AC] * last + r[BC] * m0 + (r[CC] * (m1 - m0) if r[CORR_M1] else 0.0) + r[DC] * (mt - m0)
        x = r[AP] * xc + r[BP] * mt + (r[CP] * (mt - m0) if r[PRED_M0] else 0.0)
        last, m1, m0 = xc, m0, mt
        yield x


VARIANTS = [dict(), dict(solver_type="bh1"), dict(solver_order=1), dict(solver_order=1, solver_type="bh1"),
            dict(predict_x0=False, final_sigmas_type="sigma_min"), dict(predict_x0=False, final_sigmas_type="sigma_min", solver_type="bh1"),
            dict(predict_x0=False, final_sigmas_type="sigma_min", solver_order=1), dict(final_sigmas_type="sigma_min"),
            dict(final_sigmas_type="sigma_min", lower_order_final=False), dict(timestep_spacing="linspace"),
            dict(timestep_spacing="trailing"), dict(timestep_spacing="trailing", solver_type="bh1"), dict(disable_corrector=[0, 3]),
            dict(lower_order_final=False, solver_order=1)]
_ids = lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "default"  # noqa: E731


@pytest.mark.parametrize("kw", VARIANTS, ids=_ids)
@pytest.mark.parametrize("n", [5, 8, 9, 20])
def test_table_matches_restatement_on_analytic_model(kw, n):
    """rows of coefficient_table() applied in numpy against the restatement's step() loop (diffusers' form, fp32), state by state"""
    s = _unipc(**kw)
    s.set_timesteps(n)
    r = UniPCRestatement(**kw)
    r.set_timesteps(n)
    assert torch.equal(s.timesteps, r.timesteps) and torch.equal(s.sigmas, r.sigmas)
    tab = s.coefficient_table()
    assert tab.dtype == torch.float32 and tab.shape == (n, 16) and torch.isfinite(tab).all()
    x0 = np.linspace(-2.0, 2.0, 81)
    x = torch.from_numpy(x0).float()
    rows = apply_unipc_rows(tab, s.sigmas, 1.5, x0)
    for i, t in enumerate(r.timesteps):
        a = 1.0 / (1.0 + float(s.sigmas[i]) ** 2)
        x = r.step(torch.from_numpy(_eps(x.double().numpy(), a, 1.5)).float(), t, x).prev_sample
        want = next(rows)
        assert torch.isfinite(x).all()
        np.testing.assert_allclose(x.double().numpy(), want, rtol=1e-4, atol=1e-4, err_msg=f"step {i}")


@pytest.mark.parametrize("begin", [1, 2, 5])
@pytest.mark.parametrize("kw", [dict(), dict(solver_type="bh1", disable_corrector=[3])], ids=_ids)
def test_begun_table_matches_restatement(kw, begin):
    """a schedule begun at begin_index (audio-to-audio): empty history, the final-step rule on the full N"""
    n = 9
    s = _unipc(**kw)
    s.set_timesteps(n)
    r = UniPCRestatement(**kw)
    r.set_timesteps(n)
    r.set_begin_index(begin)
    tab = s.coefficient_table(begin)
    assert tab.shape == (n - begin, 16)
    x0 = np.linspace(-2.0, 2.0, 81)
    x = torch.from_numpy(x0).float()
    rows = apply_unipc_rows(tab, s.sigmas, 1.5, x0, first=begin)
    for i in range(begin, n):
        a = 1.0 / (1.0 + float(s.sigmas[i]) ** 2)
        x = r.step(torch.from_numpy(_eps(x.double().numpy(), a, 1.5)).float(), r.timesteps[i], x).prev_sample
        np.testing.assert_allclose(x.double().numpy(), next(rows), rtol=1e-4, atol=1e-4, err_msg=f"step {i}")


@pytest.mark.parametrize("n", [5, 10, 25])
def test_predictor_without_corrector_is_dpm_solver_pp_2m(n):
    """with the corrector off on every step, {Ap, Bp, Cp} are DPMSolverMultistepScheduler's {A, B, C} row for row (merged code)"""
    u = _unipc(disable_corrector=list(range(n)))
    u.set_timesteps(n)
    d = _dpm()
    d.set_timesteps(n)
    tu, td = u.coefficient_table(), d.coefficient_table()
    assert torch.equal(u.timesteps, d.timesteps) and torch.equal(u.sigmas, d.sigmas)
    assert float(tu[:, CORR].abs().max()) == 0.0 and float(tu[:, AC:DC + 1].abs().max()) == 0.0
    torch.testing.assert_close(tu[:, [ALPHA, SIG]], td[:, [0, 1]], rtol=0, atol=0)
    torch.testing.assert_close(tu[:, [AP, BP, CP]], td[:, [2, 3, 4]], rtol=1e-5, atol=0)
    assert torch.equal(tu[:, PRED_M0], td[:, 6]) and torch.equal(tu[:, CONVERT], td[:, 5])


def _flow_error_unipc(table, sigmas, s):
    """Largest deviation from the exact flow of the intermediate states (steps 0 .. N-2), x over [-2, 2] -- the measure of
    test_dpm_solver_host._flow_error"""
    a_of = 1.0 / (1.0 + sigmas.double().numpy() ** 2)
    x0 = np.linspace(-2.0, 2.0, 81)
    z = (x0 - math.sqrt(a_of[0]) * MU) / math.sqrt(a_of[0] * s * s + 1 - a_of[0])
    err = 0.0
    for i, x in enumerate(apply_unipc_rows(table[:-1], sigmas, s, x0)):
        a = a_of[i + 1]
        err = max(err, float(np.abs(x - (math.sqrt(a) * MU + z * math.sqrt(a * s * s + 1 - a))).max()))
    return err


def _flow_error_dpm(table, sigmas, s):
    tab = table.double().numpy()
    a_of = 1.0 / (1.0 + sigmas.double().numpy() ** 2)
    x = np.linspace(-2.0, 2.0, 81)
    z = (x - math.sqrt(a_of[0]) * MU) / math.sqrt(a_of[0] * s * s + 1 - a_of[0])
    m1, err = np.zeros_like(x), 0.0
    for i in range(len(tab) - 1):
        alpha_s, sig_s, A, B, C, conv, second = tab[i, :7]
        e = _eps(x, a_of[i], s)
        m0 = (x - sig_s * e) / alpha_s if conv else e
        x = A * x + B * m0 + (C * (m0 - m1) if second else 0.0)
        m1 = m0
        a = a_of[i + 1]
        err = max(err, float(np.abs(x - (math.sqrt(a) * MU + z * math.sqrt(a * s * s + 1 - a))).max()))
    return err


def test_more_accurate_than_dpm_solver_pp_at_few_steps():
    """UniPC order 2 bh2 against DPM-Solver++ 2M on the analytic model: 1.3 x less flow error at N = 5 and 8 (float64 ratios 1.6-2.2)"""
    ratios = {}
    for s in (0.5, 1.5, 3.0):
        for n in (5, 8):
            u, d = _unipc(), _dpm()
            u.set_timesteps(n)
            d.set_timesteps(n)
            eu, ed = _flow_error_unipc(u.coefficient_table(), u.sigmas, s), _flow_error_dpm(d.coefficient_table(), d.sigmas, s)
            off = _unipc(disable_corrector=list(range(n)))
            off.set_timesteps(n)
            e_off = _flow_error_unipc(off.coefficient_table(), off.sigmas, s)
            ratios[(s, n)] = ed / eu
            print(f"s={s} N={n}: unipc {eu:.3e}  dpm++2M {ed:.3e}  ratio {ed / eu:.2f}  (corrector off {e_off:.3e})")
            assert abs(e_off - ed) <= 1e-4 * ed, (s, n, e_off, ed)          # corrector off IS DPM-Solver++ 2M
    for k, v in ratios.items():
        assert np.isfinite(v) and v >= 1.3, (k, v)


def test_exact_entries():
    for kw in (dict(), dict(solver_type="bh1"), dict(timestep_spacing="trailing")):
        for n in (5, 9, 20):
            s = _unipc(**kw)
            s.set_timesteps(n)
            t = s.coefficient_table()
            # row 0: no corrector, first-order predictor, reads nothing
            assert t[0, AC:DC + 1].tolist() == [0.0] * 4 and float(t[0, CP]) == 0.0
            assert t[0, CONVERT:].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
            # row 1: first-order corrector (Cc == 0, m1 unread), second-order predictor
            assert float(t[1, CC]) == 0.0 and t[1, CORR:PRED_M0 + 1].tolist() == [1.0, 0.0, 1.0]
            assert t[2, CORR:PRED_M0 + 1].tolist() == [1.0, 1.0, 1.0] and float(t[2, CC]) != 0.0
            # the row that steps to sigma 0: x' = m_t exactly, after a second-order corrector
            assert t[-1, AP:CP + 1].tolist() == [0.0, 1.0, 0.0] and t[-1, CORR:PRED_M0 + 1].tolist() == [1.0, 1.0, 0.0]
            assert [s.row_order(i) for i in range(n)] == [1] + [2] * (n - 2) + [1]
    s = _unipc(solver_order=1)
    s.set_timesteps(9)
    t = s.coefficient_table()
    assert float(t[:, CC].abs().max()) == 0.0 and float(t[:, CP].abs().max()) == 0.0
    assert float(t[:, CORR_M1].abs().max()) == 0.0 and float(t[:, PRED_M0].abs().max()) == 0.0
    assert t[:, CORR].tolist() == [0.0] + [1.0] * 8
    s = _unipc(disable_corrector=[0, 3])
    s.set_timesteps(9)
    assert s.coefficient_table()[:, CORR].tolist() == [0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    s = _unipc(final_sigmas_type="sigma_min", lower_order_final=False)
    s.set_timesteps(9)
    assert [s.row_order(i) for i in range(9)] == [1] + [2] * 8


@pytest.mark.parametrize("begin", [1, 4, 8])
def test_begun_schedule_first_row(begin):
    s = _unipc()
    s.set_timesteps(9)
    full, t = s.coefficient_table(), s.coefficient_table(begin)
    assert t.shape == (9 - begin, 16)
    assert t[0, AC:DC + 1].tolist() == [0.0] * 4 and float(t[0, CP]) == 0.0 and t[0, CORR:PRED_M0 + 1].tolist() == [0.0, 0.0, 0.0]
    assert torch.equal(t[0, [ALPHA, SIG, AP, BP]], full[begin, [ALPHA, SIG, AP, BP]])
    if len(t) > 1:
        assert t[1, CORR:CORR_M1 + 1].tolist() == [1.0, 0.0] and float(t[1, CC]) == 0.0       # a first-order corrector
    if len(t) > 2:
        assert torch.equal(t[2:], full[begin + 2:])
    assert t[-1, AP:CP + 1].tolist() == [0.0, 1.0, 0.0]                                        # the final rule: full N
    with pytest.raises(ValueError):
        s.coefficient_table(9)


def test_from_config_round_trips():
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
    d = DDIMScheduler()
    s = UniPCMultistepScheduler.from_config(d.config)
    assert s.config.timestep_spacing == "leading" and s.config.steps_offset == 1
    assert (s.config.solver_order, s.config.predict_x0, s.config.solver_type, s.config.lower_order_final, s.config.disable_corrector,
            s.config.final_sigmas_type) == (2, True, "bh2", True, [], "zero")
    assert torch.equal(s.betas, d.betas) and torch.equal(s.alphas_cumprod, d.alphas_cumprod)
    assert not hasattr(s.config, "clip_sample")
    assert vars(DDIMScheduler.from_config(s.config).config) == vars(d.config)
    p = DPMSolverMultistepScheduler.from_config(d.config, solver_order=1)
    u = UniPCMultistepScheduler.from_config(p.config)                      # from a DPM config: shared keys carry over, midpoint does not
    assert u.config.solver_order == 1 and u.config.solver_type == "bh2" and not hasattr(u.config, "algorithm_type")
    assert vars(UniPCMultistepScheduler.from_config(vars(s.config)).config) == vars(s.config)
    b = UniPCMultistepScheduler.from_config(s.config, solver_type="bh1", clip_sample=True)
    assert b.config.solver_type == "bh1" and s.config.solver_type == "bh2"
    assert s.init_noise_sigma == 1.0
    x = torch.randn(3)
    assert s.scale_model_input(x, 5) is x
    s.set_timesteps(10)
    p.set_timesteps(10)
    assert torch.equal(s.timesteps, p.timesteps) and torch.equal(s.sigmas, p.sigmas)
    assert torch.equal(s.blend_table(3), p.blend_table(3)) and s.index_for_timestep(s.timesteps[4]) == 4
    ts, begin = s.get_timesteps(10, 0.5)
    assert begin == 5 and torch.equal(ts, s.timesteps[5:])


def test_from_pretrained(tmp_path):
    import json
    from audioldm_with_lora_amd.scheduler import UniPCMultistepScheduler
    os.makedirs(tmp_path / "scheduler")
    cfg = {"_class_name": "DDIMScheduler", "num_train_timesteps": 1000, "beta_start": 0.0015, "beta_end": 0.0195,
           "beta_schedule": "scaled_linear", "clip_sample": False, "set_alpha_to_one": False, "steps_offset": 1,
           "prediction_type": "epsilon", "timestep_spacing": "leading"}
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    s = UniPCMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    s.set_timesteps(8)
    assert int(s.timesteps[0]) == 8 * (1000 // 9) + 1
    with pytest.raises(FileNotFoundError):
        UniPCMultistepScheduler.from_pretrained(str(tmp_path), subfolder="nope")


@pytest.mark.parametrize("kw,exc,word", [
    (dict(solver_order=3), NotImplementedError, "solver_order"),
    (dict(thresholding=True), NotImplementedError, "thresholding"),
    (dict(use_karras_sigmas=True), NotImplementedError, "use_karras_sigmas"),
    (dict(use_exponential_sigmas=True), NotImplementedError, "use_exponential_sigmas"),
    (dict(use_beta_sigmas=True), NotImplementedError, "use_beta_sigmas"),
    (dict(rescale_betas_zero_snr=True), NotImplementedError, "rescale_betas_zero_snr"),
    (dict(solver_p=object()), NotImplementedError, "solver_p"),
    (dict(prediction_type="v_prediction"), NotImplementedError, "v_prediction"),
    (dict(prediction_type="sample"), NotImplementedError, "prediction_type"),
    (dict(beta_schedule="linear"), NotImplementedError, "beta_schedule"),
    (dict(beta_schedule="squaredcos_cap_v2"), NotImplementedError, "beta_schedule"),
    (dict(trained_betas=[0.1, 0.2]), NotImplementedError, "trained_betas"),
    (dict(solver_type="bh3"), NotImplementedError, "solver_type"),
    (dict(predict_x0=False), ValueError, "final_sigmas_type"),
    (dict(lower_order_final=False), ValueError, "lower_order_final"),
])
def test_unsupported_options_raise(kw, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        _unipc(**kw)


def test_supported_corner_configurations_construct():
    _unipc(lower_order_final=False, solver_order=1)                        # a first-order row may step to sigma 0
    _unipc(lower_order_final=False, final_sigmas_type="sigma_min")
    _unipc(predict_x0=False, final_sigmas_type="sigma_min")


def test_product_step_has_no_cpu_fallback():
    from audioldm_with_lora_amd._lib import AldmError
    s = _unipc()
    s.set_timesteps(8)
    with pytest.raises(AldmError):
        s.step(torch.zeros(2, 4), s.timesteps[0], torch.zeros(2, 4))
