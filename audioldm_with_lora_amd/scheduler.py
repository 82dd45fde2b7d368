"""DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler, EulerAncestralDiscreteScheduler and RePaintScheduler for the HIP path (host-side integer logic + device step kernels).

Same surface the reference touches: `from_pretrained(id, subfolder="scheduler")`, `.config.num_train_timesteps`,
`.add_noise` [REF script/train/train_audioldm_lora.py:367,503-504] and, through the pipeline,
`set_timesteps / timesteps / step / init_noise_sigma / scale_model_input` [REF script/inference/generate_audio.py:47-52].
Arithmetic spec: SURVEY.md Appendix B.1 (diffusers 0.32.2).  Timestep indices are int64 and computed exactly as
diffusers does ("leading" spacing, steps_offset); the fp32 alpha-bar table uses the same torch ops as diffusers.
DPMSolverMultistepScheduler is diffusers 0.32.2's deterministic multistep solver, swapped in the way diffusers
users do it: `pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`.
UniPCMultistepScheduler is diffusers 0.32.2's multistep predictor-corrector, swapped in the same way: the
sampler for 5-10 steps.
EulerAncestralDiscreteScheduler is diffusers 0.32.2's stochastic sampler, swapped in the same way; its per-step
noise is drawn on the device by the step kernel itself (a Philox stream, ops.philox_state).
RePaintScheduler is RePaint's resampling loop for inpainting, swapped in the same way on the audio-to-audio
pipeline; its two noises per step come from the same kind of stream.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .configs import SCHEDULER


def _read_config(path, subfolder):
    d = os.path.join(path, subfolder) if subfolder else path
    f = os.path.join(d, "scheduler_config.json")
    if not os.path.isfile(f):
        raise FileNotFoundError(f"{f} not found: hub downloads are unavailable, pass a local directory")
    with open(f) as fh:
        return json.load(fh)


def _config_dict(config, over):
    d = dict(config) if isinstance(config, dict) else dict(vars(config))
    d.update(over)
    return d


def strength_begin_index(num_inference_steps, strength):
    """Index of the first step an audio-to-audio / inpainting loop runs at `strength` (diffusers' pipelines' get_timesteps):
    init = min(int(N * strength), N), begin = max(N - init, 0); the loop runs timesteps[begin:].  Host-only."""
    N = int(num_inference_steps)
    if N <= 0:
        raise ValueError(f"num_inference_steps must be positive, got {num_inference_steps}")
    if not 0.0 <= float(strength) <= 1.0:
        raise ValueError(f"The value of strength should be in [0.0, 1.0] but is {strength}")
    init = min(int(N * strength), N)
    if init == 0:
        raise ValueError(f"strength {strength} with {N} inference steps leaves no step to run (int(N * strength) == 0)")
    return max(N - init, 0)


class _SuffixMixin:
    """The audio-to-audio pieces both schedulers share (host-only: no device, no shared library).  After set_timesteps(N):
    `get_timesteps(N, strength)` -> (timesteps[begin:], begin); `blend_table(begin)` -> fp32 [N - begin, 2], row k the
    add_noise_coefficients of schedule index begin + k + 1 and the last row exactly (1, 0) -- diffusers' legacy inpaint loop noises
    the known latents to timesteps[i + 1] after step i and uses them clean after the last step."""

    def get_timesteps(self, num_inference_steps, strength):
        begin = strength_begin_index(num_inference_steps, strength)
        self.set_timesteps(num_inference_steps)
        return self.timesteps[begin:], begin

    def blend_table(self, begin_index=0):
        N = len(self.timesteps)
        if not 0 <= begin_index < N:
            raise ValueError(f"begin_index {begin_index} outside the schedule of {N} steps")
        rows = [torch.stack([torch.as_tensor(v, dtype=torch.float32) for v in self.add_noise_coefficients(i)])
                for i in range(begin_index + 1, N)]
        rows.append(torch.tensor([1.0, 0.0], dtype=torch.float32))
        return torch.stack(rows).float().contiguous()


class DDIMScheduler(_SuffixMixin):
    def __init__(self, **over):
        cfg = dict(SCHEDULER)
        cfg.update({k: v for k, v in over.items() if k in SCHEDULER})
        self.config = SimpleNamespace(**cfg)
        if cfg["beta_schedule"] != "scaled_linear" or cfg["prediction_type"] != "epsilon" or cfg["timestep_spacing"] != "leading":
            raise NotImplementedError("only the AudioLDM scheduler configuration is implemented")
        n = cfg["num_train_timesteps"]
        self.betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg["set_alpha_to_one"] else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, n)[::-1].copy().astype(np.int64))
        self._dev = {}

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **kw):
        return cls(**_read_config(path, subfolder))

    @classmethod
    def from_config(cls, config, **over):
        """dict or SimpleNamespace (e.g. another scheduler's `.config`); keys this class does not know are ignored."""
        return cls(**_config_dict(config, over))

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        n = self.config.num_train_timesteps
        if num_inference_steps > n:
            raise ValueError("num_inference_steps > num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        ratio = n // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
        self.timesteps = torch.from_numpy(ts)
        if device is not None:
            self.timesteps = self.timesteps.to(device)

    def prev_timestep(self, t):
        return int(t) - self.config.num_train_timesteps // self.num_inference_steps

    def step_coefficients(self, t):
        """fp32 {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)} for timestep t (eta = 0)."""
        p = self.prev_timestep(t)
        a_t = self.alphas_cumprod[int(t)]
        a_p = self.alphas_cumprod[p] if p >= 0 else self.final_alpha_cumprod
        return torch.stack([a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5]).float()

    def coefficient_table(self, begin_index=0):
        """rows of timesteps[begin_index:] (a begun DDIM schedule needs no other change: each row depends on its own t only)"""
        return torch.stack([self.step_coefficients(t) for t in self.timesteps.tolist()[begin_index:]])

    def add_noise_coefficients(self, i):
        """fp32 (sqrt(abar[t_i]), sqrt(1 - abar[t_i])): what add_noise applies at schedule index i."""
        a = self.alphas_cumprod[int(self.timesteps[i])]
        return a ** 0.5, (1 - a) ** 0.5

    def step(self, model_output, timestep, sample, eta=0.0, **kw):
        """x_{t-1} from eps (eta = 0) via the fused device kernel; fp32 tensors of any layout."""
        if eta != 0.0:
            raise NotImplementedError("the reference path uses eta = 0")
        dev = sample.device
        coef = self.step_coefficients(timestep).to(dev)
        idx = self._dev.setdefault(("zero", dev), torch.zeros(1, dtype=torch.int32, device=dev))
        x = sample.detach().float().contiguous().clone()
        ops.cfg_ddim_step(model_output.detach().float().contiguous(), x, False, 0.0, coef, idx, None)
        return SimpleNamespace(prev_sample=x.to(sample.dtype))

    def add_noise(self, original_samples, noise, timesteps):
        dev = original_samples.device
        ac = self._dev.get(("ac", dev))
        if ac is None:
            ac = self._dev[("ac", dev)] = self.alphas_cumprod.to(dev, torch.float32).contiguous()
        return ops.add_noise_t(original_samples, noise, ac, timesteps.to(dev, torch.int64).reshape(-1))


# diffusers 0.32.2 DPMSolverMultistepScheduler defaults for the solver keys; the keys it shares with DDIMScheduler default to the
# AudioLDM scheduler configuration, as DDIMScheduler's do here
DPM_CONFIG = dict(
    num_train_timesteps=SCHEDULER["num_train_timesteps"], beta_start=SCHEDULER["beta_start"], beta_end=SCHEDULER["beta_end"],
    beta_schedule=SCHEDULER["beta_schedule"], trained_betas=None, solver_order=2, prediction_type=SCHEDULER["prediction_type"],
    thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint",
    lower_order_final=True, euler_at_final=False, use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False,
    use_lu_lambdas=False, final_sigmas_type="zero", lambda_min_clipped=-float("inf"), variance_type=None,
    timestep_spacing=SCHEDULER["timestep_spacing"], steps_offset=SCHEDULER["steps_offset"], rescale_betas_zero_snr=False,
)


class _SigmaMultistepBase(_SuffixMixin):
    """What DPMSolverMultistepScheduler and UniPCMultistepScheduler share, diffusers-identical between the two: the alpha-bar tables,
    set_timesteps and the sigmas (three spacings, final sigma zero or sigma_min), index_for_timestep, add_noise and the begin index.
    A subclass sets `self.config` and calls `_init_tables(cfg)`, and provides `_reset_solver()` (the multistep state a new schedule
    drops)."""

    def _init_tables(self, cfg):
        n = cfg["num_train_timesteps"]
        self.betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.sigmas = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.linspace(0, n - 1, n, dtype=np.float32)[::-1].copy().astype(np.int64))
        self._step_index = None
        self._reset_solver()
        self._dev = {}

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **kw):
        return cls(**_read_config(path, subfolder))

    @classmethod
    def from_config(cls, config, **over):
        """dict or SimpleNamespace (e.g. DDIMScheduler's `.config`); keys the class does not know (clip_sample, ...) are ignored."""
        return cls(**_config_dict(config, over))

    def scale_model_input(self, sample, *args, **kw):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        cfg = self.config
        n = cfg.num_train_timesteps
        if not 0 < num_inference_steps <= n:
            raise ValueError("need 0 < num_inference_steps <= num_train_timesteps")
        last = n                                      # lambda_min_clipped = -inf clips nothing
        N = num_inference_steps
        if cfg.timestep_spacing == "linspace":
            ts = np.linspace(0, last - 1, N + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif cfg.timestep_spacing == "leading":
            ratio = last // (N + 1)
            ts = (np.arange(0, N + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64)
            ts += cfg.steps_offset
        else:                                         # trailing
            ts = np.arange(last, 0, -n / N).round().copy().astype(np.int64)
            ts -= 1
        sig = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        if cfg.final_sigmas_type == "sigma_min":
            sigma_last = float(((1 - self.alphas_cumprod[0]) / self.alphas_cumprod[0]) ** 0.5)
        else:
            sigma_last = 0.0
        self.sigmas = torch.from_numpy(np.concatenate([sig, [sigma_last]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts).to(dtype=torch.int64)
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self.num_inference_steps = len(ts)
        self._step_index = None
        self._begin_index = None
        self._reset_solver()

    @staticmethod
    def _alpha_sigma(sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha_t, sigma * alpha_t

    def add_noise_coefficients(self, i):
        """fp32 (alpha, sigma) of sigmas[i]: what add_noise applies at schedule index i (diffusers' add_noise after set_begin_index(i))."""
        return self._alpha_sigma(self.sigmas[i])

    def set_begin_index(self, begin_index=0):
        self._begin_index = begin_index

    @property
    def begin_index(self):
        return getattr(self, "_begin_index", None)

    def index_for_timestep(self, timestep):
        """diffusers' index_for_timestep: the second match of `timestep` in the schedule when there are two, else the only one, else
        the last index (a timestep outside the schedule)."""
        cand = (self.timesteps.cpu() == int(timestep)).nonzero()
        if len(cand) == 0:
            return len(self.timesteps) - 1
        return int(cand[1 if len(cand) > 1 else 0])

    def add_noise_indices(self, timesteps):
        """The schedule index add_noise uses for each timestep, in diffusers' order: with no begin index, index_for_timestep(t);
        else, once a step has run, the current step index (add_noise after a step, the inpaint loop); else the begin index (the
        initial latents of img2img).  Host-only."""
        t = torch.as_tensor(timesteps).reshape(-1).cpu()
        if self.begin_index is None:
            return [self.index_for_timestep(tb) for tb in t.tolist()]
        if self._step_index is not None:
            return [self._step_index] * t.numel()
        return [self.begin_index] * t.numel()

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' DPMSolverMultistepScheduler.add_noise (UniPCMultistepScheduler's is the same): alpha_t x + sigma_t noise, with
        (alpha_t, sigma_t) the add_noise_coefficients of add_noise_indices(timesteps) -- one timestep per sample, or one for the whole batch.
        Coefficients on the host, the multiply-add on the device (aldm_add_noise)."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        B = original_samples.shape[0]
        idx = self.add_noise_indices(timesteps)
        if len(idx) == 1:
            idx = idx * B
        if len(idx) != B:
            raise ValueError(f"add_noise: {len(idx)} timesteps for a batch of {B}")
        coef = torch.stack([torch.stack(self.add_noise_coefficients(i)) for i in idx]).float().contiguous()
        return ops.add_noise(original_samples, noise, coef.to(original_samples.device))

    @property
    def step_index(self):
        return self._step_index

    def _init_step_index(self, timestep):
        # diffusers: a schedule begun with set_begin_index starts there, else at the timestep's index
        self._step_index = self.index_for_timestep(timestep) if self.begin_index is None else self.begin_index


class DPMSolverMultistepScheduler(_SigmaMultistepBase):
    """DPM-Solver / DPM-Solver++ (first or second order, deterministic), diffusers 0.32.2 arithmetic restated.

    `coefficient_table()` turns the whole schedule into fp32 rows {alpha_s, sig_s, A, B, C, convert, reads_hist, 0}; the device
    update (aldm_dpm_step_fused) is then  m0 = convert ? (x - sig_s e) / alpha_s : e ;  x' = A x + B m0 + C (m0 - m1),  with m1 the
    previous step's m0 (the history buffer) and 1 / r0 folded into C.  First-order rows have C = 0 and never read the history."""

    def __init__(self, **over):
        cfg = dict(DPM_CONFIG)
        cfg.update({k: v for k, v in over.items() if k in DPM_CONFIG})
        self.config = SimpleNamespace(**cfg)
        self._check(cfg)
        self._init_tables(cfg)

    @staticmethod
    def _check(cfg):
        alg = cfg["algorithm_type"]
        if alg in ("sde-dpmsolver", "sde-dpmsolver++"):
            raise NotImplementedError(f"algorithm_type={alg!r}: the SDE variants draw noise inside every step (not in the captured graph)")
        if alg not in ("dpmsolver++", "dpmsolver"):
            raise NotImplementedError(f"algorithm_type={alg!r}")
        if cfg["solver_order"] not in (1, 2):
            raise NotImplementedError(f"solver_order={cfg['solver_order']}: only first and second order are implemented")
        if cfg["solver_type"] not in ("midpoint", "heun"):
            raise NotImplementedError(f"solver_type={cfg['solver_type']!r}")
        for k in ("thresholding", "use_karras_sigmas", "use_exponential_sigmas", "use_beta_sigmas", "use_lu_lambdas",
                  "rescale_betas_zero_snr"):
            if cfg[k]:
                raise NotImplementedError(f"{k}=True")
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError(f"prediction_type={cfg['prediction_type']!r}: only epsilon prediction is implemented")
        if cfg["beta_schedule"] != "scaled_linear" or cfg["trained_betas"] is not None:
            raise NotImplementedError(f"beta_schedule={cfg['beta_schedule']!r} / trained_betas: only scaled_linear is implemented")
        if cfg["variance_type"] is not None:
            raise NotImplementedError(f"variance_type={cfg['variance_type']!r}")
        if cfg["lambda_min_clipped"] != -float("inf"):
            raise NotImplementedError(f"lambda_min_clipped={cfg['lambda_min_clipped']}")
        if cfg["timestep_spacing"] not in ("leading", "linspace", "trailing"):
            raise NotImplementedError(f"timestep_spacing={cfg['timestep_spacing']!r}")
        if cfg["final_sigmas_type"] not in ("zero", "sigma_min"):
            raise NotImplementedError(f"final_sigmas_type={cfg['final_sigmas_type']!r}")
        if alg == "dpmsolver" and cfg["final_sigmas_type"] == "zero":
            raise ValueError(f"`final_sigmas_type` {cfg['final_sigmas_type']} is not supported for `algorithm_type` {alg}. "
                             "Please choose `sigma_min` instead.")

    def _reset_solver(self):
        self._lower_order_nums = 0
        self._hist = {}

    def row_order(self, i):
        """Solver order of step i of the schedule (diffusers' step(): the first step and, under the final-step rules, the last one
        are first order)."""
        cfg, N = self.config, len(self.timesteps)
        if cfg.solver_order == 1 or i == 0:
            return 1
        if i == N - 1 and (cfg.euler_at_final or (cfg.lower_order_final and N < 15) or cfg.final_sigmas_type == "zero"):
            return 1
        return 2

    def step_coefficients(self, i, order=None):
        """fp32 row {alpha_s, sig_s, A, B, C, convert, reads_hist, 0} of step i, from diffusers' fp32 scalar torch ops."""
        order = self.row_order(i) if order is None else order
        pp = self.config.algorithm_type == "dpmsolver++"
        alpha_t, sigma_t = self._alpha_sigma(self.sigmas[i + 1])
        alpha_s0, sigma_s0 = self._alpha_sigma(self.sigmas[i])
        lambda_t = torch.log(alpha_t) - torch.log(sigma_t)
        lambda_s0 = torch.log(alpha_s0) - torch.log(sigma_s0)
        h = lambda_t - lambda_s0
        if pp:
            A, Bc = sigma_t / sigma_s0, -(alpha_t * (torch.exp(-h) - 1.0))
        else:
            A, Bc = alpha_t / alpha_s0, -(sigma_t * (torch.exp(h) - 1.0))
        Cc = torch.zeros((), dtype=torch.float32)     # exactly 0 on first-order rows (h is +inf on a final sigma-0 row)
        if order == 2:
            alpha_s1, sigma_s1 = self._alpha_sigma(self.sigmas[i - 1])
            lambda_s1 = torch.log(alpha_s1) - torch.log(sigma_s1)
            r0 = (lambda_s0 - lambda_s1) / h
            inv_r0 = 1.0 / r0
            midpoint = self.config.solver_type == "midpoint"
            if pp:
                Cc = (-(0.5 * (alpha_t * (torch.exp(-h) - 1.0))) if midpoint else alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)) * inv_r0
            else:
                Cc = (-(0.5 * (sigma_t * (torch.exp(h) - 1.0))) if midpoint else -(sigma_t * ((torch.exp(h) - 1.0) / h - 1.0))) * inv_r0
        one, zero = torch.ones((), dtype=torch.float32), torch.zeros((), dtype=torch.float32)
        return torch.stack([alpha_s0, sigma_s0, A, Bc, Cc, one if pp else zero, one if order == 2 else zero, zero]).float()

    def coefficient_table(self, begin_index=0):
        """rows of the schedule from step begin_index on.  A begun schedule starts with an empty history (diffusers:
        lower_order_nums = 0), so its first row is first order; the later rows and the final-step rule (judged on the full N) are
        the full schedule's."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        N = len(self.timesteps)
        if not 0 <= begin_index < N:
            raise ValueError(f"begin_index {begin_index} outside the schedule of {N} steps")
        return torch.stack([self.step_coefficients(i, 1 if i == begin_index else None) for i in range(begin_index, N)])

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, **kw):
        """x at the next timestep from eps via the device kernel (aldm_dpm_step_fused, eager mode); fp32 tensors of any layout.
        The previous step's converted output stays on the device, one history tensor per sample shape."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        dev = sample.device
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        order = self.row_order(i) if self._lower_order_nums >= 1 else 1
        x = sample.detach().float().contiguous().clone()
        key = (tuple(x.shape), dev)
        hist = self._hist.get(key)
        if hist is None:
            if order == 2:
                raise ValueError(f"step(): no previous model output for a sample of shape {tuple(x.shape)}")
            hist = self._hist[key] = torch.empty_like(x)
        coef = self.step_coefficients(i, order).view(1, 8).to(dev)
        idx = self._dev.setdefault(("zero", dev), torch.zeros(1, dtype=torch.int32, device=dev))
        ops.dpm_step_fused(model_output.detach().float().contiguous(), x, False, 0.0, coef, idx, None, hist)
        if self._lower_order_nums < self.config.solver_order:
            self._lower_order_nums += 1
        self._step_index += 1
        prev = x.to(sample.dtype)
        if not return_dict:
            return (prev,)
        return SimpleNamespace(prev_sample=prev)


# diffusers 0.32.2 UniPCMultistepScheduler defaults for the solver keys; the keys it shares with DDIMScheduler default to the AudioLDM
# scheduler configuration, as the other classes' do here
UNIPC_CONFIG = dict(
    num_train_timesteps=SCHEDULER["num_train_timesteps"], beta_start=SCHEDULER["beta_start"], beta_end=SCHEDULER["beta_end"],
    beta_schedule=SCHEDULER["beta_schedule"], trained_betas=None, solver_order=2, prediction_type=SCHEDULER["prediction_type"],
    thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0, predict_x0=True, solver_type="bh2",
    lower_order_final=True, disable_corrector=[], solver_p=None, use_karras_sigmas=False, use_exponential_sigmas=False,
    use_beta_sigmas=False, timestep_spacing=SCHEDULER["timestep_spacing"], steps_offset=SCHEDULER["steps_offset"],
    final_sigmas_type="zero", rescale_betas_zero_snr=False,
)
UNIPC_ROW = 16


class UniPCMultistepScheduler(_SigmaMultistepBase):
    """UniPC (a multistep predictor plus a corrector that reuses the next step's model output; orders 1 and 2, bh1 / bh2), diffusers
    0.32.2 arithmetic for epsilon prediction restated.  The sampler for 5-10 steps; at 20 and more it is within
    a factor of about 1.5 of DPM-Solver++ 2M either way.

    `coefficient_table()` turns the whole schedule into fp32 rows of UNIPC_ROW floats
        {alpha_s, sig_s, Ac, Bc, Cc, Dc, Ap, Bp, Cp, convert, corr, corr_reads_m1, pred_reads_m0, 0, 0, 0}
    and the device update (aldm_unipc_step_fused) is then
        m_t = convert ? (x - sig_s e) / alpha_s : e
        xc  = corr ? Ac last + Bc m0 + Cc (m1 - m0) + Dc (m_t - m0) : x
        x'  = Ap xc + Bp m_t + Cp (m_t - m0)
    with m0, m1 the previous two converted outputs and `last` the previous step's corrected sample; 1 / rk, rhos, B_h and h_phi_1 are
    folded into the six coefficients.  The predictor's difference is written (m_t - m0), new minus old as in the DPM class's row, so
    that with the corrector off {Ap, Bp, Cp} IS DPM-Solver++ 2M midpoint's {A, B, C}; diffusers writes -(Cp) (m0 - m_t).  As in
    diffusers, m_t converts the UNCORRECTED sample, the corrector starts from `last` (not from the sample passed in), its result is
    what the predictor starts from and what becomes the new `last`, and the output list receives m_t after the corrector read it."""

    def __init__(self, **over):
        cfg = dict(UNIPC_CONFIG)
        cfg.update({k: v for k, v in over.items() if k in UNIPC_CONFIG})
        cfg["disable_corrector"] = [int(v) for v in (cfg["disable_corrector"] or [])]
        if cfg["solver_type"] in ("midpoint", "heun", "logrho"):      # diffusers: another solver's type (a DPM config) becomes bh2
            cfg["solver_type"] = "bh2"
        self.config = SimpleNamespace(**cfg)
        self._check(cfg)
        self._init_tables(cfg)

    @staticmethod
    def _check(cfg):
        if cfg["solver_order"] not in (1, 2):
            raise NotImplementedError(f"solver_order={cfg['solver_order']}: only first and second order are implemented")
        if cfg["solver_type"] not in ("bh1", "bh2"):
            raise NotImplementedError(f"solver_type={cfg['solver_type']!r}")
        for k in ("thresholding", "use_karras_sigmas", "use_exponential_sigmas", "use_beta_sigmas", "rescale_betas_zero_snr"):
            if cfg[k]:
                raise NotImplementedError(f"{k}=True")
        if cfg["solver_p"] is not None:
            raise NotImplementedError("solver_p: another scheduler as the predictor is not implemented")
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError(f"prediction_type={cfg['prediction_type']!r}: only epsilon prediction is implemented")
        if cfg["beta_schedule"] != "scaled_linear" or cfg["trained_betas"] is not None:
            raise NotImplementedError(f"beta_schedule={cfg['beta_schedule']!r} / trained_betas: only scaled_linear is implemented")
        if cfg["timestep_spacing"] not in ("leading", "linspace", "trailing"):
            raise NotImplementedError(f"timestep_spacing={cfg['timestep_spacing']!r}")
        if cfg["final_sigmas_type"] not in ("zero", "sigma_min"):
            raise NotImplementedError(f"final_sigmas_type={cfg['final_sigmas_type']!r}")
        if cfg["final_sigmas_type"] == "zero":
            if not cfg["predict_x0"]:
                raise ValueError("`final_sigmas_type` zero is not supported for `predict_x0` False (the noise-prediction update of the "
                                 "step to sigma 0 is 0 * inf). Please choose `sigma_min` instead.")
            if cfg["solver_order"] == 2 and not cfg["lower_order_final"]:
                raise ValueError("`lower_order_final` False with `solver_order` 2 and `final_sigmas_type` zero makes the step to sigma 0 "
                                 "second order, which divides by rk = -0. Set `lower_order_final` or choose `sigma_min`.")

    def _reset_solver(self):
        self._lower_order_nums = 0
        self._this_order = 0          # the predictor order of the step before (the corrector's order)
        self._state = {}              # (shape, device) -> [state fp32 [3, *shape], steps taken]

    def row_order(self, i, begin_index=0):
        """Predictor order of step i of a schedule begun at begin_index: min(solver_order, N - i) under lower_order_final (judged on
        the full N), capped by the warm-up (lower_order_nums + 1 = i - begin_index + 1).  The corrector of step i uses
        row_order(i - 1)."""
        cfg, N = self.config, len(self.timesteps)
        order = min(cfg.solver_order, N - i) if cfg.lower_order_final else cfg.solver_order
        return min(order, i - begin_index + 1)

    def uses_corrector(self, i, begin_index=0):
        """whether step i corrects the sample it is given: not on the first step of the loop (no previous sample), and not where
        disable_corrector names the step before"""
        return i > begin_index and (i - 1) not in self.config.disable_corrector

    def _lambda(self, i):
        alpha, sigma = self._alpha_sigma(self.sigmas[i])
        return alpha, sigma, torch.log(alpha) - torch.log(sigma)

    def _bh(self, h):
        """(h_phi_1, B_h, hh) of a step of log-SNR length h"""
        hh = -h if self.config.predict_x0 else h
        h_phi_1 = torch.expm1(hh)
        return h_phi_1, (hh if self.config.solver_type == "bh1" else torch.expm1(hh)), hh

    def step_coefficients(self, i, order=None, corrector_order=None):
        """fp32 row of step i, from diffusers' fp32 scalar torch ops.  order: the predictor's (default row_order(i));
        corrector_order: 0 for none, else 1 or 2 (default: row_order(i - 1) where uses_corrector(i))."""
        order = self.row_order(i) if order is None else order
        if corrector_order is None:
            corrector_order = self.row_order(i - 1) if self.uses_corrector(i) else 0
        x0 = self.config.predict_x0
        zero, one = torch.zeros((), dtype=torch.float32), torch.ones((), dtype=torch.float32)
        alpha_s0, sigma_s0, lambda_s0 = self._lambda(i)
        # ---- predictor: from sigmas[i] to sigmas[i + 1] ----
        alpha_t, sigma_t, lambda_t = self._lambda(i + 1)
        if float(self.sigmas[i + 1]) == 0.0:          # x' = m_t exactly (h = +inf: h_phi_1 = -1, alpha_t = 1); order 1 by _check
            Ap, Bp, Cp = zero, one, zero
        else:
            h = lambda_t - lambda_s0
            h_phi_1, B_h, _ = self._bh(h)
            scale = alpha_t if x0 else sigma_t
            Ap = sigma_t / sigma_s0 if x0 else alpha_t / alpha_s0
            Bp = -(scale * h_phi_1)
            Cp = zero
            if order == 2:
                rk = (self._lambda(i - 1)[2] - lambda_s0) / h
                Cp = scale * B_h * 0.5 / rk           # rhos_p = 0.5; -(.) (m0 - m_t) / rk written as (.) (m_t - m0)
        # ---- corrector: redoes the step from sigmas[i - 1] to sigmas[i] with this step's model output ----
        Ac = Bc = Cc = Dc = zero
        if corrector_order:
            alpha_p, sigma_p, lambda_p = self._lambda(i - 1)
            h = lambda_s0 - lambda_p
            h_phi_1, B_h, hh = self._bh(h)
            scale = alpha_s0 if x0 else sigma_s0
            Ac = sigma_s0 / sigma_p if x0 else alpha_s0 / alpha_p
            Bc = -(scale * h_phi_1)
            if corrector_order == 1:
                Dc = -(scale * B_h * 0.5)             # rhos_c = [0.5]
            else:
                rk = (self._lambda(i - 2)[2] - lambda_p) / h
                rks = torch.stack([rk, one])
                h_phi_k = h_phi_1 / hh - 1
                b1 = h_phi_k / B_h
                b2 = (h_phi_k / hh - 1 / 2) * 2 / B_h
                rhos_c = torch.linalg.solve(torch.stack([torch.pow(rks, 0), torch.pow(rks, 1)]), torch.stack([b1, b2]))
                Cc = -(scale * B_h * rhos_c[0] / rk)
                Dc = -(scale * B_h * rhos_c[1])
        flags = [one if x0 else zero, one if corrector_order else zero, one if corrector_order == 2 else zero, one if order == 2 else zero]
        return torch.stack([alpha_s0, sigma_s0, Ac, Bc, Cc, Dc, Ap, Bp, Cp, *flags, zero, zero, zero]).float()

    def coefficient_table(self, begin_index=0):
        """rows of the schedule from step begin_index on.  A begun schedule starts with an empty history (diffusers: lower_order_nums
        = 0, last_sample = None), so its first row has no corrector and a first-order predictor; the final-step rule is judged on the
        full N."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        N = len(self.timesteps)
        if not 0 <= begin_index < N:
            raise ValueError(f"begin_index {begin_index} outside the schedule of {N} steps")
        rows = []
        for i in range(begin_index, N):
            corr = self.row_order(i - 1, begin_index) if self.uses_corrector(i, begin_index) else 0
            rows.append(self.step_coefficients(i, self.row_order(i, begin_index), corr))
        return torch.stack(rows)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, **kw):
        """x at the next timestep from eps via the device kernel (aldm_unipc_step_fused, eager mode); fp32 tensors of any layout.
        The last corrected sample and the previous two converted outputs stay on the device, one state tensor per sample shape;
        the kernel's ring turns on the parity of the counter it is given, which alternates here between two one-word tensors."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        dev = sample.device
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        x = sample.detach().float().contiguous().clone()
        e = model_output.detach().float().contiguous()
        ops._require_gpu(x)
        key = (tuple(x.shape), dev)
        st = self._state.get(key)
        corr = self._this_order if (i > 0 and (i - 1) not in self.config.disable_corrector and st is not None) else 0
        cfg, N = self.config, len(self.timesteps)
        order = min(cfg.solver_order, N - i) if cfg.lower_order_final else cfg.solver_order
        order = min(order, self._lower_order_nums + 1)
        if st is None:
            if order == 2:
                raise ValueError(f"step(): no previous model output for a sample of shape {tuple(x.shape)}")
            st = self._state[key] = [torch.zeros((3, *x.shape), dtype=torch.float32, device=dev), 0]
        if st[1] < max(order - 1, corr):
            raise ValueError(f"step(): {st[1]} previous model outputs for a sample of shape {tuple(x.shape)}, the step needs more")
        row = self.step_coefficients(i, order, corr).to(dev)
        coef = torch.stack([row, row])
        idx = self._dev.get(("parity", dev))
        if idx is None:
            idx = self._dev[("parity", dev)] = [torch.full((1,), v, dtype=torch.int32, device=dev) for v in (0, 1)]
        ops.unipc_step_fused(e, x, False, 0.0, coef, idx[st[1] & 1], None, st[0])
        st[1] += 1
        self._this_order = order
        if self._lower_order_nums < cfg.solver_order:
            self._lower_order_nums += 1
        self._step_index += 1
        prev = x.to(sample.dtype)
        if not return_dict:
            return (prev,)
        return SimpleNamespace(prev_sample=prev)


# diffusers 0.32.2 EulerAncestralDiscreteScheduler defaults; the keys it shares with DDIMScheduler default to the AudioLDM scheduler
# configuration, as the other classes' do here
EULER_A_CONFIG = dict(
    num_train_timesteps=SCHEDULER["num_train_timesteps"], beta_start=SCHEDULER["beta_start"], beta_end=SCHEDULER["beta_end"],
    beta_schedule=SCHEDULER["beta_schedule"], trained_betas=None, prediction_type=SCHEDULER["prediction_type"],
    timestep_spacing=SCHEDULER["timestep_spacing"], steps_offset=SCHEDULER["steps_offset"], rescale_betas_zero_snr=False,
    use_karras_sigmas=False,
)


def _fresh_seed():
    """a 63-bit seed from torch's global CPU generator: fresh on every call, reproducible after torch.manual_seed"""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))


class EulerAncestralDiscreteScheduler(_SuffixMixin):
    """Ancestral sampling with Euler steps, diffusers 0.32.2 arithmetic for epsilon prediction restated.

    Sigma space: sigma = sqrt((1 - abar) / abar); the sample x is UNSCALED (it starts at init_noise_sigma * noise) and the UNet sees
    scale_model_input(x) = x / sqrt(sigma^2 + 1).  Step i, from s_from = sigmas[i] to s_to = sigmas[i + 1]:
        sigma_up = sqrt(s_to^2 (s_from^2 - s_to^2) / s_from^2) ;  sigma_down = sqrt(s_to^2 - sigma_up^2)
        x' = x + e (sigma_down - s_from) + sigma_up z ,  z ~ N(0, I)
    `coefficient_table()` turns the schedule into fp32 rows {dt, sigma_up, in_scale_next, sigma_down} with dt = sigma_down - s_from and
    in_scale_next = 1 / sqrt(s_to^2 + 1) (exactly 1 on the last row, where s_to = sigma_up = sigma_down = 0 and x' = x - s_from e).  The
    device update (aldm_euler_a_step_fused) draws z itself from a Philox stream whose state lives in device memory, so the step
    replays inside a captured graph.  The noise stream is this library's own (not torch's and not diffusers'): a seed reproduces this
    library's samples, not another implementation's."""

    def __init__(self, **over):
        cfg = dict(EULER_A_CONFIG)
        cfg.update({k: v for k, v in over.items() if k in EULER_A_CONFIG})
        self.config = SimpleNamespace(**cfg)
        self._check(cfg)
        n = cfg["num_train_timesteps"]
        self.betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        sig = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        self.sigmas = torch.from_numpy(np.concatenate([sig[::-1], [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(np.linspace(0, n - 1, n, dtype=np.float32)[::-1].copy())
        self.num_inference_steps = None
        self._step_index = None
        self._begin_index = None
        self._rng = {}
        self._dev = {}

    @staticmethod
    def _check(cfg):
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError(f"prediction_type={cfg['prediction_type']!r}: only epsilon prediction is implemented")
        if cfg["beta_schedule"] != "scaled_linear" or cfg["trained_betas"] is not None:
            raise NotImplementedError(f"beta_schedule={cfg['beta_schedule']!r} / trained_betas: only scaled_linear is implemented")
        for k in ("rescale_betas_zero_snr", "use_karras_sigmas"):
            if cfg[k]:
                raise NotImplementedError(f"{k}=True")
        if cfg["timestep_spacing"] not in ("leading", "linspace", "trailing"):
            raise NotImplementedError(f"timestep_spacing={cfg['timestep_spacing']!r}")

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **kw):
        return cls(**_read_config(path, subfolder))

    @classmethod
    def from_config(cls, config, **over):
        """dict or SimpleNamespace (e.g. DDIMScheduler's or DPMSolverMultistepScheduler's `.config`); keys this class does not know
        (clip_sample, solver_order, ...) are ignored."""
        return cls(**_config_dict(config, over))

    @property
    def init_noise_sigma(self):
        m = self.sigmas.max()
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return float(m)
        return float((m ** 2 + 1) ** 0.5)

    def set_timesteps(self, num_inference_steps, device=None):
        cfg = self.config
        n, N = cfg.num_train_timesteps, int(num_inference_steps)
        if not 0 < N <= n:
            raise ValueError("need 0 < num_inference_steps <= num_train_timesteps")
        if cfg.timestep_spacing == "linspace":
            ts = np.linspace(0, n - 1, N, dtype=np.float32)[::-1].copy()
        elif cfg.timestep_spacing == "leading":
            ratio = n // N
            ts = (np.arange(0, N) * ratio).round()[::-1].copy().astype(np.float32)
            ts += cfg.steps_offset
        else:                                         # trailing
            ts = np.arange(n, 0, -n / N).round().copy().astype(np.float32)
            ts -= 1
        sig = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts)
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self.num_inference_steps = N
        self._step_index = None
        self._begin_index = None
        self._rng = {}

    def _need_schedule(self):
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")

    def input_scale(self, i):
        """fp32 1 / sqrt(sigmas[i]^2 + 1): what scale_model_input multiplies by at schedule index i (exactly 1 where sigma is 0)"""
        return 1.0 / ((self.sigmas[i] ** 2 + 1) ** 0.5)

    def step_coefficients(self, i):
        """fp32 row {dt, sigma_up, in_scale_next, sigma_down} of step i, from diffusers' fp32 scalar torch ops."""
        s_from, s_to = self.sigmas[i], self.sigmas[i + 1]
        sigma_up = (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5
        sigma_down = (s_to ** 2 - sigma_up ** 2) ** 0.5
        return torch.stack([sigma_down - s_from, sigma_up, self.input_scale(i + 1), sigma_down]).float()

    def coefficient_table(self, begin_index=0):
        """rows of the schedule from step begin_index on (each row depends on its own pair of sigmas only)"""
        self._need_schedule()
        N = len(self.timesteps)
        if not 0 <= begin_index < N:
            raise ValueError(f"begin_index {begin_index} outside the schedule of {N} steps")
        return torch.stack([self.step_coefficients(i) for i in range(begin_index, N)])

    def add_noise_coefficients(self, i):
        """fp32 (1, sigmas[i]): what add_noise applies at schedule index i (sigma space: x0 + sigma noise)."""
        return torch.ones((), dtype=torch.float32), self.sigmas[i]

    def set_begin_index(self, begin_index=0):
        self._begin_index = begin_index

    @property
    def begin_index(self):
        return self._begin_index

    @property
    def step_index(self):
        return self._step_index

    def index_for_timestep(self, timestep):
        """diffusers' index_for_timestep: the second match of `timestep` in the schedule when there are two, else the first one."""
        cand = (self.timesteps.cpu() == float(timestep)).nonzero()
        if len(cand) == 0:
            raise ValueError(f"timestep {float(timestep)} is not in the schedule")
        return int(cand[1 if len(cand) > 1 else 0])

    def _init_step_index(self, timestep):
        self._step_index = self.index_for_timestep(timestep) if self.begin_index is None else self.begin_index

    def scale_model_input(self, sample, timestep):
        """sample / sqrt(sigma^2 + 1) at the current step (the step index is found from `timestep` on the first call)."""
        self._need_schedule()
        if self._step_index is None:
            self._init_step_index(timestep)
        return sample * self.input_scale(self._step_index).to(sample.device)

    def _state_for(self, generator, dev):
        """The Philox state a step draws from.  A device int32 [4] tensor (ops.philox_state) is used as it is and advanced in place.
        An int seed, or a torch.Generator -- of which ONLY initial_seed() is read: its own stream is neither used nor advanced --
        names a stream that this scheduler keeps per (seed, device) from its draw 0 on, until the next set_timesteps().  None: one
        stream per device with a fresh seed (_fresh_seed), likewise kept until set_timesteps()."""
        if torch.is_tensor(generator):
            return generator
        if generator is None:
            key = (None, dev)
            if key not in self._rng:
                self._rng[key] = ops.philox_state(_fresh_seed(), 0, dev)
            return self._rng[key]
        seed = generator.initial_seed() if isinstance(generator, torch.Generator) else int(generator)
        key = (seed, dev)
        if key not in self._rng:
            self._rng[key] = ops.philox_state(seed, 0, dev)
        return self._rng[key]

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, **kw):
        """x at the next sigma from eps via the device kernel (aldm_euler_a_step_fused, eager mode); fp32 tensors of any layout.  The
        noise is drawn inside the kernel from the Philox stream `generator` names (see _state_for), whose draw ordinal grows by 1."""
        self._need_schedule()
        dev = sample.device
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        x = sample.detach().float().contiguous().clone()
        state = self._state_for(generator, dev)
        # a one-row schedule for the kernel: its counter wraps 0 -> 0, and its ticket advances the draw ordinal
        coef = self.step_coefficients(i).view(1, 4).to(dev)
        idx = self._dev.setdefault(("zero", dev), torch.zeros(1, dtype=torch.int32, device=dev))
        ticket = self._dev.setdefault(("ticket", dev), torch.zeros(1, dtype=torch.int32, device=dev))
        t1 = self._dev.setdefault(("t1", dev), torch.zeros(1, dtype=torch.float32, device=dev))
        t_out = self._dev.setdefault(("t_out", dev), torch.zeros(1, dtype=torch.float32, device=dev))
        ops.euler_a_step_fused(model_output.detach().float().contiguous(), x, False, 0.0, coef, idx, None, state, None, None, t1, t_out, ticket)
        self._step_index += 1
        prev = x.to(sample.dtype)
        if not return_dict:
            return (prev,)
        return SimpleNamespace(prev_sample=prev)

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' EulerAncestralDiscreteScheduler.add_noise: x + sigma noise, sigma by schedule index -- index_for_timestep(t) with
        no begin index, else the current step index once a step has run, else the begin index.  The multiply-add runs on the device."""
        self._need_schedule()
        B = original_samples.shape[0]
        t = torch.as_tensor(timesteps).reshape(-1).cpu()
        if self.begin_index is None:
            idx = [self.index_for_timestep(tb) for tb in t.tolist()]
        elif self._step_index is not None:
            idx = [self._step_index] * t.numel()
        else:
            idx = [self.begin_index] * t.numel()
        if len(idx) == 1:
            idx = idx * B
        if len(idx) != B:
            raise ValueError(f"add_noise: {len(idx)} timesteps for a batch of {B}")
        coef = torch.stack([torch.stack(self.add_noise_coefficients(i)) for i in idx]).float().contiguous()
        return ops.add_noise(original_samples, noise, coef.to(original_samples.device))


# diffusers 0.32.2 RePaintScheduler's own keys (jump_length and jump_n_sample are arguments of its set_timesteps; here they are
# configuration, so that a pipeline's engine cache is keyed by them); the keys shared with DDIMScheduler default to the AudioLDM
# scheduler configuration, as the other classes' do here
REPAINT_CONFIG = dict(SCHEDULER, trained_betas=None, jump_length=10, jump_n_sample=10, eta=0.0)


class RePaintScheduler(_SuffixMixin):
    """RePaint resampling for inpainting (Lugmayr et al., CVPR 2022, Algorithm 1; diffusers 0.32.2 RePaintScheduler / RePaintPipeline)
    on DDIMScheduler's grid, eta = 0.

    THE MASK MEANS 1 = REGENERATE, 0 = KEEP, as everywhere in this library.  diffusers' RePaint uses the opposite (1 = keep).

    set_timesteps(N) builds diffusers' walk over the grid levels N - 1 .. 0: it falls one level per UNet call and, `jump_n_sample - 1`
    times at every level that is a multiple of `jump_length` below N - jump_length, climbs `jump_length` levels back up.  Level l is
    DDIM's timestep l * (T // N) + steps_offset.  The walk is FOLDED: every falling (or first) entry is one UNet call, and the run of J
    rising entries behind it is that call's jump.  `timesteps` lists the UNet calls; `coefficient_table()` has one fp32 row
        {sa, sb, sap, sbp, c1, c2, 0, 0}
    per call: DDIMScheduler.step_coefficients of its timestep, then the jump over J levels from level l - 1, where the step lands, as
    ONE Gaussian:  r = abar(l - 1 + J) / abar(l - 1),  c1 = sqrt(r),  c2 = sqrt(1 - r)  (abar(-1) = final_alpha_cumprod; exactly (1, 0)
    where J == 0).  diffusers applies J * (T // N) single-beta `undo_step`s, each with noise of its own; their composition is one
    Gaussian too, so no launch without a UNet call is needed.  The device step (aldm_repaint_step_fused_masked) is then
        xu = DDIM's update ;  xb = (1 - m) (a x0 + s zk) + m xu ;  x' = c1 xb + c2 zj
    with (a, s) the row of blend_table() and zk, zj two FRESH normals per element from a Philox stream in device memory (draws d and
    d + 1; the ordinal moves by 2 per step).  The noise stream is this library's own: a seed reproduces this library's samples."""

    def __init__(self, **over):
        cfg = dict(REPAINT_CONFIG)
        cfg.update({k: v for k, v in over.items() if k in REPAINT_CONFIG})
        self.config = SimpleNamespace(**cfg)
        self._check(cfg)
        n = cfg["num_train_timesteps"]
        self.betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg["set_alpha_to_one"] else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.walk, self.folded = [], []
        self.timesteps = torch.from_numpy(np.arange(0, n)[::-1].copy().astype(np.int64))
        self._rng = {}
        self._dev = {}

    @staticmethod
    def _check(cfg):
        if cfg["eta"] != 0:
            raise NotImplementedError(f"eta={cfg['eta']}: only the deterministic reverse step (eta = 0) is implemented")
        if cfg["clip_sample"]:
            raise NotImplementedError("clip_sample=True")
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError(f"prediction_type={cfg['prediction_type']!r}: only epsilon prediction is implemented")
        if cfg["beta_schedule"] != "scaled_linear" or cfg["trained_betas"] is not None:
            raise NotImplementedError(f"beta_schedule={cfg['beta_schedule']!r} / trained_betas: only scaled_linear is implemented")
        if cfg["timestep_spacing"] != "leading":
            raise NotImplementedError(f"timestep_spacing={cfg['timestep_spacing']!r}: only DDIMScheduler's leading grid is implemented")
        RePaintScheduler._check_jumps(cfg["jump_length"], cfg["jump_n_sample"])

    @staticmethod
    def _check_jumps(jump_length, jump_n_sample):
        if int(jump_length) != jump_length or jump_length < 1:
            raise ValueError(f"jump_length must be an integer >= 1, got {jump_length}")
        if int(jump_n_sample) != jump_n_sample or jump_n_sample < 1:
            raise ValueError(f"jump_n_sample must be an integer >= 1, got {jump_n_sample}")

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **kw):
        return cls(**_read_config(path, subfolder))

    @classmethod
    def from_config(cls, config, **over):
        """dict or SimpleNamespace (e.g. DDIMScheduler's `.config`), then overrides such as jump_length=5, jump_n_sample=3; keys this
        class does not know (solver_order, ...) are ignored."""
        return cls(**_config_dict(config, over))

    def scale_model_input(self, sample, timestep=None):
        return sample

    @staticmethod
    def walk_levels(N, jump_length, jump_n_sample):
        """diffusers' RePaintScheduler.set_timesteps list, in grid levels"""
        jumps = {j: jump_n_sample - 1 for j in range(0, N - jump_length, jump_length)}
        walk, t = [], N
        while t >= 1:
            t -= 1
            walk.append(t)
            if jumps.get(t, 0) > 0:
                jumps[t] -= 1
                for _ in range(jump_length):
                    t += 1
                    walk.append(t)
        return walk

    @staticmethod
    def fold(walk):
        """[(level, J)]: the falling (or first) entries of a walk, each with the number of rising entries behind it"""
        folded = []
        for i, l in enumerate(walk):
            if i == 0 or l < walk[i - 1]:
                folded.append([l, 0])
            else:
                folded[-1][1] += 1
        return [tuple(f) for f in folded]

    def set_timesteps(self, num_inference_steps, jump_length=None, jump_n_sample=None, device=None):
        """jump_length / jump_n_sample None: the configuration's.  timesteps: int64, one per UNet call."""
        n, N = self.config.num_train_timesteps, int(num_inference_steps)
        if not 0 < N <= n:
            raise ValueError("need 0 < num_inference_steps <= num_train_timesteps")
        jl = self.config.jump_length if jump_length is None else jump_length
        js = self.config.jump_n_sample if jump_n_sample is None else jump_n_sample
        self._check_jumps(jl, js)
        self.num_inference_steps = N
        self.walk = self.walk_levels(N, int(jl), int(js))
        self.folded = self.fold(self.walk)
        ts = np.array([l for l, _ in self.folded], dtype=np.int64) * (n // N) + self.config.steps_offset
        self.timesteps = torch.from_numpy(ts)
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self._rng = {}

    def _need_schedule(self):
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")

    def get_timesteps(self, num_inference_steps, strength):
        if float(strength) != 1.0:
            raise ValueError(f"strength {strength}: RePaint regenerates the masked region from noise, only strength 1.0 is accepted")
        self.set_timesteps(num_inference_steps)
        return self.timesteps, 0

    def prev_timestep(self, t):
        return int(t) - self.config.num_train_timesteps // self.num_inference_steps

    def _abar(self, t):
        """fp32 alpha-bar at timestep t; final_alpha_cumprod below the grid (the level -1 a step from level 0 lands on)"""
        return self.alphas_cumprod[int(t)] if t >= 0 else self.final_alpha_cumprod

    def _level_timestep(self, level):
        return level * (self.config.num_train_timesteps // self.num_inference_steps) + self.config.steps_offset if level >= 0 else -1

    def step_coefficients(self, t):
        """DDIMScheduler.step_coefficients, the same fp32 ops"""
        a_t, a_p = self.alphas_cumprod[int(t)], self._abar(self.prev_timestep(t))
        return torch.stack([a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5]).float()

    def jump_coefficients(self, t_from, t_to):
        """fp32 (c1, c2) of the forward jump from timestep t_from up to t_to as one Gaussian: r = abar(t_to) / abar(t_from) in float64
        on the fp32 table (1 - r cancels in fp32), rounded once"""
        r = self._abar(t_to).double() / self._abar(t_from).double()
        return torch.stack([r ** 0.5, (1 - r) ** 0.5]).float()

    def coefficient_table(self, begin_index=0):
        self._need_schedule()
        if begin_index:
            raise NotImplementedError("begin_index > 0: RePaint runs its whole walk (strength 1.0)")
        rows = []
        for l, J in self.folded:
            jump = self.jump_coefficients(self._level_timestep(l - 1), self._level_timestep(l - 1 + J)) if J else torch.tensor([1.0, 0.0])
            rows.append(torch.cat([self.step_coefficients(self._level_timestep(l)), jump, torch.zeros(2)]))
        return torch.stack(rows).float().contiguous()

    def blend_table(self, begin_index=0):
        """fp32 [L, 2]: row k noises the known latents to the level call k's step lands on, (sqrt(abar), sqrt(1 - abar)) of level
        l_k - 1 (before the jump; final_alpha_cumprod at level -1); the last row is exactly (1, 0)"""
        self._need_schedule()
        if begin_index:
            raise NotImplementedError("begin_index > 0: RePaint runs its whole walk (strength 1.0)")
        rows = []
        for l, _ in self.folded[:-1]:
            a = self._abar(self._level_timestep(l - 1))
            rows.append(torch.stack([a ** 0.5, (1 - a) ** 0.5]))
        rows.append(torch.tensor([1.0, 0.0], dtype=torch.float32))
        return torch.stack(rows).float().contiguous()

    def add_noise_coefficients(self, i):
        """fp32 (sqrt(abar[t_i]), sqrt(1 - abar[t_i])) of UNet call i of the folded list"""
        a = self.alphas_cumprod[int(self.timesteps[i])]
        return a ** 0.5, (1 - a) ** 0.5

    def add_noise(self, original_samples, noise, timesteps):
        dev = original_samples.device
        ac = self._dev.get(("ac", dev))
        if ac is None:
            ac = self._dev[("ac", dev)] = self.alphas_cumprod.to(dev, torch.float32).contiguous()
        return ops.add_noise_t(original_samples, noise, ac, timesteps.to(dev, torch.int64).reshape(-1))

    _state_for = EulerAncestralDiscreteScheduler._state_for

    def _scratch(self, dev):
        """the one-row schedule an eager launch runs on: counter, ticket, its timestep list and t_out"""
        s = self._dev.get(("scratch", dev))
        if s is None:
            s = self._dev[("scratch", dev)] = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                                               torch.zeros(1, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev))
        return s

    def step(self, model_output, timestep, sample, original_image, mask, generator=None, return_dict=True, **kw):
        """One row WITHOUT a jump through the device kernel (aldm_repaint_step_fused_masked, eager): the DDIM update from `timestep`,
        then the known part a x0 + s zk (a, s of the timestep the update lands on; final_alpha_cumprod below the grid) where the mask
        keeps it.  mask: 1 = REGENERATE, 0 = keep (the opposite of diffusers' RePaintScheduler.step), anything that broadcasts to the
        sample; fp32 tensors of any layout.  zk is drawn inside the kernel from the Philox stream `generator` names -- an int seed, a
        torch.Generator (only its initial_seed() is read) or an ops.philox_state -- whose draw ordinal grows by 2."""
        self._need_schedule()
        dev = sample.device
        x = sample.detach().float().contiguous().clone()
        ops._require_gpu(x)
        B = x.shape[0]
        a = self._abar(self.prev_timestep(timestep))
        coef = torch.cat([self.step_coefficients(timestep), torch.tensor([1.0, 0.0, 0.0, 0.0])]).view(1, 8).to(dev)
        blend = torch.stack([a ** 0.5, (1 - a) ** 0.5]).float().view(1, 2).to(dev)
        m = torch.as_tensor(mask).to(dev, torch.float32).expand_as(x).reshape(B, -1).contiguous()
        x0 = original_image.detach().to(dev, torch.float32).expand_as(x).reshape(B, -1, 1).contiguous()
        idx, ticket, t1, t_out = self._scratch(dev)
        # (every element its own pixel: one channel, so the mask may vary along any axis of the sample's layout)
        ops.repaint_step_fused_masked(model_output.detach().float().contiguous(), x.view(B, -1, 1), False, 0.0, coef, idx, None,
                                      self._state_for(generator, dev), None, None, t1, t_out, ticket, x0, None, m, blend)
        prev = x.to(sample.dtype)
        if not return_dict:
            return (prev,)
        return SimpleNamespace(prev_sample=prev)

    def undo_step(self, sample, timestep, generator=None):
        """The closed-form jump up ONE grid level, from `timestep` to timestep + T // N: sqrt(r) x + sqrt(1 - r) z with
        r = abar(timestep + T // N) / abar(timestep); diffusers' undo_step composes T // N single-beta steps instead.  z is one draw
        of the Philox stream `generator` names (as in step), generated and applied on the device."""
        self._need_schedule()
        dev = sample.device
        up = int(timestep) + self.config.num_train_timesteps // self.num_inference_steps
        if up >= self.config.num_train_timesteps:
            raise ValueError(f"undo_step: timestep {int(timestep)} has no grid level above it")
        x = sample.detach().float().contiguous()
        z = ops.randn(tuple(x.shape), self._state_for(generator, dev), advance=True)
        coef = self.jump_coefficients(int(timestep), up).view(1, 2).expand(x.shape[0], 2).contiguous().to(dev)
        return ops.add_noise(x, z, coef).to(sample.dtype)
