"""Test helper: a CPU restatement of diffusers 0.32.2 `DPMSolverMultistepScheduler` (deterministic algorithms, first and second
order, epsilon prediction, scaled_linear betas) -- the arithmetic the product's DPMSolverMultistepScheduler and aldm_dpm_step_fused
must reproduce.  diffusers itself is not installed, so no fixture pins it: this file is written from the documented formulas
 in diffusers' own form -- a model-output list, `lower_order_nums`, the step index found from the first
timestep -- and with diffusers' fp32 torch scalar ops, so it is an independent second statement of the product's host code.

It satisfies the scheduler interface that `oracle.pipeline.denoise_loop` and `oracle.pipeline.AudioLDMPipeline` call
(`set_timesteps`, `.timesteps`, `init_noise_sigma`, `scale_model_input`, `step(e, t, x, eta=0.0).prev_sample`), so the oracle UNet
and loop are reused unchanged.
"""
from types import SimpleNamespace

import numpy as np
import torch

AUDIOLDM = dict(num_train_timesteps=1000, beta_start=0.0015, beta_end=0.0195, steps_offset=1, timestep_spacing="leading")


class DPMSolverRestatement:
    def __init__(self, algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint", lower_order_final=True,
                 euler_at_final=False, final_sigmas_type="zero", **over):
        cfg = dict(AUDIOLDM)
        cfg.update(over)
        self.config = SimpleNamespace(algorithm_type=algorithm_type, solver_order=solver_order, solver_type=solver_type,
                                      lower_order_final=lower_order_final, euler_at_final=euler_at_final,
                                      final_sigmas_type=final_sigmas_type, **cfg)
        n = cfg["num_train_timesteps"]
        self.betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.init_noise_sigma = 1.0

    # ---- schedule ----
    def set_timesteps(self, num_inference_steps, device=None):
        c, N = self.config, num_inference_steps
        last = c.num_train_timesteps                    # lambda_min_clipped = -inf
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, last - 1, N + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ratio = last // (N + 1)
            ts = (np.arange(0, N + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64) + c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = np.arange(last, 0, -c.num_train_timesteps / N).round().copy().astype(np.int64) - 1
        else:
            raise ValueError(c.timestep_spacing)
        ac = self.alphas_cumprod
        sig = np.interp(ts, np.arange(0, len(ac)), (((1 - ac) / ac) ** 0.5).numpy())
        last_sigma = 0.0 if c.final_sigmas_type == "zero" else float(((1 - ac[0]) / ac[0]) ** 0.5)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [last_sigma]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = len(ts)
        self.model_outputs = [None] * c.solver_order
        self.lower_order_nums = 0
        self.step_index = None

    def scale_model_input(self, sample, timestep=None):
        return sample

    # ---- diffusers' pieces ----
    @staticmethod
    def _alpha_sigma(sigma):
        alpha = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha, sigma * alpha

    def _lam(self, i):
        a, s = self._alpha_sigma(self.sigmas[i])
        return a, s, torch.log(a) - torch.log(s)

    def convert_model_output(self, e, sample):
        if self.config.algorithm_type == "dpmsolver++":
            alpha_t, sigma_t = self._alpha_sigma(self.sigmas[self.step_index])
            return (sample - sigma_t * e) / alpha_t
        return e

    def first_order(self, m0, sample):
        i = self.step_index
        alpha_t, sigma_t, lambda_t = self._lam(i + 1)
        alpha_s, sigma_s, lambda_s = self._lam(i)
        h = lambda_t - lambda_s
        if self.config.algorithm_type == "dpmsolver++":
            return (sigma_t / sigma_s) * sample - (alpha_t * (torch.exp(-h) - 1.0)) * m0
        return (alpha_t / alpha_s) * sample - (sigma_t * (torch.exp(h) - 1.0)) * m0

    def second_order(self, outputs, sample):
        i = self.step_index
        alpha_t, sigma_t, lambda_t = self._lam(i + 1)
        alpha_s0, sigma_s0, lambda_s0 = self._lam(i)
        _, _, lambda_s1 = self._lam(i - 1)
        m0, m1 = outputs[-1], outputs[-2]
        h, h_0 = lambda_t - lambda_s0, lambda_s0 - lambda_s1
        r0 = h_0 / h
        D0, D1 = m0, (1.0 / r0) * (m0 - m1)
        pp, mid = self.config.algorithm_type == "dpmsolver++", self.config.solver_type == "midpoint"
        if pp and mid:
            return (sigma_t / sigma_s0) * sample - (alpha_t * (torch.exp(-h) - 1.0)) * D0 - 0.5 * (alpha_t * (torch.exp(-h) - 1.0)) * D1
        if pp:
            return (sigma_t / sigma_s0) * sample - (alpha_t * (torch.exp(-h) - 1.0)) * D0 + (alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)) * D1
        if mid:
            return (alpha_t / alpha_s0) * sample - (sigma_t * (torch.exp(h) - 1.0)) * D0 - 0.5 * (sigma_t * (torch.exp(h) - 1.0)) * D1
        return (alpha_t / alpha_s0) * sample - (sigma_t * (torch.exp(h) - 1.0)) * D0 - (sigma_t * ((torch.exp(h) - 1.0) / h - 1.0)) * D1

    def order_of(self, i, lower_order_nums=None):
        """the order diffusers' step() uses at step index i (lower_order_nums defaults to an uninterrupted loop's: min(i, order))"""
        c, N = self.config, len(self.timesteps)
        lon = min(i, c.solver_order) if lower_order_nums is None else lower_order_nums
        lower_order_final = i == N - 1 and (c.euler_at_final or (c.lower_order_final and N < 15) or c.final_sigmas_type == "zero")
        if c.solver_order == 1 or lon < 1 or lower_order_final:
            return 1
        return 2

    def step(self, model_output, timestep, sample, eta=0.0, **kw):
        if self.step_index is None:
            cand = (self.timesteps == int(timestep)).nonzero()
            self.step_index = len(self.timesteps) - 1 if len(cand) == 0 else int(cand[1 if len(cand) > 1 else 0])
        m = self.convert_model_output(model_output, sample)
        self.model_outputs = self.model_outputs[1:] + [m]
        sample = sample.to(torch.float32)
        if self.order_of(self.step_index, self.lower_order_nums) == 1:
            prev = self.first_order(m, sample)
        else:
            prev = self.second_order(self.model_outputs, sample)
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return SimpleNamespace(prev_sample=prev.to(model_output.dtype))

    # ---- the same update as rows x' = A x + B m0 + C (m0 - m1), for comparison with the product's coefficient_table() ----
    def coefficient_rows(self):
        rows = []
        pp, mid = self.config.algorithm_type == "dpmsolver++", self.config.solver_type == "midpoint"
        for i in range(len(self.timesteps)):
            alpha_t, sigma_t, lambda_t = self._lam(i + 1)
            alpha_s0, sigma_s0, lambda_s0 = self._lam(i)
            h = lambda_t - lambda_s0
            A = sigma_t / sigma_s0 if pp else alpha_t / alpha_s0
            B = -(alpha_t * (torch.exp(-h) - 1.0)) if pp else -(sigma_t * (torch.exp(h) - 1.0))
            order = self.order_of(i)
            C = 0.0
            if order == 2:
                _, _, lambda_s1 = self._lam(i - 1)
                inv_r0 = 1.0 / ((lambda_s0 - lambda_s1) / h)
                if pp:
                    d1 = -0.5 * (alpha_t * (torch.exp(-h) - 1.0)) if mid else alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)
                else:
                    d1 = -0.5 * (sigma_t * (torch.exp(h) - 1.0)) if mid else -(sigma_t * ((torch.exp(h) - 1.0) / h - 1.0))
                C = float(d1 * inv_r0)
            rows.append([float(alpha_s0), float(sigma_s0), float(A), float(B), C, 1.0 if pp else 0.0, 1.0 if order == 2 else 0.0, 0.0])
        return torch.tensor(rows, dtype=torch.float32)
