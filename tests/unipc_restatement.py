"""Test helper: a CPU restatement of diffusers 0.32.2 `UniPCMultistepScheduler` (orders 1 and 2, bh1 / bh2, predict_x0 or noise
prediction, epsilon models, scaled_linear betas) -- the arithmetic the product's UniPCMultistepScheduler and aldm_unipc_step_fused must
reproduce.  diffusers itself is not installed, so no fixture pins it: this file is written from the published update (DESIGN.md section
17) in diffusers' own form -- a model-output list that is shifted, `last_sample`, `this_order`, `lower_order_nums`, and
`multistep_uni_p_bh_update` / `multistep_uni_c_bh_update` with their `rks` / `R` / `b` / `rhos` construction -- and never looks at the
product's coefficient_table(), so it is an independent second statement of the product's host code.

`dtype`: torch.float32 (diffusers' own arithmetic) or torch.float64 (the same statements with every scalar and tensor in double; the
sigmas stay the fp32 schedule's values).  The distance between the two runs is the rounding noise of the fp32 statement itself.

It satisfies the scheduler interface that `oracle.pipeline.denoise_loop` and `oracle.pipeline.AudioLDMPipeline` call
(`set_timesteps`, `.timesteps`, `init_noise_sigma`, `scale_model_input`, `step(e, t, x, eta=0.0).prev_sample`, `add_noise`,
`set_begin_index`), so the oracle UNet and loop are reused unchanged.
"""
from types import SimpleNamespace

import numpy as np
import torch

AUDIOLDM = dict(num_train_timesteps=1000, beta_start=0.0015, beta_end=0.0195, steps_offset=1, timestep_spacing="leading")


class UniPCRestatement:
    def __init__(self, solver_order=2, predict_x0=True, solver_type="bh2", lower_order_final=True, disable_corrector=(),
                 final_sigmas_type="zero", dtype=torch.float32, **over):
        cfg = dict(AUDIOLDM)
        cfg.update(over)
        self.config = SimpleNamespace(solver_order=solver_order, predict_x0=predict_x0, solver_type=solver_type,
                                      lower_order_final=lower_order_final, disable_corrector=list(disable_corrector),
                                      final_sigmas_type=final_sigmas_type, **cfg)
        self.dtype = dtype
        self.predict_x0 = predict_x0
        self.disable_corrector = list(disable_corrector)
        n = cfg["num_train_timesteps"]
        self.betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.init_noise_sigma = 1.0
        self.begin_index = None

    # ---- schedule ----
    def set_timesteps(self, num_inference_steps, device=None):
        c, N = self.config, num_inference_steps
        n = c.num_train_timesteps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, n - 1, N + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ratio = n // (N + 1)
            ts = (np.arange(0, N + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64) + c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = np.arange(n, 0, -n / N).round().copy().astype(np.int64) - 1
        else:
            raise ValueError(c.timestep_spacing)
        ac = self.alphas_cumprod
        sig = np.interp(ts, np.arange(0, len(ac)), (((1 - ac) / ac) ** 0.5).numpy())
        last_sigma = 0.0 if c.final_sigmas_type == "zero" else float(((1 - ac[0]) / ac[0]) ** 0.5)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [last_sigma]]).astype(np.float32)).to(self.dtype)
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = len(ts)
        self.model_outputs = [None] * c.solver_order
        self.lower_order_nums = 0
        self.this_order = None
        self.last_sample = None
        self.step_index = None
        self.begin_index = None

    def set_begin_index(self, begin_index=0):
        self.begin_index = begin_index

    def scale_model_input(self, sample, timestep=None):
        return sample

    def add_noise(self, original_samples, noise, timesteps):
        if self.begin_index is None:
            idx = []
            for t in torch.as_tensor(timesteps).reshape(-1).tolist():
                cand = (self.timesteps == int(t)).nonzero()
                idx.append(len(self.timesteps) - 1 if len(cand) == 0 else int(cand[1 if len(cand) > 1 else 0]))
        elif self.step_index is not None:
            idx = [self.step_index] * torch.as_tensor(timesteps).numel()
        else:
            idx = [self.begin_index] * torch.as_tensor(timesteps).numel()
        sigma = self.sigmas[idx].to(torch.float32).flatten()
        while sigma.dim() < original_samples.dim():
            sigma = sigma.unsqueeze(-1)
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(sigma)
        return alpha_t * original_samples + sigma_t * noise

    # ---- diffusers' pieces ----
    @staticmethod
    def _sigma_to_alpha_sigma_t(sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha_t, sigma * alpha_t

    def convert_model_output(self, model_output, sample):
        if self.predict_x0:
            alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(self.sigmas[self.step_index])
            return (sample - sigma_t * model_output) / alpha_t
        return model_output

    def _bh_terms(self, h, rks, order):
        """R, b, (h_phi_1, B_h) of diffusers' two update functions (the loop they share, word for word)"""
        hh = -h if self.predict_x0 else h
        h_phi_1 = torch.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1
        factorial_i = 1
        B_h = hh if self.config.solver_type == "bh1" else torch.expm1(hh)
        R, b = [], []
        for i in range(1, order + 1):
            R.append(torch.pow(rks, i - 1))
            b.append(h_phi_k * factorial_i / B_h)
            factorial_i *= i + 1
            h_phi_k = h_phi_k / hh - 1 / factorial_i
        return torch.stack(R), torch.stack(b), h_phi_1, B_h

    def _lambda(self, i):
        alpha, sigma = self._sigma_to_alpha_sigma_t(self.sigmas[i])
        return alpha, sigma, torch.log(alpha) - torch.log(sigma)

    def multistep_uni_p_bh_update(self, sample, order):
        m0 = self.model_outputs[-1]
        x = sample
        alpha_t, sigma_t, lambda_t = self._lambda(self.step_index + 1)
        alpha_s0, sigma_s0, lambda_s0 = self._lambda(self.step_index)
        h = lambda_t - lambda_s0
        rks, D1s = [], []
        for i in range(1, order):
            mi = self.model_outputs[-(i + 1)]
            lambda_si = self._lambda(self.step_index - i)[2]
            rk = (lambda_si - lambda_s0) / h
            rks.append(rk)
            D1s.append((mi - m0) / rk)
        rks.append(torch.ones((), dtype=self.dtype))
        rks = torch.stack(rks)
        R, b, h_phi_1, B_h = self._bh_terms(h, rks, order)
        if D1s:
            D1s = torch.stack(D1s, dim=0)
            rhos_p = torch.tensor([0.5], dtype=self.dtype) if order == 2 else torch.linalg.solve(R[:-1, :-1], b[:-1])
            pred_res = torch.einsum("k,k...->...", rhos_p, D1s)
        else:
            pred_res = 0
        # (one departure from diffusers' text: a first-order step adds no `B_h * 0` term.  diffusers forms it, and with bh1 on the step
        # to sigma 0, where B_h = -inf, that product is NaN; with bh2 and everywhere else it is an exact zero)
        if self.predict_x0:
            x_t_ = sigma_t / sigma_s0 * x - alpha_t * h_phi_1 * m0
            return x_t_ - alpha_t * B_h * pred_res if len(D1s) else x_t_
        x_t_ = alpha_t / alpha_s0 * x - sigma_t * h_phi_1 * m0
        return x_t_ - sigma_t * B_h * pred_res if len(D1s) else x_t_

    def multistep_uni_c_bh_update(self, this_model_output, last_sample, order):
        m0 = self.model_outputs[-1]
        x = last_sample
        model_t = this_model_output
        alpha_t, sigma_t, lambda_t = self._lambda(self.step_index)
        alpha_s0, sigma_s0, lambda_s0 = self._lambda(self.step_index - 1)
        h = lambda_t - lambda_s0
        rks, D1s = [], []
        for i in range(1, order):
            mi = self.model_outputs[-(i + 1)]
            lambda_si = self._lambda(self.step_index - (i + 1))[2]
            rk = (lambda_si - lambda_s0) / h
            rks.append(rk)
            D1s.append((mi - m0) / rk)
        rks.append(torch.ones((), dtype=self.dtype))
        rks = torch.stack(rks)
        R, b, h_phi_1, B_h = self._bh_terms(h, rks, order)
        rhos_c = torch.tensor([0.5], dtype=self.dtype) if order == 1 else torch.linalg.solve(R, b)
        corr_res = torch.einsum("k,k...->...", rhos_c[:-1], torch.stack(D1s, dim=0)) if D1s else 0
        D1_t = model_t - m0
        if self.predict_x0:
            x_t_ = sigma_t / sigma_s0 * x - alpha_t * h_phi_1 * m0
            return x_t_ - alpha_t * B_h * (corr_res + rhos_c[-1] * D1_t)
        x_t_ = alpha_t / alpha_s0 * x - sigma_t * h_phi_1 * m0
        return x_t_ - sigma_t * B_h * (corr_res + rhos_c[-1] * D1_t)

    def step(self, model_output, timestep, sample, eta=0.0, **kw):
        if self.step_index is None:
            if self.begin_index is None:
                cand = (self.timesteps == int(timestep)).nonzero()
                self.step_index = len(self.timesteps) - 1 if len(cand) == 0 else int(cand[1 if len(cand) > 1 else 0])
            else:
                self.step_index = self.begin_index
        out_dtype = model_output.dtype
        model_output, sample = model_output.to(self.dtype), sample.to(self.dtype)
        use_corrector = (self.step_index > 0 and self.step_index - 1 not in self.disable_corrector and self.last_sample is not None)
        model_output_convert = self.convert_model_output(model_output, sample)
        if use_corrector:
            sample = self.multistep_uni_c_bh_update(model_output_convert, self.last_sample, self.this_order)
        for i in range(self.config.solver_order - 1):
            self.model_outputs[i] = self.model_outputs[i + 1]
        self.model_outputs[-1] = model_output_convert
        if self.config.lower_order_final:
            this_order = min(self.config.solver_order, len(self.timesteps) - self.step_index)
        else:
            this_order = self.config.solver_order
        self.this_order = min(this_order, self.lower_order_nums + 1)
        assert self.this_order > 0
        self.last_sample = sample
        prev_sample = self.multistep_uni_p_bh_update(sample, self.this_order)
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return SimpleNamespace(prev_sample=prev_sample.to(out_dtype if self.dtype == torch.float32 else self.dtype))
