"""Test helper: a CPU restatement of diffusers 0.32.2 `EulerAncestralDiscreteScheduler` for epsilon prediction and scaled_linear
betas -- the arithmetic the product's EulerAncestralDiscreteScheduler and aldm_euler_a_step_fused must reproduce.  diffusers itself is
not installed, so no fixture pins it: this file is written from the documented formulas with diffusers' fp32
torch scalar ops.  The noise z of a step is an ARGUMENT (`noise=` to step, or the `noise_fn(i, shape)` given at construction), so a
test can feed the device's own draw and compare the deterministic arithmetic alone.

It satisfies the scheduler interface that `oracle.pipeline.denoise_loop` calls (`set_timesteps`, `.timesteps`, `init_noise_sigma`,
`scale_model_input`, `step(e, t, x, eta=0.0).prev_sample`), so the oracle UNet and loop are reused unchanged.
"""
from types import SimpleNamespace

import numpy as np
import torch

AUDIOLDM = dict(num_train_timesteps=1000, beta_start=0.0015, beta_end=0.0195, steps_offset=1, timestep_spacing="leading")


class EulerAncestralRestatement:
    def __init__(self, noise_fn=None, **over):
        cfg = dict(AUDIOLDM)
        cfg.update(over)
        self.config = SimpleNamespace(**cfg)
        n = cfg["num_train_timesteps"]
        self.betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.noise_fn = noise_fn
        self.num_inference_steps = None

    def set_timesteps(self, num_inference_steps, device=None):
        c, N, n = self.config, num_inference_steps, self.config.num_train_timesteps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, n - 1, N, dtype=np.float32)[::-1].copy()
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, N) * (n // N)).round()[::-1].copy().astype(np.float32) + c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = np.arange(n, 0, -n / N).round().copy().astype(np.float32) - 1
        else:
            raise ValueError(c.timestep_spacing)
        ac = self.alphas_cumprod
        sig = np.interp(ts, np.arange(0, len(ac)), (((1 - ac) / ac) ** 0.5).numpy())
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts.astype(np.float32))
        self.num_inference_steps = N
        self.step_index = None

    @property
    def init_noise_sigma(self):
        m = self.sigmas.max()
        return float(m) if self.config.timestep_spacing in ("linspace", "trailing") else float((m ** 2 + 1) ** 0.5)

    def _index(self, timestep):
        return int((self.timesteps == float(timestep)).nonzero()[0])

    def scale_model_input(self, sample, timestep):
        if self.step_index is None:
            self.step_index = self._index(timestep)
        return sample / ((self.sigmas[self.step_index] ** 2 + 1) ** 0.5)

    def sigma_up_down(self, i):
        s_from, s_to = self.sigmas[i], self.sigmas[i + 1]
        up = (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5
        return up, (s_to ** 2 - up ** 2) ** 0.5

    def row(self, i):
        """{dt, sigma_up, in_scale_next, sigma_down}: the product's coefficient-table row of step i"""
        up, down = self.sigma_up_down(i)
        return torch.stack([down - self.sigmas[i], up, 1.0 / ((self.sigmas[i + 1] ** 2 + 1) ** 0.5), down]).float()

    def step(self, model_output, timestep, sample, noise=None, eta=0.0, **kw):
        if self.step_index is None:
            self.step_index = self._index(timestep)
        i = self.step_index
        if noise is None:
            noise = self.noise_fn(i, tuple(sample.shape))
        up, down = self.sigma_up_down(i)
        prev = sample + model_output * (down - self.sigmas[i]) + up * noise.to(sample.dtype)
        self.step_index += 1
        return SimpleNamespace(prev_sample=prev)
