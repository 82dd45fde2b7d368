"""Test helper: a float64 restatement of RePaint (Lugmayr et al., "RePaint: Inpainting using Denoising Diffusion Probabilistic Models",
CVPR 2022, Algorithm 1) on DDIM's "leading" grid with eta = 0 -- the arithmetic the product's RePaintScheduler and
aldm_repaint_step_fused_masked must reproduce.  diffusers is not installed, so no fixture pins it: the walk is diffusers 0.32.2
`RePaintScheduler.set_timesteps` restated, the rest is written from the paper.  Only the alpha-bar table is diffusers' fp32 one (the
scheduler's own table is the data both sides start from); everything behind it is float64.

Algorithm 1, per UNet call at grid level l (timestep t_l = l * (T // N) + steps_offset), landing on level l - 1:
    line 4   x_known   = sqrt(abar_{l-1}) x0 + sqrt(1 - abar_{l-1}) zk          zk ~ N(0, I), FRESH at every call
    line 6   x_unknown = the reverse step from eps; here DDIM's, eta = 0:
                         sqrt(abar_{l-1}) (x - sqrt(1 - abar_l) eps) / sqrt(abar_l) + sqrt(1 - abar_{l-1}) eps
    line 7   x_{l-1}   = (1 - m) x_known + m x_unknown                         m = 1 REGENERATES (the paper's mask is 1 - m)
    line 10  one level back up:  x ~ N(sqrt(1 - beta) x, beta I) for every beta between the two levels; J levels compose to
                         x_{l-1+J} = sqrt(r) x_{l-1} + sqrt(1 - r) zj ,  r = abar_{l-1+J} / abar_{l-1}
abar_{-1} = final_alpha_cumprod; after the LAST call the known part is x0 itself (no noise is left to add at the end of the loop).
The noises zk, zj are ARGUMENTS of step, so a test can feed the device's own draws and compare the deterministic arithmetic alone.
"""
import numpy as np
import torch

AUDIOLDM = dict(num_train_timesteps=1000, beta_start=0.0015, beta_end=0.0195, steps_offset=1, set_alpha_to_one=False)


def walk_levels(N, jump_length, jump_n_sample):
    """diffusers' list, in grid levels: down from N - 1; at a level that still has a jump, use it up and climb jump_length levels"""
    jumps = {}
    for j in range(0, N - jump_length, jump_length):
        jumps[j] = jump_n_sample - 1
    out = []
    t = N
    while t >= 1:
        t = t - 1
        out.append(t)
        if jumps.get(t, 0) > 0:
            jumps[t] = jumps[t] - 1
            for _ in range(jump_length):
                t = t + 1
                out.append(t)
    return out


def fold(walk):
    """every falling (or first) entry is a UNet call; the rising entries behind it are its jump: [(level, J)]"""
    calls = []
    for i, level in enumerate(walk):
        if i > 0 and level > walk[i - 1]:
            calls[-1] = (calls[-1][0], calls[-1][1] + 1)
        else:
            calls.append((level, 0))
    return calls


def n_calls(N, jump_length, jump_n_sample):
    return N + len(range(0, N - jump_length, jump_length)) * (jump_n_sample - 1) * jump_length


class RePaintRestatement:
    def __init__(self, jump_length=10, jump_n_sample=10, **over):
        cfg = dict(AUDIOLDM)
        cfg.update(over)
        self.cfg, self.jump_length, self.jump_n_sample = cfg, jump_length, jump_n_sample
        n = cfg["num_train_timesteps"]
        betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).double().numpy()
        self.final = 1.0 if cfg["set_alpha_to_one"] else float(self.alphas_cumprod[0])

    def set_timesteps(self, N, jump_length=None, jump_n_sample=None):
        self.N = N
        self.walk = walk_levels(N, self.jump_length if jump_length is None else jump_length,
                                self.jump_n_sample if jump_n_sample is None else jump_n_sample)
        self.folded = fold(self.walk)
        self.ratio = self.cfg["num_train_timesteps"] // N
        self.timesteps = np.array([l * self.ratio + self.cfg["steps_offset"] for l, _ in self.folded], dtype=np.int64)

    def abar(self, level):
        return self.final if level < 0 else float(self.alphas_cumprod[level * self.ratio + self.cfg["steps_offset"]])

    def row(self, k):
        """{sa, sb, sap, sbp, c1, c2, 0, 0} of call k, float64"""
        l, J = self.folded[k]
        a, ap = self.abar(l), self.abar(l - 1)
        r = self.abar(l - 1 + J) / ap
        c1, c2 = (np.sqrt(r), np.sqrt(1 - r)) if J else (1.0, 0.0)
        return np.array([np.sqrt(a), np.sqrt(1 - a), np.sqrt(ap), np.sqrt(1 - ap), c1, c2, 0.0, 0.0])

    def blend_row(self, k):
        if k == len(self.folded) - 1:
            return np.array([1.0, 0.0])
        ap = self.abar(self.folded[k][0] - 1)
        return np.array([np.sqrt(ap), np.sqrt(1 - ap)])

    def table(self):
        return np.stack([self.row(k) for k in range(len(self.folded))])

    def blend_table(self):
        return np.stack([self.blend_row(k) for k in range(len(self.folded))])

    def step(self, k, eps, x, x0, mask, zk, zj):
        """call k on float64 tensors (mask broadcasts; 1 = regenerate) -> the sample the NEXT call starts from"""
        sa, sb, sap, sbp, c1, c2 = self.row(k)[:6]
        a, s = self.blend_row(k)
        unknown = sap * (x - sb * eps) / sa + sbp * eps
        known = a * x0 + s * zk
        xb = (1 - mask) * known + mask * unknown
        return c1 * xb + c2 * zj


def gaussian_slope(jump_n_sample, seed, n_problems=20000, N=10, jump_length=2, rho=0.9):
    """The property RePaint exists for, on a model with an exact eps: data (u, v) ~ N(0, [[1, rho], [rho, 1]]), u kept and v
    regenerated from noise.  Returns the least-squares slope of the final v on u; the true conditional slope is rho.
    x_t = sqrt(abar) x0 + sqrt(1 - abar) e has covariance S = abar Sigma + (1 - abar) I, and E[e | x_t] = sqrt(1 - abar) S^-1 x_t."""
    g = torch.Generator().manual_seed(seed)
    r = RePaintRestatement(jump_length=jump_length, jump_n_sample=jump_n_sample)
    r.set_timesteps(N)
    sigma = torch.tensor([[1.0, rho], [rho, 1.0]], dtype=torch.float64)
    u = torch.randn(n_problems, generator=g, dtype=torch.float64)
    x0 = torch.stack([u, torch.zeros_like(u)], dim=1)                # (the regenerated pixel of x0 is never read: its mask is 1)
    mask = torch.tensor([0.0, 1.0], dtype=torch.float64)
    x = torch.randn(n_problems, 2, generator=g, dtype=torch.float64)
    for k, (level, _) in enumerate(r.folded):
        a = r.abar(level)
        s_inv = torch.linalg.inv(a * sigma + (1 - a) * torch.eye(2, dtype=torch.float64))
        eps = np.sqrt(1 - a) * x @ s_inv
        zk = torch.randn(n_problems, 2, generator=g, dtype=torch.float64)
        zj = torch.randn(n_problems, 2, generator=g, dtype=torch.float64)
        x = r.step(k, eps, x, x0, mask, zk, zj)
    return float((x[:, 0] * x[:, 1]).sum() / (x[:, 0] * x[:, 0]).sum())
