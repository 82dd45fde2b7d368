"""Test helper: a CPU restatement of the training-recipe arithmetic the product's kernels must reproduce -- diffusers'
`training_utils.compute_snr` and the min-SNR-gamma loss weighting of its `--snr_gamma` training scripts (epsilon prediction),
and torch's own `clip_grad_norm_` + `AdamW` as the optimiser-side oracle.  diffusers itself is not installed, so no fixture pins
it: this file is written from the documented formulas in diffusers' own form -- square roots of the
cumulative alphas gathered per timestep, `torch.stack([snr, gamma]).min(dim=1)`, `mse(reduction="none").mean(dim=[1, 2, 3]) * w`
-- so it is an independent second statement of what `aldm_mse_grad_snr` computes in one pass.
"""
import torch
import torch.nn.functional as F


def scaled_linear_alphas_cumprod(num_train_timesteps=1000, beta_start=0.0015, beta_end=0.0195):
    """The AudioLDM noise schedule (scaled_linear betas), as diffusers' schedulers build it."""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def compute_snr(alphas_cumprod, timesteps):
    """diffusers.training_utils.compute_snr: (alpha_t / sigma_t)^2 per sample."""
    sqrt_alphas_cumprod = alphas_cumprod ** 0.5
    sqrt_one_minus_alphas_cumprod = (1.0 - alphas_cumprod) ** 0.5
    alpha = sqrt_alphas_cumprod[timesteps].float()
    sigma = sqrt_one_minus_alphas_cumprod[timesteps].float()
    return (alpha / sigma) ** 2


def min_snr_weights(alphas_cumprod, timesteps, snr_gamma):
    """mse_loss_weights of the epsilon-prediction branch: min(snr, gamma) / snr."""
    snr = compute_snr(alphas_cumprod, timesteps)
    return torch.stack([snr, torch.full_like(snr, snr_gamma)], dim=1).min(dim=1)[0] / snr


def min_snr_loss(pred, target, alphas_cumprod, timesteps, snr_gamma):
    """loss = (mse(reduction="none").mean(over everything but the batch) * weights).mean()"""
    loss = F.mse_loss(pred.float(), target.float(), reduction="none")
    loss = loss.mean(dim=list(range(1, loss.ndim))) * min_snr_weights(alphas_cumprod, timesteps, snr_gamma)
    return loss.mean()


def clipped_adamw_steps(p0, grads, max_norm, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, lrs=None):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW over a list of gradients; yields (parameters, pre-clip norm) per step."""
    p = torch.nn.Parameter(p0.detach().clone().float())
    opt = torch.optim.AdamW([p], lr=lr, betas=betas, weight_decay=weight_decay, eps=eps)
    for i, g in enumerate(grads):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[i]
        p.grad = g.detach().clone().float()
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm) if max_norm is not None else torch.linalg.vector_norm(p.grad)
        opt.step()
        yield p.detach().clone(), float(norm)
