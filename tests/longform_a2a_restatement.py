"""Test helper, not a test: an independent statement of long-form audio-to-audio in plain torch on the CPU,
built on what exists -- longform_restatement's windowed step followed by the legacy inpaint blend, the windowed loop over a suffix
of the schedule on any UNet callable, and the windowed encode (oracle mel, oracle VAE encoder on every window in fp32, the windows'
moments blended in float64).  Everything but the encode takes the dtype of its inputs.

Layouts as in longform_restatement: the time axis at `dim` (1 channels-last, 2 NCHW); the mask is [B, rows, W] and broadcasts over
the channels.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_restatement as R  # noqa: E402


def known_coefficients(sched, solver, i):
    """(a, s) with which the known clip is noised to the level of schedule index i:  known = a x0 + s noise.  DDIM reads its
    alphas_cumprod at timesteps[i]; the sigma-parametrised solvers have alpha = 1 / sqrt(sigma^2 + 1), s = sigma alpha; Euler-ancestral
    lives in sigma space: (1, sigma)."""
    if solver == "ddim":
        abar = sched.alphas_cumprod[int(sched.timesteps[i])]
        return abar ** 0.5, (1 - abar) ** 0.5
    sig = sched.sigmas[i]
    if solver == "euler_a":
        return torch.ones((), dtype=sig.dtype), sig
    a = 1.0 / (sig ** 2 + 1) ** 0.5
    return a, sig * a


def inpaint_blend(xn, x0, noise, m, a, s, last, dim=1):
    """the legacy inpaint blend: (1 - m) (a x0 + s noise) + m xn, the last step returning x0 itself where the mask keeps it"""
    mm = m.to(xn.dtype).unsqueeze(-1 if dim == 1 else 1)
    known = x0 if last else a * x0 + s * noise
    return (1 - mm) * known + mm * xn


def masked_windowed_step(sched, solver, i, n_total, x, eps_u_win, eps_t_win, g, tables, x0, eps0, m, dim=1, **step_kw):
    """Step i (an index into the FULL schedule of n_total steps): longform_restatement.windowed_step, then the blend toward the level
    of index i + 1.  eps0: the noise the known clip is noised with (step_kw may carry Euler-ancestral's own `noise`).  m None: no
    blend."""
    xn = R.windowed_step(sched, sched.timesteps[i], x, eps_u_win, eps_t_win, g, tables, dim=dim, **step_kw)
    if m is None:
        return xn
    last = i + 1 >= n_total
    a, s = (None, None) if last else known_coefficients(sched, solver, i + 1)
    return inpaint_blend(xn, x0, eps0, m, a, s, last, dim)


def windowed_a2a_loop(unet, sched, solver, x0, eps, pe, ne, steps, begin, g, tables, mask=None, trace=None):
    """The windowed loop from schedule index `begin` over any UNet callable with the oracle's signature.  x0, eps NCHW
    [B, C, rows, W] (the scaled clip latents and the noise), mask [B, rows, W] or None.  begin == 0 starts from pure noise."""
    offs, hw, cover, weight = tables
    K, B = len(offs), x0.shape[0]
    cfg = g > 1.0

    def per_window(e):
        e = e[:, None, :].expand(B, K, e.shape[-1]) if e.dim() == 2 else e
        return e.reshape(B * K, e.shape[-1])

    emb = torch.cat([per_window(ne), per_window(pe)]) if cfg else per_window(pe)
    sched.set_timesteps(steps)
    if begin == 0:
        x = eps * sched.init_noise_sigma
    else:
        a, s = known_coefficients(sched, solver, begin)
        x = a * x0 + s * eps
    for i in range(begin, steps):
        t = sched.timesteps[i]
        win = R.gather(x, offs, hw, dim=2)
        x_in = sched.scale_model_input(torch.cat([win, win]) if cfg else win, t)
        e = unet(x_in, t, encoder_hidden_states=None, class_labels=emb)[0]
        eu, et = e.chunk(2) if cfg else (e, None)
        x = masked_windowed_step(sched, solver, i, steps, x, eu, et, g, tables, x0, eps, mask, dim=2, eta=0.0)
        if trace is not None:
            trace.append(x.clone())
    return x


def tables_from_plan(plan):
    """(offsets, hw, cover, weight) as longform_restatement uses them, out of a WindowPlan: its own float64 weights"""
    cover = [[int(k) for k in row if k >= 0] for row in plan.cover]
    weight = [[float(w) for w in plan.weight64[r][:len(cover[r])]] for r in range(plan.rows)]
    return list(plan.offsets), plan.window_rows, cover, weight


def windowed_encode(vae, audio, mel_frames, tables, mel_tables, post=None):
    """The long clip's VAE moments and x0: the oracle log-mel [B, 1, mel_frames, n_mel], its windows (mel_tables) through the oracle
    encoder in fp32, the windows' raw moments (mean | logvar) blended by `tables` in float64, then ONE posterior sample on the long
    moments with the noise `post`.  Returns (mean, std, x0 or None), fp32 NCHW long; x0 carries scaling_factor."""
    from oracle.mel import DSP, log_mel_spec
    mel = log_mel_spec(audio, dict(DSP, target_length=mel_frames))
    win = R.gather(mel, mel_tables[0], mel_tables[1], dim=2)
    mom = vae.quant_conv(vae.encoder(win)).double()
    offs, hw, cover, weight = tables
    rows = mel_frames * hw // mel_tables[1]
    long = R.blend(mom, offs, hw, rows, cover, weight, dim=2)
    mean, logvar = long.chunk(2, dim=1)
    std = torch.exp(0.5 * logvar.clamp(-30.0, 20.0))
    x0 = None if post is None else ((mean + std * post.double()) * vae.config.scaling_factor).float()
    return mean.float(), std.float(), x0
