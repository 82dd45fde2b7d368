"""Test helper, not a test: an independent statement of windowed denoising in plain torch on the CPU -- the
window plan row by row, the gather of windows out of the long latent, the blend of windows back into it, the windowed scheduler
step (blend the windows' eps halves, then the EXISTING restatement's step on the long latent) and the windowed loop over any UNet
callable.  Everything takes the dtype of its inputs, so a test runs it in fp32 and in float64 on the same numbers.

Tensors carry the time axis at `dim`: 1 for channels-last latents [B, rows, W, C], 2 for NCHW [B, C, rows, W].  Windows are batch
rows in (clip, window) order: [B * K, ...] with the window length at `dim`.
"""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dpm_restatement import DPMSolverRestatement  # noqa: E402


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def offsets_of(rows, hw, ov, loop=False):
    S = hw - ov
    if loop:
        assert rows % S == 0 and rows >= hw
        return [k * S for k in range(rows // S)]
    if rows <= hw:
        return [0]
    out = []
    o = 0
    while o + hw < rows:
        out.append(o)
        o += S
    return out + [rows - hw]


def tables_of(rows, hw, ov, loop=False, min_form=False):
    """(offsets, hw, cover, weight): cover[r] the ascending window indices over long row r, weight[r] their float64 weights.
    min_form=True: the profile as the plain min(1, (i + 1) / (L + 1), (hw - i) / (R + 1)), for comparison on plans with at most
    two windows over a row, where the two agree"""
    offs = offsets_of(rows, hw, ov, loop)
    hw = min(hw, rows) if not loop else hw
    K = len(offs)

    def overlap(a, b):                                    # rows that windows a and b (neighbours) share
        if loop:
            return ov if K > 1 else 0
        if a < 0 or b >= K:
            return 0
        return max(0, offs[a] + hw - offs[b])

    def fade_in(k, i):
        """the crossfade from window k - 1 into window k, seen from window k's row i (any integer): 0 before the window, (i + 1) /
        (L + 1) over the L shared rows, 1 behind them"""
        if i < 0:
            return 0.0
        return min(1.0, (i + 1) / (overlap(k - 1, k) + 1))

    def profile(k, i):
        """Window k fades in from its predecessor and out into its successor, and the successor's fade-in IS its fade-out: what it
        holds at row i is the difference of the two crossfades.  Where they do not run at once (all plans with at most two
        windows over a row) this is min(1, (i + 1) / (L + 1), (hw - i) / (R + 1))."""
        R = overlap(k, k + 1)
        nxt = fade_in(k + 1, i - (hw - R)) if (loop and K > 1) or k + 1 < K else 0.0      # (row i of k is row i - (hw - R) of k + 1)
        return fade_in(k, i) - nxt

    def literal(k, i):
        L, R = overlap(k - 1, k), overlap(k, k + 1)
        return min(1.0, (i + 1) / (L + 1), (hw - i) / (R + 1))

    cover, weight = [], []
    for r in range(rows):
        ks, ps = [], []
        for k in range(K):
            i = (r - offs[k]) % rows if loop else r - offs[k]
            if 0 <= i < hw:
                ks.append(k)
                ps.append(literal(k, i) if min_form else profile(k, i))
        tot = sum(ps)
        cover.append(ks)
        weight.append([p / tot for p in ps])
    return offs, hw, cover, weight


def scaled(rows, hw, ov, f):
    return rows * f, hw * f, ov * f


# ---- gather and blend ---------------------------------------------------------------------------------------------------------
def gather(x, offs, hw, dim=1):
    """long [B, ..rows at dim..] -> windows [B * K, ..hw at dim..], rows modulo the long length"""
    rows = x.shape[dim]
    wins = [x.index_select(dim, torch.tensor([(o + i) % rows for i in range(hw)])) for o in offs]
    w = torch.stack(wins, dim=1)                                           # [B, K, ...]
    return w.reshape((x.shape[0] * len(offs),) + tuple(w.shape[2:]))


def blend(win, offs, hw, rows, cover, weight, dim=1):
    """windows [B * K, ..hw at dim..] -> long [B, ..rows at dim..]:  sum_j weight[r][j] * win[cover[r][j]] at its own row"""
    K = len(offs)
    B = win.shape[0] // K
    w = win.reshape((B, K) + tuple(win.shape[1:]))
    out_rows = []
    for r in range(rows):
        acc = None
        for k, wt in zip(cover[r], weight[r]):
            i = (r - offs[k]) % rows
            term = w[:, k].select(dim, i) * torch.tensor(wt, dtype=win.dtype)          # (w[:, k] dropped the K axis: dim is the window's own)
            acc = term if acc is None else acc + term
        out_rows.append(acc)
    return torch.stack(out_rows, dim=dim)


# ---- the schedulers' restatements, with a dtype ------------------------------------------------------------------------------------
class DPMRestatementTyped(DPMSolverRestatement):
    """DPMSolverRestatement whose step() keeps the sample's dtype (its own pins fp32): the same statements in float64"""

    def step(self, model_output, timestep, sample, eta=0.0, **kw):
        if self.step_index is None:
            self.step_index = int((self.timesteps == int(timestep)).nonzero()[0])
        m = self.convert_model_output(model_output, sample)
        self.model_outputs = self.model_outputs[1:] + [m]
        first = self.order_of(self.step_index, self.lower_order_nums) == 1
        prev = self.first_order(m, sample) if first else self.second_order(self.model_outputs, sample)
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return SimpleNamespace(prev_sample=prev)


def make_restatement(solver, dtype=torch.float32, noise_fn=None):
    """the existing restatement of `solver` ("ddim", "dpm", "unipc", "euler_a")"""
    if solver == "ddim":
        from oracle.ddim import DDIMScheduler
        return DDIMScheduler()
    if solver == "dpm":
        return DPMRestatementTyped()
    if solver == "unipc":
        from unipc_restatement import UniPCRestatement
        return UniPCRestatement(dtype=dtype)
    from euler_a_restatement import EulerAncestralRestatement
    return EulerAncestralRestatement(noise_fn=noise_fn)


def set_timesteps_typed(sched, n, dtype):
    """set_timesteps, then the scheduler's own tables in `dtype`: the float64 run then computes its coefficients in float64 too (the
    restatements keep fp32 tables, as diffusers does; UniPCRestatement takes its dtype at construction)"""
    sched.set_timesteps(n)
    for name in ("sigmas", "alphas_cumprod", "final_alpha_cumprod"):
        if hasattr(sched, name) and dtype != torch.float32:
            setattr(sched, name, getattr(sched, name).to(dtype))
    return sched


def windowed_step(sched, t, x, eps_u_win, eps_t_win, g, tables, dim=1, **step_kw):
    """One windowed step: blend each half's windows into the long layout, combine the halves, then the restatement's own step.
    eps_t_win None: no guidance.  Returns the new long latent."""
    offs, hw, cover, weight = tables
    rows = x.shape[dim]
    e = blend(eps_u_win, offs, hw, rows, cover, weight, dim)
    if eps_t_win is not None:
        et = blend(eps_t_win, offs, hw, rows, cover, weight, dim)
        e = e + g * (et - e)
    return sched.step(e, t, x, **step_kw).prev_sample


def windowed_loop(unet, sched, latents, pe, ne, steps, g, tables, trace=None):
    """The windowed denoise loop over any UNet callable with the oracle's signature (oracle.pipeline.denoise_loop with windows):
    latents NCHW [B, C, rows, W]; pe / ne [B, D] or [B, K, D] (one prompt per window).  Returns the final long latent."""
    offs, hw, cover, weight = tables
    K, B = len(offs), latents.shape[0]
    cfg = g > 1.0

    def per_window(e):
        e = e[:, None, :].expand(B, K, e.shape[-1]) if e.dim() == 2 else e
        return e.reshape(B * K, e.shape[-1])

    emb = torch.cat([per_window(ne), per_window(pe)]) if cfg else per_window(pe)
    sched.set_timesteps(steps)
    x = latents * sched.init_noise_sigma
    for t in sched.timesteps:
        win = gather(x, offs, hw, dim=2)
        x_in = torch.cat([win, win]) if cfg else win
        x_in = sched.scale_model_input(x_in, t)
        eps = unet(x_in, t, encoder_hidden_states=None, class_labels=emb)[0]
        eu, et = eps.chunk(2) if cfg else (eps, None)
        x = windowed_step(sched, t, x, eu, et, g, tables, dim=2, eta=0.0)
        if trace is not None:
            trace.append(x.clone())
    return x
