"""Test helper: a numpy / float64 restatement of the training step's on-device noising (aldm_train_noise_fused), built on the
restatement of the device RNG in tests/philox_restatement.py.  Written from the stream contract and the formulas of the reference's
loop body (latent_dist.sample() * scaling_factor, DDIMScheduler.add_noise, diffusers' noise offset), not from the kernel.

A step that finds the stream at ordinal d uses four draws:
    d      B raw words       t_b = (word_b * T) >> 32
    d + 1  B*C*H*W normals   e, the posterior noise        (element index = the flat NCHW index)
    d + 2  B*C*H*W normals   n, the diffusion noise        (the same indexing)
    d + 3  B*C normals       o, the noise offset's normal per (sample, channel)
"""
import numpy as np

import philox_restatement as P

DRAWS_PER_STEP = 4
RANK_STRIDE = 2 ** 48


def timesteps_of(words, T):
    """t = (w * T) >> 32 on uint32 words: uniform on [0, T) up to 2^-32 T"""
    return ((np.asarray(words).astype(np.uint64) * np.uint64(T)) >> np.uint64(32)).astype(np.int64)


def draw_ordinals(ordinal):
    """the ordinals a step starting at `ordinal` reads, by what they supply"""
    return dict(t=ordinal, e=ordinal + 1, n=ordinal + 2, o=ordinal + 3, next=ordinal + DRAWS_PER_STEP)


def rank_base(rank):
    return rank * RANK_STRIDE


def step(seed, ordinal, shape, abar, noise_offset=0.0, moments=None, latents=None, scaling_factor=1.0, e=None, n=None, o=None):
    """One step's noising in float64.  shape = (B, C, H, W); abar [T]; exactly one of
         moments  [B, H, W, 2C] channels-last (mean | logvar)  -> lat = (mean + exp(0.5 clamp(logvar, -30, 20)) e) scaling_factor
         latents  [B, C, H, W]
    e / n / o: use these normals (NCHW [B, C, H, W] twice, [B, C]) instead of the restated ones -- the device's own fp32 draws, so
    that the arithmetic after the generator is measured on its own.
    Returns dict(timesteps int64 [B], e, n [B, C, H, W], o [B, C], target, noisy float64 channels-last [B, H, W, C], next)."""
    B, C, H, W = shape
    assert (moments is None) != (latents is None)
    abar = np.asarray(abar, dtype=np.float64)
    T = abar.shape[0]
    d = draw_ordinals(ordinal)
    t = timesteps_of(P.u32(seed, d["t"], B), T)
    N = B * C * H * W
    e = P.randn(seed, d["e"], N).reshape(shape) if e is None else np.asarray(e, dtype=np.float64).reshape(shape)
    n = P.randn(seed, d["n"], N).reshape(shape) if n is None else np.asarray(n, dtype=np.float64).reshape(shape)
    o = P.randn(seed, d["o"], B * C).reshape(B, C) if o is None else np.asarray(o, dtype=np.float64).reshape(B, C)
    if moments is not None:
        m = np.asarray(moments, dtype=np.float64).reshape(B, H, W, 2 * C).transpose(0, 3, 1, 2)       # NCHW [B, 2C, H, W]
        mean, logvar = m[:, :C], np.clip(m[:, C:], -30.0, 20.0)
        lat = (mean + np.exp(0.5 * logvar) * e) * float(scaling_factor)
    else:
        lat = np.asarray(latents, dtype=np.float64).reshape(shape)
    target = n + float(noise_offset) * o[:, :, None, None]
    a = abar[t][:, None, None, None]
    noisy = np.sqrt(a) * lat + np.sqrt(1.0 - a) * target
    nhwc = lambda x: np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    return dict(timesteps=t, e=e, n=n, o=o, target=nhwc(target), noisy=nhwc(noisy), next=d["next"])
