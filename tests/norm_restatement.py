"""Test helper: float64 restatements of the forward normalisations (csrc/norm.hip, the LayerNorm folded into the GEMMs and attention
blocks, the statistics tables the convolution epilogues hand over), written from the formulas and from the layouts documented in
ops.py (`QStats`, `conv(rowstats=)`, `pack_linear_ln`, `attach_lora`) and include/aldm_hip.h -- not from the kernels.

As in tests/bwd_restatement.py every op has an `exact` form (float64, nothing rounded) and a `rounded` form (one bf16 rounding at each
point where the CONTRACT rounds, with a comment naming the point); `check` / `accepts` / `r16` are bwd_restatement's.  Tensors are
channels-last, [B, HW, C] or [M, C], float64 holding bf16-representable inputs.

Draws: every normalisation strip -- an (image, group), or a row -- gets its own mean and its own scale from the two ladders below, so
that a kernel reading a neighbour's statistics, a neighbour's tile or a neighbour's quad computes something visibly different.

`mutant=` computes a deliberately wrong variant (host test only).  `design="onepass_f32"` restates the DESIGN of the handed-over
paths in numpy float32 -- per-tile partial (sum, sum of squares), folded, variance as q / n - mu * mu -- a reference computation of
what the documented arithmetic costs, not a mutant: it decides the ceiling of the mean ladder (tests/test_norm_restatement_host.py).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from bwd_restatement import F64, LOG2E, accepts, attention_fwd, bf16_input, check, pack_round, r16  # noqa: F401  (re-exported)

SCALES = (0.25, 1.0, 4.0)
MEANS = (0.0, 0.5, -0.5, 3.0, -3.0, 16.0, -16.0)            # in units of the strip's scale
MEAN_TOP = 16.0                                              # the contract ceiling of |mean| / std (last section)
EPS, EPS_BIG = 1e-5, 0.1                                     # EPS_BIG: comparable to the variance of a scale-0.25 strip, so that a
#                                                              misplaced or dropped eps is a visible error (at 1e-5 it is 8e-5 of rstd)

STAT_MUTANTS = ("neighbour", "n_pad", "unbiased", "eps_out", "eps_drop")


def ladder(n_outer, n_inner, top=MEAN_TOP):
    """-> (mean, scale), each [n_outer, n_inner].  Strip (o, i) takes rung (5 + i + 3 o) % 7 of MEANS and (i + o) % 3 of SCALES:
    neighbours along either axis always differ (steps of 1 and 3 modulo 7, of 1 modulo 3) and strip (0, 0) sits on the top rung."""
    o, i = torch.arange(n_outer).view(-1, 1), torch.arange(n_inner).view(1, -1)
    means = torch.tensor([math.copysign(top, m) if abs(m) == MEAN_TOP else m for m in MEANS], dtype=F64)   # `top`: the top rung itself
    return means[(5 + i + 3 * o) % 7], torch.tensor(SCALES, dtype=F64)[(i + o) % 3]


def _params(g, C):
    """fp32 gamma / beta that vary per CHANNEL (random, not periodic in the group width)."""
    return (1.0 + 0.3 * torch.randn(C, generator=g)).to(F64), (0.3 * torch.randn(C, generator=g)).to(F64)


def gn_draw(B, HW, C, groups, seed=0, top=MEAN_TOP):
    """-> x [B, HW, C], gamma [C], beta [C]: strip (image b, group g) is scale * (mean + randn) on its own rungs."""
    g = torch.Generator().manual_seed(seed + 7 * HW + 1000 * C + groups)
    mean, scale = ladder(B, groups, top)
    per = lambda t: t.repeat_interleave(C // groups, 1).view(B, 1, C)
    x = bf16_input(per(scale) * (per(mean) + torch.randn(B, HW, C, generator=g, dtype=F64)))
    return (x,) + _params(g, C)


def ln_draw(M, C, seed=1, top=MEAN_TOP):
    """-> x [M, C], gamma, beta: row r is scale * (mean + randn) on its own rungs."""
    g = torch.Generator().manual_seed(seed + 100 * C + M)
    mean, scale = ladder(M, 1, top)
    x = bf16_input(scale * (mean + torch.randn(M, C, generator=g, dtype=F64)))
    return (x,) + _params(g, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# statistics of normalisation strips
# ---------------------------------------------------------------------------------------------------------------------------------
def _finish_stats(a, q2c, n, eps, mutant=None, n_pad=None):
    """a = sum x, q2c = sum (x - a / n)^2 per strip -> (mean, rstd).  Mutants: "n_pad" counts n_pad elements (the kernel's padded
    strip), "unbiased" divides the squares by n - 1, "eps_out" adds eps to the root, "eps_drop" leaves it out."""
    mean = a / n
    var = q2c / n
    if mutant == "n_pad":
        q = q2c + n * mean * mean                            # sum x^2
        mean = a / n_pad
        var = q / n_pad - mean * mean
    if mutant == "unbiased":
        var = q2c / (n - 1)
    if mutant == "eps_out":
        return mean, 1.0 / (torch.sqrt(var) + eps)
    if mutant == "eps_drop":
        return mean, 1.0 / torch.sqrt(var)
    return mean, 1.0 / torch.sqrt(var + eps)


def _strip_stats(rows, eps, mutant=None, n_pad=None):
    """rows [S, n] -> (mean [S, 1], rstd [S, 1]), two-pass in float64."""
    n = rows.shape[1]
    a = rows.sum(1, keepdim=True)
    q2c = ((rows - a / n) ** 2).sum(1, keepdim=True)
    return _finish_stats(a, q2c, n, eps, mutant, n_pad)


# ---------------------------------------------------------------------------------------------------------------------------------
# the statistics tables of a convolution epilogue (ops.QStats / include/aldm_hip.h qstat_out, rowstat_out)
# ---------------------------------------------------------------------------------------------------------------------------------
class Tiling:
    """How a producer cut its output rows into M-tiles.  Generic launch: bm rows of the flattened [B * HW] row space per tile, a tile
    that runs into the next image puts that image's rows into slot 1.  Halo launch (tpi > 0): `tpi` image-aligned tiles per image of
    `pix` = (tile rows // OW) * OW pixels each, slot 0 only."""

    def __init__(self, bm=0, tpi=0, pix=0):
        self.bm, self.tpi, self.pix = bm, tpi, pix

    def entry_of_rows(self, B, HW, wholly_first=False):
        """-> (entry index = tile * 2 + slot of every row of [B * HW], number of tiles)"""
        row = torch.arange(B * HW)
        img = row // HW
        if self.tpi > 0:
            return (img * self.tpi + (row % HW) // self.pix) * 2, B * self.tpi
        t = row // self.bm
        slot = torch.zeros_like(t) if wholly_first else img - (t * self.bm) // HW
        return t * 2 + slot, (B * HW + self.bm - 1) // self.bm

    def image_of_entries(self, B, HW):
        """-> image of every entry [tiles * 2] as the consumer reads it: slot 0 = the image of the tile's first row, slot 1 = the next"""
        _, T = self.entry_of_rows(B, HW)
        t = torch.arange(T).repeat_interleave(2)
        slot = torch.arange(2).repeat(T)
        return (t // self.tpi if self.tpi > 0 else (t * self.bm) // HW + slot).clamp(max=B)   # (B: the unread slot 1 of a last tile)


def qstat_entries(x, tiling):
    """x [B, HW, C] -> (table [tiles, 2, C / 4, 2] float64 of (sum, sum of squares), magnitude [.., 2] of (sum |x|, sum x^2),
    count [tiles, 2] of the VALUES in an entry).  Entries with count 0 are never read by a consumer (uninitialised)."""
    B, HW, C = x.shape
    Q = C // 4
    xq = x.reshape(B * HW, Q, 4)
    idx, T = tiling.entry_of_rows(B, HW)
    vals = torch.stack([xq.sum(-1), (xq * xq).sum(-1), xq.abs().sum(-1)], -1)
    tab = torch.zeros(T * 2, Q, 3, dtype=F64).index_add_(0, idx, vals).view(T, 2, Q, 3)
    cnt = torch.zeros(T * 2, dtype=F64).index_add_(0, idx, torch.full((B * HW,), 4.0, dtype=F64)).view(T, 2)
    return tab[..., :2], torch.stack([tab[..., 2], tab[..., 1]], -1), cnt


def rowstat_entries(y, BN):
    """y [M, N] -> (table [M, N / BN, 2] of (sum, sum of squares) per row and N-tile, magnitude (sum |y|, sum y^2))."""
    M, N = y.shape
    ys = y.reshape(M, N // BN, BN)
    q = (ys * ys).sum(-1)
    return torch.stack([ys.sum(-1), q], -1), torch.stack([ys.abs().sum(-1), q], -1)


def table_bound(mag, n):
    """Any-order fp32 summation bound of n terms, (n - 1) 2^-24 sum |term|, per entry (derived, not measured: every summation tree of
    fp32 additions stays within it to first order; the squares of bf16 values are exact in fp32).  One missing or foreign pixel of a
    ladder draw exceeds it by orders of magnitude."""
    n = n if torch.is_tensor(n) else torch.tensor(float(n), dtype=F64)
    return (n - 1.0).clamp_min(1.0) * 2.0 ** -24 * mag


def table_ok(got, want, mag, n, read=None):
    """-> (ok, worst error / bound) over the entries a consumer reads."""
    got = got.detach().to("cpu").to(F64)
    bound = table_bound(mag, n)
    ratio = (got - want).abs() / bound.clamp_min(1e-300)
    if read is not None:
        ratio = ratio[read]
    if not bool(torch.isfinite(ratio).all()):
        return False, math.inf
    worst = float(ratio.max())
    return worst <= 1.0, worst


def check_table(got, want, mag, n, what, read=None):
    import conftest
    ok, worst = table_ok(got, want, mag, n, read)
    conftest.record(worst, what + " err/bound")
    assert ok, f"{what}: an entry is {worst:.4g} x its fp32 summation bound away from the float64 sum"


def _image_quad_sums(x, tiling, wholly_first=False, f32=False):
    """-> [B, C / 4, 2]: (sum, sum of squares) per image and quad as a consumer folds a producer's table.
    wholly_first (mutant): a tile that straddles two images is counted wholly into its first image.
    f32 (design): per-entry partials in numpy float32, folded in float32 in entry order."""
    B, HW, C = x.shape
    Q = C // 4
    idx, T = tiling.entry_of_rows(B, HW, wholly_first)
    img = tiling.image_of_entries(B, HW)
    if not f32:
        xq = x.reshape(B * HW, Q, 4)
        tab = torch.zeros(T * 2, Q, 2, dtype=F64).index_add_(0, idx, torch.stack([xq.sum(-1), (xq * xq).sum(-1)], -1))
        return torch.zeros(B + 1, Q, 2, dtype=F64).index_add_(0, img, tab)[:B]
    xq = x.reshape(B * HW, Q, 4).numpy().astype(np.float32)
    vals = np.stack([xq.sum(-1, dtype=np.float32), (xq * xq).sum(-1, dtype=np.float32)], -1)
    tab = np.zeros((T * 2, Q, 2), np.float32)
    np.add.at(tab, idx.numpy(), vals)                         # float32 accumulation, one row at a time
    out = np.zeros((B + 1, Q, 2), np.float32)
    np.add.at(out, img.numpy(), tab)
    return torch.from_numpy(out[:B])


def _onepass_f32(a, q, n, eps):
    """the documented fold: mu = a / n, rstd = 1 / sqrt(max(q / n - mu mu, 0) + eps), all float32"""
    a, q = a.numpy().astype(np.float32), q.numpy().astype(np.float32)
    n = np.float32(n)
    mu = a / n
    var = np.maximum(q / n - mu * mu, np.float32(0.0))
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps))
    return torch.from_numpy(mu.astype(np.float64)), torch.from_numpy(rstd.astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm(+SiLU) over one or two sources
# ---------------------------------------------------------------------------------------------------------------------------------
def groupnorm(x, gamma, beta, groups, eps, act=0, *, rounded=False, mutant=None, design=None, C1=None, tilings=None, n_pad=None):
    """act(F.group_norm(cat(sources))) on x [B, HW, C] = the concatenation, C1 channels from the first source.
    tilings: one Tiling per source (handed-over statistics: the straddle mutant and the one-pass design need them).
    mutants: STAT_MUTANTS ("neighbour" = the next image's statistics), "straddle_first", "quad_off" (the share the group that
    straddles the concatenation takes from the second source, read one quad further on), "gamma_in_group" (gamma / beta indexed
    within the group), "silu_first" (SiLU before the affine)."""
    B, HW, C = x.shape
    Cg = C // groups
    n = HW * Cg
    C1 = C if C1 is None else C1
    xs = x
    if mutant == "quad_off":
        assert C1 < C and C1 % Cg, "no group straddles the concatenation"
        lo, hi = C1, (C1 // Cg + 1) * Cg                      # the straddling group's share of the second source ...
        xs = x.clone()
        xs[..., lo:hi] = x[..., lo + 4:hi + 4]                # ... read one quad further on
    if design == "onepass_f32" or mutant == "straddle_first":
        parts = [_image_quad_sums(s.contiguous(), t, mutant == "straddle_first", design == "onepass_f32")
                 for s, t in zip((xs[..., :C1], xs[..., C1:]) if C1 < C else (xs,), tilings)]
        qs = torch.cat(parts, 1).view(B, groups, Cg // 4, 2)
        if design == "onepass_f32":
            acc = np.zeros((B, groups, 2), np.float32)
            for k in range(Cg // 4):                          # the group's quads, added in float32
                acc += qs[:, :, k].numpy()
            mean, rstd = _onepass_f32(torch.from_numpy(acc[..., 0]), torch.from_numpy(acc[..., 1]), n, eps)
        else:
            a, q = qs[..., 0].sum(2), qs[..., 1].sum(2)
            mean = a / n
            rstd = 1.0 / torch.sqrt(q / n - mean * mean + eps)
    else:
        rows = xs.view(B, HW, groups, Cg).permute(0, 2, 1, 3).reshape(B * groups, n)
        mean, rstd = _strip_stats(rows, eps, mutant if mutant in STAT_MUTANTS else None, n_pad)
        mean, rstd = mean.view(B, groups), rstd.view(B, groups)
    if mutant == "neighbour":
        assert B > 1
        mean, rstd = torch.roll(mean, -1, 0), torch.roll(rstd, -1, 0)
    gm, bt = gamma, beta
    if mutant == "gamma_in_group":
        gm, bt = gamma[:Cg].repeat(groups), beta[:Cg].repeat(groups)
    xh = ((x.view(B, HW, groups, Cg) - mean.view(B, 1, groups, 1)) * rstd.view(B, 1, groups, 1)).view(B, HW, C)
    if mutant == "silu_first":
        assert act
        y = F.silu(xh) * gm + bt
    else:
        y = xh * gm + bt
        if act:
            y = F.silu(y)
    return r16(y) if rounded else y                           # every GroupNorm kernel: `o[k] = (bf16)t`, the one rounding of the op


def gn_n_pad(HW, Cg):
    """the element count of a strip padded to whole 512-thread rounds of quads (what a kernel that forgot its tail mask would count)"""
    nq = HW * (Cg // 4)
    return (nq + 511) // 512 * 512 * 4


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm, embedding LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------
def layernorm(x, gamma, beta, eps, *, rounded=False, mutant=None, n_pad=None):
    """F.layer_norm over the rows of x [M, C].  mutants: STAT_MUTANTS ("neighbour" = the next row's statistics)."""
    mean, rstd = _strip_stats(x, eps, mutant if mutant in STAT_MUTANTS else None, n_pad)
    if mutant == "neighbour":
        assert x.shape[0] > 1
        mean, rstd = torch.roll(mean, -1, 0), torch.roll(rstd, -1, 0)
    y = (x - mean) * rstd * gamma + beta
    return r16(y) if rounded else y                           # layernorm_kernel: `o[k] = (bf16)((v - mean) * rstd * g + b)`


def ln_n_pad(C):
    """a row padded to the 8-channel chunks of all its lanes: 32 lanes up to 256 channels, 64 beyond (4 chunks per lane at most)"""
    lanes = 32 if C <= 256 else 64
    return (C // 8 + lanes - 1) // lanes * lanes * 8


def position_ids(ids, pad, mutant=None):
    """RoBERTa's rule: pad + (number of non-pad tokens up to and including this one) for a token, pad for a pad.
    mutant "pos_plain": pad + 1 + index, pads counted."""
    mask = ids != pad
    if mutant == "pos_plain":
        return (pad + 1 + torch.arange(ids.shape[1])).expand_as(ids).clone()
    return pad + torch.where(mask, torch.cumsum(mask.to(torch.int64), 1), torch.zeros_like(ids))


def embed_layernorm(ids, word, pos, type0, gamma, beta, eps, pad, *, rounded=False, mutant=None):
    """LayerNorm(word[ids] + type0 + pos[position_ids]) -> [B * L, C]; the tables are fp32 and the sum is not rounded to bf16."""
    B, L = ids.shape
    e = word[ids] + type0 + pos[position_ids(ids, pad, mutant)]
    return layernorm(e.view(B * L, -1), gamma, beta, eps, rounded=rounded, mutant=None if mutant == "pos_plain" else mutant)


def embed_draw(B, L, C, pad=1, seed=2, top=MEAN_TOP):
    """A vocabulary whose every row has its own ladder statistics; ids walk through it so that neighbouring tokens differ.  Row 0 of
    the batch has pads INSIDE the sequence, the last row is all pads."""
    g = torch.Generator().manual_seed(seed + L + C)
    V = 23
    mean, scale = ladder(V, 1, top)
    word = (scale * (mean + torch.randn(V, C, generator=g, dtype=F64))).float().to(F64)
    pos = (0.1 * torch.randn(L + pad + 2, C, generator=g, dtype=F64)).float().to(F64)
    type0 = (0.1 * torch.randn(C, generator=g, dtype=F64)).float().to(F64)
    ids = (2 + (torch.arange(L).view(1, L) * 5 + torch.arange(B).view(B, 1) * 3) % (V - 2)).to(torch.int64)
    ids[0, 2::7] = pad
    ids[0, L - 3:] = pad
    ids[B - 1, :] = pad
    return (ids, word, pos, type0) + _params(g, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# Linear over a folded LayerNorm (ops.pack_linear_ln, ops.attach_lora)
#   LN(x) W^T + b = rstd (x W'^T - mean s) + c,  W' = bf16(W diag(gamma)),  s = row sums of the ROUNDED W',  c = W beta + b
#   LoRA on LN(x): A' = bf16(A diag(gamma)), sA = row sums of A', cA = A beta;  T'' = x A'^T - mean sA + cA / rstd joins the
#   accumulator as T'' (sB)^T, sB = bf16(scaling B), and takes the epilogue's rstd (. - mean s) + c with it.
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_linear(x, W, bias, gamma, beta, eps, parts=(), *, rounded=False, mutant=None, design=None, nparts=None):
    """x [M, K], W [N, K] (bf16-representable), bias fp32 or None, parts [(row0, nrows, A [r, K], B [nrows, r], scaling)] fp32.
    exact: the operation itself, float64.  rounded: the fold, with bf16 at the pack, at T'' and at the output.
    mutants: STAT_MUTANTS, "s_unrounded" (s summed from the unrounded W diag(gamma)), "t_round_first" (T rounded to bf16 BEFORE the
    mean correction).  design "onepass_f32": the statistics from `nparts` float32 partial pairs per row, q / K - mu mu."""
    M, K = x.shape
    b = bias if bias is not None else torch.zeros(W.shape[0], dtype=F64)
    if design == "onepass_f32":
        xs = x.numpy().astype(np.float32).reshape(M, nparts, K // nparts)
        pa, pq = xs.sum(-1, dtype=np.float32), (xs * xs).sum(-1, dtype=np.float32)
        a, q = np.zeros(M, np.float32), np.zeros(M, np.float32)
        for j in range(nparts):
            a += pa[:, j]
            q += pq[:, j]
        mean, rstd = _onepass_f32(torch.from_numpy(a), torch.from_numpy(q), K, eps)
        mean, rstd = mean.view(M, 1), rstd.view(M, 1)
    else:
        mean, rstd = _strip_stats(x, eps, mutant if mutant in STAT_MUTANTS else None, ln_n_pad(K))
    if mutant == "neighbour":
        mean, rstd = torch.roll(mean, -1, 0), torch.roll(rstd, -1, 0)
    if not rounded and mutant is None and design is None:
        xn = (x - mean) * rstd * gamma + beta
        y = xn @ W.t() + b
        for row0, nrows, A, Bm, s in parts:
            y[:, row0:row0 + nrows] += s * (xn @ A.to(F64).t()) @ Bm.to(F64).t()
        return y
    Wg = W * gamma
    Wp = r16(Wg)                                              # pack_linear_ln: `wp = (w * g[None, :]).to(torch.bfloat16)`
    s_ = (Wg if mutant == "s_unrounded" else Wp).sum(1)       # pack_linear_ln: `s = wp.float().sum(1)` -- of the ROUNDED rows
    c = W @ beta + b
    acc = x @ Wp.t()
    for row0, nrows, A, Bm, s in parts:
        A64 = A.to(F64)
        Ap = r16(A64 * gamma)                                 # attach_lora: `Ap = (Af * ln[0][None, :]).to(torch.bfloat16)`
        sA, cA = Ap.sum(1), A64 @ beta
        t = x @ Ap.t()
        if mutant == "t_round_first":
            t = r16(t)
        T = r16(t - mean * sA + cA / rstd)                    # the GEMM's LoRA stage: T'' goes to the MFMA as bf16
        sB = pack_round(Bm, s)                                # attach_lora: `(Bm.float() * s).to(torch.bfloat16)`
        acc[:, row0:row0 + nrows] += T @ sB.t()
    return r16(rstd * (acc - mean * s_) + c)                  # the GEMM epilogue's bf16 store


def ln_linear_draw(M, K, N, r, seed=3, top=MEAN_TOP, nparts=3):
    """Rows with ladder statistics; a LoRA term of the size of the base term, so that an error in T shows in y."""
    g = torch.Generator().manual_seed(seed + M + 10 * K + N)
    x, gamma, beta = ln_draw(M, K, seed + 50, top)
    W = bf16_input(torch.randn(N, K, generator=g, dtype=F64) / math.sqrt(K))
    bias = torch.randn(N, generator=g).to(F64)
    parts = []
    if r:
        nrows = N // nparts
        for i in range(nparts):
            A = (torch.randn(r, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).float()
            Bm = (torch.randn(nrows, r, generator=g) / math.sqrt(r)).to(torch.bfloat16).float()
            parts.append((i * nrows, nrows, A, Bm, 1.0 + 0.5 * i))
    return x, W, bias, gamma, beta, parts


def attn_block(x, W, gamma, beta, eps, parts, B, N, H, d, rounded=False, **kw):
    """The fused attention block: q | k | v = ln_linear(x) with W = (Wq * log2(e) / sqrt(d) | Wk | Wv), then softmax(q k^T) v per
    (sample, head) -- composed with bwd_restatement.attention_fwd, which applies the scale itself, so q is handed over unscaled.
    kw: ln_linear's mutant= / design= / nparts= (they enter through the projection; the attention is always the float64 one)."""
    qkv = ln_linear(x, W, None, gamma, beta, eps, parts, rounded=rounded, **kw)
    qkv[:, :H * d] /= LOG2E / math.sqrt(d)
    return attention_fwd(qkv, B, N, H, d, rounded=rounded)[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# consumers of a GroupNorm that end in a convolution
# ---------------------------------------------------------------------------------------------------------------------------------
def conv3x3(a, H, W, w, bias):
    """a [B, HW, C] channels-last -> [B, HW, Cout]: 3x3 / pad 1, float64.  w [Cout, C, 3, 3]."""
    B, HW, C = a.shape
    y = F.conv2d(a.view(B, H, W, C).permute(0, 3, 1, 2), w, bias, padding=1)
    return y.permute(0, 2, 3, 1).reshape(B, HW, -1)


def gn_conv(x, gamma, beta, groups, eps, H, W, w, bias, extra=None, *, rounded=False, out_bf16=True, **kw):
    """conv3x3(SiLU(GroupNorm(x))) (+ extra): the norm applied on the way into the consuming convolution.
    rounded: the activation is bf16 where the MFMA reads it; the output is bf16 (conv(gn_in=)) or fp32 (gn_silu_conv_out)."""
    a = groupnorm(x, gamma, beta, groups, eps, 1, rounded=rounded, **kw)    # rounded: `(bf16)silu_f(fmaf(v, sc, sh))` into LDS
    y = conv3x3(a, H, W, w, bias)
    if extra is not None:
        y = y + extra
    return r16(y) if (rounded and out_bf16) else y            # conv(gn_in=): the standard bf16 epilogue


def identity_weight(C, k):
    """[C, C, k, k]: the identity at the centre tap -- the convolution stores its input bit for bit"""
    w = torch.zeros(C, C, k, k)
    w[torch.arange(C), torch.arange(C), k // 2, k // 2] = 1.0
    return w


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch arithmetic (asserted by the GPU tests: every case names the arm it is there for)
# ---------------------------------------------------------------------------------------------------------------------------------
def gn_arm(HW, C, groups):
    """aldm_groupnorm: the register-strip kernel of 4 / 8 / 16 / 32 quads per thread (512 threads, groups of <= 256 channels), else
    groupnorm_kernel, LDS-cached up to 16384 quads, streaming beyond."""
    Cg = C // groups
    nq = HW * (Cg // 4)
    if Cg <= 256:
        for qpt in (4, 8, 16, 32):
            if nq <= qpt * 512:
                return f"reg{qpt}"
    return "lds" if nq <= 16384 else "stream"


def partials_arm(HW, Ct, groups):
    nq = HW * (Ct // groups // 4)
    return next(qpt for qpt in (1, 2, 4, 8) if nq <= qpt * 512)


def apply_lpg(groups):
    lpg = 1
    while lpg * 2 * groups <= 256 and lpg < 64:
        lpg *= 2
    return lpg


def apply_pxb(C):
    pxb = 16
    while pxb < 256 and pxb * C * 2 < 32768:
        pxb *= 2
    return pxb


def apply_tiles(HW, tilings):
    return max(t.tpi if t.tpi > 0 else HW // t.bm + 1 for t in tilings)


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_norm_edges.py (shared with the host test, which proves the comparator sharp AT these shapes)
# ---------------------------------------------------------------------------------------------------------------------------------
# aldm_groupnorm: (B, HW, C, groups, C1, act, eps, arm).  One quad per pixel (C = 8, 2 groups): every QPT boundary from both sides.
GN_CASES = [
    (2, 2048, 8, 2, 8, 1, EPS, "reg4"), (2, 2049, 8, 2, 8, 0, EPS, "reg8"), (2, 4096, 8, 2, 8, 0, EPS_BIG, "reg8"),
    (2, 4097, 8, 2, 8, 1, EPS, "reg16"), (2, 8192, 8, 2, 8, 1, EPS, "reg16"), (2, 8193, 8, 2, 8, 0, EPS, "reg32"),
    (2, 16384, 8, 2, 8, 0, EPS, "reg32"), (2, 16385, 8, 2, 8, 1, EPS, "stream"),
    (2, 410, 40, 2, 40, 1, EPS, "reg8"),                      # Cg = 20: five quads per pixel, 2050 quads
    (2, 63, 520, 2, 520, 1, EPS, "lds"),                      # Cg = 260 > 256: groupnorm_kernel, 4095 quads in LDS
    (2, 253, 520, 2, 520, 0, EPS_BIG, "stream"),              # 16445 quads: the streaming form
    # two sources whose split falls inside group 0 (Cg = 8: 4 channels from each), once per arm
    (2, 1000, 16, 2, 4, 1, EPS, "reg4"), (2, 2000, 16, 2, 4, 0, EPS, "reg8"), (2, 4000, 16, 2, 4, 1, EPS_BIG, "reg16"),
    (2, 8000, 16, 2, 4, 0, EPS, "reg32"), (2, 8200, 16, 2, 4, 1, EPS, "stream"),
    (2, 63, 520, 2, 256, 0, EPS, "lds"),                      # group 0 = 256 channels of x + 4 of x2
]
LN_CS, LN_MS = (8, 248, 256, 264, 640, 2048), (1, 7, 8, 9, 33)
LN_BAD_CS = (2056, 12)
EMBED_CASES = [(3, 130, 768), (2, 9, 64)]                     # (B, L, C)

# aldm_groupnorm_apply over identity producers: (name, B, H, W, C1, C2, groups, tile1, tile2, act, eps).  tile2: the 1x1 producer of x2.
APPLY_CASES = [
    ("straddle", 3, 130, 16, 128, 0, 32, 2, 0, 1, EPS),       # HW = 2080, bm = 64: tiles cross both image boundaries (slot 1)
    ("halo7", 2, 131, 16, 128, 0, 32, 7, 0, 1, EPS_BIG),      # image-aligned tiles, a ragged last tile
    ("halo8", 2, 131, 16, 128, 0, 32, 8, 0, 0, EPS),
    ("concat", 3, 130, 16, 256, 128, 32, 4, 2, 1, EPS),       # Cg = 12: group 21 = channels 252..255 of x and 0..7 of x2
    ("tiles95", 2, 376, 16, 64, 0, 8, 2, 0, 1, EPS),          # 6016 / 64 + 1 = 95 tiles: statistics summed by every workgroup
    ("tiles96", 2, 380, 16, 64, 0, 8, 2, 0, 1, EPS),          # 96: the finalize launch
    ("tiles95x2", 2, 376, 16, 64, 64, 8, 2, 2, 0, EPS),
    ("tiles96x2", 2, 380, 16, 64, 64, 8, 2, 2, 0, EPS),
    ("g64", 2, 130, 16, 256, 0, 64, 4, 0, 1, EPS),            # lpg 4
    ("g1", 3, 130, 16, 64, 0, 1, 2, 0, 1, EPS),               # lpg 64; C = 64: pxb 256, HW % 256 = 32
    ("c2048", 2, 257, 8, 2048, 0, 32, 4, 0, 0, EPS),          # 1x1 producer; pxb 16, HW % 16 = 8
]
TILE_ROWS = {1: 128, 2: 64, 3: 128, 4: 64, 6: 128, 7: 128, 8: 64, 9: 256, 10: 64, 11: 128, 12: 256, 13: 64, 14: 128, 15: 128, 16: 64}
HALO_TILES = (7, 8, 15, 16)


def tiling_for(tile, B, H, W):
    """the Tiling conv(qstats=True) documents for this tile (ops.QStats: bm for generic tiles, tpi for the image-aligned halo tiles)"""
    rows = TILE_ROWS[tile]
    if tile in HALO_TILES:
        return Tiling(0, -(-H // (rows // W)), (rows // W) * W)
    return Tiling(rows, 0, 0)


def apply_draw(case, top=MEAN_TOP):
    name, B, H, W, C1, C2, groups, t1, t2, act, eps = case
    x, gamma, beta = gn_draw(B, H * W, C1 + C2, groups, seed=11, top=top)
    tilings = [tiling_for(t1, B, H, W)] + ([tiling_for(t2, B, H, W)] if C2 else [])
    return x, gamma, beta, tilings


# aldm_groupnorm_partials through conv(gn=) / conv(defer=): Cout = 64, 16 groups (one quad per pixel): (H, W) with HW on both sides of
# every template boundary (512 / 1024 / 2048 quads) and the 4096-quad maximum
PARTIALS_HW = [(32, 16), (27, 19), (64, 16), (41, 25), (128, 16), (683, 3), (256, 16)]


def partials_draw(H, W):
    """Inputs of one aldm_groupnorm_partials case (B = 2): a 128-channel ladder draw in 32 groups whose first 64 channels go through the
    (identity-weight, split-K) convolution and whose last 64 are the skip tensor; bias, row bias [B, 72] (read from column 8), residual.
    -> dict with the three float64 sums h the norm sees: "rowbias", "res" (64 channels, 16 groups) and "cat" (128 channels, 32 groups)."""
    B, C, HW = 2, 64, H * W
    g = torch.Generator().manual_seed(HW)
    x, gamma, beta = gn_draw(B, HW, 2 * C, 32, seed=13)
    xc, skip = x[..., :C].contiguous(), x[..., C:].contiguous()
    bias = torch.randn(C, generator=g)
    rb = torch.randn(B, C + 8, generator=g)
    res = bf16_input(torch.randn(B, HW, C, generator=g, dtype=F64))
    hb = xc + bias.to(F64)
    return dict(xc=xc, skip=skip, bias=bias, rb=rb, res=res, gamma=gamma, beta=beta, h_plain=hb,
                h_rowbias=hb + rb[:, None, 8:].to(F64), h_res=hb + res, h_cat=torch.cat([hb, skip], -1))


def consumer_draw():
    """Inputs of the consumers that end in a convolution (aldm_gn_silu_conv3x3_small, conv(gn_in=)): a 3 x 131 x 16 x 128 ladder draw in
    32 groups, the 8-channel fp32-output filter of the first, the 128-channel filter, row bias and residual of the second."""
    B, H, W, C, groups, N = 3, 131, 16, 128, 32, 128
    x, gamma, beta = gn_draw(B, H * W, C, groups, seed=11)
    g = torch.Generator().manual_seed(6)
    w8 = bf16_input(torch.randn(8, C, 3, 3, generator=g, dtype=F64) * 0.05)
    b8 = torch.randn(8, generator=g)
    g = torch.Generator().manual_seed(7)
    w = bf16_input(torch.randn(N, C, 3, 3, generator=g, dtype=F64) * 0.03)
    b = torch.randn(N, generator=g)
    rb = torch.randn(B, N, generator=g)
    res = bf16_input(torch.randn(B, H * W, N, generator=g, dtype=F64))
    return dict(B=B, H=H, W=W, C=C, groups=groups, N=N, x=x, gamma=gamma, beta=beta, w8=w8, b8=b8, w=w, b=b, rb=rb, res=res,
                extra=rb[:, None, :].to(F64) + res)


CONSUMER_PTILES = (2, 7)                                      # the producers of the consumers' input: a generic and a halo tile
RANDOM_PRODUCER_TILES = (2, 7)


def random_producer_draw():
    """The random-weight producer (one per tile family): a 64 -> 128 channel 3x3 convolution over 3 x 130 x 16 whose bias gives every
    group its own mean (ladder rungs, half a unit of the convolution's spread per unit) -> xin, w, bias, gamma, beta."""
    B, H, W, Cin, C, groups = 3, 130, 16, 64, 128, 32
    g = torch.Generator().manual_seed(5)
    xin = bf16_input(torch.randn(B, H * W, Cin, generator=g, dtype=F64))
    w = bf16_input((torch.randn(C, Cin, 3, 3, generator=g) * 0.06).to(F64))
    mean, scale = ladder(1, groups)
    bias = (mean * scale * 0.5).repeat_interleave(C // groups, 1).view(C).float()
    _, gamma, beta = gn_draw(1, 1, C, groups)
    return dict(B=B, H=H, W=W, C=C, groups=groups, xin=xin, w=w, bias=bias, gamma=gamma, beta=beta)


# folded LayerNorm: (route, M, K, N, r)
# pgemm_vt: the q | k | v projection of 2 x 35 tokens with the V columns stored token-major -- the LayerNorm-folded form aldm_pgemm has with
# LoRA; a plain LayerNorm-folded linear at a pgemm width (K = 256) has no pgemm instantiation and must run on aldm_igemm.
LNLIN_CASES = [("igemm_own", 70, 256, 192, 4), ("igemm_parts", 130, 128, 192, 4), ("igemm_parts", 70, 256, 192, 4),
               ("igemm_own", 130, 640, 192, 0), ("pgemm_vt", 70, 256, 768, 4)]
ATTN64_NS, ATTN256_NS = (40, 64), (17, 252)
