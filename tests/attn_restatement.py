"""Test helper: float64 restatements of the INFERENCE forms of the attention core -- ops.attention(prescaled=True), ops.attention(kv_len=),
ops.attention(fp8=True) and ops.attention_wide -- written from the formulas and the operand layouts of the two docstrings, not from
the kernels.  (The training forward, aldm_attention_lse, is bwd_restatement.attention_fwd and stays there.)

One body gives two results on the same bf16-representable inputs:

  exact    sum_k 2^(s - m) v_k / sum_k 2^(s - m) over the keys < Nk, Nk = max(1, min(kv_len[b], N)) (N without kv_len), in float64;
  rounded  the same arithmetic with a rounding at exactly the points where the kernel's CONTRACT rounds; each point carries a
           comment naming the kernel line it stands for.

`q` is "as handed over": for the prescaled, fp8-prescaled and wide forms it already carries d^-0.5 log2(e) and nothing is multiplied
here; for the kv_len and the non-prescaled fp8 form it is unscaled and the factor is applied here.

Two comparators.  bf16 forms: `check_elem`, a per-element bound with nothing measured in it (last section), and
bwd_restatement.check (2 x the L2 floor, 4 x the max floor).  fp8 form: `check` alone, against the e4m3 floor.

The value of these tests is in the DRAWS as much as in the comparator (a key admitted with score 0 weighs 1 / N on random scores
and is invisible; with every true score near -8 log2 units it outweighs the real keys): `draw()` has diffuse, negative, edge-key and
staircase / descending draws and, for fp8, a tail draw, all deterministic per (shape, seed).  A `mutant=` argument computes a deliberately wrong variant (host test only)."""
import math
from collections import namedtuple
from functools import lru_cache

import torch

from bwd_restatement import F64, LOG2E, _heads, _rows, accepts, bf16_input, check, floor_ratios, l_sums_rounded_p, r16  # noqa: F401
from conv_restatement import half_ulp_bf16

KV = 64                 # keys per tile, attention.hip
KT_WIDE = 32            # keys per tile, attention_wide.hip
RESCALE_THR = 5.0       # log2 units over the running maximum before it is raised (both kernels)
PBIAS = 8.0             # log2 of the factor P carries into its e4m3 conversion
N_CONST = 16            # see bound()

MUTANTS = ("phantom", "drop_last", "kslot", "l_not_rescaled", "no_reshift", "merge_swapped", "alpha_tile0", "fp8_no_bias")
BF16_FORMS = ("prescaled", "varlen", "wide")
FP8_FORMS = ("fp8", "fp8p")


def cdiv(a, b):
    return (a + b - 1) // b


def r8(x):
    """Round to OCP e4m3 (nearest even, subnormals kept), back in float64.  Every argument here is far below 448."""
    return x.to(torch.float32).to(torch.float8_e4m3fn).to(F64)


def padded_d(d, form="prescaled"):
    return d if form == "wide" else next(p for p in (16, 32, 48, 64, 80) if d <= p)


def q_carries_scale(form):
    return form in ("prescaled", "fp8p", "wide")


def score_factor(form, d):
    """What the restatement multiplies q k^T by: 1 where q was handed over pre-scaled."""
    return 1.0 if q_carries_scale(form) else LOG2E / math.sqrt(d)


# ---------------------------------------------------------------------------------------------------------------------------------
# launch arithmetic restated (the GPU test asserts it per case)
# ---------------------------------------------------------------------------------------------------------------------------------
def arm(N, H, B):
    """launch_attn_d's rule: (waves, key groups)."""
    if N < 64:
        return 1, 1
    if N < 192:
        return 4, 1
    if N < 768:
        return 4, 2
    return (8, 1) if cdiv(N, 256) * H * B >= 256 else (8, 2)


def wide_qt(N, B):
    """aldm_attention_wide: two query tiles per wave once that still fills the chip."""
    return 2 if cdiv(N, 128) * B >= 192 else 1


def remap_on(B, H):
    """attention_kernel's XCD pair remap: only when the (batch, head) pairs divide over the 8 XCDs."""
    return (B * H) % 8 == 0


Geo = namedtuple("Geo", "kt sp wave_rows wg_rows")


def geometry(form, B, H, N):
    """Key tile, key groups, the rows that share one wave-uniform rescale decision, and the query rows per workgroup."""
    if form == "wide":
        return Geo(KT_WIDE, 1, 16, 64 * wide_qt(N, B))
    nw, sp = arm(N, H, B)
    return Geo(KV, sp, 32, 32 * nw // sp)


def clamp_len(n, N):
    return max(1, min(int(n), N))


def edge_set(Nk, geo):
    """0, 31, 32, 63, 64, Nk - 1, Nk - 2 and the first and last key of each key group's last tile (wide: 32-key tiles, so 0, 15, 16,
    31, 32, ...)."""
    h = geo.kt // 2
    keys = [0, h - 1, h, geo.kt - 1, geo.kt, Nk - 1, Nk - 2]
    ntiles = cdiv(Nk, geo.kt)
    for g in range(geo.sp):
        mine = list(range(g, ntiles, geo.sp))
        if mine:
            keys += [mine[-1] * geo.kt, min(mine[-1] * geo.kt + geo.kt - 1, Nk - 1)]
    return sorted({e for e in keys if 0 <= e < Nk})


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _structural(s, v, mutant):
    """Mutants 1 - 3 change which keys enter, or which V row a probability meets; they act on (scores, V) before any softmax."""
    if mutant == "phantom":                                       # key Nk read as a zero K row and a zero V column
        s = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
        v = torch.cat([v, torch.zeros_like(v[:, :1])], 1)
    elif mutant == "drop_last":                                   # key Nk - 1 masked
        s, v = s[..., :-1], v[:, :-1]
    elif mutant == "kslot":                                       # V rows of keys 4..7 and 8..11 of every 16 exchanged
        Nk = s.shape[-1]
        Lp = cdiv(Nk, 16) * 16
        s = torch.cat([s, torch.full(s.shape[:-1] + (Lp - Nk,), -math.inf, dtype=F64)], -1)
        vp = torch.cat([v, torch.zeros(v.shape[0], Lp - Nk, v.shape[2], dtype=F64)], 1)
        idx = torch.arange(Lp).view(-1, 16)[:, [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]].reshape(-1)
        v = vp[:, idx]
    return s, v


def _row_max(s, v, rounded, ones_l):
    """bf16 forms, P referred to the row maximum.  s [H, N, Nk] in log2 units, v [H, Nk, d]."""
    m = s.max(-1, keepdim=True)[0]
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    if rounded:
        p = r16(p)                                                # attention_kernel: `pf[s2][i] = (bf16)p0` / wide: `pf[u][sub * 4 + j] = (bf16)...exp2f(...)`
        if ones_l:
            l = p.sum(-1, keepdim=True)                           # attention_kernel: l = row DP of O^T (the row of ones of V^T); wide: `o[u][DTL - 1][0]`
    return (p @ v) / l                                            # (VL head dims: `l_pk += f32x2{p0, p1}`, the fp32 probabilities)


def _online(s, v, geo, thr, quant, bias, ones_l, mutant=None):
    """The tile-by-tile form: per key group a running maximum that is raised, for all rows of a wave together, when one of them
    exceeds it by more than `thr` (fp8: thr = 0, so every row tracks its maximum exactly); P of a tile is quantised against the
    maximum in force at that tile, earlier tiles are rescaled in float64; the key groups are merged at the end.
    -> (out [H, N, d], ex [H, N, tiles]: the excess of every non-first tile over the running maximum it met, NaN for first tiles)."""
    H, N, Nk = s.shape
    kt, sp, wr = geo.kt, geo.sp, geo.wave_rows
    ntiles, Np = cdiv(Nk, kt), cdiv(N, wr) * wr
    ex_all = torch.full((H, N, ntiles), math.nan, dtype=F64)
    rows = torch.arange(N)
    second = (rows % 32) >= 16
    groups = []
    for g in range(sp):
        m = O = l = None
        for j, t in enumerate(range(g, ntiles, sp)):
            st, vt = s[..., t * kt:(t + 1) * kt], v[:, t * kt:(t + 1) * kt]
            mx = st.max(-1)[0]
            if j == 0:
                m, O, l = mx.clone(), torch.zeros(H, N, v.shape[2], dtype=F64), torch.zeros(H, N, dtype=F64)
                ref = m
            else:
                ex = mx - m
                ex_all[..., t] = ex
                over = torch.zeros(H, Np, dtype=torch.bool)
                over[:, :N] = ex > thr
                trig = over.view(H, Np // wr, wr).any(-1, keepdim=True).expand(H, Np // wr, wr).reshape(H, Np)[:, :N]
                delta = torch.where(trig, ex.clamp_min(0.0), torch.zeros_like(ex))    # `delta = fmaxf(ex, 0.f)` in every lane of the wave
                alpha = torch.exp2(-delta)
                if mutant == "alpha_tile0":                       # the second 16-row tile of a wave rescaled by the first tile's alpha
                    a2 = alpha.clone()
                    a2[:, second] = alpha[:, rows[second] - 16]
                    alpha = a2
                O = O * alpha.unsqueeze(-1)
                if mutant != "l_not_rescaled":
                    l = l * alpha
                ref = m if mutant == "no_reshift" else m + delta  # the maximum this tile's scores are referred to
                m = m + delta
            p = torch.exp2(st - ref.unsqueeze(-1) + bias)
            P = quant(p)                                          # fp8: `__builtin_amdgcn_cvt_pk_fp8_f32(P0, P1, ...)` of p x 2^8
            O = O + P @ vt
            l = l + (P if ones_l else p).sum(-1)
        if m is not None:
            groups.append((m, O, l))
    m0, O0, l0 = groups[0]
    for m1, O1, l1 in groups[1:]:                                 # the key groups' merge
        mn = torch.maximum(m0, m1)
        a0, a1 = torch.exp2(m0 - mn), torch.exp2(m1 - mn)
        O0 = O0 * a0.unsqueeze(-1) + O1 * a1.unsqueeze(-1)
        l0 = l0 * a0 + l1 * (a0 if mutant == "merge_swapped" else a1)
        m0 = mn
    return O0 / l0.unsqueeze(-1), ex_all


def _scores(q, k, v, form, b, Nk, rounded):
    d = q.shape[-1]
    qb, kb, vb = q[b], k[b][:, :Nk], v[b][:, :Nk]
    if rounded and form in FP8_FORMS:
        qb, kb, vb = r8(qb), r8(kb), r8(vb)                       # attention_kernel: `bf16x8_to_fp8(qv)`, stage_k / stage_v `bf16x8_to_fp8(...)`
    return (qb @ kb.transpose(-1, -2)) * score_factor(form, d), vb


def attention(q, k, v, form, lens=None, rounded=False, mutant=None, geo=None):
    """q, k, v [B, H, N, d] float64 (bf16-representable) -> [B * N, H * d].  lens: the kv_len the kernel receives (unclamped)."""
    B, H, N, d = q.shape
    geo = geo or geometry(form, B, H, N)
    ones_l = True if form == "wide" else l_sums_rounded_p(d)
    outs = []
    for b in range(B):
        Nk = clamp_len(lens[b], N) if lens is not None else N
        s, vb = _scores(q, k, v, form, b, Nk, rounded or mutant is not None)
        s, vb = _structural(s, vb, mutant)
        if s.shape[-1] == 0:
            outs.append(torch.full((H, N, d), math.nan, dtype=F64))
            continue
        if form in FP8_FORMS:
            if rounded or mutant is not None:
                o, _ = _online(s, vb, geo, 0.0, r8, 0.0 if mutant == "fp8_no_bias" else PBIAS, ones_l, mutant)
            else:
                o = _row_max(s, vb, False, False)
        elif mutant in ("l_not_rescaled", "no_reshift", "merge_swapped", "alpha_tile0", "online"):
            o, _ = _online(s, vb, geo, RESCALE_THR, r16, 0.0, ones_l, mutant)
        else:
            o = _row_max(s, vb, rounded or mutant is not None, ones_l)
        outs.append(r16(o) if (rounded or mutant is not None) else o)     # `(bf16)(o[t][4 * g] * inv)` / wide `(bf16)(o[u][t][0] * inv)`
    return _rows(torch.stack(outs))


def rescale_trace(q, k, v, form, lens=None, geo=None):
    """-> ex [B, H, N, tiles]: every non-first tile's excess over the running maximum the kernel's rule gives it (NaN: first tiles
    and tiles past Nk).  ex > RESCALE_THR is a raise."""
    B, H, N, d = q.shape
    geo = geo or geometry(form, B, H, N)
    out = torch.full((B, H, N, cdiv(N, geo.kt)), math.nan, dtype=F64)
    for b in range(B):
        Nk = clamp_len(lens[b], N) if lens is not None else N
        s, vb = _scores(q, k, v, form, b, Nk, False)
        ex = _online(s, vb, geo, RESCALE_THR, r16, 0.0, True)[1]
        out[b, :, :, :ex.shape[-1]] = ex
    return out


def softmax_weight(q, k, form, lens, b, row, key):
    """The exact softmax weight of `key` in `row`, smallest over the heads."""
    N, d = q.shape[2], q.shape[3]
    Nk = clamp_len(lens[b], N) if lens is not None else N
    s = torch.einsum("hd,hkd->hk", q[b][:, row], k[b][:, :Nk]) * score_factor(form, d)
    p = torch.exp2(s - s.max(-1, keepdim=True)[0])
    return float((p[:, key] / p.sum(-1)).min())


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-element bound of the bf16 forms
# ---------------------------------------------------------------------------------------------------------------------------------
def bound(q, k, v, form, lens=None, geo=None):
    """-> (exact, bound) [B * N, H * d].
        A     = sum_k p |v_k| / sum_k p                              the scale of every relative error below
        bound = (2 * 2^-9 + n 2^-24 + e_exp) A + half_ulp_bf16(|exact| + that)
    2 * 2^-9: P is rounded to bf16 in the numerator, and (row of ones) in l, or the fp32 l disagrees with the rounded numerator by as
    much.  n = Nk + tiles + padded d + N_CONST fp32 roundings: one per key added, one rescale product per tile, the products of one
    score; N_CONST = 16 covers 1 / l (1 ulp = 2), the product with it (1), l's cross-lane add (1), and the key groups' merge: a0 and
    a1 from v_exp_f32 (2 each) and two products and a sum for O and for l (6) -- 14, rounded up.  e_exp = ln 2 * |argument error| +
    2^-23: the argument s - m is an fp32 accumulation of padded d products, the -m initial accumulator, one `s -= delta` and (unscaled
    q) the fma with the fp32 scale: (padded d + 4) roundings of partial sums no larger than |m| + sum_j |q_j k_j|, and v_exp_f32 is
    good to 1 ulp = 2^-23."""
    B, H, N, d = q.shape
    geo = geo or geometry(form, B, H, N)
    dp, c = padded_d(d, form), score_factor(form, d)
    exacts, bounds = [], []
    for b in range(B):
        Nk = clamp_len(lens[b], N) if lens is not None else N
        qb, kb, vb = q[b], k[b][:, :Nk], v[b][:, :Nk]
        s = (qb @ kb.transpose(-1, -2)) * c
        m = s.max(-1, keepdim=True)[0]
        p = torch.exp2(s - m)
        l = p.sum(-1, keepdim=True)
        exact = (p @ vb) / l
        A = (p @ vb.abs()) / l
        sabs = ((qb.abs() @ kb.abs().transpose(-1, -2)) * c).max(-1, keepdim=True)[0] + m.abs()
        e_exp = math.log(2.0) * (dp + 4) * 2.0 ** -24 * sabs + 2.0 ** -23
        n = Nk + cdiv(Nk, geo.kt) + dp + N_CONST
        b32 = (2.0 * 2.0 ** -9 + n * 2.0 ** -24 + e_exp) * A
        exacts.append(exact)
        bounds.append(b32 + half_ulp_bf16(exact.abs() + b32))
    return _rows(torch.stack(exacts)), _rows(torch.stack(bounds))


def elem_ratio(got, exact, bnd):
    got = got.detach().to("cpu").to(F64)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - exact).abs() / bnd).max()) if got.numel() else 0.0


def check_elem(got, exact, bnd, what, record=None):
    if record is None:
        import conftest
        record = conftest.record
    assert bool(torch.isfinite(got.detach().to("cpu").to(F64)).all()), f"{what}: non-finite values"
    ratio = elem_ratio(got, exact, bnd)
    record(ratio, what + " err/bound")
    if ratio > 1.0:
        err = (got.detach().to("cpu").to(F64) - exact).abs() / bnd
        bad = (err > 1.0).nonzero()
        raise AssertionError(f"{what}: error {ratio:.4g} x the bound; {len(bad)} elements, first (row, column) {bad[:6].tolist()}, "
                             f"rows {sorted(set(bad[:, 0].tolist()))[:12]}")


# the comparator of the attention tests of tests/test_gpu_ops.py as it stands (their `close`): data about the past, for the host test
def old_close(got, want, rtol=2e-2, atol=1e-2):
    got, want = got.float(), want.float()
    err = (got - want).abs()
    return not bool((~(err <= atol + rtol * want.abs())).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# draws: q, k, v [B, H, N, d], q as handed over
# ---------------------------------------------------------------------------------------------------------------------------------
Q_CTRL = 4.0              # a special row's handed-over control component (exact in bf16 and e4m3)
T_DOM, T_PILOT = 30.0, 27.0   # log2 score of a dominant key and of the pilot that sets the running maximum 3 under it


def _gen(seed, B, H, N, d):
    return torch.Generator().manual_seed(seed + 7 * N + d + 1000 * B + 10 * H)


def _hand_over(qbase, form, d):
    """qbase in units where the log2 score is qbase . k * d^-0.5 log2(e)."""
    return bf16_input(qbase * (LOG2E / math.sqrt(d))) if q_carries_scale(form) else bf16_input(qbase)


def _split(t, B, N, H, d):
    return t.view(B, N, H, d).permute(0, 2, 1, 3).contiguous()


def draw_diffuse(form, B, H, N, d, seed=9):
    """tests/test_gpu_ops.py::test_attention's draw, q x 1.5."""
    g = _gen(seed, B, H, N, d)
    q, k, v = (bf16_input(torch.randn(B, N, H * d, generator=g, dtype=F64)) for _ in range(3))
    return _hand_over(_split(bf16_input(q * 1.5), B, N, H, d), form, d), _split(k, B, N, H, d), _split(v, B, N, H, d), {}


def draw_negative(form, B, H, N, d, seed=19):
    """q = (a u + n) c, k = -a u + n', u a unit vector per head, a^2 c = 8: every true score sits near -8 log2 units (noise of
    standard deviation about 1), so a key admitted with score 0 outweighs the real ones."""
    g = _gen(seed, B, H, N, d)
    u = torch.randn(B, H, 1, d, generator=g, dtype=F64)
    u = u / u.norm(dim=-1, keepdim=True)
    a = math.sqrt(8.0 / (LOG2E / math.sqrt(d)))
    qb = a * u + 0.5 * torch.randn(B, H, N, d, generator=g, dtype=F64)
    k = bf16_input(-a * u + 0.5 * torch.randn(B, H, N, d, generator=g, dtype=F64))
    v = bf16_input(torch.randn(B, H, N, d, generator=g, dtype=F64))
    if form in FP8_FORMS:                                         # (host test only: e4m3-representable, as in draw_edge)
        return r8(_hand_over(qb, form, d)), r8(k), r8(v), {}
    return _hand_over(qb, form, d), k, v, {}


def draw_tail(form, B, H, N, d, seed=49):
    """The draw meant for a P quantised without its 2^8 (host test only): key 0 at the origin, so every row has one key at score 0,
    and N - 1 keys near -10.5 log2 units -- under e4m3's smallest subnormal 2^-9 unless P carries the factor.  q, k and v are
    e4m3-representable, so that the floor is P's quantisation alone and not the operands'."""
    g = _gen(seed, B, H, N, d)
    u = torch.randn(B, H, 1, d, generator=g, dtype=F64)
    u = u / u.norm(dim=-1, keepdim=True)
    c = LOG2E / math.sqrt(d)
    a = math.sqrt(10.5 / c)
    qb = a * u + 0.25 * torch.randn(B, H, N, d, generator=g, dtype=F64)
    k = r8(-a * u + 0.25 * torch.randn(B, H, N, d, generator=g, dtype=F64))
    k[:, :, 0] = 0.0
    v = r8(torch.randn(B, H, N, d, generator=g, dtype=F64))
    return r8(qb * c if q_carries_scale(form) else qb), k, v, {}


def _base(form, B, H, N, d, seed, qscale):
    """Ordinary rows and keys with the two CONTROL coordinates d - 2, d - 1 at zero: a special row (q only in the control plane, and
    0.05 randn elsewhere) then meets exactly the scores its keys' control components give it, and ordinary rows never see them."""
    g = _gen(seed, B, H, N, d)
    qb = qscale * torch.randn(B, H, N, d, generator=g, dtype=F64)
    k = torch.randn(B, H, N, d, generator=g, dtype=F64)
    v = bf16_input(torch.randn(B, H, N, d, generator=g, dtype=F64))
    qb[..., d - 2:] = 0.0
    k[..., d - 2:] = 0.0
    return g, qb, k, v


def _special_row(qb, b, row, d, cos, sin, g):
    c = LOG2E / math.sqrt(d)
    qb[b, :, row, :d - 2] = 0.05 * torch.randn(qb.shape[1], d - 2, generator=g, dtype=F64)
    qb[b, :, row, d - 2] = Q_CTRL / c * cos
    qb[b, :, row, d - 1] = Q_CTRL / c * sin


def draw_edge(form, B, H, N, d, lens=None, seed=29):
    """Every key of the launch's edge set is the dominant key (softmax weight >= 0.5) of some query, and every 32-row block has such a
    query.  Edge key i owns the direction theta_i of the control plane: its rows carry Q_CTRL in that direction, the key T_DOM /
    Q_CTRL, and one PILOT key in the first tile of every key group T_PILOT / Q_CTRL -- so the running maximum stands 3 under the
    dominant score when that arrives, below RESCALE_THR.  fp8 forms: q, k and v are e4m3-representable here (the diffuse draw is the
    one that carries the operands' own rounding), so that the floor is P's quantisation and a wrong key is not hidden under it, and
    the pilots stand 8 under.  info["special"]: (b, row, key)."""
    geo = geometry(form, B, H, N)
    g, qb, k, v = _base(form, B, H, N, d, seed, 1.5)
    special = []
    nblk = cdiv(N, 32)
    pilot = T_DOM - 8.0 if form in FP8_FORMS else T_PILOT          # (fp8 tracks the maximum exactly: no threshold to stay under)
    for b in range(B):
        Nk = clamp_len(lens[b], N) if lens is not None else N
        edges = edge_set(Nk, geo)
        used = set()
        for i in range(max(nblk, len(edges))):
            blk, ei = i % nblk, i % len(edges)
            th = 2.0 * math.pi * ei / len(edges)
            row = next((r for r in (blk * 32 + (5 + 11 * (i // nblk) + j) % 32 for j in range(32)) if r < N and r not in used), None)
            if row is None:                                       # the block is full (a last block of a few rows): any free row
                row = next((r for r in range(N) if r not in used), None)
            if row is None:
                continue
            used.add(row)
            _special_row(qb, b, row, d, math.cos(th), math.sin(th), g)
            special.append((b, row, edges[ei]))
        for ei, e in enumerate(edges):
            th = 2.0 * math.pi * ei / len(edges)
            k[b, :, e, d - 2], k[b, :, e, d - 1] = T_DOM / Q_CTRL * math.cos(th), T_DOM / Q_CTRL * math.sin(th)
            for grp in range(geo.sp):
                pk = grp * geo.kt + 1 + ei
                if pk < min(Nk, (grp + 1) * geo.kt) and pk not in edges:
                    k[b, :, pk, d - 2], k[b, :, pk, d - 1] = pilot / Q_CTRL * math.cos(th), pilot / Q_CTRL * math.sin(th)
    if form in FP8_FORMS:
        return r8(_hand_over(qb, form, d)), r8(k), r8(v), dict(special=special)
    return _hand_over(qb, form, d), bf16_input(k), v, dict(special=special)


def stair_rises(n_tiles, grp):
    """Rises of a key group's tile maxima: +4 (under RESCALE_THR: the maximum stays) then +6 over that (10 over the running
    maximum: a raise), alternating; group 1 starts with the +6, and so does a group of two tiles."""
    if n_tiles <= 1:
        return []
    first = 6.0 if (grp == 1 or n_tiles == 2) else 4.0
    return [first if j % 2 == 0 else 10.0 - first for j in range(n_tiles - 1)]


def draw_stairs(form, B, H, N, d, descending=False, seed=39):
    """A few rows of ONE wave meet one spike key per 64-key (wide: 32-key) tile whose scores follow stair_rises() within each key
    group, from 10; the other rows of the wave, and every other row, stay flat.  descending: the first tile of each group at 40, no
    spike after it (every later tile at least 30 below).  wide: the stair rows sit in the SECOND 16-row tile of a wave's 32 rows and
    none in the first.  info["rows"]: the stair rows."""
    geo = geometry(form, B, H, N)
    g, qb, k, v = _base(form, B, H, N, d, seed, 0.5)
    if form == "wide":
        rows = [r for r in (16 + 3, 16 + 9) if r < N] or [min(3, N - 1)]
    else:
        w0 = 32 if N > 64 else 0
        rows = [r for r in (w0 + 3, w0 + 17) if r < N] or [N - 1]
    ntiles = cdiv(N, geo.kt)
    for b in range(B):
        for r in rows:
            _special_row(qb, b, r, d, 1.0, 0.0, g)
        for grp in range(geo.sp):
            mine = list(range(grp, ntiles, geo.sp))
            level = 40.0 if descending else 10.0
            rises = stair_rises(len(mine), grp)
            for j, t in enumerate(mine[:1] if descending else mine):
                if j > 0:
                    level += rises[j - 1]
                key = min(t * geo.kt + 7, N - 1)
                k[b, :, key, d - 2] = level / Q_CTRL
    return _hand_over(qb, form, d), bf16_input(k), v, dict(rows=rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_attn_edges.py (shared with the host test, which proves the comparators sharp AT these shapes)
# ---------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "group form B H N d lens draw")
DRAWS3 = ("diffuse", "negative", "edge")

A_NS = (1, 31, 33, 63, 64, 65, 127, 129, 191, 192, 193, 252, 320, 767, 768, 769)
A_SHAPES = [(1, 2, n) for n in A_NS] + [(11, 8, 768), (3, 2, 200), (4, 2, 200)]          # (B, H, N) at d = 32
B_DS, B_NS = tuple(range(8, 81, 8)), (100, 252)
C_NS, C_DS = (191, 320, 767, 769), (32, 48, 80)
D_DS = (16, 64, 48)
D_LENS = {129: (0, 1, 63, 64, 65, 128, 129, 134), 252: (1, 64, 65, 128, 129, 252), 320: (1, 64, 65, 128, 129, 320)}
E_DS, E_NS = (16, 32, 48, 80), (40, 64, 129, 252, 320, 769)
F_DS = (128, 256, 512)
F_QT1, F_QT2 = [(1, 5), (1, 37), (2, 64), (2, 130)], [(192, 33), (192, 128), (96, 130)]    # (B, N)


def cases_a():
    return [Case("A", "prescaled", B, H, N, 32, None, dr) for B, H, N in A_SHAPES for dr in DRAWS3]


def cases_b():
    return [Case("B", "prescaled", 1, 2, N, d, None, dr) for d in B_DS for N in B_NS for dr in DRAWS3]


def cases_c():
    return [Case("C", "prescaled", 1, 2, N, d, None, dr) for N in C_NS for d in C_DS for dr in ("stairs", "descending")]


def cases_d():
    return [Case("D", "varlen", len(ls), 2, N, d, ls, dr) for N, ls in D_LENS.items() for d in D_DS for dr in DRAWS3]


def cases_e():
    return [Case("E", f, 1, 2, N, d, None, dr) for f in FP8_FORMS for d in E_DS for N in E_NS for dr in ("diffuse", "edge", "tail")]


def cases_f():
    return [Case("F", "wide", B, 1, N, d, None, dr) for B, N in F_QT1 + F_QT2 for d in F_DS for dr in DRAWS3 + ("stairs",)]


def all_cases():
    return cases_a() + cases_b() + cases_c() + cases_d() + cases_e() + cases_f()


def case_id(c):
    ln = "" if c.lens is None else "-len"
    return f"{c.form}-B{c.B}H{c.H}N{c.N}d{c.d}{ln}-{c.draw}"


def draw(c):
    """-> q, k, v [B, H, N, d], info."""
    if c.draw == "diffuse":
        return draw_diffuse(c.form, c.B, c.H, c.N, c.d)
    if c.draw == "negative":
        return draw_negative(c.form, c.B, c.H, c.N, c.d)
    if c.draw == "edge":
        return draw_edge(c.form, c.B, c.H, c.N, c.d, c.lens)
    if c.draw == "tail":
        return draw_tail(c.form, c.B, c.H, c.N, c.d)
    return draw_stairs(c.form, c.B, c.H, c.N, c.d, descending=c.draw == "descending")


def draw_properties(c, ref):
    """What a draw claims about itself, asserted on the float64 scores."""
    q, k, v, info = ref["q"], ref["k"], ref["v"], ref["info"]
    geo = geometry(c.form, c.B, c.H, c.N)
    if c.draw == "edge":
        nblk = cdiv(c.N, 32)
        assert {(b, r // 32) for b, r, _ in info["special"]} == {(b, j) for b in range(c.B) for j in range(nblk)}
        for b in range(c.B):
            Nk = clamp_len(c.lens[b], c.N) if c.lens is not None else c.N
            assert {e for bb, _, e in info["special"] if bb == b} == set(edge_set(Nk, geo)), "an edge key without its query"
        some = info["special"] if len(info["special"]) <= 40 else info["special"][::len(info["special"]) // 40]
        for b, row, key in some:
            assert softmax_weight(q, k, c.form, c.lens, b, row, key) >= 0.5, (b, row, key)
        if c.form not in FP8_FORMS:
            ex = rescale_trace(q, k, v, c.form, c.lens)
            for b, row, key in info["special"]:
                e = ex[b, :, row, key // geo.kt]
                assert bool((e.isnan() | (e <= RESCALE_THR)).all()), f"dominant key {key} of row {row} raises the maximum: {e}"
    if c.draw in ("stairs", "descending"):
        ex = rescale_trace(q, k, v, c.form, c.lens)
        raised = (ex > RESCALE_THR).any(-1)                                   # [B, H, N]
        if ex.shape[-1] > geo.sp and c.draw == "stairs":
            assert bool(raised[:, :, info["rows"]].all()), "a stair row that never raises its maximum"
            assert bool((~raised).any()), "no row stays under the threshold"
            under = (ex > 3.0) & (ex <= RESCALE_THR)
            if ex.shape[-1] > 2 * geo.sp:
                assert bool(under[:, :, info["rows"]].any()), "no +4 step under the threshold"
        if c.draw == "descending":
            assert not bool(raised.any())
            later = ex[:, :, info["rows"]]
            assert bool((later.isnan() | (later <= -30.0)).all())


def attn_block_fp8(x, W, gamma, beta, eps, parts, B, N, H, d, rounded=False):
    """attn_block64(fp8=True), composed as norm_restatement.attn_block composes the bf16 form: the folded-LayerNorm projection, whose
    bf16 outputs (q already scaled: W carries log2(e) / sqrt(d)) enter the e4m3 attention of one 64-key tile."""
    from norm_restatement import attn_block, ln_linear
    if not rounded:
        return attn_block(x, W, gamma, beta, eps, parts, B, N, H, d)
    qkv = ln_linear(x, W, None, gamma, beta, eps, parts, rounded=True)
    C = H * d
    q, k, v = (_heads(qkv[:, i * C:(i + 1) * C], B, N, H, d) for i in range(3))
    return attention(q, k, v, "fp8p", rounded=True)


def valid_rows(c):
    """Row indices of [B * N] whose query is < Nk (all of them without kv_len)."""
    if c.lens is None:
        return torch.arange(c.B * c.N)
    return torch.cat([b * c.N + torch.arange(clamp_len(c.lens[b], c.N)) for b in range(c.B)])


def reference(c):
    """dict(q, k, v, info, exact, rounded[, bound]) of one case; exact / rounded / bound [B * N, H * d]."""
    q, k, v, info = draw(c)
    ref = dict(q=q, k=k, v=v, info=info)
    if c.form in FP8_FORMS:
        ref["exact"] = attention(q, k, v, c.form, c.lens)
    else:
        ref["exact"], ref["bound"] = bound(q, k, v, c.form, c.lens)
    ref["rounded"] = attention(q, k, v, c.form, c.lens, rounded=True)
    return ref


@lru_cache(maxsize=8)
def cached_reference(c):
    """reference(c), kept for the tests that share it (nobody writes into it)."""
    return reference(c)


def judge(got, ref, c, what, record=None):
    """The comparators of one case over the rows whose query is valid: check_elem + check (bf16 forms), check alone (fp8)."""
    rows = valid_rows(c)
    got = got.detach().to("cpu").to(F64)[rows]
    if c.form not in FP8_FORMS:
        check_elem(got, ref["exact"][rows], ref["bound"][rows], what, record)
    check(got, ref["exact"][rows], ref["rounded"][rows], what, record=record)


def rejected(mut, ref, c):
    """-> (rejected?, the ratio that rejects most strongly: err / bound for the bf16 forms' check_elem, else l2 / floor of check)."""
    rows = valid_rows(c)
    mut, exact, rounded = mut[rows], ref["exact"][rows], ref["rounded"][rows]
    if not bool(torch.isfinite(mut).all()):
        return True, math.inf
    e_l2, f_l2, e_max, f_max = floor_ratios(mut, exact, rounded)
    ok = accepts(mut, exact, rounded)
    ratio = e_l2 / f_l2 if f_l2 > 0 else math.inf
    if c.form not in FP8_FORMS:
        er = elem_ratio(mut, exact, ref["bound"][rows])
        ok = ok and er <= 1.0
        ratio = max(ratio / 2.0, er)          # in units of each comparator's own limit
    else:
        ratio = max(ratio / 2.0, (e_max / f_max if f_max > 0 else math.inf) / 4.0)
    return (not ok), ratio
