"""Test helper: a float64 restatement of the projection GEMM family (aldm_pgemm), written from the formulas and from the documented
layouts -- the docstrings of ops.pack_linear / pack_linear_ln / pack_geglu / attach_lora / conv and the aldm_pgemm_t block of
include/aldm_hip.h -- not from the kernel.

As in tests/bwd_restatement.py every form has an `exact` value (float64, nothing rounded) and a `rounded` value (bf16 at exactly the
points where the CONTRACT rounds, each with a comment naming the line it stands for).  `forward()` returns both, and for the forms
without a folded LayerNorm also `packed` (float64 on the operands AS PACKED, T unrounded) with a per-element `bound` around it that has
nothing measured in it:

    t_err_r = (K + 1) 2^-24 sum_k |x_k a_rk| |gate_r|  +  half_ulp_bf16(|t_r| + that)          the fp32 product T, then its bf16 rounding
    mag     = sum_k |x_k w_k| + sum_r |t_r sB_r| + |b| + |res|
    n       = K + 32 RT + 2                                                                 terms of the accumulator and the epilogue
    bound   = (n + 1) 2^-24 mag  +  sum_r t_err_r |sB_r|  +  half_ulp_bf16(|packed| + those)   any-order fp32 sum, T's error, the store

GEGLU (out = v gelu(g), v and g two such accumulators, unrounded until the product):  |gelu(g)| dv + |v| (1.13 dg + SILU_MARGIN unit)
+ 1.13 dv dg, then the store's half ulp; 1.13 bounds |gelu'| (its maximum is 1.1289), `unit` is the largest error one float32 CPU
erf-gelu shows on the same arguments (conv_restatement's rule for a transcendental; it multiplies |v| because the gelu does).

The LayerNorm-folded forms are judged as DESIGN section 20 judges norm_restatement.ln_linear -- `check`, 2 x the L2 floor and 4 x the max
floor per output tensor -- and agree with ln_linear bit for bit where the two overlap (tests/test_pgemm_restatement_host.py).

`mutant=` computes a deliberately wrong variant (host test only); MUTANTS lists them.
"""
import math

import numpy as np
import torch

from bwd_restatement import (F64, GEGLU_EDGE_GATES, accepts, bf16_input, check, geglu_fwd, geglu_pack_order, pack_round,  # noqa: F401
                             r16)
from conv_restatement import SILU_MARGIN, half_ulp_bf16
from norm_restatement import (EPS, EPS_BIG, STAT_MUTANTS, _onepass_f32, _strip_stats, check_table, ladder, ln_draw, ln_linear, ln_n_pad,  # noqa: F401
                              rowstat_entries, table_ok)

GELU_LIP = 1.13                                              # max |d/dg gelu_erf(g)| = 1.12891...
MUTANTS = ("t_round_first", "s_unrounded") + STAT_MUTANTS + (
    "ca_no_irs", "rank_slot_swap", "rank_tile2_dropped", "gate_of_block", "gate_after_last", "parts_drop_last", "parts_first4",
    "vec_from_range0", "res_chunk_xor", "vt_group_straddle", "vt_stats_of_lane", "stats_pre_round", "geglu_pair_shift", "row_last_dup")
LN_ONLY = ("t_round_first", "s_unrounded", "ca_no_irs", "parts_drop_last", "parts_first4", "vt_stats_of_lane") + STAT_MUTANTS


UNBIASED_NOTE = """STAT_MUTANTS' "unbiased" (variance over n - 1) scales rstd by sqrt(1 - 1 / K): 1 / (2 K) <= 2^-9 at K >= 256, half a
bf16 ulp of the output at most.  `check` admits 2 x the L2 floor and 4 x the max floor, and the floor IS the bf16 rounding: the mutation
is below what these margins can separate at every K the kernel is built for (DESIGN section 20 lists it for the norm kernels, where
strips of 8 .. 40 elements make it 1 % and more, and not for ln_linear).  It is recorded, not asserted."""


def gelu(g):
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


def gelu_unit(arg):
    """The largest |float32 CPU erf-gelu - float64 erf-gelu| on these arguments (as float32 arguments): measured on the reference."""
    a32 = arg.to(torch.float32)
    return float((torch.nn.functional.gelu(a32).to(F64) - gelu(a32.to(F64))).abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# packs (ops.pack_linear_ln, ops.attach_lora, ops.pack_geglu restated; the host test compares them bit for bit with ops on CPU tensors)
# ---------------------------------------------------------------------------------------------------------------------------------
def part_columns(parts, layout=None):
    """attach_lora: without a layout the parts fill T's columns from 0 in the order given; with layout = {adapter: (first column,
    width)} the parts of an adapter (sixth element of a part) fill its block from the left.  -> (first column of each part, ranks_used =
    one past the last column in use, Rp = 32 up to 32 columns, else 64)."""
    cols, cursor = [], ({} if layout is None else {n: c0 for n, (c0, _) in layout.items()})
    c = 0
    for p in parts:
        r = p[2].shape[0]
        if layout is None:
            cols.append(c)
            c += r
        else:
            cols.append(cursor[p[5]])
            cursor[p[5]] += r
    used = max(c0 + p[2].shape[0] for c0, p in zip(cols, parts))
    return cols, used, (32 if used <= 32 else 64)


def pack_lora(parts, N, K, ln=None, layout=None, Rp=None, rounded=True):
    """-> dict(A [Rp, K], sB [N, Rp], sA [Rp], cA [Rp], used, Rp): A_cat and the block-structured, pre-scaled B_ext; with a folded
    LayerNorm (ln = (gamma, beta)) A' = A diag(gamma), sA = its row sums, cA = A beta.  rounded=False: nothing rounded."""
    cols, used, rp = part_columns(parts, layout)
    rp = Rp or rp
    A, sB = torch.zeros(rp, K, dtype=F64), torch.zeros(N, rp, dtype=F64)
    sA, cA = torch.zeros(rp, dtype=F64), torch.zeros(rp, dtype=F64)
    for col, (row0, nrows, Ai, Bi, s, *_) in zip(cols, parts):
        r = Ai.shape[0]
        A64 = Ai.to(F64)
        if ln is not None:
            Ap = A64 * ln[0]
            if rounded:
                Ap = r16(Ap)                                  # attach_lora: `Ap = (Af * ln[0][None, :]).to(torch.bfloat16)`
            sA[col:col + r] = Ap.sum(1)                       # attach_lora: `sa[col:col + r] = Ap.float().sum(1)` -- of the ROUNDED rows
            cA[col:col + r] = A64 @ ln[1]
        else:
            Ap = r16(A64) if rounded else A64                 # attach_lora: `Ap = Af.to(torch.bfloat16)`
        A[col:col + r] = Ap
        sB[row0:row0 + nrows, col:col + r] = pack_round(Bi, s) if rounded else s * Bi.to(F64)   # attach_lora: `(Bm.float() * s).to(bf16)`
    return dict(A=A, sB=sB, sA=sA, cA=cA, used=used, Rp=rp)


def pack_ln(W, bias, gamma, beta, rounded=True):
    """pack_linear_ln: W' = W diag(gamma) (bf16), s = row sums of the bf16 W', c = W beta + b."""
    Wg = W * gamma
    Wp = r16(Wg) if rounded else Wg                           # pack_linear_ln: `wp = (w * g[None, :]).to(torch.bfloat16)`
    return Wp, Wp.sum(1), W @ beta + (bias if bias is not None else 0.0)   # pack_linear_ln: `s = wp.float().sum(1)`


def ln_partials(x, nparts):
    """The statistics a producer hands over: float32 [M, nparts, 2] = (sum, sum of squares) of `nparts` column ranges of every row
    (ranges as torch.tensor_split cuts them, so nparts need not divide K)."""
    xs = x.numpy().astype(np.float32)
    cuts = [t.shape[1] for t in torch.tensor_split(torch.empty(1, x.shape[1]), nparts, dim=1)]
    out, k0 = np.zeros((x.shape[0], nparts, 2), np.float32), 0
    for j, w in enumerate(cuts):
        out[:, j, 0] = xs[:, k0:k0 + w].sum(-1, dtype=np.float32)
        out[:, j, 1] = (xs[:, k0:k0 + w] ** 2).sum(-1, dtype=np.float32)
        k0 += w
    return torch.from_numpy(out)


def stats_from_partials(lp, K, eps, mutant=None):
    """design onepass_f32 (norm_restatement): the pairs added in float32, mu = a / K, rstd = 1 / sqrt(max(q / K - mu mu, 0) + eps)."""
    lp = lp.numpy()
    nparts = lp.shape[1]
    use = range(nparts - 1) if mutant == "parts_drop_last" else (range(min(4, nparts)) if mutant == "parts_first4" else range(nparts))
    a, q = np.zeros(lp.shape[0], np.float32), np.zeros(lp.shape[0], np.float32)
    for j in use:
        a += lp[:, j, 0]
        q += lp[:, j, 1]
    mean, rstd = _onepass_f32(torch.from_numpy(a), torch.from_numpy(q), K, eps)
    return mean.view(-1, 1), rstd.view(-1, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the forward forms
# ---------------------------------------------------------------------------------------------------------------------------------
def _gate_rows_of(M, gate, gate_rows, mutant, bm):
    """-> [M, Rp] gate of every row: the row's own sample, row // gate_rows."""
    row = torch.arange(M)
    if mutant == "gate_of_block":
        row = row // bm * bm
    smp = row // gate_rows
    if mutant == "gate_after_last":
        smp = torch.where(smp == gate.shape[0] - 1, smp - 1, smp)
    return gate[smp]


def _vt_stat_rows(M, mi, waves):
    """mutant vt_stats_of_lane: [M, 16] -> the row whose statistics element (row, column c = n % 16) of a token-major tile takes.  A
    lane's token-major rows are 4 mi q + 4 i + e of its wave's 16 mi rows; its standard-order row is 4 mi (c >> 2) + 4 i + (c & 3)."""
    m = torch.arange(M).view(-1, 1)
    c = torch.arange(16).view(1, -1)
    blk, l = m // (16 * mi) * (16 * mi), m % (16 * mi)
    i = (l % (4 * mi)) // 4
    return (blk + 4 * mi * (c >> 2) + 4 * i + (c & 3)).clamp(max=M - 1)


def forward(x, W, bias, parts=(), *, res=None, gate=None, gate_rows=0, ln=None, lp=None, geglu=False, layout=None, Rp=None, vt_col0=None,
            mutant=None, shape=(1, 32, 1, 4), forms=("exact", "packed", "rounded")):
    """x [M, K], W [N, K] float64 holding bf16 values; bias fp32 or None; parts as attach_lora's; res [M, N]; gate fp32 [samples, Rp] with
    gate_rows rows of the GEMM per sample; ln = (gamma, beta, eps) with lp = ln_partials(x, nparts); geglu: W / bias in ORIGINAL row order
    (value | gate halves), the output in original value order [M, N / 2]; vt_col0: first token-major column (only the mutants of the
    token-major store read it); shape = (mi, nt, tiles per range, waves) of the launch (only mutants read it).
    -> dict(exact, rounded, T_exact, T [M, Rp] (rounded), and without ln: packed, bound; stats_src = the fp32 value before the store)."""
    M, K = x.shape
    N = W.shape[0]
    mi, nt, tpr, waves = shape
    bm, bnw = 16 * mi * waves, nt * tpr
    b = bias.to(F64) if bias is not None else torch.zeros(N, dtype=F64)
    out = {}
    if parts:
        _, out["used"], out["Rp"] = part_columns(parts, layout)
        out["Rp"] = Rp or out["Rp"]
    for form in forms:
        rd = form != "exact"
        mu = mutant if form == "rounded" else None
        if ln is not None:
            gamma, beta, eps = ln
            if form == "rounded" and mu not in STAT_MUTANTS + ("twopass",):   # ("twopass": the unmutated form the STAT_MUTANTS are compared with)
                mean, rstd = stats_from_partials(lp, K, eps, mu)
            else:
                mean, rstd = _strip_stats(x, eps, mu if mu in STAT_MUTANTS else None, ln_n_pad(K))
                if mu == "neighbour":
                    mean, rstd = torch.roll(mean, -1, 0), torch.roll(rstd, -1, 0)
            Wg = W * gamma
            Wp, s_, c = pack_ln(W, bias, gamma, beta, rounded=rd)
            if mu == "s_unrounded":
                s_ = Wg.sum(1)
        else:
            Wp, s_, c = W, None, b
        vec = lambda v: v.view(N // bnw, bnw)[0].repeat(N // bnw) if (mu == "vec_from_range0" and v is not None) else v
        c_, s_ = vec(c), vec(s_)
        acc = x @ Wp.t()
        mag = x.abs() @ Wp.abs().t()
        terr = torch.zeros(M, N, dtype=F64)
        T = None
        if parts:
            pk = pack_lora(parts, N, K, ln[:2] if ln is not None else None, layout, Rp, rounded=rd)
            sB = pk["sB"].clone()
            if mu == "rank_slot_swap":
                sB[:, 4:8], sB[:, 16:20] = pk["sB"][:, 16:20], pk["sB"][:, 4:8]
            if mu == "rank_tile2_dropped":
                sB[:, 16:] = 0.0
            t = x @ pk["A"].t()
            g_ = _gate_rows_of(M, gate.to(F64), gate_rows, mu, bm) if gate is not None else torch.ones(1, pk["Rp"], dtype=F64)
            if ln is not None:
                if mu == "t_round_first":
                    t = r16(t)
                t = t - mean * pk["sA"] + (pk["cA"] if mu == "ca_no_irs" else pk["cA"] / rstd)
            t = t * g_
            if form == "packed":
                tm = (K + 1) * 2.0 ** -24 * (x.abs() @ pk["A"].abs().t()) * g_.abs()
                te = tm + half_ulp_bf16(t.abs() + tm)
                terr = te @ sB.abs().t()
                mag = mag + t.abs() @ sB.abs().t()
            T = t
            if form == "rounded":
                T = r16(t)                                    # the GEMM's LoRA stage: T (T'' under a folded LayerNorm) is bf16 for the MFMA
            acc = acc + T @ sB.t()
            out["T" if form == "rounded" else "T_" + form] = T
        if ln is not None:
            mean_n, rstd_n = mean, rstd
            v = rstd_n * (acc - mean_n * s_) + c_
            if mu == "vt_stats_of_lane" and vt_col0 is not None:
                src = _vt_stat_rows(M, mi, waves)[:, torch.arange(N) % 16]       # [M, N]
                alt = rstd.view(-1)[src] * (acc - mean.view(-1)[src] * s_) + c_
                v[:, vt_col0:] = alt[:, vt_col0:]
        else:
            v = acc + c_
            mag = mag + c_.abs()
        if res is not None:
            r_ = res
            if mu == "res_chunk_xor":
                odd = ((torch.arange(M) >> 1) & 1).bool()
                swapped = res.view(M, N // 16, 2, 8).flip(2).reshape(M, N)
                r_ = torch.where(odd.view(-1, 1), swapped, res)
            v = v + r_
            mag = mag + res.abs()
        if geglu:
            I = N // 2
            val, gt = v[:, :I], v[:, I:]
            if mu == "geglu_pair_shift":                      # packed order: block j = (16 value | 16 gate); the gate read 16 packed columns on
                pk_ = v[:, geglu_pack_order(I)]               # is the NEXT block's value columns
                gt = torch.roll(pk_, -16, 1)[:, torch.argsort(geglu_pack_order(I))][:, I:]
            y = val * gelu(gt)
            if form == "packed":
                n = K + 2
                dv, dg = (n + 1) * 2.0 ** -24 * mag[:, :I], (n + 1) * 2.0 ** -24 * mag[:, I:]
                pre = gelu(gt).abs() * dv + val.abs() * (GELU_LIP * dg + SILU_MARGIN * gelu_unit(gt)) + GELU_LIP * dv * dg
                out["bound"] = pre + half_ulp_bf16(y.abs() + pre)
        else:
            y = v
            if form == "packed":
                rt = 0 if not parts else (1 if out["used"] <= 16 else 2)
                pre = (K + 32 * rt + 2 + 1) * 2.0 ** -24 * mag + terr
                out["bound"] = pre + half_ulp_bf16(y.abs() + pre)
        if form == "rounded":
            out["stats_src"] = y                              # (mutant stats_pre_round: the statistics of this instead of the store)
            y = r16(y)                                        # the epilogue's bf16 store (the one rounding of the output, GEGLU included)
            if mu == "row_last_dup" and M > 1:
                y[M - 1] = y[M - 2]
        out[form] = y
    if ln is not None:
        out.pop("packed", None), out.pop("bound", None)
    return out


def t_stored(T, used, Rp):
    """lora_t_out [M, Rp]: the bf16 T, zeros beyond ranks_used."""
    t = torch.zeros(T.shape[0], Rp, dtype=F64)
    t[:, :used] = T[:, :used]
    return t


def rowstats(y_stored, bnw):
    """rowstat_out [M, N / bnw, 2] of the values AS STORED -> (table, magnitude) (norm_restatement.rowstat_entries)."""
    return rowstat_entries(y_stored, bnw)


def vt_store(y, B, OHW, vt_col0, vt_ld, mutant=None, mi=1, fill=float("nan")):
    """columns >= vt_col0 of y [B * OHW, N] token-major: vt[b][n - vt_col0][pix], [B, C, vt_ld], padding columns = `fill` (untouched).
    mutant vt_group_straddle: a lane's group of 4 mi rows is stored contiguously from its first row's place."""
    C = y.shape[1] - vt_col0
    vt = torch.full((B, C, vt_ld), fill, dtype=F64)
    if mutant != "vt_group_straddle":
        vt[:, :, :OHW] = y[:, vt_col0:].view(B, OHW, C).permute(0, 2, 1)
        return vt
    flat, g = vt.view(-1), 4 * mi
    ch = torch.arange(C)
    for m in range(B * OHW):
        m0 = m // g * g
        pos = (m0 // OHW) * C * vt_ld + ch * vt_ld + (m0 % OHW) + (m - m0)
        ok = pos < flat.numel()
        flat[pos[ok]] = y[m, vt_col0:][ok]
    return vt


# ---------------------------------------------------------------------------------------------------------------------------------
# comparators (bwd_restatement.check / accepts, norm_restatement.check_table, and the per-element bound)
# ---------------------------------------------------------------------------------------------------------------------------------
def elem_ratio(got, ref):
    got = got.detach().to("cpu").to(F64)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - ref["packed"]).abs() / ref["bound"]).max())


def check_elem(got, ref, what, record=None):
    if record is None:
        import conftest
        record = conftest.record
    ratio = elem_ratio(got, ref)
    record(ratio, what + " err/bound")
    if ratio > 1.0:
        err = (got.detach().to("cpu").to(F64) - ref["packed"]).abs() / ref["bound"]
        bad = (~(err <= 1.0)).nonzero()
        raise AssertionError(f"{what}: error {ratio:.4g} x the bound; {len(bad)} elements, first (row, column) {bad[:6].tolist()}, columns "
                             f"{sorted(set(bad[:, 1].tolist()))[:12]}, rows {sorted(set(bad[:, 0].tolist()))[:12]}")


def check_out(got, ref, what, record=None):
    """one output tensor: the per-element bound where the form has one, and `check` (2 x the L2 floor, 4 x the max floor) always"""
    if "bound" in ref:
        check_elem(got, ref, what, record)
    check(got, ref["exact"], ref["rounded"], what, record=record)


def accepts_out(got, ref):
    return ("bound" not in ref or elem_ratio(got, ref) <= 1.0) and accepts(got, ref["exact"], ref["rounded"])


# the comparator of tests/test_gpu_pgemm.py as it stood when this file was written (against a float32 product): data about the past
def old_close(got, want, rtol=1.2e-2):
    got, want = got.float(), want.float()
    atol = 8e-3 * float(want.abs().max()) + 1e-6
    return not bool((~((got - want).abs() <= atol + rtol * want.abs())).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# launch arithmetic restated (the GPU test asserts it against the label of what launched, the host test against an enumeration)
# ---------------------------------------------------------------------------------------------------------------------------------
LDS_MAX = 160 * 1024


def rt_of(ranks_used):
    """LoRA k-tiles of 16 ranks: 0 without an adapter, 1 up to 16 ranks in use, 2 up to 32."""
    return 0 if not ranks_used else (1 if ranks_used <= 16 else 2)


def lds_bytes(K, mi, nt, tpr, waves, res, Rp):
    """min(tpr, 3) ring stages of a weight tile (+ the residual tile), mean / rstd of the row block, two column vectors, the LoRA-B rows"""
    bm = 16 * mi * waves
    stage = nt * K * 2 + (bm * nt * 2 if res else 0)
    return min(tpr, 3) * stage + 2 * bm * 4 + 2 * tpr * nt * 4 + tpr * nt * Rp * 2


def plan_candidates(M, N, K, *, Rp=0, ranks_used=0, res=False, geglu=False, vt_col0=None, max_ranges=0, fixed=(0, 0, 0, 0)):
    """every (mi, nt, tpr, waves) a launch may take, in the planner's order: waves 4 then 8; mi 2 only with 4 waves and (K <= 384 or no
    adapter); nt 64 only for GEGLU, nt | vt_col0; tpr | N / nt with tpr nt <= 512, at most max_ranges ranges, within the LDS"""
    rt = rt_of(ranks_used) if Rp else 0
    fmi, fnt, ftpr, fnw = fixed
    out = []
    for nw in (4, 8):
        if fnw and fnw != nw:
            continue
        for mi in ((1, 2) if ((K <= 384 or rt == 0) and nw == 4) else (1,)):
            if fmi and fmi != mi:
                continue
            for nt in (32, 64):
                if (fnt and fnt != nt) or (geglu and nt != 64) or (vt_col0 is not None and vt_col0 % nt):
                    continue
                ntiles = N // nt
                for tpr in range(1, ntiles + 1):
                    if tpr * nt > 512 or ntiles % tpr or (ftpr and ftpr != tpr):
                        continue
                    if max_ranges > 0 and ntiles // tpr > max_ranges:
                        continue
                    if lds_bytes(K, mi, nt, tpr, nw, res, Rp) > LDS_MAX:
                        continue
                    out.append((mi, nt, tpr, nw))
    return out


def plan_cost(M, N, K, cfg, *, Rp=0, ranks_used=0, res=False, geglu=False):
    """bytes one workgroup pulls (its rows of x, its weight and LoRA-A rows, residual, output) + 48 KiB per workgroup, times the rounds
    of 256 workgroups, times 1.05 for 8 waves"""
    mi, nt, tpr, nw = cfg
    rt = rt_of(ranks_used) if Rp else 0
    bm = 16 * mi * nw
    wgs = -(-M // bm) * (N // nt // tpr)
    nbytes = bm * K * 2.0 + (tpr * nt + 16 * rt) * K * 2.0 + (bm * tpr * nt * 2.0 if res else 0.0) + bm * tpr * nt * (1.0 if geglu else 2.0)
    return ((wgs + 255) // 256) * (nbytes + 48.0 * 1024) * (1.05 if nw == 8 else 1.0)


def plan(M, N, K, **kw):
    """the first candidate of the least cost, or None (no launch shape: the GEMM stays on the convolution kernel)"""
    fixed = kw.pop("fixed", (0, 0, 0, 0))
    ckw = {k: kw[k] for k in ("Rp", "ranks_used", "res", "geglu") if k in kw}
    best, bc = None, None
    for cfg in plan_candidates(M, N, K, fixed=fixed, **kw):
        cost = plan_cost(M, N, K, cfg, **ckw)
        if bc is None or cost < bc:
            best, bc = cfg, cost
    return best


def vt_vec(OHW, vt_ld, vt_batch_stride, base_elem_offset):
    """tokens per token-major store: 8 when the tokens per sample, the row pitch, the batch stride and the base (in bf16 elements from a
    16-byte aligned address) are all multiples of 8, else 4 when all are multiples of 4, else 1"""
    for v in (8, 4):
        if OHW % v == 0 and vt_ld % v == 0 and vt_batch_stride % v == 0 and base_elem_offset % v == 0:
            return v
    return 1


def label_of(cfg, Rp, vt=False, dual=False):
    mi, nt, tpr, nw = cfg
    return f"pgemm_{16 * mi * nw}x{nt}x{tpr}w{nw}_r{Rp}" + ("_vt" if vt else "") + ("d" if dual else "")


def grid_of(M, N, cfg):
    mi, nt, tpr, nw = cfg
    return -(-M // (16 * mi * nw)) * (N // nt // tpr)


# ---------------------------------------------------------------------------------------------------------------------------------
# draws (deterministic per shape)
# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def column_code(N, g):
    """a vector whose entry n carries its own index: ((n % 61) - 30) / 16 + noise below 1/128 -- read from a neighbouring range, tile or
    row (any shift that is no multiple of 61) it is wrong by 3/64 at least, several times the bound of an output of this size (half a
    bf16 ulp of a value below 4 is 1/128); a larger code would only raise the output's rounding floor and hide the other mutants"""
    n = torch.arange(N, dtype=F64)
    return (((n % 61) - 30.0) / 16.0 + (torch.rand(N, generator=g, dtype=F64) - 0.5) / 64.0).float()


def balanced_parts(N, K, ranks, g, scalings=(1.0, 1.5, 2.0), names=None):
    """one part per entry of `ranks` over equal shares of the N columns; s (x A^T) B^T is as large as the base term x W^T (both of unit
    variance for unit-variance x), every part with its own rank and scaling; B rows column-coded in their sign pattern"""
    nrows = N // len(ranks)
    parts = []
    for i, r in enumerate(ranks):
        A = (torch.randn(r, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).float()
        Bm = (torch.randn(nrows, r, generator=g) / (math.sqrt(r) * scalings[i % 3])).to(torch.bfloat16).float()
        p = (i * nrows, nrows, A, Bm, scalings[i % 3])
        parts.append(p + (names[i],) if names else p)
    return parts


def draw(M, K, N, ranks=(), *, res=False, ladder_rows=False, geglu=False, seed=0):
    """-> dict(x, W, bias, parts, res, gamma, beta): the balanced, column-coded draw; ladder_rows: ln_draw's rows (|mean| / std up to 16)"""
    g = _gen(M, K, N, len(ranks), sum(ranks), seed)
    x_l, gamma, beta = ln_draw(M, K, seed + 50)
    x = x_l if ladder_rows else bf16_input(torch.randn(M, K, generator=g, dtype=F64))
    W = bf16_input(torch.randn(N, K, generator=g, dtype=F64) / math.sqrt(K))
    bias = column_code(N, g)
    d = dict(x=x, W=W, bias=bias, parts=balanced_parts(N, K, ranks, g) if ranks else [], gamma=gamma, beta=beta, res=None)
    if res:
        d["res"] = bf16_input(torch.randn(M, N, generator=g, dtype=F64) + column_code(N, g).to(F64))
    return d


GATE_VALUES = (0.0, 1.0, 0.5, -0.75)


def gate_draw(M, gate_rows, Rp, used):
    """fp32 [M / gate_rows, Rp]: column r of sample s takes GATE_VALUES[(s + r) % 4]; the LAST sample is all 1.5 on the columns in use
    (distinct from every other: rows >= M read it), columns beyond `used` hold 3 (they multiply zeros)."""
    S = M // gate_rows
    s, r = torch.arange(S).view(-1, 1), torch.arange(Rp).view(1, -1)
    gt = torch.tensor(GATE_VALUES)[(s + r) % 4].clone()
    gt[S - 1] = 1.5
    gt[:, used:] = 3.0
    return gt.float()


def plant_edge_gates(d):
    """GEGLU: the gate columns 0, 15, 16, 31, I - 16 and I - 1 (both ends of a 16-column block, first and last block) get a zero weight
    row and GEGLU_EDGE_GATES[i] as their bias, so the pre-activation gate there IS the edge value in every row -- with a folded
    LayerNorm too (a zero row of W has s = 0 and c = b).  -> the planted gate columns."""
    I = d["W"].shape[0] // 2
    cols = [0, 15, 16, 31, I - 16, I - 1]
    for col, v in zip(cols, GEGLU_EDGE_GATES):
        d["W"][I + col] = 0.0
        d["bias"][I + col] = v
    return cols


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_pgemm_edges.py (shared with the host test, which proves the comparators sharp AT these shapes)
# ---------------------------------------------------------------------------------------------------------------------------------
A_MS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193)
A_SHAPES = ((1, 4), (2, 4), (1, 8))                          # (mi, waves)
A_KS = (256, 640)
A_N = 128
B_NS = (64, 128, 192, 320, 576, 1152)
B_TPRS = (1, 2, 3, 4, 6, 8, 16)
B_KS = (256, 384, 640)
C_RANKS = (1, 4, 15, 16, 17, 31, 32)
C_PART_RANKS = ((4, 8, 4), (16, 8, 8))
GATE_ROWS = (1, 7, 40, 64, 100)
D_TOKENS = (1, 3, 4, 7, 8, 9, 12, 60, 63, 64, 65, 100)
D_NPARTS = (1, 2, 4, 5, 13, 15, 16)
E_KS, E_MS = (256, 384, 640), (1, 65, 130)
E_SHAPES = ((1, 64, 4), (2, 64, 4), (1, 64, 8))              # (mi, nt, waves)
E_TPRS = (1, 2, 4, 8)
OLD_SHAPES = [(1000, 256, 256, 4), (504, 384, 384, 8), (512, 640, 640, 4), (200, 256, 256, 16), (333, 384, 384, 32)]   # test_lora_residual


def b_cfgs(N, K, res=False, Rp=0):
    """(1, 32, tpr, 4) for every B_TPRS entry that divides N / 32, spans <= 512 columns and fits the LDS"""
    return [(1, 32, t, 4) for t in B_TPRS if (N // 32) % t == 0 and t * 32 <= 512 and lds_bytes(K, 1, 32, t, 4, res, Rp) <= LDS_MAX]



def case(group, name, M, K, N, cfg, *, ranks=(), res=False, stats=False, t_out=False, gate_rows=0, nparts=0, vt=None, geglu=False,
         layout_col0=0, Rp=0, ladder_rows=None, expect_cfg=True):
    """One launch of the GPU file.  cfg = (mi, nt, tiles per range, waves); nparts > 0: LayerNorm folded with that many partial pairs;
    vt = dict(B, col0, dual, pad, off): B samples of M / B tokens, first token-major column, vt_dual, extra elements of row pitch beyond
    the tokens rounded up to 8, base offset in elements; layout_col0: the (single) adapter's column block starts there; Rp: 64 = the
    direct launch with a 64-wide T; eps: EPS_BIG (0.1, where a misplaced or dropped eps shows: norm_restatement) on every other folded case;
    expect_cfg False: the forced shape is set aside (more than 16 statistics ranges)."""
    return dict(group=group, name=name, M=M, K=K, N=N, cfg=cfg, ranks=tuple(ranks), res=res, stats=stats, t_out=t_out, gate_rows=gate_rows,
                nparts=nparts, eps=(EPS_BIG if (nparts and (M + nparts) % 2) else EPS), vt=vt, geglu=geglu, layout_col0=layout_col0, Rp=Rp, ladder_rows=bool(nparts) if ladder_rows is None else ladder_rows,
                expect_cfg=expect_cfg)


def vt_geom(c):
    """-> (B, OHW, col0, C, vt_ld, vt_batch_stride, base offset, vt_vec) of a token-major case"""
    v = c["vt"]
    B = v["B"]
    OHW = c["M"] // B
    ld = (OHW + 7) // 8 * 8 + v.get("pad", 0)
    C = c["N"] - v["col0"]
    return B, OHW, v["col0"], C, ld, C * ld, v.get("off", 0), vt_vec(OHW, ld, C * ld, v.get("off", 0))


def fits(c):
    mi, nt, tpr, nw = c["cfg"]
    rp = c["Rp"] or (32 if c["ranks"] else 0)
    return (c["N"] // nt) % tpr == 0 and tpr * nt <= 512 and lds_bytes(c["K"], mi, nt, tpr, nw, c["res"], rp) <= LDS_MAX


def all_cases():
    cs = []
    # A, rows: every M on both sides of a wave's rows, a row block, two row blocks; grids of 1 .. 4 (one range), 5 .. 20 (five ranges)
    for K in A_KS:
        for mi, nw in A_SHAPES:
            for M in A_MS:
                cs.append(case("A", f"plain M{M} K{K} mi{mi}w{nw}", M, K, 128, (mi, 32, 4, nw)))
                ranks = () if (K == 640 and mi == 2) else (4,)           # (K = 640 has no mi = 2 form with an adapter: group C asserts it)
                cs.append(case("A", f"res+lora+stats M{M} K{K} mi{mi}w{nw}", M, K, 320, (mi, 32, 2, nw), ranks=ranks, res=True, stats=True))
    for M in (1, 65, 129, 193):
        cs.append(case("A", f"plain 7 ranges M{M}", M, 256, 448, (1, 64, 1, 4)))     # grids 7, 14, 21, 28
    cs.append(case("A", "plain 3 ranges M65", 65, 256, 192, (1, 64, 1, 4)))          # grid 6
    # B, ranges: the ring unfilled (1, 2), exactly filled (3), wrapped (4 ..); column-coded bias and residual; > 16 ranges with statistics
    for K in B_KS:
        for N in B_NS + (512,):                              # (512: the only N <= 1920 here whose 16 tiles take tiles per range 8 and 16)
            for cfg in b_cfgs(N, K, res=True):
                nr = N // (32 * cfg[2])
                cs.append(case("B", f"res+stats N{N} K{K} tpr{cfg[2]}", 70, K, N, cfg, res=True, stats=True, expect_cfg=nr <= 16))
                if nr > 16:
                    cs.append(case("B", f"res N{N} K{K} tpr{cfg[2]}", 70, K, N, cfg, res=True))
    # C, ranks
    for r in C_RANKS:
        cs.append(case("C", f"rank {r}", 70, 256, 128, (1, 32, 2, 4), ranks=(r,), res=True, t_out=True))
        cs.append(case("C", f"rank {r} mi2", 70, 384, 128, (2, 64, 1, 4), ranks=(r,), t_out=True))
    for pr in C_PART_RANKS:
        cs.append(case("C", f"parts {pr}", 70, 256, 192, (1, 32, 2, 4), ranks=pr, t_out=True))
        cs.append(case("C", f"parts {pr} vt ln", 70, 256, 192, (1, 32, 2, 4), ranks=pr, nparts=4, vt=dict(B=2, col0=128)))
    cs.append(case("C", "adapter at 16..19", 70, 256, 128, (1, 32, 2, 4), ranks=(4,), res=True, t_out=True, layout_col0=16))
    cs.append(case("C", "K640 mi1", 70, 640, 128, (1, 32, 2, 4), ranks=(4,), res=True, t_out=True))
    cs.append(case("C", "Rp64 ranks 20", 70, 256, 128, (1, 32, 2, 4), ranks=(20,), res=True, t_out=True, Rp=64))
    for gr, M in zip(GATE_ROWS, (70, 70, 200, 192, 200)):
        for res in (False, True):
            cs.append(case("C", f"gate rows {gr} res{int(res)}", M, 256, 192, (1, 32, 2, 4), ranks=(4, 8, 4), res=res, gate_rows=gr))
        cs.append(case("C", f"gate rows {gr} mi2 r20", M, 256, 192, (2, 32, 2, 4), ranks=(4, 12, 4), res=True, gate_rows=gr))
        cs.append(case("C", f"gate rows {gr} vt ln", M, 256, 192, (1, 32, 2, 4), ranks=(4, 8, 4), nparts=3, vt=dict(B=M // gr, col0=128), gate_rows=gr))
    # D, token-major stores: every token count x B, both row-group sizes; LayerNorm folded on every other one, nparts cycling
    k = 0
    for tok in D_TOKENS:
        for B in (2, 3):
            for mi in (1, 2):
                npt = D_NPARTS[k % len(D_NPARTS)] if k % 2 == 0 else 0
                k += 1
                cs.append(case("D", f"tok{tok} B{B} mi{mi} np{npt}", tok * B, 256, 192, (mi, 32, 2, 4), ranks=(4, 4, 4), nparts=npt,
                               vt=dict(B=B, col0=128)))
    for npt in D_NPARTS:                                     # every nparts at one shape whose rows straddle samples and the row block
        cs.append(case("D", f"nparts {npt}", 130, 256, 192, (1, 32, 2, 4), ranks=(4, 4, 4), nparts=npt, vt=dict(B=2, col0=128)))
        cs.append(case("D", f"nparts {npt} mi2 K384", 130, 384, 192, (2, 64, 1, 4), ranks=(), nparts=npt, vt=dict(B=2, col0=128)))
    # store paths by a row pitch or base offset: 8 kept (both multiples of 8), demoted 8 -> 4, 8 -> 1, 4 -> 1
    for tok, pad, off in ((64, 8, 8), (64, 4, 0), (64, 0, 4), (64, 1, 0), (64, 0, 1), (12, 0, 2), (12, 2, 0)):
        for mi in (1, 2):
            cs.append(case("D", f"tok{tok} pad{pad} off{off} mi{mi}", tok * 2, 256, 192, (mi, 32, 2, 4), ranks=(4, 4, 4),
                           vt=dict(B=2, col0=128, pad=pad, off=off)))
    cs.append(case("D", "range straddles vt_col0", 130, 256, 768, (1, 64, 6, 4), ranks=(4, 4, 4), nparts=5, vt=dict(B=2, col0=512)))
    cs.append(case("D", "range straddles vt_col0 mi2", 126, 256, 768, (2, 64, 6, 4), ranks=(), vt=dict(B=2, col0=512)))
    for tok in (9, 60, 64):
        cs.append(case("D", f"dual col0 0 tok{tok}", tok * 2, 256, 192, (1, 32, 2, 4), ranks=(8,), t_out=True, vt=dict(B=2, col0=0, dual=True)))
        cs.append(case("D", f"dual col0 2C tok{tok}", tok * 2, 256, 192, (2, 32, 2, 4), ranks=(8,), t_out=True, vt=dict(B=2, col0=128, dual=True)))
    # E, GEGLU: N = 512 packed columns (I = 256): 8 tiles of 64, every T in E_TPRS; plain and LayerNorm-folded (nparts 1 / 16)
    for K in E_KS:
        for im, M in enumerate(E_MS):
            for ish, (mi, nt, nw) in enumerate(E_SHAPES):
                for it, T in enumerate(E_TPRS):
                    for npt in (0, (1, 16)[(im + ish + it) % 2]):
                        c = case("E", f"geglu M{M} K{K} mi{mi}w{nw} T{T} np{npt}", M, K, 512, (mi, nt, T, nw), geglu=True, nparts=npt)
                        if fits(c):                          # (K = 640: a 64-column tile is 80 KiB, only T = 1 fits the LDS)
                            cs.append(c)
    return cs


def inputs(c):
    """the case's draw -> dict(x, W, bias, parts, res, gamma, beta, gate, lp, layout)"""
    d = draw(c["M"], c["K"], c["N"], c["ranks"], res=c["res"], ladder_rows=c["ladder_rows"], geglu=c["geglu"])
    d["layout"] = None
    if c["layout_col0"]:
        d["parts"] = [p + ("a",) for p in d["parts"]]
        d["layout"] = {"a": (c["layout_col0"], sum(c["ranks"]))}
    if c["geglu"]:
        d["edge_cols"] = plant_edge_gates(d)
    _, used, rp = part_columns(d["parts"], d["layout"]) if d["parts"] else ([], 0, 0)
    d["used"], d["Rp"] = used, (c["Rp"] or rp)
    d["gate"] = gate_draw(c["M"], c["gate_rows"], d["Rp"], used) if c["gate_rows"] else None
    d["lp"] = ln_partials(d["x"], c["nparts"]) if c["nparts"] else None
    return d


def reference(c, d=None, mutant=None, forms=("exact", "packed", "rounded")):
    """-> dict of output tensors of the case, each a dict(exact, rounded[, packed, bound]):
    "y" the row-major columns, "vt" the token-major buffer [B, C, vt_ld] (NaN = untouched padding), "T" lora_t_out [M, Rp];
    and "stats_src" (the unrounded value) for the statistics mutant."""
    d = d if d is not None else inputs(c)
    ln = (d["gamma"], d["beta"], c["eps"]) if c["nparts"] else None
    v = c["vt"]
    f = forward(d["x"], d["W"], d["bias"].to(F64), d["parts"], res=d["res"], gate=d["gate"], gate_rows=c["gate_rows"], ln=ln, lp=d["lp"],
                geglu=c["geglu"], layout=d["layout"], Rp=c["Rp"] or None, vt_col0=(v["col0"] if v else None), mutant=mutant, shape=c["cfg"],
                forms=forms)
    keys = [k for k in ("exact", "packed", "rounded", "bound") if k in f]
    out = {}
    if v is None:
        out["y"] = {k: f[k] for k in keys}
    else:
        B, OHW, col0, C, ld, bs, off, vec = vt_geom(c)
        ncol = c["N"] if v.get("dual") else col0
        if ncol:
            out["y"] = {k: f[k][:, :ncol] for k in keys}
        out["vt"] = {k: vt_store(f[k], B, OHW, col0, ld, mutant if k == "rounded" else None, c["cfg"][0],
                                 fill=(1.0 if k == "bound" else float("nan"))) for k in keys}
    if c["t_out"]:
        out["T"] = {"exact": t_stored(f["T_exact"], f["used"], f["Rp"]), "rounded": t_stored(f["T"], f["used"], f["Rp"])} if "exact" in forms \
            else {"rounded": t_stored(f["T"], f["used"], f["Rp"])}
    if "rounded" in forms:
        out["stats_src"] = f["stats_src"]
    return out


def stats_width(c, cfg=None):
    mi, nt, tpr, nw = cfg or c["cfg"]
    return nt * tpr


# ---------------------------------------------------------------------------------------------------------------------------------
# judging a whole case (every output tensor on its own, never pooled)
# ---------------------------------------------------------------------------------------------------------------------------------
def _valid(c, key, t):
    """the part of an output that holds values: the token columns of the token-major buffer, everything of the others"""
    return t[:, :, :vt_geom(c)[1]] if key == "vt" else t


def reject_ratio(c, got, ref):
    """got = {output: tensor} judged against ref = reference(c): the largest of err / bound, l2 / (2 floor), max / (4 floor) over the
    outputs (> 1: rejected; inf: a value where the padding must stay untouched, or a non-finite value).  The statistics table, where
    got has one, is judged by its own bound against the statistics of got's stored y."""
    from bwd_restatement import L2_MARGIN, MAX_MARGIN, _ratio, floor_ratios
    worst = 0.0
    for key in ("y", "vt", "T"):
        if key not in ref:
            continue
        g, r = got[key].detach().to("cpu").to(F64), ref[key]
        if key == "vt" and not torch.equal(torch.isnan(g), torch.isnan(r["exact"])):
            return math.inf
        g = _valid(c, key, g)
        r = {k: _valid(c, key, v) for k, v in r.items()}
        if not bool(torch.isfinite(g).all()):
            return math.inf
        if "bound" in r:
            worst = max(worst, elem_ratio(g, r))
        e_l2, f_l2, e_max, f_max = floor_ratios(g, r["exact"], r["rounded"])
        worst = max(worst, _ratio(e_l2, f_l2) / L2_MARGIN, _ratio(e_max, f_max) / MAX_MARGIN)
    if "stats" in got:
        bnw = got["y"].shape[1] // got["stats"].shape[1]
        want, mag = rowstat_entries(got["y"].detach().to("cpu").to(F64), bnw)
        worst = max(worst, table_ok(got["stats"], want, mag, bnw)[1])
    return worst


def check_case(c, got, ref, record=None):
    """the GPU test's comparator: check_out per output tensor, the padding of the token-major buffer untouched, check_table"""
    what = f"{c['group']} {c['name']}"
    for key in ("y", "vt", "T"):
        if key not in ref:
            continue
        g, r = got[key].detach().to("cpu").to(F64), ref[key]
        if key == "vt":
            assert torch.equal(torch.isnan(g), torch.isnan(r["exact"])), f"{what}: the padding columns of the token-major buffer were written"
        check_out(_valid(c, key, g), {k: _valid(c, key, v) for k, v in r.items()}, f"{what} {key}", record)
    if "stats" in got:
        bnw = got["y"].shape[1] // got["stats"].shape[1]
        want, mag = rowstat_entries(got["y"].detach().to("cpu").to(F64), bnw)
        check_table(got["stats"], want, mag, bnw, f"{what} stats")


def outputs_of(c, ref, mutant=None):
    """what a kernel computing `ref`'s rounded form would leave: {y, vt, T, stats} (host test)"""
    got = {k: ref[k]["rounded"] for k in ("y", "vt", "T") if k in ref}
    if c["stats"]:
        src = ref["stats_src"] if mutant == "stats_pre_round" else got["y"]
        got["stats"] = rowstat_entries(src, stats_width(c))[0].float()
    return got


def relevant(c, mutant):
    """can this mutant differ from the unmutated form at this case at all?  (the host test still compares the outputs)"""
    if mutant in LN_ONLY and not c["nparts"]:
        return False
    if mutant in ("eps_out", "eps_drop") and c["eps"] != EPS_BIG:
        return False                                         # (at 1e-5 the mutation is 8e-5 of rstd, below the bf16 floor: norm_restatement)
    if mutant == "unbiased":
        return False                                         # (see UNBIASED_NOTE: the host test records it, it cannot assert it)
    lora = bool(c["ranks"])
    need = {"t_round_first": lora, "ca_no_irs": lora, "rank_slot_swap": lora, "rank_tile2_dropped": lora, "gate_of_block": c["gate_rows"] > 0,
            "gate_after_last": c["gate_rows"] > 0, "res_chunk_xor": c["res"], "vt_group_straddle": c["vt"] is not None,
            "vt_stats_of_lane": c["vt"] is not None, "stats_pre_round": c["stats"], "geglu_pair_shift": c["geglu"], "row_last_dup": c["M"] > 1}
    return need.get(mutant, True)
