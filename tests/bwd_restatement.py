"""Test helper: float64 restatements of the backward (training) ops of csrc/train.hip and csrc/attention_bwd.hip, written from the
formulas and the documented layouts, not from the kernels.

Every op comes in two forms that share one body and the same bf16-representable inputs:

  exact    the operation in float64, nothing rounded (`rounded=False`);
  rounded  the same float64 arithmetic with a bf16 rounding at exactly the points where the kernel's CONTRACT rounds
           (`rounded=True`); each point carries a comment naming the kernel line it stands for.

`||rounded - exact||` is the FLOOR: the distance from the truth that the kernel's number formats alone impose.  It is measured on
this reference, never on the code under test.  `check(got, exact, rounded, what)` -- the one comparator of
tests/test_gpu_bwd_edges.py -- asks, per output tensor and never pooled across tensors,

    ||got - exact||2 / ||exact||2  <=  2 * ||rounded - exact||2 / ||exact||2          max|got - exact|  <=  4 * max|rounded - exact|

The margins are conditions, not measurements: a kernel differs from `rounded` only by fp32 accumulation order and the fast exp2 /
sigmoid / erf (all of order 1e-6), an L2 over thousands of elements concentrates within a few per cent (2x), and the maximum is
an extreme statistic of the same distribution (4x).  tests/test_bwd_restatement_host.py proves on the CPU that these two
conditions reject every listed mutant of every op at every shape the GPU test uses (last section).

A `mutant=` argument computes a deliberately wrong variant (host test only).
"""
import math

import torch

F64 = torch.float64
LOG2E = 1.4426950408889634


def r16(x):
    """Round to bf16 (nearest even), back in float64."""
    return x.to(torch.bfloat16).to(F64)


def bf16_input(x):
    """A bf16-representable float64 tensor: what every kernel input is."""
    return x.to(torch.bfloat16).to(F64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------------------------------------
L2_MARGIN, MAX_MARGIN = 2.0, 4.0


def floor_ratios(got, exact, rounded):
    """-> (e_l2, f_l2, e_max, f_max) of one output tensor."""
    got = got.detach().to("cpu").to(F64)
    exact, rounded = exact.to(F64), rounded.to(F64)
    assert got.shape == exact.shape == rounded.shape, (got.shape, exact.shape, rounded.shape)
    en = float(exact.norm())
    en = en if en > 0.0 else 1.0                              # an all-zero truth (dQ at one token): absolute norms
    e, f = got - exact, rounded - exact
    return float(e.norm()) / en, float(f.norm()) / en, float(e.abs().max()), float(f.abs().max())


def _ratio(e, f):
    return e / f if f > 0.0 else (0.0 if e == 0.0 else math.inf)   # a floor of zero (exactly representable result) admits only equality


def accepts(got, exact, rounded):
    """The two conditions of `check`, as a bool (host mutant test)."""
    if not bool(torch.isfinite(got.detach().to("cpu").to(F64)).all()):
        return False
    e_l2, f_l2, e_max, f_max = floor_ratios(got, exact, rounded)
    return e_l2 <= L2_MARGIN * f_l2 and e_max <= MAX_MARGIN * f_max


def check(got, exact, rounded, what, record=None):
    """record(value, what): where the two measured ratios go (default: conftest.record, one line each in the test log)."""
    if record is None:
        import conftest
        record = conftest.record
    assert bool(torch.isfinite(got.detach().to("cpu").to(F64)).all()), f"{what}: non-finite values"
    e_l2, f_l2, e_max, f_max = floor_ratios(got, exact, rounded)
    record(_ratio(e_l2, f_l2), what + " l2/floor")
    record(_ratio(e_max, f_max), what + " max/floor")
    assert e_l2 <= L2_MARGIN * f_l2, f"{what}: rel L2 {e_l2:.4g} > {L2_MARGIN} x floor {f_l2:.4g}"
    assert e_max <= MAX_MARGIN * f_max, f"{what}: max err {e_max:.4g} > {MAX_MARGIN} x floor {f_max:.4g}"


# the comparator of tests/test_gpu_train_ops.py as it stood when these tests were written: data about the past, for the host test
def old_close(got, want, rtol=2e-2, atol=None):
    got, want = got.float(), want.float()
    atol = atol if atol is not None else 1.5e-2 * float(want.abs().max()) + 1e-7
    err = (got - want).abs()
    return not bool((~(err <= atol + rtol * want.abs())).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def norm_inputs(g, x, groups_of, a=0.5, b=0.5):
    """dy = randn + a * xhat + b: correlated with the normalised input and with a mean, so both mean-subtraction terms of a norm
    backward (s1, s2) are O(1) of the result -- with independent gaussians they are O(1 / sqrt(n)) and invisible.
    groups_of(t) -> [rows, n] view of the normalisation strips."""
    xs = groups_of(x)
    xh = (xs - xs.mean(1, keepdim=True)) / xs.std(1, keepdim=True, unbiased=False)
    return bf16_input(torch.randn(x.shape, generator=g, dtype=F64) + (a * xh + b).reshape(x.shape))


# ---------------------------------------------------------------------------------------------------------------------------------
# group norm / layer norm backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _norm_bwd_rows(x, dy, gamma, beta, eps, silu, mutant=None, n_extra=0):
    """x, dy, gamma, beta: [rows, n] (gamma / beta broadcastable) -> dx [rows, n], float64, nothing rounded.
        xhat = (x - mean) rstd ; z = xhat gamma + beta ; gd = dy act'(z) gamma
        dx   = rstd (gd - mean(gd) - xhat mean(gd xhat))
    mutants: "no_s1", "no_s2", "neither" drop the mean-subtraction terms; "n" counts n + n_extra elements per strip."""
    n = x.shape[1] + (n_extra if mutant == "n" else 0)
    mean = x.sum(1, keepdim=True) / n
    var = ((x - mean) ** 2).sum(1, keepdim=True) / n
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    dz = dy
    if silu:
        z = xh * gamma + beta
        sg = torch.sigmoid(z)
        dz = dy * sg * (1.0 + z * (1.0 - sg))
    gd = dz * gamma
    s1 = gd.sum(1, keepdim=True) / n
    s2 = (gd * xh).sum(1, keepdim=True) / n
    if mutant in ("no_s1", "neither"):
        s1 = torch.zeros_like(s1)
    if mutant in ("no_s2", "neither"):
        s2 = torch.zeros_like(s2)
    return rstd * (gd - s1 - xh * s2)


def gn_rows(t, groups):
    """[B, C, H, W] -> [B * groups, Cg * H * W]: the strips of F.group_norm."""
    return t.reshape(t.shape[0] * groups, -1)


def groupnorm_bwd(x, dy, gamma, beta, groups, eps, silu, prior=None, rounded=False, mutant=None):
    """dX of act(F.group_norm(x, groups, gamma, beta, eps)), NCHW float64.  prior: the gradient x already holds (dx_add)."""
    B, C, H, W = x.shape
    Cg = C // groups
    per = lambda p: p.view(1, groups, Cg, 1).expand(B, groups, Cg, H * W).reshape(B * groups, Cg * H * W)
    dx = _norm_bwd_rows(gn_rows(x, groups), gn_rows(dy, groups), per(gamma), per(beta), eps, silu, mutant, n_extra=Cg).view(x.shape)
    if rounded:
        dx = r16(dx)                                  # groupnorm_bwd_kernel: `o[k] = (bf16)(rstd * (gd - s1 - xh * s2))`
    if prior is not None:
        dx = dx + prior
        if rounded:
            dx = r16(dx)                              # groupnorm_bwd_kernel: `o[k] = (bf16)((float)o[k] + (float)pa[i][k])`
    return dx


def layernorm_bwd(x, dy, gamma, eps, prior=None, rounded=False, mutant=None):
    """dX of F.layer_norm(x, (C,), gamma, beta, eps), x [M, C] float64 (beta does not enter)."""
    dx = _norm_bwd_rows(x, dy, gamma.view(1, -1), torch.zeros(1, 1, dtype=F64), eps, False, mutant, n_extra=8)
    if rounded:
        dx = r16(dx)                                  # layernorm_bwd_kernel: `r[k] = (bf16)(rstd * (... - s1 - xh * s2))`
    if prior is not None:
        dx = dx + prior
        if rounded:
            dx = r16(dx)                              # layernorm_bwd_kernel: `r[k] = (bf16)((float)r[k] + (float)acc[i][k])`
    return dx


# ---------------------------------------------------------------------------------------------------------------------------------
# GEGLU (value | gate halves; the kernels read ops.pack_geglu's interleaving of 16 value | 16 gate columns)
# ---------------------------------------------------------------------------------------------------------------------------------
def geglu_pack_order(I):
    """packed position -> original column of h [M, 2I] = (value[0:I] | gate[0:I])."""
    idx = torch.arange(I).view(-1, 16)
    return torch.cat([idx, idx + I], 1).reshape(-1)


def geglu_fwd(h, rounded=False):
    I = h.shape[1] // 2
    a, g = h[:, :I], h[:, I:]
    y = a * (0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0))))
    return r16(y) if rounded else y                   # geglu_fwd_kernel: `o[k] = (bf16)(a * gelu_erf_f(g))`


def geglu_bwd(h, dout, rounded=False, mutant=None):
    """-> dh [M, 2I] = (dvalue | dgate).  mutant "no_pdf": the density term of gelu' dropped from dgate."""
    I = h.shape[1] // 2
    a, g = h[:, :I], h[:, I:]
    cdf = 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    da = dout * g * cdf
    dg = dout * a * (cdf + (0.0 if mutant == "no_pdf" else 1.0) * g * pdf)
    dh = torch.cat([da, dg], 1)
    return r16(dh) if rounded else dh                 # geglu_bwd_kernel: `da[k] = (bf16)(...)`, `dg[k] = (bf16)(...)`


# ---------------------------------------------------------------------------------------------------------------------------------
# adjoint of nearest up-sampling: src = floor(dst * IH / OH)
# ---------------------------------------------------------------------------------------------------------------------------------
def _nearest_src(O, I, mutant=None):
    src = (torch.arange(O) * I) // O
    if mutant == "shift" and O % I != 0:              # preimage window of every source moved up by one destination
        src = torch.cat([src[:1], src[:-1]])
        src[0] = I                                    # (destination 0 falls out of every window)
    return src


def upsample_nearest_bwd(dy, ih, iw, rounded=False, mutant=None):
    """dy [B, C, OH, OW] -> dx [B, C, ih, iw]: the sum of dy over each source pixel's preimage."""
    B, C, OH, OW = dy.shape
    sh, sw = _nearest_src(OH, ih, mutant), _nearest_src(OW, iw, mutant)
    t = torch.zeros(B, C, ih + 1, OW, dtype=F64).index_add_(2, sh, dy)[:, :, :ih]
    dx = torch.zeros(B, C, ih, iw + 1, dtype=F64).index_add_(3, sw, t)[:, :, :, :iw]
    return r16(dx) if rounded else dx                 # upsample_nearest_bwd_kernel: `o[k] = (bf16)acc[k]` (one rounding of the fp32 sum)


# ---------------------------------------------------------------------------------------------------------------------------------
# eps-prediction MSE
# ---------------------------------------------------------------------------------------------------------------------------------
def mse_grad(pred, target, rounded=False):
    """-> (loss, dpred): mean((pred - target)^2) and its gradient."""
    e = pred.to(F64) - target.to(F64)
    d = 2.0 * e / e.numel()
    return float((e * e).mean()), (r16(d) if rounded else d)     # mse_grad_kernel: `dpred[i] = (bf16)(2 e / n * gscale)`


# ---------------------------------------------------------------------------------------------------------------------------------
# attention: qkv [B * N, 3C] rows = (q | k | v), heads of d columns; scores in the log2 domain, lse = log2 sum_k 2^(s c)
# ---------------------------------------------------------------------------------------------------------------------------------
def _heads(t, B, N, H, d):
    return t.reshape(B, N, H, d).permute(0, 2, 1, 3)             # [B, H, N, d]


def _rows(t):
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, H * d)


def l_sums_rounded_p(d):
    """attention.hip AttnCfg::VL: at padded head dims 32 and 64 the row sum l is added up from the fp32 probabilities; at 16, 48 and
    80 it rides in the P V product as a row of ones, i.e. it is the sum of the bf16-ROUNDED probabilities."""
    dp = next(p for p in (16, 32, 48, 64, 80) if d <= p)
    return dp % 32 != 0


def attention_fwd(qkv, B, N, H, d, rounded=False):
    """-> (out [B*N, C], lse [B, H, N] in log2 units)."""
    C = H * d
    q, k, v = (_heads(qkv[:, i * C:(i + 1) * C], B, N, H, d) for i in range(3))
    c = LOG2E / math.sqrt(d)
    outs, lses = [], []
    for b in range(B):                                           # (one batch element at a time: bounds the N x N temporaries)
        s2 = (q[b] @ k[b].transpose(-1, -2)) * c                 # [H, N, N]
        m = s2.max(-1, keepdim=True)[0]
        p = torch.exp2(s2 - m)
        l = p.sum(-1, keepdim=True)
        lses.append(m[..., 0] + torch.log2(l[..., 0]))
        if rounded:
            p = r16(p)                                           # attention_kernel: `pf[s2][i] = (bf16)p0`
            if l_sums_rounded_p(d):
                l = p.sum(-1, keepdim=True)                      # attention_kernel: l = row DP of O^T (the row of ones of V^T)
        o = (p @ v[b]) / l
        outs.append(r16(o) if rounded else o)                    # attention_kernel: `(bf16)(o[t][4 * g] * inv)`
    return _rows(torch.stack(outs)), torch.stack(lses)


def attention_bwd(qkv, dO, O, lse, B, N, H, d, rounded=False, mutant=None):
    """-> dqkv [B*N, 3C] = (dQ | dK | dV).  O: the forward's output as the backward receives it (bf16 in the rounded form), lse in
    log2 units.      P = 2^(s c - lse) ; delta = rowsum(dO * O) ; dV = P^T dO ; dS = P * (dO V^T - delta) ;
                     dK = scale dS^T Q ; dQ = scale dS K
    mutants: "last_query" (left out of the dK / dV sums), "delta8" (delta misses the last 8 columns of d), "noscale" (dK),
    "lse_ulp" (the P of dV from lse + 2^-8)."""
    C = H * d
    q, k, v = (_heads(qkv[:, i * C:(i + 1) * C], B, N, H, d) for i in range(3))
    do, o = _heads(dO, B, N, H, d), _heads(O, B, N, H, d)
    scale = 1.0 / math.sqrt(d)
    c = LOG2E * scale
    rd = r16 if rounded else (lambda t: t)
    dqs, dks, dvs = [], [], []
    for b in range(B):
        dd = do[b] * o[b]
        if mutant == "delta8":
            dd = dd[..., :d - 8]
        delta = dd.sum(-1, keepdim=True)                         # attn_bwd_dq_kernel: delta from dO and O as given (bf16), fp32 sum
        s2 = (q[b] @ k[b].transpose(-1, -2)) * c
        p = torch.exp2(s2 - lse[b].unsqueeze(-1))
        pv = torch.exp2(s2 - (lse[b].unsqueeze(-1) + 2.0 ** -8)) if mutant == "lse_ulp" else p
        ds = p * (do[b] @ v[b].transpose(-1, -2) - delta)
        pv = rd(pv)                                              # attn_bwd_dkv_kernel: `pf[i >> 3][i & 7] = (bf16)p`
        ds = rd(ds)                                              # attn_bwd_dkv_kernel / attn_bwd_dq_kernel: `dsf[...] = (bf16)(p * (dp[i] - ...))`
        if mutant == "last_query":
            pv, dsk = pv[:, :N - 1], ds[:, :N - 1]
            dv = pv.transpose(-1, -2) @ do[b][:, :N - 1]
            dk = dsk.transpose(-1, -2) @ q[b][:, :N - 1] * scale
        else:
            dv = pv.transpose(-1, -2) @ do[b]
            dk = ds.transpose(-1, -2) @ q[b] * (1.0 if mutant == "noscale" else scale)
        dq = ds @ k[b] * scale
        dqs.append(rd(dq))                                       # attn_bwd_dq_kernel: `(bf16)(acc[t][4 * g] * scale)`
        dks.append(rd(dk))                                       # attn_bwd_dkv_kernel: `(bf16)(acck[t][4 * g] * scale)`
        dvs.append(rd(dv))                                       # attn_bwd_dkv_kernel: `(bf16)accv[t][4 * g]`
    return torch.cat([_rows(torch.stack(t)) for t in (dqs, dks, dvs)], 1)


def attention_pair(qkv, dO, B, N, H, d):
    """The four reference results of one attention case: (out, lse, dqkv) exact and (out, dqkv) rounded.  The rounded backward
    receives the rounded forward's own bf16 output and the exact lse -- nothing of the code under test enters a reference."""
    o_e, lse = attention_fwd(qkv, B, N, H, d)
    o_r, _ = attention_fwd(qkv, B, N, H, d, rounded=True)
    g_e = attention_bwd(qkv, dO, o_e, lse, B, N, H, d)
    g_r = attention_bwd(qkv, dO, o_r, lse, B, N, H, d, rounded=True)
    return o_e, o_r, lse, g_e, g_r


LSE_BOUND = 2.0 ** -12     # log2 units: scales every recomputed P by at most 1.7e-4, a tenth of P's bf16 half-ulp


# ---------------------------------------------------------------------------------------------------------------------------------
# one LoRA site:  y = x W^T + bias + sum_parts s (x A^T) B^T [rows of the part] (+ res)
# ---------------------------------------------------------------------------------------------------------------------------------
def pack_round(src_f32, scale):
    """lora_pack_kernel: `(bf16)(j.src[...] * j.scale)` -- the product is taken in fp32."""
    return (src_f32.to(torch.float32) * torch.tensor(scale, dtype=torch.float32)).to(torch.bfloat16).to(F64)


def lora_site(x, W, bias, parts, dy, res=None, prior=None, rounded=False):
    """parts: [(row0, nrows, A [r, K], B [nrows, r], s)] with fp32 A / B.  -> dict(y, dx, T, U, dA[], dB[]) in float64.
    exact: dA / dB are the true gradients.  rounded: T = x A^T and U = dy (sB) are bf16, A and sB are the packed bf16 operands."""
    M, K = x.shape
    rd = r16 if rounded else (lambda t: t)
    y = x @ W.t() + (bias if bias is not None else 0.0) + (res if res is not None else 0.0)
    dx = dy @ W + (prior if prior is not None else 0.0)
    Ts, Us, dAs, dBs = [], [], [], []
    for row0, nrows, A, Bm, s in parts:
        A64, B64 = A.to(F64), Bm.to(F64)
        Ap = pack_round(A, 1.0) if rounded else A64              # lora_pack_kernel, jobs 0 and 3 of a part (scale 1)
        sBp = pack_round(Bm, s) if rounded else s * B64          # lora_pack_kernel, jobs 1 and 2 of a part (scale s)
        T = rd(x @ Ap.t())                                       # the GEMM's lora_t_out: T = x A^T stored bf16
        dyp = dy[:, row0:row0 + nrows]
        U = rd(dyp @ sBp)                                        # the dX GEMM's lora_t_out: U = dy (sB) stored bf16
        y[:, row0:row0 + nrows] += T @ sBp.t()
        dx = dx + U @ Ap
        Ts.append(T); Us.append(U)
        dAs.append(s * B64.t() @ dyp.t() @ x)                    # exact gradients (the fp32 outputs are judged by tn_bound)
        dBs.append(s * dyp.t() @ (x @ A64.t()))
    return dict(y=rd(y), dx=rd(dx), T=Ts, U=Us, dA=dAs, dB=dBs)  # the GEMM epilogues' bf16 stores of y and dX


def tn_exact(P, Q):
    """(P^T Q, |P|^T |Q|) in float64: the product of aldm_tn_small / aldm_tn_batched and the scale of its rounding error."""
    P, Q = P.to(F64), Q.to(F64)
    return P.t() @ Q, P.abs().t() @ Q.abs()


def tn_unit(P, Q):
    """The largest |float32 CPU matmul - float64| / (|P|^T |Q|) of these operands: what fp32 accumulation costs at this shape."""
    want, mag = tn_exact(P, Q)
    f32 = (P.to(torch.float32).t() @ Q.to(torch.float32)).to(F64)
    return float(((f32 - want).abs() / mag.clamp_min(1e-300)).max())


TN_MARGIN = 8.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_bwd_edges.py (shared with the host mutant test, which proves the comparator sharp AT these shapes)
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, groups, C, H, W): quads per strip = H * W * C / groups / 4, one on each side of every groupnorm_bwd template boundary
GN_CASES = [
    (1, 2, 8, 64, 32),       # 2048: last strip of <4, 512>
    (1, 2, 8, 3, 683),       # 2049: first of <4, 1024>
    (2, 2, 24, 25, 40),      # 3000
    (1, 2, 8, 64, 64),       # 4096: last of <4, 1024>
    (1, 2, 8, 17, 241),      # 4097: first of <8, 1024>
    (2, 2, 40, 25, 40),      # 5000
    (1, 2, 8, 128, 64),      # 8192: last of <8, 1024>
    (1, 2, 8, 3, 2731),      # 8193: first of <16, 1024> (the recomputing second sweep)
    (1, 2, 80, 25, 40),      # 10000
    (1, 2, 128, 32, 32),     # 16384: the register-resident maximum
]
GN_PIVOT_CASES = [(2, 2, 24, 25, 40), (1, 2, 80, 25, 40)]      # x = 40 + 0.5 randn: loads the pivot-shifted variance
GN_VARIANTS = ("plain", "silu", "x2", "add")
GN_OLD_CASES = [(2, 32, 128, 16, 16, 1), (2, 8, 160, 7, 4, 1), (1, 32, 640, 63, 4, 0)]   # (B, groups, C, H, W, act) of test_gpu_train_ops
LN_CS, LN_MS = (8, 248, 256, 264, 1280, 2048), (1, 9, 50)
LN_OLD = [(50, 64), (50, 256), (50, 640)]
GEGLU_CASES = [(1, 16), (3, 16), (40, 64), (17, 1280)]
GEGLU_EDGE_GATES = (0.0, -0.0, 6.0, -6.0, 12.0, -12.0)
UPS_SIZES = [(32, 2, 63, 4), (63, 4, 125, 8), (8, 4, 16, 8), (5, 3, 5, 3)]           # (ih, iw, oh, ow)
UPS_BC = [(1, 8), (3, 24)]
MSE_NS = (1, 255, 257, 100003)
ADD_NS = (1, 5, 8, 2051, 256 * 8 * 3 + 3)
ATTN_DS = (8, 16, 24, 32, 40, 48, 56, 64, 72, 80)                                     # at B = 1, H = 2, N = 100
ATTN_NS = (1, 31, 33, 63, 64, 65, 100, 191, 192, 767, 768)                            # at B = 1, H = 2, d = 32: every wave-count arm
ATTN_PAIRS = [(1, 3), (3, 4), (2, 4), (3, 8)]                                         # (B, H) at N = 200, d = 32
ATTN_PEAKED = [(200, 32), (200, 80), (768, 32), (768, 80)]                            # (N, d) at B = 1, H = 2, logit std ~ 4
# launch_attn_d's arms of the lse form: N < 64 <1, 1>, < 192 <4, 1>, < 768 <4, 2> (keys split), then <8, 2>, and <8, 1> once
# ceil(N / 256) * H * B >= 256.  The N thresholds are in ATTN_NS; these two sit on either side of the last one (255 and 264).
ATTN_FWD_ARMS = [(5, 17, 768, 32), (11, 8, 768, 32)]                                  # (B, H, N, d)
ATTN_OLD = [(2, 200, 4, 32), (1, 252, 8, 48), (2, 64, 4, 80), (1, 1000, 2, 32), (1, 40, 4, 24)]   # (B, N, H, d) of test_gpu_train_ops


def gn_draw(case, variant, pivot=False, seed=0):
    """Inputs of one groupnorm_bwd case (NCHW float64, bf16-representable): x, dy, gamma, beta, act, C1, prior."""
    B, groups, C, H, W = case
    g = torch.Generator().manual_seed(seed + 1000 * C + H * W)
    x = bf16_input(40.0 + 0.5 * torch.randn(B, C, H, W, generator=g, dtype=F64)) if pivot else \
        bf16_input(torch.randn(B, C, H, W, generator=g, dtype=F64) * 2 + 0.3)
    gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).to(F64)          # fp32 parameters
    beta = (0.3 * torch.randn(C, generator=g)).to(F64)
    dy = norm_inputs(g, x, lambda t: gn_rows(t, groups))
    Cg = C // groups
    C1 = C if variant not in ("x2", "add") else (8 if Cg > 8 else 4)   # Cg > 8: the join splits group 0 between x and x2
    prior = bf16_input(torch.randn(B, C, H, W, generator=g, dtype=F64)) if variant == "add" else None
    return x, dy, gamma, beta, (1 if variant == "silu" else 0), C1, prior


def ln_draw(M, Cc, seed=1):
    g = torch.Generator().manual_seed(seed + 100 * Cc + M)
    x = bf16_input(torch.randn(M, Cc, generator=g, dtype=F64) * 2 + 1)
    gamma = (1.0 + 0.3 * torch.randn(Cc, generator=g)).to(F64)
    dy = norm_inputs(g, x, lambda t: t)
    prior = bf16_input(torch.randn(M, Cc, generator=g, dtype=F64))
    return x, dy, gamma, prior


def geglu_draw(M, I, seed=2):
    g = torch.Generator().manual_seed(seed + M + I)
    h = bf16_input(torch.randn(M, 2 * I, generator=g, dtype=F64))
    edge = torch.tensor(GEGLU_EDGE_GATES, dtype=F64)
    gates = h[:, I:].clone().reshape(-1)
    gates[: min(len(edge), gates.numel())] = edge[: gates.numel()]
    h[:, I:] = gates.view(M, I)
    return h, bf16_input(torch.randn(M, I, generator=g, dtype=F64))


def attn_draw(B, N, H, d, peaked=False, seed=3):
    """qkv [B*N, 3C], dO [B*N, C].  peaked: q and k scaled by 2, logits q.k / sqrt(d) of standard deviation 4."""
    g = torch.Generator().manual_seed(seed + 7 * N + d + 1000 * B + 10 * H)
    C = H * d
    qkv = torch.randn(B * N, 3 * C, generator=g, dtype=F64)
    if peaked:
        qkv[:, :2 * C] *= 2.0
    return bf16_input(qkv), bf16_input(torch.randn(B * N, C, generator=g, dtype=F64))


# name -> (M, K, N, ranks, res): the out-projection form (res given) and the fused q | k | v form at 2 x 37 and 2 x 64 tokens
SITE_CASES = {"out": (74, 64, 64, (4,), True), "qkv37": (74, 64, 192, (16, 16, 16), False), "qkv64": (128, 64, 192, (16, 16, 16), False)}


def site_draw(M, K, N, ranks, seed=5, res=False):
    """One LoRA-bearing GEMM: x [M, K], W [N, K], bias, parts (N split evenly, fp32 A / B, scalings 0.5, 0.75, ..), dy, res.
    x, dy and the rows of A and B are 1 + 0.5 randn up to a sign per rank, so that no element of x, dy, T = x A^T or U = dy (sB)
    is near zero: the one-missing-row condition of the dA / dB bound (host test) needs every row to matter in every element."""
    g = torch.Generator().manual_seed(seed)
    off = lambda *shape: 1.0 + 0.5 * torch.randn(*shape, generator=g, dtype=F64)
    x = bf16_input(off(M, K))
    W = bf16_input(torch.randn(N, K, generator=g, dtype=F64) / math.sqrt(K))
    bias = bf16_input(torch.randn(N, generator=g, dtype=F64))
    nrows = N // len(ranks)
    parts = []
    for i, r in enumerate(ranks):
        sign = (1.0 - 2.0 * (torch.arange(r) % 2)).to(F64)
        A = (sign.view(r, 1) * off(r, K) / math.sqrt(K)).to(torch.float32)
        Bm = (sign.view(1, r) * off(nrows, r) / math.sqrt(r)).to(torch.float32)
        parts.append((i * nrows, nrows, A, Bm, 0.5 + 0.25 * i))
    dy = bf16_input(off(M, N))
    rs = bf16_input(torch.randn(M, N, generator=g, dtype=F64)) if res else None
    return x, W, bias, parts, dy, rs
