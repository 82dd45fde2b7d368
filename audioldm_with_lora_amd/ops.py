"""Tensor-level wrappers over the C-ABI (include/aldm_hip.h).

torch is used for device memory and the current stream only; all arithmetic happens in the HIP
kernels.  Activations are channels-last bf16 tensors: images [B, H, W, C], token sequences [B*N, C].
"""
import ctypes as C
import json
import math
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_LRELU, ACT_NONE, ACT_SILU, ACT_TANH, OUT_BF16, OUT_F32, IgemmArgs, check)

BK = 64


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _require_gpu(t):
    if not t.is_cuda:
        raise _lib.AldmError("the product path runs on the MI355X only (got a CPU tensor); there is no CPU fallback")


@dataclass
class PackedW:
    """bf16 weights packed for aldm_igemm: w [N][Kpad] (K = (kh*KW+kw)*Cin + c), fp32 bias."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    N: int
    Cin: int            # total input channels (both concat sources)
    KH: int = 1
    KW: int = 1
    geglu: bool = False
    lora_a: Optional[torch.Tensor] = None      # [Rp][Kpad] bf16
    lora_b: Optional[torch.Tensor] = None      # [N][Rp] bf16, pre-scaled by alpha/r
    Rp: int = 0
    ln_s: Optional[torch.Tensor] = None        # LayerNorm folded into the GEMM: fp32 [N] column sums of W diag(gamma)
    ln_sa: Optional[torch.Tensor] = None       # fp32 [Rp]: row sums of A diag(gamma)
    ln_ca: Optional[torch.Tensor] = None       # fp32 [Rp]: A beta
    ln_eps: float = 1e-5
    Cext: int = 0                               # channels of the fused 1x1 second-source segment appended to every weight row

    @property
    def Kpad(self):
        return self.w.shape[1]

    @property
    def ln(self):
        return self.ln_s is not None


def _pad_k(w2d: torch.Tensor) -> torch.Tensor:
    n, k = w2d.shape
    kp = (k + BK - 1) // BK * BK
    out = torch.zeros(n, kp, dtype=torch.bfloat16, device=w2d.device)
    out[:, :k] = w2d.to(torch.bfloat16)
    return out.contiguous()


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor]) -> PackedW:
    """Conv2d weight [Cout, Cin, KH, KW] -> [Cout][(kh, kw, cin)]."""
    co, ci, kh, kw = weight.shape
    w = _pad_k(weight.detach().permute(0, 2, 3, 1).reshape(co, kh * kw * ci))
    return PackedW(w, None if bias is None else bias.detach().float().contiguous(), co, ci, kh, kw)


def pack_conv_shortcut(weight, bias, sc_weight, sc_bias) -> PackedW:
    """ResnetBlock2D.conv2 [Cout, C, 3, 3] and conv_shortcut [Cout, Cin, 1, 1] as ONE weight matrix [Cout][(kh, kw, c) | cin]:
    conv2(h) + conv_shortcut(x) is then a single implicit GEMM whose K loop ends with a 1x1 segment over the block input
    (aldm_igemm x3 / x4).  Needs C % 64 == 0 and Cin % 64 == 0 (the LDS-DMA path); the caller falls back to two launches otherwise."""
    co, ci, kh, kw = weight.shape
    w2 = weight.detach().permute(0, 2, 3, 1).reshape(co, kh * kw * ci)
    ws = sc_weight.detach().reshape(co, -1)
    pw = PackedW(_pad_k(torch.cat([w2, ws], dim=1)), (bias.detach().float() + sc_bias.detach().float()).contiguous(), co, ci, kh, kw)
    pw.Cext = ws.shape[1]
    return pw


def pack_conv1d(weight: torch.Tensor, bias: Optional[torch.Tensor]) -> PackedW:
    """Conv1d weight [Cout, Cin, K] -> KH = 1, KW = K."""
    return pack_conv(weight.unsqueeze(2), bias)


def pack_linear(weight: torch.Tensor, bias: Optional[torch.Tensor]) -> PackedW:
    n, k = weight.shape
    return PackedW(_pad_k(weight.detach()), None if bias is None else bias.detach().float().contiguous(), n, k)


def pack_geglu(weight: torch.Tensor, bias: torch.Tensor) -> PackedW:
    """GEGLU.proj [2*inner, C]: rows re-ordered into blocks of (16 value | 16 gate) so that a lane holds
    a value and its gate in adjacent MFMA tiles (value = first half, gate = second half)."""
    two_inner, k = weight.shape
    inner = two_inner // 2
    assert inner % 16 == 0
    idx = torch.arange(inner, device=weight.device).view(-1, 16)
    order = torch.cat([idx, idx + inner], dim=1).reshape(-1)
    pw = PackedW(_pad_k(weight.detach()[order]), bias.detach().float()[order].contiguous(), two_inner, k)
    pw.geglu = True
    return pw


def pack_linear_ln(weight, bias, gamma, beta, eps=1e-5, geglu=False):
    """Linear applied to LayerNorm(x) with the norm folded in:  LN(x) W^T + b = rstd (x W'^T - mean s) + c,
    W' = W diag(gamma) (bf16), s = row sums of the bf16 W' (what the MFMA really sums), c = W beta + b."""
    w = weight.detach().float()
    g, bt = gamma.detach().float(), beta.detach().float()
    wp = (w * g[None, :]).to(torch.bfloat16)
    s = wp.float().sum(1)
    c = w @ bt + (bias.detach().float() if bias is not None else 0.0)
    if geglu:
        inner = w.shape[0] // 2
        idx = torch.arange(inner, device=w.device).view(-1, 16)
        order = torch.cat([idx, idx + inner], dim=1).reshape(-1)
        wp, s, c = wp[order], s[order], c[order]
    pw = PackedW(_pad_k(wp), c.contiguous(), w.shape[0], w.shape[1])
    pw.geglu = geglu
    pw.ln_s, pw.ln_eps = s.contiguous(), eps
    pw._ln = (g, bt)
    return pw


def attach_lora(pw: PackedW, parts, layout=None):
    """parts: list of (row_offset, n_rows, A [r, K], B [n_rows, r], scaling) -- one per LoRA-wrapped target
    that shares this GEMM.  Builds A_cat [Rp][Kpad] and the block-structured, pre-scaled B_ext [N][Rp].

    Several adapters: parts carry a sixth element, the adapter's name, and layout = {adapter: (first column, width)} (lora.lora_layout)
    gives every adapter the same column block in every fused GEMM of the model; the parts of an adapter fill its block from the left
    in the order given, unused columns stay zero.  ranks_used = one past the last column in use.  A single adapter whose block starts
    at column 0 gives exactly the packing without a layout."""
    parts = [p for p in parts if p is not None]
    if not parts:
        pw.lora_a = pw.lora_b = None
        pw.Rp = 0
        return pw
    if layout is None:
        cols, c = [], 0
        for p in parts:
            cols.append(c)
            c += p[2].shape[0]
    else:
        cursor = {n: c0 for n, (c0, _) in layout.items()}
        cols = []
        for p in parts:
            c0, wd = layout[p[5]]
            cols.append(cursor[p[5]])
            cursor[p[5]] += p[2].shape[0]
            if cursor[p[5]] > c0 + wd:
                raise _lib.AldmError(f"attach_lora: adapter {p[5]!r} overflows its column block {layout[p[5]]}")
    rtot = max(c + p[2].shape[0] for c, p in zip(cols, parts))
    rp = 32 if rtot <= 32 else 64
    if rtot > 64:
        raise _lib.AldmError(f"fused LoRA supports a combined rank <= 64 per GEMM (got {rtot})")
    dev = pw.w.device
    a = torch.zeros(rp, pw.Kpad, dtype=torch.bfloat16, device=dev)
    b = torch.zeros(pw.N, rp, dtype=torch.bfloat16, device=dev)
    ln = getattr(pw, "_ln", None) if pw.ln_s is not None else None
    sa = torch.zeros(rp, dtype=torch.float32, device=dev)
    ca = torch.zeros(rp, dtype=torch.float32, device=dev)
    for col, (row0, nrows, A, Bm, s, *_) in zip(cols, parts):
        r, k = A.shape
        Af = A.detach().float()
        if ln is not None:                      # LayerNorm folded: A' = A diag(gamma), sA = row sums, cA = A beta
            Ap = (Af * ln[0][None, :]).to(torch.bfloat16)
            sa[col:col + r] = Ap.float().sum(1)
            ca[col:col + r] = Af @ ln[1]
        else:
            Ap = Af.to(torch.bfloat16)
        a[col:col + r, :k] = Ap
        b[row0:row0 + nrows, col:col + r] = (Bm.detach().float() * s).to(torch.bfloat16)
    pw.lora_a, pw.lora_b, pw.Rp = a.contiguous(), b.contiguous(), rp
    pw.ranks_used = rtot
    if ln is not None:
        pw.ln_sa, pw.ln_ca = sa, ca
    return pw


# How a convolution is launched (tile table, halo rule, tuning key, heuristics, plan()) lives in igemm_plan.py; these names stay
# importable from here.
from . import igemm_plan
from .igemm_plan import (HALO_ROWS, TILE_DIMS, TILE_NAMES, TILES, auto_splits, halo_candidates, heuristic_cfg, parse_key,  # noqa: E402,F401
                         pick_ring, pick_tile, tune_key)


def halo_tiles(OW, eligible):
    """Halo tiles able to take a 3x3/s1/p1 conv whose output is OW wide: BM a multiple of OW and the halo within capacity."""
    return halo_candidates(igemm_plan.Geom(B=1, IH=OW, IW=OW, C1=64, OH=OW, OW=OW, N=64, Kpad=576, Cin=64, KH=3, KW=3, pad=(1, 1))) if eligible else []

# ---- measured launch configurations ------------------------------------------------------------------------------
# "Measure, don't guess": tools/autotune.py picks (tile, ring, splits) per distinct GEMM in two stages and writes
# tuned_gfx950.json next to this file.  Stage 1 times every valid triple on the live operands in isolation and keeps a
# shortlist; stage 2 replays the whole step (all launches queued behind a sleep kernel, so they run back to back as in the
# captured graph) once per shortlist slot and times each GEMM IN CONTEXT -- repeated isolated launches see warm caches
# and mis-rank configurations (a table built from stage 1 alone measured 4.64 ms/step against 4.52 for the heuristics).
# At run time the table is only looked up; GEMMs it does not hold fall back to the heuristics.
TUNED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_gfx950.json")
TUNED = {}
TUNED_LEGACY_KEYS = False
TUNER = None
if os.path.exists(TUNED_PATH) and os.environ.get("ALDM_NO_TUNED") != "1":
    with open(TUNED_PATH) as _f:
        TUNED = {k: tuple(v) for k, v in json.load(_f)["igemm"].items()}
if os.environ.get("ALDM_TUNED_PATCH"):                           # A/B aid: a JSON {key: [tile, ring, splits]} laid over the table
    with open(os.environ["ALDM_TUNED_PATCH"]) as _f:
        TUNED.update({k: tuple(v) for k, v in json.load(_f).items()})
TUNED_LEGACY_KEYS = any(" k3x3 " in k and " ow" not in k for k in TUNED)


class Tuner:
    """Two-stage launch-configuration search driven by tools/autotune.py."""

    def __init__(self, shortlist=5, reps=4, verbose=False):
        self.shortlist, self.reps, self.verbose = shortlist, reps, verbose
        self.cands = {}          # key -> [cfg, ...]   (slot 0 = heuristic)
        self.times = {}          # key -> {cfg: [event pairs]}
        self.slot = None         # stage 2: which shortlist slot this pass runs

    # ---- stage 1 ----
    def isolated(self, key, g, forced_splits, make_args, device, halo=()):
        """g: the launch's igemm_plan.Geom; make_args(): its argument struct, filled except for the launch configuration"""
        lib = _lib.load()
        a = make_args()
        M, N, ktiles = g.M, g.N, g.ktiles
        can_split = g.can_split and forced_splits is None
        default = heuristic_cfg(M, g, ktiles, can_split, g.fast_path, g.vt, forced_splits)
        cands = []
        for t in map(TILES.get, igemm_plan.generic_candidates(g)):
            if g.vt and g.vt_col0 % t.bn:
                continue
            base = math.ceil(M / t.bm) * math.ceil(N / t.bn)
            sp_list = [forced_splits or 1]
            if can_split and base <= 640:
                sp_list += [sp for sp in (2, 3, 4, 6, 8, 12, 16)
                            if sp <= ktiles // 2 and base * sp <= 2560 and sp * M * N * 4 <= (1 << 28)]
            cands += [(t.id, rg, sp) for sp in sp_list for rg in t.rings]
        if forced_splits in (None, 1):
            cands += [(t, rg, 1) for t in halo for rg in TILES[t].rings]
            if can_split and " gi" not in key:              # the halo tiles split by 64-channel chunk (csrc/igemm_halo.hip)
                nch = ktiles // 9
                for t in map(TILES.get, halo):
                    base = math.ceil(M / t.bm) * math.ceil(N / t.bn)
                    cands += [(t.id, rg, sp) for sp in (2, 3, 4, 5, 6, 8, 10) for rg in t.rings[1:]    # (split: the two deeper rings)
                              if sp <= nch and base * sp <= 2560 and sp * M * N * 4 <= (1 << 28)]
        max_sp = max(c[2] for c in cands)
        defer_flags = (_lib.DEFER_ROWMAJOR | (_lib.DEFER_PLANAR if SLAB_LAYOUT == _lib.SLAB_PLANAR else 0)
                       | (_lib.DEFER_WRITE_THROUGH if SLAB_WT else 0))
        ws = _workspace(max_sp * M * N * 4, device) if max_sp > 1 else None
        results = []
        for t, rg, sp in cands:
            a.tile, a.ring, a.splits = t, rg, sp
            a.workspace = ws.data_ptr() if sp > 1 else None
            a.defer_reduce = defer_flags if (sp > 1 and key.endswith(" gn")) else 0   # the consumer GroupNorm pays the reduce
            if lib.aldm_igemm(C.byref(a), _stream()) != 0:              # warm-up doubles as the validity check
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sleep_us(60)                                                 # let the timed launches queue up behind it
            e0.record()
            for _ in range(self.reps):
                lib.aldm_igemm(C.byref(a), _stream())
            e1.record()
            results.append(((t, rg, sp), e0, e1))
        torch.cuda.synchronize()
        ranked = sorted(results, key=lambda r: r[1].elapsed_time(r[2]))
        short = [default] + [r[0] for r in ranked if r[0] != default][: self.shortlist]
        self.cands[key] = short
        if self.verbose:
            print(f"[autotune] {key}: isolated best {ranked[0][0]} {ranked[0][1].elapsed_time(ranked[0][2]) / self.reps * 1e3:.1f} us, "
                  f"default {default}, {len(results)} valid", flush=True)
        return default

    # ---- called by conv() ----
    def choose(self, key, *args):
        if key not in self.cands:
            return self.isolated(key, *args)
        c = self.cands[key]
        return c[self.slot % len(c)] if self.slot is not None else c[0]

    def record(self, key, cfg, e0, e1):
        self.times.setdefault(key, {}).setdefault(cfg, []).append((e0, e1))

    # ---- stage 2 result ----
    def finish(self):
        torch.cuda.synchronize()
        out = {}
        for key, per in self.times.items():
            avg = {cfg: sum(a.elapsed_time(b) for a, b in evs) / len(evs) for cfg, evs in per.items()}
            best = min(avg, key=avg.get)
            default = self.cands[key][0]
            # keep the heuristic unless the measured gain is clear (>3 %): the table then only lists real wins
            if default in avg and avg[best] > 0.97 * avg[default]:
                best = default
            out[key] = (best, avg[best], avg.get(default))
        return out


def save_tuned(path=TUNED_PATH):
    with open(path, "w") as f:
        json.dump({"device": "MI355X gfx950", "format": "key -> [tile, ring, splits]",
                   "igemm": {k: list(v) for k, v in sorted(TUNED.items())}}, f, indent=0)


# Optional launch profiler (bench.py): a list that receives (label, flops, bytes, start_event, end_event, site) per C-ABI call.
# Events are recorded on the stream the kernel is launched on.  SITE tags the launches of one fused-LoRA attention module
# (unet.run_attention) so that bench.py can price the module as a whole.
PROFILE = None
SITE = None

# Multi-adapter routing: the per-sample gate table (fp32 [samples][32], device) of the forward pass in progress.  Every launch with a
# LoRA side channel takes it (UNet2DConditionModel.forward sets it for the duration of a pass); None = ungated launches.
LORA_GATE = None


class lora_gate_scope:
    """with ops.lora_gate_scope(table): every fused-LoRA launch inside reads `table` (None: ungated)."""

    def __init__(self, table):
        self.table = table

    def __enter__(self):
        global LORA_GATE
        self.prev, LORA_GATE = LORA_GATE, self.table
        return self.table

    def __exit__(self, *exc):
        global LORA_GATE
        LORA_GATE = self.prev
        return False


def _gate_for(pw, M, lora_gate, lora_t_out=None):
    """(gate tensor, rows of the GEMM per sample) for a launch over M rows with this weight pack, or (None, 0)"""
    g = lora_gate if lora_gate is not None else LORA_GATE
    if g is None or not pw.Rp:
        if lora_gate is not None:
            raise _lib.AldmError("lora_gate given for a weight pack without an adapter")
        return None, 0
    if lora_t_out is not None:
        raise _lib.AldmError("lora_t_out (the trainer's copy of T) is not combined with a gate table")
    if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.dim() == 2 and g.shape[1] == pw.Rp):
        raise _lib.AldmError(f"gate table must be a contiguous fp32 device tensor [samples][{pw.Rp}] (got {tuple(g.shape)} {g.dtype})")
    if M % g.shape[0]:
        raise _lib.AldmError(f"gate table has {g.shape[0]} rows, which does not divide the launch's {M} rows")
    return g, M // g.shape[0]
KEYLOG = None        # with PROFILE: (row index, (tuning-table key, (tile, ring, splits) used)) of every igemm launch (tools/ab_overlay.py)


def _launch(label, flops, nbytes, fn):
    if PROFILE is None:
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    rc = fn()
    e.record()
    PROFILE.append((label, flops, nbytes, s, e, SITE))
    return rc


_ws_cache = {}


def _workspace(nbytes, device):
    key = (device, torch.cuda.current_stream().cuda_stream)
    t = _ws_cache.get(key)
    if t is None or t.numel() * 4 < nbytes:
        t = torch.empty(max(nbytes // 4, 1 << 22), dtype=torch.float32, device=device)
        _ws_cache[key] = t
    return t


GN_FINALIZE_MIN_TILES = 96          # = ALDM_GN_FINALIZE_MIN_TILES (csrc/norm.hip)


@dataclass
class QStats:
    """GroupNorm statistics a convolution left next to its output (aldm_igemm qstat_out): per M-tile, image slot and 4-channel quad
    the (sum, sum of squares) of the stored values.  Travels as the attribute `.qstats` of the output tensor; groupnorm() then
    runs as one coalesced apply pass (aldm_groupnorm_apply).  bm: rows per generic M-tile; tpi > 0: image-aligned halo tiles."""
    table: torch.Tensor
    bm: int
    tpi: int


QSTATS_MIN_HW = igemm_plan.QSTATS_MIN_HW                   # (read per call: tests lower it)


# aldm_igemm_t.xcd_map: 0 = the library decides per launch which operand an XCD's L2 keeps (weight-stationary where the weight matrix
# is the larger operand), 1 / 2 force activation- / weight-stationary (A/B measurements only).
XCD_MAP = int(os.environ.get("ALDM_XCD_MAP", "0"))


# Form of the standard bf16 epilogue of the unsplit igemm launches (aldm_igemm_t.xcd_map bits 4-5): the plain ones store straight from
# the accumulator registers (no fp32 LDS image, no barrier) unless ALDM_NO_DIRECT_EPI=1 (every launch walks the LDS image, as before).
# `out` is bit-identical either way; the GroupNorm hand-over table differs in the order of its fp32 sums.  conv(epi=) overrides per launch.
EPI_FORM = _lib.EPI_LDS if os.environ.get("ALDM_NO_DIRECT_EPI") == "1" else _lib.EPI_AUTO
EPI_TRACE = None                    # tests / tools: a list that receives aldm_igemm_epilogue_form (1 direct, 0 LDS walk) of every conv() launch


# Layout of the fp32 slabs a split-K launch leaves for a deferred reduce: quad-planar ([split][image][C / 4][HW][4]: what one
# (image, group) workgroup of the consuming GroupNorm reads is contiguous) unless ALDM_NO_SLAB_PLANAR=1 (row-major [split][M][C], the
# layout of every non-deferred split-K launch).  The slab stores of a deferred launch are write-through (the partials drain to memory
# while the kernel still runs instead of at the kernel boundary) unless ALDM_NO_SLAB_WT=1.  Same results bit for bit either way; measured
# in the replayed denoise step: 2.949 ms row-major / plain, 2.930 planar, 2.929 write-through, 2.900 both.
SLAB_LAYOUT = _lib.SLAB_ROWMAJOR if os.environ.get("ALDM_NO_SLAB_PLANAR") == "1" else _lib.SLAB_PLANAR
SLAB_WT = os.environ.get("ALDM_NO_SLAB_WT") != "1"


class Deferred:
    """A split-K convolution whose reduce is still pending (conv(..., defer=True)): the fp32 partial tiles sit in the shared
    workspace, `out` is the bf16 tensor the consumer will fill.  The ONLY valid consumer is the next groupnorm() call on this
    stream -- it sums the tiles, adds bias / row bias / residual, writes `out` and returns the norm; no other split-K conv may
    run in between (the workspace is shared; conv() refuses).  `layout` (_lib.SLAB_*) is how the launch wrote its slabs: a
    consumer either reads that layout or refuses the Deferred."""
    __slots__ = ("out", "ws", "eff", "bias", "rowbias", "rowbias_ld", "res", "keep", "layout")

    def __init__(self, out, ws, eff, bias, rowbias, rowbias_ld, res, keep, layout=_lib.SLAB_ROWMAJOR):
        global DEFERRED_COUNT
        DEFERRED_COUNT += 1
        self.out, self.ws, self.eff, self.bias, self.rowbias, self.rowbias_ld, self.res = out, ws, eff, bias, rowbias, rowbias_ld, res
        self.keep = keep                                   # tensors the pointers above refer to
        self.layout = layout

    @property
    def shape(self):
        return self.out.shape


DEFERRED_COUNT = 0                                         # diagnostics / tests: how many split-K launches deferred their reduce


class _PendingMap(dict):
    """(device, stream) -> the Deferred whose partial tiles currently own THAT stream's split-K workspace.  The workspace is per
    (device, stream) (_workspace), so the producer -> consumer hand-over is too: two engines on two streams (or two devices) never
    see each other's pending reduce."""

    def key(self, t):
        return (t.device.index, torch.cuda.current_stream(t.device).cuda_stream)


_PENDING_BY_STREAM = _PendingMap()


def _pending_get(t):
    return _PENDING_BY_STREAM.get(_PENDING_BY_STREAM.key(t))


def _pending_set(t, d):
    k = _PENDING_BY_STREAM.key(t)
    if d is None:
        _PENDING_BY_STREAM.pop(k, None)
    else:
        _PENDING_BY_STREAM[k] = d


def drop_pending(t=None):
    """Forget a deferred reduce nobody consumed (an exception between producer and consumer): called at the top of a forward with
    that forward's input (its device / current stream); without an argument, every stream's."""
    if t is None:
        _PENDING_BY_STREAM.clear()
    else:
        _pending_set(t, None)


def tensor_of(x):
    """the bf16 tensor behind a conv result (for a Deferred: valid on the stream once its consumer norm has been launched)"""
    return x.out if isinstance(x, Deferred) else x


def _has_qstats(x, x2):
    """Is every source of a gn_in launch a raw convolution output with a statistics table the launch can read?"""
    if not isinstance(x, torch.Tensor) or getattr(x, "qstats", None) is None or x.dim() != 4:
        return False
    if x2 is not None and (not isinstance(x2, torch.Tensor) or getattr(x2, "qstats", None) is None):
        return False
    hw = x.shape[1] * x.shape[2]
    return all(q.tpi > 0 or q.bm <= hw for q in (x.qstats, x2.qstats if x2 is not None else None) if q is not None)


def _igemm_args(g, x, x2, x3, x4, pw, out, *, in_slope, rowbias, rowbias_ld, out_slope, res, res2, post_slope, out2, vt, vt_ld,
                vt_batch_stride, lora_t_out, lora_gate, ln_parts, gn_in):
    """conv()'s aldm_igemm_t with every operand in place; the launch configuration (tile, ring, splits, workspace, statistics tables,
    xcd_map, defer_reduce) is left to the caller.  g: the call's igemm_plan.Geom."""
    a = IgemmArgs()
    if x3 is not None:
        for t in (x3, x4):
            assert t is None or (t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape[:3]) == (g.B, g.OH, g.OW))
        a.x3, a.Cin3 = x3.data_ptr(), g.C3
        if x4 is not None:
            a.x4, a.Cin4 = x4.data_ptr(), g.C4
    a.x, a.x2 = x.data_ptr(), (x2.data_ptr() if x2 is not None else None)
    a.B, a.IH, a.IW, a.Cin, a.Cin2 = g.B, g.IH, g.IW, g.C1, g.C2
    a.UH, a.UW = (g.up_size if g.up_size is not None else (0, 0))
    a.in_dilate = g.in_dilate
    a.w, a.Kpad = pw.w.data_ptr(), pw.Kpad
    a.KH, a.KW = g.KH, g.KW
    a.stride_h, a.stride_w = g.stride
    a.pad_h, a.pad_w = g.pad
    a.dil_h, a.dil_w = g.dil
    a.OH, a.OW, a.Cout = g.OH, g.OW, pw.N
    a.in_act, a.in_slope = g.in_act, in_slope
    if pw.Rp:
        a.lora_a, a.lora_b, a.Rp = pw.lora_a.data_ptr(), pw.lora_b.data_ptr(), pw.Rp
        a.lora_t_out = lora_t_out.data_ptr() if lora_t_out is not None else None
    gate, gate_rows = _gate_for(pw, g.M, lora_gate, lora_t_out)
    if gate is not None:
        a.lora_gate, a.gate_rows = gate.data_ptr(), gate_rows
    a.bias = pw.bias.data_ptr() if pw.bias is not None else None
    if pw.ln_s is not None:
        a.ln_s, a.ln_eps = pw.ln_s.data_ptr(), pw.ln_eps
        if pw.Rp:
            a.ln_sa, a.ln_ca = pw.ln_sa.data_ptr(), pw.ln_ca.data_ptr()
        if ln_parts is not None:
            assert ln_parts.dtype == torch.float32 and ln_parts.is_contiguous() and ln_parts.dim() == 3 and ln_parts.shape[2] == 2
            assert ln_parts.shape[0] == g.B * g.IH * g.IW and g.KH == 1 and g.KW == 1, "ln_parts: one row of partials per GEMM row"
            a.ln_parts, a.ln_nparts = ln_parts.data_ptr(), ln_parts.shape[1]
    elif ln_parts is not None:
        raise _lib.AldmError("conv: ln_parts without a LayerNorm-folded weight pack (pack_linear_ln)")
    if g.rowstats and (g.vt or g.geglu or g.out_f32 or g.out2 or g.N % 64 or g.gn_groups is not None or g.defer):
        raise _lib.AldmError("conv: rowstats needs the standard bf16 epilogue and N % 64 == 0")
    if rowbias is not None:
        assert rowbias.dtype == torch.float32
        a.rowbias, a.rowbias_ld = rowbias.data_ptr(), rowbias_ld
    a.geglu = 1 if pw.geglu else 0
    a.out_act, a.out_slope = g.out_act, out_slope
    a.res = res.data_ptr() if res is not None else None
    a.res2 = res2.data_ptr() if res2 is not None else None
    a.alpha = g.alpha
    a.post_act, a.post_slope = g.post_act, post_slope
    a.out2 = out2.data_ptr() if out2 is not None else None
    a.out, a.out_dtype, a.out_ld = out.data_ptr(), g.out_dtype, g.out_ld
    a.out_batch_stride = g.out_batch_stride
    a.out_pix_stride, a.out_pix_offset = g.out_pix_stride, g.out_pix_offset
    if vt is not None:
        a.vt, a.vt_col0, a.vt_ld, a.vt_batch_stride = vt.data_ptr(), g.vt_col0, vt_ld, vt_batch_stride
        a.vt_dual = 1 if g.vt_dual else 0
    if gn_in is not None:
        # GroupNorm of the input inside the launch: statistics from the producers' tables
        q1, q2 = x.qstats, (x2.qstats if x2 is not None else None)
        gm_, bt_, a.gnin_groups, a.gnin_eps, a.gnin_act = gn_in
        a.gnin_gamma, a.gnin_beta = gm_.data_ptr(), bt_.data_ptr()
        a.gnin_q1, a.gnin_bm1, a.gnin_tpi1 = q1.table.data_ptr(), q1.bm, q1.tpi
        if q2 is not None:
            a.gnin_q2, a.gnin_bm2, a.gnin_tpi2 = q2.table.data_ptr(), q2.bm, q2.tpi
    return a


def conv(x: torch.Tensor, pw: PackedW, *, x2: Optional[torch.Tensor] = None, stride=(1, 1), pad=(0, 0), dil=(1, 1),
         up_size=None, in_dilate=0, out_hw=None, in_act=ACT_NONE, in_slope=0.0, rowbias=None, rowbias_ld=0, out_act=ACT_NONE,
         out_slope=0.0, res=None, res2=None, alpha=1.0, post_act=ACT_NONE, post_slope=0.0, out2=None, out=None, out_f32=False, out_ld=None, out_batch_stride=None,
         out_pix_stride=1, out_pix_offset=0, vt=None, vt_col0=0, vt_ld=0, vt_batch_stride=0, lora_t_out=None,
         splits=None, tile=0, ring=0, gn=None, gn_keep=False, defer=False, rowstats=False, ln_parts=None, x3=None, x4=None,
         vt_dual=False, qstats=False, gn_in=None, lora_gate=None, slab_layout=None, slab_wt=None, epi=None):
    """Implicit-GEMM convolution over channels-last x [B, IH, IW, C1] (+ x2 [B, IH, IW, C2]).

    gn=(gamma, beta, groups, eps, act) returns GroupNorm(+act) of the convolution instead of the convolution: when the launch
    is split-K the partial tiles are summed by the GroupNorm kernel itself (aldm_groupnorm_partials) and the convolution's
    bf16 output is never written (ResnetBlock2D.conv1 -> norm2 -> SiLU).  gn_keep=True returns (convolution, its GroupNorm)
    -- ResnetBlock2D.conv2 (+ shortcut `res`) in front of a Transformer2DModel's norm: the block output stays on the residual
    stream and the fused kernel writes both.  defer=True: the same for a norm that is launched later by the caller -- returns
    a Deferred (see there) when the launch is split-K, else the tensor as usual.

    gn_in=(gamma, beta, groups, eps, act): x (| x2) are RAW convolution outputs carrying `.qstats`; their GroupNorm (+ act) is applied
    inside this launch, on the halo tile's way into LDS (gn_in_ok() says whether a launch can take it; a halo tile is then forced).

    LayerNorm hand-over (BasicTransformerBlock: h -> LayerNorm -> projection): rowstats=True returns (out, stats), stats fp32
    [M, N / BN, 2] = per-row partial (sum, sum of squares) written by the epilogue; a consumer packed with pack_linear_ln takes
    them as ln_parts= and derives mean / rstd from them -- no LayerNorm launch, no statistics pass in either GEMM's K loop.

    slab_layout / slab_wt: layout (_lib.SLAB_*) and store policy of the slabs a deferred split-K launch leaves for its consumer.
    gn= (the consumer is this call's own groupnorm) takes ops.SLAB_LAYOUT; a defer= caller names the layout its consumer reads --
    groupnorm() reads either (the UNet forward passes ops.SLAB_LAYOUT), groupnorm_bwd() reads row-major only, which is the default.
    slab_wt defaults to ops.SLAB_WT.

    epi (default: ops.EPI_FORM): _lib.EPI_AUTO / EPI_LDS / EPI_DIRECT, the form of the standard epilogue (EPI_DIRECT is an error for a
    launch the direct form cannot take; EPI_AUTO walks the LDS image there).

    lora_gate (default: ops.LORA_GATE): fp32 [samples][Rp] per-sample gates of the LoRA side channel's columns (multi-adapter routing)."""
    # ---- checks on the operands
    _require_gpu(x)
    if _pending_get(x) is not None:
        raise _lib.AldmError("conv: a deferred split-K reduce is pending on this stream -- its consumer groupnorm() must be the next launch")
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 4
    B, IH, IW, C1 = x.shape
    C2 = 0
    if x2 is not None:
        assert x2.dtype == torch.bfloat16 and x2.is_contiguous() and x2.shape[:3] == x.shape[:3]
        C2 = x2.shape[3]
    assert C1 + C2 == pw.Cin, f"conv: input channels {C1}+{C2} != packed {pw.Cin}"
    C3 = x3.shape[3] if x3 is not None else 0
    C4 = x4.shape[3] if x4 is not None else 0
    assert C3 + C4 == pw.Cext, f"conv: fused 1x1 segment channels {C3}+{C4} != packed {pw.Cext}"
    assert out_batch_stride is not None or (out_pix_stride == 1 and out_pix_offset == 0), "strided output rows need an explicit batch stride"
    # ---- geometry: the call without its tensors
    g = igemm_plan.geometry(
        (B, IH, IW, C1), pw, C2=C2, C3=C3, C4=C4, x2=x2 is not None, x3=x3 is not None, stride=stride, pad=pad, dil=dil, up_size=up_size,
        in_dilate=in_dilate, out_hw=out_hw, in_act=in_act, vt=vt is not None, vt_dual=bool(vt_dual), vt_col0=vt_col0, rowbias=rowbias is not None,
        res=res is not None, res_numel=(res.numel() if res is not None and res.is_contiguous() else None), res2=res2 is not None,
        out2=out2 is not None, out_act=out_act, post_act=post_act, alpha=alpha, lora_t_out=lora_t_out is not None,
        ln_parts=None if ln_parts is None else ln_parts.shape[1], rowstats=bool(rowstats), qstats=qstats, qstats_min_hw=QSTATS_MIN_HW,
        gn_groups=None if gn is None else gn[2], defer=defer, gn_in=gn_in is not None, tile=tile, ring=ring, splits=splits, out_f32=out_f32,
        out_dtype=None if out is None else (OUT_F32 if out.dtype == torch.float32 else OUT_BF16), out_ld=out_ld,
        out_batch_stride=out_batch_stride, out_pix_stride=out_pix_stride, out_pix_offset=out_pix_offset)
    OH, OW, M = g.OH, g.OW, g.M
    if out is None:
        out = torch.empty(B, OH, OW, g.out_ld, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    if gn_in is not None and not (_has_qstats(x, x2) and halo_candidates(g)):
        raise _lib.AldmError("conv: gn_in needs a 3x3 / stride 1 / pad 1 launch that fits a halo tile and inputs with .qstats (gn_in_ok)")
    # ---- plan: route, tile, ring, splits, the statistics tables (igemm_plan.py)

    def fill():
        return _igemm_args(g, x, x2, x3, x4, pw, out, in_slope=in_slope, rowbias=rowbias, rowbias_ld=rowbias_ld, out_slope=out_slope, res=res,
                           res2=res2, post_slope=post_slope, out2=out2, vt=vt, vt_ld=vt_ld, vt_batch_stride=vt_batch_stride,
                           lora_t_out=lora_t_out, lora_gate=lora_gate, ln_parts=ln_parts, gn_in=gn_in)

    tuning = TUNER is not None and not tile and not ring and not torch.cuda.is_current_stream_capturing()
    p = igemm_plan.plan(g, TUNED, (lambda key, gg, sp, halo: TUNER.choose(key, gg, sp, fill, x.device, halo)) if tuning else None,
                        PGEMM_CFG if PGEMM else None, TUNED_LEGACY_KEYS)
    if p.route == "pgemm":
        return _pgemm(x, pw, out, g.out_ld, M, C1, OH * OW, res, vt, vt_col0, vt_ld, vt_batch_stride, rowstats, ln_parts, lora_t_out, vt_dual,
                      lora_gate=lora_gate)
    key, tile, ring, splits, gn_defer = p.key, p.tile, p.ring, p.splits, p.gn_defer
    # ---- the argument struct: operands, then what the plan decided
    a = fill()
    a.tile, a.ring, a.splits = tile, ring, splits
    a.xcd_map = XCD_MAP | (EPI_FORM if epi is None else epi)
    qs = stats = None
    if p.qstats is not None:
        rows, bm, tpi = p.qstats
        qs = QStats(torch.empty(rows, 2, pw.N // 4, 2, dtype=torch.float32, device=x.device), bm, tpi)
        a.qstat_out = qs.table.data_ptr()
    if p.rowstats_cols is not None:
        stats = torch.empty(M, p.rowstats_cols, 2, dtype=torch.float32, device=x.device)
        a.rowstat_out = stats.data_ptr()
    if splits > 1:
        a.workspace = _workspace(splits * M * pw.N * 4, x.device).data_ptr()
    lib = _lib.load()
    eff = lib.aldm_igemm_effective_splits(C.byref(a)) if (gn_defer and splits > 1) else 1
    layout = _lib.SLAB_ROWMAJOR
    if eff > 1:
        layout = slab_layout if slab_layout is not None else (SLAB_LAYOUT if gn is not None else _lib.SLAB_ROWMAJOR)
    a.defer_reduce = ((_lib.DEFER_ROWMAJOR | (_lib.DEFER_PLANAR if layout == _lib.SLAB_PLANAR else 0)
                       | (_lib.DEFER_WRITE_THROUGH if (SLAB_WT if slab_wt is None else slab_wt) else 0)) if eff > 1 else 0)
    if EPI_TRACE is not None:
        EPI_TRACE.append(lib.aldm_igemm_epilogue_form(C.byref(a)))
    ncols = vt_col0 if (vt is not None and not vt_dual) else (pw.N // 2 if pw.geglu else pw.N)
    ktot = pw.KH * pw.KW * pw.Cin + pw.Cext
    flops = 2.0 * M * pw.N * ktot + (2.0 * M * pw.Rp * (ktot + pw.N) if pw.Rp else 0.0)
    nbytes = 2.0 * (B * IH * IW * pw.Cin + M * pw.Cext + pw.N * ktot + M * ncols)
    label = (f"igemm_{TILE_NAMES[tile]}_r{pw.Rp}{'_vt' if vt is not None else ''}{'_sk' if splits > 1 else ''}"
             f"|M{M} N{pw.N} K{ktot}{' geglu' if pw.geglu else ''}")

    if qs is not None:
        out.qstats = qs                                     # (a Python attribute of this tensor object: skip lists keep the object)
    elif hasattr(out, "qstats"):
        del out.qstats                                      # a caller-supplied buffer rewritten without statistics: drop the stale table

    def finish():
        # the GroupNorm of gn=: over the partial tiles when the launch deferred its reduce, else over the bf16 output
        if gn is None:
            if eff > 1:
                d = Deferred(out, a.workspace, eff, a.bias, a.rowbias, a.rowbias_ld, a.res, (pw, rowbias, res, x3, x4), layout)
                _pending_set(out, d)
                return d
            return (out, stats) if rowstats else out
        gamma, beta, groups, eps, act = gn
        if eff <= 1:
            y = groupnorm(out, gamma, beta, groups, eps, act)
            return (out, y) if gn_keep else y
        y = torch.empty(B, OH, OW, pw.N, dtype=torch.bfloat16, device=x.device)
        n = M * pw.N
        check(_launch(f"groupnorm_partials|HW{OH * OW} C{pw.N} S{eff}", 10.0 * n, (4.0 * eff + 2.0) * n, lambda: lib.aldm_groupnorm_partials_layout(
            a.workspace, eff, B, OH * OW, pw.N, a.bias, a.rowbias, a.rowbias_ld, a.res, (a.out if gn_keep else None), None, 0,
            groups, eps, _p(gamma), _p(beta), act, _p(y), layout, _stream())), "aldm_groupnorm_partials")
        return (out, y) if gn_keep else y

    # ---- launch and finish
    if tuning and TUNER.slot is not None:                      # stage 2 of the tuner: time this launch in context
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = lib.aldm_igemm(C.byref(a), _stream())
        check(rc, "aldm_igemm")
        y = finish() if gn_defer else None                     # a deferred reduce is paid by the GroupNorm: time both
        e1.record()
        TUNER.record(key, (tile, ring, splits), e0, e1)
        return y if gn_defer else finish()
    if KEYLOG is not None and PROFILE is not None:
        KEYLOG.append((len(PROFILE), (key, (tile, ring, splits))))
    check(_launch(label, flops, nbytes, lambda: lib.aldm_igemm(C.byref(a), _stream())), "aldm_igemm")
    return finish()


# ---- the transformer blocks' projection GEMMs (csrc/pgemm.hip) ---------------------------------------------------------------
PGEMM = os.environ.get("ALDM_NO_PGEMM") != "1"
PGEMM_K = igemm_plan.PGEMM_K
PGEMM_CFG = {}                                               # (M, N, K, kind) -> (mi, nt, tiles_per_range): tools/tune_pgemm.py
PGEMM_TUNED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pgemm_gfx950.json")
if os.path.exists(PGEMM_TUNED_PATH) and os.environ.get("ALDM_NO_TUNED") != "1":
    with open(PGEMM_TUNED_PATH) as _f:
        for _k, _v in json.load(_f)["pgemm"].items():
            _m, _n, _kk, _kind = _k.split("|")
            PGEMM_CFG[(int(_m), int(_n), int(_kk), _kind)] = tuple(_v)


if os.environ.get("ALDM_PGEMM_PATCH"):                        # A/B aid: {"M|N|K|kind": [mi, nt, tpr, nw] | null (= no entry: the planner decides)}
    with open(os.environ["ALDM_PGEMM_PATCH"]) as _f:
        for _k, _v in json.load(_f).items():
            _m, _n, _kk, _kind = _k.split("|")
            if _v is None:
                PGEMM_CFG.pop((int(_m), int(_n), int(_kk), _kind), None)
            else:
                PGEMM_CFG[(int(_m), int(_n), int(_kk), _kind)] = tuple(_v)
PGEMM_USE_IGEMM = igemm_plan.PGEMM_USE_IGEMM                 # table entry: this GEMM measured faster on aldm_igemm, keep it there


def _pgemm_key(M, pw, K, res, vt, rowstats=False, lora_t=False, dual=False):
    return igemm_plan.pgemm_key(M, pw.N, K, pw.geglu, vt is not None, res is not None, pw.Rp, rowstats, lora_t, dual)


def _pgemm(x, pw, out, out_ld, M, K, OHW, res, vt, vt_col0, vt_ld, vt_bs, rowstats, ln_parts, lora_t_out=None, vt_dual=False, lora_gate=None):
    """conv()'s 1x1 / short-K case on aldm_pgemm: same operands, same results (to rounding), a kernel built for it."""
    lib = _lib.load()
    a = _lib.PgemmArgs()
    a.x, a.w, a.M, a.N, a.K = x.data_ptr(), pw.w.data_ptr(), M, pw.N, K
    a.bias = pw.bias.data_ptr() if pw.bias is not None else None
    if pw.ln_s is not None:
        assert ln_parts.dtype == torch.float32 and ln_parts.is_contiguous() and ln_parts.dim() == 3 and ln_parts.shape[2] == 2
        assert ln_parts.shape[0] == M, "ln_parts: one row of partials per GEMM row"
        a.ln_s, a.ln_eps, a.ln_parts, a.ln_nparts = pw.ln_s.data_ptr(), pw.ln_eps, ln_parts.data_ptr(), ln_parts.shape[1]
        if pw.Rp:
            a.ln_sa, a.ln_ca = pw.ln_sa.data_ptr(), pw.ln_ca.data_ptr()
    elif ln_parts is not None:
        raise _lib.AldmError("conv: ln_parts without a LayerNorm-folded weight pack (pack_linear_ln)")
    if pw.Rp:
        a.lora_a, a.lora_b, a.Rp, a.ranks_used = pw.lora_a.data_ptr(), pw.lora_b.data_ptr(), pw.Rp, pw.ranks_used
        if lora_t_out is not None:
            assert lora_t_out.dtype == torch.bfloat16 and lora_t_out.is_contiguous() and tuple(lora_t_out.shape) == (M, pw.Rp)
            a.lora_t_out = lora_t_out.data_ptr()
    gate, gate_rows = _gate_for(pw, M, lora_gate, lora_t_out)
    if gate is not None:
        a.lora_gate, a.gate_rows = gate.data_ptr(), gate_rows
    a.geglu = 1 if pw.geglu else 0
    a.res = res.data_ptr() if res is not None else None
    a.out, a.out_ld = out.data_ptr(), out_ld
    if vt is not None:
        a.vt, a.vt_col0, a.vt_ld, a.vt_batch_stride, a.OHW = vt.data_ptr(), vt_col0, vt_ld, vt_bs, OHW
        a.vt_dual = 1 if vt_dual else 0
    cfg = PGEMM_CFG.get(_pgemm_key(M, pw, K, res, vt, rowstats, lora_t_out is not None, vt_dual))
    if cfg is not None and rowstats and pw.N // (cfg[1] * cfg[2]) > 16:
        cfg = None                                           # (consumers take at most 16 partial pairs per row)
    if cfg is not None:
        a.mi, a.nt, a.tiles_per_range = cfg[:3]
        a.waves = cfg[3] if len(cfg) > 3 else 4
    if rowstats:
        a.max_ranges = 16                                    # consumers take at most 16 partial pairs per row (aldm_attn_block64)
    check(lib.aldm_pgemm_plan(C.byref(a)), "aldm_pgemm_plan")
    stats = None
    if rowstats:
        stats = torch.empty(M, pw.N // (a.nt * a.tiles_per_range), 2, dtype=torch.float32, device=x.device)
        a.rowstat_out = stats.data_ptr()
    ncols = pw.N // 2 if pw.geglu else (vt_col0 if (vt is not None and not vt_dual) else pw.N)
    flops = 2.0 * M * pw.N * K + (2.0 * M * pw.Rp * (K + pw.N) if pw.Rp else 0.0)
    nbytes = 2.0 * (M * K + pw.N * K + M * ncols)
    label = (f"pgemm_{16 * a.mi * a.waves}x{a.nt}x{a.tiles_per_range}w{a.waves}_r{pw.Rp}{'_vt' if vt is not None else ''}{'d' if vt_dual else ''}"
             f"|M{M} N{pw.N} K{K}{' geglu' if pw.geglu else ''}")
    if hasattr(out, "qstats"):
        del out.qstats                                       # (see conv(): never leave a stale GroupNorm table on a rewritten buffer)
    if KEYLOG is not None and PROFILE is not None:
        KEYLOG.append((len(PROFILE), ("pg:" + "|".join(str(v) for v in _pgemm_key(M, pw, K, res, vt, rowstats, lora_t_out is not None, vt_dual)),
                                      (a.mi, a.nt, a.tiles_per_range, a.waves))))
    check(_launch(label, flops, nbytes, lambda: lib.aldm_pgemm(C.byref(a), _stream())), "aldm_pgemm")
    return (out, stats) if rowstats else out


def linear(x2d: torch.Tensor, pw: PackedW, **kw):
    """x2d [M, K] bf16 -> [M, N]; thin view over conv with a 1x1 filter."""
    M, K = x2d.shape
    out = kw.pop("out", None)
    y = conv(x2d.view(1, 1, M, K), pw, out=(None if out is None else out), **kw)
    if kw.get("rowstats"):
        return (y[0] if out is not None else y[0].view(M, -1)), y[1]
    return y if out is not None else y.view(M, -1)


def groupnorm(x, gamma, beta, groups, eps, act=ACT_NONE, x2=None):
    """GroupNorm(+SiLU) over channels-last x (| x2).  x may be a Deferred: its split-K reduce then happens here (and fills x.out)."""
    if isinstance(x, Deferred):
        if x is not _pending_get(x.out):
            raise _lib.AldmError("groupnorm: this deferred convolution's partial tiles are gone (not the one pending on this stream)")
        B, H, W, C1 = x.out.shape
        C2 = x2.shape[3] if x2 is not None else 0
        Cg = (C1 + C2) // groups
        if (C1 + C2) % groups or Cg % 4 or C1 % Cg or H * W * (Cg // 4) > 4096:
            raise _lib.AldmError(f"groupnorm: deferred input [{B} x {H * W} x {C1}+{C2} / {groups} groups] does not fit aldm_groupnorm_partials")
        y = torch.empty(B, H, W, C1 + C2, dtype=torch.bfloat16, device=x.out.device)
        lib = _lib.load()
        n = B * H * W * (C1 + C2)
        check(_launch(f"groupnorm_partials|HW{H * W} C{C1}+{C2} S{x.eff}", 10.0 * n, (4.0 * x.eff + 2.0) * n, lambda: lib.aldm_groupnorm_partials_layout(
            x.ws, x.eff, B, H * W, C1, x.bias, x.rowbias, x.rowbias_ld, x.res, _p(x.out), _p(x2), C2, groups, eps,
            _p(gamma), _p(beta), act, _p(y), x.layout, _stream())), "aldm_groupnorm_partials")
        _pending_set(x.out, None)
        return y
    _require_gpu(x)
    B, H, W, C1 = x.shape
    C2 = x2.shape[3] if x2 is not None else 0
    y = torch.empty(B, H, W, C1 + C2, dtype=torch.bfloat16, device=x.device)
    lib = _lib.load()
    n = B * H * W * (C1 + C2)
    q1, q2 = getattr(x, "qstats", None), (getattr(x2, "qstats", None) if x2 is not None else None)
    Cg = (C1 + C2) // groups
    if (q1 is not None and (x2 is None or q2 is not None) and (C1 + C2) % groups == 0 and Cg % 4 == 0
            and C1 % 8 == 0 and C2 % 8 == 0 and groups <= 64 and (C1 + C2) // 8 <= 256
            and x.is_contiguous() and (x2 is None or x2.is_contiguous())):
        # one coalesced pass: the producing convolution(s) handed the statistics over
        # big images (the VAE's mels): the (mean, rstd) table is summed once, by a launch of its own, instead of by every workgroup
        tiles = max(q.tpi if q.tpi > 0 else H * W // q.bm + 1 for q in (q1, q2) if q is not None)
        ws = torch.empty(B, 64, 2, dtype=torch.float32, device=x.device) if tiles >= GN_FINALIZE_MIN_TILES else None
        check(_launch(f"groupnorm_apply|HW{H * W} C{C1 + C2}", 10.0 * n, 4.0 * n, lambda: lib.aldm_groupnorm_apply(
            _p(x), _p(q1.table), q1.bm, q1.tpi, _p(x2), _p(q2.table) if q2 is not None else None, q2.bm if q2 is not None else 0,
            q2.tpi if q2 is not None else 0, B, H * W, C1, C2, groups, eps, _p(gamma), _p(beta), act, _p(y), _p(ws), _stream())),
            "aldm_groupnorm_apply")
        return y
    check(_launch(f"groupnorm|HW{H * W} C{C1 + C2}", 10.0 * n, 4.0 * n, lambda: lib.aldm_groupnorm(
        _p(x), _p(x2), B, H * W, C1, C2, groups, eps, _p(gamma), _p(beta), act, _p(y), _stream())), "aldm_groupnorm")
    return y


def gn_in_ok(x, x2, pw, stride=(1, 1), pad=(1, 1), dil=(1, 1), up_size=None, x3=None):
    """Can a convolution apply the GroupNorm of its input itself (conv(gn_in=))?  Every source a raw convolution output with its statistics
    table, and the launch one a halo tile takes in its gn_in form (igemm_plan.halo_candidates: 3x3 / stride 1 / pad 1, channel counts
    multiples of 64, at most 512 input channels)."""
    if not _has_qstats(x, x2):
        return False
    C2 = x2.shape[3] if x2 is not None else 0
    return bool(halo_candidates(igemm_plan.geometry(tuple(x.shape), pw, C2=C2, x3=x3 is not None, stride=stride, pad=pad, dil=dil,
                                                    up_size=up_size, gn_in=True)))


def gn_silu_conv_out_ok(x, pw, groups):
    """Can conv_norm_out -> SiLU -> conv_out run as the one fused launch?  (the AudioLDM latent: width 16, 128 channels, <= 16 outputs,
    3x3 / pad 1, GroupNorm statistics handed over by the convolution that produced x)"""
    q = getattr(x, "qstats", None) if isinstance(x, torch.Tensor) else None
    return (q is not None and x.dim() == 4 and x.shape[2] == 16 and x.shape[3] == 128 and x.is_contiguous() and x.dtype == torch.bfloat16
            and pw.KH == 3 and pw.KW == 3 and pw.N <= 16 and pw.Cin == 128 and not pw.Rp and 128 % groups == 0 and (128 // groups) % 4 == 0
            and groups <= 64 and (q.tpi > 0 or q.bm <= x.shape[1] * x.shape[2]))


def gn_silu_conv_out(x, gamma, beta, groups, eps, pw):
    """F.silu(F.group_norm(x)) -> 3x3 conv (pad 1) to pw.N channels, fp32 NHWC out, ONE launch (aldm_gn_silu_conv3x3_small)."""
    _require_gpu(x)
    B, H, W, Cc = x.shape
    q = x.qstats
    out = torch.empty(B, H, W, pw.N, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    n = B * H * W
    check(_launch(f"gn_silu_conv3x3|HW{H * W} C{Cc} N{pw.N}", 2.0 * n * pw.N * 9 * Cc + 10.0 * n * Cc, 2.0 * n * Cc + 4.0 * n * pw.N,
                  lambda: lib.aldm_gn_silu_conv3x3_small(_p(x), _p(q.table), q.bm, q.tpi, B, H, W, Cc, groups, eps, _p(gamma), _p(beta), _p(pw.w),
                                                         pw.Kpad, _p(pw.bias), pw.N, _p(out), _stream())), "aldm_gn_silu_conv3x3_small")
    return out


def layernorm(x2d, gamma, beta, eps=1e-5):
    _require_gpu(x2d)
    M, Cc = x2d.shape
    y = torch.empty_like(x2d)
    lib = _lib.load()
    check(_launch(f"layernorm|M{M} C{Cc}", 10.0 * M * Cc, 4.0 * M * Cc, lambda: lib.aldm_layernorm(
        _p(x2d), M, Cc, _p(gamma), _p(beta), eps, _p(y), _stream())), "aldm_layernorm")
    return y


LOG2E = 1.4426950408889634


def attention(qk, vt, B, N, H, d, out=None, kv_len=None, fp8=False, prescaled=False):
    """qk [B*N, 2C] (Q | K), vt [B, C, Npad]; returns [B*N, C].  kv_len: optional int32 [B] valid-key counts
    (right-padded batches).  prescaled: Q already carries d^-0.5 * log2(e) (folded into the to_q weights at pack time)."""
    _require_gpu(qk)
    Cc = H * d
    if out is None:
        out = torch.empty(B * N, Cc, dtype=torch.bfloat16, device=qk.device)
    q_ptr = C.c_void_p(qk.data_ptr())
    k_ptr = C.c_void_p(qk.data_ptr() + Cc * 2)
    lib = _lib.load()
    if kv_len is not None:
        if prescaled or fp8:
            raise _lib.AldmError("attention: the varlen kernel applies d^-0.5 itself and has no fp8 form -- a pre-scaled Q (or "
                                 "fp8=True) with kv_len would be scaled twice / silently ignored")
        assert kv_len.dtype == torch.int32 and kv_len.numel() == B and kv_len.is_cuda
        check(_launch(f"attention_varlen_d{d}_n{N}", 4.0 * B * N * N * Cc, 2.0 * 4 * B * N * Cc, lambda: lib.aldm_attention_varlen(
            q_ptr, qk.shape[1], k_ptr, qk.shape[1], _p(vt), vt.shape[2], vt.stride(0), B, N, H, d, 1.0 / math.sqrt(d),
            _p(kv_len), _p(out), Cc, _stream())), "aldm_attention_varlen")
        return out
    if fp8:                                                   # config 5: e4m3 Q / K / V / P operands
        check(_launch(f"attention_fp8_d{d}_n{N}", 4.0 * B * N * N * Cc, 2.0 * 4 * B * N * Cc, lambda: lib.aldm_attention_fp8(
            q_ptr, qk.shape[1], k_ptr, qk.shape[1], _p(vt), vt.shape[2], vt.stride(0), B, N, H, d,
            (1.0 / LOG2E) if prescaled else 1.0 / math.sqrt(d), _p(out), Cc, _stream())), "aldm_attention_fp8")
        return out
    if prescaled:
        check(_launch(f"attention_d{d}_n{N}", 4.0 * B * N * N * Cc, 2.0 * 4 * B * N * Cc, lambda: lib.aldm_attention_prescaled(
            q_ptr, qk.shape[1], k_ptr, qk.shape[1], _p(vt), vt.shape[2], vt.stride(0), B, N, H, d, _p(out), Cc, _stream())),
            "aldm_attention_prescaled")
        return out
    check(_launch(f"attention_d{d}_n{N}", 4.0 * B * N * N * Cc, 2.0 * 4 * B * N * Cc, lambda: lib.aldm_attention(
        q_ptr, qk.shape[1], k_ptr, qk.shape[1], _p(vt), vt.shape[2], vt.stride(0), B, N, H, d, 1.0 / math.sqrt(d),
        _p(out), Cc, _stream())), "aldm_attention")
    return out


def attn_block64_ok(pw, N, H, d, ln_parts):
    """Can the (sample, head)-fused projection + attention launch take this module?  (C = 640 = 8 x 80, N <= 64, LayerNorm folded
    with the producer's statistics at hand, combined LoRA rank <= 32.)"""
    return (N <= 64 and H == 8 and d == 80 and pw.N == 1920 and pw.Kpad == 640 and pw.ln_s is not None and ln_parts is not None
            and (pw.Rp == 0 or getattr(pw, "ranks_used", 99) <= 32))


# The 252-token level's fused projection + attention launch (csrc/attn_block256.hip) is parity-green and OFF by default: measured in the
# replayed step (round 4, gpurun_out/r4_step_b256.txt) 25.4 us per module against 12.9 + 8.1 us for the projection launch + the attention
# launch.  A (sample, head) workgroup carries 31.5 MFLOP of projection + 12 MFLOP of attention on ONE CU (64 of 256 CUs busy): 4.4 us at
# the MFMA peak of a CU before any latency, where the two launches spread the same work over the whole chip.  ALDM_ATTN_BLOCK256=1 turns it on.
ATTN_BLOCK256 = os.environ.get("ALDM_ATTN_BLOCK256") == "1"


def attn_block_ok(pw, N, H, d, ln_parts):
    """Which (sample, head)-fused projection + attention launch takes this module: 64 (C = 640, N <= 64), 256 (C = 384, N <= 256) or 0."""
    if attn_block64_ok(pw, N, H, d, ln_parts):
        return 64
    if (ATTN_BLOCK256 and N <= 256 and H == 8 and d == 48 and pw.N == 1152 and pw.Kpad == 384 and pw.ln_s is not None and ln_parts is not None
            and ln_parts.shape[1] <= 16 and (pw.Rp == 0 or getattr(pw, "ranks_used", 99) <= 32)):
        return 256
    return 0


def attn_block(x2d, pw, ln_parts, B, N, H, d, fp8=False, lora_gate=None):
    """x2d [B*N, C] raw hidden state -> attention output [B*N, C] through the fused launch attn_block_ok() names (fp8: config 5's e4m3
    attention operands; the 64-token launch has that form, the 256-token one does not)."""
    kind = attn_block_ok(pw, N, H, d, ln_parts)
    if kind == 64:
        return attn_block64(x2d, pw, ln_parts, B, N, H, d, fp8=fp8, lora_gate=lora_gate)
    if fp8:
        raise _lib.AldmError("attn_block: the 256-token fused launch has no fp8 form")
    if kind != 256:
        raise _lib.AldmError(f"attn_block: no fused projection + attention launch for N {N}, {H} heads x {d}")
    _require_gpu(x2d)
    Cc = H * d
    assert x2d.dtype == torch.bfloat16 and x2d.is_contiguous() and tuple(x2d.shape) == (B * N, Cc)
    assert ln_parts.dtype == torch.float32 and ln_parts.is_contiguous() and ln_parts.shape[0] == B * N
    out = torch.empty(B * N, Cc, dtype=torch.bfloat16, device=x2d.device)
    fl = B * (6.0 * N * Cc * Cc + 4.0 * N * N * Cc + (12.0 * N * Cc * getattr(pw, "ranks_used", 0) if pw.Rp else 0.0))
    gate, _ = _gate_for(pw, B, lora_gate)                    # one row per sample: the workgroup's
    if gate is not None and gate.shape[0] != B:
        raise _lib.AldmError(f"gate table has {gate.shape[0]} rows for {B} samples")
    fn = _lib.load().aldm_attn_block256_gated if gate is not None else _lib.load().aldm_attn_block256
    check(_launch(f"attn_block256_d{d}_n{N}", fl, 2.0 * (2 * B * N * Cc + 3 * Cc * Cc), lambda: fn(
        _p(x2d), _p(ln_parts), ln_parts.shape[1], _p(pw.w), pw.Kpad, _p(pw.bias), _p(pw.ln_s), _p(pw.lora_a), _p(pw.lora_b), pw.Rp,
        getattr(pw, "ranks_used", 0) if pw.Rp else 0, _p(pw.ln_sa), _p(pw.ln_ca), pw.ln_eps, B, N, H, d, _p(out), _stream(),
        *(() if gate is None else (_p(gate),)))),
        "aldm_attn_block256")
    return out


def attn_block64(x2d, pw, ln_parts, B, N, H, d, fp8=False, lora_gate=None):
    """x2d [B*N, C] raw hidden state -> attention output [B*N, C]: LayerNorm-folded QKV projection with LoRA + 64-token attention,
    one launch (aldm_attn_block64)."""
    _require_gpu(x2d)
    Cc = H * d
    assert x2d.dtype == torch.bfloat16 and x2d.is_contiguous() and tuple(x2d.shape) == (B * N, Cc)
    assert ln_parts.dtype == torch.float32 and ln_parts.is_contiguous() and ln_parts.shape[0] == B * N
    out = torch.empty(B * N, Cc, dtype=torch.bfloat16, device=x2d.device)
    fl = B * (6.0 * N * Cc * Cc + 4.0 * N * N * Cc + (12.0 * N * Cc * getattr(pw, "ranks_used", 0) if pw.Rp else 0.0))
    gate, _ = _gate_for(pw, B, lora_gate)                    # one row per sample: the workgroup's
    if gate is not None and gate.shape[0] != B:
        raise _lib.AldmError(f"gate table has {gate.shape[0]} rows for {B} samples")
    fn = getattr(_lib.load(), "aldm_attn_block64" + ("_fp8" if fp8 else "") + ("_gated" if gate is not None else ""))
    check(_launch(f"attn_block64{'_fp8' if fp8 else ''}_d{d}_n{N}", fl, 2.0 * (2 * B * N * Cc + 3 * Cc * Cc), lambda: fn(
        _p(x2d), _p(ln_parts), ln_parts.shape[1], _p(pw.w), pw.Kpad, _p(pw.bias), _p(pw.ln_s), _p(pw.lora_a), _p(pw.lora_b), pw.Rp,
        getattr(pw, "ranks_used", 0) if pw.Rp else 0, _p(pw.ln_sa), _p(pw.ln_ca), pw.ln_eps, B, N, H, d, _p(out), _stream(),
        *(() if gate is None else (_p(gate),)))),
        "aldm_attn_block64")
    return out


HIFIGAN_PAIR = os.environ.get("ALDM_NO_HIFIGAN_PAIR") != "1"        # A/B aid: the vocoder's low-channel stages back on aldm_igemm


def hifigan_respair_ok(x, c1, c2, dil):
    """Can one aldm_hifigan_respair launch take this (convs1[q], convs2[q]) pair?  (C = 32 / 64 channels, 3 / 7 / 11 taps, dilation <= 5.)"""
    Cc = x.shape[3]
    return (HIFIGAN_PAIR and x.shape[1] == 1 and c1.N == Cc and c2.N == Cc and c1.Cin == Cc and c2.Cin == Cc and c1.KH == 1 and c2.KH == 1
            and c1.KW == c2.KW and c1.bias is not None and c2.bias is not None
            and bool(_lib.load().aldm_hifigan_respair_supported(Cc, c1.KW, dil)))


def hifigan_respair(x, c1, c2, dil, slope, alpha=1.0, res2=None, post_act=ACT_NONE, post_slope=0.0):
    """x [B, 1, T, C] bf16 residual stream -> post_act(alpha (x + conv2(lrelu(conv1(lrelu(x))))) + res2), one launch."""
    _require_gpu(x)
    B, _, T, Cc = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and (res2 is None or (res2.shape == x.shape and res2.is_contiguous()))
    out = torch.empty_like(x)
    K = c1.KW
    fl = 2.0 * 2.0 * B * T * Cc * Cc * K
    check(_launch(f"hifigan_pair_c{Cc}_k{K}_d{dil}|M{B * T}", fl, 2.0 * B * T * Cc * (2 + (1 if res2 is not None else 0)), lambda: _lib.load().aldm_hifigan_respair(
        _p(x), B, T, Cc, _p(c1.w), c1.Kpad, _p(c1.bias), dil, _p(c2.w), c2.Kpad, _p(c2.bias), K, slope, alpha, _p(res2), post_act, post_slope,
        _p(out), _stream())), "aldm_hifigan_respair")
    return out


def conv1d_to1(x, pw, act=ACT_NONE):
    """x [B, 1, T, C] bf16 (activated) -> fp32 [B, T]: Conv1d(C -> 1, K taps, same padding) (+ tanh) as one HBM-bound stencil launch.
    pw = ops.pack_conv of the [1 (padded to 8), C, 1, K] weight: row 0 holds the filter in (tap, cin) order."""
    _require_gpu(x)
    B, _, T, Cc = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and pw.Cin == Cc and pw.KH == 1
    out = torch.empty(B, T, dtype=torch.float32, device=x.device)
    check(_launch(f"conv1d_to1_c{Cc}_k{pw.KW}|M{B * T}", 2.0 * B * T * Cc * pw.KW, 2.0 * B * T * Cc + 4.0 * B * T, lambda: _lib.load().aldm_conv1d_to1(
        _p(x), B, T, Cc, _p(pw.w), _p(pw.bias), pw.KW, act, _p(out), _stream())), "aldm_conv1d_to1")
    return out


WIDE_HEAD_DIMS = (128, 256, 512)


def attention_wide(qk, vt, B, N, d, out=None):
    """Single wide head (AutoencoderKL mid-block): qk [B*N, 2d] (pre-scaled Q | K), vt [B, d, npad] zero beyond N, npad % 32 == 0."""
    _require_gpu(qk)
    assert d in WIDE_HEAD_DIMS and vt.shape[2] % 32 == 0 and vt.shape[2] >= N
    if out is None:
        out = torch.empty(B * N, d, dtype=torch.bfloat16, device=qk.device)
    check(_launch(f"attention_wide_d{d}_n{N}", 4.0 * B * N * N * d, 2.0 * 4 * B * N * d, lambda: _lib.load().aldm_attention_wide(
        C.c_void_p(qk.data_ptr()), qk.shape[1], C.c_void_p(qk.data_ptr() + 2 * d), qk.shape[1], _p(vt), vt.shape[2], vt.stride(0),
        B, N, d, _p(out), d, _stream())), "aldm_attention_wide")
    return out


def embed_layernorm(ids, word, pos, type0, gamma, beta, eps, pad_idx):
    """ids int64 [B, L] (device) -> LayerNorm(word[ids] + type0 + pos[position_ids]) as bf16 [B*L, C]."""
    _require_gpu(ids)
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    B, L = ids.shape
    Cc = word.shape[1]
    for t in (word, pos, type0, gamma, beta):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
    y = torch.empty(B * L, Cc, dtype=torch.bfloat16, device=ids.device)
    check(_lib.load().aldm_embed_layernorm(_p(ids), B, L, Cc, _p(word), word.shape[0], _p(pos), pos.shape[0], _p(type0),
                                           _p(gamma), _p(beta), eps, pad_idx, _p(y), _stream()), "aldm_embed_layernorm")
    return y


def softmax_rows(s, scale, cols, ld_out):
    rows = s.shape[0]
    p = torch.empty(rows, ld_out, dtype=torch.bfloat16, device=s.device)
    check(_lib.load().aldm_softmax_rows(_p(s), rows, cols, s.shape[1], scale, _p(p), ld_out, _stream()),
          "aldm_softmax_rows")
    return p


def timestep_embedding(t_dev, B, dim):
    out = torch.empty(B, dim, dtype=torch.bfloat16, device=t_dev.device)
    stride = 0 if t_dev.numel() == 1 else 1
    check(_lib.load().aldm_timestep_embedding(_p(t_dev), stride, B, dim, _p(out), _stream()), "aldm_timestep_embedding")
    return out


def nchw_to_nhwc(x_f32, out_f32=False):
    _require_gpu(x_f32)
    B, Cc, H, W = x_f32.shape
    y = torch.empty(B, H, W, Cc, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x_f32.device)
    check(_lib.load().aldm_nchw_f32_to_nhwc(_p(x_f32.contiguous()), B, Cc, H * W, _p(y), int(out_f32), _stream()),
          "aldm_nchw_f32_to_nhwc")
    return y


def nhwc_to_nchw_f32(x):
    _require_gpu(x)
    B, H, W, Cc = x.shape
    y = torch.empty(B, Cc, H, W, dtype=torch.float32, device=x.device)
    check(_lib.load().aldm_nhwc_to_nchw_f32(_p(x.contiguous()), int(x.dtype == torch.float32), B, Cc, H * W, _p(y),
                                            _stream()), "aldm_nhwc_to_nchw_f32")
    return y


def f32_to_bf16(x, mul=1.0, out=None):
    _require_gpu(x)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(_lib.load().aldm_f32_to_bf16(_p(x), x.numel(), mul, _p(out), _stream()), "aldm_f32_to_bf16")
    return out


def cfg_ddim_step(eps, x, cfg, guidance, coef, step_idx, x_in):
    B = x.shape[0]
    n = x.numel() // B
    check(_launch("cfg_ddim_step", 6.0 * x.numel(), (4.0 * (2 if cfg else 1) + 8.0 + 2.0 * (2 if cfg else 1)) * x.numel(),
                  lambda: _lib.load().aldm_cfg_ddim_step(_p(eps), _p(x), B, n, int(cfg), guidance, _p(coef), _p(step_idx), _p(x_in),
                                                          _stream())), "aldm_cfg_ddim_step")


def _inpaint_args(x, x0, noise, mask, blend, n_steps, noise_optional=False):
    """checks the masked steps' extra operands; returns the channel count (x is channels-last [B, h, w, C]).  noise_optional: the
    solver draws the blend's noise itself (RePaint), so `noise` may be None"""
    C = x.shape[-1]
    assert noise is not None or noise_optional, "noise: the eps the loop started from"
    for t in (x0, mask, blend) + (() if noise is None else (noise,)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.device == x.device
    assert x0.numel() == x.numel() and (noise is None or noise.numel() == x.numel()) and mask.numel() * C == x.numel(), "x0 / noise / mask geometry"
    assert blend.dim() == 2 and blend.shape == (n_steps, 2), "blend rows [n_steps, 2]"
    return C


# solver -> (columns of its coefficient table, flops per element, bytes per element beside the frame's, ticket may be None)
#   dpm: hist read/write (upper bound: second-order rows); euler_a: ~100 flops for ten Philox rounds and a Box-Muller, no noise tensor;
#   unipc: last, m0, m1 read and last, m_t written (upper bound: second-order corrector rows); repaint (masked only): two Philox
#   blocks and Box-Mullers on rows with a jump, one on the others (upper bound), and the blend's noise is not read (-4 B)
_STEP_SOLVERS = {"ddim": (4, 6.0, 0.0, False), "dpm": (8, 10.0, 8.0, True), "euler_a": (4, 110.0, 0.0, True),
                 "unipc": (16, 22.0, 20.0, True), "repaint": (8, 212.0, -4.0, True)}


def _step_fused(solver, eps, x, cfg, guidance, coef, step_idx, x_in, operand, table, rowbias, timesteps_f32, t_out, ticket, inpaint=None):
    """The frame the eight fused scheduler steps share (csrc/elementwise.hip step_fused_body / launch_step_fused): the checks, the
    flops / bytes model and the launch of aldm_<solver>_step_fused[_masked].  operand: the solver's extra tensors, () or a 1-tuple;
    inpaint: None or (x0, noise, mask, blend)."""
    coef_cols, flops, solver_bytes, ticket_optional = _STEP_SOLVERS[solver]
    _require_gpu(x)
    B = x.shape[0]
    n = x.numel() // B
    halves = 2 if cfg else 1
    row = table[0].numel() if table is not None else 0
    assert coef.dtype == torch.float32 and coef.dim() == 2 and coef.shape[1] == coef_cols and step_idx.dtype == torch.int32
    assert eps.numel() == x.numel() * halves
    assert (ticket_optional and ticket is None) or (ticket.dtype == torch.int32 and timesteps_f32 is not None and t_out is not None)
    n_steps = timesteps_f32.numel() if timesteps_f32 is not None else coef.shape[0]
    name = f"{solver}_step_fused"
    # bytes per element: eps (1 or 2 halves) + x read/write + the solver's, + bf16 UNet input (1 or 2 halves) at the end
    per_elem = 4.0 * halves + 8.0 + solver_bytes
    tail = ()
    if inpaint is not None:
        C = _inpaint_args(x, *inpaint, n_steps, noise_optional=solver == "repaint")
        name, flops = name + "_masked", flops + 4.0
        per_elem = per_elem + 8.0 + 4.0 / C                  # x0 and noise (4 B each) and the mask (4 B per pixel)
        tail = (*map(_p, inpaint), C)
    fn = getattr(_lib.load(), "aldm_" + name)
    check(_launch(name, flops * x.numel(), (per_elem + 2.0 * halves) * x.numel() + 8.0 * row,
                  lambda: fn(_p(eps), _p(x), B, n, int(cfg), guidance, _p(coef), _p(step_idx), _p(x_in), *map(_p, operand), _p(table), row,
                             _p(rowbias), _p(timesteps_f32), n_steps, _p(t_out), _p(ticket), *tail, _stream())), "aldm_" + name)


def ddim_step_fused(eps, x, cfg, guidance, coef, step_idx, x_in, table, rowbias, timesteps_f32, t_out, ticket):
    """cfg_ddim_step + gather_row(next step) + advance_step as one launch (aldm_ddim_step_fused)."""
    _step_fused("ddim", eps, x, cfg, guidance, coef, step_idx, x_in, (), table, rowbias, timesteps_f32, t_out, ticket)


def dpm_step_fused(eps, x, cfg, guidance, coef, step_idx, x_in, hist, table=None, rowbias=None, timesteps_f32=None, t_out=None,
                   ticket=None):
    """CFG + DPM-Solver(++) multistep update (+ gather_row(next step) + advance_step when `ticket` is given) as one launch
    (aldm_dpm_step_fused).  coef fp32 [n_steps, 8] (DPMSolverMultistepScheduler.coefficient_table); hist fp32, x's shape: the
    previous step's converted model output, read by second-order rows and overwritten.  ticket None: eager, the counter stays."""
    assert hist.dtype == torch.float32 and hist.numel() == x.numel()
    _step_fused("dpm", eps, x, cfg, guidance, coef, step_idx, x_in, (hist,), table, rowbias, timesteps_f32, t_out, ticket)


def ddim_step_fused_masked(eps, x, cfg, guidance, coef, step_idx, x_in, table, rowbias, timesteps_f32, t_out, ticket, x0, noise, mask, blend):
    """ddim_step_fused followed by the inpainting blend (aldm_ddim_step_fused_masked): x' = (1 - m) (a x0 + s noise) + m x_ddim with
    (a, s) = blend[step_idx].  x, x0, noise fp32 [B, h, w, C]; mask fp32 [B, h, w] (1 = regenerate); blend fp32 [n_steps, 2]."""
    _step_fused("ddim", eps, x, cfg, guidance, coef, step_idx, x_in, (), table, rowbias, timesteps_f32, t_out, ticket, (x0, noise, mask, blend))


def dpm_step_fused_masked(eps, x, cfg, guidance, coef, step_idx, x_in, hist, table, rowbias, timesteps_f32, t_out, ticket, x0, noise, mask,
                          blend):
    """dpm_step_fused followed by the inpainting blend (aldm_dpm_step_fused_masked); operands as ddim_step_fused_masked.  hist
    receives the unblended converted model output.  ticket None: eager, the counter stays (table must be None then)."""
    assert hist.dtype == torch.float32 and hist.numel() == x.numel()
    _step_fused("dpm", eps, x, cfg, guidance, coef, step_idx, x_in, (hist,), table, rowbias, timesteps_f32, t_out, ticket,
                (x0, noise, mask, blend))


def _check_unipc_state(state, x):
    assert state.dtype == torch.float32 and state.is_contiguous() and state.device == x.device, "unipc state: contiguous fp32 on x's device"
    assert state.dim() >= 1 and state.shape[0] == 3 and state.numel() == 3 * x.numel(), "unipc state: [3, *x.shape]"


def unipc_step_fused(eps, x, cfg, guidance, coef, step_idx, x_in, state, table=None, rowbias=None, timesteps_f32=None, t_out=None,
                     ticket=None):
    """CFG + UniPC predictor-corrector update (+ gather_row(next step) + advance_step when `ticket` is given) as one launch
    (aldm_unipc_step_fused).  coef fp32 [n_steps, 16] (UniPCMultistepScheduler.coefficient_table); state fp32 [3, *x.shape]: the last
    corrected sample and the two previous converted model outputs, a ring turned by the parity of step_idx (include/aldm_hip.h).
    ticket None: eager, the counter stays (the caller alternates it between 0 and 1)."""
    _check_unipc_state(state, x)
    _step_fused("unipc", eps, x, cfg, guidance, coef, step_idx, x_in, (state,), table, rowbias, timesteps_f32, t_out, ticket)


def unipc_step_fused_masked(eps, x, cfg, guidance, coef, step_idx, x_in, state, table, rowbias, timesteps_f32, t_out, ticket, x0, noise, mask,
                            blend):
    """unipc_step_fused followed by the inpainting blend (aldm_unipc_step_fused_masked); operands as ddim_step_fused_masked.  state
    receives unblended values.  ticket None: eager, the counter stays (table must be None then)."""
    _check_unipc_state(state, x)
    _step_fused("unipc", eps, x, cfg, guidance, coef, step_idx, x_in, (state,), table, rowbias, timesteps_f32, t_out, ticket,
                (x0, noise, mask, blend))


# ---- on-device RNG (csrc/rng.hip, csrc/philox.h) -----------------------------------------------------------------------------
def _u32_words(v):
    """a 64-bit unsigned value as two int32 bit patterns (torch has no uint32 arithmetic; the kernels read the words as unsigned)"""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return [w - (1 << 32) if w >= (1 << 31) else w for w in (v & 0xFFFFFFFF, v >> 32)]


def philox_state(seed, draw=0, device="cuda"):
    """The Philox stream state the RNG kernels read: int32 [4] on the device holding the bit patterns {seed_lo, seed_hi, draw_lo,
    draw_hi} -- a 64-bit seed (the key) and the 64-bit ordinal of the next tensor-sized draw."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.AldmError("the product path runs on the MI355X only (philox_state on a CPU device); there is no CPU fallback")
    return torch.tensor(_u32_words(seed) + _u32_words(draw), dtype=torch.int32, device=dev)


def philox_state_values(state):
    """(seed, draw) of a philox_state as Python ints (synchronises; for tests and logs)"""
    w = [int(v) & 0xFFFFFFFF for v in state.cpu().tolist()]
    return w[0] | (w[1] << 32), w[2] | (w[3] << 32)


def philox_set(state, seed=None, draw=None):
    """Sets the seed and / or the draw ordinal of a philox_state IN PLACE (the tensor keeps its address, so a captured graph that
    reads it goes on from the new values)."""
    _check_state(state)
    if seed is not None:
        state[:2].copy_(torch.tensor(_u32_words(seed), dtype=torch.int32))
    if draw is not None:
        state[2:].copy_(torch.tensor(_u32_words(draw), dtype=torch.int32))
    return state


def _check_state(state):
    _require_gpu(state)
    assert state.dtype == torch.int32 and state.numel() == 4 and state.is_contiguous(), "philox state: int32 [4] (ops.philox_state)"


def philox_u32(n, state, first_block=0):
    """n raw Philox4x32-10 words of the state's current draw, from block `first_block` (element 4 * first_block) on, as int32 bit
    patterns [n] (aldm_philox_u32); the state stays."""
    _check_state(state)
    out = torch.empty(int(n), dtype=torch.int32, device=state.device)
    check(_lib.load().aldm_philox_u32(_p(out), int(n), _p(state), int(first_block) & 0xFFFFFFFFFFFFFFFF, _stream()), "aldm_philox_u32")
    return out


def randn(shape, state, advance=True):
    """fp32 standard normals of `shape` from the state's current draw (aldm_randn): element i of the flattened tensor is element i of
    the draw, whatever the shape.  advance: the draw ordinal grows by 1 on the device, so the next call draws a new tensor."""
    _check_state(state)
    out = torch.empty(shape, dtype=torch.float32, device=state.device)
    check(_lib.load().aldm_randn(_p(out), out.numel(), _p(state), int(bool(advance)), _stream()), "aldm_randn")
    return out


def euler_a_step_fused(eps, x, cfg, guidance, coef, step_idx, x_in, rng_state, table=None, rowbias=None, timesteps_f32=None, t_out=None,
                       ticket=None):
    """CFG + Euler-ancestral update with the noise drawn in the kernel from rng_state (+ gather_row(next step) + advance_step + the
    draw ordinal's advance when `ticket` is given) as one launch (aldm_euler_a_step_fused).  coef fp32 [n_steps, 4]
    (EulerAncestralDiscreteScheduler.coefficient_table); x fp32, unscaled (sigma space); x_in receives bf16(x' * in_scale_next).
    ticket None: the counter and the ordinal stay."""
    _check_state(rng_state)
    _step_fused("euler_a", eps, x, cfg, guidance, coef, step_idx, x_in, (rng_state,), table, rowbias, timesteps_f32, t_out, ticket)


def euler_a_step_fused_masked(eps, x, cfg, guidance, coef, step_idx, x_in, rng_state, table, rowbias, timesteps_f32, t_out, ticket, x0, noise,
                              mask, blend):
    """euler_a_step_fused followed by the inpainting blend (aldm_euler_a_step_fused_masked); operands as ddim_step_fused_masked, blend
    rows (1, sigma_next).  ticket None: the counter and the ordinal stay (table must be None then)."""
    _check_state(rng_state)
    _step_fused("euler_a", eps, x, cfg, guidance, coef, step_idx, x_in, (rng_state,), table, rowbias, timesteps_f32, t_out, ticket,
                (x0, noise, mask, blend))


def repaint_step_fused_masked(eps, x, cfg, guidance, coef, step_idx, x_in, rng_state, table, rowbias, timesteps_f32, t_out, ticket, x0, noise,
                              mask, blend):
    """CFG + one RePaint step as one launch (aldm_repaint_step_fused_masked): the DDIM update, the inpainting
    blend whose known part is noised with FRESH noise zk, and the closed-form jump x' = c1 xb + c2 zj.  coef fp32 [n_steps, 8]
    (RePaintScheduler.coefficient_table), blend fp32 [n_steps, 2] (RePaintScheduler.blend_table).  With the ordinal of rng_state at
    d, zk is draw d and zj draw d + 1 (the bits of ops.randn); with a ticket the ordinal ends at d + 2, on every row.  `noise` is not
    read and may be None.  mask: 1 = regenerate.  ticket None: the counter and the ordinal stay (table must be None then)."""
    _check_state(rng_state)
    _step_fused("repaint", eps, x, cfg, guidance, coef, step_idx, x_in, (rng_state,), table, rowbias, timesteps_f32, t_out, ticket,
                (x0, noise, mask, blend))


# ---- windowed denoising: long-form and loopable generation (csrc/elementwise.hip, longform.py) ------------
def _window_plan(plan):
    """aldm_window_plan_t of a plan's device tables (longform.WindowPlan.device(): offset int32 [K], cover int32 [rows, KC], weight
    fp32 [rows, KC] and K, KC, rows, hw).  What the tables hold goes along as counted here, so the launcher itself rejects tables
    that do not fit the plan."""
    for t, dt in ((plan.offset, torch.int32), (plan.cover, torch.int32), (plan.weight, torch.float32)):
        _require_gpu(t)
        assert t.dtype == dt and t.is_contiguous(), "window plan tables: contiguous int32 offset / cover and fp32 weight on the device"
    return _lib.WindowPlanArgs(plan.offset.data_ptr(), plan.cover.data_ptr(), plan.weight.data_ptr(), int(plan.K), int(plan.KC),
                               int(plan.rows), int(plan.hw), plan.offset.numel(), plan.cover.numel(), plan.weight.numel())


def window_gather(x, plan, mul=1.0, out_f32=False, out=None):
    """Windows out of a long tensor (aldm_window_gather): x fp32 [B, rows, W, C] -> [B * K, hw, W, C], window k of clip b at batch row
    b * K + k, rows taken modulo `rows`.  bf16(x * mul) -- the rounding of f32_to_bf16 -- or fp32 (out_f32)."""
    _require_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 2
    B = x.shape[0]
    shape = (B * int(plan.K), int(plan.hw)) + tuple(x.shape[2:])
    dt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty(shape, dtype=dt, device=x.device)
    assert out.dtype == dt and out.is_contiguous() and tuple(out.shape) == shape
    args = _window_plan(plan)
    check(_launch("window_gather", 0.0, (4.0 + (4.0 if out_f32 else 2.0)) * out.numel(),
                  lambda: _lib.load().aldm_window_gather(_p(x), B, x.numel() // B, float(mul), _p(out), int(out_f32), C.byref(args), _stream())),
          "aldm_window_gather")
    return out


def window_blend(win, plan, out=None):
    """Windows back into a long tensor (aldm_window_blend): win fp32 [B * K, hw, W, C] -> [B, rows, W, C], every long row the
    weighted sum of the windows over it (weight[r][0] * win_0, then fused multiply-adds in table order)."""
    _require_gpu(win)
    assert win.dtype == torch.float32 and win.is_contiguous() and win.dim() >= 2 and win.shape[0] % int(plan.K) == 0
    B = win.shape[0] // int(plan.K)
    shape = (B, int(plan.rows)) + tuple(win.shape[2:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=win.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape
    args = _window_plan(plan)
    check(_launch("window_blend", 2.0 * win.numel(), 4.0 * (win.numel() + out.numel()),
                  lambda: _lib.load().aldm_window_blend(_p(win), B, out.numel() // B, _p(out), C.byref(args), _stream())),
          "aldm_window_blend")
    return out


def _step_fused_windowed(solver, eps, x, cfg, guidance, coef, step_idx, x_in, operand, table, rowbias, timesteps_f32, t_out, ticket, plan,
                         inpaint=None):
    """The frame of the four windowed fused steps (launch_step_fused_windowed): _step_fused's checks with eps and x_in per window.
    x fp32 [B, rows, W, C] long; eps fp32 [halves * B * K, hw, W, C]; x_in bf16 of eps's shape (or None).  inpaint: None or the LONG
    (x0, noise, mask, blend) of aldm_<solver>_step_fused_windowed_masked."""
    coef_cols, flops, solver_bytes, ticket_optional = _STEP_SOLVERS[solver]
    _require_gpu(x)
    B = x.shape[0]
    n = x.numel() // B
    halves = 2 if cfg else 1
    row = table[0].numel() if table is not None else 0
    assert coef.dtype == torch.float32 and coef.dim() == 2 and coef.shape[1] == coef_cols and step_idx.dtype == torch.int32
    assert x.dtype == torch.float32 and x.is_contiguous() and eps.dtype == torch.float32 and eps.is_contiguous()
    win_elems = B * int(plan.K) * int(plan.hw) * (n // max(1, int(plan.rows)))
    assert eps.numel() == win_elems * halves, "eps: [halves * B * K, hw, W, C]"
    assert x_in is None or (x_in.dtype == torch.bfloat16 and x_in.is_contiguous() and x_in.numel() == eps.numel()), "x_in: bf16 of eps's shape"
    assert (ticket_optional and ticket is None) or (ticket.dtype == torch.int32 and timesteps_f32 is not None and t_out is not None)
    n_steps = timesteps_f32.numel() if timesteps_f32 is not None else coef.shape[0]
    name = f"{solver}_step_fused_windowed"
    args = _window_plan(plan)
    flops = flops + 4.0 * halves
    long_bytes = 8.0 + solver_bytes
    tail = ()
    if inpaint is not None:
        assert x.dim() >= 2, "x: channels-last [B, rows, W, C]"
        ch = _inpaint_args(x, *inpaint, n_steps, noise_optional=solver == "repaint")
        name, flops = name + "_masked", flops + 4.0
        long_bytes = long_bytes + 8.0 + 4.0 / ch             # the three extra long reads: x0 and noise (4 B each), the mask (4 B per pixel)
        tail = (*map(_p, inpaint), ch)
    fn = getattr(_lib.load(), "aldm_" + name)
    # bytes: every window's eps and bf16 input (1 or 2 halves), x read / write and the solver's per long element, the table row
    check(_launch(name, flops * x.numel(), 6.0 * eps.numel() + long_bytes * x.numel() + 8.0 * row,
                  lambda: fn(_p(eps), _p(x), B, n, int(cfg), guidance, _p(coef), _p(step_idx), _p(x_in), *map(_p, operand), _p(table), row,
                             _p(rowbias), _p(timesteps_f32), n_steps, _p(t_out), _p(ticket), C.byref(args), *tail, _stream())), "aldm_" + name)


def ddim_step_fused_windowed(eps, x, cfg, guidance, coef, step_idx, x_in, table, rowbias, timesteps_f32, t_out, ticket, plan):
    """ddim_step_fused on a long latent with eps and x_in per window (aldm_ddim_step_fused_windowed): the windows' eps halves are
    blended into the long row, the update runs on the blend, and the next UNet input is stored into every window over the row."""
    _step_fused_windowed("ddim", eps, x, cfg, guidance, coef, step_idx, x_in, (), table, rowbias, timesteps_f32, t_out, ticket, plan)


def dpm_step_fused_windowed(eps, x, cfg, guidance, coef, step_idx, x_in, hist, table, rowbias, timesteps_f32, t_out, ticket, plan):
    """dpm_step_fused on a long latent (aldm_dpm_step_fused_windowed); hist fp32 in x's long shape."""
    assert hist.dtype == torch.float32 and hist.numel() == x.numel()
    _step_fused_windowed("dpm", eps, x, cfg, guidance, coef, step_idx, x_in, (hist,), table, rowbias, timesteps_f32, t_out, ticket, plan)


def unipc_step_fused_windowed(eps, x, cfg, guidance, coef, step_idx, x_in, state, table, rowbias, timesteps_f32, t_out, ticket, plan):
    """unipc_step_fused on a long latent (aldm_unipc_step_fused_windowed); state fp32 [3, *x.shape], long."""
    _check_unipc_state(state, x)
    _step_fused_windowed("unipc", eps, x, cfg, guidance, coef, step_idx, x_in, (state,), table, rowbias, timesteps_f32, t_out, ticket, plan)


def euler_a_step_fused_windowed(eps, x, cfg, guidance, coef, step_idx, x_in, rng_state, table, rowbias, timesteps_f32, t_out, ticket, plan):
    """euler_a_step_fused on a long latent (aldm_euler_a_step_fused_windowed): element i of the LONG latent is element i of the draw."""
    _check_state(rng_state)
    _step_fused_windowed("euler_a", eps, x, cfg, guidance, coef, step_idx, x_in, (rng_state,), table, rowbias, timesteps_f32, t_out, ticket, plan)


def ddim_step_fused_windowed_masked(eps, x, cfg, guidance, coef, step_idx, x_in, table, rowbias, timesteps_f32, t_out, ticket, plan, x0, noise,
                                    mask, blend):
    """ddim_step_fused_windowed followed by the inpainting blend on the long latent, before the scatter
    (aldm_ddim_step_fused_windowed_masked).  x0, noise fp32 [B, rows, W, C] and mask fp32 [B, rows, W] are long like x; blend fp32
    [n_steps, 2].  Every covering window receives the bf16 of the BLENDED value."""
    _step_fused_windowed("ddim", eps, x, cfg, guidance, coef, step_idx, x_in, (), table, rowbias, timesteps_f32, t_out, ticket, plan,
                         (x0, noise, mask, blend))


def dpm_step_fused_windowed_masked(eps, x, cfg, guidance, coef, step_idx, x_in, hist, table, rowbias, timesteps_f32, t_out, ticket, plan, x0,
                                   noise, mask, blend):
    """dpm_step_fused_windowed with the inpainting blend (aldm_dpm_step_fused_windowed_masked); hist long, receives unblended values."""
    assert hist.dtype == torch.float32 and hist.numel() == x.numel()
    _step_fused_windowed("dpm", eps, x, cfg, guidance, coef, step_idx, x_in, (hist,), table, rowbias, timesteps_f32, t_out, ticket, plan,
                         (x0, noise, mask, blend))


def unipc_step_fused_windowed_masked(eps, x, cfg, guidance, coef, step_idx, x_in, state, table, rowbias, timesteps_f32, t_out, ticket, plan, x0,
                                     noise, mask, blend):
    """unipc_step_fused_windowed with the inpainting blend (aldm_unipc_step_fused_windowed_masked); state long, receives unblended values."""
    _check_unipc_state(state, x)
    _step_fused_windowed("unipc", eps, x, cfg, guidance, coef, step_idx, x_in, (state,), table, rowbias, timesteps_f32, t_out, ticket, plan,
                         (x0, noise, mask, blend))


def euler_a_step_fused_windowed_masked(eps, x, cfg, guidance, coef, step_idx, x_in, rng_state, table, rowbias, timesteps_f32, t_out, ticket, plan,
                                       x0, noise, mask, blend):
    """euler_a_step_fused_windowed with the inpainting blend (aldm_euler_a_step_fused_windowed_masked); blend rows (1, sigma_next)."""
    _check_state(rng_state)
    _step_fused_windowed("euler_a", eps, x, cfg, guidance, coef, step_idx, x_in, (rng_state,), table, rowbias, timesteps_f32, t_out, ticket, plan,
                         (x0, noise, mask, blend))


def repaint_step_fused_windowed_masked(eps, x, cfg, guidance, coef, step_idx, x_in, rng_state, table, rowbias, timesteps_f32, t_out, ticket, plan,
                                       x0, noise, mask, blend):
    """repaint_step_fused_masked on a long latent (aldm_repaint_step_fused_windowed_masked): element i of the LONG latent is element i
    of both draws; `noise` may be None."""
    _check_state(rng_state)
    _step_fused_windowed("repaint", eps, x, cfg, guidance, coef, step_idx, x_in, (rng_state,), table, rowbias, timesteps_f32, t_out, ticket, plan,
                         (x0, noise, mask, blend))


def add_noise(x, noise, coef):
    _require_gpu(x)
    B = x.shape[0]
    xf, nf = x.float().contiguous(), noise.float().contiguous()
    out = torch.empty_like(xf)
    check(_lib.load().aldm_add_noise(_p(xf), _p(nf), _p(coef), B, xf.numel() // B, _p(out), _stream()), "aldm_add_noise")
    return out.to(x.dtype)


def add_noise_t(x, noise, alphas_cumprod, timesteps):
    """DDIMScheduler.add_noise with device-side coefficients: x, noise fp32 [B, ...], alphas_cumprod fp32 [T], timesteps int64 [B]."""
    _require_gpu(x)
    B = x.shape[0]
    xf, nf = x.float().contiguous(), noise.float().contiguous()
    assert alphas_cumprod.dtype == torch.float32 and timesteps.dtype == torch.int64 and timesteps.numel() == B
    out = torch.empty_like(xf)
    check(_lib.load().aldm_add_noise_t(_p(xf), _p(nf), _p(alphas_cumprod), _p(timesteps.contiguous()), alphas_cumprod.numel(), B,
                                       xf.numel() // B, _p(out), _stream()), "aldm_add_noise_t")
    return out.to(x.dtype)


def gaussian_sample(params_nchw, noise):
    """mean + exp(0.5 clamp(logvar)) * noise for params [B, 2C, H, W] fp32 (mean | logvar), noise [B, C, H, W] fp32."""
    _require_gpu(params_nchw)
    B, C2 = params_nchw.shape[:2]
    pf, nf = params_nchw.float().contiguous(), noise.float().contiguous()
    out = torch.empty_like(nf)
    check(_lib.load().aldm_gaussian_sample(_p(pf), _p(nf), B, nf.numel() // B, _p(out), _stream()), "aldm_gaussian_sample")
    return out


def resample_poly(x, up, down, lens=None, table=None):
    """scipy.signal.resample_poly(x, up, down) on the device (aldm_resample_poly; resample.py has the definition): x fp32 [B, T] whose
    row b holds lens[b] samples (all T when None) -> (y fp32 [B, ceil(T up / down)], out_lens int32 [B] on the host); y is 0 from
    out_lens[b] = ceil(lens[b] up / down) on.  table: resample.phase_table(up, down) on x's device (looked up when None)."""
    from . import resample as R
    up, down = R.check_ratio(up, down)
    _require_gpu(x)
    if x.dim() != 2 or x.numel() == 0:
        raise ValueError(f"resample_poly: x must be a non-empty [B, T], got {tuple(x.shape)}")
    x = x.to(torch.float32).contiguous()
    B, T = x.shape
    lens = torch.full((B,), T, dtype=torch.int32) if lens is None else torch.as_tensor(lens).to("cpu", torch.int32).reshape(-1)
    if lens.numel() != B or int(lens.min()) < 0 or int(lens.max()) > T:
        raise ValueError(f"resample_poly: lens must hold {B} lengths in [0, {T}], got {lens.tolist()}")
    if table is None:
        table = R.device_table(up, down, x.device)
    half = 10 * max(up, down)
    K = -(-(2 * half + 1) // up)
    if tuple(table.shape) != (up, K) or table.dtype != torch.float32 or table.device != x.device or not table.is_contiguous():
        raise ValueError(f"resample_poly: table must be contiguous fp32 [{up}, {K}] on {x.device}")
    y = _resample_poly_rows(x, up, down, _h2d(lens, x.device), table)
    return y, ((lens.to(torch.int64) * up + down - 1) // down).to(torch.int32)


def _resample_poly_rows(x, up, down, dev_lens, table):
    """resample_poly's launch with the lengths already on the device (int32 [B]; the kernel cuts them to [0, T]): nothing is copied
    from the host, so a captured graph can hold it.  x contiguous fp32 [B, T], table the checked phase table."""
    from . import resample as R
    B, T = x.shape
    half = 10 * max(up, down)
    K = -(-(2 * half + 1) // up)
    T_out = R.output_length(T, up, down)
    y = torch.empty(B, T_out, dtype=torch.float32, device=x.device)
    check(_lib.load().aldm_resample_poly(_p(x), _p(dev_lens), B, T, _p(table), up, down, K, half, _p(y), T_out, _stream()),
          "aldm_resample_poly")
    return y


def _h2d(t, device):
    """A small host tensor -> `device` from pinned memory, without blocking the host: a pageable `.to(device)` on the current stream
    waits for everything queued there (the previous training step's graph), a pinned non-blocking copy is only enqueued.  torch's
    pinned-memory cache keeps the staging block alive until the copy has run."""
    return t.pin_memory().to(device, non_blocking=True)


def clip_segment(pool, offsets, lens, ordinals, S, state, max_len, advance=True):
    """A random, non-silent window of S samples per recording (aldm_clip_segment; the rule is in include/aldm_hip.h, the stream
    contract in csrc/philox.h).  pool: fp32 1-D on the device; row b is the lens[b] samples from pool[offsets[b]] on.  offsets int64
    [B], lens int32 [B], ordinals int32 [B]: device tensors (a captured graph reads them), or anything torch.as_tensor takes, which
    is then checked against the pool on the host and copied over.  max_len: a host-side upper bound of lens.  advance: leave the
    draw ordinal one further (False for every call but the last of a batch that is split by sampling rate).
    Returns (seg fp32 [B, S], start int32 [B] on the device)."""
    _check_state(state)
    _require_gpu(pool)
    if pool.dtype != torch.float32 or pool.dim() != 1 or pool.numel() == 0 or not pool.is_contiguous():
        raise ValueError("clip_segment: the pool must be a non-empty contiguous fp32 1-D tensor")
    S, max_len = int(S), int(max_len)
    if S <= 0 or max_len <= 0:
        raise ValueError(f"clip_segment: S and max_len must be positive (got {S}, {max_len})")
    on_dev = [torch.is_tensor(t) and t.is_cuda for t in (offsets, lens, ordinals)]
    if not all(on_dev):
        if any(on_dev):
            raise ValueError("clip_segment: offsets, lens and ordinals must all be on the device or all on the host")
        offsets = torch.as_tensor(offsets, dtype=torch.int64).reshape(-1)
        lens = torch.as_tensor(lens, dtype=torch.int32).reshape(-1)
        ordinals = torch.as_tensor(ordinals, dtype=torch.int32).reshape(-1)
        if not (offsets.numel() == lens.numel() == ordinals.numel() > 0):
            raise ValueError("clip_segment: offsets, lens and ordinals must hold one entry per row")
        if int(lens.min()) < 0 or int(lens.max()) > max_len or int(offsets.min()) < 0 or int((offsets + lens).max()) > pool.numel():
            raise ValueError("clip_segment: a row leaves the pool or is longer than max_len")
        if int(ordinals.min()) < 0:
            raise ValueError("clip_segment: ordinals must not be negative")
        offsets, lens, ordinals = _h2d(offsets, pool.device), _h2d(lens, pool.device), _h2d(ordinals, pool.device)
    B = lens.numel()
    for t, dt in ((offsets, torch.int64), (lens, torch.int32), (ordinals, torch.int32)):
        assert t.dtype == dt and t.numel() == B and t.is_contiguous() and t.device == pool.device, "clip_segment: int64 / int32 / int32 [B]"
    lib = _lib.load()
    ws = torch.empty(max(1, lib.aldm_clip_segment_workspace_floats(B, max_len)), dtype=torch.float32, device=pool.device)
    seg = torch.empty(B, S, dtype=torch.float32, device=pool.device)
    start = torch.empty(B, dtype=torch.int32, device=pool.device)
    check(lib.aldm_clip_segment(_p(pool), pool.numel(), _p(offsets), _p(lens), _p(ordinals), B, S, max_len, _p(state), int(bool(advance)),
                                _p(ws), _p(seg), _p(start), _stream()), "aldm_clip_segment")
    return seg, start


def clip_normalize(y, n, target):
    """Mean removal, peak normalisation to 0.5 and zero padding / cropping to `target` samples (aldm_clip_normalize): y fp32 [B, T]
    whose row b holds n[b] samples (int32 [B]; a host tensor or list is copied over) -> fp32 [B, target]."""
    _require_gpu(y)
    if y.dtype != torch.float32 or y.dim() != 2 or y.numel() == 0 or not y.is_contiguous():
        raise ValueError("clip_normalize: y must be a non-empty contiguous fp32 [B, T]")
    B, T = y.shape
    target = int(target)
    if target <= 0:
        raise ValueError(f"clip_normalize: target must be positive (got {target})")
    if not (torch.is_tensor(n) and n.is_cuda):
        n = _h2d(torch.as_tensor(n, dtype=torch.int32).reshape(-1), y.device)
    assert n.dtype == torch.int32 and n.numel() == B and n.is_contiguous() and n.device == y.device, "clip_normalize: n int32 [B]"
    lib = _lib.load()
    ws = torch.empty(3 * B * lib.aldm_clip_normalize_parts(T, target), dtype=torch.float64, device=y.device)
    out = torch.empty(B, target, dtype=torch.float32, device=y.device)
    check(lib.aldm_clip_normalize(_p(y), _p(n), B, T, target, _p(ws), _p(out), _stream()), "aldm_clip_normalize")
    return out


def _wave_rows(x, lens, what, longest=None):
    """(B, T) of a contiguous fp32 [B, T] device tensor x, and lens as int32 [B] on x's device (checked against `longest`, default T,
    and copied over when it is not there; the kernels cut device lengths to the row themselves)"""
    _require_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.numel() == 0 or not x.is_contiguous():
        raise ValueError(f"{what}: x must be a non-empty contiguous fp32 [B, T]")
    B, T = x.shape
    if not (torch.is_tensor(lens) and lens.is_cuda):
        lens = torch.as_tensor(lens).to("cpu", torch.int32).reshape(-1)
        if lens.numel() != B or int(lens.min()) < 0 or int(lens.max()) > (T if longest is None else longest):
            raise ValueError(f"{what}: lens must hold {B} lengths in [0, {T}], got {lens.tolist()}")
        lens = _h2d(lens, x.device)
    assert lens.dtype == torch.int32 and lens.numel() == B and lens.is_contiguous() and lens.device == x.device, f"{what}: lens int32 [B]"
    return B, T, lens


def _f64_table(t, n, device, what):
    if not (torch.is_tensor(t) and t.dtype == torch.float64 and t.numel() == n and t.is_contiguous() and t.device == device):
        raise ValueError(f"{what} must be a contiguous float64 tensor of {n} elements on {device}")


def kweight_energy(x, lens, hop, coef, mpow, chunk):
    """K-weighted energy per hop of `hop` samples (aldm_kweight_energy; loudness.py has the definition): x fp32 [B, T] whose row b holds
    lens[b] samples -> float64 [B, T // hop], zero behind a row's complete hops.  coef float64 [10], mpow float64 [6, 2, 4, 4] on the device:
    the two biquads and the chunk's state-transition powers (loudness.LoudnessMeter builds both)."""
    B, T, lens = _wave_rows(x, lens, "kweight_energy")
    hop, chunk = int(hop), int(chunk)
    _f64_table(coef, 10, x.device, "kweight_energy: coef")
    _f64_table(mpow, 192, x.device, "kweight_energy: mpow")
    lib = _lib.load()
    e = torch.empty(B, T // hop if hop > 0 else 0, dtype=torch.float64, device=x.device)
    ws = torch.empty(max(1, lib.aldm_kweight_energy_workspace_doubles(B, T)), dtype=torch.float64, device=x.device)
    n = float(B) * T
    # two passes over the samples, 10 fused multiply-adds a sample each, and the squares; every sample is read twice
    check(_launch(f"kweight_energy|B{B} T{T} H{hop}", 2.0 * (2 * 10 + 4) * n, 2 * 4.0 * n + 8.0 * e.numel() + 8.0 * ws.numel(),
                  lambda: lib.aldm_kweight_energy(_p(x), _p(lens), B, T, hop, _p(coef), _p(mpow), chunk, _p(ws), _p(e), _stream())),
          "aldm_kweight_energy")
    return e


def loudness_gate(energy, lens, T, hop):
    """Gated BS.1770 loudness from hop energies (aldm_loudness_gate): energy float64 [B, T // hop], lens int32 [B] -> float64 [B] in
    LUFS, -inf for a clip without a 400 ms block above -70."""
    _require_gpu(energy)
    T, hop = int(T), int(hop)
    if energy.dtype != torch.float64 or energy.dim() != 2 or not energy.is_contiguous() or hop <= 0 or energy.shape[1] != T // hop:
        raise ValueError(f"loudness_gate: energy must be a contiguous float64 [B, {T} // {hop}]")
    B = energy.shape[0]
    if not (torch.is_tensor(lens) and lens.is_cuda):
        lens = _h2d(torch.as_tensor(lens).to("cpu", torch.int32).reshape(-1), energy.device)
    assert lens.dtype == torch.int32 and lens.numel() == B and lens.is_contiguous() and lens.device == energy.device, "loudness_gate: lens int32 [B]"
    out = torch.empty(B, dtype=torch.float64, device=energy.device)
    n = float(energy.numel())
    check(_launch(f"loudness_gate|B{B} hops{energy.shape[1]}", 2.0 * 8 * n, 2 * 4 * 8.0 * n + 8.0 * B,
                  lambda: _lib.load().aldm_loudness_gate(_p(energy), _p(lens), B, T, hop, _p(out), _stream())), "aldm_loudness_gate")
    return out


def peak_abs(x, lens, lens_ratio=(1, 1)):
    """max |x| over the first lens[b] samples of every row (aldm_peak_abs): x fp32 [B, T] -> fp32 [B].  lens_ratio = (up, down): lens
    are those of the rows x was resampled FROM, and row b holds ceil(lens[b] up / down) samples (resample_poly's out_lens, worked out
    on the device)."""
    up, down = int(lens_ratio[0]), int(lens_ratio[1])
    if up < 1 or down < 1:
        raise ValueError(f"peak_abs: lens_ratio must be two positive integers, got {lens_ratio!r}")
    B, T, lens = _wave_rows(x, lens, "peak_abs", longest=x.shape[-1] * down // up)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    check(_launch(f"peak_abs|B{B} T{T}", 1.0 * B * T, 4.0 * B * T + 4.0 * B,
                  lambda: _lib.load().aldm_peak_abs(_p(x), _p(lens), B, T, up, down, _p(out), _stream())), "aldm_peak_abs")
    return out


def loudness_gain(x, lens, lufs, peak, target_lufs, ceiling_dbfs=None):
    """The gain that brings rows of loudness `lufs` (float64 [B]) to target_lufs, capped so that gain * peak (fp32 [B]) stays at or
    under ceiling_dbfs (None: no cap), applied out of place (aldm_loudness_gain) -> (y fp32 [B, T], gain fp32 [B], gain_db float64 [B]).
    A row whose loudness is -inf keeps gain 1; y is 0 from lens[b] on."""
    B, T, lens = _wave_rows(x, lens, "loudness_gain")
    _f64_table(lufs, B, x.device, "loudness_gain: lufs")
    cap = ceiling_dbfs is not None
    if cap and not (torch.is_tensor(peak) and peak.dtype == torch.float32 and peak.numel() == B and peak.is_contiguous()
                    and peak.device == x.device):
        raise ValueError(f"loudness_gain: peak must be a contiguous fp32 [{B}] on {x.device}")
    y = torch.empty_like(x)
    gain = torch.empty(B, dtype=torch.float32, device=x.device)
    gain_db = torch.empty(B, dtype=torch.float64, device=x.device)
    check(_launch(f"loudness_gain|B{B} T{T}", 1.0 * B * T, 8.0 * B * T + 24.0 * B,
                  lambda: _lib.load().aldm_loudness_gain(_p(x), _p(lens), B, T, _p(lufs), _p(peak) if cap else None, float(target_lufs),
                                                         float(ceiling_dbfs) if cap else 0.0, int(cap), _p(gain), _p(gain_db), _p(y),
                                                         _stream())), "aldm_loudness_gain")
    return y, gain, gain_db


def train_noise_fused(state, alphas_cumprod, moments=None, latents=None, scaling_factor=1.0, noise_offset=0.0, ticket=None,
                      timesteps_out=None):
    """The training step's batch noising with on-device randomness as one launch (aldm_train_noise_fused; stream contract in
    csrc/philox.h): timesteps, the posterior noise, the diffusion noise and the noise offset's normals are draws d .. d + 3 of `state`.
    Exactly one source: moments fp32 channels-last [B, H, W, 2C] (mean | logvar, what vae.encode_nhwc returns; the sample is scaled by
    scaling_factor) or latents fp32 NCHW [B, C, H, W].  alphas_cumprod fp32 [T].  ticket: int32 [1], zero (the kernel leaves it zero) --
    the ordinal then moves by 4 on the device; None leaves the state alone.  timesteps_out: int64 [B] to write the timesteps into.
    Returns (x_in bf16 [B, H, W, C], target fp32 [B, H, W, C], timesteps int64 [B], t_f32 fp32 [B])."""
    _check_state(state)
    if (moments is None) == (latents is None):
        raise _lib.AldmError("train_noise_fused: give either moments= or latents=")
    src = moments if moments is not None else latents
    _require_gpu(src)
    _require_gpu(alphas_cumprod)
    assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 4, "train_noise_fused: fp32 contiguous 4-d source"
    assert alphas_cumprod.dtype == torch.float32 and alphas_cumprod.is_contiguous()
    if moments is not None:
        B, H, W, C2 = moments.shape
        assert C2 % 2 == 0, "moments: channels-last mean | logvar"
        Cc = C2 // 2
    else:
        B, Cc, H, W = latents.shape
    assert ticket is None or (ticket.dtype == torch.int32 and ticket.numel() == 1 and ticket.is_cuda)
    dev = src.device
    x_in = torch.empty(B, H, W, Cc, dtype=torch.bfloat16, device=dev)
    target = torch.empty(B, H, W, Cc, dtype=torch.float32, device=dev)
    if timesteps_out is None:
        timesteps_out = torch.empty(B, dtype=torch.int64, device=dev)
    assert timesteps_out.dtype == torch.int64 and timesteps_out.numel() == B and timesteps_out.is_contiguous() and timesteps_out.is_cuda
    t_f32 = torch.empty(B, dtype=torch.float32, device=dev)
    n = x_in.numel()
    # flops: ~100 per normal (ten Philox rounds + Box-Muller), two normals per element; bytes: the source, bf16 + fp32 out
    check(_launch("train_noise_fused", 220.0 * n, ((8.0 if moments is not None else 4.0) + 6.0) * n,
                  lambda: _lib.load().aldm_train_noise_fused(_p(state), _p(alphas_cumprod), alphas_cumprod.numel(), _p(moments), _p(latents),
                                                             float(scaling_factor), float(noise_offset), B, Cc, H, W, _p(x_in), _p(target),
                                                             _p(timesteps_out), _p(t_f32), _p(ticket), _stream())),
          "aldm_train_noise_fused")
    return x_in, target, timesteps_out, t_f32


def sleep_us(us):
    check(_lib.load().aldm_sleep_us(int(us), _stream()), "aldm_sleep_us")


def gather_row(table, idx, out):
    """out[...] = table[idx[0]] (device-side index); table [n, ...] fp32 contiguous, out one row."""
    row = table[0].numel()
    assert table.dtype == torch.float32 and out.dtype == torch.float32 and out.numel() == row and idx.dtype == torch.int32
    check(_launch("gather_row", 0.0, 8.0 * row, lambda: _lib.load().aldm_gather_row(_p(table), _p(idx), row, _p(out), _stream())),
          "aldm_gather_row")


def advance_step(step_idx, timesteps_f32, t_out):
    check(_launch("advance_step", 0.0, 16.0, lambda: _lib.load().aldm_advance_step(_p(step_idx), _p(timesteps_f32), timesteps_f32.numel(),
                                                                                    _p(t_out), _stream())), "aldm_advance_step")


def adamw_flat(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    check(_lib.load().aldm_adamw_flat(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, wd, step,
                                      grad_scale, _stream()), "aldm_adamw_flat")


SUMSQ_PARTS = 256          # workgroups (= partial sums) of sumsq_flat: plenty for the <= 1.8 M floats of a LoRA gradient buffer


def _flat_f32(*ts):
    for t in ts:
        _require_gpu(t)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.AldmError("flat-buffer kernels take contiguous fp32 tensors")


def sumsq_flat(g, partials=None):
    """partials [SUMSQ_PARTS] fp32: per-workgroup sums of squares of g (no float atomics: bitwise reproducible).  The consumers
    (adamw_flat_clip, clip_flat) add them in index order."""
    if partials is None:
        partials = torch.empty(SUMSQ_PARTS, dtype=torch.float32, device=g.device)
    _flat_f32(g, partials)
    check(_lib.load().aldm_sumsq_flat(_p(g), g.numel(), _p(partials), partials.numel(), _stream()), "aldm_sumsq_flat")
    return partials


def adamw_flat_clip(p, g, m, v, lr, beta1, beta2, eps, wd, step, partials, max_norm, norm_out, grad_scale=1.0):
    """adamw_flat on g * grad_scale * min(1, max_norm / (total + 1e-6)), total = sqrt(sum(partials)) * grad_scale -> norm_out[0]."""
    _flat_f32(p, g, m, v, partials, norm_out)
    n = p.numel()
    assert g.numel() == n and m.numel() == n and v.numel() == n and norm_out.numel() >= 1
    check(_lib.load().aldm_adamw_flat_clip(_p(p), _p(g), _p(m), _p(v), n, lr, beta1, beta2, eps, wd, step, grad_scale, _p(partials),
                                           partials.numel(), max_norm, _p(norm_out), _stream()), "aldm_adamw_flat_clip")


def clip_flat(g, partials, max_norm, norm_out, grad_scale=1.0):
    """g *= min(1, max_norm / (total + 1e-6)) in place; norm_out[0] = total (see adamw_flat_clip)."""
    _flat_f32(g, partials, norm_out)
    assert norm_out.numel() >= 1
    check(_lib.load().aldm_clip_flat(_p(g), g.numel(), _p(partials), partials.numel(), max_norm, grad_scale, _p(norm_out), _stream()),
          "aldm_clip_flat")


def accum_flat(acc, g, first):
    """acc = g if first else acc + g."""
    _flat_f32(acc, g)
    assert acc.numel() == g.numel()
    check(_lib.load().aldm_accum_flat(_p(acc), _p(g), g.numel(), int(bool(first)), _stream()), "aldm_accum_flat")


# ---------------------------------------------------------------------------------------------------------
# training-side wrappers (LoRA fine-tune step)
# ---------------------------------------------------------------------------------------------------------
def transpose_tokens(x2d, B, N, Cc, npad=None):
    """rows [B*N, C] -> token-major [B, C, Npad] (zero padded)."""
    _require_gpu(x2d)
    npad = npad or (N + 7) // 8 * 8
    out = torch.empty(B, Cc, npad, dtype=torch.bfloat16, device=x2d.device)
    check(_lib.load().aldm_transpose_tokens(_p(x2d), x2d.stride(0), B, N, Cc, npad, _p(out), _stream()), "aldm_transpose_tokens")
    return out


def attention_train(qkv, qkvT, B, N, H, d):
    """qkv [B*N, 3C] row-major, qkvT [B, 3C, Npad] token-major -> (out [B*N, C], lse [B, H, N] fp32)."""
    Cc = H * d
    out = torch.empty(B * N, Cc, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    base, tb = qkv.data_ptr(), qkvT.data_ptr()
    npad = qkvT.shape[2]
    check(_lib.load().aldm_attention_lse(C.c_void_p(base), 3 * Cc, C.c_void_p(base + 2 * Cc), 3 * Cc,
                                         C.c_void_p(tb + 2 * (2 * Cc) * npad), npad, 3 * Cc * npad, B, N, H, d,
                                         1.0 / math.sqrt(d), _p(out), Cc, _p(lse), _stream()), "aldm_attention_lse")
    return out, lse


def attention_bwd(qkv, qkvT, dO, O, lse, B, N, H, d, dOT=None):
    """-> dqkv [B*N, 3C] (dQ | dK | dV).  dOT: dO token-major [B, C, Npad] when its producer already stored it that way."""
    Cc = H * d
    npad = qkvT.shape[2]
    if dOT is None:
        dOT = transpose_tokens(dO, B, N, Cc, npad)
    assert tuple(dOT.shape) == (B, Cc, npad)
    dqkv = torch.empty(B * N, 3 * Cc, dtype=torch.bfloat16, device=qkv.device)
    delta = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    base, tb, gb = qkv.data_ptr(), qkvT.data_ptr(), dqkv.data_ptr()
    check(_lib.load().aldm_attention_bwd(
        C.c_void_p(base), C.c_void_p(base + 2 * Cc), C.c_void_p(base + 4 * Cc), 3 * Cc,
        C.c_void_p(tb), C.c_void_p(tb + 2 * Cc * npad), _p(dOT), npad, 3 * Cc * npad, 3 * Cc * npad, Cc * npad,
        _p(dO), _p(O), Cc, _p(lse), _p(delta), B, N, H, d, 1.0 / math.sqrt(d),
        C.c_void_p(gb), C.c_void_p(gb + 2 * Cc), C.c_void_p(gb + 4 * Cc), 3 * Cc, _stream()), "aldm_attention_bwd")
    return dqkv


def _like(buf, like):
    assert buf.is_contiguous() and buf.numel() == like.numel() and buf.dtype == like.dtype
    return buf


def groupnorm_bwd(x, dy, gamma, beta, groups, eps, act, x2=None, need_dx2=True, dx_add=None, dx2_add=None):
    """dx (dx2) of act(group_norm(cat[x, x2])).  dx_add / dx2_add: gradients x / x2 already hold from their other consumers;
    they are added inside the kernel (fresh output tensors, the inputs are not modified)."""
    B, H, W, C1 = x.shape
    C2 = x2.shape[3] if x2 is not None else 0
    dx = torch.empty_like(x)
    dx2 = torch.empty_like(x2) if (x2 is not None and need_dx2) else None
    a1 = _like(dx_add, x) if dx_add is not None else None
    a2 = _like(dx2_add, x2) if (dx2 is not None and dx2_add is not None) else None
    if isinstance(dy, Deferred):                           # dY = partial tiles of the dX convolution launched just before
        if dy is not _pending_get(dy.out) or dy.bias is not None or dy.rowbias is not None or dy.res is not None:
            raise _lib.AldmError("groupnorm_bwd: deferred dY must be the pending split-K launch, without bias / residual")
        if dy.layout != _lib.SLAB_ROWMAJOR:
            raise _lib.AldmError("groupnorm_bwd: deferred dY must be left in row-major slabs (conv(..., slab_layout=_lib.SLAB_ROWMAJOR))")
        assert tuple(dy.out.shape) == (B, H, W, C1 + C2)
        check(_lib.load().aldm_groupnorm_bwd_partials(_p(x), _p(x2), dy.ws, dy.eff, B, H * W, C1, C2, groups, eps, _p(gamma), _p(beta),
                                                      act, _p(dx), _p(dx2), _p(a1), _p(a2), _stream()), "aldm_groupnorm_bwd_partials")
        _pending_set(dy.out, None)
        return dx, dx2
    check(_lib.load().aldm_groupnorm_bwd(_p(x), _p(x2), _p(dy), B, H * W, C1, C2, groups, eps, _p(gamma), _p(beta), act,
                                         _p(dx), _p(dx2), _p(a1), _p(a2), _stream()), "aldm_groupnorm_bwd")
    return dx, dx2


def layernorm_bwd(x2d, dy, gamma, eps=1e-5, dx_add=None):
    M, Cc = x2d.shape
    dx = torch.empty_like(x2d)
    a = _like(dx_add, x2d) if dx_add is not None else None
    check(_lib.load().aldm_layernorm_bwd(_p(x2d), _p(dy), M, Cc, _p(gamma), eps, _p(dx), _p(a), _stream()), "aldm_layernorm_bwd")
    return dx


def geglu_fwd(h):
    M, two_i = h.shape
    out = torch.empty(M, two_i // 2, dtype=torch.bfloat16, device=h.device)
    check(_lib.load().aldm_geglu_fwd(_p(h), M, two_i // 2, _p(out), _stream()), "aldm_geglu_fwd")
    return out


def geglu_bwd(h, dout):
    dh = torch.empty_like(h)
    check(_lib.load().aldm_geglu_bwd(_p(h), _p(dout), h.shape[0], h.shape[1] // 2, _p(dh), _stream()), "aldm_geglu_bwd")
    return dh


def add_bf16(a, b):
    c = torch.empty_like(a)
    check(_lib.load().aldm_add_bf16(_p(a), _p(b), a.numel(), _p(c), _stream()), "aldm_add_bf16")
    return c


def upsample_nearest_bwd(dy, ih, iw):
    B, OH, OW, Cc = dy.shape
    dx = torch.empty(B, ih, iw, Cc, dtype=torch.bfloat16, device=dy.device)
    check(_lib.load().aldm_upsample_nearest_bwd(_p(dy), B, ih, iw, OH, OW, Cc, _p(dx), _stream()), "aldm_upsample_nearest_bwd")
    return dx


def tn_small(P, Q, rows_dev, Qc=None):
    """flat_grad rows += P^T Q  through the device row table (see aldm_tn_small)."""
    M, Rp = P.shape
    check(_lib.load().aldm_tn_small(_p(P), Rp, _p(Q), Q.stride(0), Qc or Q.shape[1], M, _p(rows_dev), _stream()), "aldm_tn_small")



class TnBatch:
    """Deferred LoRA-gradient products: collects (P, Q, rows) jobs during the backward pass and runs them in ONE
    aldm_tn_batched launch per rank padding (Rp = 32 / 64).  The device job tables are allocated once (stable pointers for
    hipGraph capture); under capture the launch is recorded first and `upload()` fills the tables after the capture ends."""
    REC = 48                         # sizeof(TnJob): 3 pointers + 6 ints

    def __init__(self, capacity, device):
        self.capacity = capacity
        self.tab = {rp: torch.zeros(capacity * self.REC, dtype=torch.uint8, device=device) for rp in (32, 64)}
        self.jobs = {32: [], 64: []}
        self.keep = []               # operand tensors stay referenced until the launch is recorded
        self._packed = {}
        self.owner = None            # the snapshot whose records the device tables currently hold (None: an eager launch's)

    def add(self, P, Q, rows_dev, Qc):
        M, Rp = P.shape
        ldq = Q.stride(0)
        if ldq % 8 or Qc % 8 or P.data_ptr() % 16 or Q.data_ptr() % 16 or len(self.jobs[Rp]) >= self.capacity:
            tn_small(P, Q, rows_dev, Qc=Qc)                  # odd shapes: the per-call (scalar) path
            return
        qt = -(-Qc // 128)
        msplit = max(1, 24 // qt)                            # ~24 workgroups per job: the whole batch fills the GPU
        mpb = max(64, -(-(-(-M // msplit)) // 32) * 32)
        self.jobs[Rp].append((P.data_ptr(), Q.data_ptr(), rows_dev.data_ptr(), M, ldq, Qc, qt, mpb, qt * (-(-M // mpb))))
        self.keep += [P, Q, rows_dev]

    def _pack(self):
        import struct
        self._packed = {}
        for rp, jobs in self.jobs.items():
            if not jobs:
                continue
            wg0, recs = 0, []
            for (pp, qq, rr, M, ldq, Qc, qt, mpb, nwg) in jobs:
                recs.append(struct.pack("<qqqiiiiii", pp, qq, rr, M, ldq, Qc, qt, mpb, wg0))
                wg0 += nwg
            self._packed[rp] = (b"".join(recs), len(jobs), wg0)

    def upload(self):
        """Copy the packed tables to the device (outside any capture)."""
        for rp, (blob, n, _) in self._packed.items():
            self.tab[rp][: len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
        self.owner = None

    def snapshot(self):
        """The records of the launch just recorded (call right after a capture ends): a captured graph replays aldm_tn_batched
        against the ONE device table, so it must be able to put ITS records back (restore) after anything else used the table."""
        return {rp: blob for rp, (blob, _, _) in self._packed.items()}

    def restore(self, snap):
        """Make the device tables hold `snap`'s records (no-op when they already do).  Stream-ordered H2D copies on the current
        stream, i.e. in front of the replay that needs them."""
        if snap is None or self.owner is snap:
            return
        for rp, blob in snap.items():
            self.tab[rp][: len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
        self.owner = snap

    def launch(self):
        self._pack()
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.upload()
        for rp, (_, n, total) in self._packed.items():
            check(_lib.load().aldm_tn_batched(_p(self.tab[rp]), n, total, rp, _stream()), "aldm_tn_batched")
        self.jobs = {32: [], 64: []}
        self.keep = []

def lora_pack(jobs_dev, njobs):
    check(_lib.load().aldm_lora_pack(_p(jobs_dev), njobs, _stream()), "aldm_lora_pack")


def mse_grad(pred, target, loss, grad_scale=1.0):
    dp = torch.empty(pred.shape, dtype=torch.bfloat16, device=pred.device)
    check(_lib.load().aldm_mse_grad(_p(pred), _p(target), pred.numel(), grad_scale, _p(dp), _p(loss), _stream()), "aldm_mse_grad")
    return dp


def mse_grad_snr(pred, target, loss, alphas_cumprod, timesteps, snr_gamma, grad_scale=1.0):
    """mse_grad with diffusers' min-SNR-gamma weight per sample (epsilon prediction), looked up on the device: pred / target fp32
    [B, ...], alphas_cumprod fp32 [T], timesteps int64 [B]."""
    _require_gpu(pred)
    B = timesteps.numel()
    assert pred.dtype == torch.float32 and target.dtype == torch.float32 and pred.is_contiguous() and target.is_contiguous()
    assert alphas_cumprod.dtype == torch.float32 and timesteps.dtype == torch.int64 and timesteps.is_contiguous()
    assert pred.shape[0] == B and target.numel() == pred.numel() and pred.numel() % B == 0
    dp = torch.empty(pred.shape, dtype=torch.bfloat16, device=pred.device)
    check(_lib.load().aldm_mse_grad_snr(_p(pred), _p(target), pred.numel(), pred.numel() // B, _p(alphas_cumprod), _p(timesteps),
                                        alphas_cumprod.numel(), snr_gamma, grad_scale, _p(dp), _p(loss), _stream()), "aldm_mse_grad_snr")
    return dp


def pack_conv_bwd(weight, lo=0, hi=None):
    """dX weights of a stride-1 'same' conv: Wt[cin][(kh, kw, cout)] = W[cout][cin][KH-1-kh][KW-1-kw] for cin in [lo, hi)."""
    w = weight.detach()[:, lo:hi]
    return pack_conv(w.flip(2, 3).permute(1, 0, 2, 3).contiguous(), None)


def pack_linear_bwd(weight, lo=0, hi=None):
    return pack_linear(weight.detach().t()[lo:hi].contiguous(), None)
