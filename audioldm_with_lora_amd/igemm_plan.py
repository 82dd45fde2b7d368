"""How a convolution is launched, decided without a GPU: the tile table, the halo rule, the tuning key and plan().

ops.conv() describes its call as a Geom (shapes, what it reads of the weight pack, what the caller asked for -- no tensors), plan()
answers with a LaunchPlan (route, key, tile, ring, splits, the statistics tables to allocate), and conv() fills the argument struct
from the two.  Nothing here touches torch.cuda or the native library, so the whole dispatch can be tested on any machine
(tests/test_igemm_plan_host.py replays every launch recorded in tests/golden/igemm_launch_plans.json.gz).

A new tile is one row of TILES; a new halo eligibility rule is one clause of halo_candidates().  The split count a launch really uses
stays the library's answer (aldm_igemm_effective_splits on the filled struct, in conv())."""
import math
import os
import re
import sys
from dataclasses import dataclass
from typing import Callable, Optional, Tuple, Union

from . import _lib
from ._lib import ACT_NONE, OUT_BF16

BK = 64


# ---- the tile table -----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Tile:
    """One ALDM_TILE_* of include/aldm_hip.h.  kind: "w4" four waves, "w8" eight waves, "ws" compute + loader waves (csrc/igemm_ws.hip),
    "halo" / "halo-ws" the 3x3 tiles that keep the input halo in LDS (csrc/igemm_halo.hip).  halo_rows: LDS halo capacity in rows (128x128:
    three or five DMA passes), halo_rows_fused: the same for the fused-shortcut form (x3 | x4; 0: the tile has no such form).  rings: the
    LDS-DMA ring depths the tile runs with; fixed_ring: the one depth pick_ring() gives it (0: pick_ring's residency rule decides)."""
    id: int
    c_name: str
    name: str
    bm: int
    bn: int
    kind: str
    halo_rows: int = 0
    halo_rows_fused: int = 0
    rings: Tuple[int, ...] = (2, 3, 4)
    fixed_ring: int = 0

    @property
    def halo(self):
        return self.kind in ("halo", "halo-ws")


TILES = {t.id: t for t in (
    Tile(_lib.TILE_128x128, "ALDM_TILE_128x128", "128x128", 128, 128, "w4"),
    Tile(_lib.TILE_64x64, "ALDM_TILE_64x64", "64x64", 64, 64, "w4"),
    Tile(_lib.TILE_128x64, "ALDM_TILE_128x64", "128x64", 128, 64, "w4"),
    Tile(_lib.TILE_64x128, "ALDM_TILE_64x128", "64x128", 64, 128, "w4"),
    Tile(_lib.TILE_128x128_W8, "ALDM_TILE_128x128_W8", "128x128w8", 128, 128, "w8", rings=(2, 3), fixed_ring=2),
    Tile(_lib.TILE_HALO_128x128, "ALDM_TILE_HALO_128x128", "halo128x128", 128, 128, "halo", halo_rows=320),
    Tile(_lib.TILE_HALO_64x128, "ALDM_TILE_HALO_64x128", "halo64x128", 64, 128, "halo", halo_rows=128),
    Tile(_lib.TILE_256x128_W8, "ALDM_TILE_256x128_W8", "256x128w8", 256, 128, "w8", rings=(2, 3), fixed_ring=2),
    Tile(_lib.TILE_64x128_W8, "ALDM_TILE_64x128_W8", "64x128w8", 64, 128, "w8"),
    Tile(_lib.TILE_128x64_W8, "ALDM_TILE_128x64_W8", "128x64w8", 128, 64, "w8"),
    Tile(_lib.TILE_256x128_WS, "ALDM_TILE_256x128_WS", "256x128ws", 256, 128, "ws", rings=(3,), fixed_ring=3),
    Tile(_lib.TILE_64x128_WS, "ALDM_TILE_64x128_WS", "64x128ws", 64, 128, "ws", rings=(3, 4)),
    Tile(_lib.TILE_128x64_WS, "ALDM_TILE_128x64_WS", "128x64ws", 128, 64, "ws", rings=(3, 4)),
    Tile(_lib.TILE_HALO_128x128_WS, "ALDM_TILE_HALO_128x128_WS", "halo128x128ws", 128, 128, "halo-ws", halo_rows=320, halo_rows_fused=192),
    Tile(_lib.TILE_HALO_64x128_WS, "ALDM_TILE_HALO_64x128_WS", "halo64x128ws", 64, 128, "halo-ws", halo_rows=128, halo_rows_fused=128),
)}
HALO_TILES = tuple(t for t in TILES.values() if t.halo)
# views of the table (ops re-exports them; tests and tools read them)
TILE_DIMS = {t.id: (t.bm, t.bn) for t in TILES.values()}
TILE_NAMES = {t.id: t.name for t in TILES.values()}
HALO_ROWS = {t.id: t.halo_rows for t in HALO_TILES}

FUSED_HALO_RING = 3                 # the fused-shortcut form of the halo tiles has one ring depth
GNIN_RING = int(os.environ.get("ALDM_GNIN_RING", "0"))     # LDS-DMA ring depth of the input-norm-folding halo launches (0: pick_ring); tuning aid
# Stand-alone GroupNorms read the statistics their producer handed over where that pays: big images (the strip-per-workgroup kernel
# is L2-request-bound there) -- below this many pixels per image the register-resident kernel is as fast (HW = 1000: 6.7 us against
# 10.0 us for fold + apply) and the producers' epilogues stay free of the statistics code.
QSTATS_MIN_HW = 2048
PGEMM_K = (256, 384, 640)
PGEMM_USE_IGEMM = (0, 0, 0, 0)      # pgemm table entry: this GEMM measured faster on aldm_igemm, keep it there


# ---- what a launch looks like without its tensors -------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Geom:
    """One conv() call: geometry, what planning reads of the weight pack, what the caller asked for.  Tensors appear as "is it there"."""
    B: int
    IH: int
    IW: int
    C1: int
    OH: int
    OW: int
    # the weight pack
    N: int
    Kpad: int
    Cin: int
    KH: int = 1
    KW: int = 1
    Cext: int = 0
    Rp: int = 0
    ranks_used: Optional[int] = None
    geglu: bool = False
    ln: bool = False                 # LayerNorm folded into the pack (pack_linear_ln)
    # further sources and the filter's walk
    C2: int = 0
    C3: int = 0
    C4: int = 0
    x2: bool = False
    x3: bool = False
    stride: Tuple[int, int] = (1, 1)
    pad: Tuple[int, int] = (0, 0)
    dil: Tuple[int, int] = (1, 1)
    up_size: Optional[Tuple[int, int]] = None   # parse_key(): (0, 0) = up-sampled, size not in the key
    in_dilate: int = 0
    in_act: int = ACT_NONE
    fast_path: bool = True           # the LDS-DMA path: every channel count a multiple of 64, no input activation
    # the epilogue asked for
    vt: bool = False
    vt_dual: bool = False
    vt_col0: int = 0
    rowbias: bool = False
    res: bool = False
    res_dense: bool = True           # res is contiguous with exactly the output's element count
    res2: bool = False
    out2: bool = False
    out_act: int = ACT_NONE
    post_act: int = ACT_NONE
    alpha: float = 1.0
    lora_t_out: bool = False
    ln_parts: Optional[int] = None   # partial pairs per row of the LayerNorm hand-over table, None: no table
    rowstats: bool = False
    qstats: bool = False             # statistics asked for AND the image big enough for them to pay (geometry(): QSTATS_MIN_HW)
    gn_groups: Optional[int] = None  # gn=: groups of the GroupNorm this call returns
    defer: Union[bool, Tuple[int, int]] = False
    gn_in: bool = False
    gn_deferred: Optional[bool] = None   # None: gn_defer follows from the fields above; parse_key() sets it from the key's " gn" flag
    # forced launch configuration (0 / None: plan() decides)
    tile: int = 0
    ring: int = 0
    splits: Optional[int] = None
    # the output buffer
    out_f32: bool = False            # the caller's out_f32= flag
    out_dtype: int = OUT_BF16        # dtype of the buffer really written
    out_ld: int = 0
    out_batch_stride: int = 0
    out_pix_stride: int = 1
    out_pix_offset: int = 0

    @property
    def M(self):
        return self.B * self.OH * self.OW

    @property
    def ktiles(self):
        return self.Kpad // BK

    @property
    def can_split(self):
        return not (self.vt or self.N % 4 or self.ln)

    @property
    def conv1d(self):
        """a 1 x KW filter over a 1 x T image (the vocoder)"""
        return self.KH == 1 and self.IH == 1 and self.KW > 1

    @property
    def gn_defer(self):
        """May a split-K launch leave its reduce to the consuming GroupNorm (gn= / defer=)?"""
        if self.gn_deferred is not None:
            return self.gn_deferred
        ok = ((self.gn_groups is not None or bool(self.defer)) and self.can_split and not self.geglu and not self.res2 and not self.out2
              and self.out_act == ACT_NONE and self.post_act == ACT_NONE and self.alpha == 1.0 and self.out_dtype == OUT_BF16
              and self.out_ld == self.N and self.out_pix_stride == 1)
        if not ok:
            return False
        if self.gn_groups is not None:
            ct, ng = self.N, self.gn_groups
            return ct % ng == 0 and (ct // ng) % 4 == 0 and self.OH * self.OW * (ct // ng // 4) <= 4096
        ct, ng = self.defer if isinstance(self.defer, tuple) else (self.N, 32)   # (channels, groups) of the consuming norm (it may append a skip tensor)
        cg = ct // ng
        return ct % ng == 0 and cg % 4 == 0 and self.N % cg == 0 and self.OH * self.OW * (cg // 4) <= 4096


def geometry(xshape, pw, *, C2=0, C3=0, C4=0, x2=None, x3=None, stride=(1, 1), pad=(0, 0), dil=(1, 1), up_size=None, out_hw=None,
             in_act=ACT_NONE, out_ld=None, out_batch_stride=None, vt=False, vt_dual=False, vt_col0=0, qstats=False,
             qstats_min_hw=QSTATS_MIN_HW, out_f32=False, out_dtype=None, res=False, res_numel=None, **request):
    """The Geom of conv(x, pw, ...): pw is anything with the weight pack's N / Kpad / Cin / KH / KW / Cext / Rp / geglu / ln attributes
    (ln: the pack folds a LayerNorm), `request` the remaining Geom fields.  qstats is kept only for images of at least qstats_min_hw pixels;
    out_dtype None: a buffer of out_f32's choosing; res_numel: elements of a contiguous `res` (None: not contiguous)."""
    B, IH, IW, C1 = xshape
    stride, pad, dil = tuple(stride), tuple(pad), tuple(dil)
    up_size = None if up_size is None else tuple(up_size)
    VH, VW = up_size if up_size is not None else (IH, IW)
    if out_hw is None:
        OH = (VH + 2 * pad[0] - dil[0] * (pw.KH - 1) - 1) // stride[0] + 1
        OW = (VW + 2 * pad[1] - dil[1] * (pw.KW - 1) - 1) // stride[1] + 1
    else:
        OH, OW = out_hw
    if out_ld is None:
        out_ld = vt_col0 if (vt and not vt_dual) else (pw.N // 2 if pw.geglu else pw.N)
    if out_batch_stride is None:
        out_batch_stride = OH * OW * out_ld
    x2 = C2 > 0 if x2 is None else x2
    return Geom(B=B, IH=IH, IW=IW, C1=C1, OH=OH, OW=OW, N=pw.N, Kpad=pw.Kpad, Cin=pw.Cin, KH=pw.KH, KW=pw.KW, Cext=pw.Cext, Rp=pw.Rp,
                ranks_used=getattr(pw, "ranks_used", None), geglu=bool(pw.geglu), ln=bool(pw.ln), C2=C2, C3=C3, C4=C4, x2=x2,
                x3=(C3 > 0 if x3 is None else x3), stride=stride, pad=pad, dil=dil, up_size=up_size, in_act=in_act,
                fast_path=not (pw.Cin % 64 or (x2 and C2 % 64) or in_act), vt=vt, vt_dual=vt_dual, vt_col0=vt_col0, out_ld=out_ld,
                out_batch_stride=out_batch_stride, qstats=bool(qstats) and OH * OW >= qstats_min_hw, out_f32=bool(out_f32),
                out_dtype=(_lib.OUT_F32 if out_f32 else OUT_BF16) if out_dtype is None else out_dtype, res=res,
                res_dense=not res or res_numel == B * OH * OW * out_ld, **request)


# ---- THE halo rule ------------------------------------------------------------------------------------------------------------------
def _image_halo(t, OW):
    """halo rows of a 3x3 tile whose BM rows cover BM / OW image rows of width OW"""
    return (t.bm // OW + 2) * (OW + 2)


def halo_candidates(g):
    """The halo tiles (ids) this launch can take, in table order.  All of them: LDS-DMA path, stride 1, no zero-dilated input, no LoRA /
    V^T / GEGLU / folded LayerNorm.  Then one of
      * 3x3 "same" (pad 1, dilation 1) at any nearest up-sampling size: BM a multiple of OW, the halo within the tile's capacity;
          - with the fused 1x1 shortcut segment (x3 | x4): the wave-specialised tiles, no up-sampling, C3 and C4 multiples of 64, the
            halo within the three-pass capacity;
          - with the input's GroupNorm applied in the launch (gn_in): the wave-specialised tiles (their loader waves normalise), no
            up-sampling, no x3, C1 and C2 multiples of 64, at most 512 input channels;
      * conv1d, an odd KW > 1 with "same" padding and a forward dilation (dil >= 1, pad >= 0: a transposed convolution's phase walks
        backwards and is none): the wave-specialised tiles read it as a KW x 1 filter over a T x 1 image, halo = BM + (KW - 1) dil rows."""
    if not (g.fast_path and g.stride == (1, 1) and not g.in_dilate and not g.Rp and not g.vt and not g.geglu and not g.ln):
        return []
    if g.KH == 3 and g.KW == 3 and g.pad == (1, 1) and g.dil == (1, 1):
        tiles = [t for t in HALO_TILES if t.bm % g.OW == 0 and _image_halo(t, g.OW) <= t.halo_rows]
        if g.x3:
            tiles = [t for t in tiles if t.kind == "halo-ws" and g.up_size is None and g.C3 % 64 == 0 and g.C4 % 64 == 0
                     and _image_halo(t, g.OW) <= t.halo_rows_fused]
        if g.gn_in:
            tiles = [t for t in tiles if t.kind == "halo-ws" and g.up_size is None and not g.x3 and g.C1 % 64 == 0 and g.C2 % 64 == 0
                     and g.C1 + g.C2 <= 512 and g.Cin == g.C1 + g.C2]
    elif (g.conv1d and g.KW % 2 == 1 and g.dil[0] == 1 and g.dil[1] >= 1 and g.pad[1] >= 0 and g.pad == (0, (g.KW - 1) * g.dil[1] // 2)
          and g.up_size is None and not g.x3 and not g.gn_in):
        tiles = [t for t in HALO_TILES if t.kind == "halo-ws" and t.bm + (g.KW - 1) * g.dil[1] <= t.halo_rows]
    else:
        tiles = []
    return [t.id for t in tiles]


# ---- the tuning key -------------------------------------------------------------------------------------------------------------------
def tune_key(M, N, c1, c2, kh, kw, stride, up, dilate, rp, vt, geglu, ln, fast, ow=None, pad=None, dil=None):
    """Key of one GEMM in the measured table.  The geometry suffix (output width, padding, filter dilation) is part of the key for
    every filter larger than 1x1: two convolutions with equal M / N / C can differ in OW (UNet level 0 is 16 wide, the VAE
    decoder's last level 64) and then differ in which tiles are even legal (the halo tiles need BM % OW == 0)."""
    key = (f"M{M} N{N} C{c1}+{c2} k{kh}x{kw} s{stride[0]} up{int(up)} d{dilate} r{rp} vt{int(vt)} g{int(bool(geglu))} "
           f"ln{int(ln)} f{int(fast)}")
    if ow is not None and (kh > 1 or kw > 1):
        key += f" ow{ow} p{pad[0]}x{pad[1]} dl{dil[0]}x{dil[1]}"
    return key


def launch_key(g, splits=None, legacy=False, gn_defer=None):
    """The table key of a launch: tune_key() of its geometry plus what was asked of it.  A caller-fixed split count is part of the key.
    legacy: the form tables had before the geometry suffix existed.  gn_defer: g.gn_defer where the caller has it at hand."""
    sfx = (("" if splits is None else f" sp{splits}") + (" gn" if (g.gn_defer if gn_defer is None else gn_defer) else "") + (" rs" if g.rowstats else "")
           + (" lp" if g.ln_parts is not None else "") + (f" e{g.C3}+{g.C4}" if g.x3 else "") + (" vd" if g.vt_dual else "")
           + (" gi" if g.gn_in else ""))
    return tune_key(g.M, g.N, g.C1, g.C2, g.KH, g.KW, g.stride, g.up_size is not None, g.in_dilate, g.Rp, g.vt, g.geglu, g.ln,
                    g.fast_path, *(() if legacy else (g.OW, g.pad, g.dil))) + sfx


_KEY = re.compile(r"M(\d+) N(\d+) C(\d+)\+(\d+) k(\d+)x(\d+) s(\d+) up([01]) d(\d+) r(\d+) vt([01]) g([01]) ln([01]) f([01])"
                  r"(?: ow(\d+) p(-?\d+)x(-?\d+) dl(-?\d+)x(-?\d+))?(?: sp(\d+))?( gn)?( rs)?( lp)?(?: e(\d+)\+(\d+))?( vd)?( gi)?$")


def parse_key(key):
    """(Geom, splits) a table key stands for: launch_key(*parse_key(k)) == k.  The key does not hold everything: the batch is folded into
    the rows (B = 1, or B = M / T for conv1d, which is how a 1 x K filter is read), both strides equal the one in the key, an up-sampled
    launch has up_size (0, 0), a LayerNorm hand-over table 0 pairs.  None for anything that is no igemm key (the "pg:" keys of KEYLOG)."""
    m = _KEY.match(key)
    if m is None:
        return None
    (M, N, c1, c2, kh, kw, s, up, d, rp, vt, gg, ln, f, ow, p0, p1, d0, d1, sp, gn, rs, lp, c3, c4, vd, gi) = m.groups()
    M, N, c1, c2, kh, kw, c3i, c4i = int(M), int(N), int(c1), int(c2), int(kh), int(kw), int(c3 or 0), int(c4 or 0)
    OW = int(ow) if ow is not None else M
    one_d = kh == 1 and kw > 1
    rows = M // OW
    cext = c3i + c4i
    g = Geom(B=rows if one_d else 1, IH=1 if one_d else rows, IW=OW, C1=c1, OH=1 if one_d else rows, OW=OW, N=N,
             Kpad=-(-(kh * kw * (c1 + c2) + cext) // BK) * BK, Cin=c1 + c2, KH=kh, KW=kw, Cext=cext, Rp=int(rp), geglu=gg == "1", ln=ln == "1",
             C2=c2, C3=c3i, C4=c4i, x2=c2 > 0, x3=c3 is not None, stride=(int(s), int(s)), pad=(int(p0 or 0), int(p1 or 0)),
             dil=(int(d0 or 1), int(d1 or 1)), up_size=(0, 0) if up == "1" else None, in_dilate=int(d), fast_path=f == "1", vt=vt == "1",
             vt_dual=vd is not None, rowstats=rs is not None, ln_parts=0 if lp is not None else None, gn_in=gi is not None,
             gn_deferred=gn is not None, out_ld=N, out_batch_stride=rows * OW * N if not one_d else OW * N)
    return g, (None if sp is None else int(sp))


# ---- heuristics -----------------------------------------------------------------------------------------------------------------------
def auto_splits(M, N, ktiles):
    """Split-K heuristic (tools/bench_igemm.py sweep): the low-resolution UNet levels have few 64x64 output
    tiles but deep K; split until ~512 workgroups are in flight, at most 4 ways, >= 8 K-tiles per split."""
    tiles = math.ceil(M / 64) * math.ceil(N / 64)
    if tiles >= 256 or ktiles < 16:
        return 1
    return max(1, min(4, math.ceil(512 / tiles), ktiles // 8))


def pick_tile(M, N):
    """Tile heuristic from tools/bench_igemm.py sweeps on MI355X: the 8-wave 128x128 tile once it still yields ~2
    workgroups per CU (256 CUs), 128x64 down to ~2 per CU, else 64x64 (more, smaller workgroups hide the short K loops
    of the low-resolution levels)."""
    if N >= 256 and N % 128 == 0 and math.ceil(M / 128) * (N // 128) >= 448:
        return _lib.TILE_128x128_W8
    if N > 64 and math.ceil(M / 128) * math.ceil(N / 64) >= 448:
        return _lib.TILE_128x64
    if N <= 64 and M >= 4096:
        return _lib.TILE_128x64
    return _lib.TILE_64x64


def pick_ring(tile, bm, bn, rp, nwg, ktiles):
    """LDS-DMA ring depth (2..4 K-tiles in flight).  Rule from tools/bench_igemm.py --ring sweeps on MI355X:
    residency first -- the ring must leave room for ceil(nwg / 256 CUs) workgroups per CU inside the 160 KiB of LDS,
    otherwise the grid runs in two rounds (128x64 tile, 500 workgroups: ring 4 = 98 KiB/WG -> 38.9 us, ring 3 -> 23.9 us);
    then depth -- few workgroups (low-resolution levels) have nothing else to hide the weight stream's latency behind, so
    they take the deepest ring that fits; big grids gain nothing past 2-3.  Tiles with one depth of their own (Tile.fixed_ring) keep it."""
    if TILES[tile].fixed_ring:
        return TILES[tile].fixed_ring
    stage = (bm + bn + rp) * 128
    extra = (bn * 128 if rp else 0) + 2 * bm * 4
    per_cu = min(8, max(1, math.ceil(nwg / 256)))
    fit = ((160 * 1024) // per_cu - extra) // stage
    want = 4 if nwg <= 512 else (2 if ktiles <= 24 else 3)
    return max(2, min(want, fit))


def _ring_for(tile, g, splits):
    t = TILES[tile]
    return pick_ring(tile, t.bm, t.bn, g.Rp, math.ceil(g.M / t.bm) * math.ceil(g.N / t.bn) * max(1, splits), g.ktiles)


def heuristic_cfg(M, pw, ktiles, can_split, fast_path, has_vt, splits=None):
    """(tile, ring, splits) without the table; pw: anything with N and Rp (a weight pack, a Geom)"""
    if splits is None:
        splits = auto_splits(M, pw.N, ktiles) if can_split else 1
    tile = _lib.TILE_64x64 if pw.Rp else pick_tile(M, pw.N)      # LoRA GEMMs are short-K: favour many workgroups
    if tile == _lib.TILE_128x128_W8 and (not fast_path or has_vt or ktiles < 16):
        tile = _lib.TILE_128x64           # the 8-wave tile only exists on the LDS-DMA path and only pays on deep K loops
    bm, bn = TILE_DIMS[tile]
    nwg = math.ceil(M / bm) * math.ceil(pw.N / bn) * max(1, splits)
    return tile, pick_ring(tile, bm, bn, pw.Rp, nwg, ktiles), splits


def generic_candidates(g):
    """The non-halo tiles (ids) a tuner may try on this launch, in the order it tries them"""
    lds = g.fast_path and not g.vt and g.ktiles >= 8
    plain = lds and not g.Rp
    return ([_lib.TILE_64x64, _lib.TILE_128x64, _lib.TILE_128x128, _lib.TILE_64x128] + ([_lib.TILE_128x128_W8] if lds else [])
            + ([_lib.TILE_256x128_W8, _lib.TILE_256x128_WS] if (plain and g.M >= 32768 and g.N % 128 == 0 and not g.ln and not g.geglu
                                                                and not g.Cext) else [])
            + ([_lib.TILE_64x128_W8, _lib.TILE_128x64_W8] if (plain and g.M <= 8192) else [])
            + ([_lib.TILE_64x128_WS, _lib.TILE_128x64_WS] if (plain and g.M <= 8192 and not g.ln and not g.geglu) else []))


# ---- the projection GEMMs' route (csrc/pgemm.hip) -------------------------------------------------------------------------------------
def pgemm_key(M, N, K, geglu, vt, res, Rp, rowstats=False, lora_t=False, dual=False):
    kind = (("g" if geglu else "") + ("v" if vt else "") + ("r" if res else "") + (f"l{Rp}" if Rp else "")
            + ("s" if rowstats else "") + ("t" if lora_t else "") + ("d" if dual else ""))
    return (M, N, K, kind)


def takes_pgemm(g, pgemm_cfg):
    """Does aldm_pgemm take this launch?  pgemm_cfg: the measured pgemm table ((M, N, K, kind) -> configuration; an entry equal to
    PGEMM_USE_IGEMM keeps the GEMM on aldm_igemm)."""
    return (not g.tile and not g.ring and g.KH == 1 and g.KW == 1 and g.stride == (1, 1) and g.pad == (0, 0) and g.up_size is None
            and not g.in_dilate and g.in_act == ACT_NONE and not g.x2 and not g.x3 and g.Kpad == g.C1 and g.C1 in PGEMM_K
            and g.N % 64 == 0 and g.out_dtype == OUT_BF16 and g.out_pix_stride == 1 and g.out_pix_offset == 0
            and g.out_batch_stride == g.OH * g.OW * g.out_ld and g.out_ld % 8 == 0 and not g.rowbias and g.out_act == ACT_NONE
            and g.post_act == ACT_NONE and not g.res2 and not g.out2 and g.alpha == 1.0 and (not g.lora_t_out or g.Rp)
            and g.splits in (None, 1) and g.gn_groups is None and (not g.vt_dual or g.vt)
            and not g.qstats
            and (not g.Rp or (99 if g.ranks_used is None else g.ranks_used) <= 32)
            # aldm_pgemm folds a LayerNorm in its V^T and GEGLU forms only: a plain LayerNorm-folded linear stays on aldm_igemm
            and (not g.ln or (g.ln_parts is not None and g.ln_parts <= 16 and (g.vt or g.geglu)))
            and not (g.geglu and (g.res or g.vt or g.Rp or g.rowstats))
            and not (g.vt and (g.res or g.rowstats or g.vt_col0 % 32 or (g.vt_col0 <= 0 and not g.vt_dual) or g.vt_col0 < 0))
            and (not g.res or g.res_dense)
            and pgemm_cfg.get(pgemm_key(g.M, g.N, g.C1, g.geglu, g.vt, g.res, g.Rp, g.rowstats, g.lora_t_out, g.vt_dual)) != PGEMM_USE_IGEMM)


# ---- plan() -----------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class LaunchPlan:
    route: str                                   # "pgemm" | "igemm"; a pgemm plan holds nothing else (aldm_pgemm_plan decides the rest)
    key: Optional[str] = None                    # tuning-table key; None when the caller fixed tile or ring
    tile: int = 0
    ring: int = 0
    splits: int = 1                              # as requested of the library; aldm_igemm_effective_splits may clamp it
    gn_defer: bool = False
    qstats: Optional[Tuple[int, int, int]] = None   # GroupNorm hand-over table: (rows, bm, tpi) -- fp32 [rows][2][N / 4][2]; bm: rows per
    #                                              generic M-tile, tpi > 0: image-aligned halo tiles (ops.QStats)
    rowstats_cols: Optional[int] = None          # LayerNorm hand-over table: fp32 [M][rowstats_cols][2]
    halo: Tuple[int, ...] = ()                   # the halo candidates a tuner was / would be handed


def plan(g, tuned, tuner: Optional[Callable] = None, pgemm_cfg=None, legacy_keys=False):
    """How to launch g.  tuned: key -> (tile, ring, splits), the measured table; tuner(key, g, splits, halo) -> (tile, ring, splits)
    replaces the lookup while tools/autotune.py searches; pgemm_cfg: the pgemm table, None = aldm_pgemm is switched off."""
    if pgemm_cfg is not None and takes_pgemm(g, pgemm_cfg):
        return LaunchPlan("pgemm")
    tile, ring, splits = g.tile, g.ring, g.splits
    if g.rowstats and splits is None:
        splits = 1                                       # the statistics come out of the (single) epilogue
    key, halo, gn_defer = None, None, g.gn_defer
    if not tile and not ring:
        # the measured table (tuned_gfx950.json, written by tools/autotune.py) where it has this GEMM, else the heuristics below
        key = launch_key(g, splits, gn_defer=gn_defer)
        halo = halo_candidates(g)
        cfg = tuned.get(key)
        if cfg is None and legacy_keys:
            cfg = tuned.get(launch_key(g, splits, True, gn_defer))
        if cfg is not None and TILES[cfg[0]].halo and cfg[0] not in halo:
            if os.environ.get("ALDM_VERBOSE_TUNED") == "1":
                print(f"[ops] table entry {cfg} of '{key}' names a halo tile this geometry cannot take: heuristics instead", file=sys.stderr)
            cfg = None                                   # never trust a table entry into a tile this geometry cannot take
        if tuner is not None:
            cfg = tuner(key, g, splits, halo)
        if cfg is not None:
            tile, ring, splits = cfg
            if g.x3 and TILES[tile].halo:
                ring = FUSED_HALO_RING
    if g.gn_in:
        # GroupNorm of the input inside the launch: the tile is normalised once in LDS, by the loader waves of a wave-specialised halo tile
        if not (tile and TILES[tile].halo):
            tile, ring = (halo_candidates(g) if halo is None else halo)[0], GNIN_RING
        splits = 1
    if splits is None:
        splits = auto_splits(g.M, g.N, g.ktiles) if (g.can_split and not (tile and TILES[tile].halo)) else 1
    if not tile:
        tile = heuristic_cfg(g.M, g, g.ktiles, g.can_split, g.fast_path, g.vt, splits)[0]
    if not ring:
        ring = _ring_for(tile, g, splits)
    t = TILES[tile]
    qs = None
    if (g.qstats and splits == 1 and not g.vt and not g.geglu and not g.out_f32 and not g.out2 and g.out_pix_stride == 1
            and not g.Rp and not g.ln and not g.rowstats
            and g.N % 8 == 0 and g.N % t.bn == 0 and g.out_ld == g.N):
        if t.halo:
            if not g.conv1d:                             # (a conv1d halo launch has no image rows to align the table to: no table)
                tpi = math.ceil(g.OH / (t.bm // g.OW))
                qs = (g.B * tpi, 0, tpi)
        elif g.OH * g.OW >= t.bm:
            qs = (math.ceil(g.M / t.bm), t.bm, 0)
    cols = None
    if g.rowstats:
        if t.halo or g.N % t.bn or splits != 1:
            tile, splits = _lib.TILE_64x64, 1            # always legal: conv() checked N % 64 == 0
            ring = _ring_for(tile, g, 1)
        cols = g.N // TILES[tile].bn
    return LaunchPlan("igemm", key, tile, ring, splits, gn_defer, qs, cols, tuple(halo or ()))
