"""Test helper: a float64 restatement of the forward forms of ops.conv (the implicit-GEMM convolution family of csrc/igemm*.hip), written
from the formula of a convolution and the argument meanings in ops.conv's docstring, not from the kernels: an explicit tap loop over a
zero-padded float64 image.  Layout: channels-last [B, H, W, C] float64, every value bf16-representable; Conv2d weights [Cout, Cin, KH, KW];
the fused 1x1 segment's weight [Cout, C3 + C4] (the layout of ops.pack_conv_shortcut: appended to every weight row, its bias added to the
convolution's).

`reference(case)` returns, per output element,

  exact    everything in float64;
  rounded  the same value with ONE bf16 rounding, at the store (and one at the `out2` store).  Split-K adds no rounding point: the
           partial slabs are fp32 and the reduce sums them in fp32 before the one epilogue, so a split launch has the contract of an
           unsplit one;
  mag, n   sum |x_i w_i| + |bias| + |row bias| + |res| + |res2| and the number of summed terms.

The bound has nothing measured in it (vocoder_restatement.f32_bound, extended by the bf16 store):

  b32   = (n + 1) 2^-24 mag                      any-order fp32 summation of n terms
  bound = b32                                    fp32 output
  bound = b32 + half_ulp_bf16(|exact| + b32)     bf16 output: the fp32 value lies within b32 of `exact`, its store rounds once

half_ulp_bf16(t) = 2^(floor(log2 t) - 8): bf16 keeps 8 significant bits, so a value in [2^e, 2^(e+1)) is stored within 2^(e-8).  (Written
as a multiple of t this is between 2^-9 t and 2^-8 t; 2^-9 t alone is below the format's own rounding for most values -- `rounded` fails
it, see test_conv_restatement_host.py::test_half_ulp_is_the_formats -- so the exact half-ulp is used.)  Leaky ReLU is 1-Lipschitz and
exact and passes the bound through; SiLU multiplies it by its Lipschitz constant and adds SILU_MARGIN x the error one float32 CPU silu
shows on the same arguments.

`mutant=` computes a deliberately wrong variant (tests/test_conv_restatement_host.py proves `check_elem` rejects each at every shape of
tests/test_gpu_conv_edges.py).  `old_close` is the comparator of tests/test_gpu_ops.py's conv tests as it stood when this was written:
data about the past, for the host test's table only.
"""
import math
import zlib
from functools import lru_cache

import torch

from bwd_restatement import F64, bf16_input, check, r16

BK = 64
LRELU_SLOPE = float(torch.tensor(0.1, dtype=torch.float32))    # the fp32 value the kernel multiplies by
IN_SLOPE = 0.25            # in_act: a power of two, so the activated input is bf16-representable and the gather adds no rounding point
SILU_LIP = 1.1             # max |d/dx x sigmoid(x)| = 1.0998...
SILU_MARGIN = 8.0          # the reasoning of TANH_MARGIN / TN_MARGIN: the unit is what one correctly-working float32 implementation shows on the same arguments

MUTANTS = ("pad_right_wrap", "pad_bottom_next", "up_round", "concat8", "ktile_dropped", "ktile_twice", "rowbias_tile_first",
           "res_before_act", "alpha_on_res2", "x4_reads_x3", "stride_no_pad", "k_elem_lastcol")
BF16_ONLY = ("res_before_act", "alpha_on_res2")                # graded on the bf16 output only


def cdiv(a, b):
    return -(-a // b)


def silu(v):
    return v * torch.sigmoid(v)


def lrelu(v, slope):
    return torch.where(v >= 0, v, v * slope)


def _act(v, kind, slope=LRELU_SLOPE):
    return v if kind is None else (silu(v) if kind == "silu" else lrelu(v, slope))


def silu_unit(arg):
    """The largest |float32 CPU silu - float64 silu| on these arguments (as float32 arguments): measured on the reference."""
    a32 = arg.to(torch.float32)
    return float((torch.nn.functional.silu(a32).to(F64) - silu(a32.to(F64))).abs().max())


def half_ulp_bf16(t):
    """2^(floor(log2 t) - 8) per element (0 at t = 0): the largest distance from a value of magnitude t to the nearest bf16."""
    _, e = torch.frexp(t)                                      # t = m 2^e, m in [0.5, 1)
    return torch.where(t > 0, torch.ldexp(torch.ones_like(t), e - 9), torch.zeros_like(t))


# ---------------------------------------------------------------------------------------------------------------------------------
# cases and draws
# ---------------------------------------------------------------------------------------------------------------------------------
def case(name, B, IH, IW, C1, N, C2=0, k=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), up=None, C3=0, C4=0, bias=True, rowbias=False,
         res=False, res2=False, alpha=1.0, in_act=False, out_act=None, post_act=None, out2=False):
    """One convolution problem as a hashable tuple of items (`dict(c)` reads it).  up: the virtual (up-sampled) input size or None."""
    return tuple(sorted(dict(name=name, B=B, IH=IH, IW=IW, C1=C1, C2=C2, N=N, k=k, stride=stride, pad=pad, dil=dil, up=up, C3=C3, C4=C4,
                             bias=bias, rowbias=rowbias, res=res, res2=res2, alpha=alpha, in_act=in_act, out_act=out_act,
                             post_act=post_act, out2=out2).items()))


def out_hw(c):
    c = dict(c)
    VH, VW = c["up"] if c["up"] is not None else (c["IH"], c["IW"])
    (KH, KW), (sh, sw), (ph, pw), (dh, dw) = c["k"], c["stride"], c["pad"], c["dil"]
    return (VH + 2 * ph - dh * (KH - 1) - 1) // sh + 1, (VW + 2 * pw - dw * (KW - 1) - 1) // sw + 1


def _randn(shape, seed, scale=1.0):
    return bf16_input(torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale)


@lru_cache(maxsize=None)
def draw(c):
    """Fixed-seed inputs of a case: unit gaussians, weights scaled by fan_in^-0.5, every image its own seed stream."""
    d = dict(c)
    s = zlib.crc32(d["name"].encode()) % 1000003
    B, N, Ct = d["B"], d["N"], d["C1"] + d["C2"]
    OH, OW = out_hw(c)
    img = lambda C, h, w, o: torch.stack([_randn((h, w, C), s + 7919 * b + o) for b in range(B)])
    t = dict(x=img(d["C1"], d["IH"], d["IW"], 1))
    t["x2"] = img(d["C2"], d["IH"], d["IW"], 2) if d["C2"] else None
    Cext = d["C3"] + d["C4"]
    fan = d["k"][0] * d["k"][1] * Ct + Cext
    t["w"] = _randn((N, Ct) + tuple(d["k"]), s + 3, fan ** -0.5)
    t["w_sc"] = _randn((N, Cext), s + 4, fan ** -0.5) if Cext else None
    t["x3"] = img(d["C3"], OH, OW, 5) if d["C3"] else None
    t["x4"] = img(d["C4"], OH, OW, 6) if d["C4"] else None
    t["bias"] = _randn((N,), s + 8) if d["bias"] else None
    t["rowbias"] = _randn((B, N), s + 9) if d["rowbias"] else None
    t["res"] = img(N, OH, OW, 10) if d["res"] else None
    t["res2"] = img(N, OH, OW, 11) if d["res2"] else None
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def nearest_src(O, I, mutant=None):
    """nearest up-sampling: src = floor(dst * I / O)."""
    dst = torch.arange(O)
    if mutant == "up_round":
        return ((2 * dst + 1) * I) // (2 * O)                  # the source whose centre is nearest: floor((dst + 0.5) I / O)
    return (dst * I) // O


def virtual_image(x, x2, up, mutant=None):
    """x | x2 (virtual concat), then nearest up-sampling to `up` -> [B, VH, VW, C1 + C2]."""
    v = x if x2 is None else torch.cat([x, x2], dim=-1)
    if mutant == "concat8" and x2 is not None:
        v = v.clone()
        v[..., x.shape[3] - 8:x.shape[3]] = x2[..., :8]        # the last 8 channels of x from the first 8 of x2
    if up is not None:
        v = v[:, nearest_src(up[0], x.shape[1], mutant)][:, :, nearest_src(up[1], x.shape[2], mutant)]
    return v


def padded_image(v, ph, pw, mutant=None):
    """Zero padding of ph rows / pw columns on every side (and ph spare zero rows below, which only the stride mutant reads)."""
    B, VH, VW, C = v.shape
    p = torch.zeros(B, VH + 3 * ph, VW + 2 * pw, C, dtype=F64)
    p[:, ph:ph + VH, pw:pw + VW] = v
    if mutant == "pad_right_wrap":                             # flat pixel index (b VH + r) VW + VW + j: the next row's (next image's) first pixels
        flat = torch.cat([v.reshape(B * VH * VW, C), torch.zeros(pw, C, dtype=F64)])
        for j in range(pw):
            p[:, ph:ph + VH, pw + VW + j] = flat[torch.arange(B * VH).view(B, VH) * VW + VW + j]
    if mutant == "pad_bottom_next":                            # the rows below an image are the next image's first rows
        for i in range(min(ph, VH)):
            p[:-1, ph + VH + i, pw:pw + VW] = v[1:, i]
    return p


def reference(c, mutant=None, bm=64):
    """The convolution of case c -> dict(exact, rounded, mag, n, lip, unit [, exact2, rounded2, lip2, unit2]).  bm: rows per M-tile, read
    by the rowbias_tile_first mutant only."""
    d, t = dict(c), draw(c)
    assert abs(d["alpha"]) <= 1.0                              # mag below sums |res| and |res2| unscaled: an upper bound while |alpha| <= 1
    x, x2 = t["x"], t["x2"]
    if d["in_act"]:
        x, x2 = lrelu(x, IN_SLOPE), (lrelu(x2, IN_SLOPE) if x2 is not None else None)
    B, N = d["B"], d["N"]
    (KH, KW), (sh, sw), (ph, pw), (dh, dw) = d["k"], d["stride"], d["pad"], d["dil"]
    OH, OW = out_hw(c)
    v = virtual_image(x, x2, d["up"], mutant)
    C = v.shape[3]
    p = padded_image(v, ph, pw, mutant)
    Ktot, Cext = KH * KW * C, d["C3"] + d["C4"]
    kmul = torch.ones(Ktot + Cext, dtype=F64)                  # per K index (tap-major, channel-minor, then the 1x1 segment)
    if mutant in ("ktile_dropped", "ktile_twice"):             # the tail 64-wide K-tile: the last one of the last split
        kmul[(cdiv(Ktot + Cext, BK) - 1) * BK:] = 0.0 if mutant == "ktile_dropped" else 2.0
    acc = torch.zeros(B, OH, OW, N, dtype=F64)
    mag = torch.zeros(B, OH, OW, N, dtype=F64)
    y0 = ph if mutant == "stride_no_pad" else 0                # the window of output row oy starts at oy sh instead of oy sh - ph
    for kh in range(KH):
        for kw in range(KW):
            tap = kh * KW + kw
            patch = p[:, y0 + kh * dh:y0 + kh * dh + (OH - 1) * sh + 1:sh, kw * dw:kw * dw + (OW - 1) * sw + 1:sw]
            wt = t["w"][:, :, kh, kw] * kmul[tap * C:(tap + 1) * C]
            if mutant == "k_elem_lastcol" and (kh, kw) == (KH // 2, KW // 2):
                wt = wt.clone()
                wt[N - 1, int(wt[N - 1].abs().argmax())] = 0.0   # one channel of the centre tap (never a padding pixel; its largest weight, so
                #                                                  that the draw cannot make the mistake invisible), output column N - 1 only
            acc += patch @ wt.t()
            mag += patch.abs() @ t["w"][:, :, kh, kw].abs().t()
    if Cext:                                                   # the 1x1 segment over the OUTPUT pixels
        x3, x4 = t["x3"], t["x4"]
        if mutant == "x4_reads_x3" and x4 is not None:
            x4 = x3[..., torch.arange(d["C4"]) % d["C3"]]
        e = x3 if x4 is None else torch.cat([x3, x4], dim=-1)
        acc += e @ (t["w_sc"] * kmul[Ktot:]).t()
        e0 = t["x3"] if t["x4"] is None else torch.cat([t["x3"], t["x4"]], dim=-1)
        mag += e0.abs() @ t["w_sc"].abs().t()
    n = Ktot + Cext
    pre = acc
    if t["bias"] is not None:
        pre, mag, n = pre + t["bias"], mag + t["bias"].abs(), n + 1
    if t["rowbias"] is not None:
        img = torch.arange(B * OH * OW) // (OH * OW)
        if mutant == "rowbias_tile_first":
            img = (torch.arange(B * OH * OW) // bm * bm) // (OH * OW)
        pre, mag, n = pre + t["rowbias"][img].view(B, OH, OW, N), mag + t["rowbias"].abs().view(B, 1, 1, N), n + 1
    units, lip = [], 1.0
    if d["out_act"] == "silu":
        units, lip = units + [silu_unit(pre)], lip * SILU_LIP
    if t["res"] is not None:
        mag, n = mag + t["res"].abs(), n + 1
    if mutant == "res_before_act" and t["res"] is not None:
        val = _act(pre + t["res"], d["out_act"])
    else:
        val = _act(pre, d["out_act"])                          # out_act
        if t["res"] is not None:
            val = val + t["res"]                               # + res
    if t["res2"] is not None:
        mag, n = mag + t["res2"].abs(), n + 1
    if mutant == "alpha_on_res2" and t["res2"] is not None:
        val = d["alpha"] * (val + t["res2"])
    else:
        val = d["alpha"] * val                                 # * alpha
        if t["res2"] is not None:
            val = val + t["res2"]                              # + res2
    out = dict(mag=mag, n=n)
    units2, lip2 = list(units), lip
    if d["post_act"] == "silu":
        units2, lip2 = units2 + [silu_unit(val)], lip2 * SILU_LIP
    if d["out2"]:                                              # out = v, out2 = bf16(post_act(v)): both from the unrounded v
        post = _act(val, d["post_act"])
        out.update(exact=val, rounded=r16(val), lip=lip, unit=sum(units), exact2=post, rounded2=r16(post), lip2=lip2, unit2=sum(units2))
    else:
        val = _act(val, d["post_act"])                         # v = post_act(v), then the store
        out.update(exact=val, rounded=r16(val), lip=lip2, unit=sum(units2))
    return out


@lru_cache(maxsize=None)
def cached_reference(c):
    """reference(c): computed once per case and shared (nobody writes into it)."""
    return reference(c)


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound and the comparators
# ---------------------------------------------------------------------------------------------------------------------------------
def bound(ref, f32, second=False):
    sfx = "2" if second else ""
    b32 = ref["lip" + sfx] * (ref["n"] + 1) * 2.0 ** -24 * ref["mag"] + SILU_MARGIN * ref["unit" + sfx]
    if f32:
        return b32
    return b32 + half_ulp_bf16(ref["exact" + sfx].abs() + b32)


def elem_ratio(got, ref, f32, second=False):
    """max |got - exact| / bound (inf for a non-finite value): <= 1 passes."""
    got = got.detach().to("cpu").to(F64)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - ref["exact2" if second else "exact"]).abs() / bound(ref, f32, second)).max())


def check_elem(got, ref, what, f32=False, second=False, record=None):
    if record is None:
        import conftest
        record = conftest.record
    assert bool(torch.isfinite(got.detach().to("cpu").to(F64)).all()), f"{what}: non-finite values"
    ratio = elem_ratio(got, ref, f32, second)
    record(ratio, what + " err/bound")
    if ratio > 1.0:
        err = (got.detach().to("cpu").to(F64) - ref["exact2" if second else "exact"]).abs() / bound(ref, f32, second)
        bad = (err > 1.0).nonzero()
        raise AssertionError(f"{what}: error {ratio:.4g} x the {'fp32' if f32 else 'bf16'} bound; {len(bad)} elements, first (b, oy, ox, n) "
                             f"{bad[:6].tolist()}, columns {sorted(set(bad[:, 3].tolist()))[:12]}, rows {sorted(set(bad[:, 1].tolist()))[:12]}")


def check_both(got, ref, what, f32, second=False, record=None):
    """check_elem, and for a bf16 output also bwd_restatement.check (2 x the L2 floor, 4 x the max floor)."""
    check_elem(got, ref, what, f32, second, record)
    if not f32:
        sfx = "2" if second else ""
        check(got, ref["exact" + sfx], ref["rounded" + sfx], what, record=record)


# the comparator of the conv tests of tests/test_gpu_ops.py as it stood when this file was written (their `close` against a float32
# F.conv2d): data about the past, for the host test's table
def old_close(got, want, rtol=1.2e-2, atol=None):
    got, want = got.float(), want.float()
    atol = atol if atol is not None else 8e-3 * float(want.abs().max()) + 1e-6
    err = (got - want).abs()
    return not bool((~(err <= atol + rtol * want.abs())).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# launch arithmetic restated (the GPU test asserts it against the library, the host test against itself)
# ---------------------------------------------------------------------------------------------------------------------------------
TILE_BM = {1: 128, 2: 64, 3: 128, 4: 64, 6: 128, 7: 128, 8: 64, 9: 256, 10: 64, 11: 128, 12: 256, 13: 64, 14: 128, 15: 128, 16: 64}
HALO = (7, 8, 15, 16)
NO_DIRECT = (1, 9, 12)                                          # tiles whose instantiation has no register-direct epilogue


def nkt_of(c):
    d = dict(c)
    return cdiv(d["k"][0] * d["k"][1] * (d["C1"] + d["C2"]), BK) + (d["C3"] + d["C4"]) // BK


def split_rule(want, nkt, nch, taps, halo):
    """The split rule: even K-tile shares, no empty split; the halo tiles then split by whole 64-channel chunks."""
    s = max(1, min(want, nkt))
    s = cdiv(nkt, cdiv(nkt, s))
    if halo and s > 1:
        s = cdiv(nch, cdiv(nch, min(s, nch)))
    return s


def eff_splits(c, tile, want):
    d = dict(c)
    return split_rule(want, nkt_of(c), (d["C1"] + d["C2"]) // BK, d["k"][0] * d["k"][1], tile in HALO)


def straddles(c, bm):
    """Some bm-row M-tile holds rows of two images."""
    OH, OW = out_hw(c)
    hw, M = OH * OW, dict(c)["B"] * OH * OW
    return any(t // hw != (min(t + bm, M) - 1) // hw for t in range(0, M, bm))


def halo_need(tile, OW, k=(3, 3), dil=(1, 1)):
    """Halo rows a tile of BM / OW image rows needs (3x3: (BM / OW + 2)(OW + 2))."""
    return (TILE_BM[tile] // OW + (k[0] - 1) * dil[0]) * (OW + (k[1] - 1) * dil[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_conv_edges.py (shared with the host test, which proves the comparator sharp AT these shapes)
# ---------------------------------------------------------------------------------------------------------------------------------
FULL = dict(rowbias=True, res=True)                             # bias + row bias + res

# A. generic tiles x geometry: three images of 11 x 7 (M = 231), two of 37 x 7 (M = 518) for the 256-row tiles
A_CH = [(8, 0, 136), (72, 0, 40), (64, 0, 72), (128, 64, 136), (64, 0, 8)]
A_BASE = [case(f"A base {c1}+{c2}->{n}", 3, 11, 7, c1, n, C2=c2, **FULL) for c1, c2, n in A_CH] + [
    case("A base 64->72 no row bias", 3, 11, 7, 64, 72, res=True)]      # (77 pixels an image: with a row bias the 128-row tiles walk the LDS image)
A_BIG = [case(f"A big {c1}+{c2}->{n}", 2, 37, 7, c1, n, C2=c2, **FULL) for c1, c2, n in [(64, 0, 72), (128, 64, 136)]]
UPS = [((8, 4), (16, 8)), ((63, 4), (125, 8)), ((5, 8), (13, 16))]
A_GEOM = [case("A s2 odd", 3, 11, 7, 64, 72, stride=(2, 2), **FULL),
          case("A s2 even", 3, 12, 8, 64, 72, stride=(2, 2), **FULL),
          case("A 1x1", 3, 11, 7, 64, 72, k=(1, 1), pad=(0, 0), **FULL),
          case("A dil 2x1", 3, 11, 7, 64, 72, dil=(2, 1), pad=(2, 1), **FULL)] + [
         case(f"A up {i[0]}x{i[1]}", 2, i[0], i[1], 64, 72, C2=64, up=o, **FULL) for i, o in UPS]

# B. halo tiles at the capacity edges: two images, OH % (BM / OW) in {0, 1, rows_pt - 1}
B_CH = [(64, 0), (64, 64), (192, 0)]
B_OW = {7: (16, 8, 4, 32, 64), 15: (16, 8, 4, 32, 64), 8: (16, 4, 8), 16: (16, 4, 8)}
B_RINGS = {7: (2, 3, 4), 8: (2, 3, 4), 15: (3, 4), 16: (3, 4)}


def b_heights(tile, OW):
    r = TILE_BM[tile] // OW
    return sorted({2 * r, r + 1, 2 * r - 1} - {0})


def b_cases(tile):
    """(case, ring): every OW of the tile x the three heights, the channel sets and the ring depths cycling through them."""
    out, i = [], 0
    for OW in B_OW[tile]:
        for OH in b_heights(tile, OW):
            c1, c2 = B_CH[i % 3]
            out.append((case(f"B {OH}x{OW} {c1}+{c2}", 2, OH, OW, c1, (136, 72)[i % 2], C2=c2, **FULL), B_RINGS[tile][i % len(B_RINGS[tile])]))
            i += 1
    return out


B_ACT = case("B silu 17x8", 2, 17, 8, 64, 72, out_act="silu", res=True)       # an activation: the LDS walk as dispatched on every halo tile
B_UP = [case(f"B up {i[0]}x{i[1]}", 2, i[0], i[1], 64, 136, C2=64, up=o, **FULL) for i, o in UPS]
B_SHORTCUT = [case(f"B sc {OH}x{OW} {c3}+{c4}", 2, OH, OW, 64, 136, C3=c3, C4=c4, **FULL)
              for OH, OW in ((17, 8), (9, 16)) for c3, c4 in ((64, 0), (64, 128))]
B_FILTER = [case("B 5x5", 2, 17, 8, 64, 72, k=(5, 5), pad=(2, 2), **FULL),
            case("B 3x1", 2, 17, 8, 64, 72, k=(3, 1), pad=(1, 0), **FULL),
            case("B 3x1 w16", 2, 9, 16, 64, 72, k=(3, 1), pad=(1, 0), **FULL),
            case("B dil 2x1", 2, 17, 8, 64, 72, dil=(2, 1), pad=(2, 1), **FULL)]
B_REFUSED = [(8, case("B refused w32", 2, 4, 32, 64, 72)), (16, case("B refused w2", 2, 33, 2, 64, 72)),
             (16, case("B refused 5x5", 2, 17, 8, 64, 72, k=(5, 5), pad=(2, 2))),
             (7, case("B refused dil", 2, 17, 8, 64, 72, dil=(2, 2), pad=(2, 2)))]

# C. split-K
C_SPLITS = (2, 4, 5, 7, 9, 12)
C_GENERIC = [case(f"C nkt9 ->{n}", 3, 11, 7, 64, n, **FULL) for n in (72, 136)]
C_TAIL = [case(f"C nkt11 ->{n}", 3, 11, 7, 72, n, **FULL) for n in (72, 136)]
C_HALO = [case(f"C halo {c1}+{c2}->{n}", 2, 17, 8, c1, n, C2=c2, **FULL) for (c1, c2), n in (((192, 0), 72), ((128, 128), 136))]
C_HALO_SPLITS = (2, 3, 4, 5)
C_SHORTCUT = [case(f"C sc 128 {c3}+{c4}->{n}", 2, 17, 8, 128, n, C3=c3, C4=c4, **FULL) for (c3, c4), n in (((64, 0), 72), ((64, 128), 136))]

# D. epilogue forms
D_IMAGES = {2: ((7, 7), (11, 7)), 14: ((11, 7), (19, 7)), 16: ((5, 8), (9, 8))}     # OH x OW: below and from one tile of rows per image


def d_forms():
    return [("rowbias", dict(rowbias=True)), ("res res2 alpha", dict(res=True, res2=True, alpha=0.5, rowbias=True)),
            ("silu", dict(out_act="silu", res=True)), ("leaky", dict(out_act="lrelu", res=True, res2=True, alpha=0.5)),
            ("out2", dict(out2=True, res=True)), ("out2 leaky", dict(out2=True, post_act="lrelu", res=True)),
            ("out2 silu", dict(out2=True, post_act="silu", out_act="lrelu")), ("post silu", dict(post_act="silu", res2=True)),
            ("plain", dict())]


def d_cases(tile, N):
    return [(what, case(f"D {tile} {OH}x{OW} {what} ->{N}", 3, OH, OW, 64, N, **kw)) for OH, OW in D_IMAGES[tile] for what, kw in d_forms()]


D_IN_ACT = [case(f"D in_act {c1}->{n}", 3, 11, 7, c1, n, in_act=True, **FULL) for c1, n in ((64, 72), (8, 40))]


def all_cases():
    """Every case of the GPU file with the M-tile heights it runs under: [(case, (bm, ...))]."""
    gen = (64, 128)
    out = [(c, gen) for c in A_BASE + A_GEOM] + [(c, (256,)) for c in A_BIG]
    for tile in HALO:
        out += [(c, (TILE_BM[tile],)) for c, _ in b_cases(tile)]
    out += [(c, gen) for c in [B_ACT] + B_UP + B_SHORTCUT + B_FILTER + C_GENERIC + C_TAIL + C_HALO + C_SHORTCUT + D_IN_ACT]
    for tile in D_IMAGES:
        for N in (40, 72):
            out += [(c, (TILE_BM[tile],)) for _, c in d_cases(tile, N)]
    seen, uniq = set(), []
    for c, bms in out:
        if c not in seen:
            seen.add(c)
            uniq.append((c, bms))
    return uniq
