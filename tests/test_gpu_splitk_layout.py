"""GPU: the quad-planar slab layout of a deferred split-K reduce (and write-through slab stores) against the row-major path.

conv(defer=...) -> groupnorm() per tile family that can defer, at one UNet shape per level: (a) the consumer's two outputs (the
block output it fills and the norm) are EQUAL BIT FOR BIT across {row-major, quad-planar} x {plain, write-through} -- the partials
are the same fp32 values added in the same order, only their address changes; (b) the result meets the fp32 F.conv2d +
F.group_norm bound of tests/test_gpu_ops.py.  Row bias, residual, a concatenated skip tensor (x2) and the kept sum are all present."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def bf(x):
    return x.to(torch.bfloat16).float()


def close(got, want, rtol=1.2e-2, atol=None):          # the bound of tests/test_gpu_ops.py
    want = want.float()
    got = got.float().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if atol is None:
        atol = 8e-3 * float(want.abs().max()) + 1e-6
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    bad = ~(err <= bound)
    assert not bad.any(), f"max err {float(err.max()):.4g} (ref max {float(want.abs().max()):.4g}), {int(bad.sum())} bad"


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)


def to_nchw(y):
    return y.float().cpu().permute(0, 3, 1, 2)


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    return o


# tile, (B, H, W), Cin, Cout, C2 (skip channels in front of the norm), splits, ext (channels of the fused 1x1 shortcut source, 0 = res)
CASES = [
    (2, (8, 32, 2), 640, 640, 640, 6, 0),       # pipe 64x64, 64-token level, up-block norm over cat([h, skip])
    (4, (8, 63, 4), 384, 640, 384, 4, 0),       # pipe 64x128, 252-token level (M = 2016: not a multiple of 128), 20 + 12 channels per group
    (3, (3, 63, 4), 256, 384, 0, 3, 0),         # pipe 128x64, M = 756 ragged
    (1, (2, 125, 8), 128, 256, 0, 2, 0),        # pipe 128x128, 1000-pixel level, group width 8
    (13, (8, 32, 2), 640, 640, 0, 6, 0),        # wave-specialised 64x128
    (14, (8, 63, 4), 384, 384, 0, 4, 0),        # wave-specialised 128x64
    (10, (8, 32, 2), 640, 640, 640, 5, 0),      # 8-wave 64x128
    (11, (3, 63, 4), 384, 640, 384, 4, 0),      # 8-wave 128x64
    (6, (2, 125, 8), 256, 256, 0, 3, 0),        # 8-wave 128x128
    (7, (8, 32, 2), 640, 640, 0, 5, 0),         # halo 128x128: splits by 64-channel chunk
    (8, (3, 63, 4), 384, 384, 0, 3, 0),         # halo 64x128
    (15, (2, 125, 8), 256, 256, 0, 2, 0),       # halo 128x128, wave-specialised
    (16, (3, 63, 4), 384, 640, 384, 3, 0),      # halo 64x128, wave-specialised
    (15, (2, 125, 8), 192, 256, 0, 2, 128),     # conv2 + conv_shortcut as one launch (x3), deferred
    (16, (3, 63, 4), 192, 256, 0, 3, 128),
    (13, (8, 32, 2), 128, 128, 0, 7, 192),      # the same on the small wave-specialised tile, split boundary inside the segment
]


@pytest.mark.parametrize("tile,shape,Cin,Cout,C2,splits,ext", CASES)
def test_planar_slabs_equal_rowmajor_bit_for_bit(ops, tile, shape, Cin, Cout, C2, splits, ext):
    from audioldm_with_lora_amd import _lib
    B, H, W = shape
    groups = 32
    g = torch.Generator().manual_seed(500 + tile + splits)
    x = bf(torch.randn(B, Cin, H, W, generator=g))
    w = bf(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g)
    temb = torch.randn(B, Cout + 8, generator=g)
    skip = bf(torch.randn(B, C2, H, W, generator=g) * 1.5 + 0.3) if C2 else None
    gamma, beta = torch.randn(Cout + C2, generator=g), torch.randn(Cout + C2, generator=g)
    if ext:
        xa = bf(torch.randn(B, ext, H, W, generator=g))
        wsc, bsc = bf(torch.randn(Cout, ext, 1, 1, generator=g) / math.sqrt(ext)), torch.randn(Cout, generator=g)
        want_h = F.conv2d(x, w, b, padding=1) + F.conv2d(xa, wsc, bsc) + temb[:, 8:, None, None]
        pw = ops.pack_conv_shortcut(w.to(DEV), b.to(DEV), wsc.to(DEV), bsc.to(DEV))
        kw = dict(x3=nhwc(xa), ring=3)
    else:
        r = bf(torch.randn(B, Cout, H, W, generator=g))
        want_h = F.conv2d(x, w, b, padding=1) + temb[:, 8:, None, None] + r
        pw = ops.pack_conv(w.to(DEV), b.to(DEV))
        kw = dict(res=nhwc(r))
    cat = torch.cat([bf(want_h), skip], 1) if C2 else want_h
    want_n = F.silu(F.group_norm(cat, groups, gamma, beta, 1e-5))
    td = temb.to(DEV)
    xd, sd, gd, bd = nhwc(x), (nhwc(skip) if C2 else None), gamma.to(DEV), beta.to(DEV)

    def run(layout, wt):
        d = ops.conv(xd, pw, pad=(1, 1), rowbias=td[:, 8:], rowbias_ld=Cout + 8, splits=splits, tile=tile, defer=(Cout + C2, groups),
                     slab_layout=layout, slab_wt=wt, **kw)
        assert isinstance(d, ops.Deferred) and d.eff > 1 and d.layout == layout
        y = ops.groupnorm(d, gd, bd, groups, 1e-5, ops.ACT_SILU, x2=sd)
        torch.cuda.synchronize()
        return ops.tensor_of(d).clone(), y.clone()

    h0, y0 = run(_lib.SLAB_ROWMAJOR, False)
    close(to_nchw(h0), want_h)
    close(to_nchw(y0), want_n, rtol=1.5e-2)
    for layout, wt in ((_lib.SLAB_PLANAR, False), (_lib.SLAB_PLANAR, True), (_lib.SLAB_ROWMAJOR, True)):
        h1, y1 = run(layout, wt)
        assert torch.equal(h1, h0) and torch.equal(y1, y0), (layout, wt)
        close(to_nchw(h1), want_h)
        close(to_nchw(y1), want_n, rtol=1.5e-2)


@pytest.mark.parametrize("B,HW,C,C2,groups,splits", [(8, 64, 640, 640, 32, 6), (8, 252, 640, 384, 32, 4), (2, 1000, 256, 0, 32, 3),
                                                     (3, 252, 384, 0, 32, 12), (2, 64, 128, 0, 8, 5)])
def test_groupnorm_partials_over_both_layouts(ops, B, HW, C, C2, groups, splits):
    """aldm_groupnorm_partials_layout over a quad-planar workspace == the same call over the row-major one, bit for bit (the planar
    workspace is the row-major one permuted on the host: [S][B][HW][C/4][4] -> [S][B][C/4][HW][4])"""
    from audioldm_with_lora_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(77 + splits)
    ws = (torch.randn(splits, B, HW, C // 4, 4, generator=g) * 3).to(DEV)
    wp = ws.permute(0, 1, 3, 2, 4).contiguous()
    bias, rb = torch.randn(C, generator=g).to(DEV), torch.randn(B, C + 4, generator=g).to(DEV)
    res = torch.randn(B, HW, C, generator=g).to(torch.bfloat16).to(DEV)
    x2 = torch.randn(B, HW, C2, generator=g).to(torch.bfloat16).to(DEV) if C2 else None
    gamma, beta = torch.randn(C + C2, generator=g).to(DEV), torch.randn(C + C2, generator=g).to(DEV)
    outs = []
    for layout, w_ in ((_lib.SLAB_ROWMAJOR, ws), (_lib.SLAB_PLANAR, wp)):
        y = torch.full((B, HW, C + C2), float("nan"), dtype=torch.bfloat16, device=DEV)
        s = torch.full((B, HW, C), float("nan"), dtype=torch.bfloat16, device=DEV)
        rc = lib.aldm_groupnorm_partials_layout(w_.data_ptr(), splits, B, HW, C, bias.data_ptr(), rb.data_ptr(), C + 4, res.data_ptr(),
                                                s.data_ptr(), (x2.data_ptr() if C2 else None), C2, groups, 1e-5, gamma.data_ptr(),
                                                beta.data_ptr(), 1, y.data_ptr(), layout, None)
        assert rc == 0, lib.aldm_last_error()
        torch.cuda.synchronize()
        outs.append((s, y))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[1][0].float()).all() and torch.isfinite(outs[1][1].float()).all()
    want_s = ws.sum(0).reshape(B, HW, C).float() + bias + rb[:, None, :C] + res.float()
    close(outs[1][0], want_s.cpu())
    assert lib.aldm_groupnorm_partials_layout(wp.data_ptr(), splits, B, HW, C, None, None, 0, None, None, None, 0, groups, 1e-5,
                                              gamma.data_ptr(), beta.data_ptr(), 1, outs[0][1].data_ptr(), 2, None) != 0   # unknown layout


def test_effective_splits_equals_launched_splits_with_the_fused_segment(ops):
    """Cin = 768, C3tot = 64, splits = 12 on a halo tile: the generic clamp (109 K-tiles -> 11) and then the per-chunk rule (12 chunks
    -> 6) -- aldm_igemm_effective_splits used to say 12.  The launch writes exactly `eff` slabs: the slabs behind them keep their NaNs."""
    from audioldm_with_lora_amd import _lib
    B, H, W, Cin, Cout, C3 = 2, 125, 8, 768, 128, 64
    g = torch.Generator().manual_seed(9)
    x, xa = bf(torch.randn(B, Cin, H, W, generator=g)), bf(torch.randn(B, C3, H, W, generator=g))
    w, b = bf(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)), torch.randn(Cout, generator=g)
    wsc, bsc = bf(torch.randn(Cout, C3, 1, 1, generator=g) / math.sqrt(C3)), torch.randn(Cout, generator=g)
    pw = ops.pack_conv_shortcut(w.to(DEV), b.to(DEV), wsc.to(DEV), bsc.to(DEV))
    M = B * H * W
    gamma, beta = torch.randn(Cout, generator=g).to(DEV), torch.randn(Cout, generator=g).to(DEV)
    want = F.conv2d(x, w, b, padding=1) + F.conv2d(xa, wsc, bsc)
    for layout in (_lib.SLAB_ROWMAJOR, _lib.SLAB_PLANAR):
        wsbuf = ops._workspace(12 * M * Cout * 4, torch.device(DEV, torch.cuda.current_device()))
        wsbuf.fill_(float("nan"))
        d = ops.conv(nhwc(x), pw, pad=(1, 1), x3=nhwc(xa), tile=15, ring=3, splits=12, defer=(Cout, 32), slab_layout=layout)
        assert isinstance(d, ops.Deferred) and d.ws == wsbuf.data_ptr()
        assert d.eff == 6
        torch.cuda.synchronize()
        slabs = wsbuf[:12 * M * Cout].view(12, M * Cout)
        written = [bool(torch.isfinite(s).all()) for s in slabs]
        untouched = [bool(torch.isnan(s).all()) for s in slabs]
        assert written == [True] * d.eff + [False] * (12 - d.eff) and untouched == [False] * d.eff + [True] * (12 - d.eff)
        y = ops.groupnorm(d, gamma, beta, 32, 1e-5, ops.ACT_SILU)
        close(to_nchw(ops.tensor_of(d)), want)
        close(to_nchw(y), F.silu(F.group_norm(want, 32, gamma.cpu(), beta.cpu(), 1e-5)), rtol=1.5e-2)


def test_backward_groupnorm_refuses_planar_slabs(ops):
    """groupnorm_bwd sums row-major slabs: a quad-planar Deferred is refused, never misread"""
    from audioldm_with_lora_amd import _lib
    g = torch.Generator().manual_seed(3)
    x = nhwc(bf(torch.randn(2, 128, 32, 2, generator=g)))
    pw = ops.pack_conv(bf(torch.randn(128, 128, 3, 3, generator=g) * 0.03).to(DEV), None)
    gamma, beta = torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
    d = ops.conv(x, pw, pad=(1, 1), splits=4, tile=2, defer=(128, 32), slab_layout=_lib.SLAB_PLANAR)
    assert isinstance(d, ops.Deferred) and d.layout == _lib.SLAB_PLANAR
    with pytest.raises(_lib.AldmError, match="row-major"):
        ops.groupnorm_bwd(x, d, gamma, beta, 32, 1e-5, ops.ACT_NONE)
    ops.drop_pending(x)
