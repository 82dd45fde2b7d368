"""The split-K slab layouts (csrc/igemm_core.h igemm_slab_index) without a GPU: the library's host restatement of the kernels' store
address (aldm_igemm_slab_offset) against a numpy restatement -- bijection onto [0, S * B * HW * C), bounds (= the size ops.conv
asks _workspace for), a group's reads being Cg / 4 contiguous runs -- over the shapes of the UNet's denoise step at batch 8 / 2 / 1
(CFG on and off), the training step and the VAE's split-K levels; and the one split rule behind aldm_igemm_effective_splits."""
import ctypes
import os

import numpy as np
import pytest

ROWMAJOR, PLANAR = 0, 1

# (B, HW, C): B * HW rows of C channels.  HW = 64 / 252 / 1000 / 4000 are the UNet's four levels (32x2 .. 250x16 latents), C their widths
# and the widths in front of an up-block's concatenation; 17 / 130 x 16 = training crops (M not a multiple of any tile); 4096 = VAE mid.
SHAPES = [(b, hw, c) for b in (1, 2, 8) for hw in (64, 252, 1000) for c in (256, 384, 640, 1280)] + [
    (8, 4000, 128), (2, 4000, 128), (1, 4000, 256), (4, 17 * 4, 640), (4, 130 * 16, 128), (3, 33 * 2, 384), (1, 4096, 512), (16, 64, 640)]
TILES = [(64, 64), (64, 128), (128, 64), (128, 128), (256, 128)]


@pytest.fixture(scope="module")
def lib():
    from audioldm_with_lora_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def np_offset(layout, B, HW, C, split, m, n):
    """numpy restatement: row-major [S][B*HW][C]; quad-planar [S][B][C/4][HW][4]"""
    m, n = np.asarray(m, dtype=np.int64), np.asarray(n, dtype=np.int64)
    base = np.int64(split) * B * HW * C
    if layout == ROWMAJOR:
        return base + m * C + n
    b, pix = m // HW, m % HW
    return base + ((b * (C // 4) + n // 4) * HW + pix) * 4 + n % 4


def test_arguments_out_of_range_are_refused(lib):
    f = lib.aldm_igemm_slab_offset
    assert f(PLANAR, 2, 64, 640, 0, 0, 0) == 0
    for bad in [(2, 2, 64, 640, 0, 0, 0), (PLANAR, 2, 64, 640, 0, 128, 0), (PLANAR, 2, 64, 640, 0, 0, 640), (PLANAR, 2, 64, 642, 0, 0, 0),
                (PLANAR, 2, 64, 640, -1, 0, 0), (PLANAR, 0, 64, 640, 0, 0, 0), (PLANAR, 2, 64, 640, 0, -1, 0)]:
        assert f(*bad) == -1


@pytest.mark.parametrize("layout", [ROWMAJOR, PLANAR])
def test_library_offset_equals_numpy_restatement(lib, layout):
    """every row m (the magic-number division by HW is the only non-affine step) at the first, the last and a middle channel quad, and
    every channel of the first / last / an image-boundary row"""
    f = lib.aldm_igemm_slab_offset
    rng = np.random.default_rng(5)
    seen = set()
    for B, HW, C in SHAPES:
        M = B * HW
        ns = [0, C - 4, 4 * int(rng.integers(0, C // 4)) + 1, C - 1]
        if (M, HW) not in seen:                                   # the division depends on (m, HW) only
            seen.add((M, HW))
            ms = np.arange(M)
        else:
            ms = np.unique(np.concatenate([rng.integers(0, M, 256), [0, M - 1, HW - 1, min(HW, M - 1)]]))
        for s in (0, 11):
            for n in ns:
                got = np.array([f(layout, B, HW, C, s, int(m), n) for m in ms], dtype=np.int64)
                assert np.array_equal(got, np_offset(layout, B, HW, C, s, ms, n)), (B, HW, C, s, n)
        for m in {0, M - 1, HW - 1, min(HW, M - 1)}:
            got = np.array([f(layout, B, HW, C, 3, m, n) for n in range(C)], dtype=np.int64)
            assert np.array_equal(got, np_offset(layout, B, HW, C, 3, m, np.arange(C))), (B, HW, C, m)


@pytest.mark.parametrize("B,HW,C", SHAPES)
def test_planar_slab_is_a_bijection_inside_the_workspace(B, HW, C):
    M = B * HW
    m, n = np.meshgrid(np.arange(M), np.arange(C), indexing="ij")
    for S in range(2, 13):
        if S * M * C > (1 << 24) and S not in (2, 12):            # big shapes: the ends of the split range only
            continue
        lo, hi = S * M * C, -1
        for s in range(S):
            off = np_offset(PLANAR, B, HW, C, s, m.ravel(), n.ravel())
            assert off.min() == s * M * C and off.max() == (s + 1) * M * C - 1          # each slab fills exactly its own range
            if s in (0, S - 1):
                assert np.array_equal(np.sort(off), np.arange(s * M * C, (s + 1) * M * C))
            lo, hi = min(lo, int(off.min())), max(hi, int(off.max()))
        assert lo == 0 and (hi + 1) * 4 == S * M * C * 4             # == the bytes ops.conv asks _workspace for (splits * M * N * 4)


@pytest.mark.parametrize("B,HW,C", [s for s in SHAPES if s[0] * s[1] * s[2] <= 3_000_000])
@pytest.mark.parametrize("tile", TILES)
def test_tile_walk_stores_every_quad_once(B, HW, C, tile):
    """the epilogue's walk: tiles of BM x BN over (M, C), 16-byte quad stores guarded by m < M and n < C (M, C no multiples of the tile)"""
    BM, BN = tile
    M = B * HW
    hits = np.zeros(M * C // 4, dtype=np.int32)
    for m0 in range(0, M, BM):
        for n0 in range(0, C, BN):
            mm, nn = np.meshgrid(np.arange(m0, m0 + BM), np.arange(n0, n0 + BN, 4), indexing="ij")
            keep = (mm < M) & (nn < C)
            off = np_offset(PLANAR, B, HW, C, 0, mm[keep], nn[keep])
            assert (off % 4 == 0).all() and off.min() >= 0 and off.max() + 4 <= M * C
            np.add.at(hits, off // 4, 1)
    assert (hits == 1).all()


@pytest.mark.parametrize("B,HW,C,C2,groups", [(8, 64, 640, 0, 32), (8, 64, 640, 640, 32), (8, 252, 640, 384, 32), (8, 252, 384, 0, 32),
                                             (2, 1000, 256, 0, 32), (8, 1000, 256, 256, 32), (8, 1000, 384, 0, 32), (1, 4000, 128, 0, 32),
                                             (4, 68, 640, 384, 32), (2, 64, 128, 128, 32), (2, 252, 96, 0, 8)])
def test_a_groups_reads_are_contiguous_runs(B, HW, C, C2, groups):
    """what one (image, group) workgroup of the deferred GroupNorm reads from a slab: Cg / 4 runs of HW * 4 floats (one per quad
    plane; the planes of a group follow each other), against HW pieces of Cg floats in the row-major slab"""
    Cg = (C + C2) // groups
    assert (C + C2) % groups == 0 and Cg % 4 == 0 and C % Cg == 0
    for b in (0, B - 1):
        for g in range(C // Cg):                                   # groups of the first source (the others come from x2, not the slab)
            pix, c = np.meshgrid(np.arange(HW), np.arange(g * Cg, (g + 1) * Cg), indexing="ij")
            off = np.sort(np_offset(PLANAR, B, HW, C, 1, b * HW + pix.ravel(), c.ravel()))
            runs = np.split(off, np.nonzero(np.diff(off) != 1)[0] + 1)
            assert len(runs) == 1 and len(runs[0]) == HW * Cg      # Cg / 4 planes of HW * 4 floats, back to back
            for q in range(Cg // 4):
                plane = np_offset(PLANAR, B, HW, C, 1, b * HW + np.arange(HW), g * Cg + 4 * q)
                assert np.array_equal(plane, plane[0] + 4 * np.arange(HW))
            rm = np.sort(np_offset(ROWMAJOR, B, HW, C, 1, b * HW + pix.ravel(), c.ravel()))
            assert len(np.split(rm, np.nonzero(np.diff(rm) != 1)[0] + 1)) == (HW if Cg < C else 1)


def _args(_lib, Cin, Cin2, C3, tile, splits, K=3):
    a = _lib.IgemmArgs()
    a.B, a.IH, a.IW, a.OH, a.OW, a.Cin, a.Cin2, a.Cout = 8, 32, 2, 32, 2, Cin, Cin2, 640
    a.KH = a.KW = K
    a.x3, a.Cin3 = (1 if C3 else None), C3                        # (never dereferenced by the host-side planner)
    a.tile, a.splits = tile, splits
    return a


def test_effective_splits_is_the_launch_rule():
    """generic clamp first (whole 64-wide K-tiles per split), then the halo tiles' per-chunk rule ON THE CLAMPED COUNT -- the order the
    launch applies them in.  The fused x3 | x4 segment adds K-tiles to the clamp but no chunk to the halo rule: for Cin = 768,
    C3tot = 64, splits = 12 the two used to disagree (12 slabs summed, 6 written)."""
    from audioldm_with_lora_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    f = _lib.load().aldm_igemm_effective_splits

    def rule(Cin, C3, K, halo, want):
        nkt = -(-K * K * Cin // 64) + C3 // 64
        s = min(max(want, 1), nkt)
        s = -(-nkt // -(-nkt // s))
        if halo and s > 1:
            nch = Cin // 64
            s = -(-nch // -(-nch // min(s, nch)))
        return s

    assert f(ctypes.byref(_args(_lib, 768, 0, 64, 15, 12))) == rule(768, 64, 3, True, 12) == 6
    for Cin, Cin2 in ((640, 0), (768, 0), (640, 384), (1280, 640), (256, 0), (64, 0)):
        for C3 in (0, 64, 640):
            for tile in (2, 4, 10, 13, 7, 8, 15, 16):
                for want in range(1, 17):
                    got = f(ctypes.byref(_args(_lib, Cin, Cin2, C3, tile, want)))
                    assert got == rule(Cin + Cin2, C3, 3, tile in (7, 8, 15, 16), want), (Cin, Cin2, C3, tile, want)
                    assert 1 <= got <= max(want, 1)
