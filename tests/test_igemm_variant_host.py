"""The native half of the conv dispatch on the CPU: aldm_igemm_variant (csrc/igemm_select.hip) answers, for every aldm_igemm argument
struct recorded on the MI355X (tests/golden/igemm_launch_plans.json.gz), with the kernel the GPU was seen to run for it
(tests/golden/igemm_kernel_variants.json.gz, recorded by tools/record_launch_plans.py --kernels on the commit before the selection
existed); the library's tile table equals igemm_plan.TILES; the documented refusals keep their code and text."""
import ctypes as C
import gzip
import json
import os

import pytest

from audioldm_with_lora_amd import _lib, igemm_plan as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_ARG, E_UNSUPPORTED = -1, -3
POINTERS = [n for n, t in _lib.IgemmArgs._fields_ if t is C.c_void_p]


def _load(name):
    with gzip.open(os.path.join(GOLDEN, name), "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def recorded():
    """[(record, {"name", "grid", "block", "lds"})] of every igemm record of the launch-plan fixture"""
    plans, kernels = _load("igemm_launch_plans.json.gz"), _load("igemm_kernel_variants.json.gz")
    assert len(kernels["variants"]) == len(plans["records"])
    out = []
    for r, k in zip(plans["records"], kernels["variants"]):
        if r["route"] == "igemm":
            assert k is not None, r["key"]                               # no record without its kernel
            out.append((dict(r, args=dict(zip(plans["fields"]["igemm"], r["args"]))),
                        dict(zip(("name", "grid", "block", "lds"), [kernels["names"][k[0]]] + k[1:]))))
        else:
            assert k is None
    used = {i for mode in ("tuned", "no_tuned") for order in plans[mode].values() for i in order}
    assert used <= set(range(len(plans["records"]))) and len(out) == 943
    return out


def struct_of(values, nonnull):
    a = _lib.IgemmArgs()
    for k, v in values.items():
        setattr(a, k, v)
    for k in nonnull:
        assert k in POINTERS
        setattr(a, k, 0x1000)                                            # never dereferenced on the host
    return a


def variant(lib, a):
    v = _lib.IgemmVariant()
    rc = lib.aldm_igemm_variant(C.byref(a), C.byref(v))
    return rc, v, lib.aldm_last_error().decode()


def squeeze(s):
    return "".join(s.split())


def test_recorded_launches_select_the_recorded_kernel(lib, recorded):
    families = set()
    for r, k in recorded:
        a = struct_of(r["args"], r["nonnull"])
        rc, v, err = variant(lib, a)
        assert rc == 0, (r["key"], err)
        assert squeeze(v.name.decode()) == squeeze(k["name"]), r["key"]
        assert _lib.IGEMM_FAMILIES[v.family] + "<" in k["name"]
        if k["grid"] is not None:
            assert [v.grid, 1, 1] == k["grid"], (r["key"], k)
        if k["block"] is not None:
            assert [v.block, 1, 1] == k["block"], (r["key"], k)
        if k["lds"] is not None:
            assert v.lds == k["lds"], (r["key"], k)
        assert 0 < v.lds <= 160 * 1024
        assert lib.aldm_igemm_epilogue_form(C.byref(a)) == r["epi"] == v.direct
        assert lib.aldm_igemm_effective_splits(C.byref(a)) == v.splits >= 1
        assert (v.bm, v.bn) == P.TILE_DIMS[v.tile] and (r["args"]["tile"] in (0, v.tile))
        families.add(v.family)
    assert families == set(range(5))                                     # the recorded workloads reach every kernel family


def test_tile_table_is_igemm_plans(lib):
    info = _lib.IgemmTileInfo()
    for tid in range(0, 20):
        rc = lib.aldm_igemm_tile_info(tid, C.byref(info))
        if tid not in P.TILES:
            assert rc == E_UNSUPPORTED and lib.aldm_last_error().decode() == f"igemm: unknown tile {tid}"
            continue
        t = P.TILES[tid]
        assert rc == 0 and info.tile == tid
        assert (info.bm, info.bn, _lib.IGEMM_TILE_KINDS[info.kind]) == (t.bm, t.bn, t.kind)
        assert (info.kind >= 3) == t.halo
        assert (info.halo_rows, info.halo_rows_fused) == (t.halo_rows, t.halo_rows_fused)
        assert tuple(s for s in range(32) if info.rings >> s & 1) == t.rings
        assert info.blocks == (info.bm // info.wm // 16) * (info.bn // info.wn // 16)
        if t.fixed_ring:
            assert info.ring == info.ring_lora == t.fixed_ring
    assert _lib.TILE_128x128 in P.TILES and 5 not in P.TILES             # ALDM_TILE_32x64 stays without a row


# ---- the documented refusals: code and text as the library has always given them ------------------------------------------------------
HALO = "igemm: the halo tiles take no LoRA / V^T / row statistics (and a second-source segment only in the wave-specialised forms)"
WS = "igemm: the wave-specialised tiles take plain launches only (LDS-DMA path, no LoRA / V^T / folded LayerNorm / GEGLU)"
GNIN_TABLES = dict(gnin_groups=16, gnin_tpi1=2)
GNIN_PTRS = ("gnin_gamma", "gnin_beta", "gnin_q1")


def conv3x3(tile, OW=16, OH=16, Cin=64, Cout=128, **kw):
    """a plain 3x3 'same' convolution over two OH x OW images"""
    d = dict(B=2, IH=OH, IW=OW, OH=OH, OW=OW, Cin=Cin, Cout=Cout, KH=3, KW=3, Kpad=9 * Cin, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dil_h=1,
             dil_w=1, alpha=1.0, out_ld=Cout, out_batch_stride=OH * OW * Cout, tile=tile)
    d.update(kw)
    return d


def linear(tile, M=512, K=256, N=256, **kw):
    d = dict(B=1, IH=M, IW=1, OH=M, OW=1, Cin=K, Cout=N, KH=1, KW=1, Kpad=K, stride_h=1, stride_w=1, dil_h=1, dil_w=1, alpha=1.0, out_ld=N,
             out_batch_stride=M * N, tile=tile)
    d.update(kw)
    return d


BASE = ("x", "w", "out")
REFUSALS = [
    ("halo LoRA", conv3x3(7, Rp=32), BASE + ("lora_a", "lora_b"), E_UNSUPPORTED, HALO),
    ("halo-ws LoRA", conv3x3(16, Rp=64), BASE + ("lora_a", "lora_b"), E_UNSUPPORTED, HALO),
    ("halo V^T", conv3x3(8), BASE + ("vt",), E_UNSUPPORTED, HALO),
    ("halo-ws V^T", conv3x3(15), BASE + ("vt",), E_UNSUPPORTED, HALO),
    ("halo rowstats", conv3x3(7), BASE + ("rowstat_out",), E_UNSUPPORTED, HALO),
    ("halo-ws rowstats", conv3x3(15), BASE + ("rowstat_out",), E_UNSUPPORTED, HALO),
    ("x3 on halo 128x128", conv3x3(7, Cin3=64, Kpad=9 * 64 + 64), BASE + ("x3",), E_UNSUPPORTED, HALO),
    ("x3 on halo 64x128", conv3x3(8, Cin3=64, Cin4=64, Kpad=9 * 64 + 128), BASE + ("x3", "x4"), E_UNSUPPORTED, HALO),
    ("ws LoRA", linear(12, Rp=32), BASE + ("lora_a", "lora_b"), E_UNSUPPORTED, WS),
    ("ws small LoRA", linear(13, Rp=64), BASE + ("lora_a", "lora_b"), E_UNSUPPORTED, WS),
    ("ws GEGLU", linear(14, geglu=1), BASE, E_UNSUPPORTED, WS),
    ("ws folded LN", linear(13), BASE + ("ln_s",), E_UNSUPPORTED, WS),
    ("ws V^T", linear(12), BASE + ("vt",), E_UNSUPPORTED, WS),
    ("gnin split", conv3x3(15, Cin=128, splits=2, **GNIN_TABLES), BASE + GNIN_PTRS + ("workspace",), E_UNSUPPORTED, "igemm_halo: gnin_* launches are not split"),
    ("gnin split, halo", conv3x3(8, Cin=128, splits=2, **GNIN_TABLES), BASE + GNIN_PTRS + ("workspace",), E_UNSUPPORTED,
     "igemm_halo: gnin_* launches are not split"),
    ("gnin out_act", conv3x3(7, out_act=_lib.ACT_SILU, **GNIN_TABLES), BASE + GNIN_PTRS, E_UNSUPPORTED, "igemm_halo: gnin_* launches take no output activation"),
    ("gnin post_act", conv3x3(16, post_act=_lib.ACT_SILU, **GNIN_TABLES), BASE + GNIN_PTRS, E_UNSUPPORTED,
     "igemm_halo: gnin_* launches take no output activation"),
    ("gnin off halo", conv3x3(1, **GNIN_TABLES), BASE + GNIN_PTRS, E_ARG, "igemm: gnin_* (GroupNorm of the input inside the launch) needs a halo tile"),
    ("width 64 on halo 64x128", conv3x3(8, OW=64), BASE, E_UNSUPPORTED,
     "igemm_halo: image width 64 / filter 3x3 does not fit the 64x128 halo tile (198 halo rows of 128)"),
    ("width 12 on halo-ws 64x128", conv3x3(16, OW=12), BASE, E_UNSUPPORTED,
     "igemm_halo: image width 12 / filter 3x3 does not fit the 64x128 halo tile (98 halo rows of 128)"),
    ("width 128 on halo 128x128", conv3x3(7, OW=128), BASE, E_UNSUPPORTED,
     "igemm_halo: image width 128 / filter 3x3 does not fit the 128x128 halo tile (390 halo rows of 320)"),
    ("x3, width 4 on halo-ws 128x128", conv3x3(15, OW=4, OH=64, Cin3=64, Kpad=9 * 64 + 64), BASE + ("x3",), E_UNSUPPORTED,
     "igemm_halo: the second-source segment needs a wave-specialised halo tile whose halo fits three DMA passes (OW >= 8 at 128 rows)"),
    ("unknown tile", linear(5), BASE, E_UNSUPPORTED, "igemm: unknown tile 5"),
    ("unknown tile 17", linear(17), BASE, E_UNSUPPORTED, "igemm: unknown tile 17"),
]


@pytest.mark.parametrize("what,values,nonnull,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_keep_code_and_text(lib, what, values, nonnull, code, text):
    rc, _, err = variant(lib, struct_of(values, nonnull))
    assert (rc, err) == (code, text)


def test_widths_that_fit_are_taken(lib):
    """the same shapes at the last width that fits: the refusals above are the capacity edge, not the shape"""
    for values, hp in ((conv3x3(8, OW=16), 2), (conv3x3(7, OW=64), 5), (conv3x3(7, OW=16), 3), (conv3x3(15, OW=8, Cin3=64, Kpad=640), 3)):
        rc, v, err = variant(lib, struct_of(values, BASE + (("x3",) if "Cin3" in values else ())))
        assert rc == 0 and v.hp == hp and v.ext == ("Cin3" in values), err
