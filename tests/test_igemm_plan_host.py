"""The launch planner (audioldm_with_lora_amd/igemm_plan.py) on the CPU: every launch recorded on the MI355X
(tests/golden/igemm_launch_plans.json.gz, written by tools/record_launch_plans.py) is planned again from its recorded inputs and must come
out as recorded; then the tile table, the halo rule and the tuning key on their own."""
import gzip
import json
import math
import os
import re
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from audioldm_with_lora_amd import _lib, igemm_plan as P, ops  # noqa: E402

PKG = os.path.join(ROOT, "audioldm_with_lora_amd")
FIXTURE = os.path.join(ROOT, "tests", "golden", "igemm_launch_plans.json.gz")


def _table(name, section):
    with open(os.path.join(PKG, name)) as f:
        return json.load(f)[section]


TUNED = {k: tuple(v) for k, v in _table("tuned_gfx950.json", "igemm").items()}
PGEMM_CFG = {(int(m), int(n), int(k), kind): tuple(v) for (m, n, k, kind), v in
             ((key.split("|"), v) for key, v in _table("pgemm_gfx950.json", "pgemm").items())}


@pytest.fixture(scope="module")
def fixture():
    import record_launch_plans as R
    with gzip.open(FIXTURE) as f:
        assert os.path.getsize(FIXTURE) < len(f.read()) < 1_000_000        # (gzipped JSON: under the fixtures' limit unpacked as well)
    return R.load_fixture(FIXTURE)


def geom_of(i):
    """the Geom of a recorded conv() call (`in` of a fixture record)"""
    shape = lambda k: i[k]["shape"] if k in i else None
    C = lambda k: shape(k)[3] if k in i else 0
    res = i.get("res")
    d = i.get("defer", False)
    return P.geometry(
        tuple(i["x"]), SimpleNamespace(**i["pw"]), C2=C("x2"), C3=C("x3"), C4=C("x4"), x2="x2" in i, x3="x3" in i,
        stride=i.get("stride", (1, 1)), pad=i.get("pad", (0, 0)), dil=i.get("dil", (1, 1)), up_size=i.get("up_size"),
        in_dilate=i.get("in_dilate", 0), out_hw=i.get("out_hw"), in_act=i.get("in_act", 0), vt="vt" in i, vt_dual=bool(i.get("vt_dual", False)),
        vt_col0=i.get("vt_col0", 0), rowbias="rowbias" in i, res=res is not None,
        res_numel=(math.prod(res["shape"]) if res is not None and res["contig"] else None), res2="res2" in i, out2="out2" in i,
        out_act=i.get("out_act", 0), post_act=i.get("post_act", 0), alpha=i.get("alpha", 1.0), lora_t_out="lora_t_out" in i,
        ln_parts=shape("ln_parts")[1] if "ln_parts" in i else None, rowstats=bool(i.get("rowstats", False)), qstats=i.get("qstats", False),
        gn_groups=i.get("gn_groups"), defer=tuple(d) if isinstance(d, list) else d, gn_in=i.get("gn_in", False), tile=i.get("tile", 0),
        ring=i.get("ring", 0), splits=i.get("splits"), out_f32=i.get("out_f32", False),
        out_dtype=(_lib.OUT_F32 if i["out"]["f32"] else _lib.OUT_BF16) if "out" in i else None, out_ld=i.get("out_ld"),
        out_batch_stride=i.get("out_batch_stride"), out_pix_stride=i.get("out_pix_stride", 1), out_pix_offset=i.get("out_pix_offset", 0))


@pytest.mark.parametrize("mode", ["tuned", "no_tuned"])
def test_every_recorded_launch_plans_as_recorded(fixture, mode):
    tuned, pgemm_cfg = (TUNED, PGEMM_CFG) if mode == "tuned" else ({}, {})
    records = fixture[mode]["records"]
    assert len(records) > 300 and {r["route"] for r in records} == {"igemm", "pgemm"}
    for r in records:
        g = geom_of(r["in"])
        p = P.plan(g, tuned, None, pgemm_cfg)
        assert p.route == r["route"], r
        if p.route == "pgemm":
            continue
        a = r["args"]
        assert (p.key, p.tile, p.ring, p.splits) == (r["key"], a["tile"], a["ring"], a["splits"]), (r, p)
        assert (g.M, g.OH, g.OW, g.out_ld, g.out_batch_stride, g.out_dtype) == (
            a["B"] * a["OH"] * a["OW"], a["OH"], a["OW"], a["out_ld"], a["out_batch_stride"], a["out_dtype"]), (r, g)
        if r["key"] is not None:
            assert p.gn_defer == (" gn" in r["key"]), (r, p)                  # the key says whether the launch may defer its reduce
        assert p.gn_defer or not a["defer_reduce"], (r, p)
        assert (p.qstats is not None) == ("qstat_out" in r["nonnull"]) and (p.rowstats_cols is not None) == ("rowstat_out" in r["nonnull"]), (r, p)
        # the tables' shapes, where the call's result showed them (a gn= call returns the norm, not the tensor that carries the table)
        assert r["qstats"] is None or p.qstats == tuple(r["qstats"]), (r, p)
        assert p.rowstats_cols == r["rowstats_cols"], (r, p)


def test_fixture_keys_round_trip(fixture):
    keys = set(TUNED) | {r["key"] for m in fixture.values() for r in m["records"] if r["route"] == "igemm" and r["key"] is not None}
    assert len(keys) > len(TUNED)
    for k in keys:
        g, sp = P.parse_key(k)
        assert P.launch_key(g, sp) == k
    assert P.parse_key("pg:1000|256|256|l32") is None
    for m in fixture.values():                                               # and the parsed key admits what the real geometry admits
        for r in m["records"]:
            if r["route"] == "igemm" and r["key"] is not None:
                assert P.halo_candidates(P.parse_key(r["key"])[0]) == P.halo_candidates(geom_of(r["in"])), r


def test_tuned_halo_entries_are_admitted():
    halo = {k: v for k, v in TUNED.items() if v[0] in P.HALO_ROWS}
    assert len(halo) > 50
    for k, (tile, ring, splits) in halo.items():
        assert tile in P.halo_candidates(P.parse_key(k)[0]), (k, tile)


# ---- the rule, against the expression ops.conv() held before there was one ----------------------------------------------------------
OLD_DIMS = {1: (128, 128), 2: (64, 64), 3: (128, 64), 4: (64, 128), 6: (128, 128), 7: (128, 128), 8: (64, 128), 9: (256, 128), 10: (64, 128),
            11: (128, 64), 12: (256, 128), 13: (64, 128), 14: (128, 64), 15: (128, 128), 16: (64, 128)}
OLD_NAMES = {1: "128x128", 2: "64x64", 3: "128x64", 4: "64x128", 6: "128x128w8", 7: "halo128x128", 8: "halo64x128", 9: "256x128w8",
             10: "64x128w8", 11: "128x64w8", 12: "256x128ws", 13: "64x128ws", 14: "128x64ws", 15: "halo128x128ws", 16: "halo64x128ws"}
OLD_HALO_ROWS = {7: 320, 8: 128, 15: 320, 16: 128}


def old_halo(g):
    """ops.halo_tiles() and conv()'s inline amendments, as they stood (without the two defects' fixes)"""
    plain = g.fast_path and not g.in_dilate and not g.Rp and not g.vt and not g.geglu and not g.ln
    halo = []
    if g.KH == 3 and g.KW == 3 and g.stride == (1, 1) and g.pad == (1, 1) and g.dil == (1, 1) and plain:
        halo = [t for t in (7, 8, 15, 16) if OLD_DIMS[t][0] % g.OW == 0 and (OLD_DIMS[t][0] // g.OW + 2) * (g.OW + 2) <= OLD_HALO_ROWS[t]]
    if (g.KH == 1 and g.IH == 1 and g.KW % 2 == 1 and g.KW > 1 and g.stride == (1, 1) and g.pad == (0, (g.KW - 1) * g.dil[1] // 2)
            and g.dil[0] == 1 and plain and g.up_size is None and not g.x3 and not g.gn_in):
        halo = [t for t in (15, 16) if OLD_DIMS[t][0] + (g.KW - 1) * g.dil[1] <= OLD_HALO_ROWS[t]]
    if g.x3:
        halo = [t for t in halo if t in (15, 16) and g.up_size is None and g.C3 % 64 == 0 and g.C4 % 64 == 0
                and (OLD_DIMS[t][0] // g.OW + 2) * (g.OW + 2) <= (192 if t == 15 else 128)]
    return halo


def pack(N, Cin, KH, KW, Cext=0):
    return SimpleNamespace(N=N, Kpad=-(-(KH * KW * Cin + Cext) // 64) * 64, Cin=Cin, KH=KH, KW=KW, Cext=Cext, Rp=0, geglu=False, ln=False)


def test_halo_rule_equals_the_old_expression_3x3():
    n = 0
    for OW in (4, 5, 8, 16, 32, 64, 128):
        for up in (False, True):
            for x3 in (False, True):
                for C3 in (0, 64, 96, 128):
                    for C4 in (0, 64, 96, 128):
                        if x3 and C3 == 0:
                            continue
                        if not x3 and (C3 or C4):
                            continue
                        I = OW // 2 if up else OW
                        g = P.geometry((2, I, I, 128), pack(128, 128, 3, 3, C3 + C4), C3=C3, C4=C4, x3=x3, pad=(1, 1),
                                       up_size=(OW, OW) if up else None)
                        assert g.OW == OW and P.halo_candidates(g) == old_halo(g), g
                        assert ops.halo_tiles(OW, True) == old_halo(P.geometry((2, OW, OW, 128), pack(128, 128, 3, 3), pad=(1, 1)))
                        n += 1
    assert n == 7 * 2 * (1 + 3 * 4)
    assert ops.halo_tiles(16, False) == []


def test_halo_rule_equals_the_old_expression_conv1d():
    seen = set()
    for KW in (3, 5, 7, 11):
        for dil in (1, 3, 5, 9, 27):
            for T in (64, 2048, 8192):
                g = P.geometry((2, 1, T, 128), pack(128, 128, 1, KW), pad=(0, (KW - 1) * dil // 2), dil=(1, dil))
                assert g.OW == T and P.halo_candidates(g) == old_halo(g), g
                seen.add(tuple(P.halo_candidates(g)))
    assert seen == {(), (15,), (15, 16)}                                     # the grid reaches both capacities


def test_transposed_conv_phase_is_no_halo_launch():
    """A conv_transpose1d phase walks its taps backwards: negative dilation with negative padding.  With an odd tap count the old
    expression read it as a conv1d halo launch (wrong numbers); the rule wants dil >= 1 and pad >= 0."""
    g = P.geometry((2, 1, 2048, 128), pack(128, 128, 1, 3), pad=(0, -1), dil=(1, -1), out_hw=(1, 2048))
    assert old_halo(g) == [15, 16] and P.halo_candidates(g) == []
    p = P.plan(g, {})
    assert not P.TILES[p.tile].halo and p.route == "igemm"


def test_conv1d_halo_launch_gets_no_qstats_table():
    """qstats=True on a conv1d halo launch with T > BM used to divide by BM // OW == 0"""
    g = P.geometry((1, 1, 4096, 128), pack(128, 128, 1, 3), pad=(0, 1), qstats=True)
    assert g.qstats and P.halo_candidates(g) == [15, 16]
    for tuned in ({P.launch_key(g): (15, 3, 1)}, {P.launch_key(g): (16, 3, 1)}):
        p = P.plan(g, tuned)
        assert P.TILES[p.tile].halo and p.qstats is None and p.splits == 1
    p = P.plan(g, {})                                                        # (the heuristics take a generic tile: that one has a table)
    assert not P.TILES[p.tile].halo and p.qstats == (math.ceil(4096 / P.TILES[p.tile].bm), P.TILES[p.tile].bm, 0)


def test_gn_in_form():
    g = P.geometry((8, 250, 16, 128), pack(128, 256, 3, 3), C2=128, pad=(1, 1), gn_in=True)
    assert P.halo_candidates(g) == [15, 16]
    p = P.plan(g, {})
    assert (p.tile, p.splits, p.key.endswith(" gi")) == (15, 1, True)
    assert P.halo_candidates(P.geometry((8, 250, 16, 96), pack(128, 96, 3, 3), pad=(1, 1), gn_in=True)) == []       # C1 % 64
    assert P.halo_candidates(P.geometry((8, 250, 16, 640), pack(128, 640, 3, 3), pad=(1, 1), gn_in=True)) == []     # > 512 channels
    assert P.halo_candidates(P.geometry((8, 125, 8, 128), pack(128, 128, 3, 3), pad=(1, 1), up_size=(250, 16), gn_in=True)) == []


# ---- the tile table -------------------------------------------------------------------------------------------------------------------
def test_tile_table_matches_the_header():
    with open(os.path.join(ROOT, "include", "aldm_hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(ALDM_TILE_\w+)\s*=\s*(\d+)", src))
    assert len(enum) == 17 and enum["ALDM_TILE_AUTO"] == 0
    assert {t.c_name: t.id for t in P.TILES.values()} == {n: v for n, v in enum.items() if n not in ("ALDM_TILE_AUTO", "ALDM_TILE_32x64")}
    for name, v in enum.items():
        if name != "ALDM_TILE_32x64":                                        # (declared, never planned: no Python constant)
            assert getattr(_lib, name[5:]) == v, name
    assert sorted(n for n in dir(_lib) if n.startswith("TILE_")) == sorted(n[5:] for n in enum if n != "ALDM_TILE_32x64")


def test_derived_views_equal_the_old_literals():
    assert ops.TILE_DIMS == OLD_DIMS and ops.TILE_NAMES == OLD_NAMES and ops.HALO_ROWS == OLD_HALO_ROWS
    assert {t.id: t.halo_rows_fused for t in P.TILES.values() if t.halo_rows_fused} == {15: 192, 16: 128}
    assert {t.id: t.fixed_ring for t in P.TILES.values() if t.fixed_ring} == {6: 2, 9: 2, 12: 3}
    assert {t.id: t.rings for t in P.TILES.values() if t.rings != (2, 3, 4)} == {6: (2, 3), 9: (2, 3), 12: (3,), 13: (3, 4), 14: (3, 4)}
    for t in P.TILES.values():
        assert t.halo == (t.id in OLD_HALO_ROWS) and (t.kind, t.name.startswith("halo")) in (
            ("w4", False), ("w8", False), ("ws", False), ("halo", True), ("halo-ws", True))
