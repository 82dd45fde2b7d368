"""GPU parity of the projection GEMM family (aldm_pgemm) against the float64 restatement of tests/pgemm_restatement.py at the row, range,
rank and token-major edges of its dispatch, through ops.linear / ops.conv with PGEMM_CFG forcing the launch shape.  Every case asserts
from the launch label that the pgemm kernel ran with the intended (rows, nt, tiles per range, waves); x, res, the output, the
token-major buffer and lora_t_out are middle slices of NaN arenas whose guards must still be NaN afterwards, the padding columns of the
token-major buffer included.  Forms without a folded LayerNorm are held by the derived per-element bound and by `check`; the folded
forms by `check` (2 x the L2 floor, 4 x the max floor) per output tensor; statistics tables by `check_table` against the sums of the
values as stored.  tests/test_pgemm_restatement_host.py proves on the CPU that these comparators reject every listed mutant at exactly
these cases.  The log carries the largest ratio of every quantity per test (conftest.record)."""
import ctypes as C

import pytest
import torch

import conftest
import pgemm_restatement as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
G = 64                                                       # guard rows (elements, for the flat token-major arena) on either side
CASES = P.all_cases()


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    assert o.PGEMM, "ALDM_NO_PGEMM is set: these tests need the pgemm route"
    return o


class Worst:
    """record(value, what) that keeps the largest value per kind of quantity; flush() hands them to conftest.record"""

    def __init__(self):
        self.top = {}

    def __call__(self, value, what):
        kind = what.rsplit(" ", 1)[-1]
        self.top[kind] = max(self.top.get(kind, 0.0), float(value))
        return value

    def flush(self, what):
        for kind, v in sorted(self.top.items()):
            conftest.record(v, f"{what}: largest {kind}")


def arena(rows, cols, dtype=torch.bfloat16):
    """-> (whole [rows + 2 G, cols] of NaN, its middle rows)"""
    whole = torch.full((rows + 2 * G, cols), float("nan"), dtype=dtype, device=DEV)
    return whole, whole[G:G + rows]


def guards_intact(whole, rows, what):
    assert bool(torch.isnan(whole[:G]).all()) and bool(torch.isnan(whole[G + rows:]).all()), f"{what}: a guard row was written"


def put(t, dtype=torch.bfloat16):
    """a middle slice of a NaN arena holding t [rows, cols]"""
    whole, mid = arena(t.shape[0], t.shape[1], dtype)
    mid.copy_(t.to(dtype))
    return mid


def pack(ops, c, d):
    W, bias = d["W"].float().to(DEV), d["bias"].to(DEV)
    if c["nparts"]:
        pw = ops.pack_linear_ln(W, bias, d["gamma"].float().to(DEV), d["beta"].float().to(DEV), eps=c["eps"], geglu=c["geglu"])
    else:
        pw = ops.pack_geglu(W, bias) if c["geglu"] else ops.pack_linear(W, bias)
    if d["parts"]:
        ops.attach_lora(pw, [(p[0], p[1], p[2].to(DEV), p[3].to(DEV)) + tuple(p[4:]) for p in d["parts"]], d["layout"])
        assert (pw.Rp, pw.ranks_used) == (d["Rp"], d["used"])
    return pw


def run(ops, c, record):
    """one launch of case c through ops.conv, judged; -> the label"""
    d = P.inputs(c)
    ref = P.reference(c, d)
    what = f"{c['group']} {c['name']}"
    M, K, N, v = c["M"], c["K"], c["N"], c["vt"]
    pw = pack(ops, c, d)
    x = put(d["x"])
    res = put(d["res"]) if c["res"] else None
    kw, got, held = {}, {}, []
    ncols = N // 2 if c["geglu"] else (v["col0"] if (v and not v.get("dual")) else N)
    Bc, OHW = (v["B"], M // v["B"]) if v else (1, M)
    out_whole = None
    if ncols:
        out_whole, out = arena(M, ncols)
        kw["out"] = out.view(Bc, 1, OHW, ncols)
        held.append((out_whole, M, "out"))
    if v:
        _, _, col0, Cc, ld, bs, off, vec = P.vt_geom(c)
        flat = torch.full((2 * G + off + Bc * bs,), float("nan"), dtype=torch.bfloat16, device=DEV)
        vt = flat[G + off:G + off + Bc * bs].view(Bc, Cc, ld)
        assert vec == P.vt_vec(OHW, ld, bs, (vt.data_ptr() % 16) // 2), "the store path this case is there for"
        kw.update(vt=vt, vt_col0=col0, vt_ld=ld, vt_batch_stride=bs, vt_dual=bool(v.get("dual")))
    if c["t_out"]:
        t_whole, T = arena(M, d["Rp"])
        kw["lora_t_out"] = T
        held.append((t_whole, M, "lora_t_out"))
    if c["t_out"] or (v and v.get("dual")):
        kw["splits"] = 1
    if c["gate_rows"]:
        kw["lora_gate"] = d["gate"].to(DEV).contiguous()
    if c["nparts"]:
        kw["ln_parts"] = d["lp"].to(DEV).contiguous()
    if c["stats"]:
        kw["rowstats"] = True
    key = ops._pgemm_key(M, pw, K, res, kw.get("vt"), c["stats"], c["t_out"], bool(v and v.get("dual")))
    had = ops.PGEMM_CFG.get(key)
    ops.PGEMM_CFG[key] = c["cfg"]                            # forced for this launch only; whatever the tuned table held comes back
    before, ops.PROFILE = ops.PROFILE, []
    try:
        y = ops.conv(x.view(Bc, 1, OHW, K), pw, res=(res.view(Bc, 1, OHW, N) if res is not None else None), **kw)
        torch.cuda.synchronize()
        labels = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = before
        ops.PGEMM_CFG.pop(key, None)
        if had is not None:
            ops.PGEMM_CFG[key] = had
    assert len(labels) == 1 and labels[0].startswith("pgemm_"), labels
    tail = f"|M{M} N{N} K{K}" + (" geglu" if c["geglu"] else "")
    if c["expect_cfg"]:
        assert labels[0] == P.label_of(c["cfg"], d["Rp"], v is not None, bool(v and v.get("dual"))) + tail, (what, labels[0])
    else:                                                    # more than 16 statistics ranges: the entry is set aside, the planner's shape runs
        a = c["cfg"]
        planned = P.plan(M, N, K, Rp=d["Rp"], ranks_used=d["used"], res=c["res"], max_ranges=16)
        assert planned != a and labels[0] == P.label_of(planned, d["Rp"]) + tail, (what, labels[0], planned)
    if c["stats"]:
        y, st = y
        assert st.shape[0] == M and st.shape[1] <= 16 and st.shape[2] == 2
        if c["expect_cfg"]:
            assert st.shape[1] == N // P.stats_width(c)
        got["stats"] = st
    if ncols:
        got["y"] = out_whole[G:G + M]
    if v:
        got["vt"] = vt
        assert bool(torch.isnan(flat[:G + off]).all()) and bool(torch.isnan(flat[G + off + Bc * bs:]).all()), f"{what}: a guard of the token-major buffer was written"
    if c["t_out"]:
        got["T"] = T
    for whole, rows, name in held:
        guards_intact(whole, rows, f"{what} {name}")
    P.check_case(c, got, ref, record)
    return labels[0]


def run_all(ops, cases, what):
    assert cases
    rec = Worst()
    try:
        for c in cases:
            run(ops, c, rec)
    finally:
        rec.flush(what)


def group(g, pred=lambda c: True):
    return [c for c in CASES if c["group"] == g and pred(c)]


# ---------------------------------------------------------------------------------------------------------------------------------
# A, rows: M = 1 .. 193 under 64- and 128-row blocks (grids of 1 .. 7 workgroups and beyond 8 with a remainder in the XCD remap)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", P.A_KS)
@pytest.mark.parametrize("mi,nw", P.A_SHAPES)
def test_a_rows(ops, K, mi, nw):
    run_all(ops, group("A", lambda c: c["K"] == K and c["cfg"][0] == mi and c["cfg"][3] == nw and " ranges M" not in c["name"]), f"A K{K} mi{mi} w{nw}")


def test_a_rows_three_and_seven_ranges(ops):
    run_all(ops, group("A", lambda c: " ranges M" in c["name"]), "A 3 / 7 ranges")


# ---------------------------------------------------------------------------------------------------------------------------------
# B, ranges: the ring unfilled, filled and wrapped; column-coded vectors; more than 16 statistics ranges
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", P.B_KS)
def test_b_ranges(ops, K):
    cases = group("B", lambda c: c["K"] == K)
    assert {c["cfg"][2] for c in cases} >= ({1, 2, 3, 4, 6, 8, 16} if K < 640 else {1, 2, 3, 4, 6}), "tiles per range"
    assert any(not c["expect_cfg"] for c in cases)
    run_all(ops, cases, f"B K{K}")


# ---------------------------------------------------------------------------------------------------------------------------------
# C, ranks: ranks_used on either side of the RT 1 -> 2 switch, parts, a block in the second rank tile, gates
# ---------------------------------------------------------------------------------------------------------------------------------
def test_c_ranks(ops):
    cases = group("C", lambda c: not c["gate_rows"] and not c["Rp"])
    assert {sum(c["ranks"]) for c in cases} >= set(P.C_RANKS) and any(c["layout_col0"] == 16 for c in cases)
    run_all(ops, cases, "C ranks")


@pytest.mark.parametrize("gate_rows", P.GATE_ROWS)
def test_c_gates(ops, gate_rows):
    run_all(ops, group("C", lambda c: c["gate_rows"] == gate_rows), f"C gate rows {gate_rows}")


def test_c_k640_refuses_two_row_tiles_with_an_adapter(ops):
    from audioldm_with_lora_amd import _lib
    c = dict(next(c for c in CASES if c["name"] == "K640 mi1"), cfg=(2, 32, 2, 4))
    with pytest.raises(_lib.AldmError):
        run(ops, c, Worst())


def test_c_rp64_direct_with_every_output_in_an_arena(ops):
    """aldm_pgemm through _lib.PgemmArgs: a 64-wide T with 20 ranks in use (ops never sends it), residual, statistics table and
    lora_t_out -- the only launch here whose statistics table is a slice of an arena too (ops allocates the table itself)"""
    from audioldm_with_lora_amd import _lib
    lib = _lib.load()
    c = next(c for c in CASES if c["name"] == "Rp64 ranks 20")
    c = dict(c, stats=True)
    d = P.inputs(c)
    ref = P.reference(c, d)
    M, K, N = c["M"], c["K"], c["N"]
    pk = P.pack_lora(d["parts"], N, K, Rp=64)
    assert pk["Rp"] == 64 and pk["used"] == 20
    w, bias = d["W"].to(torch.bfloat16).to(DEV).contiguous(), d["bias"].to(DEV)
    la, lb = pk["A"].to(torch.bfloat16).to(DEV).contiguous(), pk["sB"].to(torch.bfloat16).to(DEV).contiguous()
    x, res = put(d["x"]), put(d["res"])
    out_w, out = arena(M, N)
    t_w, T = arena(M, 64)
    nr = N // P.stats_width(c)
    st_w, st = arena(M, nr * 2, torch.float32)
    a = _lib.PgemmArgs()
    a.x, a.w, a.M, a.N, a.K, a.bias = x.data_ptr(), w.data_ptr(), M, N, K, bias.data_ptr()
    a.lora_a, a.lora_b, a.Rp, a.ranks_used = la.data_ptr(), lb.data_ptr(), 64, 20
    a.res, a.out, a.out_ld, a.rowstat_out, a.lora_t_out = res.data_ptr(), out.data_ptr(), N, st.data_ptr(), T.data_ptr()
    a.mi, a.nt, a.tiles_per_range, a.waves = c["cfg"]
    rc = lib.aldm_pgemm(C.byref(a), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.aldm_last_error()
    for whole, name in ((out_w, "out"), (t_w, "lora_t_out"), (st_w, "rowstat_out")):
        guards_intact(whole, M, f"Rp64 {name}")
    rec = Worst()
    P.check_case(c, dict(y=out, T=T, stats=st.view(M, nr, 2)), ref, rec)
    rec.flush("C Rp64 direct")


# ---------------------------------------------------------------------------------------------------------------------------------
# D, token-major stores: samples shorter than a lane's row group, the three store paths by their natural route and demoted, a range that
# straddles vt_col0, dual stores, the folded LayerNorm on ladder rows with 1 .. 16 partial pairs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (2, 3))
def test_d_tokens_per_sample(ops, B):
    cases = group("D", lambda c: c["name"].startswith("tok") and "pad" not in c["name"] and c["vt"]["B"] == B)
    assert {c["M"] // B for c in cases} == set(P.D_TOKENS)
    run_all(ops, cases, f"D tokens B{B}")


def test_d_demoted_store_paths(ops):
    run_all(ops, group("D", lambda c: "pad" in c["name"]), "D demoted")


def test_d_folded_layernorm_partial_counts(ops):
    run_all(ops, group("D", lambda c: c["name"].startswith("nparts")), "D nparts")


def test_d_straddling_range_and_dual_stores(ops):
    run_all(ops, group("D", lambda c: "straddles" in c["name"] or "dual" in c["name"]), "D straddle / dual")


def test_d_seventeen_partial_pairs_leave_pgemm(ops):
    """ln_parts with 17 pairs per row: more than the kernel's four lanes x four slots -- the launch must go to the convolution kernel"""
    c = dict(next(c for c in CASES if c["name"] == "nparts 16"), nparts=17)
    d = P.inputs(c)
    ref = P.reference(c, d)
    pw = pack(ops, c, d)
    M, K = c["M"], c["K"]
    Bc, OHW, col0, Cc, ld, bs, off, _ = P.vt_geom(c)
    vt = torch.full((Bc, Cc, ld), float("nan"), dtype=torch.bfloat16, device=DEV)
    before, ops.PROFILE = ops.PROFILE, []
    try:
        y = ops.conv(put(d["x"]).view(Bc, 1, OHW, K), pw, vt=vt, vt_col0=col0, vt_ld=ld, vt_batch_stride=bs, ln_parts=d["lp"].to(DEV))
        torch.cuda.synchronize()
        labels = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = before
    assert labels and not any(l.startswith("pgemm_") for l in labels) and labels[-1].startswith("igemm"), labels
    rec = Worst()
    P.check_case(c, dict(y=y.view(M, col0), vt=vt), ref, rec)
    rec.flush("D 17 pairs on igemm")


# ---------------------------------------------------------------------------------------------------------------------------------
# E, GEGLU: plain and LayerNorm-folded (1 and 16 partial pairs), every launch shape x ring depth, edge gates on both ends of a block
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", P.E_KS)
@pytest.mark.parametrize("M", P.E_MS)
def test_e_geglu(ops, K, M):
    cases = group("E", lambda c: c["K"] == K and c["M"] == M)
    assert {c["nparts"] for c in cases} == {0, 1, 16} and {(c["cfg"][0], c["cfg"][3]) for c in cases} == {(1, 4), (2, 4), (1, 8)}
    run_all(ops, cases, f"E K{K} M{M}")
