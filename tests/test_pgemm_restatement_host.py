"""CPU proof that tests/test_gpu_pgemm_edges.py can fail: the float64 restatement of the projection GEMM family equals torch's float64
compositions, its packs equal ops' bit for bit, its own rounded form passes its comparators at every case of the GPU file, and every
listed mutant is rejected at every case where its output differs from the unmutated form (last section).  Recorded, not
asserted: how many of tests/test_gpu_pgemm.py's own shapes and draws accept each mutant under that file's `close`."""
import ctypes as C
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import conftest
import pgemm_restatement as P
from norm_restatement import ln_linear, ln_linear_draw

F64 = torch.float64
CASES = P.all_cases()
GROUPS = "ABCDE"


def by_group(g):
    return [c for c in CASES if c["group"] == g]


# ---------------------------------------------------------------------------------------------------------------------------------
# exact = torch float64
# ---------------------------------------------------------------------------------------------------------------------------------
def close9(a, b):
    return float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max()))


def peft(xn, parts, gate, gate_rows, cols):
    """peft lora.Linear per part, the per-sample gate written as a loop over samples"""
    out = {}
    for (row0, nrows, A, Bm, s, *_), col in zip(parts, cols):
        lo = s * F.linear(F.linear(xn, A.to(F64)), Bm.to(F64))
        if gate is not None:
            r = A.shape[0]
            lo = torch.zeros_like(lo)
            for smp in range(gate.shape[0]):
                rows = slice(smp * gate_rows, (smp + 1) * gate_rows)
                lo[rows] = s * F.linear(F.linear(xn[rows], A.to(F64)) * gate[smp, col:col + r].to(F64), Bm.to(F64))
        out[(row0, nrows)] = lo
    return out


@pytest.mark.parametrize("name", ["A res+lora+stats M65 K256 mi1w4", "C gate rows 7 res1", "C gate rows 40 vt ln", "C parts (16, 8, 8) vt ln",
                                  "C adapter at 16..19", "D nparts 5", "E geglu M65 K256 mi1w4 T2 np0", "E geglu M65 K384 mi1w4 T2 np1"])
def test_exact_is_the_torch_float64_composition(name):
    c = next(c for c in CASES if f"{c['group']} {c['name']}" == name)
    d = P.inputs(c)
    f = P.forward(d["x"], d["W"], d["bias"].to(F64), d["parts"], res=d["res"], gate=d["gate"], gate_rows=c["gate_rows"],
                  ln=(d["gamma"], d["beta"], c["eps"]) if c["nparts"] else None, lp=d["lp"], geglu=c["geglu"], layout=d["layout"], forms=("exact",))
    xn = F.layer_norm(d["x"], (c["K"],), d["gamma"], d["beta"], c["eps"]) if c["nparts"] else d["x"]
    want = F.linear(xn, d["W"], d["bias"].to(F64))
    cols = P.part_columns(d["parts"], d["layout"])[0] if d["parts"] else []
    for (row0, nrows), lo in peft(xn, d["parts"], d["gate"], c["gate_rows"], cols).items():
        want[:, row0:row0 + nrows] += lo
    if d["res"] is not None:
        want = want + d["res"]
    if c["geglu"]:
        I = c["N"] // 2
        want = want[:, :I] * F.gelu(want[:, I:])
        assert close9(P.geglu_fwd(F.linear(xn, d["W"], d["bias"].to(F64))), want)
    assert close9(f["exact"], want)


def test_token_major_store_is_the_permutation():
    y = torch.arange(2 * 9 * 6, dtype=F64).view(18, 6)
    vt = P.vt_store(y, 2, 9, 2, 16)
    assert torch.equal(vt[:, :, :9], y[:, 2:].view(2, 9, 4).permute(0, 2, 1)) and bool(torch.isnan(vt[:, :, 9:]).all())
    for b, ch, pix in itertools.product(range(2), range(4), range(9)):
        assert vt[b, ch, pix] == y[b * 9 + pix, 2 + ch]


def test_folded_form_is_ln_linear_where_they_overlap():
    """norm_restatement.ln_linear and forward(ln=) agree: exact to 1e-9, rounded (on the one-pass statistics) and the shared mutants bit for bit"""
    for M, K, N, r, nparts in [(70, 256, 192, 4, 4), (33, 384, 192, 8, 2), (17, 640, 192, 0, 16)]:
        x, W, bias, gm, bt, parts = ln_linear_draw(M, K, N, r)
        f = P.forward(x, W, bias, parts, ln=(gm, bt, 1e-5), lp=P.ln_partials(x, nparts))
        assert close9(f["exact"], ln_linear(x, W, bias, gm, bt, 1e-5, parts))             # (the same operation, another order of sums)
        assert torch.equal(f["rounded"], ln_linear(x, W, bias, gm, bt, 1e-5, parts, rounded=True, design="onepass_f32", nparts=nparts))
        for m in ("t_round_first", "s_unrounded", "neighbour", "n_pad", "unbiased", "eps_out", "eps_drop"):
            fm = P.forward(x, W, bias, parts, ln=(gm, bt, 1e-5), lp=P.ln_partials(x, nparts), mutant=m, forms=("rounded",))
            kw = {} if m in P.STAT_MUTANTS else dict(design="onepass_f32", nparts=nparts)
            assert torch.equal(fm["rounded"], ln_linear(x, W, bias, gm, bt, 1e-5, parts, rounded=True, mutant=m, **kw)), m


# ---------------------------------------------------------------------------------------------------------------------------------
# the packs, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def test_packs_equal_ops_on_cpu_tensors():
    from audioldm_with_lora_amd import ops
    g = torch.Generator().manual_seed(3)
    K, N = 256, 192
    W = (torch.randn(N, K, generator=g) / 16).to(torch.bfloat16).float()
    bias, gm, bt = torch.randn(N, generator=g), 1 + 0.3 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)
    parts = P.balanced_parts(N, K, (4, 8, 4), g)
    for ln in (False, True):
        for layout in (None, {"a": (16, 16)}):
            pp = [p + ("a",) for p in parts] if layout else parts
            pw = ops.pack_linear_ln(W, bias, gm, bt) if ln else ops.pack_linear(W, bias)
            ops.attach_lora(pw, pp, layout)
            mine = P.pack_lora(pp, N, K, (gm.to(F64), bt.to(F64)) if ln else None, layout)
            assert pw.Rp == mine["Rp"] and pw.ranks_used == mine["used"]
            assert torch.equal(pw.lora_a.to(F64), mine["A"]) and torch.equal(pw.lora_b.to(F64), mine["sB"])
            if ln:
                Wp, s, c = P.pack_ln(W.to(F64), bias.to(F64), gm.to(F64), bt.to(F64))
                assert torch.equal(pw.w.to(F64), Wp)
                f32sum = lambda a, b: torch.allclose(a.to(F64), b, rtol=0.0, atol=K * 2.0 ** -24 * 8.0)   # fp32 sums of K terms below 8 each
                assert f32sum(pw.ln_s, s) and f32sum(pw.bias, c)                    # (the bf16 tensors bit for bit, the fp32 vectors to
                assert f32sum(pw.ln_sa, mine["sA"]) and f32sum(pw.ln_ca, mine["cA"])  #  the rounding of their fp32 summation)
    pg = ops.pack_geglu(W, bias)
    order = P.geglu_pack_order(N // 2)
    assert torch.equal(pg.w.float(), W[order]) and torch.equal(pg.bias, bias[order])
    pgl = ops.pack_linear_ln(W, bias, gm, bt, geglu=True)
    Wp, s, _ = P.pack_ln(W.to(F64), bias.to(F64), gm.to(F64), bt.to(F64))
    assert torch.equal(pgl.w.to(F64), Wp[order]) and torch.allclose(pgl.ln_s.to(F64), s[order], rtol=0.0, atol=K * 2.0 ** -21)
    with pytest.raises(Exception):
        ops.attach_lora(ops.pack_linear(W, bias), [p + ("a",) for p in parts], {"a": (0, 8)})   # 16 ranks overflow an 8-wide block


# ---------------------------------------------------------------------------------------------------------------------------------
# the draws hold what they claim
# ---------------------------------------------------------------------------------------------------------------------------------
def test_draws_hold_their_claims():
    d = P.draw(200, 256, 192, (4, 8, 4), res=True)
    base = d["x"] @ d["W"].t()
    pk = P.pack_lora(d["parts"], 192, 256)
    lora = (d["x"] @ pk["A"].t()) @ pk["sB"].t()
    assert 0.5 < float(lora.std() / base.std()) < 2.0, "balanced: the LoRA term is as large as the base term"
    assert len({(p[2].shape[0], p[4]) for p in d["parts"]}) == 3, "every part its own (rank, scaling)"
    code = P.column_code(1920, P._gen(1)).to(F64)
    for shift in (1, 8, 16, 32, 64, 128, 512):
        assert float((code - torch.roll(code, shift)).abs().min()) >= 3.0 / 64.0, shift
    x, _, _ = P.ln_draw(130, 256)
    ratio = (x.mean(1).abs() / x.std(1, unbiased=False))
    assert float(ratio.max()) > 14.0 and float(ratio.min()) < 0.5, "ladder: |mean| / std from 0 up to the contract ceiling"
    for gr in P.GATE_ROWS:
        gt = P.gate_draw(200 if gr in (40, 100) else (192 if gr == 64 else 70), gr, 32, 16)
        assert all(not torch.equal(gt[-1], gt[i]) for i in range(gt.shape[0] - 1)), "the last sample is distinct"
        assert all(not torch.equal(gt[i], gt[i + 1]) for i in range(gt.shape[0] - 1)), "neighbouring samples differ"
        assert set(gt[:-1, :16].flatten().tolist()) <= set(P.GATE_VALUES)
    assert any(gr % 4 for gr in P.GATE_ROWS) and any(gr % 16 for gr in P.GATE_ROWS) and any(gr % 64 for gr in P.GATE_ROWS)
    c = next(c for c in CASES if c["geglu"] and not c["nparts"])
    d = P.inputs(c)
    h = d["x"] @ d["W"].t() + d["bias"].to(F64)
    I = c["N"] // 2
    for col, v in zip(d["edge_cols"], P.GEGLU_EDGE_GATES):
        assert bool((h[:, I + col] == v).all()) and col % 16 in (0, 15)


# ---------------------------------------------------------------------------------------------------------------------------------
# rounded passes, mutants fail -- at every case of the GPU file
# ---------------------------------------------------------------------------------------------------------------------------------
WEAKEST = {}                                                  # mutant -> (ratio, case) of its weakest rejection


@pytest.mark.parametrize("group", GROUPS)
def test_rounded_is_accepted_and_every_mutant_rejected(group):
    top = 0.0
    for c in by_group(group):
        d = P.inputs(c)
        ref = P.reference(c, d)
        own = P.reject_ratio(c, P.outputs_of(c, ref), ref)
        top = max(top, own)
        assert own <= 1.0, f"{c['name']}: the rounded form misses its own comparator ({own:.4g}): the derivation lacks a term"
        base1 = P.outputs_of(c, ref)
        base2 = None
        for m in P.MUTANTS:
            if not P.relevant(c, m):
                continue
            base = base1
            if m in P.STAT_MUTANTS:                           # these take two-pass float64 statistics: so does the form they are compared with
                if base2 is None:
                    r2 = P.reference(c, d, mutant="twopass", forms=("rounded",))
                    base2 = P.outputs_of(c, {**{k: {"rounded": v["rounded"]} for k, v in r2.items() if k != "stats_src"}, "stats_src": r2["stats_src"]})
                base = base2
            mref = P.reference(c, d, mutant=m, forms=("rounded",))
            got = P.outputs_of(c, {**{k: {"rounded": v["rounded"]} for k, v in mref.items() if k != "stats_src"}, "stats_src": mref["stats_src"]}, m)
            if all(torch.equal(torch.nan_to_num(got[k], nan=-7.0), torch.nan_to_num(base[k], nan=-7.0)) for k in base):
                continue                                      # the mutant computes the same thing here
            ratio = P.reject_ratio(c, got, ref)
            assert ratio > 1.0, f"{c['group']} {c['name']}: mutant {m} is accepted ({ratio:.4g})"
            if m not in WEAKEST or ratio < WEAKEST[m][0]:
                WEAKEST[m] = (ratio, f"{c['group']} {c['name']}")
            WEAKEST.setdefault(m + " #", [0])[0] += 1
    conftest.record(top, f"group {group}: rounded, largest ratio")


def test_record_the_unbiased_variance_mutant():
    """P.UNBIASED_NOTE: recorded, not asserted -- at how many folded cases `check` accepts a variance over n - 1"""
    acc, n, top = 0, 0, 0.0
    for c in [c for c in CASES if c["nparts"]][::4]:
        d = P.inputs(c)
        ref = P.reference(c, d)
        mref = P.reference(c, d, mutant="unbiased", forms=("rounded",))
        ratio = P.reject_ratio(c, {k: v["rounded"] for k, v in mref.items() if k != "stats_src"}, ref)
        acc, n, top = acc + int(ratio <= 1.0), n + 1, max(top, ratio)
    conftest.record(acc, f"mutant unbiased: accepted at (of {n} folded cases; largest ratio {top:.3f})")


def test_every_mutant_was_rejected_somewhere():
    """(runs after the groups) every listed mutant differed, and was rejected, at one case of the GPU file at least"""
    if len([k for k in WEAKEST if not k.endswith("#")]) == 0:
        pytest.skip("the group tests did not run in this session")
    for m in [m for m in P.MUTANTS if m != "unbiased"]:
        assert m in WEAKEST, f"mutant {m} never differs from the unmutated form at any case"
        conftest.record(WEAKEST[m][0], f"mutant {m}: weakest rejection over {WEAKEST[m + ' #'][0]} cases ({WEAKEST[m][1]})")


# ---------------------------------------------------------------------------------------------------------------------------------
# recorded, not asserted: what tests/test_gpu_pgemm.py's `close` makes of the mutants at ITS shapes and draws
# ---------------------------------------------------------------------------------------------------------------------------------
def bf(x):
    return x.to(torch.bfloat16).float()


def old_draws():
    """(case, inputs, float32 want) for test_lora_residual, test_qkv_layernorm_folded_lora_vt and test_geglu_layernorm_folded as that file
    draws them (same seeds, same order of draws)"""
    out = []
    for M, K, N, r in [(1000, 256, 256, 4), (504, 384, 384, 8), (512, 640, 640, 4), (200, 256, 256, 16), (333, 384, 384, 32)]:
        g = torch.Generator().manual_seed(2)
        x, w, b = bf(torch.randn(M, K, generator=g)), bf(torch.randn(N, K, generator=g) / math.sqrt(K)), torch.randn(N, generator=g)
        A, Bm = bf(torch.randn(r, K, generator=g) / r), bf(torch.randn(N, r, generator=g) * 0.05)
        res = bf(torch.randn(M, N, generator=g))
        want = x @ w.t() + b + 2.0 * (x @ A.t()) @ Bm.t() + res
        c = P.case("old", f"lora_residual M{M} K{K} r{r}", M, K, N, (1, 32, 1, 4), ranks=(r,), res=True, stats=True)
        out.append((c, dict(x=x.to(F64), W=w.to(F64), bias=b, parts=[(0, N, A, Bm, 2.0)], res=res.to(F64), gate=None, lp=None, layout=None), want))
    for B, Nt, Cc, r, nparts in [(2, 1000, 256, 4, 4), (3, 252, 384, 4, 6), (2, 64, 640, 4, 10), (2, 63, 256, 8, 2), (1, 250, 384, 0, 3)]:
        g = torch.Generator().manual_seed(3)
        M = B * Nt
        x, w, b = bf(torch.randn(M, Cc, generator=g) * 1.7 + 0.4), bf(torch.randn(3 * Cc, Cc, generator=g) / math.sqrt(Cc)), torch.randn(3 * Cc, generator=g)
        gm, bt = torch.randn(Cc, generator=g) * 0.3 + 1, torch.randn(Cc, generator=g) * 0.2
        xn = F.layer_norm(x, (Cc,), gm, bt, 1e-5)
        want = xn @ w.t() + b
        parts = []
        for i in range(3 if r else 0):
            A, Bm = bf(torch.randn(r, Cc, generator=g) / r), bf(torch.randn(Cc, r, generator=g) * 0.05)
            want[:, i * Cc:(i + 1) * Cc] += 1.5 * (xn @ A.t()) @ Bm.t()
            parts.append((i * Cc, Cc, A, Bm, 1.5))
        c = P.case("old", f"qkv_ln_vt B{B} N{Nt} C{Cc} r{r}", M, Cc, 3 * Cc, (1, 32, 1, 4), ranks=(r,) * (3 if r else 0), nparts=nparts,
                   vt=dict(B=B, col0=2 * Cc))
        out.append((c, dict(x=x.to(F64), W=w.to(F64), bias=b, parts=parts, res=None, gate=None, gamma=gm.to(F64), beta=bt.to(F64),
                            lp=P.ln_partials(x.to(F64), nparts), layout=None), want))
    for M, Cc, nparts in [(1000, 256, 4), (130, 640, 5)]:     # (the 2016 x 384 case is left out of this record: 3 s per mutant)
        g = torch.Generator().manual_seed(4)
        x, w, b = bf(torch.randn(M, Cc, generator=g) * 1.3 - 0.2), bf(torch.randn(8 * Cc, Cc, generator=g) / math.sqrt(Cc)), torch.randn(8 * Cc, generator=g)
        gm, bt = torch.randn(Cc, generator=g) * 0.3 + 1, torch.randn(Cc, generator=g) * 0.2
        h = F.layer_norm(x, (Cc,), gm, bt, 1e-5) @ w.t() + b
        c = P.case("old", f"geglu_ln M{M} C{Cc}", M, Cc, 8 * Cc, (1, 64, 1, 4), geglu=True, nparts=nparts)
        out.append((c, dict(x=x.to(F64), W=w.to(F64), bias=b, parts=[], res=None, gate=None, gamma=gm.to(F64), beta=bt.to(F64),
                            lp=P.ln_partials(x.to(F64), nparts), layout=None), h[:, :4 * Cc] * F.gelu(h[:, 4 * Cc:])))
    return out


def test_record_what_the_old_comparator_accepts():
    accepted, tried = {}, {}
    wrap = lambda r: {k: v["rounded"] for k, v in r.items() if k in ("y", "vt")}
    for c, d, want in old_draws():
        c["eps"] = P.EPS                                      # (that file's eps)
        rtol = 1.2e-2 if c["name"].startswith("lora") else 2e-2
        base1, base2 = wrap(P.reference(c, d, forms=("rounded",))), None
        for m in P.MUTANTS:
            if not (P.relevant(c, m) or (m == "unbiased" and c["nparts"])) or m in ("gate_of_block", "gate_after_last"):
                continue
            base = base1
            if m in P.STAT_MUTANTS:
                base2 = base2 if base2 is not None else wrap(P.reference(c, d, mutant="twopass", forms=("rounded",)))
                base = base2
            mref = P.reference(c, d, mutant=m, forms=("rounded",))
            y = torch.cat([mref["y"]["rounded"], mref["vt"]["rounded"][:, :, :c["M"] // c["vt"]["B"]].permute(0, 2, 1).reshape(c["M"], -1)], 1) \
                if c["vt"] else mref["y"]["rounded"]
            same = all(torch.equal(torch.nan_to_num(mref[k]["rounded"], nan=-7.0), torch.nan_to_num(base[k], nan=-7.0)) for k in base)
            if m == "stats_pre_round":                        # that file's check of the table: the row sums at rtol 1e-4, atol 1e-2
                st = P.rowstat_entries(mref["stats_src"], 32)[0].float()
                s1, s2 = mref["y"]["rounded"].float().sum(1), (mref["y"]["rounded"].float() ** 2).sum(1)
                ok = torch.allclose(st[:, :, 0].sum(1), s1, rtol=1e-4, atol=1e-2) and torch.allclose(st[:, :, 1].sum(1), s2, rtol=1e-4, atol=1e-2)
            elif same:
                continue
            else:
                pad_ok = not c["vt"] or bool(torch.isnan(mref["vt"]["rounded"][:, :, c["M"] // c["vt"]["B"]:]).all())
                ok = pad_ok and bool(torch.isfinite(y).all()) and P.old_close(y, want, rtol)
            tried[m] = tried.get(m, 0) + 1
            accepted[m] = accepted.get(m, 0) + int(ok)
    for m in sorted(tried):
        conftest.record(accepted[m], f"old comparator: mutant {m} accepted at (of {tried[m]} old shapes)")
    assert tried


# ---------------------------------------------------------------------------------------------------------------------------------
# launch arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def brute_plan(M, N, K, Rp, used, res, geglu, vt_col0, max_ranges):
    """every quadruple in a plain product of the value sets, filtered by the stated rules, least cost first in the planner's order"""
    rt = P.rt_of(used) if Rp else 0
    best = None
    for nw, mi, nt, tpr in itertools.product((4, 8), (1, 2), (32, 64), range(1, 65)):
        if mi == 2 and not ((K <= 384 or rt == 0) and nw == 4):
            continue
        if (geglu and nt != 64) or (vt_col0 is not None and vt_col0 % nt) or N % (nt * tpr) or tpr * nt > 512:
            continue
        if max_ranges and N // (nt * tpr) > max_ranges:
            continue
        bm = 16 * mi * nw
        if min(tpr, 3) * (nt * K * 2 + (bm * nt * 2 if res else 0)) + 8 * bm + 8 * tpr * nt + tpr * nt * Rp * 2 > 160 * 1024:
            continue
        cost = P.plan_cost(M, N, K, (mi, nt, tpr, nw), Rp=Rp, ranks_used=used, res=res, geglu=geglu)
        if best is None or cost < best[0]:
            best = (cost, (mi, nt, tpr, nw))
    return best and best[1]


def test_plan_restatement_against_enumeration_and_library():
    from audioldm_with_lora_amd import _lib
    lib = _lib.load()
    dummy = C.c_void_p(64)
    for M, (N, K), (Rp, used), res, max_ranges in itertools.product((1, 70, 260, 1000, 8000), ((128, 256), (768, 256), (1152, 384), (640, 640), (1920, 640)),
                                                                    ((0, 0), (32, 4), (32, 17), (64, 20)), (False, True), (0, 16)):
        for geglu, vt_col0 in ((False, None), (True, None), (False, N // 2 if (N // 2) % 32 == 0 else None)):
            if geglu and (Rp or res):
                continue
            mine = P.plan(M, N, K, Rp=Rp, ranks_used=used, res=res, geglu=geglu, vt_col0=vt_col0, max_ranges=max_ranges)
            assert mine == brute_plan(M, N, K, Rp, used, res, geglu, vt_col0, max_ranges)
            a = _lib.PgemmArgs()
            a.M, a.N, a.K, a.Rp, a.ranks_used, a.geglu, a.max_ranges = M, N, K, Rp, used, int(geglu), max_ranges
            a.res = dummy if res else None
            if vt_col0 is not None:
                a.vt, a.vt_col0 = dummy, vt_col0
            rc = lib.aldm_pgemm_plan(C.byref(a))
            assert (rc == 0) == (mine is not None) and (mine is None or (a.mi, a.nt, a.tiles_per_range, a.waves) == mine), (M, N, K, Rp, used, res, mine)
    for c in CASES:                                           # every forced shape of the GPU file is a candidate of its launch
        rp = c["Rp"] or (32 if c["ranks"] else 0)
        cands = P.plan_candidates(c["M"], c["N"], c["K"], Rp=rp, ranks_used=sum(c["ranks"]) + c["layout_col0"], res=c["res"], geglu=c["geglu"],
                                  vt_col0=(c["vt"]["col0"] if c["vt"] else None), fixed=c["cfg"])
        assert cands == [c["cfg"]], c["name"]
    assert [P.rt_of(r) for r in (0, 1, 15, 16, 17, 31, 32)] == [0, 1, 1, 1, 2, 2, 2]
    assert not P.plan_candidates(70, 128, 640, Rp=32, ranks_used=4, fixed=(2, 32, 2, 4)), "K = 640 with an adapter has no mi = 2 form"
    assert P.lds_bytes(640, 1, 64, 2, 4, False, 0) > P.LDS_MAX >= P.lds_bytes(640, 1, 64, 1, 4, False, 0)


def test_vt_vec_restatement_and_the_arms_of_group_d():
    assert [P.vt_vec(*a) for a in [(64, 64, 4096, 0), (64, 68, 68 * 64, 0), (64, 64, 4096, 4), (64, 65, 65 * 64, 0), (64, 64, 4096, 1),
                                   (12, 16, 1024, 0), (12, 16, 1024, 2), (9, 16, 1024, 0), (8, 8, 512, 0)]] == [8, 4, 4, 1, 1, 4, 1, 1, 8]
    arms = {}
    for c in by_group("D"):
        *_, off, vec = P.vt_geom(c)
        arms.setdefault((vec, c["cfg"][0]), set()).add("offset" if (c["vt"].get("pad") or off) else "natural")
    for vec in (8, 4, 1):
        for mi in (1, 2):
            assert arms[(vec, mi)] == {"natural", "offset"}, (vec, mi, arms.get((vec, mi)))   # (offset: demoted from above; 8: kept)
    grids = {P.grid_of(c["M"], c["N"], c["cfg"]) for c in by_group("A")}
    assert set(range(1, 8)) <= grids and any(g > 8 and g % 8 for g in grids), sorted(grids)
    assert {c["nparts"] for c in by_group("D")} >= set(P.D_NPARTS) and {c["nparts"] for c in by_group("E")} == {0, 1, 16}
