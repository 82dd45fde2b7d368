"""CPU proof that the comparators of tests/test_gpu_attn_edges.py are sharp at the shapes that file uses (tests/attn_restatement.py):
(a) `exact` is torch's own float64 scaled_dot_product_attention; (b) every listed mutant is rejected at every GPU-file shape where it
changes anything, on the draw meant for it; (c) `rounded` itself is accepted everywhere and the draws have the properties they
claim; (d) what test_gpu_ops.py's `close` makes of the same mutants on that file's own shapes and draws -- recorded, not asserted;
(e) the finding that started this: a phantom key passes the floor rule on random scores and is caught on the negative draw."""
import math

import pytest
import torch
import torch.nn.functional as F

import attn_restatement as R
import conftest
from attn_restatement import F64, LOG2E

# mutant -> the draw meant for it
MUTANT_DRAW = dict(phantom="negative", drop_last="edge", kslot="diffuse", l_not_rescaled="stairs", no_reshift="stairs",
                   merge_swapped="diffuse", alpha_tile0="stairs", fp8_no_bias="tail")


def shapes():
    seen = {}
    for c in R.all_cases():
        seen.setdefault(c._replace(group="", draw=""), set()).add(c.draw)
    return seen


SHAPES = shapes()


def could_act(mutant, s):
    """Where a mutant can change anything at all, from the launch arithmetic alone (whether it DOES is then read off its output)."""
    geo = R.geometry(s.form, s.B, s.H, s.N)
    nks = [R.clamp_len(n, s.N) for n in s.lens] if s.lens is not None else [s.N]
    fp8 = s.form in R.FP8_FORMS
    return dict(phantom=True, drop_last=True, kslot=max(nks) >= 5,
                l_not_rescaled=s.form in ("prescaled", "varlen") and not R.l_sums_rounded_p(s.d) and max(nks) > geo.kt * geo.sp,
                no_reshift=s.form in ("prescaled", "wide") and max(nks) > geo.kt * geo.sp,
                merge_swapped=geo.sp == 2 and max(nks) > geo.kt,
                alpha_tile0=s.form == "wide" and R.wide_qt(s.N, s.B) == 2 and s.N > geo.kt,
                fp8_no_bias=fp8)[mutant] and (fp8 or mutant != "fp8_no_bias")


RESULTS = {m: [] for m in R.MUTANTS}          # mutant -> (shape id, rejected?, ratio) at every shape where it acted


@pytest.mark.parametrize("s", list(SHAPES), ids=lambda s: R.case_id(s._replace(draw="shape")))
def test_rounded_is_accepted_and_every_mutant_rejected(s):
    gpu_draws = SHAPES[s]
    mutants = {m: MUTANT_DRAW[m] for m in R.MUTANTS if could_act(m, s)}
    for dr in sorted(gpu_draws | set(mutants.values())):
        c = s._replace(draw=dr)
        ref = R.reference(c)
        rows = R.valid_rows(c)
        if c.form not in R.FP8_FORMS:                                           # (c): the restatement's own rounded form meets the bound
            ratio = R.elem_ratio(ref["rounded"][rows], ref["exact"][rows], ref["bound"][rows])
            assert ratio <= 1.0, f"{R.case_id(c)}: rounded is {ratio:.3f} x the bound"
        assert R.accepts(ref["rounded"][rows], ref["exact"][rows], ref["rounded"][rows])
        if dr in gpu_draws:
            R.draw_properties(c, ref)
        online = None
        for m, mdraw in mutants.items():
            if mdraw != dr:
                continue
            mut = R.attention(ref["q"], ref["k"], ref["v"], c.form, c.lens, mutant=m)
            base = ref["rounded"]
            if m in ("l_not_rescaled", "no_reshift", "merge_swapped", "alpha_tile0"):
                if online is None:                                              # the unmutated tile-by-tile form
                    online = R.attention(ref["q"], ref["k"], ref["v"], c.form, c.lens, mutant="online")
                    assert R.rejected(online, ref, c)[0] is False, "the unmutated tile-by-tile form is itself rejected"
                base = online
            if torch.equal(mut[rows].nan_to_num(nan=1e30), base[rows].nan_to_num(nan=1e30)):
                continue                                                        # changes nothing here
            rej, ratio = R.rejected(mut, ref, c)
            RESULTS[m].append((R.case_id(c), rej, ratio))
            assert rej, f"{m} is accepted at {R.case_id(c)} (strongest ratio {ratio:.3f})"


def test_every_mutant_acted_and_the_weakest_ratios():
    """Runs after the shapes above (file order): every mutant acted somewhere, and the table DESIGN.md quotes."""
    for m in R.MUTANTS:
        acted = RESULTS[m]
        assert acted, f"{m} never changed an output"
        assert all(r for _, r, _ in acted)
        conftest.record(len(acted), f"{m}: shapes that reject it")
        for name, part in (("bf16", [t for t in acted if not t[0].startswith("fp8")]), ("fp8", [t for t in acted if t[0].startswith("fp8")])):
            if part:
                weakest = min(part, key=lambda t: t[2])
                conftest.record(weakest[2], f"{m}: weakest {name} ratio (x its comparator's limit) at {weakest[0]}, of {len(part)}")


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,B,H,N,d,lens", [("varlen", 3, 2, 129, 40, (0, 65, 134)), ("varlen", 2, 2, 70, 48, (64, 70)),
                                               ("prescaled", 1, 2, 100, 56, None), ("prescaled", 2, 2, 65, 80, None),
                                               ("wide", 2, 1, 37, 128, None), ("fp8", 1, 2, 40, 24, None)])
def test_exact_is_float64_sdpa(form, B, H, N, d, lens):
    q, k, v, _ = R.draw_diffuse(form, B, H, N, d)
    got = R.attention(q, k, v, form, lens).view(B, N, H, d).permute(0, 2, 1, 3)
    qs = q / (LOG2E / math.sqrt(d)) if R.q_carries_scale(form) else q           # SDPA applies d^-0.5 and works in base e
    mask = None
    if lens is not None:
        nk = torch.tensor([R.clamp_len(n, N) for n in lens])
        mask = torch.zeros(B, 1, 1, N, dtype=F64).masked_fill(torch.arange(N).view(1, 1, 1, N) >= nk.view(B, 1, 1, 1), -math.inf)
    want = F.scaled_dot_product_attention(qs, k, v, attn_mask=mask)
    assert float((got - want).abs().max()) <= 1e-9


def test_e4m3_rounding_is_nearest_even_with_subnormals():
    x = torch.tensor([1.06, 300.0, 2.0 ** -10, 2.0 ** -9, 1.1875, 17.0], dtype=F64)
    assert R.r8(x).tolist() == [1.0, 288.0, 0.0, 2.0 ** -9, 1.25, 16.0]


def test_launch_rules():
    assert [R.arm(n, 2, 1) for n in (63, 64, 191, 192, 767, 768)] == [(1, 1), (4, 1), (4, 1), (4, 2), (4, 2), (8, 2)]
    assert R.arm(768, 8, 11) == (8, 1) and R.arm(768, 17, 5) == (8, 2)
    assert [R.wide_qt(n, b) for b, n in R.F_QT1] == [1] * 4 and [R.wide_qt(n, b) for b, n in R.F_QT2] == [2] * 3
    assert R.remap_on(11, 8) and R.remap_on(4, 2) and not R.remap_on(3, 2)
    assert R.edge_set(320, R.geometry("prescaled", 1, 2, 320)) == [0, 31, 32, 63, 64, 192, 255, 256, 318, 319]


# ---- (e) ------------------------------------------------------------------------------------------------------------------------
def test_phantom_key_passes_the_floor_rule_on_random_scores_and_not_on_negative_ones():
    s = R.Case("", "prescaled", 1, 2, 1000, 32, None, "diffuse")
    ref = R.reference(s)
    mut = R.attention(ref["q"], ref["k"], ref["v"], s.form, mutant="phantom")
    e_l2, f_l2, e_max, f_max = R.floor_ratios(mut, ref["exact"], ref["rounded"])
    conftest.record(e_l2 / f_l2, "phantom key, diffuse (1000, 32): l2 / floor")
    assert R.accepts(mut, ref["exact"], ref["rounded"]), "the floor rule now sees the phantom key on random scores: update DESIGN"
    neg = s._replace(draw="negative")
    ref = R.reference(neg)
    mut = R.attention(ref["q"], ref["k"], ref["v"], s.form, mutant="phantom")
    e_l2, f_l2, _, _ = R.floor_ratios(mut, ref["exact"], ref["rounded"])
    conftest.record(e_l2 / f_l2, "phantom key, negative (1000, 32): l2 / floor")
    assert not R.accepts(mut, ref["exact"], ref["rounded"]) and e_l2 / f_l2 > 20.0


# ---- (d) ------------------------------------------------------------------------------------------------------------------------
OLD_SHAPES = [(2, 1000, 8, 32), (2, 252, 8, 48), (2, 64, 8, 80), (1, 1008, 4, 16), (2, 256, 4, 24), (1, 64, 4, 40), (1, 16, 4, 40), (1, 1024, 8, 32)]


def old_draw(B, N, H, d, seed=9, qmul=1.5, spikes=()):
    """test_gpu_ops.py's attention draws (float32 randn, bf16-rounded, q x qmul, a key made a multiple of a query); kept to the first
    two heads of batch 0, which is what the mutants are evaluated on here."""
    bf = lambda x: x.to(torch.bfloat16).float()
    g = torch.Generator().manual_seed(seed)
    q, k, v = (bf(torch.randn(B, N, H * d, generator=g)) for _ in range(3))
    if qmul != 1.0:
        q = bf(q * qmul)
    for (bk, key, bq, row, f) in spikes:
        k[bk, key] = bf(q[bq, row] * f)
    return tuple(t[:1].view(1, N, H, d)[:, :, :2].permute(0, 2, 1, 3).to(F64).contiguous() for t in (q, k, v))


def test_what_the_old_comparator_made_of_the_mutants():
    """Data about the past: not asserted."""
    accepted = {m: [] for m in R.MUTANTS}
    for B, N, H, d in OLD_SHAPES:
        q, k, v = old_draw(B, N, H, d)
        geo = R.geometry("varlen", B, H, N)
        want = R.attention(q, k, v, "varlen", geo=geo)
        for m in ("phantom", "drop_last", "kslot", "merge_swapped"):
            if m == "merge_swapped" and geo.sp != 2:
                continue
            if R.old_close(R.attention(q, k, v, "varlen", mutant=m, geo=geo), want):
                accepted[m].append((N, d))
    # test_attention_prescaled_path_and_deferred_rescale's draw: a key 6 x a query at tile 14, batch 0
    B, N, H, d = 2, 1000, 8, 32
    q, k, v = old_draw(B, N, H, d, seed=12, qmul=1.0, spikes=[(0, 900, 0, 7, 6.0)])
    qs = R.bf16_input(q * (LOG2E / math.sqrt(d)))
    geo = R.geometry("prescaled", B, H, N)
    want = R.attention(q, k, v, "varlen", geo=geo)
    for m in ("l_not_rescaled", "no_reshift"):
        if R.old_close(R.attention(qs, k, v, "prescaled", mutant=m, geo=geo), want, rtol=3e-2, atol=1.5e-2):
            accepted[m].append((N, d))
    # test_attention_wide_head's draw (q x 2, key N - 10 = 1.5 x query 3): no case of that file reaches two query tiles per wave, so the
    # mutant is evaluated as if it had
    for B, N, d in [(2, 200, 128), (1, 1000, 256), (1, 37, 512)]:
        q, k, v = old_draw(B, N, 1, d, seed=13, qmul=2.0, spikes=[(0, N - 10, 0, 3, 1.5)] if N > 100 else ())
        qs = R.bf16_input(q * (LOG2E / math.sqrt(d)))
        want = R.attention(qs, k, v, "wide")
        mut = R.attention(qs, k, v, "wide", mutant="alpha_tile0")
        if not torch.equal(mut, R.attention(qs, k, v, "wide", mutant="online")) and R.old_close(mut, want, rtol=3e-2, atol=1.5e-2):
            accepted["alpha_tile0"].append((N, d))
    # test_attention_fp8_operands: rel L2 < 4e-2 against the reference on e4m3-rounded q, k, v and < 8e-2 against the plain one
    rel = lambda a, b: float((a - b).norm() / b.norm())
    for d, H, N, B in [(32, 8, 1000, 2), (48, 8, 252, 2), (80, 8, 64, 3), (16, 4, 40, 2)]:
        q, k, v = old_draw(B, N, H, d, seed=d + N, qmul=1.0)
        geo = R.geometry("fp8", B, H, N)
        mut = R.attention(q, k, v, "fp8", mutant="fp8_no_bias", geo=geo)
        if rel(mut, R.attention(R.r8(q), R.r8(k), R.r8(v), "fp8")) < 4e-2 and rel(mut, R.attention(q, k, v, "fp8")) < 8e-2:
            accepted["fp8_no_bias"].append((N, d))
    for m, where in accepted.items():
        conftest.record(len(where), f"old comparator accepts {m} at {where}")
