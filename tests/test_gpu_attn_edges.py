"""GPU parity of the attention forms that INFERENCE runs -- ops.attention(prescaled=True), ops.attention(kv_len=),
ops.attention(fp8=True), attn_block64(fp8=True) and ops.attention_wide -- against the float64 restatements of
tests/attn_restatement.py: per element within a bound that has nothing measured in it (`check_elem`) and within twice the L2 floor /
four times the max floor (`check`) for the bf16 forms, `check` against the e4m3 floor for the fp8 form.  Every case asserts the
arithmetic that puts it on its arm.  Q | K is a contiguous slice from the middle of a NaN arena, the V^T padding columns are NaN
(ops.attention: padding is ignored) or zero (ops.attention_wide: its contract), the output is the middle slice of a NaN arena whose
guard rows must still be NaN.  The draws matter as much as the comparator: see attn_restatement.draw_*.
tests/test_attn_restatement_host.py proves on the CPU that these comparators reject every listed mutant at exactly these shapes.
ALDM_ATTN_LOADERS stays unset: the product rule picks the loader-wave forms (bit-equal to NL = 0: test_gpu_attention_loaders.py)."""
import pytest
import torch

import attn_restatement as R
import conftest
import norm_restatement as NR
from attn_restatement import cdiv

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8           # NaN rows either side of Q | K and of the output


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    return o


def arena(rows, cols):
    """-> (whole NaN arena, its contiguous middle slice of `rows` rows)"""
    a = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=torch.bfloat16, device=DEV)
    return a, a[GUARD:GUARD + rows]


def operands(c, ref, zero_pad=False):
    """qk [B * N, 2C] in a NaN arena, vt [B, C, npad] with NaN (or, wide, zero) padding columns, out in a NaN arena"""
    q, k, v = ref["q"], ref["k"], ref["v"]
    B, H, N, d = q.shape
    C = H * d
    _, qk = arena(B * N, 2 * C)
    qk.copy_(torch.cat([R._rows(q), R._rows(k)], 1).to(torch.bfloat16))
    assert qk.is_contiguous() and qk.storage_offset() == GUARD * 2 * C
    npad = cdiv(N, 32) * 32 if zero_pad else cdiv(N, 8) * 8 + 8
    vt = torch.full((B, C, npad), 0.0 if zero_pad else float("nan"), dtype=torch.bfloat16, device=DEV)
    vt[:, :, :N] = v.permute(0, 1, 3, 2).reshape(B, C, N).to(torch.bfloat16)
    whole, out = arena(B * N, C)
    return qk, vt, whole, out


def guards_untouched(whole, rows):
    assert bool(whole[:GUARD].isnan().all()) and bool(whole[GUARD + rows:].isnan().all()), "the kernel wrote outside its output"


def run_attention(ops, c, **kw):
    ref = R.cached_reference(c)
    qk, vt, whole, out = operands(c, ref)
    got = ops.attention(qk, vt, c.B, c.N, c.H, c.d, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    guards_untouched(whole, c.B * c.N)
    return ref, out


def launch_rule(N, H, B):
    """launch_attn_d, restated"""
    if N < 64: return 1, 1
    if N < 192: return 4, 1
    if N < 768: return 4, 2
    return (8, 1) if cdiv(N, 256) * H * B >= 256 else (8, 2)


A_ARMS = {1: (1, 1), 31: (1, 1), 33: (1, 1), 63: (1, 1), 64: (4, 1), 65: (4, 1), 127: (4, 1), 129: (4, 1), 191: (4, 1),
          192: (4, 2), 193: (4, 2), 200: (4, 2), 252: (4, 2), 320: (4, 2), 767: (4, 2), 768: (8, 2), 769: (8, 2)}


# ---- A: prescaled, every arm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.cases_a(), ids=R.case_id)
def test_prescaled_on_every_arm(ops, c):
    want = (8, 1) if (c.B, c.H) == (11, 8) else A_ARMS[c.N]
    assert launch_rule(c.N, c.H, c.B) == want == R.arm(c.N, c.H, c.B)
    assert R.remap_on(c.B, c.H) == ((c.B, c.H) in ((11, 8), (4, 2)))
    if c.N == 320:
        assert cdiv(c.N, 64) == 5                             # five tiles over two key groups: group 1 sits the last iteration out
    if c.N == 769:
        assert cdiv(c.N, 64) == 13
    ref, out = run_attention(ops, c, prescaled=True)
    if c.draw == "edge":
        R.draw_properties(c, ref)
    R.judge(out, ref, c, f"A {R.case_id(c)}")


# ---- B: every head dim ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.cases_b(), ids=R.case_id)
def test_prescaled_at_every_head_dim(ops, c):
    assert R.padded_d(c.d) in (16, 32, 48, 64, 80) and R.padded_d(c.d) - c.d in (0, 8)
    assert launch_rule(c.N, c.H, c.B) == ((4, 1) if c.N == 100 else (4, 2))
    ref, out = run_attention(ops, c, prescaled=True)
    R.judge(out, ref, c, f"B {R.case_id(c)}")


# ---- C: the deferred rescale ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.cases_c(), ids=R.case_id)
def test_prescaled_rescale_staircase(ops, c):
    assert launch_rule(c.N, c.H, c.B) == {191: (4, 1), 320: (4, 2), 767: (4, 2), 769: (8, 2)}[c.N]
    assert R.l_sums_rounded_p(c.d) == (c.d != 32)             # d = 32: l is the VALU sum; 48 / 80: the row of ones
    ref, out = run_attention(ops, c, prescaled=True)
    R.draw_properties(c, ref)                                 # which tiles cross RESCALE_THR: some row does, some row does not
    ex = R.rescale_trace(ref["q"], ref["k"], ref["v"], c.form)
    if c.draw == "stairs":
        geo = R.geometry(c.form, c.B, c.H, c.N)
        tiles = (ex[0, 0, ref["info"]["rows"][0]] > R.RESCALE_THR).nonzero().flatten().tolist()
        assert tiles and (geo.sp == 1 or {t % 2 for t in tiles} == {0, 1}), f"raises in tiles {tiles}: not in both key groups"
    R.judge(out, ref, c, f"C {R.case_id(c)}")


# ---- D: kv_len --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.cases_d(), ids=R.case_id)
def test_kv_len(ops, c):
    geo = R.geometry(c.form, c.B, c.H, c.N)
    assert launch_rule(c.N, c.H, c.B) == ((4, 1) if c.N == 129 else (4, 2))
    assert R.remap_on(c.B, c.H) == (c.N == 129) and len(set(c.lens)) == c.B
    if c.N == 129:
        assert R.clamp_len(c.lens[0], c.N) == 1 and R.clamp_len(c.lens[-1], c.N) == c.N and c.lens[-1] == c.N + 5
    lens = torch.tensor(c.lens, dtype=torch.int32, device=DEV)
    ref, out = run_attention(ops, c, kv_len=lens)
    if c.draw == "edge":
        R.draw_properties(c, ref)
    R.judge(out, ref, c, f"D {R.case_id(c)}")                 # rows < Nk
    o = out.view(c.B, c.N, c.H * c.d)
    for b in range(c.B):
        Nk = R.clamp_len(c.lens[b], c.N)
        pad0 = min(c.N, cdiv(Nk, geo.wg_rows) * geo.wg_rows)  # the first all-padding workgroup's first row
        assert bool(torch.isfinite(o[b, Nk:pad0].float()).all()), f"batch {b}: padding queries beside valid ones are not finite"
        assert not bool(o[b, pad0:].float().ne(0).any()), f"batch {b}: an all-padding workgroup did not write zeros"
        if geo.sp == 2 and Nk <= 64:
            assert cdiv(Nk, 64) == 1                          # key group 1 never sees a tile: the merge's idle branch


# ---- E: fp8 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.cases_e(), ids=R.case_id)
def test_fp8_operands(ops, c):
    assert launch_rule(c.N, c.H, c.B) == {40: (1, 1), 64: (4, 1), 129: (4, 1), 252: (4, 2), 320: (4, 2), 769: (8, 2)}[c.N]
    ref, out = run_attention(ops, c, fp8=True, prescaled=c.form == "fp8p")
    assert all(float(ref[t].abs().max()) < 448.0 for t in "qkv")
    e_l2, f_l2, _, _ = R.floor_ratios(out, ref["exact"], ref["rounded"])
    conftest.record(e_l2, f"E {R.case_id(c)} rel l2")
    conftest.record(f_l2, f"E {R.case_id(c)} e4m3 floor rel l2")
    R.judge(out, ref, c, f"E {R.case_id(c)}")


def pack_ln(ops, W, gm, bt, eps, parts):
    dv = lambda t: t.to(torch.float32).to(DEV)
    pw = ops.pack_linear_ln(dv(W), None, dv(gm), dv(bt), eps)
    if parts:
        ops.attach_lora(pw, [(r0, nr, A.to(DEV), Bm.to(DEV), s) for r0, nr, A, Bm, s in parts])
    return pw


@pytest.mark.parametrize("N", NR.ATTN64_NS)
def test_attn_block64_fp8(ops, N):
    H, d, B = 8, 80, 2
    C = H * d
    x, W, _, gm, bt, parts = NR.ln_linear_draw(B * N, C, 3 * C, 4)
    pw = pack_ln(ops, W, gm, bt, NR.EPS, parts)
    xd = x.to(torch.bfloat16).to(DEV)
    xs = xd.float().view(B * N, C // 64, 64)
    lp = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).contiguous()
    assert ops.attn_block64_ok(pw, N, H, d, lp)
    got = ops.attn_block64(xd, pw, lp, B, N, H, d, fp8=True)
    exact = R.attn_block_fp8(x, W, gm, bt, NR.EPS, parts, B, N, H, d)
    rounded = R.attn_block_fp8(x, W, gm, bt, NR.EPS, parts, B, N, H, d, rounded=True)
    R.check(got, exact, rounded, f"E attn_block64 fp8 N{N}")


# ---- F: the wide head -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.cases_f(), ids=R.case_id)
def test_attention_wide(ops, c):
    two = (c.B, c.N) in R.F_QT2
    assert (cdiv(c.N, 128) * c.B >= 192) == two and R.wide_qt(c.N, c.B) == (2 if two else 1)
    if (c.B, c.N) == (96, 130):
        assert cdiv(c.N, 128) == 2 and c.N - 128 == 2         # the second workgroup holds two queries
    ref = R.cached_reference(c)
    qk, vt, whole, out = operands(c, ref, zero_pad=True)
    assert vt.shape[2] % 32 == 0 and not bool(vt[:, :, c.N:].ne(0).any())
    got = ops.attention_wide(qk, vt, c.B, c.N, c.d, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    guards_untouched(whole, c.B * c.N)
    if c.draw in ("edge", "stairs"):
        R.draw_properties(c, ref)
    if c.draw == "stairs":
        rows = ref["info"]["rows"]
        assert all(r % 32 >= 16 for r in rows) or c.N < 32    # spikes for queries of a wave's second 16-row tile, none in its first
    R.judge(out, ref, c, f"F {R.case_id(c)}")
