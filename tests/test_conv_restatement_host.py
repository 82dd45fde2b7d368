"""CPU: tests/conv_restatement.py is what it claims to be, and its comparator is sharp at the shapes of tests/test_gpu_conv_edges.py.

  * the tap loop equals float64 F.conv2d (F.interpolate(mode="nearest"), concat, stride, dilation, the 1x1 segment as a second conv2d, the
    epilogue spelled out again) to 1e-12 at every geometry of the GPU file;
  * `rounded` passes both comparators, and `exact` stored as float32 passes the fp32 bound: the reference stays inside its own bound;
  * every mutant of conv_restatement.MUTANTS is rejected by check_elem at every GPU-file shape where it applies, for the fp32 and the
    bf16 output (res_before_act / alpha_on_res2: bf16 only); whether the old comparator of test_gpu_ops.py accepted it is printed, not
    asserted (last section);
  * the launch arithmetic the GPU file asserts (split rule, halo capacity, straddling tiles) holds for the shapes as listed."""
import pytest
import torch
import torch.nn.functional as F

import conv_restatement as R
from bwd_restatement import F64, accepts

CASES = R.all_cases()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def torch_reference(c):
    """The same operation from torch's own float64 operators."""
    d, t = dict(c), R.draw(c)
    act = lambda v, k: v if k is None else (F.silu(v) if k == "silu" else F.leaky_relu(v, R.LRELU_SLOPE))
    x = t["x"] if t["x2"] is None else torch.cat([t["x"], t["x2"]], dim=-1)
    if d["in_act"]:
        x = F.leaky_relu(x, R.IN_SLOPE)
    x = _nchw(x)
    if d["up"] is not None:
        x = F.interpolate(x, size=d["up"], mode="nearest")
    y = F.conv2d(x, t["w"], None, stride=d["stride"], padding=d["pad"], dilation=d["dil"])
    if d["C3"]:
        e = t["x3"] if t["x4"] is None else torch.cat([t["x3"], t["x4"]], dim=-1)
        y = y + F.conv2d(_nchw(e), t["w_sc"][:, :, None, None])
    y = y.permute(0, 2, 3, 1)
    if t["bias"] is not None:
        y = y + t["bias"]
    if t["rowbias"] is not None:
        y = y + t["rowbias"][:, None, None, :]
    y = act(y, d["out_act"])
    if t["res"] is not None:
        y = y + t["res"]
    y = d["alpha"] * y
    if t["res2"] is not None:
        y = y + t["res2"]
    if d["out2"]:
        return y, act(y, d["post_act"])
    return act(y, d["post_act"]), None


def test_case_names_are_unique():
    names = [dict(c)["name"] for c, _ in CASES]
    assert len(set(names)) == len(names)


def test_restatement_equals_torch_float64():
    worst = 0.0
    for c, _ in CASES:
        ref = R.cached_reference(c)
        want, want2 = torch_reference(c)
        assert ref["exact"].shape == want.shape == (dict(c)["B"],) + R.out_hw(c) + (dict(c)["N"],)
        err = float((ref["exact"] - want).abs().max())
        if want2 is not None:
            err = max(err, float((ref["exact2"] - want2).abs().max()))
        worst = max(worst, err)
        assert err <= 1e-12, (dict(c)["name"], err)
        assert float(ref["exact"].abs().max()) > 0.5
    print(f"restatement vs torch float64 over {len(CASES)} cases: max |diff| {worst:.3g}")


def test_reference_stays_inside_its_own_bound():
    silu_units = []
    for c, _ in CASES:
        ref = R.cached_reference(c)
        name = dict(c)["name"]
        for second in ((False, True) if dict(c)["out2"] else (False,)):
            sfx = "2" if second else ""
            R.check_both(ref["rounded" + sfx], ref, name, False, second, record=lambda v, w: None)
            R.check_elem(ref["exact" + sfx].to(torch.float32), ref, name, True, second, record=lambda v, w: None)
            if ref["unit" + sfx]:
                silu_units.append(ref["unit" + sfx])
    assert silu_units and max(silu_units) < 2e-6                # a float32 silu is good to a few ulps of O(1) values
    print(f"silu unit on the reference: max {max(silu_units):.3g} over {len(silu_units)} outputs (x SILU_MARGIN {R.SILU_MARGIN})")


def test_half_ulp_is_the_formats():
    """2^-9 t, the smallest multiple of t a half-ulp can be, is below bf16's own rounding: `rounded` fails a bound built on it, so
    conv_restatement.bound uses the exact half-ulp 2^(floor(log2 t) - 8), which lies in (2^-9 t, 2^-8 t]."""
    t = torch.tensor([1.0, 1.5, 1.99, 2.0, 3.0, 0.75], dtype=F64)
    assert torch.equal(R.half_ulp_bf16(t), torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -9], dtype=F64))
    v = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=F64)              # just below the midpoint of two bf16 values
    err = (v.to(torch.bfloat16).to(F64) - v).abs()
    assert bool(err <= R.half_ulp_bf16(v)) and bool(err > 2.0 ** -9 * v)
    c = CASES[0][0]
    ref = R.cached_reference(c)
    b32 = (ref["n"] + 1) * 2.0 ** -24 * ref["mag"]
    ratio = float(((ref["rounded"] - ref["exact"]).abs() / (b32 + 2.0 ** -9 * (ref["exact"].abs() + b32))).max())
    print(f"`rounded` against b32 + 2^-9 (|exact| + b32) at '{dict(c)['name']}': {ratio:.3f} x")
    assert ratio > 1.0


def applies(mutant, c, bm):
    d = dict(c)
    (OH, OW), (VH, VW) = R.out_hw(c), (d["up"] if d["up"] is not None else (d["IH"], d["IW"]))
    last_row = (OH - 1) * d["stride"][0] + (d["k"][0] - 1) * d["dil"][0] - d["pad"][0]       # the last image row / column a window reads:
    last_col = (OW - 1) * d["stride"][1] + (d["k"][1] - 1) * d["dil"][1] - d["pad"][1]       # (12 x 8 under stride 2 never reads past the image)
    return {"pad_right_wrap": last_col >= VW, "pad_bottom_next": last_row >= VH and d["B"] > 1, "up_round": d["up"] is not None,
            "concat8": d["C2"] > 0, "ktile_dropped": True, "ktile_twice": True,
            "rowbias_tile_first": d["rowbias"] and R.straddles(c, bm), "res_before_act": d["res"] and d["out_act"] is not None,
            "alpha_on_res2": d["res2"] and d["alpha"] != 1.0, "x4_reads_x3": d["C4"] > 0,
            "stride_no_pad": d["stride"][0] > 1 and d["pad"][0] > 0, "k_elem_lastcol": True}[mutant]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_rejected_at_every_gpu_shape(mutant):
    shapes, old_ok, floor_ok, weakest = 0, 0, 0, float("inf")
    for c, bms in CASES:
        d = dict(c)
        ref = R.cached_reference(c)
        for bm in (bms if mutant == "rowbias_tile_first" else bms[:1]):
            if not applies(mutant, c, bm):
                continue
            m = R.reference(c, mutant=mutant, bm=bm)
            if mutant == "up_round" and d["up"] == (2 * d["IH"], 2 * d["IW"]):
                assert torch.equal(m["exact"], ref["exact"])        # exact 2x: both index rules agree
                continue
            shapes += 1
            rb = R.elem_ratio(m["rounded"], ref, False)
            assert rb > 1.0, (mutant, d["name"], bm, "bf16", rb)
            weakest = min(weakest, rb)
            floor_ok += accepts(m["rounded"], ref["exact"], ref["rounded"])      # the per-tensor floor rule alone (not asserted: one column in 136 hides in it)
            if mutant not in R.BF16_ONLY:
                rf = R.elem_ratio(m["exact"].to(torch.float32), ref, True)
                assert rf > 1.0, (mutant, d["name"], bm, "fp32", rf)
            old_ok += R.old_close(m["rounded"], ref["exact"])
    assert shapes > 0, f"{mutant}: no GPU-file shape exercises it"
    print(f"| {mutant} | rejected at {shapes} of {shapes} shapes (weakest bf16 err/bound {weakest:.3g}) | old comparator accepted it at {old_ok} of {shapes} | "
          f"floor rule alone accepted it at {floor_ok} |")


def test_launch_arithmetic_of_the_listed_shapes():
    # split rule: an effective count below the request, a one-K-tile tail, a zero-padded tail K-tile
    assert [R.split_rule(s, 9, 1, 9, False) for s in R.C_SPLITS] == [2, 3, 5, 5, 9, 9]
    assert 9 % R.cdiv(9, 2) == 4 and 9 - 4 * R.cdiv(9, 5) == 1      # 5 + 4; 2 + 2 + 2 + 2 + 1
    assert R.nkt_of(R.C_TAIL[0]) == 11 and (9 * 72) % 64 == 8
    assert [R.split_rule(s, 27, 3, 9, True) for s in R.C_HALO_SPLITS] == [2, 3, 3, 3]           # 3 chunks: 2 + 1, 1 + 1 + 1, more splits than chunks
    assert [R.split_rule(s, 36, 4, 9, True) for s in R.C_HALO_SPLITS] == [2, 2, 4, 4]           # 4 chunks asked 3 -> 2 + 2
    # halo capacity: three and five DMA passes on the 128-row tiles, 128 rows on the 64-row tiles
    assert [R.halo_need(7, w) for w in (16, 8, 4, 32, 64)] == [180, 180, 204, 204, 264]
    assert [R.halo_need(8, w) for w in (16, 4, 8, 2, 32)] == [108, 108, 100, 136, 136]
    for tile in R.HALO:
        for c, _ in R.b_cases(tile):
            OH, OW = R.out_hw(c)
            assert OH % (R.TILE_BM[tile] // OW) in (0, 1, R.TILE_BM[tile] // OW - 1)
    # every generic base shape: a ragged last tile and a tile over an image boundary
    for c in R.A_BASE:
        OH, OW = R.out_hw(c)
        assert all((3 * OH * OW) % bm and R.straddles(c, bm) for bm in (64, 128)) and 3 * OH * OW < 256
    for c in R.A_BIG:
        OH, OW = R.out_hw(c)
        assert (2 * OH * OW) % 256 and R.straddles(c, 256)

