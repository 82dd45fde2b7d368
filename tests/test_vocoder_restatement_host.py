"""CPU proof that the floor rule of tests/test_gpu_vocoder_edges.py is sharp at the shapes that test runs: `accepts` (the two conditions
of `check`) and the fp32 bound reject every listed mutant of tests/vocoder_restatement.py wherever the mutant changes anything, and
accept the rounded restatement itself.  Where a mutant cannot be seen the reason is arithmetic, stated next to the predicate, and the
test asserts that the mutant's output is then IDENTICAL to the rounded restatement -- nothing is skipped silently.  Also: what the old
comparators (the end-to-end rel L2 < 4e-2 through oracle.hifigan, and `old_close`) accept of the same mistakes."""
import math

import pytest
import torch
import torch.nn.functional as F

import vocoder_restatement as V
from bwd_restatement import F64, accepts, floor_ratios, old_close


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements against torch and against each other
# ---------------------------------------------------------------------------------------------------------------------------------
def test_phase_plan_is_the_product_plan():
    from audioldm_with_lora_amd.vocoder import transpose_phase_plan
    for k, u, p in V.CT_KUP + [(3, 4, 0), (7, 3, 2)]:
        for T in (1, 2, 3, 9, 86):
            L = V.ct_out_len(T, k, u, p)
            assert transpose_phase_plan(k, u, p, L) == V.phase_plan(k, u, p, L), (k, u, p, T)


def test_restatements_match_torch_float64():
    for k, u, p in V.CT_KUP:
        w, b = V.draw_convt(8, 4, k, u, 1)
        for T in (1, 2, 3, 13):
            x = V.draw_x(2, T, 8, T)
            L = V.ct_out_len(T, k, u, p)
            want = F.conv_transpose1d(x.transpose(1, 2), w, b, stride=u, padding=p).transpose(1, 2)
            assert want.shape[1] == L
            torch.testing.assert_close(V.conv_transpose1d(x, w, b, u, p, L), want, rtol=0, atol=1e-12)
            torch.testing.assert_close(V._ct_phases(x, w, b, u, p, L), want, rtol=0, atol=1e-12)
    for K, d in ((3, 1), (7, 3), (11, 5)):
        x = V.draw_x(2, 300, 8, K)
        (w1, b1), (w2, b2) = V.draw_conv(8, 8, K, K), V.draw_conv(8, 8, K, K + 2)
        want = F.conv1d(x.transpose(1, 2), w1, b1, dilation=d, padding=d * (K - 1) // 2).transpose(1, 2)
        torch.testing.assert_close(V.conv1d(x, w1, b1, d), want, rtol=0, atol=1e-12)
        t = F.leaky_relu(F.conv1d(F.leaky_relu(x, 0.1).transpose(1, 2), w1, b1, dilation=d, padding=d * (K - 1) // 2), 0.1)
        want = x + F.conv1d(t, w2, b2, padding=(K - 1) // 2).transpose(1, 2)
        torch.testing.assert_close(V.respair(x, w1, b1, d, w2, b2, 0.1), want, rtol=0, atol=1e-12)
        torch.testing.assert_close(V.respair(x, w1, b1, d, w2, b2, 0.1, mutant="tiled"), want, rtol=0, atol=1e-12)
        wp, bp = V.draw_conv(1, 8, K, 5)
        want = torch.tanh(F.conv1d(x.transpose(1, 2), wp, bp, padding=(K - 1) // 2))[:, 0]
        torch.testing.assert_close(V.to1(x, wp[0], bp[0])["out"], want, rtol=0, atol=1e-12)


def test_stage_forms_match_the_oracle_stage():
    """Both compositions of one stage (fused pairs, igemm chain), exact form, against HifiGanResidualBlock / ConvTranspose1d of the oracle."""
    from oracle.hifigan import HifiGanResidualBlock
    prm = V.draw_stage(16, 4, 2, (3, 7, 11), ((1, 3, 5),) * 3, seed=3)
    a = V.draw_x(2, 9, 16, 4)
    w, b, u, p = prm["up"]
    h = F.conv_transpose1d(a.transpose(1, 2), w, b, stride=u, padding=p)
    acc = 0.0
    for K, dils, pairs in prm["blocks"]:
        rb = HifiGanResidualBlock(8, K, dils, 0.1).double()
        for q, (w1, b1, w2, b2) in enumerate(pairs):
            rb.convs1[q].weight.data, rb.convs1[q].bias.data, rb.convs2[q].weight.data, rb.convs2[q].bias.data = w1, b1, w2, b2
        with torch.no_grad():
            acc = acc + rb(h)
    for last in (False, True):
        want = F.leaky_relu(acc / 3, 0.01 if last else 0.1).transpose(1, 2)
        for fused in (True, False):
            hh, aa = V.stage(a, prm, 0.1, last, fused)
            torch.testing.assert_close(hh, h.transpose(1, 2), rtol=0, atol=1e-12)
            torch.testing.assert_close(aa, want, rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------------------
# transposed convolution
# ---------------------------------------------------------------------------------------------------------------------------------
def _ct_visible(m, k, u, p, T, entry):
    """Does mutant m, put into this phase launch, change any output?  Index arithmetic only.  A phase's tap i reads input q - i for the
    outputs q = q0 .. q0 + nq - 1; a tap is live when phi + u i < k."""
    phi, q0, t0, nq = entry
    qs = range(q0, q0 + nq)
    ntap = V.cdiv(k, u)
    live = [i for i in range(ntap) if phi + u * i < k]
    if m == "ghost_tap":      # only a phase with a zero column (k % u != 0 and phi >= k % u) has a ghost tap, and it must read an input that exists
        return any(0 <= q - i < T for i in range(ntap) if i not in live for q in qs)
    if m == "fwd_taps":       # tap 0 reads input q in either order: nothing changes unless some other tap has an input in range in one of the orders
        return any(0 <= q - i < T or 0 <= q + i < T for i in live if i > 0 for q in qs)
    if m == "next_item":      # nothing changes unless the phase reads past the end of an item (q - i >= T) at all
        return any(q - i >= T for i in live for q in qs)
    return True


@pytest.mark.parametrize("kup", V.CT_KUP)
@pytest.mark.parametrize("ch", V.CT_CH)
def test_check_rejects_transposed_conv_mutants(kup, ch):
    (k, u, p), (ci, co) = kup, ch
    w, b = V.draw_convt(ci, co, k, u, k * u + ci)
    seen = set()
    for T in V.ct_Ts(k, u, p):
        x = V.draw_x(V.CT_B, T, ci, T + k)
        L = V.ct_out_len(T, k, u, p)
        e, e2 = V.conv_transpose1d(x, w, b, u, p, L, copy_slope=0.1)
        r, r2 = V.conv_transpose1d(x, w, b, u, p, L, copy_slope=0.1, rounded=True)
        assert accepts(r, e, r) and accepts(r2, e2, r2)
        g, g2 = V.conv_transpose1d(x, w, b, u, p, L, copy_slope=0.1, rounded=True, mutant="copy_slope")
        assert bool((g == r).all()) and not accepts(g2, e2, r2), ("copy_slope", T)
        for mp, entry in enumerate(V.phase_plan(k, u, p, L)):
            for m in V.CT_MUTANTS[:-1]:
                g, g2 = V.conv_transpose1d(x, w, b, u, p, L, copy_slope=0.1, rounded=True, mutant=m, mphase=mp)
                if _ct_visible(m, k, u, p, T, entry):
                    assert not accepts(g, e, r) and not accepts(g2, e2, r2), (m, T, entry)
                    seen.add(m)
                else:
                    assert bool((g == r).all()) and bool((g2 == r2).all()), (m, T, entry)
    # every mutant was visible, and rejected, at some T of this case -- except the ghost tap where k % u == 0: no phase has a zero column
    assert seen == set(V.CT_MUTANTS[:-1]) - ({"ghost_tap"} if k % u == 0 else set()), seen


def test_ragged_T_really_is_ragged():
    for k, u, p in V.CT_KUP:
        for bm in V.CT_TILE_HEIGHTS:
            T = V.ct_ragged_T(bm, k, u, p)
            rows = [V.CT_B * nq for _, _, _, nq in V.phase_plan(k, u, p, V.ct_out_len(T, k, u, p))]
            assert any(m > bm and m % bm for m in rows), (k, u, p, bm, T, rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# residual pair
# ---------------------------------------------------------------------------------------------------------------------------------
def _pair_applies(m, C, K, d, B, T, mrf, last):
    """Does the mutant change anything at this shape?  (False: its output must be identical.)"""
    P2, PH = (K - 1) // 2, V.pair_halo(K, d)
    if m in ("left_halo", "mid_left"):
        return T > V.TT                                        # a tile with a left neighbour exists (its halo rows are inside the sequence: PH < 256)
    if m == "right_halo":
        return T >= V.TT + PH                                  # the last halo row of tile 0, t = 255 + PH, is inside the sequence
    if m == "mid_right":
        return T >= V.TT + P2                                  # the last conv1 position of tile 0, t = 255 + P2, is inside the sequence
    if m == "alpha_on_res2":
        return mrf                                             # the plain form has no res2
    if m == "post_slope":
        return mrf and last                                    # 0.1 in place of 0.01: only the last stage's MRF form asks for 0.01
    if m == "stale_tile":
        return B * V.cdiv(T, V.TT) > V.pair_grid(C)            # some workgroup walks a second tile
    if m == "prev_item":
        return B > 1
    return True


def _pair_required(m, K, mrf):
    """The run one row short changes ONE output row, by one conv1 tap seen through one conv2 tap: rms alpha E[lrelu(x)^2] / K =
    0.505 alpha / K per element.  At K = 11 in the MRF form (alpha = 1/3) that is 0.015: below the half-ulp 2^-6 of the largest outputs
    (|v| >= 4) that sets the max floor, and one row of >= 771 cannot move the L2.  Rejection is required everywhere else; the same
    tile edge is guarded at K = 11 by mid_left / mid_right (conv2's own halo, 0.5 alpha / sqrt(K) = 0.05), required everywhere."""
    return not (m in ("left_halo", "right_halo") and K == 11 and mrf)


# The exception, pinned: of its 24 applicable shapes ((mutant, C, d, T), K = 11, MRF form, B = 3) exactly these seven pass `accepts`
# (max 2.93 - 3.86 x floor); the other seventeen are rejected (4.07 - 5.99).  A change of the draws, the rule or the restatement that
# widens the exception shows up here.
HALO_K11_MRF_ACCEPTED = {("right_halo", 32, 1, 267), ("left_halo", 32, 5, 285), ("right_halo", 32, 5, 287), ("left_halo", 64, 3, 257),
                         ("left_halo", 64, 3, 275), ("left_halo", 64, 3, 277), ("right_halo", 64, 5, 287)}


def _pair_case(C, K, d, B, T, mrf, last):
    x, (w1, b1), (w2, b2), res2 = V.pair_draw(C, K, d, B, T, mrf)
    kw = V.pair_kwargs(mrf, last)
    args = (x, w1, b1, d, w2, b2, V.PAIR_SLOPE)
    e = V.respair(*args, res2=res2, **kw)
    r = V.respair(*args, res2=res2, rounded=True, **kw)
    assert accepts(r, e, r)
    assert bool((V.respair(*args, res2=res2, rounded=True, mutant="tiled", **kw) == r).all())
    seen = set()
    for m in V.PAIR_MUTANTS:
        g = V.respair(*args, res2=res2, rounded=True, mutant=m, **kw)
        if not _pair_applies(m, C, K, d, B, T, mrf, last):
            assert bool((g == r).all()), (m, C, K, d, T, mrf)
        elif _pair_required(m, K, mrf):
            assert not accepts(g, e, r), (m, C, K, d, T, mrf, floor_ratios(g, e, r))
            seen.add(m)
        else:
            e_l2, f_l2, e_max, f_max = floor_ratios(g, e, r)
            assert accepts(g, e, r) == ((m, C, d, T) in HALO_K11_MRF_ACCEPTED), (m, C, d, T, e_max / f_max)
            assert e_max > 2.5 * f_max and e_l2 > 1.05 * f_l2, (m, C, d, T)          # even where accepted it is well off the rounded restatement
    return seen


@pytest.mark.parametrize("C,K,d", V.PAIR_CKD)
def test_check_rejects_residual_pair_mutants(C, K, d):
    seen = set()
    for mrf in (False, True):
        for T in V.pair_Ts(K, d):
            seen |= _pair_case(C, K, d, V.PAIR_B, T, mrf, last=V.pair_last(C))
    # (no second trip below 257 tiles: the persistent cases; 0.01 is the slope after the last, 32-channel, stage only)
    assert seen == set(V.PAIR_MUTANTS) - {"stale_tile"} - (set() if V.pair_last(C) else {"post_slope"}), seen


@pytest.mark.parametrize("C,B,T,mrf", V.PAIR_PERSISTENT)
def test_check_rejects_residual_pair_mutants_on_the_second_trip(C, B, T, mrf):
    assert B * V.cdiv(T, V.TT) > V.pair_grid(C)
    seen = _pair_case(C, 3, 1, B, T, mrf, last=V.pair_last(C))
    assert "stale_tile" in seen and (B == 1 or "prev_item" in seen)


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_post
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", V.TO1_CS + (256,))
def test_f32_bound_rejects_to1_mutants(C):
    for K in (V.TO1_KS if C <= 128 else (7,)):                 # 256 x 7: the igemm form of conv_post
        w, b = V.draw_conv(1, C, K, C + K)
        for T in V.TO1_TS:
            x = V.draw_x(V.TO1_B, T, C, T + C)
            ref = V.to1(x, w[0], b[0])
            f32 = torch.tanh(F.conv1d(x.float().transpose(1, 2), w.float(), b.float(), padding=(K - 1) // 2))[:, 0]
            assert V.f32_ratio(f32, ref) <= 1.0                 # a float32 implementation in another summation order passes
            for m in V.TO1_MUTANTS:
                assert V.f32_ratio(V.to1(x, w[0], b[0], mutant=m)["out"], ref) > 1.0, (m, C, K, T)


# ---------------------------------------------------------------------------------------------------------------------------------
# what the old comparators accepted
# ---------------------------------------------------------------------------------------------------------------------------------
def _oracle_full_config():
    """The weights and the 24-frame mel of tests/test_gpu_pipeline.py::test_vocoder_full_config_matches_oracle."""
    from oracle.hifigan import SpeechT5HifiGan as OVoc
    torch.manual_seed(11)
    ref = OVoc().eval()
    g = torch.Generator().manual_seed(12)
    sd = ref.state_dict()
    for k, v in sd.items():
        if k.endswith("weight"):
            fan_in = v[0].numel() if "upsampler" not in k else v.shape[0] * v.shape[2] / 2
            v.copy_(torch.randn(v.shape, generator=g) * (1.0 / fan_in) ** 0.5)
    ref.load_state_dict(sd)
    return ref, torch.randn(1, 24, 64, generator=g)


def test_end_to_end_bound_accepts_boundary_faults(capsys):
    """rel L2 < 4e-2 of the 24-frame waveform, the bound of test_vocoder_full_config_matches_oracle, on that test's own weights and mel,
    with one boundary fault put into the oracle.  Measured (recorded in DESIGN.md 21): stage-0 first output zeroed 0.039, last 0.042,
    stage 2 last 0.0092, stage 4 first / last 0.0037 / 0.0032, one conv2 tap dropped at every position 255 mod 256 in the first pair of a
    resblock of stage 3 / 4: 0.0039 - 0.0099."""
    ref, mel = _oracle_full_config()
    with torch.no_grad():
        want = ref(mel)

    def faulty(mod, hook):
        h = mod.register_forward_hook(hook)
        try:
            with torch.no_grad():
                return float((ref(mel) - want).norm() / want.norm())
        finally:
            h.remove()

    def zero_at(idx):
        def hook(m, i, o):
            o = o.clone()
            o[:, :, idx] = 0.0
            return o
        return hook

    def drop_last_tap(m, i, o):                                # a right halo one row short: the last tap of the tile's last output reads nothing
        K = m.weight.shape[2]
        pos = torch.arange(255, o.shape[2] - (K - 1) // 2, 256)
        o = o.clone()
        o[:, :, pos] -= torch.einsum("oc,bct->bot", m.weight[:, :, K - 1], i[0][:, :, pos + (K - 1) // 2])
        return o

    rels = {f"stage {s} output {idx} zeroed": faulty(ref.upsampler[s], zero_at(idx)) for s, idx in ((0, 0), (0, -1), (2, -1), (4, 0), (4, -1))}
    rels.update({f"stage {s} resblock {j} conv2 tap": faulty(ref.resblocks[3 * s + j].convs2[0], drop_last_tap) for s in (3, 4) for j in (0, 2)})
    with capsys.disabled():
        print("\n" + "\n".join(f"  end-to-end rel L2, {k}: {v:.4f}" for k, v in rels.items()))
    accepted = [k for k, v in rels.items() if v < 4e-2]
    assert len(accepted) >= 8 and all(v > 2e-3 for v in rels.values()), rels      # (each fault is far above fp32 noise: it is a real error)
    assert rels["stage 0 output -1 zeroed"] > 4e-2                                 # the one fault of the list that bound does reject


def test_old_close_accepts_boundary_mutants():
    """`old_close` (rtol 2e-2, atol 1.5e-2 max|want|: the comparator of tests/test_gpu_ops.py's residual-pair test) on that test's own
    draws (x = randn, w = randn / sqrt(C K), b = 0.1 randn, running sum = randn) and shapes: every tile-edge mutant passes it."""
    accepted = []
    for B, T, C, K, d, mrf in [(2, 1000, 32, 3, 1, False), (1, 777, 32, 11, 5, True), (2, 600, 64, 7, 3, True), (1, 300, 64, 11, 5, False)]:
        g = torch.Generator().manual_seed(77 + K)
        bf = lambda t: t.to(torch.bfloat16).to(F64)
        x = bf(torch.randn(B, C, T, generator=g)).transpose(1, 2).contiguous()
        w1, w2 = bf(torch.randn(C, C, K, generator=g) / math.sqrt(C * K)), bf(torch.randn(C, C, K, generator=g) / math.sqrt(C * K))
        b1, b2 = (torch.randn(C, generator=g) * 0.1).to(F64), (torch.randn(C, generator=g) * 0.1).to(F64)
        res2 = bf(torch.randn(B, C, T, generator=g)).transpose(1, 2).contiguous() if mrf else None
        kw = dict(alpha=1.0 / 3, post_slope=0.01) if mrf else {}
        e = V.respair(x, w1, b1, d, w2, b2, 0.1, res2=res2, **kw)
        r = V.respair(x, w1, b1, d, w2, b2, 0.1, res2=res2, rounded=True, **kw)
        for m in ("left_halo", "right_halo", "mid_left", "mid_right"):
            got = V.respair(x, w1, b1, d, w2, b2, 0.1, res2=res2, rounded=True, mutant=m, **kw)
            assert not bool((got == r).all())
            if old_close(got, e):
                accepted.append((m, C, K, d, mrf))
                if m.startswith("mid_"):
                    assert not accepts(got, e, r), (m, C, K, d, mrf)            # ... and the floor rule rejects the conv2-halo ones on this draw too
    assert len(accepted) >= 3, accepted
    assert {m for m, *_ in accepted} >= {"left_halo", "right_halo"}, accepted
