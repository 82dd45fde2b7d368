"""The vocoder's kernels (vocoder.py, csrc/hifigan.hip and the igemm launches they drive) against the float64 restatements of
tests/vocoder_restatement.py under the floor rule of tests/bwd_restatement.py (`rel L2 <= 2 x floor`, `max <= 4 x floor`, per output
tensor), at the phase, tile and sequence edges: the transposed convolution through run_conv_transpose1d into NaN-filled buffers on
every tile and both epilogue forms, aldm_hifigan_respair at every (C, K, d) of the real config around the 256-sample tile and on the
second trip of its persistent loop, aldm_conv1d_to1 up to its > 48 KiB LDS arm, the unfused igemm chain, and the whole model one stage
at a time.  tests/test_vocoder_restatement_host.py proves on the CPU that the rule rejects the listed mutants at these shapes.
Every case asserts the arithmetic that puts it in its arm."""
import pytest
import torch

import vocoder_restatement as V
from bwd_restatement import F64, check

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE = 0.1


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    return o


@pytest.fixture(scope="module")
def voc():
    from audioldm_with_lora_amd import vocoder
    return vocoder


WORST = {}


@pytest.fixture(autouse=True)
def _record_worst():
    """A test here makes hundreds of comparisons of a few kinds of output (`what`): the log gets one line per kind and test, the largest
    ratio to the floor (1.000 = the kernel is the rounded restatement) or to the fp32 bound -- the rows of DESIGN.md 21's tables."""
    WORST.clear()
    yield
    import conftest
    for what, v in sorted(WORST.items()):
        conftest.record(v, what)


def _note(v, what):
    WORST[what] = max(WORST.get(what, 0.0), v)


def chk(got, exact, rounded, what, where=""):
    """bwd_restatement.check, its two ratios pooled per `what` (above) instead of one log line per call."""
    try:
        check(got, exact, rounded, what, record=_note)
    except AssertionError as err:
        raise AssertionError(f"{where}: {err}") from None


def chk_f32(got, ref, what, where="", tanh=True):
    assert bool(torch.isfinite(got).all()), f"{what} {where}: non-finite values"
    ratio = V.f32_ratio(got, ref, tanh)
    _note(ratio, what + " err/bound")
    assert ratio <= 1.0, f"{what} {where}: error {ratio:.3g} x the fp32 bound"


def dev(t):
    """[B, T, C] float64 (bf16-representable) -> [B, 1, T, C] bf16 on the device."""
    return t.to(torch.bfloat16).unsqueeze(1).contiguous().to(DEV)


def host(t, c=None):
    """[B, 1, T, Cpad] on the device -> [B, T, c] float64; the padded channels must hold exact zeros."""
    t = t.detach().to("cpu").to(F64)[:, 0]
    if c is not None and c < t.shape[2]:
        assert bool((t[:, :, c:] == 0).all()), "padded output channels are not zero"
        t = t[:, :, :c]
    return t


def nan_like(B, T, C):
    return torch.full((B, 1, T, C), float("nan"), dtype=torch.bfloat16, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# transposed convolution
# ---------------------------------------------------------------------------------------------------------------------------------
def _igemm_tiles(cin):
    """Every non-halo tile aldm_igemm accepts for a launch of the transposed convolution (no LoRA, no V^T): ops.conv hands tile= straight
    to the library, whose selection refuses only by path -- 1, 2, 3, 4 (reg_staged rows of IGEMM_TILES) take any input; the 8-wave tiles
    6, 9, 10, 11 and the wave-specialised 12, 13, 14 (select_ring, igemm_select.hip) need the LDS-DMA path,
    Cin % 64 == 0.  No row has a condition on M, N or the number of K-tiles: 9 and 12 are the 256-row tiles."""
    return [1, 2, 3, 4] + ([6, 9, 10, 11, 12, 13, 14] if cin % 64 == 0 else [])


@pytest.mark.parametrize("kup", V.CT_KUP, ids=lambda t: "k%d_u%d_p%d" % t)
@pytest.mark.parametrize("ch", V.CT_CH, ids=lambda t: "c%d_%d" % t)
def test_transposed_conv_every_phase_edge(ops, voc, monkeypatch, kup, ch):
    (k, u, p), (ci, co) = kup, ch
    w, b = V.draw_convt(ci, co, k, u, k * u + ci)
    P = voc.pack_conv_transpose1d(w.float().to(DEV), b.float().to(DEV), u, p)
    N = P.phases[0].N
    assert N == max(8, co) and (ci % 64 == 0) == (ci >= 64)          # Cout 4 is padded to 8; Cin 128 / 64 ride the LDS-DMA path, 32 / 8 the generic gather
    assert N <= 64                                                   # N below the 128-wide tiles' width, and below 64 for all but the largest config
    force, trace, real = {}, [], ops.conv
    monkeypatch.setattr(ops, "conv", lambda *a, **kw: real(*a, **{**kw, **force}))
    monkeypatch.setattr(ops, "EPI_TRACE", trace)

    def run(xd, L, copy, **f):
        force.clear()
        force.update(f)
        del trace[:]
        y, y2 = nan_like(V.CT_B, L, N), nan_like(V.CT_B, L, N)
        if copy:
            voc.run_conv_transpose1d(P, xd, L, post_act=ops.ACT_LRELU, post_slope=SLOPE, out2=True, out=y, out2_buf=y2)
        else:
            assert voc.run_conv_transpose1d(P, xd, L, out=y) is y
        return y, (y2 if copy else None), list(trace)

    Ts = V.ct_Ts(k, u, p)
    assert len(Ts) == len(V.CT_TS_BASE) + len(V.CT_TILE_HEIGHTS)
    direct_seen = False
    for T in Ts:
        x = V.draw_x(V.CT_B, T, ci, T + k)
        L = V.ct_out_len(T, k, u, p)
        plan = voc.transpose_phase_plan(k, u, p, L)
        e, e2 = V.conv_transpose1d(x, w, b, u, p, L, copy_slope=SLOPE)
        r, r2 = V.conv_transpose1d(x, w, b, u, p, L, copy_slope=SLOPE, rounded=True)
        xd = dev(x)
        for tile in [0] + _igemm_tiles(ci):
            where = f"T={T} tile={tile}"
            f = dict(tile=tile) if tile else {}
            # bare (the fused stages' form) with the epilogue forced to the LDS walk, then as dispatched, then forced direct where every launch can take it
            y_lds, _, tr = run(xd, L, False, epi=ops._lib.EPI_LDS, **f)
            assert tr == [0] * len(plan), tr
            chk(host(y_lds, co), e, r, "convT bare", where)
            y, _, tr = run(xd, L, False, **f)
            assert len(tr) == len(plan)
            assert torch.equal(y.view(torch.int16), y_lds.view(torch.int16)), f"{where}: dispatched epilogue differs from the LDS walk"
            if all(tr):
                direct_seen = True
                y_dir, _, tr2 = run(xd, L, False, epi=ops._lib.EPI_DIRECT, **f)
                assert tr2 == [1] * len(plan)
                assert torch.equal(y_dir.view(torch.int16), y_lds.view(torch.int16)), f"{where}: direct epilogue differs from the LDS walk"
            # out2 + post_act: the LDS-walk epilogue only
            y, y2, tr = run(xd, L, True, **f)
            assert tr == [0] * len(plan), tr
            assert torch.equal(y.view(torch.int16), y_lds.view(torch.int16)), f"{where}: the stream differs between the bare and the out2 form"
            chk(host(y2, co), e2, r2, "convT activated copy", where)
    for bm in V.CT_TILE_HEIGHTS:                                     # the ragged arm: some phase's B * nq rows end inside a tile beyond the first
        Tr = V.ct_ragged_T(bm, k, u, p)
        assert Tr in Ts and any(V.CT_B * nq > bm and (V.CT_B * nq) % bm for _, _, _, nq in voc.transpose_phase_plan(k, u, p, V.ct_out_len(Tr, k, u, p)))
    assert direct_seen == (ci % 64 == 0)                             # the register-direct epilogue exists on the LDS-DMA path only, and was reached there


# ---------------------------------------------------------------------------------------------------------------------------------
# aldm_hifigan_respair
# ---------------------------------------------------------------------------------------------------------------------------------
def _pair_launch(ops, x, c1, c2, d, res2, mrf, last):
    kw = dict(alpha=1.0 / 3.0, res2=res2, post_act=ops.ACT_LRELU, post_slope=(0.01 if last else SLOPE)) if mrf else {}
    return ops.hifigan_respair(x, c1, c2, d, SLOPE, **kw)


def _pair_refs(C, K, d, B, T, mrf):
    x, (w1, b1), (w2, b2), res2 = V.pair_draw(C, K, d, B, T, mrf)
    kw = V.pair_kwargs(mrf, V.pair_last(C))
    e = V.respair(x, w1, b1, d, w2, b2, SLOPE, res2=res2, **kw)
    r = V.respair(x, w1, b1, d, w2, b2, SLOPE, res2=res2, rounded=True, **kw)
    return x, (w1, b1), (w2, b2), res2, e, r


def _pack(ops, wb):
    return ops.pack_conv(wb[0].float().unsqueeze(2).to(DEV), wb[1].float().to(DEV))


@pytest.mark.parametrize("C,K,d", V.PAIR_CKD)
def test_respair_every_config_around_the_tile(ops, C, K, d):
    h = V.pair_halo(K, d)
    Ts = V.pair_Ts(K, d)
    assert Ts == (1, 5, 255, 256, 257, 256 + h - 1, 256 + h + 1) and h == (K - 1) // 2 * (1 + d)
    for mrf in (False, True):
        for T in Ts:
            assert V.PAIR_B * V.cdiv(T, 256) <= V.pair_grid(C)       # one trip of the tile loop
            x, wb1, wb2, res2, e, r = _pair_refs(C, K, d, V.PAIR_B, T, mrf)
            c1, c2 = _pack(ops, wb1), _pack(ops, wb2)
            xd = dev(x)
            assert ops.hifigan_respair_ok(xd, c1, c2, d)
            got = _pair_launch(ops, xd, c1, c2, d, dev(res2) if mrf else None, mrf, V.pair_last(C))
            chk(host(got), e, r, "respair MRF form" if mrf else "respair", f"T={T}")


@pytest.mark.parametrize("C,B,T,mrf", V.PAIR_PERSISTENT)
def test_respair_second_trip_of_the_persistent_loop(ops, C, B, T, mrf):
    K, d = 3, 1
    tpi, grid = V.cdiv(T, 256), V.pair_grid(C)
    assert grid == (256 if C == 64 else 512) and grid < B * tpi <= grid + 5      # a few workgroups walk a second tile
    assert B == 1 or (grid // tpi >= 1 and grid % tpi != 0)                       # ... which belongs to another item, at another offset, than their first
    x, wb1, wb2, res2, e, r = _pair_refs(C, K, d, B, T, mrf)
    c1, c2 = _pack(ops, wb1), _pack(ops, wb2)
    xd, rd = dev(x), (dev(res2) if mrf else None)
    got = _pair_launch(ops, xd, c1, c2, d, rd, mrf, V.pair_last(C))
    chk(host(got), e, r, "respair second trip")
    # bit for bit the same values from one-item launches short enough for one trip: whole items where they fit under the grid, else two
    # halves of the item that overlap by the halo (compared away from the cut: a cut end is zero-padded like a sequence end)
    h = V.pair_halo(K, d)
    cut = (tpi // 2) * 256
    for b in range(B):
        spans = [(0, T, 0, T)] if tpi <= grid else [(0, cut + h, 0, cut), (cut - h, T, cut, T)]
        for lo, hi, keep_lo, keep_hi in spans:
            assert V.cdiv(hi - lo, 256) <= grid
            part = _pair_launch(ops, xd[b:b + 1, :, lo:hi].contiguous(), c1, c2, d, rd[b:b + 1, :, lo:hi].contiguous() if mrf else None, mrf, V.pair_last(C))
            assert torch.equal(part[0, 0, keep_lo - lo:keep_hi - lo].view(torch.int16), got[b, 0, keep_lo:keep_hi].view(torch.int16)), (b, lo, hi)


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_post: aldm_conv1d_to1 and the igemm form
# ---------------------------------------------------------------------------------------------------------------------------------
def _pack_to1(ops, w, b):
    """[1, C, K] -> the [8, C, 1, K] pack forward_nhwc builds (pack_conv1d pads the output channels to 8)."""
    C, K = w.shape[1], w.shape[2]
    return ops.pack_conv(torch.cat([w.float(), torch.zeros(7, C, K)]).unsqueeze(2).to(DEV), torch.cat([b.float(), torch.zeros(7)]).to(DEV))


@pytest.mark.parametrize("C", V.TO1_CS)
def test_conv1d_to1_every_arm(ops, C):
    for K in V.TO1_KS:
        lds = (256 + K - 1) * (2 * C + 16) + 2 * K * C             # aldm_conv1d_to1: above 48 KiB the launch raises the kernel's LDS limit first
        assert (lds > 48 * 1024) == (C == 128)                         # 69888 .. 77280 bytes at C = 128
        w, b = V.draw_conv(1, C, K, C + K)
        pw = _pack_to1(ops, w, b)
        for T in V.TO1_TS:
            x = V.draw_x(V.TO1_B, T, C, T + C)
            ref = V.to1(x, w[0], b[0])
            chk_f32(ops.conv1d_to1(dev(x), pw, act=ops.ACT_TANH), ref, "conv1d_to1", f"K={K} T={T}")
            ref = V.to1(x, w[0], b[0], tanh=False)
            chk_f32(ops.conv1d_to1(dev(x), pw, act=ops.ACT_NONE), ref, "conv1d_to1 no tanh", f"K={K} T={T}", tanh=False)


@pytest.mark.parametrize("C,K", [(136, 7), (64, 6), (64, 17)])
def test_conv1d_to1_rejects_what_it_cannot_run(ops, C, K):
    w, b = V.draw_conv(1, C, K, 1)
    with pytest.raises(ops._lib.AldmError):
        ops.conv1d_to1(dev(V.draw_x(1, 9, C, 2)), _pack_to1(ops, w, b), act=ops.ACT_TANH)


@pytest.mark.parametrize("T", V.TO1_TS)
def test_conv_post_igemm_form(ops, T):
    """forward_nhwc's fall-back for a stream conv1d_to1 does not take (C > 128): out_act = TANH, fp32 output, N = 1 padded to 8."""
    C, K = 256, 7
    assert not (C <= 128)
    w, b = V.draw_conv(1, C, K, 5)
    x = V.draw_x(V.TO1_B, T, C, T)
    got = ops.conv(dev(x), _pack_to1(ops, w, b), pad=(0, (K - 1) // 2), out_act=ops.ACT_TANH, out_f32=True)
    assert got.dtype == torch.float32 and got.shape == (V.TO1_B, 1, T, 8)
    assert bool((got[:, 0, :, 1:] == 0).all())                     # tanh(0 + 0) of the seven padded columns
    chk_f32(got[:, 0, :, 0], V.to1(x, w[0], b[0]), "conv_post igemm form", f"T={T}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the unfused chain (igemm): conv1 with dilation and out_act, conv2 with res / out2 / post_act, the MRF form
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", [(C, K) for C in (128, 16) for K in (3, 7, 11)])
def test_unfused_chain_launches(ops, C, K):
    B = 3
    (w1, b1), (w2, b2) = V.draw_conv(C, C, K, 7 * K + C), V.draw_conv(C, C, K, 7 * K + C + 3)
    c1, c2 = _pack(ops, (w1, b1)), _pack(ops, (w2, b2))
    for T in (130, 777):
        ra, t, r, acc = (V.draw_x(B, T, C, 10 * K + i + T) for i in range(4))
        rad, td, rd, accd = dev(ra), dev(t), dev(r), dev(acc)
        e2, e2a = V.conv1d(t, w2, b2, 1, res=r, post_act=SLOPE, out2=True)
        r2, r2a = V.conv1d(t, w2, b2, 1, res=r, post_act=SLOPE, out2=True, rounded=True)
        for d in (1, 3, 5):
            tiles = [0]
            if C == 128:                                           # ops.conv's conv1d halo rule: the wave-specialised halo tiles where the run fits their LDS rows
                tiles += ops.halo_candidates(ops.igemm_plan.geometry((B, 1, T, C), c1, pad=(0, (K * d - d) // 2), dil=(1, d)))
                assert tiles == [0, 15, 16]
            else:
                assert C % 64 != 0                                 # the generic gather: no halo tile, no LDS-DMA
            e1 = V.conv1d(ra, w1, b1, d, out_act=SLOPE)
            r1 = V.conv1d(ra, w1, b1, d, out_act=SLOPE, rounded=True)
            for tile in tiles:
                where = f"T={T} d={d} tile={tile}"
                got = ops.conv(rad, c1, pad=(0, (K * d - d) // 2), dil=(1, d), out_act=ops.ACT_LRELU, out_slope=SLOPE, tile=tile)
                chk(host(got), e1, r1, "chain conv1", where)
                if d > 1:
                    continue                                       # conv2 has dilation 1: once per (T, tile)
                o2 = nan_like(B, T, C)
                got = ops.conv(td, c2, pad=(0, (K - 1) // 2), res=rd, out2=o2, post_act=ops.ACT_LRELU, post_slope=SLOPE, tile=tile)
                chk(host(got), e2, r2, "chain conv2 stream", where)
                chk(host(o2), e2a, r2a, "chain conv2 activated copy", where)
                for post in (SLOPE, 0.01):
                    kw = dict(res=r, alpha=1.0 / 3.0, res2=acc, post_act=post)
                    got = ops.conv(td, c2, pad=(0, (K - 1) // 2), res=rd, alpha=1.0 / 3.0, res2=accd, post_act=ops.ACT_LRELU, post_slope=post, tile=tile)
                    chk(host(got), V.conv1d(t, w2, b2, 1, **kw), V.conv1d(t, w2, b2, 1, rounded=True, **kw), "chain MRF form", where + f" slope={post}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole model, one stage deep at a time
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(voc, tiny, seed):
    from oracle import configs
    torch.manual_seed(seed)
    m = voc.SpeechT5HifiGan(**(configs.tiny_vocoder() if tiny else {}))
    g = torch.Generator().manual_seed(seed + 1)
    sd = m.state_dict()
    for k, v in sd.items():                                          # O(1) activations through the stack
        if k.endswith("weight"):
            fan_in = v[0].numel() if "upsampler" not in k else v.shape[0] * v.shape[2] / 2
            v.copy_(torch.randn(v.shape, generator=g) * (1.0 / fan_in) ** 0.5)
    m.load_state_dict(sd)
    return m


def _stage_prm(m, i):
    wq = lambda t: t.detach().to(torch.bfloat16).to(F64)            # the packs hold bf16 weights and fp32 biases
    bq = lambda t: t.detach().to(F64)
    up, nk = m.upsampler[i], m.num_kernels
    blocks = [(rb.k, rb.dil, [(wq(a.weight), bq(a.bias), wq(c.weight), bq(c.bias)) for a, c in zip(rb.convs1, rb.convs2)])
              for rb in m.resblocks[i * nk:(i + 1) * nk]]
    return dict(up=(wq(up.weight), bq(up.bias), up.stride[0], up.padding[0]), blocks=blocks)


@pytest.mark.parametrize("tiny,T", [(False, 7), (True, 12)], ids=["full_T7", "tiny_T12"])
def test_whole_model_stage_by_stage(ops, voc, tiny, T):
    B = 2
    m = _model(voc, tiny, 31 + T)
    prms = [_stage_prm(m, i) for i in range(len(m.upsampler))]
    pre = (m.conv_pre.weight.detach().to(torch.bfloat16).to(F64), m.conv_pre.bias.detach().to(F64))
    post = (m.conv_post.weight.detach().to(torch.bfloat16).to(F64), m.conv_post.bias.detach().to(F64))
    m = m.to(DEV)
    mel = V.draw_x(B, T, 64, 5)
    meld = dev(mel)
    taps = []
    wav = m.forward_nhwc(meld, taps=taps)
    assert torch.equal(wav, m.forward_nhwc(meld))                    # the tap changes nothing
    assert [s for s, _, _ in taps] == list(range(5)) and wav.shape == (B, 160 * T + 32) and wav.dtype == torch.float32
    P = m.plan()
    a_dev = ops.conv(meld, P.pre, pad=(0, 3), out_act=ops.ACT_LRELU, out_slope=SLOPE)     # forward_nhwc's own first launch, again
    chk(host(a_dev), V.conv1d(mel, *pre, 1, out_act=SLOPE), V.conv1d(mel, *pre, 1, out_act=SLOPE, rounded=True), "conv_pre")
    fused_stages = []
    for (i, h, a), prm in zip(taps, prms):
        c = prm["up"][0].shape[1]
        fused = all(ops.hifigan_respair_ok(torch.empty(0, 1, 0, h.shape[3]), rb.c1[q], rb.c2[q], rb.dil[q])
                    for rb in P.res[3 * i:3 * i + 3] for q in range(3))
        fused_stages.append(fused)
        a_in = host(a_dev, prm["up"][0].shape[0])                    # the kernel's own previous activation, bit for bit
        he, ae = V.stage(a_in, prm, SLOPE, i == 4, fused)
        hr, ar = V.stage(a_in, prm, SLOPE, i == 4, fused, rounded=True)
        chk(host(h, c), he, hr, f"stage {i} up-sampler ({'fused' if fused else 'igemm'})")
        chk(host(a, c), ae, ar, f"stage {i} activation ({'fused' if fused else 'igemm'})")
        a_dev = a
    assert fused_stages == ([True, True, False, False, False] if tiny else [False, False, False, True, True])
    c = post[0].shape[1]
    assert a_dev.shape[3] == max(8, c) <= 128                        # conv1d_to1 takes both configs' last stream
    chk_f32(wav, V.to1(host(a_dev, c), post[0][0], post[1][0]), "waveform")
