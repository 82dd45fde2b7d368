"""The backward (training) kernels of csrc/train.hip and csrc/attention_bwd.hip against the float64 restatements of
tests/bwd_restatement.py, per output tensor, at every template instantiation and host dispatch arm: see that helper for the
comparator (`check`: twice the L2 floor, four times the max floor of the bf16 roundings the kernel's contract has) and
tests/test_bwd_restatement_host.py for the proof that it rejects the listed mutants at exactly these shapes."""
import struct

import pytest
import torch

import bwd_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    return o


@pytest.fixture(scope="module")
def AldmError():
    from audioldm_with_lora_amd._lib import AldmError as e
    return e


def dev16(t):
    return t.to(torch.bfloat16).to(DEV)


def nhwc(t):
    return dev16(t.permute(0, 2, 3, 1).contiguous())


def nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2).to(F64)


def host(t):
    return t.float().cpu().to(F64)


# ---------------------------------------------------------------------------------------------------------------------------------
# groupnorm_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def _gn_run(ops, case, variant, pivot=False):
    B, groups, C, H, W = case
    x, dy, gm, bt, act, C1, prior = R.gn_draw(case, variant, pivot)
    exact = R.groupnorm_bwd(x, dy, gm, bt, groups, EPS, act, prior)
    rounded = R.groupnorm_bwd(x, dy, gm, bt, groups, EPS, act, prior, rounded=True)
    x1, x2 = nhwc(x[:, :C1]), (nhwc(x[:, C1:]) if C1 < C else None)
    a1 = nhwc(prior[:, :C1]) if prior is not None else None
    a2 = nhwc(prior[:, C1:]) if prior is not None and C1 < C else None
    keep = a1.clone() if a1 is not None else None
    dx, dx2 = ops.groupnorm_bwd(x1, nhwc(dy), gm.float().to(DEV), bt.float().to(DEV), groups, EPS, act, x2=x2, dx_add=a1, dx2_add=a2)
    tag = f"groupnorm_bwd {variant}{' pivot' if pivot else ''}"
    R.check(nchw(dx), exact[:, :C1], rounded[:, :C1], tag + " dx")
    if x2 is not None:
        R.check(nchw(dx2), exact[:, C1:], rounded[:, C1:], tag + " dx2")
    if a1 is not None:
        assert dx.data_ptr() != a1.data_ptr() and torch.equal(a1, keep)              # the prior gradient is not modified


@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_groupnorm_bwd_every_form(ops, case):
    for variant in R.GN_VARIANTS:
        _gn_run(ops, case, variant)


@pytest.mark.parametrize("case", R.GN_PIVOT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_groupnorm_bwd_large_mean(ops, case):
    _gn_run(ops, case, "plain", pivot=True)


def test_groupnorm_bwd_rejections(ops, AldmError):
    def call(B, groups, C, H, W):
        x = torch.zeros(B, H, W, C, dtype=torch.bfloat16, device=DEV)
        p = torch.ones(C, device=DEV)
        return ops.groupnorm_bwd(x, x.clone(), p, p, groups, EPS, 0)
    with pytest.raises(AldmError, match="register-resident"):
        call(1, 2, 8, 5, 3277)                                        # 16385 quads per strip
    with pytest.raises(AldmError, match="channels per group"):
        call(1, 2, 520, 2, 2)                                         # Cg = 260
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# layernorm_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", R.LN_CS)
def test_layernorm_bwd_widths_and_dead_rows(ops, Cc):
    for M in R.LN_MS:
        x, dy, gm, prior = R.ln_draw(M, Cc)
        for pr in (None, prior):
            exact = R.layernorm_bwd(x, dy, gm, EPS, pr)
            rounded = R.layernorm_bwd(x, dy, gm, EPS, pr, rounded=True)
            buf = dev16(pr) if pr is not None else None
            got = ops.layernorm_bwd(dev16(x), dev16(dy), gm.float().to(DEV), EPS, dx_add=buf)
            R.check(host(got), exact, rounded, f"layernorm_bwd M={M}{' add' if pr is not None else ''}")
            if buf is not None:
                assert got.data_ptr() != buf.data_ptr() and torch.equal(buf, dev16(pr))


def test_layernorm_bwd_rejects_wider_rows(ops, AldmError):
    x = torch.zeros(2, 2056, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(AldmError):
        ops.layernorm_bwd(x, x.clone(), torch.ones(2056, device=DEV))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# geglu, add, up-sampling adjoint, mse, lora_pack
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,I", R.GEGLU_CASES)
def test_geglu_fwd_bwd(ops, M, I):
    h, dout = R.geglu_draw(M, I)
    order = R.geglu_pack_order(I)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(2 * I)
    hp = dev16(h[:, order].contiguous())
    R.check(host(ops.geglu_fwd(hp)), R.geglu_fwd(h), R.geglu_fwd(h, rounded=True), "geglu_fwd")
    dh = host(ops.geglu_bwd(hp, dev16(dout)))[:, inv]
    exact, rounded = R.geglu_bwd(h, dout), R.geglu_bwd(h, dout, rounded=True)
    R.check(dh[:, :I], exact[:, :I], rounded[:, :I], "geglu_bwd dvalue")
    R.check(dh[:, I:], exact[:, I:], rounded[:, I:], "geglu_bwd dgate")


@pytest.mark.parametrize("n", R.ADD_NS)
def test_add_bf16_bit_exact(ops, n):
    g = torch.Generator().manual_seed(n)
    a = (torch.randn(n, generator=g) * 3).to(torch.bfloat16)
    b = (torch.randn(n, generator=g) * 3).to(torch.bfloat16)
    got = ops.add_bf16(a.to(DEV), b.to(DEV))
    assert torch.equal(got.cpu(), (a.float() + b.float()).bfloat16())


@pytest.mark.parametrize("B,C", R.UPS_BC)
@pytest.mark.parametrize("ih,iw,oh,ow", R.UPS_SIZES)
def test_upsample_nearest_bwd(ops, B, C, ih, iw, oh, ow):
    g = torch.Generator().manual_seed(ih + oh)
    dy = R.bf16_input(torch.randn(B, C, oh, ow, generator=g, dtype=F64))
    got = nchw(ops.upsample_nearest_bwd(nhwc(dy), ih, iw))
    R.check(got, R.upsample_nearest_bwd(dy, ih, iw), R.upsample_nearest_bwd(dy, ih, iw, rounded=True), "upsample_nearest_bwd")


@pytest.mark.parametrize("n", R.MSE_NS)
def test_mse_grad_accumulates(ops, n):
    import conftest
    g = torch.Generator().manual_seed(n)
    pred, tgt = torch.randn(n, generator=g), torch.randn(n, generator=g)
    want, d_exact = R.mse_grad(pred, tgt)
    loss = torch.full((1,), 0.25, device=DEV)                         # the kernel ADDS its loss (the trainer zeroes the slot per step)
    dp = ops.mse_grad(pred.to(DEV), tgt.to(DEV), loss)
    rel = abs(float(loss.double()) - 0.25 - want) / want
    conftest.record(rel, "mse loss rel")
    assert rel <= 1e-6, rel
    R.check(host(dp), d_exact, R.mse_grad(pred, tgt, rounded=True)[1], "mse_grad dpred")


def test_lora_pack_windows(ops):
    g = torch.Generator().manual_seed(11)
    # (rows, cols, src_ld, dst_ld, transpose, scale): plain; transposed with dst_ld > rows; src_ld > cols and dst_ld > cols, scaled;
    # 1 x 1; more than 256 elements (the block's stride loop), transposed and scaled
    shapes = [(3, 5, 5, 5, 0, 1.0), (4, 6, 6, 7, 1, 0.5), (5, 3, 8, 4, 0, 0.3), (1, 1, 1, 1, 0, 1.0), (20, 17, 17, 24, 1, 1.7)]
    src = torch.randn(2048, generator=g)
    sentinel = torch.full((4096,), -7.0, dtype=torch.bfloat16)
    want = sentinel.clone()
    src_d, dst_d = src.to(DEV), sentinel.to(DEV)
    recs, so, do = [], 3, 5
    for (rows, cols, sld, dld, tr, scale) in shapes:
        recs.append(struct.pack("<qqiiiiif", src_d.data_ptr() + 4 * so, dst_d.data_ptr() + 2 * do, rows, cols, sld, dld, tr, scale))
        win = src[so:so + rows * sld].view(rows, sld)[:, :cols]
        val = (win * torch.tensor(scale, dtype=torch.float32)).to(torch.bfloat16)      # bf16(fp32(src) * scale)
        if tr:
            want[do:do + cols * dld].view(cols, dld)[:, :rows] = val.t()
            do += cols * dld + 3
        else:
            want[do:do + rows * dld].view(rows, dld)[:, :cols] = val
            do += rows * dld + 3
        so += rows * sld + 1
    assert len(recs[0]) == 40 and so <= src.numel() and do <= sentinel.numel()
    jobs = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(DEV)
    ops.lora_pack(jobs, len(recs))
    assert torch.equal(dst_d.cpu(), want)                             # bit-equal inside the windows, the sentinel everywhere else


# ---------------------------------------------------------------------------------------------------------------------------------
# attention_train + attention_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
_ATTN_REF = {}


def _attn_ref(B, N, H, d, peaked=False):
    key = (B, N, H, d, peaked)
    if key not in _ATTN_REF:
        qkv, dO = R.attn_draw(B, N, H, d, peaked)
        _ATTN_REF[key] = (qkv, dO) + R.attention_pair(qkv, dO, B, N, H, d)
    return _ATTN_REF[key]


def _lse_err(lse, want):
    import conftest
    err = float((host(lse) - want).abs().max())
    conftest.record(err / R.LSE_BOUND, "lse err/bound")
    return err


def _attn_run(ops, B, N, H, d, peaked=False):
    qkv, dO, o_e, o_r, lse_e, g_e, g_r = _attn_ref(B, N, H, d, peaked)
    C = H * d
    dev = dev16(qkv)
    qkvT = ops.transpose_tokens(dev, B, N, 3 * C)
    out, lse = ops.attention_train(dev, qkvT, B, N, H, d)
    dqkv = ops.attention_bwd(dev, qkvT, dev16(dO), out, lse, B, N, H, d)
    tag = f"attention{' peaked' if peaked else ''}"
    R.check(host(out), o_e, o_r, tag + " out")
    got = host(dqkv)
    for i, name in enumerate(("dQ", "dK", "dV")):
        R.check(got[:, i * C:(i + 1) * C], g_e[:, i * C:(i + 1) * C], g_r[:, i * C:(i + 1) * C], f"{tag} {name}")
    err = _lse_err(lse, lse_e)
    assert err <= R.LSE_BOUND, f"lse off by {err:.3g} log2 units ({err / R.LSE_BOUND:.2f} x the bound)"


@pytest.mark.parametrize("d", R.ATTN_DS)
def test_attention_every_head_dim(ops, d):
    _attn_run(ops, 1, 100, 2, d)


@pytest.mark.parametrize("N", R.ATTN_NS)
def test_attention_every_wave_count_arm(ops, N):
    _attn_run(ops, 1, N, 2, 32)


@pytest.mark.parametrize("B,H", R.ATTN_PAIRS)
def test_attention_pair_order(ops, B, H):
    _attn_run(ops, B, 200, H, 32)


@pytest.mark.parametrize("N,d", R.ATTN_PEAKED)
def test_attention_peaked_softmax(ops, N, d):
    _attn_run(ops, 1, N, 2, d, peaked=True)


@pytest.mark.parametrize("B,H,N,d", R.ATTN_FWD_ARMS)
def test_attention_forward_pair_count_arm(ops, B, H, N, d):
    """The lse form's last threshold: 8 waves with the keys split below ceil(N / 256) * H * B = 256, one wave per query block from there."""
    qkv, _ = R.attn_draw(B, N, H, d)
    o_e, lse_e = R.attention_fwd(qkv, B, N, H, d)
    o_r, _ = R.attention_fwd(qkv, B, N, H, d, rounded=True)
    dev = dev16(qkv)
    out, lse = ops.attention_train(dev, ops.transpose_tokens(dev, B, N, 3 * H * d), B, N, H, d)
    R.check(host(out), o_e, o_r, "attention out")
    err = _lse_err(lse, lse_e)
    assert err <= R.LSE_BOUND, f"lse off by {err:.3g} log2 units ({err / R.LSE_BOUND:.2f} x the bound)"


def test_attention_rejects_head_dim_88(ops, AldmError):
    B, N, H, d = 1, 16, 2, 88
    C = H * d
    qkv = torch.zeros(B * N, 3 * C, dtype=torch.bfloat16, device=DEV)
    qkvT = torch.zeros(B, 3 * C, N, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(AldmError, match="head dim"):
        ops.attention_train(qkv, qkvT, B, N, H, d)
    o = torch.zeros(B * N, C, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(AldmError, match="head dim"):
        ops.attention_bwd(qkv, qkvT, o, o, torch.zeros(B, H, N, device=DEV), B, N, H, d, dOT=torch.zeros(B, C, N, dtype=torch.bfloat16, device=DEV))
    torch.cuda.synchronize()


@pytest.mark.parametrize("N", [100, 37, 191])
def test_attention_bwd_token_major_dO_and_padding_contract(ops, N):
    """dOT handed over (the trainer's path: the out-projection's dX launch stores it) == dOT made inside; and whatever sits in the
    token-major copies' padding columns [N, Npad) never reaches a result ("tokens past N must read as zeros")."""
    B, H, d = 1, 2, 32
    C = H * d
    qkv, dO = _attn_ref(B, N, H, d)[:2]
    dev, dOd = dev16(qkv), dev16(dO)
    qkvT = ops.transpose_tokens(dev, B, N, 3 * C)
    out, lse = ops.attention_train(dev, qkvT, B, N, H, d)
    clean = ops.attention_bwd(dev, qkvT, dOd, out, lse, B, N, H, d)
    dOT = ops.transpose_tokens(dOd, B, N, C)
    assert torch.equal(ops.attention_bwd(dev, qkvT, dOd, out, lse, B, N, H, d, dOT=dOT), clean)
    npad = qkvT.shape[2]
    if npad > N:
        dirtyT, dirty_dOT = qkvT.clone(), dOT.clone()              # copies: the forward above saw the clean ones
        dirtyT[:, :, N:] = float("nan")
        dirty_dOT[:, :, N:] = float("nan")
        got = ops.attention_bwd(dev, dirtyT, dOd, out, lse, B, N, H, d, dOT=dirty_dOT)
        assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, clean)


# ---------------------------------------------------------------------------------------------------------------------------------
# one LoRA site: LoraSite + t_lora_linear + Tape
# ---------------------------------------------------------------------------------------------------------------------------------
class _Adapters(torch.nn.Module):
    """The smallest module FlatLora accepts: parameters whose names contain "lora_"."""

    def __init__(self, parts):
        super().__init__()
        for i, (_, _, A, Bm, _) in enumerate(parts):
            self.register_parameter(f"lora_A{i}", torch.nn.Parameter(A.clone()))
            self.register_parameter(f"lora_B{i}", torch.nn.Parameter(Bm.clone()))


@pytest.mark.parametrize("batched", [True, False], ids=["TnBatch", "tn_small"])
@pytest.mark.parametrize("name", sorted(R.SITE_CASES))
def test_lora_site(ops, monkeypatch, name, batched):
    import conftest
    from audioldm_with_lora_amd import training as tr
    M, K, N, ranks, with_res = R.SITE_CASES[name]
    Bq, Nq = 2, M // 2
    x, W, bias, parts, dy, rs = R.site_draw(M, K, N, ranks, res=with_res)
    exact = R.lora_site(x, W, bias, parts, dy, res=rs)
    rounded = R.lora_site(x, W, bias, parts, dy, res=rs, rounded=True)

    mod = _Adapters(parts)
    flat = tr.FlatLora(mod, DEV)
    site_parts = [(row0, nrows, getattr(mod, f"lora_A{i}"), getattr(mod, f"lora_B{i}"), s) for i, (row0, nrows, _, _, s) in enumerate(parts)]
    site = tr.LoraSite(W.float().to(DEV), bias.float().to(DEV), site_parts, flat, DEV)
    assert site.Rp == (32 if sum(ranks) <= 32 else 64)
    jobs = torch.frombuffer(bytearray(b"".join(struct.pack("<qqiiiiif", *j) for j in site.jobs)), dtype=torch.uint8).to(DEV)
    ops.lora_pack(jobs, len(site.jobs))

    seen = []
    if not batched:
        real = ops.tn_small
        monkeypatch.setattr(ops, "tn_small", lambda P, Q, rows, Qc=None: (seen.append((P, Q)), real(P, Q, rows, Qc=Qc))[1])
    tape = tr.Tape(tn=ops.TnBatch(8, DEV) if batched else None)
    xv = tr.Var(dev16(x), True)
    xv.want_T = (Bq, Nq)                                              # the dX launch also leaves the gradient token-major
    res = tr.Var(dev16(rs), True) if with_res else None
    y = tr.t_lora_linear(tape, xv, site, res=res, tok=None if with_res else (Bq, Nq))
    R.check(host(y.t), exact["y"], rounded["y"], "lora y")
    npad = (Nq + 7) // 8 * 8
    if not with_res:
        wantT = torch.zeros(Bq, N, npad, dtype=torch.bfloat16, device=DEV)
        wantT[:, :, :Nq] = y.t.view(Bq, Nq, N).transpose(1, 2)
        assert torch.equal(y.tT, wantT)
    y.g = dev16(dy)
    tape.backward()
    if batched:
        assert len(tape.tn.keep) == 6
        seen = [(tape.tn.keep[0], tape.tn.keep[1]), (tape.tn.keep[3], tape.tn.keep[4])]
        tape.tn.launch()
    (T, Qdy), (U, Qx) = seen
    assert Qdy.data_ptr() == y.g.data_ptr() and Qx.data_ptr() == xv.t.data_ptr()
    if with_res:
        assert res.g is y.g
    R.check(host(xv.g), exact["dx"], rounded["dx"], "lora dX")
    wantT = torch.zeros(Bq, K, npad, dtype=torch.bfloat16, device=DEV)
    wantT[:, :, :Nq] = xv.g.view(Bq, Nq, K).transpose(1, 2)
    assert torch.equal(xv.gT, wantT)

    col = 0
    for i, (row0, nrows, A, Bm, s) in enumerate(parts):
        r = A.shape[0]
        Tp, Up = host(T)[:, col:col + r], host(U)[:, col:col + r]
        R.check(Tp, exact["T"][i], rounded["T"][i], f"lora T part {i}")
        R.check(Up, exact["U"][i], rounded["U"][i], f"lora U part {i}")
        dyp = dy[:, row0:row0 + nrows]
        # dA = U^T x and dB = s dy^T T are fp32 products of the bf16 operands the kernels themselves stored
        for what, got, (want, mag), unit in (
                ("dA", getattr(mod, f"lora_A{i}").grad, R.tn_exact(Up, x), R.tn_unit(Up, x)),
                ("dB", getattr(mod, f"lora_B{i}").grad.t(), tuple(s * v for v in R.tn_exact(Tp, dyp)), R.tn_unit(Tp, dyp))):
            err = ((host(got) - want).abs() / mag).max()
            conftest.record(float(err) / unit, f"lora {what} part {i} err/fp32 unit")
            assert float(err) <= R.TN_MARGIN * unit, (what, i, float(err), unit)
        col += r
    torch.cuda.synchronize()
    assert float(flat.grads[flat.n:].abs().max()) == 0.0              # nothing scattered past the parameters (the loss slot)
