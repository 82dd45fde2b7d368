"""GPU: multi-adapter LoRA -- the per-sample gate on the LoRA side channel of the four kernel families, and the routing built on it.

Operator level (through the C-ABI), for every family, with 252 rows per sample so that a tile straddles two samples:
  1. a gate of ones == the ungated launch, torch.equal (multiplying by 1.0f is exact);
  2. row independence, torch.equal: sample b of a mixed batch == sample b of a batch in which every sample carries b's gates;
  3. against fp32 torch  x @ (W + sum_a g_a s_a B_a A_a)^T  on the bf16-rounded operands, at the tolerance of the family's existing
     LoRA case in tests/test_gpu_ops.py / tests/test_gpu_pgemm.py (quoted at each call).
UNet / engine / pipeline level: the merged fp32 oracle of tests/multi_adapter_restatement.py, bounds of tests/test_gpu_unet.py."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
GATES4 = [[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [0.5, 0.5]]          # a, b, base, 50/50 blend


def bf(x):
    return x.to(torch.bfloat16).float()


def dv(t):
    return t.to(torch.bfloat16).to(DEV)


def close(got, want, rtol=1.2e-2, atol=None):
    """the bound of tests/test_gpu_ops.py / tests/test_gpu_pgemm.py; records the measured relative L2 error"""
    import conftest
    want = want.float()
    got = got.float().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    conftest.record(float((got - want).norm() / want.norm()))
    if atol is None:
        atol = 8e-3 * float(want.abs().max()) + 1e-6
    err = (got - want).abs()
    bad = ~(err <= atol + rtol * want.abs())
    assert not bad.any(), f"max err {float(err.max()):.4g} (ref max {float(want.abs().max()):.4g}), {int(bad.sum())} bad"


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    return o


@pytest.fixture()
def labels(ops):
    ops.PROFILE = []
    yield ops.PROFILE
    ops.PROFILE = None


def table(gates, widths, rp=32):
    """gate table [samples][rp]: adapter i owns columns sum(widths[:i]) .. + widths[i]"""
    t = torch.zeros(len(gates), rp)
    c = 0
    for i, w in enumerate(widths):
        for b, g in enumerate(gates):
            t[b, c:c + w] = g[i]
        c += w
    return t.to(DEV)


def three_checks(run, gates, widths, check):
    """run(table or None) -> [samples, ...] device tensor; check(got, gates) compares with fp32 torch"""
    nb = len(gates)
    ungated = run(None)
    ones = run(table([[1.0] * len(widths)] * nb, widths))
    assert torch.equal(ones, ungated), "a gate of ones must reproduce the ungated launch bit for bit"
    mixed = run(table(gates, widths))
    for b in range(nb):
        same = run(table([gates[b]] * nb, widths))
        assert torch.equal(same[b], mixed[b]), f"sample {b} depends on another sample's gates"
    assert not torch.equal(mixed, ungated)
    check(mixed, gates)
    check(ungated, [[1.0] * len(widths)] * nb)


def _two_adapters(g, N, K, r, std_a=None):
    return [(bf(torch.randn(r, K, generator=g) * (std_a or 1.0 / r)), bf(torch.randn(N, r, generator=g) * 0.05), 2.0) for _ in range(2)]


@pytest.mark.parametrize("K,N,r,tile,splits,family", [
    (96, 96, 4, 0, None, "generic"),          # K % 64 != 0: the register-staged kernel
    (256, 256, 4, 1, None, "lds-dma"),        # 128x128 tile, LDS-DMA ring
    (640, 640, 4, 2, 2, "split-k"),           # 64x64 tile, split-K: every split gates its partial T
    (384, 384, 8, 3, None, "lds-dma"),        # 128x64 tile
])
def test_igemm_gate(ops, labels, K, N, r, tile, splits, family):
    B, rows = 4, 252                                                  # 1008 rows: tiles of 64 / 128 rows straddle the samples
    M = B * rows
    g = torch.Generator().manual_seed(41)
    x = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g)
    res = bf(torch.randn(M, N, generator=g))
    ads = _two_adapters(g, N, K, r)
    pw = ops.pack_linear(w.to(DEV), b.to(DEV))
    ops.attach_lora(pw, [(0, N, A.to(DEV), Bm.to(DEV), s, n) for n, (A, Bm, s) in zip("ab", ads)], {"a": (0, r), "b": (r, r)})
    assert pw.Rp == 32 and pw.ranks_used == 2 * r
    kw = dict(tile=tile) if tile else {}
    if splits:
        kw["splits"] = splits

    def run(t):
        if tile == 0:                                                 # (K = 96 is no pgemm shape: tile 0 stays on aldm_igemm)
            return ops.linear(dv(x), pw, res=dv(res), lora_gate=t, **kw).view(B, rows, N)
        return ops.linear(dv(x), pw, res=dv(res), lora_gate=t, **kw).view(B, rows, N)

    def check(got, gates):
        want = x @ w.t() + b + res
        gr = torch.tensor(gates).repeat_interleave(rows, dim=0)      # [M, 2]
        for i, (A, Bm, s) in enumerate(ads):
            want = want + gr[:, i:i + 1] * (s * (x @ A.t()) @ Bm.t())
        close(got.reshape(M, N), want)                                 # test_linear_lora_fused: close(y, want), defaults

    three_checks(run, GATES4, [r, r], check)
    assert labels and not any(l[0].startswith("pgemm_") for l in labels), [l[0] for l in labels]


def test_igemm_gate_with_folded_layernorm(ops, labels):
    """T'' = t - mean sA + cA / rstd, THEN the gate: the epilogue's rstd is linear in it"""
    B, rows, Cc, N, r = 4, 252, 256, 768, 4
    M = B * rows
    g = torch.Generator().manual_seed(42)
    x = bf(torch.randn(M, Cc, generator=g) * 1.7 + 0.4)
    w = bf(torch.randn(N, Cc, generator=g) / math.sqrt(Cc))
    b = torch.randn(N, generator=g)
    gm, bt = torch.randn(Cc, generator=g) * 0.3 + 1, torch.randn(Cc, generator=g) * 0.2
    xn = F.layer_norm(x, (Cc,), gm, bt, 1e-5)
    ads = _two_adapters(g, N, Cc, r)
    pw = ops.pack_linear_ln(w.to(DEV), b.to(DEV), gm.to(DEV), bt.to(DEV))
    ops.attach_lora(pw, [(0, N, A.to(DEV), Bm.to(DEV), s, n) for n, (A, Bm, s) in zip("ab", ads)], {"a": (0, r), "b": (r, r)})

    def run(t):
        return ops.linear(dv(x), pw, lora_gate=t, tile=2).view(B, rows, N)       # tile=2: the implicit-GEMM kernel, not pgemm

    def check(got, gates):
        want = xn @ w.t() + b
        gr = torch.tensor(gates).repeat_interleave(rows, dim=0)
        for i, (A, Bm, s) in enumerate(ads):
            want = want + gr[:, i:i + 1] * (s * (xn @ A.t()) @ Bm.t())
        close(got.reshape(M, N), want, rtol=2e-2)                      # test_layernorm_folded_into_gemm: rtol=2e-2

    three_checks(run, GATES4, [r, r], check)
    assert labels and not any(l[0].startswith("pgemm_") for l in labels), [l[0] for l in labels]


@pytest.mark.parametrize("K,N,r", [(384, 384, 4), (256, 256, 8), (640, 640, 4)])
def test_pgemm_gate_lora_residual(ops, labels, K, N, r):
    assert ops.PGEMM
    B, rows = 4, 252
    M = B * rows
    g = torch.Generator().manual_seed(43)
    x = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g)
    res = bf(torch.randn(M, N, generator=g))
    ads = _two_adapters(g, N, K, r)
    pw = ops.pack_linear(w.to(DEV), b.to(DEV))
    ops.attach_lora(pw, [(0, N, A.to(DEV), Bm.to(DEV), s, n) for n, (A, Bm, s) in zip("ab", ads)], {"a": (0, r), "b": (r, r)})

    def run(t):
        y, _ = ops.linear(dv(x), pw, res=dv(res), rowstats=True, lora_gate=t)
        return y.view(B, rows, N)

    def check(got, gates):
        want = x @ w.t() + b + res
        gr = torch.tensor(gates).repeat_interleave(rows, dim=0)
        for i, (A, Bm, s) in enumerate(ads):
            want = want + gr[:, i:i + 1] * (s * (x @ A.t()) @ Bm.t())
        close(got.reshape(M, N), want)                                 # test_lora_residual: close(y, want), defaults

    three_checks(run, GATES4, [r, r], check)
    assert labels and all(l[0].startswith("pgemm_") for l in labels), [l[0] for l in labels]


def _qkv_case(ops, B, N, H, d, r, seed):
    """the fused to_q | to_k | to_v operands of an Attention module with two adapters (rank r on each of q, k, v)"""
    Cc = H * d
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(B * N, Cc, generator=g) * 1.3 + 0.2)
    ws = [bf(torch.randn(Cc, Cc, generator=g) / math.sqrt(Cc)) for _ in range(3)]
    gm, bt = torch.randn(Cc, generator=g) * 0.3 + 1, torch.randn(Cc, generator=g) * 0.2
    xn = F.layer_norm(x, (Cc,), gm, bt, 1e-5)
    lor = {n: [(bf(torch.randn(r, Cc, generator=g) / math.sqrt(Cc)), bf(torch.randn(Cc, r, generator=g) * 0.3), 2.0) for _ in range(3)] for n in "ab"}
    qs = ops.LOG2E / math.sqrt(d)
    pw = ops.pack_linear_ln(torch.cat([ws[0] * qs, ws[1], ws[2]]).to(DEV), None, gm.to(DEV), bt.to(DEV))
    ops.attach_lora(pw, [(i * Cc, Cc, l[0].to(DEV), l[1].to(DEV), l[2] * (qs if i == 0 else 1.0), n) for n in "ab" for i, l in enumerate(lor[n])],
                    {"a": (0, 3 * r), "b": (3 * r, 3 * r)})
    xd = x.to(torch.bfloat16).to(DEV)
    xs = xd.float().view(B * N, Cc // 64, 64)
    parts = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).contiguous()

    def qkv(gates):
        gr = torch.tensor(gates).repeat_interleave(N, dim=0)
        out = []
        for i in range(3):
            y = xn @ ws[i].t()
            for j, n in enumerate("ab"):
                A, Bm, s = lor[n][i]
                y = y + gr[:, j:j + 1] * (s * (xn @ A.t()) @ Bm.t())
            out.append(y)
        return out

    def attention(gates):
        q, k, v = qkv(gates)
        sp = lambda t: t.view(B, N, H, d).transpose(1, 2)
        return F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).reshape(B * N, Cc)

    return Cc, xd, pw, parts, qkv, attention


def test_pgemm_gate_qkv_layernorm_folded_vt(ops, labels):
    B, N, H, d, r = 4, 252, 8, 48, 4
    Cc, xd, pw, parts, qkv, _ = _qkv_case(ops, B, N, H, d, r, 44)
    npad = (N + 7) // 8 * 8
    qs = ops.LOG2E / math.sqrt(d)

    def run(t):
        vt = torch.zeros(B, Cc, npad, dtype=torch.bfloat16, device=DEV)
        qk = ops.conv(xd.view(B, 1, N, Cc), pw, vt=vt, vt_col0=2 * Cc, vt_ld=npad, vt_batch_stride=Cc * npad, ln_parts=parts, lora_gate=t)
        return torch.cat([qk.view(B, N, 2 * Cc), vt[:, :, :N].permute(0, 2, 1)], dim=2)

    def check(got, gates):
        q, k, v = qkv(gates)
        close(got.reshape(B * N, 3 * Cc), torch.cat([q * qs, k, v], dim=1), rtol=2e-2)    # test_qkv_layernorm_folded_lora_vt: rtol=2e-2

    three_checks(run, GATES4, [3 * r, 3 * r], check)
    assert labels and all(l[0].startswith("pgemm_") for l in labels), [l[0] for l in labels]


@pytest.mark.parametrize("r", [2, 4])                                  # combined rank 12 (one rank tile) / 24 (two)
def test_attn_block64_gate(ops, r):
    B, N, H, d = 4, 64, 8, 80
    Cc, xd, pw, parts, _, attention = _qkv_case(ops, B, N, H, d, r, 45)
    assert ops.attn_block64_ok(pw, N, H, d, parts)

    def run(t):
        return ops.attn_block64(xd, pw, parts, B, N, H, d, lora_gate=t).view(B, N, Cc)

    def check(got, gates):
        want = attention(gates)
        close(got.reshape(B * N, Cc), want, rtol=3e-2, atol=2.5e-2 * float(want.abs().max()))     # test_attn_block64_...: same bound

    three_checks(run, GATES4, [3 * r, 3 * r], check)


def test_attn_block64_fp8_gate(ops):
    """config 5: the gate sits in the projection (bf16 arithmetic in both variants); the fp8 launch against the two-launch fp8 path with
    the same gate, at the existing fp8 tolerance (rel. L2 < 2e-2)"""
    import conftest
    B, N, H, d, r = 4, 64, 8, 80, 4
    Cc, xd, pw, parts, _, _ = _qkv_case(ops, B, N, H, d, r, 46)
    t = table(GATES4, [3 * r, 3 * r])
    out8 = ops.attn_block64(xd, pw, parts, B, N, H, d, fp8=True, lora_gate=t)
    npad = (N + 7) // 8 * 8
    vt = torch.zeros(B, Cc, npad, dtype=torch.bfloat16, device=DEV)
    qk = ops.conv(xd.view(B, 1, N, Cc), pw, vt=vt, vt_col0=2 * Cc, vt_ld=npad, vt_batch_stride=Cc * npad, ln_parts=parts, lora_gate=t)
    ref8 = ops.attention(qk.view(B * N, 2 * Cc), vt, B, N, H, d, prescaled=True, fp8=True)
    rl2 = conftest.record(float((out8.float() - ref8.float()).norm() / ref8.float().norm()))
    assert rl2 < 2e-2, rl2
    ones = ops.attn_block64(xd, pw, parts, B, N, H, d, fp8=True, lora_gate=table([[1.0, 1.0]] * B, [3 * r, 3 * r]))
    assert torch.equal(ones, ops.attn_block64(xd, pw, parts, B, N, H, d, fp8=True))
    assert not torch.equal(ones, out8)


@pytest.mark.parametrize("r", [2, 4])
def test_attn_block256_gate(ops, monkeypatch, r):
    B, N, H, d = 4, 252, 8, 48
    Cc, xd, pw, parts, _, attention = _qkv_case(ops, B, N, H, d, r, 47)
    monkeypatch.setattr(ops, "ATTN_BLOCK256", True)
    assert ops.attn_block_ok(pw, N, H, d, parts) == 256

    def run(t):
        return ops.attn_block(xd, pw, parts, B, N, H, d, lora_gate=t).view(B, N, Cc)

    def check(got, gates):
        want = attention(gates)
        close(got.reshape(B * N, Cc), want, rtol=3e-2, atol=2.5e-2 * float(want.abs().max()))     # test_attn_block256_...: same bound

    three_checks(run, GATES4, [3 * r, 3 * r], check)


def test_gate_argument_checks(ops):
    from audioldm_with_lora_amd._lib import AldmError
    g = torch.Generator().manual_seed(48)
    M, K, N, r = 504, 256, 256, 4
    x = dv(torch.randn(M, K, generator=g))
    w = torch.randn(N, K, generator=g) / 16
    pw0 = ops.pack_linear(w.to(DEV), None)
    t = torch.ones(2, 32, device=DEV)
    with pytest.raises(AldmError, match="without an adapter"):
        ops.linear(x, pw0, lora_gate=t)
    pw = ops.pack_linear(w.to(DEV), None)
    ops.attach_lora(pw, [(0, N, torch.randn(r, K, generator=g).to(DEV), torch.randn(N, r, generator=g).to(DEV), 1.0)])
    with pytest.raises(AldmError, match="does not divide"):
        ops.linear(x, pw, lora_gate=torch.ones(5, 32, device=DEV))
    tout = torch.empty(M, 32, dtype=torch.bfloat16, device=DEV)
    for tile in (0, 2):                                                # pgemm and igemm
        with pytest.raises(AldmError, match="lora_t_out"):
            ops.linear(x, pw, lora_gate=t, lora_t_out=tout, splits=1, tile=tile)
    # the C-ABI's own checks (the wrapper refuses the same things earlier)
    import ctypes as C
    from audioldm_with_lora_amd import _lib
    a = _lib.PgemmArgs()
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    a.x, a.w, a.M, a.N, a.K, a.out, a.out_ld = x.data_ptr(), pw.w.data_ptr(), M, N, K, out.data_ptr(), N
    a.lora_a, a.lora_b, a.Rp, a.ranks_used = pw.lora_a.data_ptr(), pw.lora_b.data_ptr(), 32, r
    a.lora_gate, a.gate_rows = t.data_ptr(), 500
    assert _lib.load().aldm_pgemm(C.byref(a), None) != 0 and b"gate_rows" in _lib.load().aldm_last_error()
    a.gate_rows = 0
    assert _lib.load().aldm_pgemm(C.byref(a), None) != 0
    a.gate_rows, a.Rp, a.lora_a, a.lora_b = 252, 0, None, None
    assert _lib.load().aldm_pgemm(C.byref(a), None) != 0 and b"without an adapter" in _lib.load().aldm_last_error()


# ----------------------------------------------------------------------------------------------
# UNet level
# ----------------------------------------------------------------------------------------------
def rel_l2(got, want):
    import conftest
    return conftest.record(float((got - want).norm() / want.norm()))


def _bound(got, want, what):
    r = rel_l2(got, want)
    m = float((got - want).abs().max() / want.abs().max())
    assert r < 3e-2 and m < 6e-2, f"{what}: rel_l2={r:.4g} max_rel={m:.4g}"       # the bound of tests/test_gpu_unet.py


def _pair(cfg, seed):
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from oracle.unet import UNet2DConditionModel as OracleUNet
    torch.manual_seed(seed)
    ref = OracleUNet(**cfg).eval()
    mine = UNet2DConditionModel(**cfg)
    mine.load_state_dict(ref.state_dict(), strict=True)
    return ref, mine


def _load(mine, adapters):
    """the adapters of the restatement helper into the HIP model through the code under test"""
    import multi_adapter_restatement as mar
    from audioldm_with_lora_amd import lora as plora
    pm = None
    for name, ad in adapters.items():
        cfg = plora.LoraConfig(r=ad["r"], lora_alpha=ad["alpha"], target_modules=list(ad["targets"]), init_lora_weights="gaussian")
        if pm is None:
            pm = plora.get_peft_model(mine, cfg, adapter_name=name)
            pm.load_adapter(mar.peft_state_dict(ad), name, cfg)
        else:
            pm.load_adapter(mar.peft_state_dict(ad), name, cfg)
    return pm


def test_tiny_unet_mixed_batch_matches_merged_oracle():
    import multi_adapter_restatement as mar
    from oracle import configs
    ref, mine = _pair(configs.tiny_unet(), seed=3)
    adapters = {"a": mar.make_adapter(ref, 4, 8, mar.TARGETS4, seed=4), "b": mar.make_adapter(ref, 4, 8, mar.TARGETS4, seed=5)}
    g = torch.Generator().manual_seed(2)
    x = torch.randn(4, 8, 32, 16, generator=g)
    c = F.normalize(torch.randn(4, 64, generator=g), dim=-1)
    t = torch.tensor([400, 20, 700, 150])
    routing = ["a", "b", "__base__", {"a": 0.5, "b": 0.5}]
    want = mar.expected_batch(ref, adapters, routing, x, t, c)
    # item 5: the recipe can tell the adapters apart (oracle against oracle)
    base = mar.expected_batch(ref, adapters, ["__base__"] * 4, x, t, c)
    all_a = mar.expected_batch(ref, adapters, ["a"] * 4, x, t, c)
    all_b = mar.expected_batch(ref, adapters, ["b"] * 4, x, t, c)
    for b in range(4):
        for u, v, what in ((all_a, base, "a / base"), (all_b, base, "b / base"), (all_a, all_b, "a / b")):
            dist = float((u[b] - v[b]).norm() / v[b].norm())
            assert dist > 5e-2, f"sample {b}: {what} only {dist:.3g} apart -- the test could not tell them apart"
    mine = mine.to(DEV)
    with torch.no_grad():
        plain = mine(x.cuda(), t.cuda(), class_labels=c.cuda())[0].float().cpu()          # no adapter injected at all
    pm = _load(mine, adapters)
    assert pm.lora_adapters() == ["a", "b"] and mine.lora_layout() == {"a": (0, 12), "b": (12, 12)}
    with torch.no_grad():
        got = pm(x.cuda(), t.cuda(), class_labels=c.cuda(), adapter_names=routing)[0].float().cpu()
        got_a = pm(x.cuda(), t.cuda(), class_labels=c.cuda(), adapter_names=["a"] * 4)[0].float().cpu()
        pm.set_adapter("a")
        got_a2 = pm(x.cuda(), t.cuda(), class_labels=c.cuda())[0].float().cpu()          # active adapter, no per-sample routing
        with pm.disable_adapter():
            got_off = pm(x.cuda(), t.cuda(), class_labels=c.cuda())[0].float().cpu()
    for b in range(4):
        _bound(got[b], want[b], f"sample {b} ({routing[b]})")
    _bound(got[2], plain[2], "__base__ sample against the UNet without adapters")
    assert torch.equal(got_a[0], got[0]), "sample 0 (adapter a) of the mixed batch differs from the all-a batch"
    assert torch.equal(got_a2, got_a), "set_adapter('a') differs from adapter_names=['a'] * 4"
    assert torch.equal(got_off[2], got[2]), "disable_adapter() differs from the __base__ row"
    _bound(got_a, all_a, "all-a batch")


def test_full_width_config2_shape_four_adapters_mixed_batch():
    """latents 250 x 16, the reference's r = 2 to_q / to_v, four adapters, one per clip + base + blend: all four kernel families and
    the straddling tiles are live"""
    import multi_adapter_restatement as mar
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref, mine = _pair({}, seed=1234)
    names = ["boom_bap", "trap", "lofi", "drill"]
    adapters = {n: mar.make_adapter(ref, 2, 2, ("to_q", "to_v"), seed=10 + i, b_std=0.02) for i, n in enumerate(names)}
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4, 8, 250, 16, generator=g)
    c = F.normalize(torch.randn(4, 512, generator=g), dim=-1)
    t = torch.tensor([996, 501, 250, 20])
    routing = ["boom_bap", "drill", "__base__", {"trap": 0.5, "lofi": 0.5}]
    want = mar.expected_batch(ref, adapters, routing, x, t, c)
    pm = _load(mine.to(DEV), adapters)
    assert mine.lora_layout() == {n: (4 * i, 4) for i, n in enumerate(names)}
    with torch.no_grad():
        got = pm(x.cuda(), t.cuda(), class_labels=c.cuda(), adapter_names=routing)[0].float().cpu()
    for b in range(4):
        _bound(got[b], want[b], f"sample {b} ({routing[b]})")


# ----------------------------------------------------------------------------------------------
# engine and pipeline (tests/synth_checkpoint.py's checkpoint)
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    import multi_adapter_restatement as mar
    import synth_checkpoint
    root = str(tmp_path_factory.mktemp("ckpt"))
    src = synth_checkpoint.write_model_dir(root, seed=0, with_text=False)
    adapters = {"a": mar.make_adapter(src["unet"], 4, 8, mar.TARGETS4, seed=4), "b": mar.make_adapter(src["unet"], 4, 8, mar.TARGETS4, seed=5)}
    return root, adapters


def _pipe(root, adapters=None, cls=None):
    import multi_adapter_restatement as mar
    from audioldm_with_lora_amd.pipeline import AudioLDMPipeline
    pipe = (cls or AudioLDMPipeline).from_pretrained(root).to(DEV)
    for n, ad in (adapters or {}).items():
        pipe.load_lora_weights(mar.peft_state_dict(ad), adapter_name=n, lora_alpha=ad["alpha"])
    return pipe


ROUTING = ["a", "b", "__base__", {"a": 0.5, "b": 0.5}]


def test_engine_switches_routing_without_repack_or_recapture(ckpt):
    from audioldm_with_lora_amd.engine import DenoiseEngine
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    root, adapters = ckpt
    pipe = _pipe(root, adapters)
    unet = pipe._unet
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(4, 8, 16, 16, generator=g)
    pe = F.normalize(torch.randn(4, 64, generator=g), dim=-1)
    other = ["b", "__base__", "a", {"a": 0.25, "b": 1.5}]

    def fresh(routing):
        eng = DenoiseEngine(unet, DDIMScheduler(), 4, 16, 16, 4, 2.5, device=DEV)
        eng.set_adapters(routing)
        eng.set_condition(pe)
        eng.set_latents(lat)
        eng.capture()
        return eng

    eng = fresh(ROUTING)
    assert eng.gated
    graph, plan = eng.graph, unet.plan()
    r1 = eng.run().clone()
    eng.set_adapters(other)
    eng.set_latents(lat)
    r2 = eng.run().clone()
    assert eng.graph is graph and not eng.stale() and unet.plan() is plan
    assert not torch.equal(r1, r2)
    assert torch.equal(r1, fresh(ROUTING).run()) and torch.equal(r2, fresh(other).run())
    # CFG: both halves of a clip carry the same gates
    assert torch.equal(eng.gate[0][:4], eng.gate[0][4:]) and tuple(eng.gate[0].shape) == (8, 32)


def test_pipeline_mixed_adapter_call(ckpt):
    root, adapters = ckpt
    pipe = _pipe(root, adapters)
    bare = _pipe(root)
    pe = F.normalize(torch.randn(1, 64, generator=torch.Generator().manual_seed(3)), dim=-1).repeat(4, 1)
    kw = dict(prompt_embeds=pe, audio_length_in_s=0.64, num_inference_steps=4, guidance_scale=2.5, output_type="pt")
    gen = lambda: torch.Generator().manual_seed(11)
    mixed = pipe(adapter_names=ROUTING, generator=gen(), **kw).audios
    none = bare(generator=gen(), **kw).audios
    assert torch.equal(mixed[2], none[2]), "the __base__ clip differs from a pipeline with no adapter loaded"
    pipe.set_adapters("a")
    assert pipe.get_active_adapters() == ["a"] and pipe.get_list_adapters() == {"unet": ["a", "b"]}
    all_a = pipe(generator=gen(), **kw).audios
    assert torch.equal(mixed[0], all_a[0]), "clip 0 (adapter a) differs from set_adapters('a') for everyone"
    assert not torch.equal(mixed[1], all_a[1]) and not torch.equal(mixed[3], all_a[3])
    # one entry per prompt, repeated over num_waveforms_per_prompt like the prompt embeddings
    two = pipe(adapter_names=["a", "__base__"], generator=gen(), num_waveforms_per_prompt=2, **dict(kw, prompt_embeds=pe[:2])).audios
    assert torch.equal(two[0], mixed[0]) and torch.equal(two[1], all_a[1]) and torch.equal(two[2], none[2]) and torch.equal(two[3], none[3])
    pipe.disable_lora()
    assert torch.equal(pipe(generator=gen(), **kw).audios, none)
    pipe.enable_lora()
    pipe.delete_adapters("b")
    assert pipe.get_list_adapters() == {"unet": ["a"]}
    with pytest.raises(ValueError, match="unknown adapter"):
        pipe(adapter_names=["b"] * 4, generator=gen(), **kw)
    pipe.unload_lora_weights()
    assert torch.equal(pipe(generator=gen(), **kw).audios, none)


def test_single_default_adapter_keeps_the_single_adapter_bits(ckpt):
    """only "default" loaded, nothing set: no gate is passed and the result is the one of the pre-existing path (get_peft_model +
    load_state_dict), bit for bit"""
    import multi_adapter_restatement as mar
    from audioldm_with_lora_amd import lora as plora
    from audioldm_with_lora_amd.pipeline import AudioLDMPipeline
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    root, adapters = ckpt
    ad = adapters["a"]
    pe = F.normalize(torch.randn(2, 64, generator=torch.Generator().manual_seed(3)), dim=-1)
    kw = dict(prompt_embeds=pe, audio_length_in_s=0.64, num_inference_steps=4, guidance_scale=2.5, output_type="pt")
    # the pre-existing path
    unet = UNet2DConditionModel.from_pretrained(root, subfolder="unet")
    pm = plora.get_peft_model(unet, plora.LoraConfig(r=4, lora_alpha=8, target_modules=list(mar.TARGETS4), init_lora_weights="gaussian"))
    sd = {k.replace(".lora_A.weight", ".lora_A.default.weight").replace(".lora_B.weight", ".lora_B.default.weight"): v
          for k, v in mar.peft_state_dict(ad).items()}
    missing = pm.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys
    old = AudioLDMPipeline.from_pretrained(root, unet=pm).to(DEV)
    want = old(generator=torch.Generator().manual_seed(11), **kw).audios
    assert not old.engine(2, 16, 16, 4, 2.5).gated
    new = _pipe(root, {"default": ad})
    got = new(generator=torch.Generator().manual_seed(11), **kw).audios
    assert not any(e.gated for e in new._engines.values())
    assert torch.equal(got, want)


def test_euler_ancestral_and_audio_to_audio_accept_adapter_names(ckpt):
    from audioldm_with_lora_amd.audio2audio import AudioLDMAudioToAudioPipeline
    from audioldm_with_lora_amd.scheduler import EulerAncestralDiscreteScheduler
    root, adapters = ckpt
    pipe = _pipe(root, adapters)
    pipe.scheduler = EulerAncestralDiscreteScheduler.from_config(pipe.scheduler.config)
    pe = F.normalize(torch.randn(1, 64, generator=torch.Generator().manual_seed(3)), dim=-1).repeat(2, 1)
    kw = dict(prompt_embeds=pe, audio_length_in_s=0.64, num_inference_steps=4, guidance_scale=2.5, output_type="pt")
    u = pipe(adapter_names=["a", "__base__"], generator=torch.Generator().manual_seed(5), **kw).audios
    v = pipe(adapter_names=["b", "__base__"], generator=torch.Generator().manual_seed(5), **kw).audios
    assert torch.isfinite(u).all() and torch.isfinite(v).all()
    assert not torch.equal(u[0], v[0]) and torch.equal(u[1], v[1])
    a2a = AudioLDMAudioToAudioPipeline.from_pipe(_pipe(root, adapters))
    wav = torch.sin(torch.arange(10240) * 0.05) * 0.3
    kw = dict(prompt_embeds=pe, audio=wav, strength=0.6, num_inference_steps=5, guidance_scale=2.5, output_type="pt")
    u = a2a(adapter_names=["a", "__base__"], generator=torch.Generator().manual_seed(5), **kw).audios
    v = a2a(adapter_names=["b", "__base__"], generator=torch.Generator().manual_seed(5), **kw).audios
    assert torch.isfinite(u).all() and torch.isfinite(v).all()
    assert not torch.equal(u[0], v[0]) and torch.equal(u[1], v[1])
