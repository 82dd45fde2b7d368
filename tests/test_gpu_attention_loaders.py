"""attention_kernel with loader waves (csrc/attention.hip, NL): the compute waves' arithmetic is the NL = 0 kernel's, so every output
is compared BIT FOR BIT with the ALDM_ATTN_LOADERS=0 launch of the same inputs, and against fp32 SDPA at the tolerance
tests/test_gpu_ops.py::test_attention uses (rtol 2e-2, atol 1e-2; the fp8 form at test_attention_fp8_operands' rel. L2 < 8e-2).

The switch is read at every launch.  Unset, the product rule applies (loaders at the N >= 192 forms); 4 puts the four loader waves
on every multi-wave form (N >= 64), which is how the shorter sequences reach the loader code here.  Shapes: one tile (N = 1, 64),
a tail of one key (65), three tiles = both register sets and both LDS buffers (129), the key-split site (252: four tiles over two wave
groups; 320: five, so group 1 sits the last iteration out and still has to arrive at its barrier), and the 8-wave forms (800)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
SWITCH = "ALDM_ATTN_LOADERS"
B, H = 2, 2


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    return o


def close(got, want, rtol=2e-2, atol=1e-2):
    err = (got.float().cpu() - want).abs()
    bad = ~(err <= atol + rtol * want.abs())
    assert not bad.any(), f"max err {float(err.max()):.4g} (ref max {float(want.abs().max()):.4g}), {int(bad.sum())} bad"


@functools.lru_cache(maxsize=None)
def draw(d, N, Bn=B, Hn=H):
    """(q, k, v) bf16-representable fp32 [Bn, N, C], the fp32 SDPA output [Bn * N, C] and its log-sum-exp [Bn, Hn, N] in log2 units"""
    g = torch.Generator().manual_seed(100 * d + N)
    C = Hn * d
    q, k, v = (torch.randn(Bn, N, C, generator=g).to(torch.bfloat16).float() for _ in range(3))
    q = (q * 1.5).to(torch.bfloat16).float()
    sp = lambda z: z.view(Bn, N, Hn, d).transpose(1, 2)
    want = F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).reshape(Bn * N, C)
    lse = torch.logsumexp(sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(d), -1) * math.log2(math.e)
    return q, k, v, want, lse


def operands(q, k, v, prescale=1.0):
    """Q | K rows and V^T [B, C, Npad] on the device; the V^T padding is NaN: it must never reach a result"""
    Bn, N, C = q.shape
    qk = torch.cat([q * prescale, k], -1).view(Bn * N, 2 * C).to(torch.bfloat16).to(DEV)
    npad = (N + 7) // 8 * 8
    vt = torch.full((Bn, C, npad), float("nan"), dtype=torch.bfloat16, device=DEV)
    vt[:, :, :N] = v.transpose(1, 2).to(torch.bfloat16).to(DEV)
    return qk, vt


def forms(monkeypatch, N, fn):
    """fn() under ALDM_ATTN_LOADERS=0, and under every setting that can put loader waves on a launch of N keys"""
    monkeypatch.setenv(SWITCH, "0")
    off = fn()
    on = []
    monkeypatch.delenv(SWITCH)
    on.append(("default", fn()))
    monkeypatch.setenv(SWITCH, "4")
    on.append(("4", fn()))
    monkeypatch.delenv(SWITCH)
    return off, on


@pytest.mark.parametrize("N", [1, 64, 65, 129, 252, 320])
@pytest.mark.parametrize("d", [32, 48, 80])
def test_loader_waves_bit_identical_and_close_to_sdpa(ops, monkeypatch, d, N):
    q, k, v, want, _ = draw(d, N)
    qk, vt = operands(q, k, v)
    off, on = forms(monkeypatch, N, lambda: ops.attention(qk, vt, B, N, H, d))
    for name, out in on:
        assert torch.equal(out, off), f"loaders {name}: differs from {SWITCH}=0"
    close(off, want)


@pytest.mark.parametrize("d,N,Bn,Hn", [(32, 800, 8, 8), (32, 800, 2, 2), (48, 252, 2, 2), (80, 252, 2, 2)])
def test_loader_waves_prescaled_sites(ops, monkeypatch, d, N, Bn, Hn):
    """The UNet's instantiations: Q carries d^-0.5 log2(e).  8 x 8 (batch, head) pairs x 4 query blocks is the one-wave-per-block
    8-wave form of the N = 1000 site, 2 x 2 pairs the key-split 8-wave form."""
    q, k, v, want, _ = draw(d, N, Bn, Hn)
    qk, vt = operands(q, k, v, ops.LOG2E / math.sqrt(d))
    off, on = forms(monkeypatch, N, lambda: ops.attention(qk, vt, Bn, N, Hn, d, prescaled=True))
    for name, out in on:
        assert torch.equal(out, off), f"loaders {name}: differs from {SWITCH}=0"
    close(off, want, rtol=3e-2, atol=1.5e-2)                 # test_attention_prescaled_path_and_deferred_rescale's bound


@pytest.mark.parametrize("d,N", [(48, 129), (48, 252), (80, 320)])
def test_loader_waves_kv_len_with_an_all_padding_workgroup(ops, monkeypatch, d, N):
    """lengths 1 / 70 / N: a tail inside the first and the second tile, and workgroups whose queries are all padding (they leave
    before the first barrier, loaders included, and store zeros)"""
    lens = (1, 70, N)
    Bn = len(lens)
    q, k, v, _, _ = draw(d, N, Bn, H)
    qk, vt = operands(q, k, v)
    kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    off, on = forms(monkeypatch, N, lambda: ops.attention(qk, vt, Bn, N, H, d, kv_len=kv))
    for name, out in on:
        assert torch.equal(out, off), f"loaders {name}: differs from {SWITCH}=0"
    C = H * d
    bias = torch.zeros(Bn, 1, 1, N)
    for b, n in enumerate(lens):
        bias[b, ..., n:] = float("-inf")
    sp = lambda z: z.view(Bn, N, H, d).transpose(1, 2)
    want = F.scaled_dot_product_attention(sp(q), sp(k), sp(v), attn_mask=bias).transpose(1, 2).reshape(Bn, N, C)
    got = off.float().cpu().view(Bn, N, C)
    qwg = 128 if N < 192 else 64                             # queries per workgroup: 4 waves x 32, or 2 x 32 with the keys split
    for b, n in enumerate(lens):
        close(got[b, :n], want[b, :n])
        pad0 = (n + qwg - 1) // qwg * qwg
        assert not got[b, pad0:].any(), "an all-padding workgroup did not store zeros"


@pytest.mark.parametrize("N", [129, 252])
@pytest.mark.parametrize("d", [32, 48, 80])
def test_loader_waves_fp8_form(ops, monkeypatch, d, N):
    q, k, v, want, _ = draw(d, N)
    npad = (N + 7) // 8 * 8
    qk, _ = operands(q, k, v)
    vt = torch.zeros(B, H * d, npad, dtype=torch.bfloat16, device=DEV)
    vt[:, :, :N] = v.transpose(1, 2).to(torch.bfloat16).to(DEV)
    off, on = forms(monkeypatch, N, lambda: ops.attention(qk, vt, B, N, H, d, fp8=True))
    for name, out in on:
        assert torch.equal(out, off), f"loaders {name}: differs from {SWITCH}=0"
    rel = float((off.float().cpu() - want).norm() / want.norm())
    assert rel < 8e-2, rel                                    # test_attention_fp8_operands' bound against the fp32 reference


@pytest.mark.parametrize("N", [129, 252])
@pytest.mark.parametrize("d", [32, 48, 80])
def test_loader_waves_lse_form(ops, monkeypatch, d, N):
    """The training forward: out and the stored log-sum-exp.  The lse is fp32 arithmetic on bf16 operands throughout (d-term dot
    products, at most 320 probabilities summed, one v_exp_f32 / v_log_f32 each): errors of a few 1e-5 log2 units at these score
    magnitudes, bounded here by 1e-3."""
    q, k, v, want, lse_want = draw(d, N)
    C = H * d
    qkv = torch.cat([q, k, v], -1).view(B * N, 3 * C).to(torch.bfloat16).to(DEV)
    qkvT = ops.transpose_tokens(qkv, B, N, 3 * C)
    off, on = forms(monkeypatch, N, lambda: ops.attention_train(qkv, qkvT, B, N, H, d))
    for name, (out, lse) in on:
        assert torch.equal(out, off[0]), f"loaders {name}: out differs from {SWITCH}=0"
        assert torch.equal(lse, off[1]), f"loaders {name}: lse differs from {SWITCH}=0"
    close(off[0], want)
    err = float((off[1].cpu() - lse_want).abs().max())
    assert err < 1e-3, err
