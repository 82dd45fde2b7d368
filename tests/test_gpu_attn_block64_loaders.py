"""attn_block64_kernel with four loader waves beside the four compute waves (csrc/attn_block64.hip, LW): the compute waves keep
their arithmetic, so every output is compared BIT FOR BIT with the ALDM_B64_LOADERS=0 launch (the switch is read at every launch).

Parity: the bf16 form against the float64 restatement tests/norm_restatement.attn_block with the floor comparator `check`, as
tests/test_gpu_norm_edges.py::test_attn_block_on_ladder_rows does.  The restatement has no e4m3 form, so the fp8 launches are held to
the bound tests/test_gpu_ops.py has for them: rel. L2 < 2e-2 against the two-launch fp8 path (same quantisation points; at N <= 64
that path's attention kernel runs without loader waves).  The gated case uses one power-of-two gate per sample: scaling T''
by it commutes with the bf16 rounding, so the restatement with the adapters' scaling multiplied by the gate is the same arithmetic.

Shapes: B 1 / 3, N 17 / 40 / 64 (ragged against the wave's 16 tokens, against the 64, exact), combined LoRA rank 0 / 12 / 24 = zero,
one and two rank tiles."""
import functools

import pytest
import torch

import norm_restatement as R
from norm_restatement import EPS, check

pytestmark = pytest.mark.gpu

DEV = "cuda"
SWITCH = "ALDM_B64_LOADERS"
H, D = 8, 80
C = H * D


@pytest.fixture(scope="module")
def ops():
    from audioldm_with_lora_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def draw(B, N, r):
    return R.ln_linear_draw(B * N, C, 3 * C, r)


def pack(ops, W, gm, bt, parts):
    pw = ops.pack_linear_ln(W.float().to(DEV), None, gm.float().to(DEV), bt.float().to(DEV), EPS)
    if parts:
        ops.attach_lora(pw, [(r0, nr, A.to(DEV), Bm.to(DEV), s) for r0, nr, A, Bm, s in parts])
    return pw


def slab_parts(xd, M):
    xs = xd.float().view(M, C // 64, 64)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).contiguous()


def both_forms(monkeypatch, fn):
    monkeypatch.setenv(SWITCH, "0")
    off = fn()
    monkeypatch.delenv(SWITCH)
    return off, fn()


@pytest.mark.parametrize("r", [0, 4, 8])
@pytest.mark.parametrize("N", [17, 40, 64])
@pytest.mark.parametrize("B", [1, 3])
def test_loader_waves_bf16(ops, monkeypatch, B, N, r):
    x, W, _, gm, bt, parts = draw(B, N, r)
    pw = pack(ops, W, gm, bt, parts)
    xd = x.to(torch.bfloat16).to(DEV)
    lp = slab_parts(xd, B * N)
    assert ops.attn_block64_ok(pw, N, H, D, lp)
    off, on = both_forms(monkeypatch, lambda: ops.attn_block64(xd, pw, lp, B, N, H, D))
    assert torch.equal(on, off), f"loader waves: differs from {SWITCH}=0"
    fn = lambda **kw: R.attn_block(x, W, gm, bt, EPS, parts, B, N, H, D, **kw)
    check(on, fn(), fn(rounded=True), f"attn_block64 loaders B{B} N{N} r{r}")


@pytest.mark.parametrize("r", [0, 4, 8])
@pytest.mark.parametrize("N", [17, 40, 64])
@pytest.mark.parametrize("B", [1, 3])
def test_loader_waves_fp8(ops, monkeypatch, B, N, r):
    x, W, _, gm, bt, parts = draw(B, N, r)
    pw = pack(ops, W, gm, bt, parts)
    xd = x.to(torch.bfloat16).to(DEV)
    lp = slab_parts(xd, B * N)
    off, on = both_forms(monkeypatch, lambda: ops.attn_block64(xd, pw, lp, B, N, H, D, fp8=True))
    assert torch.equal(on, off), f"loader waves: differs from {SWITCH}=0"
    npad = (N + 7) // 8 * 8
    vt = torch.zeros(B, C, npad, dtype=torch.bfloat16, device=DEV)
    qk = ops.conv(xd.view(B, 1, N, C), pw, vt=vt, vt_col0=2 * C, vt_ld=npad, vt_batch_stride=C * npad, ln_parts=lp)
    ref8 = ops.attention(qk.view(B * N, 2 * C), vt, B, N, H, D, prescaled=True, fp8=True).float()
    rel = float((on.float() - ref8).norm() / ref8.norm())
    assert rel < 2e-2, rel


def test_loader_waves_gated(ops, monkeypatch):
    B, N, r = 3, 40, 4
    gates = (1.0, 0.5, 2.0)
    x, W, _, gm, bt, parts = draw(B, N, r)
    pw = pack(ops, W, gm, bt, parts)
    xd = x.to(torch.bfloat16).to(DEV)
    lp = slab_parts(xd, B * N)
    t = torch.tensor(gates, device=DEV).view(B, 1).repeat(1, pw.Rp).contiguous()
    off, on = both_forms(monkeypatch, lambda: ops.attn_block64(xd, pw, lp, B, N, H, D, lora_gate=t))
    assert torch.equal(on, off), f"loader waves: differs from {SWITCH}=0"
    assert not torch.equal(on, ops.attn_block64(xd, pw, lp, B, N, H, D))
    for b, g in enumerate(gates):
        rows = slice(b * N, (b + 1) * N)
        pb = [(r0, nr, A, Bm, s * g) for r0, nr, A, Bm, s in parts]
        fn = lambda **kw: R.attn_block(x[rows], W, gm, bt, EPS, pb, 1, N, H, D, **kw)
        check(on[rows], fn(), fn(rounded=True), f"attn_block64 loaders gated sample {b}")
