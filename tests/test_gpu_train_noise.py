"""GPU: the training step's noise and timesteps drawn on the device -- aldm_train_noise_fused from the kernel up to LoraTrainer,
its captured graphs and its checkpoints.  The oracles are the library's own aldm_randn / aldm_philox_u32 for the bits of the stream
and the float64 restatement in tests/train_noise_restatement.py for everything after the generator.  Every model is
oracle.configs.tiny_unet() on latents [2, 8, 16, 16]."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_noise_restatement as N  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1000
# [2, 8, 4, 16]: the four-wide path.  [3, 8, 5, 3]: 360 elements, H*W odd -- a Philox block straddles channels and samples, the
# per-channel offset straddles threads.  [1, 3, 5, 3]: 45 elements, not a multiple of 4 -- the one-element-per-thread path.
SHAPES = [(2, 8, 4, 16), (3, 8, 5, 3), (1, 3, 5, 3)]
# draw ordinals the kernel starts from: the 32-bit carry falls between its four draws; a rank's base with the high word in use
ORDINALS = {(2, 8, 4, 16): 2 ** 32 - 2, (3, 8, 5, 3): 2 ** 48, (1, 3, 5, 3): 12}
SEED = 0x5EED0123456789


def _rel(a, b):
    import conftest
    return conftest.record(float((a.double() - b.double()).norm() / b.double().norm()))


def _abar():
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    return DDIMScheduler().alphas_cumprod.float()


def _device_draws(seed, d, shape):
    """what the library's own generator entry points give at the step's four ordinals: (timesteps, e, n, o) on the device"""
    from audioldm_with_lora_amd import ops
    B, C, H, W = shape
    w = ops.philox_u32(B, ops.philox_state(seed, d))
    t = ((w.long() & 0xFFFFFFFF) * T) >> 32
    e = ops.randn(shape, ops.philox_state(seed, d + 1), advance=False)
    n = ops.randn(shape, ops.philox_state(seed, d + 2), advance=False)
    o = ops.randn((B, C), ops.philox_state(seed, d + 3), advance=False)
    return t, e, n, o


def _sources(shape):
    """(latents NCHW, moments channels-last) on the CPU; some log-variances lie beyond the clamp at -30 / 20"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    lat = torch.randn(shape, generator=g) * 0.92
    mom = torch.randn(B, H, W, 2 * C, generator=g)
    mom[..., C:] = mom[..., C:] * 4.0 - 3.0
    mom[0, 0, 0, C], mom[0, 0, 1, C] = 25.0, -40.0
    return lat, mom


# ---- 1. the kernel against the existing pieces ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_timesteps_target_and_ordinal_match_the_generator(shape):
    from audioldm_with_lora_amd import ops
    B, C, H, W = shape
    d = ORDINALS[shape]
    ac = _abar().cuda()
    lat, mom = _sources(shape)
    t_dev, e, n, o = _device_draws(SEED, d, shape)
    want = N.step(SEED, d, shape, ac.cpu().numpy(), latents=lat.numpy())
    assert np.array_equal(t_dev.cpu().numpy(), want["timesteps"])                # the generator's words agree with the restatement
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    for off in (0.0, 0.1):
        for src in (dict(latents=lat.cuda()), dict(moments=mom.cuda(), scaling_factor=0.9)):
            st = ops.philox_state(SEED, d)
            x_in, tgt, ts, tf = ops.train_noise_fused(st, ac, noise_offset=off, ticket=ticket, **src)
            assert x_in.shape == tgt.shape == (B, H, W, C) and x_in.dtype == torch.bfloat16 and tgt.dtype == torch.float32
            assert ts.dtype == torch.int64 and np.array_equal(ts.cpu().numpy(), want["timesteps"])
            assert tf.dtype == torch.float32 and torch.equal(tf, ts.float())
            assert ops.philox_state_values(st) == (SEED, d + 4) and int(ticket) == 0
            if off == 0.0:
                assert torch.equal(tgt, n.permute(0, 2, 3, 1).contiguous())       # bit for bit aldm_randn at d + 2
            else:
                ref = (n + off * o[:, :, None, None]).permute(0, 2, 3, 1).contiguous()
                ulp = torch.from_numpy(np.spacing(np.abs(ref.cpu().numpy())))
                err = (tgt.cpu() - ref.cpu()).abs()
                print(f"{shape} offset {off}: worst target error {float((err / ulp).max()):.3g} ulp")
                assert bool((err <= ulp).all())
    # without a ticket the state stays
    st = ops.philox_state(SEED, d)
    ops.train_noise_fused(st, ac, latents=lat.cuda())
    assert ops.philox_state_values(st) == (SEED, d)


# ---- 2. x_in against the float64 restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_unet_input_matches_float64_restatement(shape):
    """|x_in - ref| <= 2^-7 |ref| + 1e-6 on every element: one bf16 rounding is at most 2^-8 relative, and an fp32 result a few ulp off
    float64 may land on the neighbouring bf16 value (one more ulp, at most 2^-7 relative at the bottom of a binade); the absolute term
    covers cancellation in a lat + s n.  The restatement is fed the device's own e / n / o."""
    from audioldm_with_lora_amd import ops
    import conftest
    d = ORDINALS[shape]
    ac = _abar().cuda()
    lat, mom = _sources(shape)
    _, e, n, o = _device_draws(SEED, d, shape)
    dev = dict(e=e.cpu().numpy(), n=n.cpu().numpy(), o=o.cpu().numpy())
    for off in (0.0, 0.1):
        for name, src, rsrc in (("latents", dict(latents=lat.cuda()), dict(latents=lat.numpy())),
                                ("moments", dict(moments=mom.cuda(), scaling_factor=0.9), dict(moments=mom.numpy(), scaling_factor=0.9))):
            x_in = ops.train_noise_fused(ops.philox_state(SEED, d), ac, noise_offset=off, **src)[0]
            ref = N.step(SEED, d, shape, ac.cpu().numpy().astype(np.float64), noise_offset=off, **rsrc, **dev)["noisy"]
            err = np.abs(x_in.float().cpu().numpy().astype(np.float64) - ref)
            ratio = float((err / (2.0 ** -7 * np.abs(ref) + 1e-6)).max())
            conftest.record(ratio, f"x_in worst error / bound ({name}, offset {off})")
            print(f"{shape} {name} offset {off}: worst |x_in - ref| / bound = {ratio:.4f}")
            assert ratio <= 1.0


# ---- trainers ------------------------------------------------------------------------------------------------------------------
def _trainer(seed=0, lr=1e-3, **kw):
    from audioldm_with_lora_amd import lora as plora
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from audioldm_with_lora_amd.training import LoraTrainer
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from oracle import configs
    torch.manual_seed(seed)
    unet = UNet2DConditionModel(**configs.tiny_unet())
    unet.requires_grad_(False)
    pm = plora.get_peft_model(unet, plora.LoraConfig(r=4, lora_alpha=4, target_modules=["to_q", "to_k", "to_v", "to_out.0"],
                                                     init_lora_weights="gaussian"))
    g = torch.Generator().manual_seed(seed + 1)
    sd = pm.state_dict()
    for k in sd:
        if "lora_B" in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
    pm.load_state_dict(sd)
    return LoraTrainer(unet.cuda(), DDIMScheduler(), lr=lr, weight_decay=1e-2, max_train_steps=100, **kw)


def _batches(k, seed=50):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 8, 16, 16, generator=g) * 0.92, F.normalize(torch.randn(2, 64, generator=g), dim=-1)) for _ in range(k)]


def _want_t(seed, d, B=2):
    import philox_restatement as P
    return N.timesteps_of(P.u32(seed, d, B), T)


# ---- 3. graph replay moves the stream ------------------------------------------------------------------------------------------
def test_graph_replay_moves_the_stream_like_the_eager_steps():
    from audioldm_with_lora_amd import ops
    data = _batches(5)
    seen = {}
    for use_graph in (True, False):
        tr = _trainer(noise_seed=31, use_graph=use_graph)
        assert ops.philox_state_values(tr.noise_state) == (31, 0)
        ts = []
        for i, (lat, emb) in enumerate(data):                 # graph: two eager warm-ups, the capture + first replay, two more replays
            tr.step(lat, None, None, emb)
            assert tr.last_timesteps.is_cuda and tr.last_timesteps.dtype == torch.int64
            ts.append(tr.last_timesteps.cpu().numpy().copy())
            assert np.array_equal(ts[-1], _want_t(31, 4 * i)), (use_graph, i)
            assert ops.philox_state_values(tr.noise_state) == (31, 4 * (i + 1)), (use_graph, i)
        assert (tr.graph is not None) == use_graph
        seen[use_graph] = ts, tr.flat.params.detach().clone()
    assert all(np.array_equal(a, b) for a, b in zip(seen[True][0], seen[False][0]))
    assert len({tuple(t) for t in seen[True][0]}) == 5         # every replay drew new timesteps
    assert _rel(seen[True][1], seen[False][1]) < 1e-3


# ---- 4. device noise equals host-passed noise ----------------------------------------------------------------------------------
@pytest.mark.parametrize("snr_gamma", [None, 5.0])
def test_device_noise_step_equals_the_step_fed_the_same_noise_as_tensors(snr_gamma):
    """snr_gamma: mse_grad_snr must read the timesteps the fused launch drew"""
    (lat, emb), = _batches(1)
    a = _trainer(noise_seed=77, use_graph=False, snr_gamma=snr_gamma)
    b = _trainer(use_graph=False, snr_gamma=snr_gamma)
    t, _, n, _ = _device_draws(77, 0, tuple(lat.shape))
    la = float(a.loss_and_grads(lat, None, None, emb))
    lb = float(b.loss_and_grads(lat, n, t, emb))
    assert torch.equal(a.last_timesteps, t) and torch.equal(b.last_timesteps, t)
    rel = _rel(a.flat.grads[:a.flat.n], b.flat.grads[:b.flat.n])
    print(f"snr_gamma {snr_gamma}: loss {la:.6g} / {lb:.6g}, flat-gradient relative L2 {rel:.3g}")
    assert abs(la - lb) < 1e-3 * abs(lb) and rel < 1e-3


def test_device_noise_loop_body_equals_the_loop_body_fed_the_same_noise():
    """step_from_batch: the moments go to the fused launch channels-last; the host path transposes, samples and scales them first"""
    from audioldm_with_lora_amd import configs
    from audioldm_with_lora_amd.clap_text import ClapTextModelWithProjection
    from audioldm_with_lora_amd.script.train import synthetic_batch
    from audioldm_with_lora_amd.vae import AutoencoderKL
    torch.manual_seed(3)
    vae = AutoencoderKL(**configs.tiny_vae()).requires_grad_(False).cuda()
    clap = ClapTextModelWithProjection(**dict(configs.tiny_clap_text(), max_position_embeddings=514, projection_dim=64)).requires_grad_(False).cuda()
    batch = synthetic_batch(2, torch.Generator().manual_seed(2), vocab=200)
    batch["log_mel_spec"] = batch["log_mel_spec"][:, :, :64].contiguous()
    a = _trainer(noise_seed=78, use_graph=False)
    b = _trainer(use_graph=False)
    t, e, n, _ = _device_draws(78, 0, (2, 8, 16, 16))
    la = float(a.step_from_batch(vae, clap, batch, None, None, None))
    lb = float(b.step_from_batch(vae, clap, batch, n, t, e))
    assert torch.equal(a.last_timesteps, t)
    rel = _rel(a.flat.grads[:a.flat.n], b.flat.grads[:b.flat.n])
    print(f"loss {la:.6g} / {lb:.6g}, flat-gradient relative L2 {rel:.3g}")
    assert abs(la - lb) < 1e-3 * abs(lb) and rel < 1e-3


# ---- 5. resume continues the stream --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resume_runs(tmp_path_factory):
    """the uninterrupted four steps, and two steps saved both ways"""
    from audioldm_with_lora_amd import dp, ops
    data = _batches(4, seed=60)
    whole = _trainer(seed=7, noise_seed=91)
    ts = []
    for lat, emb in data:
        whole.step(lat, None, None, emb)
        ts.append(whole.last_timesteps.clone())
    half = _trainer(seed=7, noise_seed=91)
    for lat, emb in data[:2]:
        half.step(lat, None, None, emb)
    ckpt = str(tmp_path_factory.mktemp("resume") / "checkpoint-2")
    dp.Accelerator().save_state(ckpt, half)
    return dict(data=data, ts=ts, ordinal=ops.philox_state_values(whole.noise_state), params=whole.flat.params.detach().clone(),
                sd=half.state_dict(), ckpt=ckpt)


def _finish_and_compare(tr, runs):
    from audioldm_with_lora_amd import ops
    assert tr.step_count == 2 and ops.philox_state_values(tr.noise_state) == (91, 8)
    for (lat, emb), want in zip(runs["data"][2:], runs["ts"][2:]):
        tr.step(lat, None, None, emb)
        assert torch.equal(tr.last_timesteps, want)
    assert ops.philox_state_values(tr.noise_state) == runs["ordinal"] == (91, 16)
    assert _rel(tr.flat.params.detach(), runs["params"]) < 1e-3


def test_state_dict_resume_continues_the_noise_stream(resume_runs):
    from audioldm_with_lora_amd import ops
    assert resume_runs["sd"]["noise"] == dict(seed=91, ordinal=8, rank=0)
    tr = _trainer(seed=7, noise_seed=5)                        # another seed: the checkpoint's stream replaces it
    with torch.no_grad():
        tr.flat.params.add_(1.0)
    addr = tr.noise_state.data_ptr()
    tr.load_state_dict(resume_runs["sd"])
    assert tr.noise_state.data_ptr() == addr                   # written in place: a captured graph would read the new position
    _finish_and_compare(tr, resume_runs)
    # a checkpoint of rank 1 loads into this rank 0 at the same distance from its base; one without the key leaves the stream alone
    sd = dict(resume_runs["sd"], noise=dict(seed=91, ordinal=2 ** 48 + 8, rank=1))
    tr.load_state_dict(sd)
    assert ops.philox_state_values(tr.noise_state) == (91, 8)
    sd.pop("noise")
    tr.load_state_dict(sd)
    assert ops.philox_state_values(tr.noise_state) == (91, 8)


def test_accelerator_save_state_load_state_continue_the_noise_stream(resume_runs):
    from audioldm_with_lora_amd import dp
    tr = _trainer(seed=7, noise_seed=91)
    with torch.no_grad():
        tr.flat.params.add_(1.0)
    dp.Accelerator().load_state(resume_runs["ckpt"], tr)
    _finish_and_compare(tr, resume_runs)


def test_trainer_of_carries_the_stream_across_a_move():
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.training import trainer_of
    (lat, emb), = _batches(1)
    tr = _trainer(noise_seed=13, noise_offset=0.05, use_graph=False)
    tr.step(lat, None, None, emb)
    unet = tr.unet
    for p, _, _ in tr.flat._plist:                             # what a real move does: the parameters leave the flat buffer
        p.data = p.data.clone()
    assert not tr.flat.intact()
    tr2 = trainer_of(unet)
    assert tr2 is not tr and tr2.noise_seed == 13 and tr2.noise_offset == 0.05
    assert ops.philox_state_values(tr2.noise_state) == (13, 4)


# ---- 6. defaults untouched -----------------------------------------------------------------------------------------------------
NOISING_OPS = ("nhwc_to_nchw_f32", "gaussian_sample", "add_noise_t", "nchw_to_nhwc", "train_noise_fused")


def test_host_noise_keeps_its_launch_sequence_and_never_enters_the_fused_launch(monkeypatch):
    from audioldm_with_lora_amd import _lib, ops
    from audioldm_with_lora_amd._lib import AldmError
    log, entry_calls = [], []
    for name in NOISING_OPS:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda real, name: lambda *a, **kw: (log.append(name), real(*a, **kw))[1])(real, name))
    lib = _lib.load()
    real_entry = lib.aldm_train_noise_fused
    monkeypatch.setattr(lib, "aldm_train_noise_fused", lambda *a: (entry_calls.append(1), real_entry(*a))[1])
    (lat, emb), = _batches(1)
    g = torch.Generator().manual_seed(1)
    noise, t = torch.randn(lat.shape, generator=g), torch.randint(0, T, (2,), generator=g)
    plain = _trainer(use_graph=False)
    assert plain.noise_seed is None and plain.noise_state is None and plain.noise_offset == 0.0
    plain.step(lat, noise, t, emb)
    assert log == ["add_noise_t", "nchw_to_nhwc", "nchw_to_nhwc"] and not entry_calls
    assert "noise" not in plain.state_dict()
    with pytest.raises(AldmError, match="noise_seed"):
        plain.step(lat, None, None, emb)
    del log[:]
    seeded = _trainer(noise_seed=3, use_graph=False)            # a seeded trainer that is handed tensors runs the same sequence
    seeded.step(lat, noise, t, emb)
    assert log == ["add_noise_t", "nchw_to_nhwc", "nchw_to_nhwc"] and not entry_calls
    assert ops.philox_state_values(seeded.noise_state) == (3, 0)
    assert _rel(seeded.flat.params.detach(), plain.flat.params.detach()) < 1e-3
    del log[:]
    seeded.step(lat, None, None, emb)                            # ... and one launch when it draws on the device
    assert log == ["train_noise_fused"] and len(entry_calls) == 1
    offset = _trainer(noise_seed=3, noise_offset=0.1, use_graph=False)
    with pytest.raises(AldmError, match="noise_offset"):
        offset.step(lat, noise, t, emb)
