"""GPU: audio-to-audio and inpainting -- the masked fused steps against an fp32 torch restatement, the begun / masked engine, the
pipeline's identities, parity of the whole call against a CPU restatement (oracle mel + VAE + UNet + vocoder, DDIM and DPM-Solver++
over the suffix with the blend), the engine cache, the script's flags and one full-width run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dpm_restatement import DPMSolverRestatement  # noqa: E402

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _blend_ref(xn, x0, nz, m, a, s):
    """x' = (1 - m) (a x0 + s noise) + m xn, fp32 torch (mask [B, h, w] broadcast over channels-last C)"""
    mm = m[..., None]
    return (1 - mm) * (a * x0 + s * nz) + mm * xn


def _ops_case(seed, B=2, h=6, w=4, C=8):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, h, w, C, generator=g)
    x0 = torch.randn(B, h, w, C, generator=g)
    nz = torch.randn(B, h, w, C, generator=g)
    m = (torch.rand(B, h, w, generator=g) > 0.5).float()
    m[0, 0, :2] = 0.3                                       # fractional values blend
    e = [torch.randn(2 * B, h, w, C, generator=g) for _ in range(3)]
    return x, x0, nz, m, e


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("g_scale", [2.5, 1.0])
def test_masked_kernel_matches_restatement(kind, g_scale):
    """Three steps of the masked launch (counter, ticket, next time-embedding row) against the unmasked launch followed by the blend
    restated in fp32 torch; hist keeps the unblended model output."""
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    s = DDIMScheduler() if kind == "ddim" else DPMSolverMultistepScheduler()
    _, begin = s.get_timesteps(10, 0.5)
    coef = s.coefficient_table(begin_index=begin).cuda()
    ts = s.timesteps[begin:].float().cuda()
    blend = s.blend_table(begin).cuda()
    cfg = g_scale > 1.0
    x, x0, nz, m, e = _ops_case(3)
    B = x.shape[0]
    table = torch.randn(len(ts), 2 * B, 12, generator=torch.Generator().manual_seed(1)).cuda()
    st = {}
    for name in ("masked", "plain"):
        st[name] = dict(x=x.clone().cuda(), hist=torch.zeros_like(x).cuda(), x_in=torch.zeros((2 * B if cfg else B,) + x.shape[1:],
                        dtype=torch.bfloat16, device="cuda"), idx=torch.zeros(1, dtype=torch.int32, device="cuda"),
                        ticket=torch.zeros(1, dtype=torch.int32, device="cuda"), t=torch.zeros(1, device="cuda"),
                        row=torch.zeros(2 * B, 12, device="cuda"))
    x0g, nzg, mg = x0.cuda(), nz.cuda(), m.cuda()
    worst = 0.0
    for k in range(3):
        eps = (e[k] if cfg else e[k][:B]).contiguous().cuda()
        p, q = st["masked"], st["plain"]
        if kind == "ddim":
            ops.ddim_step_fused_masked(eps, p["x"], cfg, g_scale, coef, p["idx"], p["x_in"], table, p["row"], ts, p["t"], p["ticket"],
                                       x0g, nzg, mg, blend)
            ops.ddim_step_fused(eps, q["x"], cfg, g_scale, coef, q["idx"], q["x_in"], table, q["row"], ts, q["t"], q["ticket"])
        else:
            ops.dpm_step_fused_masked(eps, p["x"], cfg, g_scale, coef, p["idx"], p["x_in"], p["hist"], table, p["row"], ts, p["t"],
                                      p["ticket"], x0g, nzg, mg, blend)
            ops.dpm_step_fused(eps, q["x"], cfg, g_scale, coef, q["idx"], q["x_in"], q["hist"], table, q["row"], ts, q["t"], q["ticket"])
            assert torch.equal(p["hist"], q["hist"])           # hist: the unblended model output
        want = _blend_ref(q["x"].cpu(), x0, nz, m, blend[k, 0].item(), blend[k, 1].item())
        worst = max(worst, _rel(p["x"].cpu(), want))
        q["x"].copy_(p["x"])                                 # the plain chain follows the blended trajectory
        xb = p["x"].to(torch.bfloat16)
        assert torch.equal(p["x_in"][:B], xb) and (not cfg or torch.equal(p["x_in"][B:], xb))
        nxt = (k + 1) % len(ts)
        assert int(p["idx"].item()) == nxt and int(p["ticket"].item()) == 0 and float(p["t"].item()) == float(ts[nxt])
        assert torch.equal(p["row"], table[nxt])
    import conftest
    conftest.record(worst, "max_step_rel")
    assert worst <= 1e-5, worst


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_masked_scalar_and_vector_paths_bitwise_equal(kind):
    """VEC = 4 at n elements and VEC = 1 at n + 3 (C = 1 so the mask covers both) agree bit for bit on the shared elements."""
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    s = DDIMScheduler() if kind == "ddim" else DPMSolverMultistepScheduler()
    _, begin = s.get_timesteps(25, 0.6)
    coef = s.coefficient_table(begin_index=begin).cuda()
    ts = s.timesteps[begin:].float().cuda()
    blend = s.blend_table(begin).cuda()
    g = torch.Generator().manual_seed(6)
    n_vec = 4004
    base = [torch.randn(n_vec + 3, generator=g) for _ in range(3)]
    m = torch.rand(n_vec + 3, generator=g)
    m[:100] = 0.0
    m[100:200] = 1.0
    e = [torch.randn(2, n_vec + 3, generator=g) for _ in range(2)]
    res = {}
    for n in (n_vec, n_vec + 3):
        x = base[0][:n].clone().view(1, n, 1).cuda()
        x0, nz, mk = base[1][:n].view(1, n, 1).contiguous().cuda(), base[2][:n].view(1, n, 1).contiguous().cuda(), m[:n].view(1, n).cuda()
        hist = torch.zeros_like(x)
        x_in = torch.zeros(2, n, 1, dtype=torch.bfloat16, device="cuda")
        idx = torch.zeros(1, dtype=torch.int32, device="cuda")
        ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
        t_out = torch.zeros(1, device="cuda")
        for k in range(2):
            eps = e[k][:, :n].contiguous().view(2, n, 1).cuda()
            if kind == "ddim":
                ops.ddim_step_fused_masked(eps, x, True, 2.5, coef, idx, x_in, None, None, ts, t_out, ticket, x0, nz, mk, blend)
            else:
                ops.dpm_step_fused_masked(eps, x, True, 2.5, coef, idx, x_in, hist, None, None, ts, t_out, ticket, x0, nz, mk, blend)
        res[n] = (x[0, :n_vec].cpu(), hist[0, :n_vec].cpu(), x_in[:, :n_vec].cpu())
    for a, b in zip(res[n_vec], res[n_vec + 3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("g_scale", [2.5, 1.0])
def test_all_ones_mask_is_the_unmasked_kernel_and_ends_are_exact(kind, g_scale):
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    s = DDIMScheduler() if kind == "ddim" else DPMSolverMultistepScheduler()
    _, begin = s.get_timesteps(8, 0.5)
    coef = s.coefficient_table(begin_index=begin).cuda()
    ts = s.timesteps[begin:].float().cuda()
    blend = s.blend_table(begin).cuda()
    n = len(ts)
    cfg = g_scale > 1.0
    x, x0, nz, _, e = _ops_case(9)
    B = x.shape[0]
    table = torch.randn(n, 2 * B, 12, generator=torch.Generator().manual_seed(2)).cuda()

    def run(mask):
        st = dict(x=x.clone().cuda(), hist=torch.zeros_like(x).cuda(), x_in=torch.zeros((2 * B if cfg else B,) + x.shape[1:],
                  dtype=torch.bfloat16, device="cuda"), idx=torch.zeros(1, dtype=torch.int32, device="cuda"),
                  ticket=torch.zeros(1, dtype=torch.int32, device="cuda"), t=torch.zeros(1, device="cuda"), row=torch.zeros(2 * B, 12, device="cuda"))
        for k in range(n):
            eps = (e[k % 3] if cfg else e[k % 3][:B]).contiguous().cuda()
            a = (eps, st["x"], cfg, g_scale, coef, st["idx"], st["x_in"])
            tail = (st["row"], ts, st["t"], st["ticket"])
            if kind == "ddim":
                if mask is None:
                    ops.ddim_step_fused(*a, table, *tail)
                else:
                    ops.ddim_step_fused_masked(*a, table, *tail, x0.cuda(), nz.cuda(), mask.cuda(), blend)
            else:
                if mask is None:
                    ops.dpm_step_fused(*a, st["hist"], table, *tail)
                else:
                    ops.dpm_step_fused_masked(*a, st["hist"], table, *tail, x0.cuda(), nz.cuda(), mask.cuda(), blend)
        return {k: v.cpu() for k, v in st.items()}

    plain, ones, zeros = run(None), run(torch.ones(B, *x.shape[1:3])), run(torch.zeros(B, *x.shape[1:3]))
    for k in plain:
        assert torch.equal(plain[k], ones[k]), k
    assert torch.equal(zeros["x"], x0)                     # the last row (1, 0): known == x0, bitwise


# ---- tiny models --------------------------------------------------------------------------------------------------------------
def _tiny():
    from audioldm_with_lora_amd.pipeline import AudioLDMPipeline
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from audioldm_with_lora_amd.vae import AutoencoderKL
    from audioldm_with_lora_amd.vocoder import SpeechT5HifiGan
    from oracle import configs
    from oracle.hifigan import SpeechT5HifiGan as OVoc
    from oracle.unet import UNet2DConditionModel as OUNet
    from oracle.vae import AutoencoderKL as OVae
    torch.manual_seed(17)
    ou, ov, oh = OUNet(**configs.tiny_unet()).eval(), OVae(**configs.tiny_vae()).eval(), OVoc(**configs.tiny_vocoder()).eval()
    g = torch.Generator().manual_seed(18)
    sd = oh.state_dict()
    for k, v in sd.items():
        if k.endswith("weight"):
            fan_in = v[0].numel() if "upsampler" not in k else v.shape[0] * v.shape[2] / 2
            v.copy_(torch.randn(v.shape, generator=g) * (1.0 / fan_in) ** 0.5)
    oh.load_state_dict(sd)
    u, v, h = UNet2DConditionModel(**configs.tiny_unet()), AutoencoderKL(**configs.tiny_vae()), SpeechT5HifiGan(**configs.tiny_vocoder())
    u.load_state_dict(ou.state_dict()); v.load_state_dict(ov.state_dict()); h.load_state_dict(oh.state_dict())
    pipe = AudioLDMPipeline(v, None, None, u, DDIMScheduler(), h).to("cuda")
    return pipe, (ou, ov, oh)


def _inputs(B=2, seconds=1.28, seed=21):
    g = torch.Generator().manual_seed(seed)
    pe = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(B, 64, generator=g), dim=-1)
    n = int(seconds * 16000)
    t = torch.arange(n) / 16000.0
    audio = torch.stack([0.3 * torch.sin(2 * np.pi * (220 + 110 * b) * t) + 0.05 * torch.randn(n, generator=g) for b in range(B)])
    return pe, ne, audio


def _a2a(pipe):
    from audioldm_with_lora_amd.audio2audio import AudioLDMAudioToAudioPipeline
    return AudioLDMAudioToAudioPipeline.from_pipe(pipe)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_engine_begun_and_masked_graph_replay_equals_eager(kind):
    from audioldm_with_lora_amd.engine import DenoiseEngine
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    pipe, _ = _tiny()
    g = torch.Generator().manual_seed(4)
    lat, x0 = torch.randn(2, 8, 16, 16, generator=g), torch.randn(2, 8, 16, 16, generator=g)
    m = (torch.rand(2, 16, 16, generator=g) > 0.5).float()
    pe, ne, _ = _inputs()
    out = []
    for use_graph in (False, True):
        s = DDIMScheduler() if kind == "ddim" else DPMSolverMultistepScheduler()
        eng = DenoiseEngine(pipe._unet, s, 2, 16, 16, 12, 2.5, use_graph=use_graph, begin_index=5, masked=True)
        assert eng.n_steps == 7
        eng.set_condition(pe, ne)
        eng.set_latents(lat)
        eng.set_inpaint(x0, lat, m)
        eng.capture()
        eng.run()
        assert int(eng.step_idx.item()) == 0 and eng.temb[0].shape[0] == 7
        out.append(eng.latents_nchw().cpu())
    assert torch.equal(out[0], out[1]) and torch.isfinite(out[0]).all()
    with pytest.raises(NotImplementedError):
        DenoiseEngine(pipe._unet, DDIMScheduler(), 2, 16, 16, 12, 2.5, chains=2, masked=True)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_identities(kind):
    from audioldm_with_lora_amd.scheduler import DPMSolverMultistepScheduler
    pipe, _ = _tiny()
    if kind == "dpm":
        pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    a2a = _a2a(pipe)
    pe, ne, audio = _inputs()
    eps = torch.randn(2, 8, 32, 16, generator=torch.Generator().manual_seed(5))
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=10, guidance_scale=2.5)
    # strength 1, no mask == text-to-audio from the same eps
    want = pipe(latents=eps.clone(), audio_length_in_s=1.28, **call).audios
    got = a2a(audio=audio, strength=1.0, latents=eps.clone(), **call).audios
    assert np.array_equal(got, want)
    # an all-ones mask == no mask at the same strength
    gen = lambda: torch.Generator().manual_seed(6)
    plain = a2a(audio=audio, strength=0.5, generator=gen(), output_type="latent", **call).audios
    ones = a2a(audio=audio, strength=0.5, generator=gen(), mask=torch.ones(128, 64), output_type="latent", **call).audios
    assert torch.equal(plain, ones)
    # an all-zeros mask keeps the clip: final latents == x0 (scaling_factor * the posterior sample), bitwise
    zeros = a2a(audio=audio, strength=0.5, generator=gen(), mask=torch.zeros(128, 64), output_type="latent", **call).audios
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.mel import LogMelFrontEnd
    mel = LogMelFrontEnd(target_length=128, n_mel=64)(audio.cuda())
    post = torch.randn(2, 8, 32, 16, generator=gen())
    x0 = ops.gaussian_sample(pipe.vae.encode(mel).latent_dist.parameters.float(), post.cuda()) * pipe.vae.config.scaling_factor
    assert torch.equal(zeros, x0)


def _restate(models, kind, audio, pe, ne, strength, mask_mel, N, g_scale, seed):
    """CPU restatement: oracle log-mel -> oracle VAE encode + the same posterior noise -> add_noise at begin -> the scheduler over the
    suffix with the legacy inpaint blend -> oracle decode + vocoder."""
    from oracle.ddim import DDIMScheduler as ODDIM
    from oracle.mel import DSP, log_mel_spec
    from oracle.pipeline import cfg_combine
    ou, ov, oh = models
    B = pe.shape[0]
    dsp = dict(DSP, target_length=128)
    mel = log_mel_spec(audio, dsp)
    gen = torch.Generator().manual_seed(seed)
    dist = ov.encode(mel).latent_dist
    post = torch.randn(dist.mean.shape, generator=gen)
    x0 = (dist.mean + dist.std * post) * ov.config.scaling_factor
    eps = torch.randn(x0.shape, generator=gen)
    init = min(int(N * strength), N)
    begin = max(N - init, 0)
    if kind == "ddim":
        s = ODDIM()
        s.set_timesteps(N)
        noise_to = lambda i: s.add_noise(x0, eps, s.timesteps[i].repeat(B))
    else:
        s = DPMSolverRestatement()
        s.set_timesteps(N)
        s.step_index = begin

        def noise_to(i):
            a, sg = s._alpha_sigma(s.sigmas[i])
            return a * x0 + sg * eps
    m = None
    if mask_mel is not None:
        m = torch.nn.functional.max_pool2d(mask_mel.expand(B, -1, -1)[:, None].float(), 4)
    x = noise_to(begin)
    emb = torch.cat([ne, pe])
    ts = s.timesteps[begin:]
    for k, t in enumerate(ts):
        e = ou(torch.cat([x, x]), t, encoder_hidden_states=None, class_labels=emb)[0]
        x = s.step(cfg_combine(e, g_scale), t, x).prev_sample
        if m is not None:
            known = noise_to(begin + k + 1) if k + 1 < len(ts) else x0
            x = (1 - m) * known + m * x
    wav = oh(ov.decode(x / ov.config.scaling_factor).sample.squeeze(1)).float()[:, :20480]
    return x, wav, x0, m


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("masked", [False, True], ids=["style", "inpaint"])
def test_pipeline_parity_with_cpu_restatement(kind, masked):
    from audioldm_with_lora_amd.audio2audio import regeneration_mask
    from audioldm_with_lora_amd.scheduler import DPMSolverMultistepScheduler
    pipe, models = _tiny()
    if kind == "dpm":
        pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    a2a = _a2a(pipe)
    pe, ne, audio = _inputs()
    mask = regeneration_mask(128, 64, seconds=(0.4, 0.8)) if masked else None
    N = 12
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, strength=0.5, mask=mask, num_inference_steps=N, guidance_scale=2.5)
    lat = a2a(generator=torch.Generator().manual_seed(8), output_type="latent", **call).audios.cpu()
    wav = torch.from_numpy(a2a(generator=torch.Generator().manual_seed(8), **call).audios)
    with torch.no_grad():
        x_ref, wav_ref, x0_ref, m = _restate(models, kind, audio, pe, ne, 0.5, mask, N, 2.5, 8)
    r_lat, r_wav = _rel(lat, x_ref), _rel(wav, wav_ref)
    import conftest
    conftest.record(r_lat, "latents_rel")
    conftest.record(r_wav, "audio_rel")
    assert wav.shape == (2, 20480) and torch.isfinite(wav).all()
    assert r_lat < 8e-2 and r_wav < 8e-2, (r_lat, r_wav)
    if masked:
        keep = (m == 0).expand_as(lat)
        assert keep.any() and (~keep).any()
        r_keep = _rel(lat[keep], x_ref[keep])
        conftest.record(r_keep, "kept_rel")
        assert r_keep < 4e-2, r_keep


def test_engine_cache_hygiene():
    """plain, strength 0.3 and masked calls alternating on one pipeline give what fresh pipelines give"""
    from audioldm_with_lora_amd.audio2audio import regeneration_mask
    pe, ne, audio = _inputs()
    mask = regeneration_mask(128, 64, bands=(0.5, 1.0))
    calls = [dict(strength=1.0), dict(strength=0.3), dict(strength=0.3, mask=mask), dict(strength=1.0), dict(strength=0.3, mask=mask),
             dict(strength=0.3)]
    base = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, num_inference_steps=10, guidance_scale=2.5, output_type="latent")
    pipe, _ = _tiny()
    a2a = _a2a(pipe)
    shared = [a2a(generator=torch.Generator().manual_seed(3), **base, **c).audios.cpu() for c in calls]
    assert len(a2a._engines) == 3 and not pipe._engines
    for c, got in zip(calls[:3], shared[:3]):
        fresh_pipe, _ = _tiny()
        want = _a2a(fresh_pipe)(generator=torch.Generator().manual_seed(3), **base, **c).audios.cpu()
        assert torch.equal(got, want)
    assert torch.equal(shared[0], shared[3]) and torch.equal(shared[2], shared[4]) and torch.equal(shared[1], shared[5])
    assert not torch.equal(shared[1], shared[2])


def test_argument_errors():
    pipe, _ = _tiny()
    a2a = _a2a(pipe)
    pe, ne, audio = _inputs()
    base = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=10)
    for bad in [dict(audio=audio, sampling_rate=22050), dict(audio=audio, strength=0.05), dict(audio=audio, strength=1.5),
                dict(audio=audio[:1].expand(3, -1)), dict(audio=audio, mask=torch.ones(100, 64)), dict(),
                dict(audio=audio, latents=torch.zeros(2, 8, 8, 16))]:
        with pytest.raises(ValueError):
            a2a(**base, **bad)


def test_inference_script_audio_to_audio_flags(tmp_path):
    from scipy.io import wavfile
    import synth_checkpoint
    from audioldm_with_lora_amd.script import inference
    root = str(tmp_path / "m")
    synth_checkpoint.write_model_dir(root)
    src = str(tmp_path / "in.wav")
    n = 20480
    wavfile.write(src, 16000, (0.3 * np.sin(2 * np.pi * 330 * np.arange(n) / 16000)).astype(np.float32))
    for extra in (["--strength", "0.6"], ["--regenerate-seconds", "0.2,0.6"], ["--regenerate-bands", "0.5,1.0", "--strength", "0.8"]):
        out = str(tmp_path / f"out_{len(extra)}_{extra[0][2:]}.wav")
        inference.main(["--model-dir", root, "--no-lora", "--steps", "5", "--guidance-scale", "2.5", "--init-audio", src,
                        "--output", out, "--seed", "1"] + extra)
        sr, wav = wavfile.read(out)
        assert sr == 16000 and wav.shape == (n,) and wav.dtype == np.float32 and np.isfinite(wav).all()


def test_full_width_unet_three_masked_steps_finite():
    """configs.UNET at the config-2 shape (4 x 10 s, CFG), random weights, 3 masked DDIM steps of a 6-step schedule at strength 0.5"""
    from audioldm_with_lora_amd.audio2audio import reduce_mask, regeneration_mask
    from audioldm_with_lora_amd.engine import DenoiseEngine
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    torch.manual_seed(1234)
    unet = UNet2DConditionModel().cuda()
    g = torch.Generator().manual_seed(0)
    lat, x0 = torch.randn(4, 8, 250, 16, generator=g), torch.randn(4, 8, 250, 16, generator=g)
    pe = torch.nn.functional.normalize(torch.randn(4, 512, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(4, 512, generator=g), dim=-1)
    s = DDIMScheduler()
    _, begin = s.get_timesteps(6, 0.5)
    m = reduce_mask(regeneration_mask(1000, 64, seconds=(2.0, 6.0))[None].expand(4, -1, -1), 4)
    eng = DenoiseEngine(unet, s, 4, 250, 16, 6, 2.5, begin_index=begin, masked=True)
    eng.set_condition(pe, ne)
    eng.set_latents(lat)
    eng.set_inpaint(x0, lat, m)
    eng.capture()
    out = eng.run()
    torch.cuda.synchronize()
    assert eng.n_steps == 3 and out.shape == (4, 250, 16, 8) and torch.isfinite(out).all() and int(eng.step_idx.item()) == 0
    got = eng.latents_nchw().cpu()
    keep = (m == 0)[:, None].expand_as(got)
    assert torch.equal(got[keep], x0[keep])                     # the kept region ends on the clip's latents exactly


def test_dpm_add_noise_matches_add_noise_coefficients_in_each_case():
    """diffusers' three cases: set_begin_index alone (the begin index), set_begin_index then one step() (the step index that step
    left: the inpaint loop's timesteps[i + 1]), no begin index (each timestep's own index)."""
    from audioldm_with_lora_amd.scheduler import DPMSolverMultistepScheduler
    g = torch.Generator().manual_seed(11)
    x0, nz, e = (torch.randn(2, 8, 6, 4, generator=g) for _ in range(3))

    def want(idx, s):
        rows = [s.add_noise_coefficients(i) for i in idx]
        a = torch.tensor([float(r[0]) for r in rows]).view(-1, 1, 1, 1)
        sg = torch.tensor([float(r[1]) for r in rows]).view(-1, 1, 1, 1)
        return a * x0 + sg * nz

    s = DPMSolverMultistepScheduler()
    s.set_timesteps(10)
    ts = s.timesteps
    s.set_begin_index(4)
    got = s.add_noise(x0.cuda(), nz.cuda(), ts[4:5]).cpu()
    torch.testing.assert_close(got, want([4, 4], s), rtol=1e-6, atol=1e-6)
    s.step(e.cuda(), ts[4], x0.cuda())                          # a begun schedule's first step runs at the begin index ...
    assert s.step_index == 5
    got = s.add_noise(x0.cuda(), nz.cuda(), ts[5:6]).cpu()      # ... and add_noise then noises to timesteps[5]
    torch.testing.assert_close(got, want([5, 5], s), rtol=1e-6, atol=1e-6)
    assert not torch.allclose(got, want([4, 4], s), rtol=1e-3, atol=1e-3)
    s.set_timesteps(10)                                         # no begin index: each timestep's own index
    got = s.add_noise(x0.cuda(), nz.cuda(), ts[[3, 7]]).cpu()
    torch.testing.assert_close(got, want([3, 7], s), rtol=1e-6, atol=1e-6)


def test_mask_follows_the_audio_batching_rule():
    """with num_waveforms_per_prompt > 1 a per-prompt mask [prompts, frames, n_mel] is repeated like per-prompt audio"""
    from audioldm_with_lora_amd.audio2audio import regeneration_mask
    pipe, _ = _tiny()
    a2a = _a2a(pipe)
    pe, ne, audio = _inputs(B=1)
    per_prompt = torch.stack([regeneration_mask(128, 64, seconds=(0.2, 0.6))])
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, strength=0.6, num_inference_steps=10, guidance_scale=2.5,
                num_waveforms_per_prompt=2, output_type="latent")
    a = a2a(generator=torch.Generator().manual_seed(4), mask=per_prompt, **call).audios
    b = a2a(generator=torch.Generator().manual_seed(4), mask=per_prompt.expand(2, -1, -1), **call).audios
    assert a.shape == (2, 8, 32, 16) and torch.equal(a, b)
    with pytest.raises(ValueError):
        a2a(generator=torch.Generator().manual_seed(4), mask=per_prompt.expand(3, -1, -1), **call)
