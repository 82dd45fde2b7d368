"""GPU: long-form audio-to-audio through AudioLDMAudioToAudioPipeline.__call__ and script/inference.py on a tiny model directory
(tests/synth_checkpoint.py): a recording of 2.88 s (72 latent rows) as windows of 1.28 s -- the one-window identity with the plain
call, the windowed encode and the whole call against the restatement on the oracle models (tests/longform_a2a_restatement.py),
continuation of a 1.28 s recording, a looped clip, the engine cache, the script, and one full-width run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_a2a_restatement as A  # noqa: E402
import longform_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOWED = dict(window_length_in_s=1.28, window_overlap_in_s=0.32, guidance_scale=2.5)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """(model directory, the text-to-audio pipeline loaded from it, the oracle UNet / VAE / vocoder with the same weights)"""
    import synth_checkpoint
    from audioldm_with_lora_amd.pipeline import AudioLDMPipeline
    from oracle import configs
    from oracle.hifigan import SpeechT5HifiGan as OVoc
    from oracle.unet import UNet2DConditionModel as OUNet
    from oracle.vae import AutoencoderKL as OVae
    root = str(tmp_path_factory.mktemp("model"))
    src = synth_checkpoint.write_model_dir(root)
    ou, ov, oh = OUNet(**configs.tiny_unet()).eval(), OVae(**configs.tiny_vae()).eval(), OVoc(**configs.tiny_vocoder()).eval()
    ou.load_state_dict(src["unet"].state_dict())
    ov.load_state_dict(src["vae"].state_dict())
    oh.load_state_dict(src["vocoder"].state_dict())
    return root, AudioLDMPipeline.from_pretrained(root).to("cuda"), (ou, ov, oh)


def _a2a(pipe, kind="ddim"):
    from audioldm_with_lora_amd.audio2audio import AudioLDMAudioToAudioPipeline
    from audioldm_with_lora_amd.scheduler import DPMSolverMultistepScheduler
    a2a = AudioLDMAudioToAudioPipeline.from_pipe(pipe)
    if kind == "dpm":
        a2a.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    return a2a


def _inputs(seconds=2.88, seed=21):
    g = torch.Generator().manual_seed(seed)
    pe = torch.nn.functional.normalize(torch.randn(1, 64, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(1, 64, generator=g), dim=-1)
    n = int(round(seconds * 16000))
    t = torch.arange(n) / 16000.0
    audio = (0.3 * torch.sin(2 * np.pi * (220 + 60 * t) * t) + 0.05 * torch.randn(n, generator=g))[None]
    return pe, ne, audio


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _gen(seed=8):
    return torch.Generator().manual_seed(seed)


def test_one_window_call_equals_the_plain_call_bitwise(tiny):
    """a recording no longer than the window: one window of weight 1.0 -- the windowed encode, engine and launches reproduce the
    plain call's latents bit for bit, masked and unmasked"""
    from audioldm_with_lora_amd.audio2audio import regeneration_mask
    _, pipe, _ = tiny
    a2a = _a2a(pipe)
    pe, ne, audio = _inputs(1.28)
    for mask in (None, regeneration_mask(128, 64, seconds=(0.4, 0.8))):
        call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, strength=0.5, mask=mask, num_inference_steps=10, guidance_scale=2.5,
                    output_type="latent")
        plain = a2a(generator=_gen(), **call)
        one = a2a(generator=_gen(), window_length_in_s=1.28, **call)
        assert one.plan.K == 1 and one.plan.key == (32, 32, 0, False) and not hasattr(plain, "plan")
        assert plain.audios.shape == (1, 8, 32, 16) and torch.equal(plain.audios, one.audios)
        # None is today's path
        assert torch.equal(a2a(generator=_gen(), window_length_in_s=None, **call).audios, plain.audios)
    with pytest.raises(ValueError):
        a2a(generator=_gen(), loop=True, **call)                                 # loop needs window_length_in_s


def test_windowed_encode_against_the_restatement(tiny):
    """the long clip's moments and x0 (through an all-zeros mask, which returns x0 exactly) against the oracle mel + the oracle VAE on
    every window, blended in float64; the bound is tests/test_gpu_pipeline.py::test_vae_encode_matches_oracle's"""
    import conftest
    from audioldm_with_lora_amd.mel import LogMelFrontEnd
    _, pipe, (_, ov, _) = tiny
    a2a = _a2a(pipe)
    pe, ne, audio = _inputs()
    plan, mel_plan = a2a.window_plan(2.88, 1.28, 0.32)
    assert plan.key == (72, 32, 8, False) and plan.offsets == [0, 24, 40]
    mel = LogMelFrontEnd(device="cuda", target_length=288, n_mel=64)(audio.cuda())
    params = a2a.encode_windows(mel, plan, mel_plan)
    assert params.shape == (1, 16, 72, 16)
    got_mean, got_logvar = params.chunk(2, dim=1)
    got_std = torch.exp(0.5 * got_logvar.clamp(-30.0, 20.0))
    x0 = a2a(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, strength=0.5, mask=torch.zeros(288, 64), num_inference_steps=4,
             generator=_gen(), output_type="latent", **WINDOWED).audios.cpu()
    post = torch.randn(1, 8, 72, 16, generator=_gen())
    with torch.no_grad():
        mean, std, want = A.windowed_encode(ov, audio, 288, A.tables_from_plan(plan), A.tables_from_plan(mel_plan), post)
    r_mean, r_std, r_x0 = _rel(got_mean.cpu(), mean), _rel(got_std.cpu(), std), _rel(x0, want)
    conftest.record(r_mean, "mean_rel")
    conftest.record(r_std, "std_rel")
    conftest.record(r_x0, "x0_rel")
    assert r_mean < 4e-2 and r_std < 4e-2 and r_x0 < 4e-2, (r_mean, r_std, r_x0)


def _restate(models, kind, audio, pe, ne, mask_mel, N, begin, seed):
    """CPU restatement of the windowed call: the windowed encode with the call's posterior noise, the windowed loop over the suffix
    with the blend, then the oracle VAE on every window, the mels blended at 4 x and the oracle vocoder on the whole mel"""
    ou, ov, oh = models
    tables, mel_tables = R.tables_of(72, 32, 8), R.tables_of(*R.scaled(72, 32, 8, 4))
    gen = _gen(seed)
    post = torch.randn(1, 8, 72, 16, generator=gen)
    eps = torch.randn(1, 8, 72, 16, generator=gen)
    _, _, x0 = A.windowed_encode(ov, audio, 288, tables, mel_tables, post)
    m = None if mask_mel is None else torch.nn.functional.max_pool2d(mask_mel[None, None].float(), 4)[:, 0]
    x = A.windowed_a2a_loop(ou, R.make_restatement(kind), kind, x0, eps, pe, ne, N, begin, 2.5, tables, mask=m)
    mels = ov.decode(R.gather(x, tables[0], tables[1], dim=2) / ov.config.scaling_factor).sample
    mel = R.blend(mels, mel_tables[0], mel_tables[1], 288, mel_tables[2], mel_tables[3], dim=2)
    return x, oh(mel.squeeze(1)).float()[:, :46080], x0, m


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("masked", [False, True], ids=["style", "inpaint"])
def test_windowed_call_parity_with_the_restatement(tiny, kind, masked):
    """12 steps at strength 0.5 over three windows; the bounds are tests/test_gpu_audio2audio.py::
    test_pipeline_parity_with_cpu_restatement's: the same models, step count and strength"""
    import conftest
    from audioldm_with_lora_amd.audio2audio import regeneration_mask
    _, pipe, models = tiny
    a2a = _a2a(pipe, kind)
    pe, ne, audio = _inputs()
    mask = regeneration_mask(288, 64, seconds=(0.9, 2.0)) if masked else None
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, strength=0.5, mask=mask, num_inference_steps=12, **WINDOWED)
    out = a2a(generator=_gen(), output_type="latent", **call)
    lat = out.audios.cpu()
    full = a2a(generator=_gen(), **call)
    wav = torch.from_numpy(full.audios)
    assert out.plan.key == full.plan.key == (72, 32, 8, False) and out.mel is None and full.mel.shape == (1, 288, 64)
    with torch.no_grad():
        x_ref, wav_ref, _, m = _restate(models, kind, audio, pe, ne, mask, 12, 6, 8)
    r_lat, r_wav = _rel(lat, x_ref), _rel(wav, wav_ref)
    conftest.record(r_lat, "latents_rel")
    conftest.record(r_wav, "audio_rel")
    print(f"{kind} masked={masked}: latents {r_lat:.3e}, audio {r_wav:.3e}")
    assert lat.shape == (1, 8, 72, 16) and wav.shape == (1, 46080) and torch.isfinite(wav).all()
    assert r_lat < 8e-2 and r_wav < 8e-2, (r_lat, r_wav)
    if masked:
        keep = (m == 0)[:, None].expand_as(lat)
        assert keep.any() and (~keep).any()
        r_keep = _rel(lat[keep], x_ref[keep])
        conftest.record(r_keep, "kept_rel")
        assert r_keep < 4e-2, r_keep


def test_continuation_keeps_the_recording_and_generates_the_tail(tiny):
    """a 1.28 s recording extended to 2.88 s: strength 1.0 and the continuation mask.  The kept latent rows are the recording's own
    x0 -- what an all-zeros mask returns for the same call -- exactly; behind them the clip is no longer the encoding of silence."""
    from audioldm_with_lora_amd.audio2audio import continuation_mask
    _, pipe, _ = tiny
    a2a = _a2a(pipe)
    pe, ne, audio = _inputs(1.28)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, audio_length_in_s=2.88, strength=1.0, num_inference_steps=6, **WINDOWED)
    ext = a2a(generator=_gen(), mask=continuation_mask(288, 64, 1.28), output_type="latent", **call).audios.cpu()
    x0 = a2a(generator=_gen(), mask=torch.zeros(288, 64), output_type="latent", **call).audios.cpu()
    assert ext.shape == x0.shape == (1, 8, 72, 16) and torch.isfinite(ext).all()
    assert torch.equal(ext[:, :, :32], x0[:, :, :32])
    assert not torch.equal(ext[:, :, 32:], x0[:, :, 32:]) and _rel(ext[:, :, 32:], x0[:, :, 32:]) > 0.1
    out = a2a(generator=_gen(), mask=continuation_mask(288, 64, 1.28), **call)
    assert out.audios.shape == (1, 46080) and np.isfinite(out.audios).all() and out.plan.key == (72, 32, 8, False)
    with pytest.raises(ValueError, match=r"\[288, 64\]"):
        a2a(generator=_gen(), mask=continuation_mask(128, 64, 0.64), **call)    # a mask at the recording's height


def test_looped_call_returns_the_rounded_up_clip(tiny):
    _, pipe, _ = tiny
    a2a = _a2a(pipe)
    pe, ne, audio = _inputs(2.0)
    out = a2a(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, strength=0.6, num_inference_steps=5, loop=True, generator=_gen(), **WINDOWED)
    assert out.plan.key == (72, 32, 8, True) and out.plan.offsets == [0, 24, 48]              # 50 rows rounded up to 3 strides
    assert out.audios.shape == (1, 46080) and np.isfinite(out.audios).all() and out.mel.shape == (1, 288, 64)


def test_engine_cache_hygiene_across_plain_and_windowed_calls(tiny):
    """plain calls (the first 1.28 s of the recording) and windowed calls (all 2.88 s), masked and unmasked, alternating on one
    pipeline give what fresh pipelines give; plain keys stay as they are, windowed keys end with the plan"""
    from audioldm_with_lora_amd.audio2audio import regeneration_mask
    _, pipe, _ = tiny
    pe, ne, audio = _inputs()
    mask, short_mask = regeneration_mask(288, 64, bands=(0.5, 1.0)), regeneration_mask(128, 64, bands=(0.5, 1.0))
    plain, long = dict(audio=audio[:, :20480]), dict(WINDOWED, audio=audio)
    calls = [plain, long, dict(plain, mask=short_mask), dict(long, mask=mask), plain, dict(long, mask=mask), long,
             dict(long, window_overlap_in_s=0.64)]
    base = dict(prompt_embeds=pe, negative_prompt_embeds=ne, strength=0.3, num_inference_steps=10, guidance_scale=2.5, output_type="latent")
    a2a = _a2a(pipe)
    before = set(pipe._engines)
    shared = [a2a(generator=_gen(3), **dict(base, **c)).audios.cpu() for c in calls]
    assert len(a2a._engines) == 5 and set(pipe._engines) == before
    windowed = [k for k in a2a._engines if isinstance(k[-1], tuple) and k[-1][:1] == ("windowed",)]
    assert len(windowed) == 3 and {k[-1][1:] for k in windowed} == {(72, 32, 8, False), (72, 32, 16, False)}
    assert all(len(k) == 9 for k in a2a._engines if k not in windowed)
    for c, got in zip(calls[:4], shared[:4]):
        want = _a2a(pipe)(generator=_gen(3), **dict(base, **c)).audios.cpu()
        assert torch.equal(got, want)
    assert torch.equal(shared[0], shared[4]) and torch.equal(shared[3], shared[5]) and torch.equal(shared[1], shared[6])
    assert not torch.equal(shared[1], shared[3]) and not torch.equal(shared[1], shared[7]) and shared[0].shape == (1, 8, 32, 16)


def test_per_window_prompts(tiny):
    _, pipe, _ = tiny
    a2a = _a2a(pipe)
    pe, ne, audio = _inputs()
    call = dict(negative_prompt_embeds=ne, audio=audio, strength=0.5, num_inference_steps=6, output_type="latent", **WINDOWED)
    same = a2a(prompt_embeds=pe, generator=_gen(), **call).audios
    three = a2a(prompt_embeds=pe, window_prompt_embeds=pe[:, None, :].repeat(1, 3, 1), generator=_gen(), **call).audios
    sched = pe[:, None, :].repeat(1, 3, 1)
    sched[:, 2] = -sched[:, 2]                                      # another prompt for the last window (rows 40 .. 71)
    other = a2a(prompt_embeds=pe, window_prompt_embeds=sched, generator=_gen(), **call).audios
    assert torch.equal(same, three) and not torch.equal(same[:, :, 40:], other[:, :, 40:]) and torch.isfinite(other).all()
    with pytest.raises(ValueError):
        a2a(prompt_embeds=pe, window_prompt_embeds=pe[:, None, :].repeat(1, 2, 1), generator=_gen(), **call)       # three windows


def test_inference_script_long_form_audio_to_audio(tiny, tmp_path):
    import multi_adapter_restatement as mar
    from safetensors.torch import save_file
    from scipy.io import wavfile
    from audioldm_with_lora_amd.script import inference
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    root, _, _ = tiny
    src = str(tmp_path / "in.wav")
    n = 46080
    wavfile.write(src, 16000, (0.3 * np.sin(2 * np.pi * 330 * np.arange(n) / 16000)).astype(np.float32))
    short = str(tmp_path / "short.wav")
    wavfile.write(short, 16000, (0.3 * np.sin(2 * np.pi * 330 * np.arange(20480) / 16000)).astype(np.float32))
    base = ["--model-dir", root, "--no-lora", "--steps", "4", "--guidance-scale", "2.5", "--seed", "1", "--window-seconds", "1.28",
            "--window-overlap-seconds", "0.32"]
    runs = {"style": ["--init-audio", src, "--strength", "0.6"],
            "inpaint": ["--init-audio", src, "--regenerate-seconds", "0.9,2.0", "--regenerate-bands", "0.5,1.0", "--strength", "0.8"],
            "loop_prompts": ["--init-audio", src, "--loop", "--window-prompts", "boom bap|techno|a dog"],
            "extend": ["--init-audio", short, "--extend-to-seconds", "2.88"]}
    for name, extra in runs.items():
        out = str(tmp_path / f"{name}.wav")
        inference.main(base + extra + ["--output", out])
        sr, wav = wavfile.read(out)
        assert sr == 16000 and wav.shape == (n,) and wav.dtype == np.float32 and np.isfinite(wav).all(), name
    # --adapters with --window-seconds: text-to-audio, and from the recording; one clip per routing entry
    unet = UNet2DConditionModel.from_pretrained(root, subfolder="unet")
    adapter = str(tmp_path / "a.safetensors")
    save_file({k: v.contiguous() for k, v in mar.peft_state_dict(mar.make_adapter(unet, 4, 8, mar.TARGETS4, seed=4)).items()}, adapter)
    routed = [a for a in base if a != "--no-lora"] + ["--lora", f"a={adapter}", "--adapters", "a,base", "--prompt", "boom bap"]
    for name, extra in (("t2a", ["--audio-length", "2.88"]), ("a2a", ["--init-audio", src]), ("ext", ["--init-audio", short, "--extend-to-seconds", "2.88"])):
        out = str(tmp_path / f"routed_{name}.wav")
        inference.main(routed + extra + ["--output", out])
        clips = [wavfile.read(str(tmp_path / f"routed_{name}_{i}.wav"))[1] for i in range(2)]
        assert all(c.shape == (n,) and np.isfinite(c).all() for c in clips) and not np.array_equal(clips[0], clips[1]), name
    with pytest.raises(SystemExit):
        inference.main(base + ["--extend-to-seconds", "2.88", "--output", str(tmp_path / "x.wav")])       # needs --init-audio


def test_full_width_unet_three_masked_windowed_steps_finite():
    """configs.UNET with random weights, B = 1, CFG: two windows of 256 rows over 448, 3 masked DDIM steps of a 6-step schedule at
    strength 0.5"""
    from audioldm_with_lora_amd.engine import WindowedAudioToAudioEngine
    from audioldm_with_lora_amd.longform import WindowPlan
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    torch.manual_seed(1234)
    unet = UNet2DConditionModel().cuda()
    plan = WindowPlan(448, 256, 64)
    assert plan.K == 2 and plan.offsets == [0, 192]
    g = torch.Generator().manual_seed(0)
    lat, x0 = torch.randn(1, 8, 448, 16, generator=g), torch.randn(1, 8, 448, 16, generator=g)
    pe = torch.nn.functional.normalize(torch.randn(1, 512, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(1, 512, generator=g), dim=-1)
    m = torch.ones(1, 448, 16)
    m[:, :200] = 0.0
    s = DDIMScheduler()
    _, begin = s.get_timesteps(6, 0.5)
    eng = WindowedAudioToAudioEngine(unet, s, 1, plan, 16, 6, 2.5, begin_index=begin, masked=True)
    eng.set_condition(pe, ne)
    eng.set_latents(lat)
    eng.set_inpaint(x0, lat, m)
    eng.capture()
    out = eng.run()
    torch.cuda.synchronize()
    assert eng.n_steps == 3 and out.shape == (1, 448, 16, 8) and torch.isfinite(out).all()
