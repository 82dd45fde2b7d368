"""GPU: long-form and loopable generation through AudioLDMPipeline.__call__ and script/inference.py on a tiny model directory
(tests/synth_checkpoint.py) -- the default path untouched, a windowed clip end to end against the restatement's windowed loop on
the oracle models, a looped clip against the oracle vocoder on the tiled mel, calls with different plans in sequence, the script."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOWED = dict(audio_length_in_s=2.88, window_length_in_s=1.28, window_overlap_in_s=0.32, num_inference_steps=6, guidance_scale=2.5)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """(model directory, the pipeline loaded from it, the oracle UNet / VAE / vocoder with the same weights)"""
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


def _inputs(rows=72):
    g = torch.Generator().manual_seed(19)
    pe = torch.nn.functional.normalize(torch.randn(1, 64, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(1, 64, generator=g), dim=-1)
    return pe, ne, torch.randn(1, 8, rows, 16, generator=g)


def _rel(a, b):
    import conftest
    return conftest.record(float((a.double() - b.double()).norm() / b.double().norm()))


def test_default_path_is_untouched(tiny):
    _, pipe, _ = tiny
    pe, ne, lat = _inputs(32)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio_length_in_s=1.28, num_inference_steps=4, guidance_scale=2.5)
    a = pipe(latents=lat.clone(), **call)
    b = pipe(latents=lat.clone(), window_length_in_s=None, **call)
    assert np.array_equal(a.audios, b.audios) and a.audios.shape == (1, 20480) and not hasattr(a, "plan") and not hasattr(b, "plan")
    with pytest.raises(ValueError):
        pipe(latents=lat.clone(), loop=True, **call)                              # loop needs window_length_in_s


def test_windowed_clip_end_to_end_against_the_oracle(tiny):
    """2.88 s as three windows of 1.28 s (32 rows, overlap 8: offsets 0, 24, 40), 6 DDIM steps: the restatement's windowed loop on the
    oracle UNet, the oracle VAE on every window, the mels blended by the plan at 4 x, the oracle vocoder on the whole mel.  The bound
    is tests/test_gpu_pipeline.py's end-to-end bound for these tiny models at 6 steps."""
    from oracle.ddim import DDIMScheduler as ODDIM
    _, pipe, (ou, ov, oh) = tiny
    pe, ne, lat = _inputs()
    out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat.clone(), **WINDOWED)
    assert out.audios.shape == (1, 46080) and np.isfinite(out.audios).all()
    assert out.plan.key == (72, 32, 8, False) and out.plan.offsets == [0, 24, 40] and out.mel.shape == (1, 288, 64)
    tables, mel_tables = R.tables_of(72, 32, 8), R.tables_of(*R.scaled(72, 32, 8, 4))
    with torch.no_grad():
        x = R.windowed_loop(ou, ODDIM(), lat, pe, ne, 6, 2.5, tables)
        mels = ov.decode(R.gather(x, tables[0], tables[1], dim=2) / ov.config.scaling_factor).sample           # [3, 1, 128, 64]
        mel = R.blend(mels, mel_tables[0], mel_tables[1], 288, mel_tables[2], mel_tables[3], dim=2)            # [1, 1, 288, 64]
        want = oh(mel.squeeze(1)).float()[:, :46080]
    rel = _rel(torch.from_numpy(out.audios), want)
    assert rel < 8e-2, rel


def test_looped_clip_closes_on_itself(tiny):
    """loop=True at 2.88 s (72 rows = 3 strides of 24: offsets 0, 24, 48, the last window over the seam): the audio is the middle third
    of the oracle vocoder's output for the pipeline's own blended mel tiled three times -- sample 0 continues from the last sample.
    Tolerances: the tiny-vocoder parity test's in tests/test_gpu_pipeline.py."""
    _, pipe, (_, _, oh) = tiny
    pe, ne, lat = _inputs()
    out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat.clone(), loop=True, **WINDOWED)
    assert out.plan.key == (72, 32, 8, True) and out.plan.offsets == [0, 24, 48]
    assert out.audios.shape == (1, 46080) and np.isfinite(out.audios).all() and out.mel.shape == (1, 288, 64)
    assert pipe.vocoder_half_field() == 24
    with torch.no_grad():
        want = oh(out.mel.cpu().repeat(1, 3, 1)).float()[:, 46080:2 * 46080]
    got = torch.from_numpy(out.audios)
    assert _rel(got, want) < 3e-2 and float((got - want).abs().max()) < 3e-2
    # the open clip of the same inputs is another clip
    assert not np.array_equal(out.audios, pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat.clone(), **WINDOWED).audios)


def test_calls_with_different_plans_in_sequence(tiny):
    _, pipe, _ = tiny
    pe, ne, lat = _inputs()
    calls = [dict(WINDOWED), dict(WINDOWED, window_overlap_in_s=0.64), dict(WINDOWED, loop=True)]
    first = [pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat.clone(), **c) for c in calls]
    keys = {o.plan.key for o in first}
    assert keys == {(72, 32, 8, False), (72, 32, 16, False), (72, 32, 8, True)}
    windowed = [k for k in pipe._engines if isinstance(k[-1], tuple) and k[-1][:1] == ("windowed",)]
    assert {k[-1][1:] for k in windowed} >= keys
    for c, o in zip(calls, first):
        again = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat.clone(), **c)
        assert np.array_equal(again.audios, o.audios)
    assert not np.array_equal(first[0].audios, first[1].audios)


def test_window_prompts_through_the_text_encoder(tiny):
    _, pipe, _ = tiny
    _, _, lat = _inputs()
    same = pipe(prompt="techno music with heavy bass", latents=lat.clone(), **WINDOWED).audios
    three = pipe(prompt="techno music with heavy bass", latents=lat.clone(), window_prompts=["techno music with heavy bass"] * 3, **WINDOWED).audios
    sched = pipe(prompt="techno music with heavy bass", latents=lat.clone(),
                 window_prompts=["techno music with heavy bass", "a dog barking in the rain", "boom bap"], **WINDOWED).audios
    # (the text tower ran on batches of 1 and of 3: the same prompt, not necessarily the same bits)
    assert float(np.abs(same - three).max()) < 1e-2 * float(np.abs(same).max()) + 1e-4
    assert float(np.abs(three - sched).max()) > 10 * float(np.abs(same - three).max()) and np.isfinite(sched).all()
    with pytest.raises(ValueError):
        pipe(prompt="a dog", latents=lat.clone(), window_prompts=["a", "b"], **WINDOWED)          # three windows


def test_inference_script_window_flags(tiny, tmp_path):
    from scipy.io import wavfile
    from audioldm_with_lora_amd.script import inference
    root, _, _ = tiny
    base = ["--model-dir", root, "--no-lora", "--steps", "4", "--guidance-scale", "2.5", "--seed", "1", "--window-seconds", "1.28",
            "--window-overlap-seconds", "0.32"]
    out = str(tmp_path / "loop.wav")
    inference.main(base + ["--audio-length", "2.88", "--loop", "--output", out])
    sr, wav = wavfile.read(out)
    assert sr == 16000 and wav.shape == (46080,) and wav.dtype == np.float32 and np.isfinite(wav).all()
    out2 = str(tmp_path / "loop_rounded.wav")
    inference.main(base + ["--audio-length", "2.0", "--loop", "--window-prompts", "boom bap|techno|a dog", "--output", out2])
    sr, wav2 = wavfile.read(out2)
    assert sr == 16000 and wav2.shape == (46080,) and np.isfinite(wav2).all()               # 50 rows rounded up to 3 strides = 72 rows
    with pytest.raises(SystemExit):
        inference.main(["--model-dir", root, "--no-lora", "--loop", "--output", out])       # --loop needs --window-seconds
