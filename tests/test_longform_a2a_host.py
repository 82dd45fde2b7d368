"""Host-only pieces of long-form audio-to-audio (no GPU, no shared library): the long clip's mask rules, the
continuation mask of --extend-to-seconds, the script's flag combinations, the windowed engine-cache key, the engine subclass that
lifts the base class's refusal, and the absence of a CPU path."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from audioldm_with_lora_amd import audio2audio  # noqa: E402
from audioldm_with_lora_amd.audio2audio import (AudioLDMAudioToAudioPipeline, continuation_mask, reduce_mask,  # noqa: E402
                                                regeneration_mask)
from audioldm_with_lora_amd.longform import WindowPlan  # noqa: E402
from audioldm_with_lora_amd.scheduler import DDIMScheduler  # noqa: E402


def _bare_pipeline():
    """the pipeline's host state without any module: what _latent_mask, window_plan and engine() read"""
    p = AudioLDMAudioToAudioPipeline.__new__(AudioLDMAudioToAudioPipeline)
    p.vae_scale_factor = 4
    p.vocoder = SimpleNamespace(config=SimpleNamespace(upsample_rates=[5, 4, 2, 2, 2], sampling_rate=16000, model_in_dim=64))
    p.unet = SimpleNamespace(cfg={"in_channels": 8}, plan_version=0)
    p.scheduler = DDIMScheduler()
    p.device = torch.device("cpu")
    p._engines, p._plans = {}, {}
    return p


# ---- the mask of the long clip -----------------------------------------------------------------------------------------------
def test_long_mask_height_and_batching_errors():
    p = _bare_pipeline()
    plan, mel_plan = p.window_plan(2.88, 1.28, 0.32)
    assert plan.key == (72, 32, 8, False) and mel_plan.key == (288, 128, 32, False)
    height = plan.rows * p.vae_scale_factor
    m = p._latent_mask(regeneration_mask(height, 64, seconds=(1.0, 2.0)), 2, 1, height, 64)
    assert m.shape == (2, 72, 16) and m[0, :25].sum() == 0 and m[0, 25:50].min() == 1 and m[0, 50:].sum() == 0
    # a mask at the RECORDING's height (or the window's) is not the long clip's: the error names the expected height
    for wrong in (128, 200, 289):
        with pytest.raises(ValueError, match=r"\[288, 64\]"):
            p._latent_mask(torch.ones(wrong, 64), 2, 1, height, 64)
    with pytest.raises(ValueError, match=r"\[288, 64\]"):
        p._latent_mask(torch.ones(288, 32), 2, 1, height, 64)
    # the batching rule of the plain call: shared, per prompt (repeated over num_waveforms_per_prompt), per sample
    per_prompt = torch.stack([regeneration_mask(height, 64, seconds=(0.0, 1.0)), regeneration_mask(height, 64, seconds=(1.0, 2.0))])
    got = p._latent_mask(per_prompt, 4, 2, height, 64)
    assert got.shape == (4, 72, 16) and torch.equal(got[0], got[1]) and torch.equal(got[2], got[3]) and not torch.equal(got[1], got[2])
    assert torch.equal(p._latent_mask(per_prompt, 2, 1, height, 64), reduce_mask(per_prompt, 4))
    with pytest.raises(ValueError, match="batch 3"):
        p._latent_mask(torch.ones(3, 288, 64), 4, 2, height, 64)
    # a looped plan rounds the clip up: the mask is the LONGER clip's
    looped, _ = p.window_plan(2.0, 1.28, 0.32, loop=True)
    assert looped.rows == 72
    with pytest.raises(ValueError, match=r"\[288, 64\]"):
        p._latent_mask(torch.ones(200, 64), 1, 1, looped.rows * 4, 64)


def test_continuation_mask():
    """--extend-to-seconds: keep the recording's frames, regenerate everything behind them"""
    m = continuation_mask(4000, 64, 10.0)
    assert torch.equal(m, regeneration_mask(4000, 64, seconds=(10.0, 40.0)))
    assert m.shape == (4000, 64) and m[:1000].sum() == 0 and m[1000:].min() == 1
    # a recording that ends inside a frame / a latent row: that frame and that latent row are regenerated, none before it
    m = continuation_mask(288, 64, 1.285)
    assert m[:128].sum() == 0 and m[128:].min() == 1
    lat = reduce_mask(m[None], 4)[0]
    assert lat[:32].sum() == 0 and lat[32:].min() == 1
    lat = reduce_mask(continuation_mask(288, 64, 1.30)[None], 4)[0]        # frame 130 sits in latent row 32
    assert lat[:32].sum() == 0 and lat[32:].min() == 1
    for bad in (0.0, -1.0, 2.88, 5.0):
        with pytest.raises(ValueError):
            continuation_mask(288, 64, bad)


# ---- the script's flags ----------------------------------------------------------------------------------------------------------
BASE = ["--model-dir", "m", "--no-lora"]


@pytest.mark.parametrize("flags", [
    ["--init-audio", "a.wav", "--window-seconds", "10.24"],
    ["--init-audio", "a.wav", "--window-seconds", "10.24", "--window-overlap-seconds", "2.56", "--loop", "--window-prompts", "a|b|c"],
    ["--init-audio", "a.wav", "--window-seconds", "10.24", "--strength", "0.7", "--regenerate-seconds", "5,20", "--regenerate-bands", "0.5,1"],
    ["--init-audio", "a.wav", "--window-seconds", "10.24", "--extend-to-seconds", "40"],
    ["--init-audio", "a.wav", "--window-seconds", "10.24", "--extend-to-seconds", "40", "--lora", "x=p", "--adapters", "x,base"],
    ["--window-seconds", "10.24", "--audio-length", "60", "--lora", "x=p", "--adapters", "x,base"],
    ["--init-audio", "a.wav", "--strength", "0.4"],
], ids=["a2a_windowed", "a2a_windowed_all_window_flags", "a2a_windowed_masks", "extend", "extend_adapters", "t2a_windowed_adapters", "a2a_plain"])
def test_script_accepts(flags):
    from audioldm_with_lora_amd.script import inference
    args = inference.parse_args(BASE + flags)
    assert args.model_dir == "m"
    if "--extend-to-seconds" in flags:
        assert args.extend_to_seconds == 40.0


@pytest.mark.parametrize("flags", [
    ["--extend-to-seconds", "40"],                                                        # needs both
    ["--extend-to-seconds", "40", "--init-audio", "a.wav"],                               # needs --window-seconds
    ["--extend-to-seconds", "40", "--window-seconds", "10.24"],                           # needs --init-audio
    ["--extend-to-seconds", "40", "--init-audio", "a.wav", "--window-seconds", "10.24", "--regenerate-seconds", "1,2"],
    ["--extend-to-seconds", "-1", "--init-audio", "a.wav", "--window-seconds", "10.24"],
    ["--init-audio", "a.wav", "--loop"],                                                  # the window flags need --window-seconds
    ["--init-audio", "a.wav", "--window-prompts", "a|b"],
    ["--init-audio", "a.wav", "--window-overlap-seconds", "1"],
    ["--window-seconds", "10.24", "--regenerate-seconds", "1,2"],                         # the mask flags need --init-audio
    ["--window-seconds", "10.24", "--adapters", "x"],                                     # --adapters needs --lora
    ["--window-seconds", "10.24", "--lora", "nopath", "--adapters", "x"],
])
def test_script_refuses_a_missing_prerequisite(flags):
    from audioldm_with_lora_amd.script import inference
    with pytest.raises(SystemExit):
        inference.parse_args(BASE + flags)


# ---- the engine cache key --------------------------------------------------------------------------------------------------------
def test_windowed_engine_key_extends_the_plain_key(monkeypatch):
    built = []

    class Stub:
        def __init__(self, unet, scheduler, *a, **kw):
            self.unet, self.scheduler, self.args, self.kw = unet, scheduler, a, kw
            built.append(self)

        def stale(self):
            return False

    class Plain(Stub):
        pass

    class Windowed(Stub):
        pass

    monkeypatch.setattr(audio2audio, "DenoiseEngine", Plain)
    monkeypatch.setattr(audio2audio, "WindowedAudioToAudioEngine", Windowed)
    p = _bare_pipeline()
    plan, _ = p.window_plan(2.88, 1.28, 0.32)
    other, _ = p.window_plan(2.88, 1.28, 0.64)
    a = p.engine(1, 72, 16, 10, 2.5, begin_index=5, masked=True)
    plain_keys = list(p._engines)
    b = p.engine(1, 72, 16, 10, 2.5, begin_index=5, masked=True, plan=plan)
    c = p.engine(1, 72, 16, 10, 2.5, begin_index=5, masked=True, plan=other)
    d = p.engine(1, 72, 16, 10, 2.5, begin_index=5, masked=True, gated=True, plan=plan)
    assert type(a) is Plain and type(b) is type(c) is type(d) is Windowed and len(built) == 4
    keys = list(p._engines)
    assert keys[:1] == plain_keys and len(plain_keys[0]) == 9                        # the plain key did not change
    assert keys[1] == plain_keys[0] + (("windowed",) + plan.key,)
    assert keys[2] == plain_keys[0] + (("windowed",) + other.key,)
    assert keys[3] == plain_keys[0] + (True, ("windowed",) + plan.key)
    # the same arguments find the same engine; the windowed engine got the plan, the suffix and the mask flag
    assert p.engine(1, 72, 16, 10, 2.5, begin_index=5, masked=True, plan=plan) is b and len(built) == 4
    assert b.args[1] is plan and b.kw["begin_index"] == 5 and b.kw["masked"] is True and b.kw["gated"] is False
    # another suffix, another mask flag: other engines
    assert p.engine(1, 72, 16, 10, 2.5, begin_index=4, masked=True, plan=plan) is not b
    assert p.engine(1, 72, 16, 10, 2.5, begin_index=5, masked=False, plan=plan) is not b


# ---- the engine subclass -----------------------------------------------------------------------------------------------------
def _stub_unet():
    return SimpleNamespace(cfg={"in_channels": 8}, plan_version=0)


def test_subclass_lifts_the_refusal_and_the_base_class_keeps_it():
    from audioldm_with_lora_amd.engine import DenoiseEngine, WindowedAudioToAudioEngine, WindowedDenoiseEngine
    plan = WindowPlan(72, 32, 8)
    for kw in (dict(masked=True), dict(begin_index=1), dict(chains=2)):
        with pytest.raises(NotImplementedError):
            WindowedDenoiseEngine(_stub_unet(), DDIMScheduler(), 2, plan, 16, 10, 2.5, device="cpu", **kw)
    with pytest.raises(NotImplementedError):
        WindowedAudioToAudioEngine(_stub_unet(), DDIMScheduler(), 2, plan, 16, 10, 2.5, device="cpu", chains=2)
    s = DDIMScheduler()
    eng = WindowedAudioToAudioEngine(_stub_unet(), s, 2, plan, 16, 10, 2.5, device="cpu", begin_index=5, masked=True)
    assert issubclass(WindowedAudioToAudioEngine, WindowedDenoiseEngine)
    assert eng.begin_index == 5 and eng.masked and eng.n_steps == 5 and eng.K == 3
    assert eng.x.shape == eng.x0.shape == eng.noise.shape == (2, 72, 16, 8) and eng.mask.shape == (2, 72, 16)
    assert eng.x_in[0].shape == (2 * 2 * 3, 32, 16, 8) and eng._step.__name__ == "ddim_step_fused_windowed_masked"
    # the suffix's tables exactly as DenoiseEngine derives them
    ref = DenoiseEngine(_stub_unet(), DDIMScheduler(), 2, 72, 16, 10, 2.5, device="cpu", begin_index=5, masked=True)
    assert torch.equal(eng.coef, ref.coef) and torch.equal(eng.timesteps_f32, ref.timesteps_f32) and torch.equal(eng.blend, ref.blend)
    assert torch.equal(eng.blend, s.blend_table(5)) and eng.in_scale0 == ref.in_scale0 == 1.0
    un = WindowedAudioToAudioEngine(_stub_unet(), DDIMScheduler(), 2, plan, 16, 10, 2.5, device="cpu", begin_index=5)
    assert un._step.__name__ == "ddim_step_fused_windowed" and un.x0 is None and un._inpaint_args == ()
    with pytest.raises(ValueError):
        un.set_inpaint(torch.zeros(2, 8, 72, 16), torch.zeros(2, 8, 72, 16), torch.ones(2, 72, 16))       # not a masked engine
    with pytest.raises(ValueError):
        WindowedAudioToAudioEngine(_stub_unet(), DDIMScheduler(), 2, plan, 16, 10, 2.5, device="cpu", begin_index=10)


def test_no_cpu_fallback():
    from audioldm_with_lora_amd import _lib, ops
    from audioldm_with_lora_amd.engine import WindowedAudioToAudioEngine
    plan = WindowPlan(72, 32, 8)
    eng = WindowedAudioToAudioEngine(_stub_unet(), DDIMScheduler(), 1, plan, 16, 10, 2.5, device="cpu", begin_index=5, masked=True)
    with pytest.raises(_lib.AldmError, match="no CPU fallback"):
        eng.set_latents(torch.zeros(1, 8, 72, 16))
    with pytest.raises(ValueError, match="long clip"):
        eng.set_inpaint(torch.zeros(1, 8, 32, 16), torch.zeros(1, 8, 72, 16), torch.ones(1, 72, 16))
    with pytest.raises(ValueError, match="mask shape"):
        eng.set_inpaint(torch.zeros(1, 8, 72, 16), torch.zeros(1, 8, 72, 16), torch.ones(1, 32, 16))
    with pytest.raises(_lib.AldmError, match="no CPU fallback"):
        eng.set_inpaint(torch.zeros(1, 8, 72, 16), torch.zeros(1, 8, 72, 16), torch.ones(1, 72, 16))
    x = torch.zeros(1, 72, 16, 8)
    eps = torch.zeros(2 * 3, 32, 16, 8)
    for solver, operand in (("ddim", ()), ("dpm", (torch.zeros_like(x),)), ("unipc", (torch.zeros(3, *x.shape),)),
                            ("euler_a", (torch.zeros(4, dtype=torch.int32),))):
        fn = getattr(ops, f"{solver}_step_fused_windowed_masked")
        cols = {"ddim": 4, "dpm": 8, "unipc": 16, "euler_a": 4}[solver]
        with pytest.raises(_lib.AldmError, match="no CPU fallback"):
            fn(eps, x, True, 2.5, torch.zeros(5, cols), torch.zeros(1, dtype=torch.int32), None, *operand, None, None, torch.zeros(5),
               torch.zeros(1), torch.zeros(1, dtype=torch.int32), plan.device("cpu"), x, x, torch.ones(1, 72, 16), torch.zeros(5, 2))
    p = _bare_pipeline()
    with pytest.raises(_lib.AldmError):
        p(prompt_embeds=torch.zeros(1, 64), audio=torch.zeros(16000), window_length_in_s=1.28)
