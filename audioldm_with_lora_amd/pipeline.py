"""AudioLDMPipeline on the MI355X HIP path.

Drop-in for diffusers' `AudioLDMPipeline` as the reference drives it:
  `AudioLDMPipeline.from_pretrained(id, unet=unet, torch_dtype=...)`, `.to(device)`,
  `pipe(prompt, num_inference_steps=, audio_length_in_s=, guidance_scale=).audios[0]`
  [REF app.py:7-14] [REF script/inference/generate_audio.py:42-52] [REF script/train/train_audioldm_lora.py:365,599,142]
Steps 1-8 of SURVEY.md section 3.1.  The text encoder (CLAP, outside the north_star path) is stock transformers
host code when a local checkpoint provides it; `prompt_embeds=` bypasses it.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .engine import DenoiseEngine, WindowedDenoiseEngine
from .longform import plan_for_seconds
from .loudness import check_rate as check_loudness_rate
from .loudness import normalize_loudness
from .resample import ratio, resample
from .scheduler import DDIMScheduler, _fresh_seed
from .unet import UNet2DConditionModel
from .vae import AutoencoderKL
from .vocoder import SpeechT5HifiGan


class AudioPipelineOutput(SimpleNamespace):
    pass


def _frozen_config(scheduler):
    """the scheduler's configuration as a hashable, sorted tuple (lists become tuples)"""
    cfg = scheduler.config
    items = cfg.items() if isinstance(cfg, dict) else vars(cfg).items()
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in items))


class AudioLDMPipeline:
    def __init__(self, vae, text_encoder, tokenizer, unet, scheduler, vocoder):
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        # the reference hands the pipeline either the bare UNet [REF generate_audio.py:42] or the peft wrapper
        # (accelerator.unwrap_model(unet) is the PeftModel [REF train:598-599]); both keep `.unet` as given
        self.unet, self.scheduler, self.vocoder = unet, scheduler, vocoder
        self.vae_scale_factor = 2 ** (len(vae.cfg["block_out_channels"]) - 1)
        self.device = torch.device("cpu")
        self._engines = {}
        self._plans = {}
        self._progress = {}

    @classmethod
    def from_pretrained(cls, path, unet=None, torch_dtype=None, **kw):
        """Loads a local diffusers-format directory (unet/ vae/ vocoder/ scheduler/ [text_encoder/ tokenizer/])."""
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path}: hub downloads are unavailable offline, pass a local model directory")
        if unet is None:
            unet = UNet2DConditionModel.from_pretrained(path, subfolder="unet")
        vae = AutoencoderKL.from_pretrained(path, subfolder="vae")
        vocoder = SpeechT5HifiGan.from_pretrained(path, subfolder="vocoder")
        scheduler = DDIMScheduler.from_pretrained(path, subfolder="scheduler")
        text_encoder = tokenizer = None
        if os.path.isdir(os.path.join(path, "text_encoder")):
            from transformers import RobertaTokenizerFast          # host-side string -> ids only
            from .clap_text import ClapTextModelWithProjection    # the tower itself runs on the HIP kernels
            text_encoder = ClapTextModelWithProjection.from_pretrained(os.path.join(path, "text_encoder"))
            tokenizer = RobertaTokenizerFast.from_pretrained(os.path.join(path, "tokenizer"))
        return cls(vae, text_encoder, tokenizer, unet, scheduler, vocoder)

    @property
    def _unet(self):
        """the UNet2DConditionModel behind `.unet` (unwraps a lora.PeftModel)"""
        return getattr(getattr(self.unet, "base_model", None), "model", self.unet)

    def to(self, device):
        self.device = torch.device(device)
        for m in (self.vae, self.unet, self.vocoder, self.text_encoder):
            if m is not None:
                m.to(self.device)
        self._engines.clear()
        return self

    def set_progress_bar_config(self, **kw):
        self._progress = kw

    # ---- step 2: prompt -> L2-normalised CLAP text embedding (tokeniser on the host, tower on the GPU: clap_text.py) ----
    def _encode_prompt(self, prompt, batch):
        if self.text_encoder is None or self.tokenizer is None:
            raise ValueError("no text encoder loaded: pass prompt_embeds= / negative_prompt_embeds=")
        tok = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                             return_tensors="pt")
        with torch.no_grad():
            emb = self.text_encoder(tok.input_ids.to(self.device), attention_mask=tok.attention_mask.to(self.device)).text_embeds
        return torch.nn.functional.normalize(emb.float(), dim=-1)

    def _prompt_embeds(self, prompt, prompt_embeds, negative_prompt, negative_prompt_embeds, guidance_scale, num_waveforms_per_prompt):
        """step 2 with CFG's negative half and num_waveforms_per_prompt: (prompt_embeds, negative_prompt_embeds or None)"""
        if prompt_embeds is None:
            if prompt is None:
                raise ValueError("pass prompt or prompt_embeds")
            prompts = [prompt] if isinstance(prompt, str) else list(prompt)
            prompt_embeds = self._encode_prompt(prompts, len(prompts))
        batch = prompt_embeds.shape[0]
        cfg = guidance_scale > 1.0
        if cfg and negative_prompt_embeds is None:
            if self.text_encoder is not None:
                neg = [""] * batch if negative_prompt is None else ([negative_prompt] * batch if isinstance(negative_prompt, str) else list(negative_prompt))
                negative_prompt_embeds = self._encode_prompt(neg, batch)
            else:
                negative_prompt_embeds = torch.zeros_like(prompt_embeds)
        if num_waveforms_per_prompt > 1:
            prompt_embeds = prompt_embeds.repeat_interleave(num_waveforms_per_prompt, dim=0)
            if negative_prompt_embeds is not None:
                negative_prompt_embeds = negative_prompt_embeds.repeat_interleave(num_waveforms_per_prompt, dim=0)
        return prompt_embeds, negative_prompt_embeds

    def geometry(self, audio_length_in_s):
        vc = self.vocoder.config
        up = float(np.prod(vc.upsample_rates)) / vc.sampling_rate
        height = int(audio_length_in_s / up)
        n_samples = int(audio_length_in_s * vc.sampling_rate)
        if height % self.vae_scale_factor != 0:
            height = int(np.ceil(height / self.vae_scale_factor)) * self.vae_scale_factor
        return height, n_samples

    def engine(self, batch, h, w, steps, guidance, gated=False, plan=None):
        # the scheduler is part of the key: a graph captured with one scheduler's update and coefficients must never replay for another
        # (gated: a graph whose fused-LoRA launches read a per-clip gate table is another graph than the plain single-adapter one;
        # plan: a windowed engine's graph holds the plan's tables and window count, so different plans never share one)
        key = (batch, h, w, steps, float(guidance), type(self.scheduler).__name__, _frozen_config(self.scheduler)) + ((True,) if gated else ())
        if plan is not None:
            key = key + (("windowed",) + plan.key,)
        eng = self._engines.get(key)
        if eng is not None and (eng.unet is not self._unet or eng.scheduler is not self.scheduler or eng.stale()):
            eng = None                                  # weights / adapter / scheduler changed since the capture: never replay the old graph
        if eng is None and plan is not None:
            eng = self._engines[key] = WindowedDenoiseEngine(self._unet, self.scheduler, batch, plan, w, steps, guidance, device=self.device,
                                                             gated=gated)
        if eng is None:
            eng = self._engines[key] = DenoiseEngine(self._unet, self.scheduler, batch, h, w, steps, guidance, device=self.device, gated=gated)
        return eng

    # ---- long-form and loopable generation ----
    def window_plan(self, audio_length_in_s, window_length_in_s, window_overlap_in_s=None, loop=False):
        """(the latent plan, the mel plan) of a windowed call: longform.plan_for_seconds with this pipeline's frame rate and VAE
        scale, and the same plan at the mel's resolution.  Kept per key, so the device tables a captured graph reads stay alive."""
        vc = self.vocoder.config
        if window_overlap_in_s is None:
            window_overlap_in_s = window_length_in_s / 4.0
        up = float(np.prod(vc.upsample_rates)) / vc.sampling_rate
        plan = plan_for_seconds(audio_length_in_s, window_length_in_s, window_overlap_in_s, up, self.vae_scale_factor, loop)
        if plan.key not in self._plans:
            self._plans[plan.key] = (plan, plan.scaled(self.vae_scale_factor))
        return self._plans[plan.key]

    def vocoder_half_field(self):
        """Mel frames on either side of a frame that can reach its audio: the vocoder's receptive half-field, from its config alone
        (DESIGN.md section 18 has the derivation).  Walks the stack from the waveform back to the mel, a radius in samples of each
        stage: conv_post and conv_pre (kernel 7) add 3; a stage's residual blocks run side by side, so the widest counts, each
        dilation d of kernel k adding (k - 1) / 2 * (d + 1); a transposed conv (kernel k, stride u, padding p) maps a radius R of
        its output to ceil((R + max(p, k - 1 - p)) / u) of its input."""
        vc = self.vocoder.config
        res = max((k - 1) // 2 * (sum(d) + len(d)) for k, d in zip(vc.resblock_kernel_sizes, vc.resblock_dilation_sizes))
        r = 3
        for u, k in reversed(list(zip(vc.upsample_rates, vc.upsample_kernel_sizes))):
            p = (k - u) // 2
            r = -(-(r + res + max(p, k - 1 - p)) // u)
        return r + 3

    def _window_prompt_embeds(self, window_prompts, window_prompt_embeds, n_prompts, K, num_waveforms_per_prompt):
        """[B, K, D] L2-normalised embeddings, one per (clip, window): from K strings per prompt, or as given"""
        if window_prompt_embeds is None:
            wp = [list(window_prompts)] if isinstance(window_prompts[0], str) else [list(p) for p in window_prompts]
            if len(wp) != n_prompts or any(len(p) != K for p in wp):
                raise ValueError(f"window_prompts needs {K} strings (one per window) for each of the {n_prompts} prompts")
            window_prompt_embeds = self._encode_prompt([t for p in wp for t in p], n_prompts * K).view(n_prompts, K, -1)
        if window_prompt_embeds.dim() != 3 or tuple(window_prompt_embeds.shape[:2]) != (n_prompts, K):
            raise ValueError(f"window_prompt_embeds must be [{n_prompts}, {K}, D], got {tuple(window_prompt_embeds.shape)}")
        return window_prompt_embeds.repeat_interleave(num_waveforms_per_prompt, dim=0) if num_waveforms_per_prompt > 1 else window_prompt_embeds

    def decode_windows_nhwc(self, x_long, plan, mel_plan, loop=False):
        """steps 6-7 of a long latent [B, rows, w, 8] fp32: the VAE decodes the plan's windows as batch rows (shapes it is tuned and
        tested for), the windows' mels are blended into one long mel by the plan at the mel's resolution, and the vocoder runs on the
        whole mel -> (waveform [B, 160 * 4 rows (+ 32 when not looped)], mel [B, 4 rows, 64, 1] fp32).  loop: the mel is padded
        circularly by the vocoder's receptive half-field on both sides and the waveform trimmed back, so that sample 0 continues
        from the last sample."""
        z = ops.window_gather(x_long, plan.device(self.device), 1.0 / self.vae.config.scaling_factor)
        mel = ops.window_blend(self.vae.decode_nhwc(z).contiguous(), mel_plan.device(self.device))       # [B, T, 64, 1] fp32
        B, T, F, _ = mel.shape
        if not loop:
            return self.vocoder.forward_nhwc(ops.f32_to_bf16(mel).view(B, 1, T, F)), mel
        P = self.vocoder_half_field()
        idx = torch.arange(-P, T + P, device=mel.device) % T
        padded = mel.index_select(1, idx).contiguous()
        wav = self.vocoder.forward_nhwc(ops.f32_to_bf16(padded).view(B, 1, T + 2 * P, F))
        hop = int(np.prod(self.vocoder.config.upsample_rates))
        return wav[:, P * hop:(P + T) * hop], mel

    # ---- LoRA adapters (diffusers' surface) ----
    def _peft(self):
        from .lora import PeftModel
        if not isinstance(self.unet, PeftModel):
            for p in self.unet.parameters():
                p.requires_grad_(False)
            self.unet = PeftModel(self.unet, None)
        return self.unet

    def load_lora_weights(self, path_or_state_dict, adapter_name="default", r=None, lora_alpha=None, target_modules=None):
        """A local .safetensors / .bin file or directory, or a state dict in peft's saved form or the diffusers form.  Rank and targets
        are read from the tensors when not given; lora_alpha from an adapter_config.json next to the file, else = r.  Repacks the UNet's
        operands (captured graphs are rebuilt on the next call); choosing between loaded adapters afterwards does not."""
        from .lora import LoraConfig, _read_adapter_file, normalize_adapter_state_dict
        sd, cfg_json = path_or_state_dict, None
        if isinstance(sd, (str, os.PathLike)):
            sd, cfg_json = _read_adapter_file(os.fspath(sd))
        cfg = None
        if r is not None or lora_alpha is not None or target_modules is not None:
            t = normalize_adapter_state_dict(sd)
            rr = r if r is not None else next(v.shape[0] for (m, ab), v in t.items() if ab == "A")
            la = lora_alpha if lora_alpha is not None else (cfg_json or {}).get("lora_alpha", rr)
            cfg = LoraConfig(r=rr, lora_alpha=la, init_lora_weights="gaussian",
                             target_modules=list(target_modules) if target_modules is not None else sorted({m for m, _ in t}))
        elif cfg_json is not None and "lora_alpha" in cfg_json:
            t = normalize_adapter_state_dict(sd)
            rr = next(v.shape[0] for (m, ab), v in t.items() if ab == "A")
            cfg = LoraConfig(r=rr, lora_alpha=cfg_json["lora_alpha"], init_lora_weights="gaussian", target_modules=sorted({m for m, _ in t}))
        self._peft().load_adapter(sd, adapter_name, cfg)

    def set_adapters(self, names, adapter_weights=None):
        self._unet.set_adapters(names, adapter_weights)

    def get_active_adapters(self):
        return list(self._unet.active_adapters) if self._unet.lora_enabled else []

    def get_list_adapters(self):
        return {"unet": self._unet.lora_adapters()}

    def disable_lora(self):
        self._unet.set_lora_enabled(False)

    def enable_lora(self):
        self._unet.set_lora_enabled(True)

    def delete_adapters(self, names):
        for n in ([names] if isinstance(names, str) else list(names)):
            self._peft().delete_adapter(n)

    def unload_lora_weights(self):
        self.delete_adapters(self._unet.lora_adapters())

    def _route(self, adapter_names, adapter_weights, n_prompts, num_waveforms_per_prompt):
        """(gated?, per-clip adapter_names, per-clip adapter_weights): one entry per prompt, repeated over num_waveforms_per_prompt
        like the prompt embeddings"""
        u = self._unet
        if adapter_names is not None:
            if isinstance(adapter_names, (str, dict)) or len(adapter_names) != n_prompts:
                raise ValueError(f"adapter_names needs one entry per prompt ({n_prompts}), got {adapter_names!r}")
            adapter_names = [a for a in adapter_names for _ in range(num_waveforms_per_prompt)]
        if adapter_weights is not None:
            if len(adapter_weights) != n_prompts:
                raise ValueError(f"adapter_weights needs one entry per prompt ({n_prompts})")
            adapter_weights = [a for a in adapter_weights for _ in range(num_waveforms_per_prompt)]
        gated = adapter_weights is not None or not u.routing_is_plain(adapter_names)
        return gated, adapter_names, adapter_weights

    @staticmethod
    def _seed_engine(eng, generator):
        """Stochastic samplers (EulerAncestralDiscreteScheduler, RePaintScheduler) draw their per-step noise on the device, inside the replayed graph, from
        a Philox stream of this library's own.  Its seed is `generator.initial_seed()` when a generator is passed -- only that number is
        read, the generator's stream is neither used nor advanced by the loop -- else a fresh one from torch's global CPU generator (new
        on every call, reproducible after torch.manual_seed).  Deterministic samplers draw nothing: no-op."""
        if eng.euler or eng.repaint:
            eng.set_seed(generator.initial_seed() if generator is not None else _fresh_seed())

    def decode_latents_nhwc(self, x_nhwc_f32):
        """steps 6-7: latents [B, h, w, 8] fp32 channels-last -> waveform [B, 160*4h + 32] fp32 (device)."""
        z = ops.f32_to_bf16(x_nhwc_f32, 1.0 / self.vae.config.scaling_factor)
        mel = self.vae.decode_nhwc(z)                          # [B, T, 64, 1] fp32 == [B, 1, T, 64] channels-last
        B, T, F, _ = mel.shape
        melb = ops.f32_to_bf16(mel).view(B, 1, T, F)
        return self.vocoder.forward_nhwc(melb), mel

    @torch.no_grad()
    def __call__(self, prompt=None, audio_length_in_s=None, num_inference_steps=10, guidance_scale=2.5,
                 negative_prompt=None, num_waveforms_per_prompt=1, eta=0.0, generator=None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, return_dict=True, output_type="np", adapter_names=None,
                 adapter_weights=None, window_length_in_s=None, window_overlap_in_s=None, loop=False, window_prompts=None,
                 window_prompt_embeds=None, output_sampling_rate=None, loudness_lufs=None, peak_ceiling_dbfs=-1.0, **kw):
        """loudness_lufs (default None: the level the vocoder produced, as ever): every clip is brought to this BS.1770 integrated
        loudness on the device (loudness.py), at the rate it is delivered at -- after the output_sampling_rate resampling -- with the
        gain capped so that the oversampled peak stays at or under peak_ceiling_dbfs (None: no cap); the output carries `loudness`,
        the dict of device tensors lufs_in / gain_db / peak_in (None without loudness_lufs).
        output_sampling_rate (default None: the vocoder's 16 kHz, as ever): the trimmed waveform is resampled to this rate on the
        device before it leaves for the host (resample.py; ceil(n_samples up / down) samples); the output carries `sampling_rate`.
        window_length_in_s (default None: one clip of audio_length_in_s, as ever) turns on windowed denoising for clips longer
        than the UNet was trained on: overlapping windows of that length (window_overlap_in_s, default a quarter of it) along one
        long latent, blended at every step; loop=True makes the clip close on itself (its length is rounded UP to a whole number of
        window strides).  window_prompts: K strings per prompt, or window_prompt_embeds [B, K, D] -- one prompt per window."""
        if self.device.type != "cuda":
            raise ops._lib.AldmError("AudioLDMPipeline runs on the MI355X only: call .to('cuda') (no CPU fallback)")
        if eta != 0.0:
            raise NotImplementedError("the reference path uses eta = 0")
        vc = self.vocoder.config
        if output_sampling_rate is not None:
            ratio(vc.sampling_rate, output_sampling_rate)           # (raises on a rate that cannot be reached, before any work)
        if loudness_lufs is not None:
            check_loudness_rate(vc.sampling_rate if output_sampling_rate is None else output_sampling_rate)
        if audio_length_in_s is None:
            # diffusers: unet.config.sample_size * vae_scale_factor * prod(upsample_rates) / sampling_rate
            inner = getattr(getattr(self.unet, "base_model", None), "model", self.unet)          # a PeftModel wraps the UNet
            audio_length_in_s = inner.config.sample_size * self.vae_scale_factor * float(np.prod(vc.upsample_rates)) / vc.sampling_rate
        height, n_samples = self.geometry(audio_length_in_s)
        plan = mel_plan = None
        if window_length_in_s is None:
            if loop or window_prompts is not None or window_prompt_embeds is not None or window_overlap_in_s is not None:
                raise ValueError("loop / window_prompts / window_overlap_in_s need window_length_in_s")
        else:
            plan, mel_plan = self.window_plan(audio_length_in_s, window_length_in_s, window_overlap_in_s, loop)
            height = plan.rows * self.vae_scale_factor
            if loop:                                    # the whole rounded-up loop: trimming it would open the seam
                n_samples = height * int(np.prod(vc.upsample_rates))
            if prompt is None and prompt_embeds is None and window_prompt_embeds is not None:
                prompt_embeds = window_prompt_embeds[:, 0]          # (batch size and the negative half come from the per-clip path)
            elif prompt is None and prompt_embeds is None and window_prompts is not None:
                prompt = [window_prompts[0]] if isinstance(window_prompts[0], str) else [p[0] for p in window_prompts]
        prompt_embeds, negative_prompt_embeds = self._prompt_embeds(prompt, prompt_embeds, negative_prompt, negative_prompt_embeds,
                                                                    guidance_scale, num_waveforms_per_prompt)
        batch = prompt_embeds.shape[0]
        if plan is not None and (window_prompts is not None or window_prompt_embeds is not None):
            prompt_embeds = self._window_prompt_embeds(window_prompts, window_prompt_embeds, batch // num_waveforms_per_prompt, plan.K,
                                                       num_waveforms_per_prompt)
        h, w = height // self.vae_scale_factor, vc.model_in_dim // self.vae_scale_factor
        shape = (batch, self._unet.cfg["in_channels"], h, w)
        if latents is None:
            gdev = generator.device if generator is not None else torch.device("cpu")
            latents = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32)
        elif tuple(latents.shape) != shape:
            raise ValueError(f"Unexpected latents shape, got {tuple(latents.shape)}, expected {shape}")
        self.scheduler.set_timesteps(num_inference_steps)       # (host-only) init_noise_sigma of a sigma-space scheduler depends on the schedule
        latents = latents.to(self.device, torch.float32) * self.scheduler.init_noise_sigma

        gated, adapter_names, adapter_weights = self._route(adapter_names, adapter_weights, batch // num_waveforms_per_prompt, num_waveforms_per_prompt)
        eng = self.engine(batch, h, w, num_inference_steps, guidance_scale, gated=gated, plan=plan)
        eng.set_adapters(adapter_names, adapter_weights)
        eng.set_condition(prompt_embeds, negative_prompt_embeds)
        self._seed_engine(eng, generator)
        eng.set_latents(latents)
        if eng.graph is None and eng.use_graph:
            eng.capture()
        eng.run()
        wav, mel = self.decode_latents_nhwc(eng.x) if plan is None else self.decode_windows_nhwc(eng.x, plan, mel_plan, loop)
        audio = wav[:, :n_samples]
        rate = int(vc.sampling_rate)
        if output_sampling_rate is not None:
            audio, rate = resample(audio, rate, output_sampling_rate), int(output_sampling_rate)
        loud = None
        if loudness_lufs is not None:
            audio, loud = normalize_loudness(audio, rate, loudness_lufs, peak_ceiling_dbfs)
        if output_type == "np":
            audio = audio.float().cpu().numpy()
        if not return_dict:
            return (audio,)
        if plan is not None:                            # a windowed call also hands back its plan and the blended mel [B, T, 64] (device)
            return AudioPipelineOutput(audios=audio, sampling_rate=rate, plan=plan, mel=mel[..., 0], loudness=loud)
        return AudioPipelineOutput(audios=audio, sampling_rate=rate, loudness=loud)
