"""Text-guided audio-to-audio on the MI355X HIP path: style transfer, inpainting and band regeneration.

`AudioLDMAudioToAudioPipeline.from_pipe(pipe)(prompt, audio=wav, strength=0.5)` partly noises the encoded clip and denoises it
toward the prompt over the suffix timesteps[begin:] of the schedule (diffusers' get_timesteps rule).  With `mask=` the loop is
diffusers' legacy inpaint loop: after every step the known latents, noised to the next timestep, are blended back in where the mask
keeps them, inside the fused step launch (aldm_{ddim,dpm,unipc}_step_fused_masked), so the loop stays one captured graph.

With an EulerAncestralDiscreteScheduler every step re-draws part of the noise on the device (aldm_euler_a_step_fused[_masked]); the
rows are then in sigma space, (a, s) = (1, sigma).

    x0 = scaling_factor * vae.encode(log_mel(audio)).latent_dist.sample()
    x  = a_begin x0 + s_begin eps                         (x = eps exactly at strength 1)
    for k, t in enumerate(timesteps[begin:]):  x = step(unet(x, t), t, x);  x = (1 - m) (a_k x0 + s_k eps) + m x

With a RePaintScheduler the masked loop is RePaint's instead of the legacy one: the known latents are noised
with FRESH noise at every step and the walk jumps back up the schedule so that the regenerated region can come to agree with what
was pasted in (aldm_repaint_step_fused[_windowed]_masked).  It needs `mask=` and strength 1.0.

Long recordings: `window_length_in_s=` runs all of the above on ONE long latent as overlapping windows of the
trained length -- the recording is encoded window by window and the moments blended into the long layout, the loop is the windowed
fused step with the blend inside it (aldm_*_step_fused_windowed[_masked]), and the decode is the windowed one.  A mask that keeps
the recording and regenerates what lies behind it continues a clip to any length.
"""
import numpy as np
import torch

from . import ops
from .engine import DenoiseEngine, WindowedAudioToAudioEngine
from .loudness import check_rate as check_loudness_rate
from .loudness import normalize_loudness
from .mel import LogMelFrontEnd
from .pipeline import AudioLDMPipeline, AudioPipelineOutput, _frozen_config
from .resample import Resampler, ratio
from .resample import resample as resample_audio
from .scheduler import RePaintScheduler

HOP_SECONDS = 0.01        # one mel frame per 160 samples at 16 kHz


def regeneration_mask(height, n_mel, seconds=None, bands=None):
    """Rectangular mask [height, n_mel] fp32 at mel resolution, 1 = regenerate.  `seconds=(t0, t1)` marks the frames that overlap
    [t0, t1) at a 10 ms hop (all frames when None); `bands=(f0, f1)` marks the mel bins that overlap the fraction [f0, f1) of the bins
    (all bins when None), so bands=(0.5, 1.0) regenerates the upper half (band-limited super-resolution)."""
    m = torch.zeros(height, n_mel, dtype=torch.float32)
    r0, r1 = 0, height
    if seconds is not None:
        t0, t1 = (float(v) for v in seconds)
        if not 0.0 <= t0 < t1:
            raise ValueError(f"seconds=(t0, t1) needs 0 <= t0 < t1, got {seconds}")
        r0 = min(int(np.floor(t0 / HOP_SECONDS + 1e-6)), height)
        r1 = min(int(np.ceil(t1 / HOP_SECONDS - 1e-6)), height)
    c0, c1 = 0, n_mel
    if bands is not None:
        f0, f1 = (float(v) for v in bands)
        if not 0.0 <= f0 < f1 <= 1.0:
            raise ValueError(f"bands=(f0, f1) needs 0 <= f0 < f1 <= 1, got {bands}")
        c0 = int(np.floor(f0 * n_mel + 1e-6))
        c1 = int(np.ceil(f1 * n_mel - 1e-6))
    m[r0:r1, c0:c1] = 1.0
    return m


def continuation_mask(height, n_mel, recording_seconds):
    """The mask that CONTINUES a recording: keep its frames, regenerate every frame from its end to the end of a clip of `height` mel
    frames (regeneration_mask over [recording_seconds, the clip's end)).  With strength 1.0 and windows this extends a clip to any
    length: the kept rows are put back after every step and returned as the recording's own encoding."""
    t0 = float(recording_seconds)
    if not (t0 > 0.0 and int(np.floor(t0 / HOP_SECONDS + 1e-6)) < height):
        raise ValueError(f"a recording of {recording_seconds} s leaves nothing to generate in a clip of {height * HOP_SECONDS:g} s")
    return regeneration_mask(height, n_mel, seconds=(t0, (height + 1) * HOP_SECONDS))


def reduce_mask(mask, factor):
    """[B, H, W] mel-resolution mask -> [B, H / factor, W / factor] latent-resolution mask: the max over each factor x factor cell, so
    every latent pixel that touches a regenerated mel cell is regenerated.  Host-side (a few kB, once per call)."""
    mask = torch.as_tensor(mask, dtype=torch.float32).cpu()
    if mask.dim() != 3 or mask.shape[1] % factor or mask.shape[2] % factor:
        raise ValueError(f"mask [B, H, W] with H, W multiples of {factor} expected, got {tuple(mask.shape)}")
    return torch.nn.functional.max_pool2d(mask[:, None], factor)[:, 0].contiguous()


class AudioLDMAudioToAudioPipeline(AudioLDMPipeline):
    """AudioLDMPipeline that starts from a recording: style transfer (`strength`), inpainting / band regeneration (`mask`)."""

    @classmethod
    def from_pipe(cls, pipe):
        """shares pipe's modules (and its device); keeps an engine cache of its own"""
        new = cls(pipe.vae, pipe.text_encoder, pipe.tokenizer, pipe.unet, pipe.scheduler, pipe.vocoder)
        new.device = pipe.device
        return new

    def engine(self, batch, h, w, steps, guidance, begin_index=0, masked=False, gated=False, plan=None):
        key = (batch, h, w, steps, float(guidance), type(self.scheduler).__name__, _frozen_config(self.scheduler), int(begin_index),
               bool(masked)) + ((True,) if gated else ())
        if plan is not None:                            # (a windowed graph holds the plan's tables: plans never share one)
            key = key + (("windowed",) + plan.key,)
        eng = self._engines.get(key)
        if eng is not None and (eng.unet is not self._unet or eng.scheduler is not self.scheduler or eng.stale()):
            eng = None
        if eng is None and plan is not None:
            eng = self._engines[key] = WindowedAudioToAudioEngine(self._unet, self.scheduler, batch, plan, w, steps, guidance,
                                                                  device=self.device, begin_index=begin_index, masked=masked, gated=gated)
        if eng is None:
            eng = self._engines[key] = DenoiseEngine(self._unet, self.scheduler, batch, h, w, steps, guidance, device=self.device,
                                                     begin_index=begin_index, masked=masked, gated=gated)
        return eng

    def _audio_batch(self, audio, batch, per_prompt):
        a = torch.as_tensor(np.asarray(audio, dtype=np.float32)) if not torch.is_tensor(audio) else audio.detach().float()
        if a.dim() == 1:
            a = a[None].expand(batch, -1)
        elif a.dim() == 2:
            if a.shape[0] * per_prompt == batch and per_prompt > 1:
                a = a.repeat_interleave(per_prompt, dim=0)
            elif a.shape[0] != batch:
                raise ValueError(f"audio batch {a.shape[0]} does not match {batch // per_prompt} prompt(s)")
        else:
            raise ValueError(f"audio must be [T] or [B, T], got {tuple(a.shape)}")
        if a.shape[-1] == 0:
            raise ValueError("empty audio")
        return a.contiguous()

    def _latent_mask(self, mask, batch, per_prompt, height, n_mel):
        """the batching rule of _audio_batch: [frames, n_mel] is shared by every sample, [prompts, frames, n_mel] is repeated for
        each of a prompt's num_waveforms_per_prompt samples, [batch, frames, n_mel] is taken as is"""
        m = torch.as_tensor(mask, dtype=torch.float32).cpu()
        if m.dim() not in (2, 3) or tuple(m.shape[-2:]) != (height, n_mel):
            raise ValueError(f"mask must be [{height}, {n_mel}] or [B, {height}, {n_mel}] at mel resolution, got {tuple(m.shape)}")
        if m.dim() == 2:
            m = m[None].expand(batch, -1, -1)
        elif m.shape[0] * per_prompt == batch and per_prompt > 1:
            m = m.repeat_interleave(per_prompt, dim=0)
        elif m.shape[0] != batch:
            raise ValueError(f"mask batch {m.shape[0]} does not match {batch // per_prompt} prompt(s)")
        return reduce_mask(m.contiguous(), self.vae_scale_factor)

    def encode_windows(self, mel, plan, mel_plan):
        """The VAE moments of a long mel [B, 1, T, n_mel] fp32 as NCHW [B, 2C, rows, w] fp32: the mel plan's windows are gathered
        (bf16, the rounding of the plain path's input cast), encoded as batch rows -- shapes the VAE is tuned and tested for -- and
        the windows' MOMENTS (mean | logvar) blended linearly into the long layout by the latent plan's weights.  The posterior is
        sampled once, on the long moments: blending samples instead would average independent draws and shrink the variance in the
        overlaps.  A plan of one window is vae.encode(mel).latent_dist.parameters, bit for bit."""
        B, _, T, n_mel = mel.shape
        win = ops.window_gather(mel.contiguous().view(B, T, n_mel, 1), mel_plan.device(self.device))      # one channel: NCHW is NHWC
        mom = ops.window_blend(self.vae.encode_nhwc(win).contiguous(), plan.device(self.device))          # [B, rows, w, 2C] fp32
        return ops.nhwc_to_nchw_f32(mom)

    @torch.no_grad()
    def __call__(self, prompt=None, audio=None, sampling_rate=16000, strength=0.5, mask=None, audio_length_in_s=None,
                 num_inference_steps=50, guidance_scale=2.5, negative_prompt=None, num_waveforms_per_prompt=1, generator=None,
                 latents=None, prompt_embeds=None, negative_prompt_embeds=None, return_dict=True, output_type="np", adapter_names=None,
                 adapter_weights=None, window_length_in_s=None, window_overlap_in_s=None, loop=False, window_prompts=None,
                 window_prompt_embeds=None, resample=False, output_sampling_rate=None, loudness_lufs=None, peak_ceiling_dbfs=-1.0):
        """resample=True: a recording at another rate than the vocoder's 16 kHz is resampled on the device first (resample.py), on the
        plain and the windowed path alike, and everything downstream sees the 16 kHz clip; without it such a rate raises.
        output_sampling_rate, loudness_lufs / peak_ceiling_dbfs: as in AudioLDMPipeline.__call__ (not with output_type="latent").
        window_length_in_s / window_overlap_in_s / loop / window_prompts / window_prompt_embeds: as in AudioLDMPipeline.__call__
        (None: one clip at the recording's own length, as ever).  With windows, `mask` and `latents` are those of the LONG clip, whose
        length is audio_length_in_s or the recording's (a looped plan rounds it UP and the longer clip is returned)."""
        if self.device.type != "cuda":
            raise ops._lib.AldmError("AudioLDMAudioToAudioPipeline runs on the MI355X only: call .to('cuda') (no CPU fallback)")
        if audio is None:
            raise ValueError("pass audio= (the recording to start from)")
        if isinstance(self.scheduler, RePaintScheduler) and mask is None:
            raise ValueError("RePaintScheduler needs mask=: RePaint resamples a masked region against the kept one (style transfer "
                             "without a mask takes another scheduler)")
        if output_type not in ("np", "pt", "latent"):
            raise ValueError(f"output_type must be 'np', 'pt' or 'latent', got {output_type!r}")
        vc = self.vocoder.config
        if int(sampling_rate) != int(vc.sampling_rate):
            if not resample:
                raise ValueError(f"audio at {sampling_rate} Hz: the vocoder runs at {vc.sampling_rate} Hz; pass resample=True to resample "
                                 "the recording on the device first")
            ratio(sampling_rate, vc.sampling_rate)                  # (raises on a rate that cannot be reached, before any work)
        if output_sampling_rate is not None:
            if output_type == "latent":
                raise ValueError("output_sampling_rate applies to a waveform, not to output_type='latent'")
            ratio(vc.sampling_rate, output_sampling_rate)
        if loudness_lufs is not None:
            if output_type == "latent":
                raise ValueError("loudness_lufs applies to a waveform, not to output_type='latent'")
            check_loudness_rate(vc.sampling_rate if output_sampling_rate is None else output_sampling_rate)
        _, begin = self.scheduler.get_timesteps(num_inference_steps, strength)    # raises on a strength that leaves no step
        if window_length_in_s is None:
            if loop or window_prompts is not None or window_prompt_embeds is not None or window_overlap_in_s is not None:
                raise ValueError("loop / window_prompts / window_overlap_in_s need window_length_in_s")
        elif prompt is None and prompt_embeds is None and window_prompt_embeds is not None:
            prompt_embeds = window_prompt_embeds[:, 0]              # (batch size and the negative half come from the per-clip path)
        elif prompt is None and prompt_embeds is None and window_prompts is not None:
            prompt = [window_prompts[0]] if isinstance(window_prompts[0], str) else [p[0] for p in window_prompts]
        prompt_embeds, negative_prompt_embeds = self._prompt_embeds(prompt, prompt_embeds, negative_prompt, negative_prompt_embeds,
                                                                    guidance_scale, num_waveforms_per_prompt)
        batch = prompt_embeds.shape[0]
        if int(sampling_rate) != int(vc.sampling_rate):             # resample=True: the recording becomes its 16 kHz form here
            a = torch.as_tensor(np.asarray(audio, dtype=np.float32)) if not torch.is_tensor(audio) else audio.detach().float()
            audio = Resampler(sampling_rate, vc.sampling_rate, self.device)(a.to(self.device))
        wav = self._audio_batch(audio, batch, num_waveforms_per_prompt)
        if audio_length_in_s is None:
            audio_length_in_s = wav.shape[-1] / float(vc.sampling_rate)
        height, n_samples = self.geometry(audio_length_in_s)
        plan = mel_plan = None
        if window_length_in_s is not None:
            plan, mel_plan = self.window_plan(audio_length_in_s, window_length_in_s, window_overlap_in_s, loop)
            height = plan.rows * self.vae_scale_factor
            if loop:                                    # the whole rounded-up loop: trimming it would open the seam
                n_samples = height * int(np.prod(vc.upsample_rates))
            if window_prompts is not None or window_prompt_embeds is not None:
                prompt_embeds = self._window_prompt_embeds(window_prompts, window_prompt_embeds, batch // num_waveforms_per_prompt, plan.K,
                                                           num_waveforms_per_prompt)
        n_mel = vc.model_in_dim
        h, w = height // self.vae_scale_factor, n_mel // self.vae_scale_factor
        shape = (batch, self._unet.cfg["in_channels"], h, w)
        m_lat = self._latent_mask(mask, batch, num_waveforms_per_prompt, height, n_mel) if mask is not None else None
        if latents is not None and tuple(latents.shape) != shape:
            raise ValueError(f"Unexpected latents shape, got {tuple(latents.shape)}, expected {shape}")

        # encode: log-mel front end (pads / crops to `height` frames) -> VAE moments -> posterior sample
        mel = LogMelFrontEnd(device=self.device, target_length=height, n_mel=n_mel)(wav.to(self.device))
        if plan is None:
            params = self.vae.encode(mel).latent_dist.parameters
        else:
            params = self.encode_windows(mel, plan, mel_plan)
        if tuple(params.shape) != (shape[0], 2 * shape[1]) + shape[2:]:
            raise ValueError(f"the VAE encodes to {tuple(params.chunk(2, dim=1)[0].shape)}, the UNet expects {shape}")
        # random draws, in this order, on the generator's device: the posterior noise, then eps (unless latents= gives it)
        gdev = generator.device if generator is not None else torch.device("cpu")
        post = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32)
        if latents is None:
            latents = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32)
        eps = latents.to(self.device, torch.float32).contiguous()
        x0 = ops.gaussian_sample(params.float(), post.to(self.device)) * self.vae.config.scaling_factor
        if float(strength) == 1.0:
            x = eps                                                   # diffusers' is_strength_max: pure noise, not a * x0 + s * eps
            if self.scheduler.init_noise_sigma != 1.0:                # (sigma-space schedulers start at init_noise_sigma * noise)
                x = x * self.scheduler.init_noise_sigma
        else:
            a, s = self.scheduler.add_noise_coefficients(begin)
            coef = torch.tensor([float(a), float(s)], dtype=torch.float32).repeat(batch).to(self.device)
            x = ops.add_noise(x0, eps, coef)

        gated, adapter_names, adapter_weights = self._route(adapter_names, adapter_weights, batch // num_waveforms_per_prompt, num_waveforms_per_prompt)
        if plan is None:
            eng = self.engine(batch, h, w, num_inference_steps, guidance_scale, begin_index=begin, masked=m_lat is not None, gated=gated)
        else:
            eng = self.engine(batch, h, w, num_inference_steps, guidance_scale, begin_index=begin, masked=m_lat is not None, gated=gated,
                              plan=plan)
        eng.set_adapters(adapter_names, adapter_weights)
        eng.set_condition(prompt_embeds, negative_prompt_embeds)
        self._seed_engine(eng, generator)
        eng.set_latents(x)
        if m_lat is not None:
            eng.set_inpaint(x0, eps, m_lat)
        if eng.graph is None and eng.use_graph:
            eng.capture()
        eng.run()
        mel_out = loud = None
        rate = int(vc.sampling_rate)
        if output_type == "latent":
            out = eng.latents_nchw()
        else:
            wav_out, mel_out = self.decode_latents_nhwc(eng.x) if plan is None else self.decode_windows_nhwc(eng.x, plan, mel_plan, loop)
            out = wav_out[:, :n_samples]
            if output_sampling_rate is not None:
                out, rate = resample_audio(out, rate, output_sampling_rate), int(output_sampling_rate)
            if loudness_lufs is not None:
                out, loud = normalize_loudness(out, rate, loudness_lufs, peak_ceiling_dbfs)
            if output_type == "np":
                out = out.float().cpu().numpy()
        if not return_dict:
            return (out,)
        if plan is not None:                            # a windowed call also hands back its plan and the blended mel [B, T, 64] (device)
            return AudioPipelineOutput(audios=out, sampling_rate=rate, plan=plan, mel=None if mel_out is None else mel_out[..., 0],
                                       loudness=loud)
        return AudioPipelineOutput(audios=out, sampling_rate=rate, loudness=loud)
