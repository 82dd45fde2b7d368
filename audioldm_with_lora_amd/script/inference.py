"""LoRA inference driver -- MI355X mirror of  script/inference/generate_audio.py:main  [REF generate_audio.py:11-59]
(and app.py [REF app.py:6-16] with --no-lora --steps 200).

Loads the UNet, injects the peft-style LoRA structure, loads adapter weights from a safetensors file with peft key
names (`base_model.model.<path>.lora_{A,B}.default.weight`, strict=False as in the reference), builds the pipeline and
writes a wav.  LoRA stays un-merged and is applied inside the fused projection GEMMs (reference quirk Q4).
Defaults follow the script: r=2, 50 DDIM steps, 10 s, guidance 5.0; alpha defaults to the TRAINED value 2 rather than the
script's inconsistent 4 (quirk Q3) -- pass --lora-alpha 4 to reproduce the script literally.
`--scheduler dpmsolver++ --steps 25` swaps in DPMSolverMultistepScheduler (from the checkpoint's scheduler config) instead of DDIM.
`--scheduler unipc --steps 8` swaps in UniPCMultistepScheduler (predictor-corrector, the sampler for 5-10 steps; `--solver-order` applies).
`--scheduler euler-a` swaps in EulerAncestralDiscreteScheduler (stochastic: fresh noise in every step, drawn on the device); `--seed` then
seeds both the initial noise and that in-loop stream.
`--init-audio in.wav --strength 0.5` starts from a recording (AudioLDMAudioToAudioPipeline: style transfer toward the prompt); a file
that is not at the model's 16 kHz (44.1 / 48 kHz, ...) is resampled on the device first, and `--output-sampling-rate R` writes the
wav files at R Hz instead of 16 kHz (resample.py: scipy.signal.resample_poly's filter);
`--regenerate-seconds T0,T1` / `--regenerate-bands F0,F1` regenerate only that time span / fraction of the mel bins and keep the rest.
`--lora NAME=PATH` (repeatable) loads named adapters side by side; `--adapters SPEC` routes them per prompt -- a comma list with one item
per prompt (`--prompt` then takes prompts separated by `|`): `NAME`, `NAME:0.7`, `base`, or a blend `A:0.5+B:0.5`.  One call, one
captured graph: the adapted and the original model of the reference's log_validation side by side.
`--audio-length 60 --window-seconds 10.24 --window-overlap-seconds 2.56` generates a clip longer than the model was trained on by
windowed denoising (overlapping windows of the trained length along one long latent, blended at every step); `--loop` makes it close
on itself (the length is rounded up to a whole number of window strides); `--window-prompts "a|b|c"` gives every window its own prompt.
`--init-audio in.wav --window-seconds 10.24` restyles or inpaints a recording of any length the same way (`--strength`,
`--regenerate-seconds`, `--regenerate-bands`, `--loop` and `--window-prompts` apply); `--extend-to-seconds T` keeps the recording and
generates what follows it up to T seconds.
`--repaint JUMP_LENGTH,JUMP_N_SAMPLE` (with --init-audio and a --regenerate-* or --extend-to-seconds mask, with or without
--window-seconds) inpaints with RePaint's resampling loop (RePaintScheduler) instead of the legacy blend: more UNet calls, and a
regenerated region that agrees better with what is kept; it runs from noise (--strength 1.0).
`--loudness -14 [--peak-ceiling -1]` brings every clip to that ITU-R BS.1770 integrated loudness on the device before it is written
(loudness.py; after `--output-sampling-rate`, so the level and the peak ceiling hold for the file).
"""
import argparse
import os

import numpy as np
import torch

from ..lora import LoraConfig, get_peft_model
from ..audio2audio import AudioLDMAudioToAudioPipeline, continuation_mask, regeneration_mask
from ..pipeline import AudioLDMPipeline
from ..scheduler import DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, RePaintScheduler, UniPCMultistepScheduler
from ..unet import UNet2DConditionModel


def parse_adapters(spec):
    """--adapters SPEC -> the pipeline's adapter_names: 'boom_bap,trap:0.7,base,a:0.5+b:0.5' ->
    ['boom_bap', {'trap': 0.7}, '__base__', {'a': 0.5, 'b': 0.5}]"""
    out = []
    for item in spec.split(","):
        item = item.strip()
        if not item:
            raise ValueError(f"--adapters: empty item in {spec!r}")
        if item in ("base", "__base__"):
            out.append("__base__")
            continue
        blend = {}
        for part in item.split("+"):
            name, sep, w = part.strip().partition(":")
            if not name or name in ("base", "__base__"):
                raise ValueError(f"--adapters: bad item {item!r} ('base' stands alone)")
            try:
                blend[name] = float(w) if sep else None
            except ValueError:
                raise ValueError(f"--adapters: weight of {name!r} in {item!r} is not a number")
            if blend[name] is not None and not np.isfinite(blend[name]):
                raise ValueError(f"--adapters: weight of {name!r} in {item!r} is not finite")
        if len(blend) == 1 and next(iter(blend.values())) is None:
            out.append(next(iter(blend)))
        else:
            out.append({n: (1.0 if w is None else w) for n, w in blend.items()})
    return out


def parse_args(argv=None):
    """the command line, checked: what needs another flag exits here (SystemExit), before any model is loaded"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", required=True, help="local diffusers-format directory of cvssp/audioldm-s-full-v2")
    ap.add_argument("--lora-weights", default=None, help="checkpoint-*/model.safetensors written by the trainer")
    ap.add_argument("--no-lora", action="store_true")
    ap.add_argument("--rank", type=int, default=2)
    ap.add_argument("--lora-alpha", type=int, default=2)
    ap.add_argument("--target-modules", default="to_q,to_v")
    ap.add_argument("--prompt", default="An instrumental hip-hop track in the subgenre of boom bap")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--scheduler", choices=["ddim", "dpmsolver++", "dpmsolver", "unipc", "euler-a"], default="ddim",
                    help="sampler: the reference's DDIM (default) or diffusers' DPMSolverMultistepScheduler from the same config "
                         "(dpmsolver uses final_sigmas_type='sigma_min'), its UniPCMultistepScheduler (unipc: predictor-corrector, for 5-10 "
                         "steps), or its EulerAncestralDiscreteScheduler (euler-a)")
    ap.add_argument("--solver-order", type=int, choices=[1, 2], default=2, help="DPM-Solver / UniPC order (ignored with --scheduler ddim / euler-a)")
    ap.add_argument("--audio-length", type=float, default=None, help="seconds (default 10, or the --init-audio clip's length)")
    ap.add_argument("--window-seconds", type=float, default=None,
                    help="long-form generation: denoise --audio-length as overlapping windows of this length (10.24 = the trained length)")
    ap.add_argument("--window-overlap-seconds", type=float, default=None, help="overlap of neighbouring windows (default: a quarter of --window-seconds)")
    ap.add_argument("--loop", action="store_true", help="with --window-seconds: a clip that closes on itself (length rounded up to whole window strides)")
    ap.add_argument("--window-prompts", default=None, metavar="A|B|C", help="with --window-seconds: one prompt per window, separated by '|'")
    ap.add_argument("--guidance-scale", type=float, default=5.0)
    ap.add_argument("--output", default="./generated_audio_LoRA/ex.wav")
    ap.add_argument("--seed", type=int, default=None, help="seed of the initial-noise generator and, with --scheduler euler-a, of the in-loop noise stream (the reference seeds "
                         "nothing, quirk Q5)")
    ap.add_argument("--init-audio", default=None, help="wav to start from (audio-to-audio), any rate: resampled to the model's on the device; read with scipy")
    ap.add_argument("--output-sampling-rate", type=int, default=None, metavar="R", help="write the wav files at R Hz (default: the model's 16000)")
    ap.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                    help="bring every clip to this ITU-R BS.1770 integrated loudness on the device, at the rate it is written at (e.g. -14)")
    ap.add_argument("--peak-ceiling", type=float, default=None, metavar="DBFS",
                    help="with --loudness: cap the gain so that the 4x oversampled peak stays at or under this level (default -1.0)")
    ap.add_argument("--strength", type=float, default=None,
                    help="with --init-audio: how much of the schedule to run (1 = from noise; default 0.5, with --repaint 1.0)")
    ap.add_argument("--repaint", default=None, metavar="JUMP_LENGTH,JUMP_N_SAMPLE",
                    help="with --init-audio and a --regenerate-* / --extend-to-seconds mask: RePaint resampling (RePaintScheduler on the "
                         "DDIM grid of --steps levels) instead of the legacy inpaint blend")
    ap.add_argument("--regenerate-seconds", default=None, help="with --init-audio: T0,T1 -- regenerate only this time span")
    ap.add_argument("--regenerate-bands", default=None, help="with --init-audio: F0,F1 -- regenerate only this fraction of the mel bins")
    ap.add_argument("--extend-to-seconds", type=float, default=None, metavar="T",
                    help="with --init-audio and --window-seconds: keep the recording and generate up to T seconds after it")
    ap.add_argument("--lora", action="append", default=[], metavar="NAME=PATH",
                    help="load a named adapter (.safetensors / .bin file or directory; repeatable).  Rank and targets come from the tensors")
    ap.add_argument("--adapters", default=None, metavar="SPEC",
                    help="per-prompt routing, one item per prompt (prompts separated by '|'): NAME, NAME:0.7, base, A:0.5+B:0.5")
    args = ap.parse_args(argv)
    if args.output_sampling_rate is not None and args.output_sampling_rate <= 0:
        ap.error("--output-sampling-rate expects a positive rate in Hz")
    if args.peak_ceiling is not None and args.loudness is None:
        ap.error("--peak-ceiling needs --loudness")
    if args.loudness is not None and not np.isfinite(args.loudness):
        ap.error("--loudness expects a finite level in LUFS")
    if args.adapters and not args.lora:
        ap.error("--adapters needs --lora NAME=PATH")
    if args.init_audio is None and (args.regenerate_seconds or args.regenerate_bands):
        ap.error("--regenerate-seconds / --regenerate-bands need --init-audio")
    if args.window_seconds is None and (args.loop or args.window_prompts or args.window_overlap_seconds is not None):
        ap.error("--loop / --window-prompts / --window-overlap-seconds need --window-seconds")
    if args.extend_to_seconds is not None:
        if args.init_audio is None or args.window_seconds is None:
            ap.error("--extend-to-seconds needs --init-audio and --window-seconds")
        if args.regenerate_seconds or args.regenerate_bands:
            ap.error("--extend-to-seconds builds its own mask (no --regenerate-seconds / --regenerate-bands)")
        if args.extend_to_seconds <= 0:
            ap.error("--extend-to-seconds expects a positive number of seconds")
    if args.repaint is not None:
        try:
            args.repaint = tuple(int(v) for v in args.repaint.split(","))
        except ValueError:
            args.repaint = ()
        if len(args.repaint) != 2 or min(args.repaint) < 1:
            ap.error("--repaint expects JUMP_LENGTH,JUMP_N_SAMPLE: two integers >= 1")
        if args.init_audio is None or not (args.regenerate_seconds or args.regenerate_bands or args.extend_to_seconds is not None):
            ap.error("--repaint needs --init-audio and a mask (--regenerate-seconds / --regenerate-bands / --extend-to-seconds)")
        if args.scheduler != "ddim":
            ap.error("--repaint brings its own sampler (RePaintScheduler on the DDIM grid): no --scheduler with it")
        if args.adapters is not None and args.window_seconds is None:
            ap.error("--repaint with --adapters needs --window-seconds (routed calls start from a recording only when windowed)")
        if args.strength not in (None, 1.0):
            ap.error("--repaint regenerates from noise: --strength must be 1.0 with it")
        args.strength = 1.0
    if args.strength is None:
        args.strength = 0.5
    for item in args.lora:
        name, sep, path = item.partition("=")
        if not sep or not name or not path:
            ap.error(f"--lora expects NAME=PATH, got {item!r}")
    return args


def main(argv=None):
    args = parse_args(argv)
    device = "cuda"
    unet = UNet2DConditionModel.from_pretrained(args.model_dir, subfolder="unet")
    if not args.no_lora and not args.lora:
        unet_lora = get_peft_model(unet, LoraConfig(r=args.rank, lora_alpha=args.lora_alpha, init_lora_weights="gaussian",
                                                    target_modules=args.target_modules.split(",")))
        if args.lora_weights:
            from safetensors.torch import load_file
            unet_lora.load_state_dict(load_file(args.lora_weights), strict=False)
    pipe = AudioLDMPipeline.from_pretrained(args.model_dir, unet=unet).to(device)
    if args.scheduler == "euler-a":
        pipe.scheduler = EulerAncestralDiscreteScheduler.from_config(pipe.scheduler.config)
    elif args.scheduler == "unipc":
        pipe.scheduler = UniPCMultistepScheduler.from_config(pipe.scheduler.config, solver_order=args.solver_order)
    elif args.scheduler != "ddim":
        extra = {"final_sigmas_type": "sigma_min"} if args.scheduler == "dpmsolver" else {}
        pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config, algorithm_type=args.scheduler,
                                                                 solver_order=args.solver_order, **extra)
    for item in args.lora:
        name, _, path = item.partition("=")
        pipe.load_lora_weights(path, adapter_name=name)
    generator = torch.Generator().manual_seed(args.seed) if args.seed is not None else None
    out_rate = int(pipe.vocoder.config.sampling_rate) if args.output_sampling_rate is None else args.output_sampling_rate
    rated = {} if args.output_sampling_rate is None else {"output_sampling_rate": args.output_sampling_rate}
    if args.loudness is not None:                       # (normalised after the resampling, at the rate the file is written at)
        rated.update(loudness_lufs=args.loudness, peak_ceiling_dbfs=-1.0 if args.peak_ceiling is None else args.peak_ceiling)
    windowed = {}
    if args.window_seconds is not None:
        windowed = dict(window_length_in_s=args.window_seconds, window_overlap_in_s=args.window_overlap_seconds, loop=args.loop)
        if args.window_prompts:
            windowed["window_prompts"] = [p.strip() for p in args.window_prompts.split("|")]
    if args.adapters is not None:
        routing = parse_adapters(args.adapters)
        prompts = [p.strip() for p in args.prompt.split("|")]
        if len(prompts) == 1:
            prompts = prompts * len(routing)
        if "window_prompts" in windowed:                # the same prompt schedule for every routed clip
            windowed["window_prompts"] = [windowed["window_prompts"]] * len(prompts)
        if args.init_audio is not None and windowed:
            audios = _audio_to_audio(pipe, args, generator, windowed, prompt=prompts, adapter_names=routing, **rated)
        else:
            audios = pipe(prompt=prompts, num_inference_steps=args.steps, adapter_names=routing,
                          audio_length_in_s=10.0 if args.audio_length is None else args.audio_length,
                          guidance_scale=args.guidance_scale, generator=generator, **windowed, **rated).audios
        from scipy.io import wavfile
        stem, ext = os.path.splitext(os.path.abspath(args.output))
        os.makedirs(os.path.dirname(stem), exist_ok=True)
        for i, a in enumerate(audios):
            wavfile.write(f"{stem}_{i}{ext or '.wav'}", out_rate, np.asarray(a, dtype=np.float32))
        print(f"Generated {len(audios)} clips saved to: {stem}_*{ext or '.wav'}")
        return
    if args.init_audio is None:
        audio = pipe(prompt=args.prompt, num_inference_steps=args.steps,
                     audio_length_in_s=10.0 if args.audio_length is None else args.audio_length,
                     guidance_scale=args.guidance_scale, generator=generator, **windowed, **rated).audios[0]
    else:
        audio = _audio_to_audio(pipe, args, generator, windowed, **rated)[0]
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    from scipy.io import wavfile
    wavfile.write(args.output, out_rate, np.asarray(audio, dtype=np.float32))
    print(f"Generated audio saved to: {args.output}")


def _pair(text, name):
    try:
        a, b = (float(v) for v in text.split(","))
    except ValueError:
        raise SystemExit(f"{name} expects two comma-separated numbers, got {text!r}")
    return a, b


def read_wav(path):
    """(rate, mono fp32 samples in [-1, 1]) of a wav file read with scipy: float data as stored, signed PCM divided by 2^(bits-1),
    8-bit PCM (unsigned, centred at 128) shifted by 128 first; channels are averaged."""
    from scipy.io import wavfile
    sr, wav = wavfile.read(path)
    wav = np.asarray(wav)
    if wav.dtype == np.uint8:
        wav = (wav.astype(np.float32) - 128.0) / 128.0
    elif np.issubdtype(wav.dtype, np.signedinteger):
        wav = wav.astype(np.float32) / float(-np.iinfo(wav.dtype).min)
    elif not np.issubdtype(wav.dtype, np.floating):
        raise ValueError(f"{path}: unsupported wav sample type {wav.dtype}")
    wav = wav.astype(np.float32)
    if wav.ndim == 2:
        wav = wav.mean(axis=1)                                  # mono
    return sr, wav


def _audio_to_audio(pipe, args, generator, windowed=None, **routed):
    """the clips of an --init-audio call; windowed: the window keywords of a --window-seconds call; routed: prompt= / adapter_names= of
    an --adapters call (one clip per routing entry, all from the same recording), output_sampling_rate= and the loudness keywords"""
    sr, wav = read_wav(args.init_audio)
    a2a = AudioLDMAudioToAudioPipeline.from_pipe(pipe)
    if args.repaint is not None:
        a2a.scheduler = RePaintScheduler.from_config(pipe.scheduler.config, jump_length=args.repaint[0], jump_n_sample=args.repaint[1])
    model_rate = int(a2a.vocoder.config.sampling_rate)
    if sr != model_rate:
        print(f"Resampling {args.init_audio}: {sr} Hz -> {model_rate} Hz")
    windowed = dict(windowed or {})
    recording = wav.shape[0] / float(sr)
    seconds = recording if args.audio_length is None else args.audio_length
    strength = args.strength
    if args.extend_to_seconds is not None:
        seconds, strength = args.extend_to_seconds, 1.0
    n_mel = a2a.vocoder.config.model_in_dim
    if windowed:                                        # the mask is the LONG clip's (a looped plan rounds its length up)
        height = a2a.window_plan(seconds, windowed["window_length_in_s"], windowed["window_overlap_in_s"], windowed["loop"])[0].rows * a2a.vae_scale_factor
    else:
        height, _ = a2a.geometry(seconds)
    mask = None
    if args.extend_to_seconds is not None:
        mask = continuation_mask(height, n_mel, recording)
    elif args.regenerate_seconds or args.regenerate_bands:
        mask = regeneration_mask(height, n_mel,
                                 seconds=_pair(args.regenerate_seconds, "--regenerate-seconds") if args.regenerate_seconds else None,
                                 bands=_pair(args.regenerate_bands, "--regenerate-bands") if args.regenerate_bands else None)
    routed.setdefault("prompt", args.prompt)
    return a2a(audio=wav, sampling_rate=sr, resample=sr != model_rate, strength=strength, mask=mask, audio_length_in_s=seconds, num_inference_steps=args.steps,
               guidance_scale=args.guidance_scale, generator=generator, **windowed, **routed).audios


if __name__ == "__main__":
    main()
