"""Long-form generation at the size the feature is for: 60 s as windows of 10.24 s overlapping by 2.56 s (1500 latent rows, 8 windows
of 256), B = 1, CFG 2.5, full-width UNet with a rank-4 LoRA, random-init weights, DDIM.

    python tools/bench_longform.py [--seconds 60] [--steps 10] [--reps 20] [--skip-unwindowed]

Prints one JSON line:
  launches_per_step, ms_per_step     one windowed denoise step (UNet on 2 * B * K windows + the windowed fused step): the C-ABI calls
                                     of one eager step counted by ops.PROFILE, and the captured step's replays timed by events
  windowed_step_us / plain_step_us   the windowed fused step launch alone, and the plain fused step on a latent of as many eps
                                     bytes ([B * K, 256, 16, 8]), each as `reps` launches inside one replayed graph (the in-graph
                                     timer of tools/bench_graph.py: launches back to back, no Python floor)
  pipe_ms                            one whole pipe(...) call, windowed (second call: engine built, graph captured)
  unwindowed                         whether pipe(audio_length_in_s=seconds) WITHOUT windows runs at all on this tree -- the UNet's
                                     self-attention over all 1500 x 16 tokens, the VAE's wide head -- and its time if it does

    python tools/bench_longform.py --audio-to-audio [--seconds 60] [--steps 20] [--reps 20]

The audio-to-audio leg instead: a synthetic recording of `seconds`, strength 0.5 (the second half of `steps`),
the middle third regenerated.  One JSON line:
  first_a2a_ms_incl_capture, a2a_ms  the first call of a2a(...) (engine built, graph captured) and a later one
  encode_ms                          the one-off windowed encode: log-mel, gather, VAE encoder on the windows, moment blend, sample
  launches_per_step, ms_per_step     one masked windowed denoise step, as above
  masked_windowed_step_us / windowed_step_us / plain_masked_step_us
                                     the masked windowed launch, the unmasked windowed launch and the plain masked launch at the same
                                     number of eps bytes, each inside one replayed graph, in this one run
  extra_long_bytes                   what the masked windowed launch reads on top of the unmasked one: x0, noise and the mask
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import build_unet, synth_inputs  # noqa: E402


def in_graph_us(fn, reps):
    """microseconds per call of fn inside a replayed graph of `reps` calls (best of 5 replays)"""
    from audioldm_with_lora_amd import ops  # noqa: F401
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
    return best


def audio_to_audio_leg(args, pipe, plan, pe, ne, guidance):
    """the measurements of the --audio-to-audio leg (module docstring) as a dict"""
    import numpy as np
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.audio2audio import AudioLDMAudioToAudioPipeline, regeneration_mask
    from audioldm_with_lora_amd.mel import LogMelFrontEnd
    a2a = AudioLDMAudioToAudioPipeline.from_pipe(pipe)
    n = int(args.seconds * 16000)
    t = torch.arange(n) / 16000.0
    wav = 0.3 * torch.sin(2 * np.pi * 220.0 * t) + 0.05 * torch.randn(n, generator=torch.Generator().manual_seed(3))
    frames = plan.rows * a2a.vae_scale_factor
    mask = regeneration_mask(frames, 64, seconds=(args.seconds / 3, 2 * args.seconds / 3))
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=wav, strength=0.5, mask=mask, num_inference_steps=args.steps,
                guidance_scale=guidance, window_length_in_s=args.window_seconds, window_overlap_in_s=args.overlap_seconds)
    res = {"what": "long-form audio-to-audio, full-width UNet + rank-4 LoRA, random-init weights, B = 1, CFG 2.5, DDIM, strength 0.5, masked",
           "seconds": args.seconds, "rows": plan.rows, "windows": plan.K, "steps": args.steps}
    t0 = time.perf_counter()
    audio = a2a(generator=torch.Generator().manual_seed(1), **call).audios
    torch.cuda.synchronize()
    res["first_a2a_ms_incl_capture"] = round((time.perf_counter() - t0) * 1e3, 1)
    assert audio.shape == (1, n) and bool((audio == audio).all())
    t0 = time.perf_counter()
    a2a(generator=torch.Generator().manual_seed(1), **call)
    torch.cuda.synchronize()
    res["a2a_ms"] = round((time.perf_counter() - t0) * 1e3, 1)

    # the one-off windowed encode
    _, mel_plan = a2a.window_plan(args.seconds, args.window_seconds, args.overlap_seconds)
    front = LogMelFrontEnd(device="cuda", target_length=frames, n_mel=64)
    post = torch.randn(1, 8, plan.rows, 16, device="cuda")
    wav_dev = wav[None].cuda()
    encode = lambda: ops.gaussian_sample(a2a.encode_windows(front(wav_dev), plan, mel_plan), post)
    encode()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); encode(); e1.record(); torch.cuda.synchronize()
    res["encode_ms"] = round(e0.elapsed_time(e1), 3)

    # the step: launches counted on one eager step, replays timed
    _, begin = a2a.scheduler.get_timesteps(args.steps, 0.5)
    eng = a2a.engine(1, plan.rows, 16, args.steps, guidance, begin_index=begin, masked=True, plan=plan)
    x = torch.randn(1, 8, plan.rows, 16)
    eng.set_latents(x)
    ops.PROFILE = []
    eng._one_step()
    torch.cuda.synchronize()
    res["launches_per_step"], ops.PROFILE = len(ops.PROFILE), None
    eng.set_latents(x)
    torch.cuda.synchronize()
    e0.record(); eng.run(); e1.record(); torch.cuda.synchronize()
    res["suffix_steps"], res["ms_per_step"] = eng.n_steps, round(e0.elapsed_time(e1) / eng.n_steps, 3)

    # the three launches at the same number of eps bytes, in this one run
    K, hw = plan.K, plan.window_rows
    eps = torch.randn(2 * K, hw, 16, 8, device="cuda")
    win = plan.device("cuda")
    x_long, x_plain = torch.randn(1, plan.rows, 16, 8, device="cuda"), torch.randn(K, hw, 16, 8, device="cuda")
    long_in = (torch.randn_like(x_long), torch.randn_like(x_long), torch.rand(1, plan.rows, 16, device="cuda"), eng.blend)
    plain_in = (torch.randn_like(x_plain), torch.randn_like(x_plain), torch.rand(K, hw, 16, device="cuda"), eng.blend)
    xin = torch.zeros(2 * K, hw, 16, 8, dtype=torch.bfloat16, device="cuda")
    idx, tb, ticket = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    frame = (eng.temb[0], eng.rowbias[0], eng.timesteps_f32, tb, ticket)
    res["masked_windowed_step_us"] = round(in_graph_us(lambda: ops.ddim_step_fused_windowed_masked(
        eps, x_long, True, guidance, eng.coef, idx, xin, *frame, win, *long_in), args.reps), 2)
    res["windowed_step_us"] = round(in_graph_us(lambda: ops.ddim_step_fused_windowed(
        eps, x_long, True, guidance, eng.coef, idx, xin, *frame, win), args.reps), 2)
    res["plain_masked_step_us"] = round(in_graph_us(lambda: ops.ddim_step_fused_masked(
        eps, x_plain, True, guidance, eng.coef, idx, xin, *frame, *plain_in), args.reps), 2)
    res["eps_bytes"] = eps.numel() * 4
    res["extra_long_bytes"] = 2 * x_long.numel() * 4 + long_in[2].numel() * 4
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--window-seconds", type=float, default=10.24)
    ap.add_argument("--overlap-seconds", type=float, default=2.56)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-unwindowed", action="store_true")
    ap.add_argument("--audio-to-audio", action="store_true", help="measure the long-form audio-to-audio call instead (DESIGN.md section 19)")
    args = ap.parse_args()
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.pipeline import AudioLDMPipeline
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from audioldm_with_lora_amd.vae import AutoencoderKL
    from audioldm_with_lora_amd.vocoder import SpeechT5HifiGan
    guidance = 2.5
    unet, _ = build_unet(4)
    torch.manual_seed(99)
    pipe = AudioLDMPipeline(AutoencoderKL(), None, None, unet, DDIMScheduler(), SpeechT5HifiGan())
    pipe.device = torch.device("cuda")
    pipe.vae.cuda(); pipe.vocoder.cuda()
    plan, _ = pipe.window_plan(args.seconds, args.window_seconds, args.overlap_seconds)
    lat, pe, ne = synth_inputs(1, plan.rows, 16)
    if args.audio_to_audio:
        print(json.dumps(audio_to_audio_leg(args, pipe, plan, pe, ne, guidance)))
        return
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio_length_in_s=args.seconds, num_inference_steps=args.steps,
                guidance_scale=guidance)
    windowed = dict(call, window_length_in_s=args.window_seconds, window_overlap_in_s=args.overlap_seconds)
    res = {"seconds": args.seconds, "rows": plan.rows, "window_rows": plan.window_rows, "overlap_rows": plan.overlap_rows, "windows": plan.K,
           "max_cover": plan.KC, "steps": args.steps}

    # one whole call (the first one builds the engine and captures the graph)
    t0 = time.perf_counter()
    audio = pipe(latents=lat.clone(), **windowed).audios
    torch.cuda.synchronize()
    res["first_pipe_ms_incl_capture"] = round((time.perf_counter() - t0) * 1e3, 1)
    assert audio.shape == (1, int(args.seconds * 16000)) and bool((audio == audio).all())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipe(latents=lat.clone(), **windowed)
    torch.cuda.synchronize()
    res["pipe_ms"] = round((time.perf_counter() - t0) * 1e3, 1)

    # the step: launches counted on one eager step, replays timed
    eng = pipe.engine(1, plan.rows, 16, args.steps, guidance, plan=plan)
    eng.set_latents(lat.cuda())
    ops.PROFILE = []
    eng._one_step()
    torch.cuda.synchronize()
    res["launches_per_step"], ops.PROFILE = len(ops.PROFILE), None
    eng.set_latents(lat.cuda())
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); eng.run(); e1.record(); torch.cuda.synchronize()
    res["ms_per_step"] = round(e0.elapsed_time(e1) / args.steps, 3)

    # the windowed fused step alone, beside the plain fused step at the same number of eps bytes
    K, hw = plan.K, plan.window_rows
    eps = torch.randn(2 * K, hw, 16, 8, device="cuda")
    win = plan.device("cuda")
    x_long, x_plain = torch.randn(1, plan.rows, 16, 8, device="cuda"), torch.randn(K, hw, 16, 8, device="cuda")
    xin = torch.zeros(2 * K, hw, 16, 8, dtype=torch.bfloat16, device="cuda")
    idx, t, ticket = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    res["windowed_step_us"] = round(in_graph_us(lambda: ops.ddim_step_fused_windowed(
        eps, x_long, True, guidance, eng.coef, idx, xin, eng.temb[0], eng.rowbias[0], eng.timesteps_f32, t, ticket, win), args.reps), 2)
    res["plain_step_us"] = round(in_graph_us(lambda: ops.ddim_step_fused(
        eps, x_plain, True, guidance, eng.coef, idx, xin, eng.temb[0], eng.rowbias[0], eng.timesteps_f32, t, ticket), args.reps), 2)
    res["eps_bytes"] = eps.numel() * 4

    # does the unwindowed call run at all at this length?
    if not args.skip_unwindowed:
        lat1, _, _ = synth_inputs(1, pipe.geometry(args.seconds)[0] // pipe.vae_scale_factor, 16)
        try:
            pipe(latents=lat1.clone(), **call)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe(latents=lat1.clone(), **call)
            torch.cuda.synchronize()
            res["unwindowed"] = {"runs": True, "pipe_ms": round((time.perf_counter() - t0) * 1e3, 1)}
        except Exception as e:                                   # report, do not hide: the answer IS whether it runs
            res["unwindowed"] = {"runs": False, "error": f"{type(e).__name__}: {str(e)[:300]}"}
    print(json.dumps({"what": "long-form generation, full-width UNet + rank-4 LoRA, random-init weights, B = 1, CFG 2.5, DDIM", **res}))


if __name__ == "__main__":
    main()
