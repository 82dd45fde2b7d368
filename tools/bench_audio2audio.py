"""Audio-to-audio at config 2 (4 prompts x 10 s, CFG 2.5, rank-4 LoRA, random-init weights), built the way tools/bench_solvers.py builds
its pipeline: per sampler (DDIM, DPM-Solver++ second order) the graph-replayed step with and without the inpainting blend, and one
end-to-end style-transfer call at strength 0.5 split into encode (log-mel + VAE encode + posterior sample + add_noise), loop and
decode (VAE decode + vocoder).

    python tools/bench_audio2audio.py [--repeats 5] [--steps 50]

ms_per_step: a begun (strength 0.5) engine after one set_latents, `run()` timed with device synchronisation around the host clock,
median of `repeats`, divided by the suffix length.  masked and unmasked engines run the same suffix.  Prints one JSON line.

    python tools/bench_audio2audio.py --repaint [--repeats 5] [--steps 50]

measures RePaint instead and prints one JSON line of its own: the in-graph time of the masked fused-step launch
alone for DDIM, Euler-ancestral and RePaint on the same eps (a graph of 200 launches walking each solver's own table, device events
around 20 replays, median of `repeats`, the three solvers alternating), and one inpainting call (3 s of 10 s regenerated, strength 1.0)
at `steps` grid levels with RePaintScheduler(jump_length=5, jump_n_sample=3) against the same call on DDIM.
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


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return out[len(out) // 2]


def repaint_numbers(args):
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.audio2audio import AudioLDMAudioToAudioPipeline, reduce_mask, regeneration_mask
    from audioldm_with_lora_amd.pipeline import AudioLDMPipeline
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, EulerAncestralDiscreteScheduler, RePaintScheduler
    from audioldm_with_lora_amd.vae import AutoencoderKL
    from audioldm_with_lora_amd.vocoder import SpeechT5HifiGan
    batch, seconds, guidance, N = 4, 10.0, 2.5, args.steps
    height = int(seconds * 100)
    h, w = height // 4, 16
    g = torch.Generator().manual_seed(5)
    mask = reduce_mask(regeneration_mask(height, 64, seconds=(3.0, 6.0))[None].expand(batch, -1, -1), 4)

    # ---- the masked launch alone, inside a graph ----
    dims = (batch, h, w, 8)
    eps = torch.randn((2 * batch,) + dims[1:], generator=g).cuda()
    x0, nz, md = torch.randn(dims, generator=g).cuda(), torch.randn(dims, generator=g).cuda(), mask.cuda()
    scheds = {"ddim": DDIMScheduler(), "euler_a": EulerAncestralDiscreteScheduler.from_config(DDIMScheduler().config),
              "repaint": RePaintScheduler.from_config(DDIMScheduler().config, jump_length=5, jump_n_sample=3)}
    tables = {}
    for name, sch in scheds.items():
        sch.set_timesteps(N)
        tables[name] = (name, sch.coefficient_table().cuda(), sch.blend_table(0).cuda(), sch.timesteps.float().cuda())
    name, coef, blend, ts = tables["repaint"]
    jump = coef[coef[:, 5] > 0][:1].expand(len(coef), 8).contiguous()       # every row the first jump row: the launch's upper end
    tables["repaint_every_row_jumps"] = (name, jump, blend, ts)
    LAUNCHES, REPLAYS = 200, 20
    graphs = {}
    for key, (name, coef, blend, ts) in tables.items():
        x = torch.randn(dims, generator=g).cuda()
        buf = dict(x=x, x_in=torch.zeros((2 * batch,) + dims[1:], dtype=torch.bfloat16, device="cuda"), idx=torch.zeros(1, dtype=torch.int32, device="cuda"),
                   t=torch.zeros(1, device="cuda"), ticket=torch.zeros(1, dtype=torch.int32, device="cuda"))
        operand = () if name == "ddim" else (ops.philox_state(1, 0),)
        fn = getattr(ops, name + "_step_fused_masked")

        def launch(buf=buf, coef=coef, blend=blend, ts=ts, operand=operand, fn=fn):
            fn(eps, buf["x"], True, guidance, coef, buf["idx"], buf["x_in"], *operand, None, None, ts, buf["t"], buf["ticket"], x0, nz, md, blend)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launch()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            for _ in range(LAUNCHES):
                launch()
        graphs[key] = (graph, buf)
    times = {key: [] for key in graphs}
    for rep_i in range(args.repeats + 1):
        for key, (graph, buf) in graphs.items():
            buf["x"].normal_()                                       # (the values do not change the work; keeps them finite)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPLAYS):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            if rep_i:                                                # the first round warms up
                times[key].append(a.elapsed_time(b) * 1e3 / (REPLAYS * LAUNCHES))
    launch_us = {key: round(sorted(v)[len(v) // 2], 3) for key, v in times.items()}

    # ---- one inpainting call ----
    unet, _ = build_unet(4)
    torch.manual_seed(99)
    base = AudioLDMPipeline(AutoencoderKL(), None, None, unet, DDIMScheduler(), SpeechT5HifiGan())
    base.device = torch.device("cuda")
    base.vae.cuda(); base.vocoder.cuda()
    pipe = AudioLDMAudioToAudioPipeline.from_pipe(base)
    _, pe, ne = synth_inputs(batch, h, w)
    audio = 0.1 * torch.randn(batch, int(seconds * 16000), generator=g)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, strength=1.0, mask=regeneration_mask(height, 64, seconds=(3.0, 6.0)),
                num_inference_steps=N, guidance_scale=guidance)
    calls = {}
    for name in ("ddim", "repaint"):
        pipe.scheduler = scheds[name]
        pipe(generator=torch.Generator().manual_seed(1), **call)                    # warm-up: engine build + capture
        ms = timed(lambda: pipe(generator=torch.Generator().manual_seed(1), **call), args.repeats)
        calls[name] = {"unet_calls": len(pipe.scheduler.timesteps), "ms_per_call": round(ms, 1)}
    print(json.dumps({"what": "RePaint at config 2 (4 x 10 s, CFG 2.5, rank-4 LoRA, random-init weights, 3 s of 10 s regenerated): "
                              "masked_launch_us = the masked fused step alone inside a graph, per launch; inpaint_call = one a2a call at "
                              f"strength 1.0, {N} grid levels, RePaint jump_length 5 x jump_n_sample 3 against DDIM's legacy blend",
                      "masked_launch_us": launch_us, "inpaint_call": calls}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repaint", action="store_true", help="measure the RePaint launch and call instead (DESIGN.md section 23)")
    args = ap.parse_args()
    if args.repaint:
        return repaint_numbers(args)
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.audio2audio import AudioLDMAudioToAudioPipeline, reduce_mask, regeneration_mask
    from audioldm_with_lora_amd.mel import LogMelFrontEnd
    from audioldm_with_lora_amd.pipeline import AudioLDMPipeline
    from audioldm_with_lora_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    from audioldm_with_lora_amd.vae import AutoencoderKL
    from audioldm_with_lora_amd.vocoder import SpeechT5HifiGan
    batch, seconds, guidance, strength, N = 4, 10.0, 2.5, 0.5, args.steps
    unet, _ = build_unet(4)
    torch.manual_seed(99)
    base = AudioLDMPipeline(AutoencoderKL(), None, None, unet, DDIMScheduler(), SpeechT5HifiGan())
    base.device = torch.device("cuda")
    base.vae.cuda(); base.vocoder.cuda()
    pipe = AudioLDMAudioToAudioPipeline.from_pipe(base)
    height = int(seconds * 100)
    h, w = height // 4, 16
    lat, pe, ne = synth_inputs(batch, h, w)
    g = torch.Generator().manual_seed(5)
    audio = 0.1 * torch.randn(batch, int(seconds * 16000), generator=g)
    x0 = torch.randn(batch, 8, h, w, generator=g)
    mask = reduce_mask(regeneration_mask(height, 64, seconds=(3.0, 6.0))[None].expand(batch, -1, -1), 4)

    res = {}
    for name, sched in (("ddim", DDIMScheduler()), ("dpmsolver++", DPMSolverMultistepScheduler.from_config(DDIMScheduler().config))):
        pipe.scheduler = sched
        _, begin = sched.get_timesteps(N, strength)
        row = {"steps": N, "suffix_steps": N - begin}
        for masked in (False, True):
            eng = pipe.engine(batch, h, w, N, guidance, begin_index=begin, masked=masked)
            eng.set_condition(pe, ne)
            eng.set_latents(lat)
            if masked:
                eng.set_inpaint(x0, lat, mask)
            eng.capture()
            eng.run()
            eng.set_latents(lat)
            row["ms_per_step_masked" if masked else "ms_per_step"] = round(timed(eng.run, args.repeats) / eng.n_steps, 4)
        row["masked_minus_unmasked_us"] = round(1e3 * (row["ms_per_step_masked"] - row["ms_per_step"]), 1)
        res[name] = row

    # one end-to-end style-transfer call (DDIM, strength 0.5), split into its three stages
    pipe.scheduler = DDIMScheduler()
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, strength=strength, num_inference_steps=N, guidance_scale=guidance)
    pipe(generator=torch.Generator().manual_seed(1), **call)                        # warm-up: engine build + capture
    call_ms = timed(lambda: pipe(generator=torch.Generator().manual_seed(1), **call), args.repeats)
    _, begin = pipe.scheduler.get_timesteps(N, strength)
    fe = LogMelFrontEnd(target_length=height, n_mel=64)
    post = torch.randn(batch, 8, h, w).cuda()
    wav_d = audio.cuda()

    def encode():
        dist = pipe.vae.encode(fe(wav_d)).latent_dist
        z = ops.gaussian_sample(dist.parameters.float(), post) * pipe.vae.config.scaling_factor
        a, s = pipe.scheduler.add_noise_coefficients(begin)
        return ops.add_noise(z, lat.cuda(), torch.tensor([float(a), float(s)] * batch, device="cuda"))
    eng = pipe.engine(batch, h, w, N, guidance, begin_index=begin, masked=False)
    x = encode()

    def loop():
        eng.set_latents(x)
        eng.run()
    enc_ms, loop_ms = timed(encode, args.repeats), timed(loop, args.repeats)
    dec_ms = timed(lambda: pipe.decode_latents_nhwc(eng.x), args.repeats)
    res["style_transfer_call"] = {"strength": strength, "steps": N, "suffix_steps": N - begin, "ms_per_call": round(call_ms, 1),
                                  "encode_ms": round(enc_ms, 2), "loop_ms": round(loop_ms, 1), "decode_ms": round(dec_ms, 2)}
    print(json.dumps({"what": "audio-to-audio at config 2 (4 x 10 s, CFG 2.5, rank-4 LoRA, random-init weights); ms_per_step = graph "
                              "replays of a strength-0.5 suffix, masked = with the inpainting blend (3 s of 10 s regenerated)",
                      "results": res}))


if __name__ == "__main__":
    main()
