"""Audio-to-audio at config 2 (4 prompts x 10 s, CFG 2.5, rank-4 LoRA, random-init weights), built the way tools/bench_solvers.py builds
its pipeline: per sampler (DDIM, DPM-Solver++ second order) the graph-replayed step with and without the inpainting blend, and one
end-to-end style-transfer call at strength 0.5 split into encode (log-mel + VAE encode + posterior sample + add_noise), loop and
decode (VAE decode + vocoder).

    python tools/bench_audio2audio.py [--repeats 5] [--steps 50]

ms_per_step: a begun (strength 0.5) engine after one set_latents, `run()` timed with device synchronisation around the host clock,
median of `repeats`, divided by the suffix length.  masked and unmasked engines run the same suffix.  Prints one JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
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
