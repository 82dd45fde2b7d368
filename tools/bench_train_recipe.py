"""What the training-recipe options cost on the flagship training workload (bench.py's bench_train: full-size UNet, rank-8 LoRA on
q / k / v / out, batch 8 of [8, 256, 16] latents, graph replay).

Three configurations, timed in alternating rounds so that drift of the machine shows up as spread and not as a difference:
    a  defaults                                (the launch sequence of bench.py: ms per optimiser step)
    b  max_grad_norm=1.0, snr_gamma=5          (expected over a: one launch + one 7 MB read; ms per optimiser step)
    c  b with gradient_accumulation_steps=4    (expected over a: one accum_flat launch; ms per MICRO-step)
Prints one JSON line: per configuration the median over rounds and the min / max (the run-to-run spread of this process).

    python tools/bench_train_recipe.py --steps 40 --warmup 8 --rounds 5
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "a_defaults": {},
    "b_clip_snr": dict(max_grad_norm=1.0, snr_gamma=5.0),
    "c_clip_snr_accum4": dict(max_grad_norm=1.0, snr_gamma=5.0, gradient_accumulation_steps=4),
}


def make_trainer(batch, rank_lora, **kw):
    from audioldm_with_lora_amd.lora import LoraConfig, get_peft_model
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from audioldm_with_lora_amd.training import LoraTrainer
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    torch.manual_seed(1234)
    unet = UNet2DConditionModel()
    get_peft_model(unet, LoraConfig(r=rank_lora, lora_alpha=rank_lora, init_lora_weights="gaussian",
                                    target_modules=["to_q", "to_k", "to_v", "to_out.0"]))
    unet.cuda()
    return LoraTrainer(unet, DDIMScheduler(), lr=1e-5, weight_decay=1e-5, max_train_steps=97000, **kw)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed calls of step() per configuration and round (a multiple of 4)")
    ap.add_argument("--warmup", type=int, default=8, help="untimed calls first (two eager steps, the capture, then replays)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rank", type=int, default=8)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_recipe needs the MI355X: a CPU run cannot give a time")
    if args.steps % 4 or args.warmup % 4:
        raise SystemExit("--steps and --warmup must be multiples of 4 (the accumulation window of configuration c)")
    g = torch.Generator().manual_seed(5)
    lat = (torch.randn(args.batch, 8, 256, 16, generator=g) * 0.9228).cuda()
    noise = torch.randn(args.batch, 8, 256, 16, generator=g).cuda()
    t = torch.randint(0, 1000, (args.batch,), generator=g).cuda()
    emb = torch.nn.functional.normalize(torch.randn(args.batch, 512, generator=g), dim=-1).cuda()
    trainers = {name: make_trainer(args.batch, args.rank, **kw) for name, kw in CONFIGS.items()}
    for tr in trainers.values():
        for _ in range(args.warmup):
            tr.step(lat, noise, t, emb)
    torch.cuda.synchronize()
    ms = {name: [] for name in trainers}
    for _ in range(args.rounds):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = tr.step(lat, noise, t, emb)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            assert torch.isfinite(loss).all()
    out = {"metric": "lora_train_recipe_ms_per_call", "unit": "ms per step() call (c: per micro-step)", "per_gpu_batch": args.batch,
           "lora_rank": args.rank, "steps": args.steps, "rounds": args.rounds}
    for name, v in ms.items():
        out[name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    out["grad_norm_b"] = round(float(trainers["b_clip_snr"].last_grad_norm), 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
