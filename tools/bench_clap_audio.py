"""Times the CLAP audio front end (16 kHz -> 48 kHz resample + log-mel) and the fused HTSAT tower separately on device events,
after a warm-up, at batch 1 / 8 / 32 of 10 s clips, with recipe weights (tests/clap_audio_weights.py).  Prints one JSON line
per batch: clips/s of each part and the tower's achieved TFLOP/s, FLOPs counted from the shapes (GEMMs + attention).

    python tools/bench_clap_audio.py [--batches 1,8,32] [--reps 10]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def tower_flops(cfg):
    """Multiply-adds x 2 of one clip through the tower: patch embedding (+ fusion), every block, merges, head."""
    c0, f = cfg["patch_embeds_hidden_size"], 0.0
    T = 4096
    f += 2 * T * 16 * c0
    if cfg["enable_fusion"]:
        i = c0 // cfg["aff_block_r"]
        f += 2 * T * 48 * c0 + 2 * T * (c0 * i * 2)
    for s, (d, h) in enumerate(zip(cfg["depths"], cfg["num_attention_heads"])):
        C, N = c0 * 2 ** s, T >> (2 * s)
        blk = 2 * N * C * 3 * C + 2 * N * C * C + 2 * N * C * 4 * C * 2 + 2 * 2 * N * 64 * C
        f += d * blk
        if s < len(cfg["depths"]) - 1:
            f += 2 * (N // 4) * 4 * C * 2 * C
    f += 2 * cfg["hidden_size"] * cfg["projection_dim"] + 2 * cfg["projection_dim"] ** 2
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import clap_audio_weights as W
    from audioldm_with_lora_amd.clap_audio import ClapAudioFrontEnd, ClapAudioModelWithProjection
    m = ClapAudioModelWithProjection(**W.audio_config("fused"))
    m.load_state_dict(W.audio_state_dict("fused"))
    m = m.to("cuda")
    fe = ClapAudioFrontEnd("cuda")
    flops = tower_flops(m.cfg)
    for B in [int(b) for b in args.batches.split(",")]:
        wav = torch.stack([torch.from_numpy(W.wave16k(10.0, i)) for i in range(B)]).cuda()
        for _ in range(3):
            f = fe(wav, sampling_rate=16000)
            m(f.input_features, f.is_longer)
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t_fe = t_tw = 0.0
        for _ in range(args.reps):
            e[0].record()
            f = fe(wav, sampling_rate=16000)
            e[1].record()
            m(f.input_features, f.is_longer)
            e[2].record()
            torch.cuda.synchronize()
            t_fe += e[0].elapsed_time(e[1]) / args.reps
            t_tw += e[1].elapsed_time(e[2]) / args.reps
        print(json.dumps({"batch": B, "front_end_ms": round(t_fe, 3), "tower_ms": round(t_tw, 3),
                          "front_end_clips_per_s": round(B / t_fe * 1e3, 1), "tower_clips_per_s": round(B / t_tw * 1e3, 1),
                          "tower_gflop_per_clip": round(flops / 1e9, 2), "tower_tflops": round(flops * B / t_tw / 1e9, 2)}))


if __name__ == "__main__":
    main()
