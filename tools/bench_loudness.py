"""Times BS.1770 loudness normalisation (loudness.py) on the MI355X: the whole chain -- K-weighted hop energies,
gate, 4x oversampling, peak, gain -- captured once in a graph and replayed, for the two shapes the pipelines meet:

    4 x 10 s at 16 kHz        a batch of generated clips at the vocoder's rate
    1 x 60 s at 48 kHz        one long-form clip delivered at 48 kHz

One JSON line: the median device time of a replay in microseconds per shape (with the spread over `--repeats` replays), and the
measurement alone (hop energies + gate) beside it.

    python tools/bench_loudness.py [--repeats 50] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def replay_us(fn, warmup, repeats):
    """fn captured in a graph; the median, minimum and maximum device time of a replay"""
    fn()                                                             # tables, the library and the allocator's pools, outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loudness.py measures on the MI355X: no GPU visible")
    from audioldm_with_lora_amd.loudness import LoudnessMeter
    dev = torch.device("cuda")
    out = {"bench": "loudness"}
    for name, B, seconds, rate in (("4x10s_16k", 4, 10.0, 16000), ("1x60s_48k", 1, 60.0, 48000)):
        T = int(seconds * rate)
        g = torch.Generator(device=dev).manual_seed(0)
        x = (0.1 * torch.randn(B, T, generator=g, device=dev)).clamp_(-1, 1)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        m = LoudnessMeter(rate, dev)
        out[name] = {"normalize_us": replay_us(lambda: m.normalize(x, -14.0, -1.0, lens=lens), args.warmup, args.repeats),
                     "measure_us": replay_us(lambda: m.measure(x, lens), args.warmup, args.repeats),
                     "lufs": [round(v, 3) for v in m.measure(x, lens).tolist()]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
