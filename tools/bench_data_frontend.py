"""Times the clip front end of the training data path (data.py): batches of `--batch` clips cut out of
`--seconds`-long recordings at `--rate` Hz that are resident on the device, through segment -> resample -> normalise -> log-mel.

Two figures, one JSON line:
  clips_per_s      ClipLoader.next_batch as a training loop calls it -- the host work of a batch (index lists, the small
                   host-to-device copies of offsets and lengths, eight launches) included -- over a host clock around `--batches`
                   batches that ends in a device synchronise, the median of `--repeats` such windows (with the spread);
  stage_us         device-event medians of the four stages of one batch, each through its ops wrapper on inputs made once.
The recordings are seeded noise with a silent first quarter, so some candidate windows miss, as in real recordings.

    python tools/bench_data_frontend.py [--batch 64] [--seconds 30] [--rate 44100] [--recordings 128] [--batches 50] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class ResidentNoise:
    """what ClipLoader reads of a dataset: rates, offsets, lens, pools, input_ids, attention_mask"""

    def __init__(self, n, length, rate, device):
        g = torch.Generator(device=device).manual_seed(0)
        pool = (0.3 * torch.randn(n, length, generator=g, device=device)).clamp_(-1, 1)
        pool[:, :length // 4] = 0.0
        self.pools = {rate: pool.reshape(-1)}
        self.rates, self.lens, self.offsets = [rate] * n, [length] * n, [i * length for i in range(n)]
        self.input_ids = torch.ones(n, 1, 512, dtype=torch.long)
        self.attention_mask = torch.ones(n, 1, 512, dtype=torch.long)

    def __len__(self):
        return len(self.rates)


def event_us(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(us), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--recordings", type=int, default=128)
    ap.add_argument("--duration", type=float, default=10.24)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_data_frontend.py measures on the MI355X: no GPU visible")
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd import resample as R
    from audioldm_with_lora_amd.data import ClipFrontEnd, ClipLoader
    dev = torch.device("cuda")
    L = int(round(args.seconds * args.rate))
    ds = ResidentNoise(args.recordings, L, args.rate, dev)
    fe = ClipFrontEnd(dev, duration=args.duration, seed=1)
    loader = ClipLoader(ds, fe, args.batch, seed=1)
    for _ in range(5):
        loader.next_batch()
    torch.cuda.synchronize()
    rates = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.batches):
            loader.next_batch()
        torch.cuda.synchronize()
        rates.append(args.batches * args.batch / (time.perf_counter() - t0))

    # the stages of one batch on their own
    B, S = args.batch, fe.segment_length(args.rate)
    pool = ds.pools[args.rate]
    offsets = torch.tensor(ds.offsets[:B], dtype=torch.int64, device=dev)
    lens = torch.tensor(ds.lens[:B], dtype=torch.int32, device=dev)
    ords = torch.arange(B, dtype=torch.int32, device=dev)
    seg, _ = ops.clip_segment(pool, offsets, lens, ords, S, fe.state, max_len=L)
    up, down = R.ratio(args.rate, fe.sampling_rate)
    stage = {"segment": event_us(lambda: ops.clip_segment(pool, offsets, lens, ords, S, fe.state, max_len=L), 5, 20)}
    y, n = seg, [S] * B
    if up != down:
        table = R.device_table(up, down, dev)                     # as the front end passes it
        n_in = n
        y, n = ops.resample_poly(seg, up, down, lens=n_in, table=table)
        stage["resample"] = event_us(lambda: ops.resample_poly(seg, up, down, lens=n_in, table=table), 5, 20)
    n_dev = torch.as_tensor(n, dtype=torch.int32).to(dev)
    wav = ops.clip_normalize(y, n_dev, fe.target)
    stage["normalize"] = event_us(lambda: ops.clip_normalize(y, n_dev, fe.target), 5, 20)
    stage["log_mel"] = event_us(lambda: fe.log_mel(wav), 5, 20)
    print(json.dumps({"bench": "data_frontend", "batch": B, "seconds": args.seconds, "rate": args.rate, "recordings": args.recordings,
                      "duration": args.duration, "clips_per_s": round(statistics.median(rates), 1),
                      "clips_per_s_min": round(min(rates), 1), "clips_per_s_max": round(max(rates), 1),
                      "ms_per_batch": round(1e3 * B / statistics.median(rates), 3), "stage_us": stage,
                      "stage_us_sum": round(sum(stage.values()), 1)}), flush=True)


if __name__ == "__main__":
    main()
