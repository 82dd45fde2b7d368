"""Times the polyphase resampler (aldm_resample_poly) on 60 s clips: 44.1 -> 16 kHz, 48 -> 16 kHz, 16 -> 44.1 kHz, 16 -> 48 kHz, and
the CLAP front end's aldm_resample_up3 on the same 16 -> 48 kHz input for comparison.

The C entries are called directly on buffers made once (the Python wrappers copy the lengths to the device on every call, which
would be timed instead).  Each case is warmed up, then timed `--repeats` times on device events around `--inner` back-to-back launches (one launch is a few
microseconds: a single one would time the event pair); the line gives the median microseconds per launch, the spread (min, max) and
the achieved bytes per second -- the bytes the algorithm needs, input read once + output written once + the phase table, over the
median -- against the 6.3 TB/s a streaming kernel reaches from HBM on the MI355X (8 TB/s peak).  One clip is 4 to 21 MB in and out,
far inside the 256 MB Infinity Cache, so the rate of `--batch 1` is a launch's latency, not a memory rate; `--batch 16` is closer
to one.  Prints one JSON line per case.

    python tools/bench_resample.py [--seconds 60] [--batch 1,16] [--warmup 20] [--repeats 20] [--inner 50]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12          # bytes / s


def timed(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(us), min(us), max(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--batch", default="1,16")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the MI355X: no GPU visible")
    from audioldm_with_lora_amd import _lib
    from audioldm_with_lora_amd import resample as R
    from audioldm_with_lora_amd.clap_audio import resample_taps
    from audioldm_with_lora_amd.ops import _p, _stream
    lib = _lib.load()
    taps3 = torch.from_numpy(resample_taps(3)).float().cuda()
    g = torch.Generator().manual_seed(0)
    for B in [int(b) for b in args.batch.split(",")]:
        for rate_in, rate_out in ((44100, 16000), (48000, 16000), (16000, 44100), (16000, 48000)):
            up, down = R.ratio(rate_in, rate_out)
            T = int(round(args.seconds * rate_in))
            x = (0.3 * torch.randn(B, T, generator=g)).clamp_(-1, 1).cuda()
            table = R.device_table(up, down, x.device)
            lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
            T_out = R.output_length(T, up, down)
            y = torch.empty(B, T_out, device="cuda")
            K, half = table.shape[1], 10 * max(up, down)
            nbytes = 4.0 * B * (T + T_out) + 4.0 * table.numel()
            cases = [("aldm_resample_poly", lambda: _lib.check(lib.aldm_resample_poly(_p(x), _p(lens), B, T, _p(table), up, down, K, half, _p(y),
                                                                                      T_out, _stream()), "aldm_resample_poly"))]
            if (up, down) == (3, 1):
                cases.append(("aldm_resample_up3", lambda: _lib.check(lib.aldm_resample_up3(_p(x), _p(lens), B, T, _p(taps3), taps3.numel(), _p(y),
                                                                                        T_out, _stream()), "aldm_resample_up3")))
            for name, fn in cases:
                med, lo, hi = timed(fn, args.warmup, args.repeats, args.inner)
                print(json.dumps({"kernel": name, "rates": f"{rate_in}->{rate_out}", "up": up, "down": down, "batch": B, "seconds": args.seconds,
                                  "taps_per_output": table.shape[1], "us_median": round(med, 2), "us_min": round(lo, 2),
                                  "us_max": round(hi, 2), "mbytes": round(nbytes / 1e6, 2), "tbytes_per_s": round(nbytes / med / 1e6, 3),
                                  "share_of_hbm_6.3TBps": round(nbytes / med / 1e6 / (HBM_ACHIEVABLE / 1e12), 3)}), flush=True)


if __name__ == "__main__":
    main()
