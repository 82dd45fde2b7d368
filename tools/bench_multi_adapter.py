"""Cost of per-clip adapter routing at config 2 (4 clips x 10 s, CFG 2.5, 200 DDIM steps, random-init weights, adapters of the reference's
kind: r = 2 on to_q / to_v):

  (a) ms per step of a GATED engine -- four adapters, routed one per clip -- next to the ungated single-adapter engine;
  (b) the wall time of switching the routing on the gated engine (engine.set_adapters + one step) next to the single-adapter way of
      switching (PeftModel.load_state_dict -> repack -> a new engine, captured again, + one step).

    python tools/bench_multi_adapter.py [--steps 200] [--repeats 3]

The two engines of (a) are timed alternately, `repeats` runs of `steps` graph replays each (device synchronisation around the host
clock); min / median / max per variant.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_inputs  # noqa: E402

NAMES = ["boom_bap", "trap", "lofi", "drill"]


def build(n_adapters, seed=1234):
    from audioldm_with_lora_amd.lora import LoraConfig, get_peft_model
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    torch.manual_seed(seed)
    unet = UNet2DConditionModel()
    cfg = LoraConfig(r=2, lora_alpha=2, target_modules=["to_q", "to_v"], init_lora_weights="gaussian")
    names = NAMES[:n_adapters] if n_adapters > 1 else ["default"]
    peft = get_peft_model(unet, cfg, adapter_name=names[0])
    for n in names[1:]:
        peft.add_adapter(n, cfg)
    g = torch.Generator().manual_seed(4)
    for n, p in unet.named_parameters():
        if "lora_B" in n:
            p.data.copy_(torch.randn(p.shape, generator=g) * 0.02)
    unet.to("cuda")
    unet.invalidate_packed()
    return unet, peft


def engine_for(unet, steps, lat, pe, ne, routing=None):
    from audioldm_with_lora_amd.engine import DenoiseEngine
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    eng = DenoiseEngine(unet, DDIMScheduler(), lat.shape[0], lat.shape[2], lat.shape[3], steps, 2.5)
    if routing is not None:
        eng.set_adapters(routing)
    eng.set_condition(pe, ne)
    eng.set_latents(lat)
    eng.capture()
    return eng


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    lat, pe, ne = synth_inputs(4, 250, 16)
    single, single_peft = build(1)
    multi, _ = build(4)
    e_single = engine_for(single, args.steps, lat, pe, ne)
    e_multi = engine_for(multi, args.steps, lat, pe, ne, NAMES)
    assert not e_single.gated and e_multi.gated
    per_step = {"ungated_single_adapter": [], "gated_4_adapters": []}
    for eng in (e_single, e_multi):                                     # warm-up
        eng.set_latents(lat)
        eng.run()
    for _ in range(args.repeats):                                       # alternate the variants
        for key, eng in (("ungated_single_adapter", e_single), ("gated_4_adapters", e_multi)):
            eng.set_latents(lat)
            per_step[key].append(wall_ms(eng.run) / args.steps)
    assert bool(torch.isfinite(e_multi.x).all()) and bool(torch.isfinite(e_single.x).all())

    # (b) switching
    other = [NAMES[1], "__base__", {NAMES[0]: 0.5, NAMES[2]: 0.5}, NAMES[3]]
    sw_gate, sw_reload = [], []
    sd = {k: v.clone() for k, v in single_peft.state_dict().items() if "lora_" in k}
    for i in range(args.repeats):
        routing = other if i % 2 == 0 else NAMES

        def switch_gate():
            e_multi.set_adapters(routing)
            e_multi.step()

        sw_gate.append(wall_ms(switch_gate))
        assert not e_multi.stale()

        def switch_reload():
            single_peft.load_state_dict(sd, strict=False)               # -> invalidate_packed: repack + a new capture
            eng = engine_for(single, args.steps, lat, pe, ne)
            eng.step()

        sw_reload.append(wall_ms(switch_reload))
    print(json.dumps({"what": "multi-adapter routing at config 2 (4 x 10 s, CFG 2.5, r = 2 to_q / to_v adapters, random-init weights)",
                      "steps": args.steps, "repeats": args.repeats,
                      "ms_per_step": {k: dict(stats(v), runs=[round(x, 4) for x in v]) for k, v in per_step.items()},
                      "switch_ms": {"set_adapters_plus_one_step": stats(sw_gate), "load_state_dict_recapture_plus_one_step": stats(sw_reload)}}))


if __name__ == "__main__":
    main()
