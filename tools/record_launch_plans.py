"""Record how ops.conv() launches every convolution / linear of the shipped workloads: the regression fixture of the launch planner.

    python tools/record_launch_plans.py OUT.json [tiny|full|all] [--no-vocoder-full]

Per conv() call one record: what the caller asked for (`in`: shapes, scalar keyword values, which tensor arguments are present, the weight
pack's N / Kpad / Cin / Cext / Rp / geglu / ln), the route (igemm | pgemm), the tuning-table key where ops.KEYLOG gives one,
aldm_igemm_epilogue_form, every non-pointer field of the argument struct as the library received it and, for every pointer field, whether
it was null; from the call's result, the shape of the GroupNorm / LayerNorm hand-over tables where the result shows them.  Records are
de-duplicated: `records` holds the distinct ones, `workloads[name]` the launch order as indices into it.  The script prints one JSON
line: launches per workload and the wall time of each recorded (second) pass.

Only public surface is hooked (ops.conv is wrapped; the handle _lib.load() returns is replaced by a proxy that reads the struct of
aldm_igemm / aldm_pgemm before it forwards the call), so the same file records any commit.  The tuned-table switch (ALDM_NO_TUNED) is read
when the package is imported: one process per mode, then

    python tools/record_launch_plans.py --merge TUNED.json NO_TUNED.json tests/golden/igemm_launch_plans.json.gz

writes the committed form (pack_fixture: one record list for both modes, struct values as lists in the order of `fields`, as gzipped
JSON -- 0.6 MB of recorded numbers is nothing to read in a diff; load_fixture gives the two runs back).  To compare a commit with the fixture, record it the same way, then per mode

    python tools/record_launch_plans.py --diff tests/golden/igemm_launch_plans.json.gz tuned|no_tuned RUN.json

--kernels (recording) also traces the recorded pass of every workload (kineto, as bench.trace_steps) and keeps, per distinct igemm record,
what the GPU really ran: `kernel` = {"name": demangled kernel name, "grid", "block", "lds" where the tracer reports them}.  Every
aldm_igemm call dispatches exactly one igemm_* kernel besides igemm_reduce_kernel, so launch order pairs the trace with the calls.

    python tools/record_launch_plans.py --merge-kernels TUNED.json NO_TUNED.json tests/golden/igemm_launch_plans.json.gz \
        tests/golden/igemm_kernel_variants.json.gz

writes the committed form: one entry per record of the launch-plan fixture (null for pgemm records), names as indices into `names`.
--diff with that file as a fifth argument also compares the kernels of RUN.json (recorded with --kernels) with it."""
import ctypes as C
import gzip
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audioldm_with_lora_amd import _lib, ops  # noqa: E402

SCALARS = ("stride", "pad", "dil", "up_size", "in_dilate", "out_hw", "in_act", "out_act", "post_act", "alpha", "out_f32", "out_ld",
           "out_batch_stride", "out_pix_stride", "out_pix_offset", "vt_col0", "vt_dual", "splits", "tile", "ring", "gn_keep", "rowstats",
           "qstats", "epi")
TENSORS = ("x2", "x3", "x4", "rowbias", "res", "res2", "out2", "out", "vt", "lora_t_out", "ln_parts", "lora_gate")


def _plain(v):
    return list(v) if isinstance(v, tuple) else v


def describe_call(x, pw, kw):
    """what conv() was asked: JSON-able, no tensors"""
    d = {"x": list(x.shape), "pw": {"N": pw.N, "Kpad": pw.Kpad, "Cin": pw.Cin, "Cext": pw.Cext, "Rp": pw.Rp, "KH": pw.KH, "KW": pw.KW,
                                    "geglu": bool(pw.geglu), "ln": pw.ln_s is not None, "ranks_used": getattr(pw, "ranks_used", None)}}
    for k in SCALARS:
        if k in kw and kw[k] is not None:
            d[k] = _plain(kw[k])
    for k in TENSORS:
        t = kw.get(k)
        if t is not None:
            d[k] = {"shape": list(t.shape), "f32": t.dtype == torch.float32, "contig": t.is_contiguous()}
    if kw.get("gn") is not None:
        d["gn_groups"] = kw["gn"][2]
    if kw.get("defer"):
        d["defer"] = _plain(kw["defer"])
    if kw.get("gn_in") is not None:
        d["gn_in"] = True
    if kw.get("lora_gate") is None and ops.LORA_GATE is not None and pw.Rp:
        d["lora_gate"] = {"shape": list(ops.LORA_GATE.shape), "f32": True, "contig": True}
    return d


def describe_struct(a):
    vals, nonnull = {}, []
    for name, typ in a._fields_:
        v = getattr(a, name)
        if typ is C.c_void_p:
            if v:
                nonnull.append(name)
        else:
            vals[name] = v
    return vals, nonnull


class Recorder:
    def __init__(self):
        self.records, self.index, self.order, self.cur = [], {}, [], None
        self.calls = []                                                  # per aldm_igemm call: position in self.order of the conv() that made it, or None
        self.real = _lib.load()
        self.conv = ops.conv

    # the library handle: reads the struct of the two GEMM entry points, forwards everything
    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in ("aldm_igemm", "aldm_pgemm"):
            return fn

        def launch(ref, stream):
            a = ref._obj
            if name == "aldm_igemm":
                self.calls.append(len(self.order) if self.cur is not None else None)
            if self.cur is not None:
                vals, nonnull = describe_struct(a)
                self.cur.update(route=name[5:], args=vals, nonnull=nonnull,
                                epi=self.real.aldm_igemm_epilogue_form(ref) if name == "aldm_igemm" else None)
            return fn(ref, stream)
        return launch

    def wrapped_conv(self, x, pw, **kw):
        self.cur = {"in": describe_call(x, pw, kw), "route": None, "key": None}
        ops.PROFILE, ops.KEYLOG = [], []
        try:
            y = self.conv(x, pw, **kw)
            # the statistics tables the launch left behind, as its result shows them (QStats on the output tensor; (out, stats) of rowstats=)
            outs = [ops.tensor_of(t) for t in (y if isinstance(y, tuple) else (y,))]
            q = next((t.qstats for t in outs if getattr(t, "qstats", None) is not None), None)
            self.cur["qstats"] = None if q is None else [q.table.shape[0], q.bm, q.tpi]
            self.cur["rowstats_cols"] = outs[1].shape[1] if kw.get("rowstats") else None
        finally:
            rec, self.cur = self.cur, None
            if ops.KEYLOG:
                rec["key"] = ops.KEYLOG[0][1][0]
            ops.PROFILE = ops.KEYLOG = None
        s = json.dumps(rec, sort_keys=True)
        if s not in self.index:
            self.index[s] = len(self.records)
            self.records.append(rec)
        self.order.append(self.index[s])
        return y

    def __enter__(self):
        self.load = _lib.load
        _lib.load = lambda: self
        ops.conv = self.wrapped_conv
        return self

    def __exit__(self, *exc):
        _lib.load, ops.conv = self.load, self.conv
        return False

    def take(self):
        order, self.order, self.calls = self.order, [], []
        return order


# ---- the workloads ---------------------------------------------------------------------------------------------------------------
def _unet(tiny, rank, adapters=None):
    from audioldm_with_lora_amd import configs
    from audioldm_with_lora_amd.lora import LoraConfig, get_peft_model
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    torch.manual_seed(1234)
    unet = UNet2DConditionModel(**(configs.tiny_unet() if tiny else {}))
    if adapters is None:
        get_peft_model(unet, LoraConfig(r=rank, lora_alpha=rank, target_modules=["to_q", "to_k", "to_v", "to_out.0"], init_lora_weights="gaussian"))
    else:
        cfg = LoraConfig(r=2, lora_alpha=2, target_modules=["to_q", "to_v"], init_lora_weights="gaussian")
        peft = get_peft_model(unet, cfg, adapter_name=adapters[0])
        for n in adapters[1:]:
            peft.add_adapter(n, cfg)
    g = torch.Generator().manual_seed(4)
    for n, p in unet.named_parameters():
        if "lora_B" in n:
            p.data.copy_(torch.randn(p.shape, generator=g) * 0.02)
    unet.cuda()
    if adapters is not None:
        unet.invalidate_packed()
    return unet


def _engine(unet, batch, H, W, routing=None):
    from audioldm_with_lora_amd.engine import DenoiseEngine
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    ce = unet.cfg["class_embed_input_dim"]
    g = torch.Generator().manual_seed(0)
    eng = DenoiseEngine(unet, DDIMScheduler(), batch, H, W, 20, 2.5, use_graph=False)
    if routing is not None:
        eng.set_adapters(routing)
    eng.set_condition(torch.nn.functional.normalize(torch.randn(batch, ce, generator=g), dim=-1),
                      torch.nn.functional.normalize(torch.randn(batch, ce, generator=g), dim=-1))
    eng.set_latents(torch.randn(batch, 8, H, W, generator=g))
    return eng


def workloads(tiny, vocoder=True):
    """(name, callable) pairs; every callable makes its launches eagerly on the current stream"""
    from audioldm_with_lora_amd import configs
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from audioldm_with_lora_amd.training import LoraTrainer
    from audioldm_with_lora_amd.vae import AutoencoderKL
    from audioldm_with_lora_amd.vocoder import SpeechT5HifiGan
    pre = "tiny_" if tiny else "full_"
    H, W = (16, 16) if tiny else (250, 16)
    unet = _unet(tiny, 4)
    for cfg, batch in ((1, 1), (2, 4)):                                  # BASELINE.json config 1: one prompt; config 2: four
        yield f"{pre}unet_config{cfg}", _engine(unet, batch, H, W)._one_step
    del unet
    names = ["boom_bap", "trap", "lofi", "drill"]
    yield pre + "unet_gated", _engine(_unet(tiny, 2, names), 4, H, W, names)._one_step
    torch.manual_seed(0)
    vae = AutoencoderKL(**(configs.tiny_vae() if tiny else {})).cuda()
    gd = torch.Generator(device="cuda").manual_seed(1)
    mel = torch.randn(1, 4 * H if tiny else 1024, 64, 1, device="cuda", generator=gd).to(torch.bfloat16)
    z = torch.randn(1 if tiny else 4, H, W, 8, device="cuda", generator=gd).to(torch.bfloat16)
    yield pre + "vae_encode", lambda: vae.encode_nhwc(mel)
    yield pre + "vae_decode", lambda: vae.decode_nhwc(z)
    if tiny or vocoder:
        voc = SpeechT5HifiGan(**(configs.tiny_vocoder() if tiny else {})).cuda()
        m = torch.randn(1 if tiny else 4, 1, 4 * H, 64, device="cuda", generator=gd).to(torch.bfloat16)
        yield pre + "vocoder", lambda: voc.forward_nhwc(m)
    rank, batch, TH = (4, 2, 16) if tiny else (8, 8, 256)
    unet = _unet(tiny, rank)
    tr = LoraTrainer(unet, DDIMScheduler(), lr=1e-5, weight_decay=1e-5, max_train_steps=1000, use_graph=False)
    g = torch.Generator().manual_seed(5)
    lat, noise = torch.randn(batch, 8, TH, 16, generator=g).cuda(), torch.randn(batch, 8, TH, 16, generator=g).cuda()
    t = torch.randint(0, 1000, (batch,), generator=g).cuda()
    emb = torch.nn.functional.normalize(torch.randn(batch, unet.cfg["class_embed_input_dim"], generator=g), dim=-1).cuda()
    yield pre + "train_step", lambda: tr.step(lat, noise, t, emb)


_TRACER_WARM = False


def traced_igemm_kernels(fn):
    """fn() under the kernel tracer: [{"name", "grid", "block", "lds"}] of its igemm_* kernels (the split-K reduce left out) in launch order"""
    import tempfile
    from torch.profiler import ProfilerActivity, profile
    global _TRACER_WARM
    if not _TRACER_WARM:                                                 # the first session of a process loses its first kernels
        with profile(activities=[ProfilerActivity.CUDA]):
            torch.zeros(64, device="cuda").sum().item()
        _TRACER_WARM = True
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as tmp:
        prof.export_chrome_trace(os.path.join(tmp, "trace.json"))
        with open(os.path.join(tmp, "trace.json")) as f:
            evs = [e for e in json.load(f)["traceEvents"] if e.get("cat") == "kernel"]
    evs.sort(key=lambda e: e["ts"])
    out = []
    for e in evs:
        if "igemm_" in e["name"] and "igemm_reduce_kernel" not in e["name"]:
            a = e.get("args", {})
            out.append({"name": e["name"], "grid": a.get("grid"), "block": a.get("block"), "lds": a.get("shared memory")})
    return out


def record(sizes=("tiny",), vocoder_full=True, timing=None, kernels=False):
    """{"records": [...], "workloads": {name: [index, ...]}} of the given sizes, recorded in this process; kernels: every igemm record
    also gets `kernel`, what the tracer saw its launch run"""
    out, seen = {}, {}
    with Recorder() as rec:
        def one_pass(name, fn):
            """fn() once: its launches as indices into rec.records; with `kernels`, under the tracer (the warm-up pass too: it makes
            launches no later pass repeats)"""
            if kernels:
                ran = traced_igemm_kernels(fn)
            else:
                fn()
                torch.cuda.synchronize()
            calls = rec.calls
            order = rec.take()
            if kernels:
                if len(ran) != len(calls):
                    raise RuntimeError(f"{name}: {len(calls)} aldm_igemm calls, {len(ran)} igemm kernels in the trace")
                for pos, k in zip(calls, ran):
                    if pos is not None and seen.setdefault(order[pos], k) != k:
                        raise RuntimeError(f"{name}: record {order[pos]} ran {k} and {seen[order[pos]]}")
            return order

        for size in sizes:
            gen = workloads(size == "tiny", vocoder_full)
            while True:
                made = []
                one_pass("set-up", lambda: made.append(next(gen, None)))    # building a workload launches too (an engine's conditioning)
                if made[0] is None:
                    break
                name, fn = made[0]
                with torch.no_grad() if "train" not in name else torch.enable_grad():
                    one_pass(name, fn)                                   # warm-up: packs the weights, sizes the workspace
                    t0 = time.perf_counter()
                    out[name] = one_pass(name, fn)
                if timing is not None:
                    timing[name] = round((time.perf_counter() - t0) * 1e3, 2)
                ops.drop_pending()
        run = {"records": rec.records, "workloads": out}
        if kernels:
            missing = [i for i, r in enumerate(rec.records) if r["route"] == "igemm" and i not in seen]
            if missing:
                raise RuntimeError(f"no kernel traced for igemm records {missing[:10]}")
            run["kernels"] = [seen.get(i) for i in range(len(rec.records))]
        return run


def pack_kernels(tuned, no_tuned, plans_path):
    """The committed form of the `kernels` of two runs: one entry [name index, grid, block, lds] per record of the launch-plan fixture"""
    with gzip.open(plans_path, "rt") as f:
        d = json.load(f)
    index = {json.dumps(r, sort_keys=True): i for i, r in enumerate(d["records"])}
    names, variants = [], [None] * len(d["records"])
    for run in (tuned, no_tuned):
        for r, k in zip(run["records"], run["kernels"]):
            i = index[json.dumps(dict(r, args=[r["args"][f] for f in d["fields"][r["route"]]]), sort_keys=True)]   # KeyError: not the fixture's runs
            if k is None:
                continue
            if k["name"] not in names:
                names.append(k["name"])
            v = [names.index(k["name"]), k["grid"], k["block"], k["lds"]]
            if variants[i] not in (None, v):
                raise RuntimeError(f"record {i}: {variants[i]} and {v}")
            variants[i] = v
    return {"names": names, "variants": variants}


def load_kernels(path, plans_path):
    """{json text of a launch-plan fixture record: {"name", "grid", "block", "lds"}} from the committed forms"""
    with gzip.open(path, "rt") as f:
        k = json.load(f)
    with gzip.open(plans_path, "rt") as f:
        d = json.load(f)
    return {json.dumps(r, sort_keys=True): dict(zip(("name", "grid", "block", "lds"), [k["names"][v[0]]] + v[1:]))
            for r, v in zip(d["records"], k["variants"]) if v is not None}, d["fields"]


def diff_kernels(path, plans_path, run):
    """number of igemm records of a run (recorded with --kernels) whose kernel differs from the committed one"""
    want, fields = load_kernels(path, plans_path)
    bad = 0
    for i, (r, k) in enumerate(zip(run["records"], run["kernels"])):
        if r["route"] != "igemm":
            continue
        w = want.get(json.dumps(dict(r, args=[r["args"][f] for f in fields["igemm"]]), sort_keys=True))
        if w != k:
            bad += 1
            if bad <= 10:
                print(f"record {i} ({r['key']}): recorded {w}, now {k}")
    return bad


def pack_fixture(tuned, no_tuned):
    """The committed form of two runs: one list of distinct records for both modes, the struct values as lists in the order of `fields`"""
    fields = {r["route"]: sorted(r["args"]) for run in (tuned, no_tuned) for r in run["records"]}
    records, index, modes = [], {}, {}
    for mode, run in (("tuned", tuned), ("no_tuned", no_tuned)):
        remap = []
        for r in run["records"]:
            c = dict(r, args=[r["args"][f] for f in fields[r["route"]]])
            s = json.dumps(c, sort_keys=True)
            if s not in index:
                index[s] = len(records)
                records.append(c)
            remap.append(index[s])
        modes[mode] = {name: [remap[i] for i in order] for name, order in run["workloads"].items()}
    return {"fields": fields, "records": records, **modes}


def load_fixture(path):
    """{"tuned": run, "no_tuned": run} as record() returns runs, from the committed form"""
    with gzip.open(path, "rt") as f:
        d = json.load(f)
    records = [dict(r, args=dict(zip(d["fields"][r["route"]], r["args"]))) for r in d["records"]]
    out = {}
    for mode in ("tuned", "no_tuned"):
        used = sorted({i for order in d[mode].values() for i in order})
        pos = {i: n for n, i in enumerate(used)}
        out[mode] = {"records": [records[i] for i in used], "workloads": {k: [pos[i] for i in v] for k, v in d[mode].items()}}
    return out


def launches(run, name):
    """the records of one workload of a run, in launch order"""
    return [run["records"][i] for i in run["workloads"][name]]


def diff(want, got):
    """number of workloads / launches at which two runs differ (the first few are printed)"""
    bad = 0
    for name in sorted(set(want["workloads"]) | set(got["workloads"])):
        if name not in want["workloads"] or name not in got["workloads"]:
            print("only in one run:", name)
            bad += 1
            continue
        w, g = launches(want, name), launches(got, name)
        if len(w) != len(g):
            print(f"{name}: {len(w)} launches recorded, {len(g)} now")
            bad += 1
        for i, (a, b) in enumerate(zip(w, g)):
            if a != b:
                bad += 1
                if bad <= 10:
                    print(f"{name} launch {i}:", {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
    return bad


def main():
    if sys.argv[1] == "--diff":                                          # --diff FIXTURE.json.gz tuned|no_tuned RUN.json
        with open(sys.argv[4]) as f:
            bad = diff(load_fixture(sys.argv[2])[sys.argv[3]], json.load(f))
            if len(sys.argv) > 5:
                f.seek(0)
                bad += diff_kernels(sys.argv[5], sys.argv[2], json.load(f))
        print(f"{sys.argv[4]} against {sys.argv[2]} [{sys.argv[3]}]: " + ("no difference" if not bad else f"{bad} differences"))
        sys.exit(1 if bad else 0)
    if sys.argv[1] == "--merge-kernels":                                 # --merge-kernels TUNED.json NO_TUNED.json PLANS.json.gz OUT.json.gz
        with open(sys.argv[2]) as f1, open(sys.argv[3]) as f2:
            text = json.dumps(pack_kernels(json.load(f1), json.load(f2), sys.argv[4]), separators=(",", ":"), sort_keys=True)
        with open(sys.argv[5], "wb") as fo, gzip.GzipFile(fileobj=fo, mode="wb", mtime=0) as gz:
            gz.write(text.encode())
        return
    if sys.argv[1] == "--merge":
        with open(sys.argv[2]) as f1, open(sys.argv[3]) as f2:
            text = json.dumps(pack_fixture(json.load(f1), json.load(f2)), separators=(",", ":"), sort_keys=True)
        with open(sys.argv[4], "wb") as fo, gzip.GzipFile(fileobj=fo, mode="wb", mtime=0) as gz:   # (mtime 0: same runs, same bytes)
            gz.write(text.encode())
        return
    which = sys.argv[2] if len(sys.argv) > 2 and not sys.argv[2].startswith("--") else "all"
    timing = {}
    run = record(("tiny", "full") if which == "all" else (which,), "--no-vocoder-full" not in sys.argv, timing, "--kernels" in sys.argv)
    with open(sys.argv[1], "w") as f:
        json.dump(run, f, separators=(",", ":"), sort_keys=True)
    print(json.dumps({"distinct": len(run["records"]), "launches": {k: len(v) for k, v in run["workloads"].items()},
                      "recorded_wall_ms": timing, "tuned": bool(ops.TUNED)}))


if __name__ == "__main__":
    main()
