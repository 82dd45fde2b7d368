"""CLAP score + KAD of a folder of generated clips against a folder of reference clips -- what the reference's
script/inference/inference.py sets out to do (the shipped file does not parse).

Reads every *.wav of --gen-dir / --ref-dir with scipy.io.wavfile (the 16 kHz float32 files script/inference.py writes;
int PCM is scaled to [-1, 1], stereo is mono-mixed; a file at another rate is brought to 16 kHz on the device, resample.py --
what the reference's librosa.load(sr=16000) does, with this library's filter), embeds them with the CLAP model of --clap-dir on the HIP kernels, and
prints one JSON line: the CLAP score of every generated file against --prompt, their mean, and KAD in the inference.py
variant (bandwidth 1, no scale).  Clips must be at most 10 s long.
--normalize-loudness LUFS brings every clip of BOTH folders to that ITU-R BS.1770 integrated loudness first (loudness.py; on the
device, after the resampling to 16 kHz and before the CLAP front end; the gain is not capped -- float clips may pass full scale), so
that two folders recorded or generated at different levels are compared like with like; the report then carries the loudness each
folder was measured at ("loudness": mean, spread and range in LUFS over the clips that have one).

    python -m audioldm_with_lora_amd.script.evaluate --clap-dir clap-htsat-fused --gen-dir out/gen --ref-dir data/ref \
        --prompt "a calm piano melody"
"""
import argparse
import json
import os

import numpy as np


def load_wav(path):
    """(rate, mono fp32 samples) of a wav file"""
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if np.issubdtype(x.dtype, np.integer):
        x = x.astype(np.float32) / float(np.iinfo(x.dtype).max + 1)
    x = np.asarray(x, dtype=np.float32)
    return int(sr), (x.mean(axis=1) if x.ndim == 2 else x)


def to_16k(rate, x, device="cuda"):
    """a clip at 16 kHz: itself (the host array, untouched), or resampled on the device (a GPU tensor)"""
    if rate == 16000:
        return x
    import torch
    from ..resample import resample
    return resample(torch.from_numpy(np.ascontiguousarray(x)).to(device), rate, 16000)


def load_dir(d):
    names = sorted(f for f in os.listdir(d) if f.lower().endswith(".wav"))
    if len(names) < 2:
        raise ValueError(f"{d}: KAD needs at least two .wav files, found {len(names)}")
    return names, [to_16k(*load_wav(os.path.join(d, n))) for n in names]


def normalize_clips(clips, target_lufs, device="cuda"):
    """every 16 kHz clip (host array or GPU tensor) at target_lufs, as GPU tensors, and what the folder measured before:
    {"mean", "std", "min", "max"} in LUFS over the clips with a loudness, "n_unmeasured" (shorter than 400 ms, or silent: left as is)"""
    import torch
    from ..loudness import meter
    m = meter(16000, torch.device(device))
    out, lufs = [], []
    for x in clips:
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        y, info = m.normalize(x.to(m.device, torch.float32), target_lufs, None)
        out.append(y)
        lufs.append(info["lufs_in"])
    lufs = torch.cat(lufs).cpu().numpy()
    ok = lufs[np.isfinite(lufs)]
    stats = {"n_unmeasured": int(lufs.size - ok.size)}
    if ok.size:
        stats.update(mean=float(ok.mean()), std=float(ok.std()), min=float(ok.min()), max=float(ok.max()))
    return out, stats


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clap-dir", required=True, help="local laion/clap-htsat-* directory (config.json, model.safetensors)")
    ap.add_argument("--gen-dir", required=True)
    ap.add_argument("--ref-dir", required=True)
    ap.add_argument("--prompt", required=True, help="text, or comma-separated token ids when the directory has no tokenizer")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--normalize-loudness", type=float, default=None, metavar="LUFS",
                    help="bring both folders to this ITU-R BS.1770 integrated loudness before they are embedded (e.g. -23)")
    args = ap.parse_args(argv)
    if args.normalize_loudness is not None and not np.isfinite(args.normalize_loudness):
        ap.error("--normalize-loudness expects a finite level in LUFS")
    import torch
    from ..clap_audio import ClapModel
    from ..metrics import embed_audio, embed_text, kernel_audio_distance
    clap = ClapModel.from_pretrained(args.clap_dir).to("cuda")
    gen_names, gen = load_dir(args.gen_dir)
    _, ref = load_dir(args.ref_dir)
    loud = None
    if args.normalize_loudness is not None:
        gen, loud_gen = normalize_clips(gen, args.normalize_loudness)
        ref, loud_ref = normalize_clips(ref, args.normalize_loudness)
        loud = {"target_lufs": args.normalize_loudness, "gen": loud_gen, "ref": loud_ref}
    text = args.prompt
    if clap.tokenizer is None:
        text = torch.tensor([int(t) for t in args.prompt.split(",")])
    g = embed_audio(gen, clap, batch=args.batch)
    r = embed_audio(ref, clap, batch=args.batch)
    t = embed_text(text, clap)
    scores = (g @ t[0] + 1.0) / 2.0
    res = {"clap_score": {n: float(s) for n, s in zip(gen_names, scores)}, "clap_score_mean": float(scores.mean()),
           "kad": kernel_audio_distance(g, r, bandwidth=1.0), "n_gen": len(gen), "n_ref": len(ref)}
    if loud is not None:
        res["loudness"] = loud
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
