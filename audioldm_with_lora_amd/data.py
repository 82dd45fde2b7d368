"""Training from recordings: the reference's HfAudioDataset + DataLoader with the per-clip work on the MI355X.

The reference's dataset [REF script/data/datasets.py:494-522 read_hf_audio] cuts a random, non-silent 10.24 s segment out of each
recording, resamples it to 16 kHz, removes the mean, normalises the peak to 0.5, zero-pads to 163 840 samples and computes the
log-mel, in four CPU dataloader workers.  Here the recordings are decoded ONCE and stay resident on the device (one pool per sampling
rate); a batch is then four stages of HIP kernels:

    ops.clip_segment  ->  ops.resample_poly (skipped at 16 kHz)  ->  ops.clip_normalize  ->  LogMelFrontEnd

    ds = AudioFolder("clips/", tokenizer)                     # or HfAudioDataset(rows, tokenizer)
    fe = ClipFrontEnd("cuda", duration=10.24, seed=1)
    for batch in ClipLoader(ds, fe, batch_size=2, seed=1):    # the reference's collate_fn batch
        loss = trainer.step_from_batch(vae, text_encoder, batch, None, None, None)

Randomness: one draw of the front end's own Philox stream per batch, ten words per row (csrc/philox.h), so a resumed run
(state_dict / load_state_dict of the front end and the loader) cuts the segments the uninterrupted run would have cut.
"""
import csv
import json
import os

import numpy as np
import torch

from . import _lib, ops
from . import resample as R
from .mel import DSP, LogMelFrontEnd
from .training import noise_ordinal_base

MIN_SAMPLES = 100                  # the reference asserts `waveform_length > 100` [REF script/data/datasets.py:181]
MAX_TOKENS = 512                   # tokenizer(..., padding="max_length", truncation=True, max_length=512) [REF datasets.py:128-134]
STREAM_KEY = 0x636C69705F707265    # the segment stream's key is seed ^ this: never the key of the trainer's noise stream


class ByteTokenizer:
    """A small deterministic stand-in for the RoBERTa tokenizer where no model directory is at hand (train.py --tiny): the UTF-8 bytes
    of the caption as ids byte + 3 between <s> = 0 and </s> = 2, padded with 1 -- RoBERTa's special ids, 259 ids in all."""
    vocab_size = 259
    model_max_length = MAX_TOKENS

    def __call__(self, text, padding="max_length", truncation=True, max_length=MAX_TOKENS, return_tensors="pt"):
        body = [b + 3 for b in str(text).encode("utf-8")][:max_length - 2]
        ids = [0] + body + [2]
        n = len(ids)
        ids = ids + [1] * (max_length - n)
        mask = [1] * n + [0] * (max_length - n)
        return {"input_ids": torch.tensor([ids], dtype=torch.long), "attention_mask": torch.tensor([mask], dtype=torch.long)}


def _is_pool_form(wavs):
    return (isinstance(wavs, tuple) and len(wavs) == 3 and torch.is_tensor(wavs[0])
            and not (torch.is_tensor(wavs[1]) and wavs[1].is_floating_point()))


def _int_list(v):
    return [int(i) for i in (v.tolist() if hasattr(v, "tolist") else v)]


class ClipFrontEnd:
    """Recordings -> {"waveform" [B, 1, target], "log_mel_spec" [B, 1, target_length, n_mel], "random_start" int32 [B]}, all on the
    device.  duration: seconds per clip (target = int(16000 duration) samples, target_length = int(duration 16000 / hop) frames).
    seed, rank: the Philox stream of the segment starts -- key seed ^ STREAM_KEY, first draw training.noise_ordinal_base(rank).
    **dsp: overrides of mel.DSP."""

    def __init__(self, device="cuda", duration=10.24, seed=0, rank=0, **dsp):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AldmError("ClipFrontEnd runs on the MI355X only (got a CPU device); there is no CPU fallback")
        d = dict(DSP)
        d.update(dsp)
        self.duration = float(duration)
        self.sampling_rate = int(d["sampling_rate"])
        self.target = int(self.sampling_rate * self.duration)
        if self.target <= 0:
            raise ValueError(f"duration {duration!r} gives no samples")
        if "target_length" not in dsp:
            d["target_length"] = int(self.duration * self.sampling_rate / d["hop_length"])
        self.log_mel = LogMelFrontEnd(self.device, **d)
        self.seed, self.rank = int(seed), int(rank)
        self.state = ops.philox_state(self.seed ^ STREAM_KEY, noise_ordinal_base(self.rank), self.device)

    def segment_length(self, rate):
        """S: the segment's length in input samples, `int(sr * self.duration)` [REF script/data/datasets.py:499-501]"""
        return int(R._rate(rate) * self.duration)

    def __call__(self, wavs, rates, ordinals=None, advance=True):
        """wavs: a list of 1-D fp32 device tensors, or a tuple (pool fp32 1-D on the device, offsets [B], lens [B]).  rates: one rate,
        or one per row.  ordinals: each row's index in the logical batch (default: its index here).  A row's result depends on its
        samples, its rate and its ordinal alone, so a logical batch may be cut into several calls in any order: every call but the
        last passes advance=False (one batch, one draw)."""
        if _is_pool_form(wavs):
            pool, offsets, lens = wavs[0], _int_list(wavs[1]), _int_list(wavs[2])
        else:
            wavs = list(wavs)
            if not wavs or any(not torch.is_tensor(w) or w.dim() != 1 for w in wavs):
                raise ValueError("ClipFrontEnd: a non-empty list of 1-D tensors, or (pool, offsets, lens), is expected")
            for w in wavs:
                ops._require_gpu(w)
            lens = [int(w.numel()) for w in wavs]
            offsets = [0] + list(np.cumsum(lens[:-1], dtype=np.int64))
            pool = torch.cat([w.to(torch.float32) for w in wavs]) if len(wavs) > 1 else wavs[0].to(torch.float32).contiguous()
        B = len(lens)
        rates = [R._rate(rates)] * B if np.ndim(rates) == 0 else [R._rate(r) for r in rates]
        ordinals = list(range(B)) if ordinals is None else _int_list(ordinals)
        if not (len(offsets) == len(rates) == len(ordinals) == B and B > 0):
            raise ValueError("ClipFrontEnd: offsets, lens, rates and ordinals must hold one entry per row")
        groups = {}
        for i, r in enumerate(rates):
            groups.setdefault(r, []).append(i)
        return self.run_groups([dict(rate=r, pool=pool, offsets=[offsets[i] for i in rows], lens=[lens[i] for i in rows],
                                     ordinals=[ordinals[i] for i in rows], rows=rows) for r, rows in sorted(groups.items())], B, advance)

    def run_groups(self, groups, B, advance=True):
        """One logical batch of B rows as groups of one sampling rate each: dicts {rate, pool, offsets, lens, ordinals, rows} (host
        lists; rows: where each result goes in the batch).  All groups read the same draw; the last one moves the stream on."""
        for g in groups:
            short = [n for n in g["lens"] if n <= MIN_SAMPLES]
            if short:
                raise ValueError(f"Waveform is too short, {short[0]} (a recording needs more than {MIN_SAMPLES} samples)")
        whole = len(groups) == 1 and list(groups[0]["rows"]) == list(range(B))
        waveform = start = None
        if not whole:
            waveform = torch.empty(B, self.target, dtype=torch.float32, device=self.device)
            start = torch.empty(B, dtype=torch.int32, device=self.device)
        for gi, g in enumerate(groups):
            rate, S = g["rate"], self.segment_length(g["rate"])
            seg, st = ops.clip_segment(g["pool"], g["offsets"], g["lens"], g["ordinals"], S, self.state, max_len=max(g["lens"]),
                                       advance=advance and gi == len(groups) - 1)
            n = [min(L, S) for L in g["lens"]]                       # known on the host: nothing is read back
            up, down = R.ratio(rate, self.sampling_rate)
            if up != down:
                seg, n = ops.resample_poly(seg, up, down, lens=n, table=R.device_table(up, down, self.device))
            out = ops.clip_normalize(seg, n, self.target)
            if whole:
                waveform, start = out, st
            else:
                rows = ops._h2d(torch.tensor(g["rows"], dtype=torch.long), self.device)
                waveform[rows] = out
                start[rows] = st
        return {"waveform": waveform[:, None, :], "log_mel_spec": self.log_mel(waveform), "random_start": start}

    def state_dict(self):
        seed, ordinal = ops.philox_state_values(self.state)
        return {"seed": self.seed, "key": seed, "ordinal": ordinal, "rank": self.rank}

    def load_state_dict(self, sd):
        """the saving rank's position within its lane of the counter space, moved to this rank's lane (as LoraTrainer does)"""
        self.seed = int(sd["seed"])
        ordinal = int(sd["ordinal"]) - noise_ordinal_base(sd.get("rank", 0)) + noise_ordinal_base(self.rank)
        ops.philox_set(self.state, seed=self.seed ^ STREAM_KEY, draw=ordinal)


# ---- datasets -------------------------------------------------------------------------------------------------------------------
def to_mono_f32(array):
    """Whatever a decoder hands over -> fp32 [T] in [-1, 1): PCM 8 (unsigned) / 16 / 32 (scipy returns 24-bit files left-justified in
    int32) scaled by their full range, floats as they are; [T, channels] mixed down by the channel mean."""
    a = np.asarray(array)
    if a.dtype == np.uint8:
        a = (a.astype(np.float32) - 128.0) / 128.0
    elif a.dtype == np.int16:
        a = a.astype(np.float32) / 32768.0
    elif a.dtype == np.int32:
        a = (a.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif a.dtype.kind == "f":
        a = a.astype(np.float32)
    else:
        raise ValueError(f"unsupported sample type {a.dtype}")
    if a.ndim == 2:
        a = a.mean(axis=1, dtype=np.float32)
    if a.ndim != 1:
        raise ValueError(f"a recording must be [T] or [T, channels], got {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32)


class _ResidentAudio:
    """Recordings decoded once and kept on `device`, one pool per sampling rate; captions tokenised once.  Item i:
    rates[i], offsets[i] / lens[i] into pools[rates[i]], captions[i], input_ids[i] / attention_mask[i] ([1, 512] each)."""

    def __init__(self, items, tokenizer, device="cuda"):
        self.device = torch.device(device)
        self.rates, self.offsets, self.lens, self.captions = [], [], [], []
        parts, ids, masks = {}, [], []
        for array, rate, caption in items:
            wav, rate = to_mono_f32(array), R._rate(rate)
            filled = parts.setdefault(rate, [0, []])
            self.rates.append(rate)
            self.offsets.append(filled[0])
            self.lens.append(int(wav.shape[0]))
            filled[0] += int(wav.shape[0])
            filled[1].append(wav)
            caption = "" if caption is None else str(caption)
            self.captions.append(caption)
            enc = tokenizer(caption, padding="max_length", truncation=True, max_length=MAX_TOKENS, return_tensors="pt")
            ids.append(torch.as_tensor(enc["input_ids"]).reshape(1, MAX_TOKENS).long())
            masks.append(torch.as_tensor(enc["attention_mask"]).reshape(1, MAX_TOKENS).long())
        if not self.rates:
            raise ValueError("the dataset holds no recordings")
        self.pools = {r: torch.from_numpy(np.concatenate(p[1])).to(self.device) for r, p in parts.items()}
        self.input_ids, self.attention_mask = torch.stack(ids), torch.stack(masks)          # [N, 1, 512], on the host

    def __len__(self):
        return len(self.rates)

    def __getitem__(self, i):
        o, n, r = self.offsets[i], self.lens[i], self.rates[i]
        return {"audio": {"array": self.pools[r][o:o + n], "sampling_rate": r}, "caption": self.captions[i],
                "input_ids": self.input_ids[i], "attention_mask": self.attention_mask[i]}


class HfAudioDataset(_ResidentAudio):
    """Any iterable of {"audio": {"array", "sampling_rate"}, "caption"} rows -- what the reference's dataset takes from a Hugging Face
    audio dataset [REF script/data/datasets.py:96-106]; a missing caption is ""."""

    def __init__(self, rows, tokenizer, device="cuda"):
        super().__init__(((r["audio"]["array"], r["audio"]["sampling_rate"], r.get("caption", "")) for r in rows), tokenizer, device)


def read_metadata(root):
    """[(file_name, caption)] of a Hugging Face audiofolder: metadata.jsonl (one object per line) or metadata.csv"""
    jl, cs = os.path.join(root, "metadata.jsonl"), os.path.join(root, "metadata.csv")
    rows = []
    if os.path.isfile(jl):
        with open(jl, encoding="utf-8") as f:
            rows = [json.loads(line) for line in f if line.strip()]
    elif os.path.isfile(cs):
        with open(cs, encoding="utf-8", newline="") as f:
            rows = list(csv.DictReader(f))
    else:
        raise FileNotFoundError(f"{root} holds neither metadata.jsonl nor metadata.csv")
    if any("file_name" not in r for r in rows):
        raise ValueError("every metadata row needs a file_name")
    return [(r["file_name"], r.get("caption") or "") for r in rows]


class AudioFolder(_ResidentAudio):
    """A folder in the Hugging Face audiofolder layout: wav files and a metadata.jsonl / metadata.csv with `file_name` and `caption`."""

    def __init__(self, root, tokenizer, device="cuda"):
        from scipy.io import wavfile
        self.root = root
        self.files = []

        def items():
            for name, caption in read_metadata(root):
                rate, data = wavfile.read(os.path.join(root, name))
                self.files.append(name)
                yield data, rate, caption

        super().__init__(items(), tokenizer, device)


# ---- loader ---------------------------------------------------------------------------------------------------------------------
class ClipLoader:
    """Batches of the reference's collate_fn [REF script/train/train_audioldm_lora.py:415-420]: {"log_mel_spec" [B, 1, frames, n_mel]
    on the device, "input_ids" / "attention_mask" [B, 1, 512] on the host}.  A seeded permutation per epoch; rank r of `world` takes
    its entries r::world.  (epoch, cursor) is the position: cursor counts this rank's clips already served in the epoch."""

    def __init__(self, dataset, front_end, batch_size, seed=0, rank=0, world=1):
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"ClipLoader: bad batch_size / rank / world ({batch_size}, {rank}, {world})")
        self.dataset, self.front_end = dataset, front_end
        self.batch_size, self.seed, self.rank, self.world = int(batch_size), int(seed), int(rank), int(world)
        self.epoch, self.cursor = 0, 0
        self.last = None                                             # the front end's whole output for the last batch
        if not self.indices(0):
            raise ValueError(f"ClipLoader: rank {rank} of {world} gets no clip out of {len(dataset)}")

    def permutation(self, epoch):
        return np.random.default_rng([self.seed, int(epoch)]).permutation(len(self.dataset)).tolist()

    def indices(self, epoch):
        """this rank's clips of an epoch, in order"""
        return self.permutation(epoch)[self.rank::self.world]

    def __len__(self):
        """batches per epoch (the last one may be short)"""
        return -(-len(self.indices(0)) // self.batch_size)

    def next_indices(self):
        """the next batch's dataset indices; moves (epoch, cursor), wrapping into the next epoch at the end"""
        idx = self.indices(self.epoch)
        if self.cursor >= len(idx):
            self.epoch, self.cursor = self.epoch + 1, 0
            idx = self.indices(self.epoch)
        take = idx[self.cursor:self.cursor + self.batch_size]
        self.cursor += len(take)
        return take

    def collate(self, take):
        ds = self.dataset
        by_rate = {}
        for row, i in enumerate(take):
            by_rate.setdefault(ds.rates[i], []).append((row, i))
        groups = [dict(rate=r, pool=ds.pools[r], offsets=[ds.offsets[i] for _, i in m], lens=[ds.lens[i] for _, i in m],
                       ordinals=[row for row, _ in m], rows=[row for row, _ in m]) for r, m in sorted(by_rate.items())]
        self.last = self.front_end.run_groups(groups, len(take))
        sel = torch.tensor(take, dtype=torch.long)
        return {"log_mel_spec": self.last["log_mel_spec"], "input_ids": ds.input_ids[sel], "attention_mask": ds.attention_mask[sel]}

    def next_batch(self):
        return self.collate(self.next_indices())

    def __iter__(self):
        """the rest of the current epoch (all of it from cursor 0); the next iteration is the next epoch"""
        n = len(self.indices(self.epoch))
        while self.cursor < n:
            yield self.next_batch()
        self.epoch, self.cursor = self.epoch + 1, 0

    def state_dict(self):
        return {"epoch": self.epoch, "cursor": self.cursor, "seed": self.seed}

    def load_state_dict(self, sd):
        self.epoch, self.cursor = int(sd["epoch"]), int(sd["cursor"])
        self.seed = int(sd.get("seed", self.seed))
