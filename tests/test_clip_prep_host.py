"""Host side of training from recordings (data.py, csrc/clip_prep.hip's C-ABI): the restatement the GPU tests compare with, the
datasets on files written into tmp_path and on dict rows, the loader's sharding / permutations / resumption, the new symbols and
the driver's new flags."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import clip_prep_restatement as CR
import philox_restatement as PR
from audioldm_with_lora_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
def test_candidate_starts_lie_in_range_and_R_1_gives_0():
    for R in (1, 2, 1000, 44100 * 600, 2 ** 31 - 2049):
        for ordinal in (0, 1, 7, 63):
            starts = CR.candidate_starts(seed=5, draw=3, ordinal=ordinal, R=R)
            assert len(starts) == 10 and all(0 <= s < R for s in starts)
            if R == 1:
                assert starts == [0] * 10
    a, b = CR.candidate_starts(5, 3, 2, 10 ** 6), CR.candidate_starts(5, 4, 2, 10 ** 6)
    assert a != b and len(set(a)) > 1                                   # another draw, other starts
    w = PR.u32(5, 3, 30)
    assert a == [((int(v) >> 8) * 10 ** 6) >> 24 for v in w[20:30]]     # row 2 reads words 20 .. 29
    # the largest word gives the largest start, still below R: int(R * (1 - 2^-24))
    assert ((0xFFFFFFFF >> 8) * 1000) >> 24 == 999


def test_segment_rule_on_small_rows():
    S = 8
    x = np.zeros(5, dtype=np.float32)
    x[2] = 1.0
    start, seg = CR.segment(x, S, 1, 0, 0)
    assert start == 0 and seg.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    L = 200
    cands = CR.candidate_starts(1, 0, 3, L - S)
    quiet = np.full(L, 1e-4, dtype=np.float32)                          # exactly the threshold: silent everywhere
    assert CR.segment(quiet, S, 1, 0, 3)[0] == cands[9]
    loud = quiet.copy()
    loud[cands[0] + S - 1] = np.nextafter(np.float32(1e-4), np.float32(1))
    start, seg = CR.segment(loud, S, 1, 0, 3)
    assert start == cands[0] and np.array_equal(seg, loud[start:start + S])


def test_normalize_restatement_and_bound():
    x = (1000.0 + np.sin(np.arange(300))).astype(np.float32)
    ref = CR.normalize(x, 300, 320)
    assert ref.shape == (320,) and abs(np.abs(ref).max() - 0.5) < 1e-7 and not ref[300:].any() and abs(ref[:300].mean()) < 1e-9
    assert np.array_equal(CR.normalize(x, 400, 200), CR.normalize(x[:200], 200, 200))          # cropped at the target
    assert not CR.normalize(np.full(50, 0.25, dtype=np.float32), 50, 64).any()
    assert not CR.normalize(x, 0, 16).any()
    b = CR.normalize_bound(x)
    assert b.shape == (300,) and (b > 2.0 ** -24 * 1000).all() and (b < 2.0 ** -24 * 2010).all()     # the offset dominates
    # a plain fp32 evaluation with a correctly rounded mean stays inside it
    mean32 = np.float32(x.astype(np.float64).mean())
    d32 = x - mean32
    got = d32 / (np.abs(d32).max() + np.float32(1e-8)) * np.float32(0.5)
    assert got.dtype == np.float32 and (np.abs(got - ref[:300]) <= b).all()


# ---- datasets -------------------------------------------------------------------------------------------------------------------
def _tone(n, rate, f=330.0, amp=0.4):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / rate)).astype(np.float32)


def _write_folder(root, meta="jsonl"):
    os.makedirs(root, exist_ok=True)
    a = _tone(3000, 16000)
    wavfile.write(os.path.join(root, "a.wav"), 16000, np.round(a * 32767).astype(np.int16))            # PCM16
    wavfile.write(os.path.join(root, "b.wav"), 44100, _tone(5000, 44100))                             # float32, 44.1 kHz
    st = np.stack([_tone(4000, 44100, 220.0), _tone(4000, 44100, 440.0)], axis=1)
    wavfile.write(os.path.join(root, "c.wav"), 44100, st)                                             # float32 stereo
    rows = [{"file_name": "a.wav", "caption": "a low hum"}, {"file_name": "b.wav", "caption": "béla"}, {"file_name": "c.wav"}]
    if meta == "jsonl":
        with open(os.path.join(root, "metadata.jsonl"), "w", encoding="utf-8") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    else:
        with open(os.path.join(root, "metadata.csv"), "w", encoding="utf-8") as f:
            f.write("file_name,caption\n")
            for r in rows:
                f.write(f"{r['file_name']},{r.get('caption', '')}\n")
    return a, st


@pytest.mark.parametrize("meta", ["jsonl", "csv"])
def test_audio_folder(tmp_path, meta):
    root = str(tmp_path / "clips")
    a, st = _write_folder(root, meta)
    ds = D.AudioFolder(root, D.ByteTokenizer(), device="cpu")
    assert len(ds) == 3 and ds.files == ["a.wav", "b.wav", "c.wav"]
    assert ds.rates == [16000, 44100, 44100] and ds.lens == [3000, 5000, 4000] and ds.offsets == [0, 0, 5000]
    assert set(ds.pools) == {16000, 44100} and ds.pools[44100].shape == (9000,) and ds.pools[44100].dtype == torch.float32
    assert np.abs(ds.pools[16000].numpy() - a).max() <= 1.0 / 32767                      # PCM16 scaled by 1 / 32768
    assert np.array_equal(ds.pools[44100][:5000].numpy(), _tone(5000, 44100))
    assert np.allclose(ds.pools[44100][5000:].numpy(), st.mean(axis=1), atol=1e-7)      # mono by the channel mean
    assert ds.captions == ["a low hum", "béla", ""]                                      # a missing caption is ""
    assert ds.input_ids.shape == ds.attention_mask.shape == (3, 1, 512) and ds.input_ids.dtype == torch.long
    assert ds.input_ids[2, 0, :3].tolist() == [0, 2, 1] and int(ds.attention_mask[2].sum()) == 2
    body = list("béla".encode("utf-8"))
    assert ds.input_ids[1, 0, :len(body) + 3].tolist() == [0] + [b + 3 for b in body] + [2, 1]
    item = ds[1]
    assert item["audio"]["sampling_rate"] == 44100 and item["audio"]["array"].shape == (5000,) and item["caption"] == "béla"


def test_pcm_widths_and_bad_folders(tmp_path):
    assert np.array_equal(D.to_mono_f32(np.array([0, 128, 255], dtype=np.uint8)), np.array([-1.0, 0.0, 127 / 128], dtype=np.float32))
    assert np.array_equal(D.to_mono_f32(np.array([-32768, 16384], dtype=np.int16)), np.array([-1.0, 0.5], dtype=np.float32))
    assert np.array_equal(D.to_mono_f32(np.array([-2 ** 31, 2 ** 30], dtype=np.int32)), np.array([-1.0, 0.5], dtype=np.float32))
    assert D.to_mono_f32(np.array([0.25, -0.5], dtype=np.float64)).dtype == np.float32
    with pytest.raises(ValueError):
        D.to_mono_f32(np.array([1, 2], dtype=np.int64))
    with pytest.raises(FileNotFoundError):
        D.AudioFolder(str(tmp_path), D.ByteTokenizer(), device="cpu")
    # a 24-bit file: scipy hands it over left-justified in int32
    x = (np.array([0.5, -0.25, 0.125]) * 2 ** 23).astype(np.int32)
    raw = b"".join(int(v).to_bytes(3, "little", signed=True) for v in x)
    hdr = (b"RIFF" + (36 + len(raw)).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little")
           + (1).to_bytes(2, "little") + (8000).to_bytes(4, "little") + (24000).to_bytes(4, "little") + (3).to_bytes(2, "little")
           + (24).to_bytes(2, "little") + b"data" + len(raw).to_bytes(4, "little"))
    p = tmp_path / "w24.wav"
    p.write_bytes(hdr + raw)
    rate, data = wavfile.read(str(p))
    assert rate == 8000 and np.array_equal(D.to_mono_f32(data), np.array([0.5, -0.25, 0.125], dtype=np.float32))


def test_hf_audio_dataset_on_dict_rows():
    rows = [{"audio": {"array": np.arange(200, dtype=np.float64) / 400, "sampling_rate": 48000}, "caption": "x"},
            {"audio": {"array": np.ones(150, dtype=np.float32) * 0.1, "sampling_rate": 16000}},
            {"audio": {"array": np.zeros(120, dtype=np.float32), "sampling_rate": 48000}, "caption": None}]
    ds = D.HfAudioDataset(iter(rows), D.ByteTokenizer(), device="cpu")
    assert len(ds) == 3 and ds.rates == [48000, 16000, 48000] and ds.offsets == [0, 0, 200] and ds.captions == ["x", "", ""]
    assert ds.pools[48000].shape == (320,) and ds.pools[48000].dtype == torch.float32
    assert ds.input_ids[0, 0, :4].tolist() == [0, ord("x") + 3, 2, 1]
    with pytest.raises(ValueError):
        D.HfAudioDataset([], D.ByteTokenizer(), device="cpu")


def test_byte_tokenizer_truncates():
    enc = D.ByteTokenizer()("z" * 600)
    assert enc["input_ids"].shape == (1, 512) and enc["input_ids"][0, 0] == 0 and enc["input_ids"][0, -1] == 2
    assert int(enc["attention_mask"].sum()) == 512 and int(enc["input_ids"].max()) < D.ByteTokenizer.vocab_size


# ---- loader ---------------------------------------------------------------------------------------------------------------------
class _FakeDataset:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_loader_rank_sharding_is_disjoint_and_complete():
    ds = _FakeDataset(23)
    for world in (1, 2, 4):
        loaders = [D.ClipLoader(ds, None, 3, seed=7, rank=r, world=world) for r in range(world)]
        for epoch in (0, 1):
            parts = [ld.indices(epoch) for ld in loaders]
            assert sorted(i for p in parts for i in p) == list(range(23))
            assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
            assert [i for p in zip(*parts) for i in p] == loaders[0].permutation(epoch)[:world * min(len(p) for p in parts)]
    with pytest.raises(ValueError):
        D.ClipLoader(_FakeDataset(1), None, 1, rank=1, world=2)          # a rank without a clip
    with pytest.raises(ValueError):
        D.ClipLoader(ds, None, 0)


def test_loader_permutations_differ_between_epochs_and_repeat_for_a_seed():
    ds = _FakeDataset(50)
    a, b, c = D.ClipLoader(ds, None, 4, seed=1), D.ClipLoader(ds, None, 4, seed=1), D.ClipLoader(ds, None, 4, seed=2)
    assert a.permutation(0) == b.permutation(0) and a.permutation(3) == b.permutation(3)
    assert a.permutation(0) != a.permutation(1) and a.permutation(0) != c.permutation(0)
    assert sorted(a.permutation(1)) == list(range(50))


def test_loader_cursor_walks_epochs_and_resumes():
    ds = _FakeDataset(7)
    ld = D.ClipLoader(ds, None, 3, seed=5)
    assert len(ld) == 3
    seen = [ld.next_indices() for _ in range(7)]
    assert [len(s) for s in seen] == [3, 3, 1, 3, 3, 1, 3]                                 # short last batch, then the next epoch
    assert seen[0] + seen[1] + seen[2] == ld.permutation(0) and seen[3] + seen[4] + seen[5] == ld.permutation(1)
    assert (ld.epoch, ld.cursor) == (2, 3)
    # stopped after four batches, a fresh loader goes on with the fifth
    ld2 = D.ClipLoader(ds, None, 3, seed=5)
    for _ in range(4):
        ld2.next_indices()
    sd = ld2.state_dict()
    assert sd == {"epoch": 1, "cursor": 3, "seed": 5}
    ld3 = D.ClipLoader(ds, None, 3, seed=99)
    ld3.load_state_dict(sd)
    assert [ld3.next_indices() for _ in range(3)] == seen[4:]


def test_loader_iterates_epoch_by_epoch_and_collates_by_rate():
    """with a stand-in front end that records its groups: one iteration is (the rest of) one epoch, rows are grouped by sampling rate
    with their place in the batch as ordinal, and the token tensors follow the permutation"""
    class Rows(_FakeDataset):
        def __init__(self, n):
            super().__init__(n)
            self.rates = [16000 if i % 3 else 44100 for i in range(n)]
            self.offsets, self.lens = [10 * i for i in range(n)], [200 + i for i in range(n)]
            self.pools = {16000: "pool16", 44100: "pool44"}
            self.input_ids = torch.arange(n)[:, None, None].expand(n, 1, 512)
            self.attention_mask = torch.ones(n, 1, 512, dtype=torch.long)

    class Recorder:
        def __init__(self):
            self.calls = []

        def run_groups(self, groups, B):
            self.calls.append((groups, B))
            return {"log_mel_spec": torch.zeros(B, 1, 12, 64)}

    ds, fe = Rows(7), Recorder()
    ld = D.ClipLoader(ds, fe, 3, seed=5)
    ld.next_indices()                                                   # an epoch already under way
    batches = list(ld)
    assert len(batches) == 2 and (ld.epoch, ld.cursor) == (1, 0) and len(list(ld)) == 3 and ld.epoch == 2
    perm = ld.permutation(0)
    assert [b["input_ids"][:, 0, 0].tolist() for b in batches] == [perm[3:6], perm[6:]]
    assert set(batches[0]) == {"log_mel_spec", "input_ids", "attention_mask"} and batches[0]["input_ids"].shape == (3, 1, 512)
    groups, B = fe.calls[0]
    assert B == 3 and [g["rate"] for g in groups] == sorted({ds.rates[i] for i in perm[3:6]})
    seen_rows = sorted(r for g in groups for r in g["rows"])
    assert seen_rows == [0, 1, 2] and all(g["ordinals"] == g["rows"] for g in groups)
    for g in groups:
        assert g["pool"] == ds.pools[g["rate"]]
        assert g["offsets"] == [ds.offsets[perm[3 + r]] for r in g["rows"]] and g["lens"] == [ds.lens[perm[3 + r]] for r in g["rows"]]


# ---- C-ABI and driver -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("aldm_clip_segment", "aldm_clip_segment_workspace_floats", "aldm_clip_normalize", "aldm_clip_normalize_parts")


def test_new_symbols_are_declared_and_bound():
    from audioldm_with_lora_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aldm_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert len(_lib.PROTOTYPES["aldm_clip_segment"][1]) == 14 and len(_lib.PROTOTYPES["aldm_clip_normalize"][1]) == 8
    assert "Clip-segment stream contract" in open(os.path.join(ROOT, "audioldm_with_lora_amd", "csrc", "philox.h")).read()
    assert lib.aldm_clip_segment_workspace_floats(3, 1024) == 3 and lib.aldm_clip_segment_workspace_floats(3, 1025) == 6
    assert lib.aldm_clip_normalize_parts(2048, 2048) == 1 and lib.aldm_clip_normalize_parts(5000, 2049) == 2
    assert lib.aldm_clip_normalize_parts(163840, 163840) == 64                              # 128 workgroups at batch 2


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    """every ALDM_CHECK_ARG returns before anything is launched (the pointers are never followed)"""
    from audioldm_with_lora_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    good = [p, 4096, p, p, p, 2, 2048, 4096, p, 1, p, p, p, None]
    for pos, bad in ((0, None), (2, None), (3, None), (4, None), (8, None), (10, None), (11, None), (12, None), (1, 0), (5, 0), (5, 65536),
                     (6, 0), (7, 0)):
        args = list(good)
        args[pos] = bad
        assert lib.aldm_clip_segment(*args) == -1, (pos, bad)
        assert b"clip_segment" in lib.aldm_last_error()
    good = [p, p, 2, 2048, 2048, p, p, None]
    for pos, bad in ((0, None), (1, None), (5, None), (6, None), (2, 0), (3, 0), (4, 0)):
        args = list(good)
        args[pos] = bad
        assert lib.aldm_clip_normalize(*args) == -1, (pos, bad)
        assert b"clip_normalize" in lib.aldm_last_error()


def test_no_cpu_fallback():
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd._lib import AldmError
    with pytest.raises(AldmError):
        D.ClipFrontEnd("cpu")
    with pytest.raises(AldmError):
        ops.clip_normalize(torch.zeros(1, 64), [64], 64)


def test_package_exports():
    import audioldm_with_lora_amd as pkg
    for name in ("ClipFrontEnd", "HfAudioDataset", "AudioFolder", "ClipLoader"):
        assert getattr(pkg, name) is getattr(D, name)


def test_train_parser_accepts_the_new_flags():
    from audioldm_with_lora_amd.script import train
    ap = train.build_parser()
    args = ap.parse_args(["--audio-dir", "clips", "--duration", "2.56", "--data-seed", "11"])
    assert (args.audio_dir, args.duration, args.data_seed) == ("clips", 2.56, 11)
    args = ap.parse_args([])
    assert (args.audio_dir, args.duration, args.data_seed) == (None, 10.24, None)           # --data-seed: --seed + 1 when not given
    assert "out of scope" not in train.__doc__ and "--audio-dir" in train.__doc__


def test_resuming_from_a_checkpoint_without_a_data_position(tmp_path, capsys):
    """a checkpoint written without --audio-dir holds no data.bin: the loader stays at the start, with a warning, instead of a bare
    FileNotFoundError; one that holds it is restored"""
    from audioldm_with_lora_amd.script import train

    class FrontEnd:
        sd = {"seed": 4, "key": 1, "ordinal": 9, "rank": 0}

        def state_dict(self):
            return dict(self.sd)

        def load_state_dict(self, sd):
            self.sd = dict(sd)

    ld = D.ClipLoader(_FakeDataset(7), FrontEnd(), 3, seed=5)
    assert train.load_data_state(str(tmp_path), ld) is False and (ld.epoch, ld.cursor) == (0, 0)
    assert "no data.bin" in capsys.readouterr().out
    for _ in range(4):
        ld.next_indices()
    train.save_data_state(str(tmp_path), ld)
    fresh = D.ClipLoader(_FakeDataset(7), FrontEnd(), 3, seed=5)
    fresh.front_end.sd = {}
    assert train.load_data_state(str(tmp_path), fresh) is True
    assert (fresh.epoch, fresh.cursor) == (1, 3) and fresh.front_end.sd["ordinal"] == 9
