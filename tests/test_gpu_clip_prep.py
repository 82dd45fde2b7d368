"""GPU: the clip front end (csrc/clip_prep.hip, data.py) -- the segment rule bit for bit against the integer restatement at every
length where the kernels take another path, the normalisation against float64 within the derived bound, the whole front end on a
batch of mixed sampling rates, and the training driver from a folder of wavs, resumed.

duration = 0.128 s throughout: 2048 samples at 16 kHz, 12 log-mel frames."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import clip_prep_restatement as CR  # noqa: E402
import resample_restatement as RR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DURATION = 0.128
S = 2048                                       # the segment at 16 kHz
SEED = 0x1234567890ABCDEF
LOUD = np.float32(0.3)
THRESHOLD = np.float32(1e-4)


def _run_segment(rows, ordinals, seed=SEED, draw=5, advance=False, state=None):
    """rows: fp32 arrays -> (starts list, seg fp32 [B, S] numpy, state) of one ops.clip_segment call over a pool that holds them"""
    from audioldm_with_lora_amd import ops
    lens = [len(r) for r in rows]
    offsets = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    pool = torch.from_numpy(np.concatenate(rows)).to(DEV)
    state = ops.philox_state(seed, draw, DEV) if state is None else state
    seg, start = ops.clip_segment(pool, offsets, lens, ordinals, S, state, max_len=max(lens), advance=advance)
    assert seg.shape == (len(rows), S) and seg.dtype == torch.float32 and start.dtype == torch.int32 and start.is_cuda
    return start.cpu().tolist(), seg.cpu().numpy(), state


def _check_rows(rows, ordinals, starts, segs, seed=SEED, draw=5):
    for r, o, st, sg in zip(rows, ordinals, starts, segs):
        want_start, want_seg = CR.segment(r, S, seed, draw, o)
        assert st == want_start, (len(r), o, st, want_start)
        assert np.array_equal(sg.view(np.uint32), want_seg.view(np.uint32)), (len(r), o)


LENGTHS = (101, S - 1, S, S + 1, S + 1023, S + 1024, S + 1025, 10 * S + 7, 2 ** 20 + 3)


def test_segment_lengths_at_every_edge():
    """noise rows (every window holds a sound, so candidate 0 wins): short rows are copied and padded, rows one sample longer than the
    segment, rows that end exactly on / one before / one behind a chunk of 1024, a row of ten segments, one of 2^20 + 3 samples"""
    rows = [RR.clip(L, 40 + i) for i, L in enumerate(LENGTHS)]
    ordinals = list(range(len(rows)))
    starts, segs, _ = _run_segment(rows, ordinals)
    _check_rows(rows, ordinals, starts, segs)
    for L, st, o in zip(LENGTHS, starts, ordinals):
        assert st == (0 if L <= S else CR.candidate_starts(SEED, 5, o, L - S)[0])
    assert not segs[0][101:].any() and not segs[1][S - 1:].any()


def test_segment_one_loud_sample_at_the_window_edges():
    """zeros and ONE loud sample per row, placed from the restated candidate starts: on the first and on the last sample of candidate
    c's window (hits), one behind it and one in front of it (misses: a later candidate that holds the sample, or the tenth)"""
    rows, ordinals, expect_c = [], [], []
    for L, c in [(L, 0) for L in LENGTHS[3:]] + [(10 * S + 7, 4), (2 ** 20 + 3, 9)]:
        for place in ("first", "last", "behind", "before"):
            o = len(rows)
            cands = CR.candidate_starts(SEED, 5, o, L - S)
            pos = {"first": cands[c], "last": cands[c] + S - 1, "behind": cands[c] + S, "before": cands[c] - 1}[place]
            if pos < 0:
                pos = 0                                               # (candidate at 0: nothing in front of it; still compared)
            x = np.zeros(L, dtype=np.float32)
            x[pos] = LOUD if o % 2 else -LOUD
            rows.append(x)
            ordinals.append(o)
            holds = [k for k in range(10) if cands[k] <= pos < cands[k] + S]
            expect_c.append(holds[0] if holds else 9)
            if place in ("first", "last"):
                assert holds and holds[0] <= c
            elif cands[c] > 0 or place == "behind":
                assert c not in holds
    starts, segs, _ = _run_segment(rows, ordinals)
    _check_rows(rows, ordinals, starts, segs)
    for o, (r, st, k) in enumerate(zip(rows, starts, expect_c)):
        assert st == CR.candidate_starts(SEED, 5, o, len(r) - S)[k]
    assert len(set(expect_c)) > 2                                     # hits, later candidates and the tenth all occur


def test_segment_threshold_is_strict_and_silence_takes_the_tenth():
    L = 10 * S + 7
    above = np.nextafter(THRESHOLD, np.float32(1))
    rows = [np.zeros(L, dtype=np.float32), np.full(L, THRESHOLD, dtype=np.float32), np.full(L, -THRESHOLD, dtype=np.float32)]
    for sign in (1, -1):                                              # exactly 1e-4 everywhere but one sample just above, in window 0
        x = np.full(L, THRESHOLD, dtype=np.float32)
        x[CR.candidate_starts(SEED, 5, len(rows), L - S)[0] + 1500] = sign * above
        rows.append(x)
    ordinals = list(range(len(rows)))
    starts, segs, _ = _run_segment(rows, ordinals)
    _check_rows(rows, ordinals, starts, segs)
    for o in range(3):
        assert starts[o] == CR.candidate_starts(SEED, 5, o, L - S)[9]
    for o in (3, 4):
        assert starts[o] == CR.candidate_starts(SEED, 5, o, L - S)[0]


def test_segment_rows_in_any_order_and_any_batch():
    """a row's result depends on its ordinal and its samples, not on where it stands or what stands beside it"""
    rng = np.random.default_rng(3)
    rows = []
    for i in range(12):
        L = int(rng.integers(S + 1, 6 * S))
        x = np.zeros(L, dtype=np.float32)
        a = int(rng.integers(0, L - 300))
        x[a:a + 300] = RR.clip(300, 70 + i)                          # one short burst: most candidates miss
        rows.append(x)
    ordinals = list(range(12))
    starts, segs, _ = _run_segment(rows, ordinals)
    _check_rows(rows, ordinals, starts, segs)
    assert len({CR.candidate_starts(SEED, 5, o, len(r) - S).index(s) for o, (r, s) in enumerate(zip(rows, starts))}) > 1
    perm = [int(i) for i in rng.permutation(12)]
    s2, g2, _ = _run_segment([rows[i] for i in perm], perm)
    for k, i in enumerate(perm):
        assert s2[k] == starts[i] and np.array_equal(g2[k], segs[i])
    s3, g3, _ = _run_segment([rows[7], rows[2]], [7, 2])
    assert s3 == [starts[7], starts[2]] and np.array_equal(g3[0], segs[7]) and np.array_equal(g3[1], segs[2])


def test_segment_two_calls_use_two_draws():
    from audioldm_with_lora_amd import ops
    rows = [RR.clip(5 * S + i, 90 + i) for i in range(3)]
    d = 2 ** 32 - 1                                                   # the second draw carries into the ordinal's high word
    s1, g1, state = _run_segment(rows, [0, 1, 2], draw=d, advance=True)
    assert ops.philox_state_values(state) == (SEED, d + 1)
    s2, g2, state = _run_segment(rows, [0, 1, 2], advance=True, state=state)
    assert ops.philox_state_values(state) == (SEED, d + 2)
    _check_rows(rows, [0, 1, 2], s1, g1, draw=d)
    _check_rows(rows, [0, 1, 2], s2, g2, draw=d + 1)
    assert s1 != s2
    s3, g3, state = _run_segment(rows, [0, 1, 2], advance=False, state=state)
    assert ops.philox_state_values(state) == (SEED, d + 2)
    _check_rows(rows, [0, 1, 2], s3, g3, draw=d + 2)


def test_segment_in_a_captured_graph():
    from audioldm_with_lora_amd import ops
    rows = [RR.clip(3 * S + 11 * i, 95 + i) for i in range(4)]
    lens = [len(r) for r in rows]
    pool = torch.from_numpy(np.concatenate(rows)).to(DEV)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lens[:-1])]), dtype=torch.int64, device=DEV)
    dlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ords = torch.arange(4, dtype=torch.int32, device=DEV)
    state = ops.philox_state(SEED, 20, DEV)
    eager = [ops.clip_segment(pool, offsets, dlens, ords, S, state, max_len=max(lens)) for _ in range(2)]
    assert ops.philox_state_values(state) == (SEED, 22) and not torch.equal(eager[0][1], eager[1][1])
    seg, start = torch.empty(4, S, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV)

    def body():
        a, b = ops.clip_segment(pool, offsets, dlens, ords, S, state, max_len=max(lens))
        seg.copy_(a)
        start.copy_(b)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    ops.philox_set(state, draw=20)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        body()
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(start, eager[k][1]) and torch.equal(seg, eager[k][0])
    assert ops.philox_state_values(state) == (SEED, 22)


# ---- normalise ------------------------------------------------------------------------------------------------------------------
def _check_normalize(y, n, target):
    """y fp32 [B, T] numpy, n list -> the worst |error| / bound; asserts the bound on every counted sample and exact zeros behind"""
    from audioldm_with_lora_amd import ops
    out = ops.clip_normalize(torch.from_numpy(y).to(DEV), n, target)
    assert out.shape == (len(n), target) and out.dtype == torch.float32
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    worst = 0.0
    for b, nb in enumerate(n):
        m = min(nb, target, y.shape[1])
        want = CR.normalize(y[b], nb, target)
        assert not got[b, m:].any(), (b, nb)
        if m:
            err, lim = np.abs(got[b, :m].astype(np.float64) - want[:m]), CR.normalize_bound(y[b, :m])
            assert (err <= lim).all(), (b, nb, float((err / lim).max()))
            worst = max(worst, float((err / lim).max()))
    return worst


@pytest.mark.parametrize("target", [2048, 5000, 163840])
def test_normalize_against_float64(target):
    """a DC offset 1000 x the AC amplitude; n = 1, 101, target - 1, target, target + 5 (cropped), 0, and -- at 5000, where three
    workgroups share a row, and at the full-size 163 840, where the count is capped at 64 workgroups of 2560 samples -- both sides of
    a slice edge.  Bound: clip_prep_restatement.normalize_bound."""
    import conftest
    from audioldm_with_lora_amd import _lib
    parts = _lib.load().aldm_clip_normalize_parts(target + 5, target)
    assert parts == {2048: 1, 5000: 3, 163840: 64}[target]
    slice_ = -(-target // parts)
    n = [1, 101, target - 1, target, target + 5, 0] + ([slice_, slice_ + 1, 2 * slice_ - 1, (parts - 1) * slice_ + 1] if parts > 1 else [])
    rng = np.random.default_rng(target)
    y = (100.0 + 0.1 * rng.standard_normal((len(n), target + 5))).astype(np.float32)
    worst = _check_normalize(y, n, target)
    plain = (0.3 * rng.standard_normal((2, target + 5))).astype(np.float32)                     # and rows without an offset
    worst = max(worst, _check_normalize(plain, [target, 777], target))
    conftest.record(worst, "max_err_over_bound")


def test_normalize_constant_row_and_empty_row():
    from audioldm_with_lora_amd import ops
    y = torch.full((3, 5003), 0.25, device=DEV)
    out = ops.clip_normalize(y, [5003, 3000, 0], 5000)
    assert out.shape == (3, 5000) and not torch.isnan(out).any() and not out.any()              # exact zeros
    z = torch.from_numpy(RR.clip(4096, 1)).to(DEV)[None]
    a = ops.clip_normalize(z, torch.tensor([4096], dtype=torch.int32, device=DEV), 4096)
    b = ops.clip_normalize(z.repeat(3, 1), [4096, 1000, 4096], 4096)
    assert torch.equal(a[0], b[0]) and torch.equal(a[0], b[2])                                  # independent of B and of the row
    assert abs(float(a.abs().max()) - 0.5) < 1e-6


# ---- the whole front end ----------------------------------------------------------------------------------------------------------
def test_front_end_on_a_batch_of_mixed_rates():
    """waveform against segment -> resample_restatement -> normalize.  Bound per sample: the resampler test's tolerance
    e = (Kn + 2) 2^-24 S carried through the normalisation, plus normalize_bound.  A perturbation of y by at most e_max moves the mean
    by at most e_max and the peak by at most 2 e_max, so out = (y - mean) / (2 (peak + 1e-8)) moves by at most
    (e_max + e_max) / (2 peak) + |ref| 2 e_max / peak <= 2 e_max / (peak + 1e-8)."""
    import conftest
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd import resample as R
    from audioldm_with_lora_amd.data import STREAM_KEY, ClipFrontEnd
    from audioldm_with_lora_amd.mel import LogMelFrontEnd
    from audioldm_with_lora_amd.training import noise_ordinal_base
    fe = ClipFrontEnd(DEV, duration=DURATION, seed=21, rank=1)
    assert fe.target == 2048 and fe.log_mel.dsp["target_length"] == 12
    assert [fe.segment_length(r) for r in (16000, 24000, 44100)] == [2048, 3072, 5644]
    rates = [44100, 16000, 24000, 16000, 44100, 24000, 44100]
    lens = [20000, 5000, 3072, 900, 3001, 9001, 5645]
    rows = []
    for i, L in enumerate(lens):
        x = np.zeros(L, dtype=np.float32)
        a = L // 3
        x[a:] = 0.05 + RR.clip(L - a, 300 + i)                        # a silent head, then sound on a small offset
        rows.append(x)
    wavs = [torch.from_numpy(r).to(DEV) for r in rows]
    key, base = 21 ^ STREAM_KEY, noise_ordinal_base(1)
    assert ops.philox_state_values(fe.state) == (key, base)
    out = fe(wavs, rates)
    assert ops.philox_state_values(fe.state) == (key, base + 1) and fe.state_dict()["ordinal"] == base + 1
    wf, mel, rs = out["waveform"], out["log_mel_spec"], out["random_start"]
    assert wf.shape == (7, 1, 2048) and mel.shape == (7, 1, 12, 64) and rs.shape == (7,) and rs.dtype == torch.int32 and rs.is_cuda
    got = wf[:, 0].cpu().numpy()
    worst = 0.0
    for i, (x, rate) in enumerate(zip(rows, rates)):
        Sr = int(rate * DURATION)
        start, seg = CR.segment(x, Sr, key, base, i)
        assert int(rs[i]) == start
        n_in = min(len(x), Sr)
        up, down = R.ratio(rate, 16000)
        if up == down:
            y, e_max = seg[:n_in].astype(np.float64), 0.0
        else:
            y, Sabs, Kn = RR.restate(seg, up, down, length=n_in)
            e_max = float(RR.bound(Sabs, Kn).max())
        m = min(len(y), 2048)
        want = CR.normalize(y, len(y), 2048)
        d = y[:m] - y[:m].mean()
        lim = 2.0 * e_max / (np.abs(d).max() + 1e-8) + CR.normalize_bound(y[:m])
        err = np.abs(got[i, :m].astype(np.float64) - want[:m])
        assert (err <= lim).all(), (i, rate, float((err / lim).max()))
        assert not got[i, m:].any()
        worst = max(worst, float((err / lim).max()))
    conftest.record(worst, "max_err_over_bound")
    assert torch.equal(mel, LogMelFrontEnd(DEV, target_length=12)(wf[:, 0].contiguous()))
    # grouping changes nothing: the 44.1 kHz rows alone, and the pool form, from the same draw
    fe.load_state_dict(dict(fe.state_dict(), ordinal=base))
    sub = fe([wavs[i] for i in (4, 0, 6)], 44100, ordinals=[4, 0, 6], advance=False)
    for k, i in enumerate((4, 0, 6)):
        assert torch.equal(sub["waveform"][k], wf[i]) and torch.equal(sub["log_mel_spec"][k], mel[i]) and int(sub["random_start"][k]) == int(rs[i])
    offsets = np.concatenate([[0], np.cumsum(lens[:-1])])
    again = fe((torch.cat(wavs), offsets, lens), rates)
    assert torch.equal(again["waveform"], wf) and torch.equal(again["log_mel_spec"], mel) and torch.equal(again["random_start"], rs)
    assert ops.philox_state_values(fe.state) == (key, base + 1)
    with pytest.raises(ValueError, match="too short"):
        fe([wavs[0], torch.zeros(100, device=DEV)], 16000)
    assert ops.philox_state_values(fe.state) == (key, base + 1)      # a refused batch draws nothing


# ---- training -------------------------------------------------------------------------------------------------------------------
def _write_clips(root):
    from scipy.io import wavfile
    os.makedirs(root)
    meta = []
    for i, (rate, secs) in enumerate(((16000, 1.0), (44100, 1.5), (16000, 0.5), (44100, 0.9), (24000, 1.2))):
        n = int(rate * secs)
        x = RR.clip(n, 500 + i)
        x[:n // 4] = 0.0
        name = f"clip{i}.wav"
        wavfile.write(os.path.join(root, name), rate, x if i % 2 else np.round(x * 32767).astype(np.int16))
        meta.append({"file_name": name, "caption": f"sound number {i}"})
    with open(os.path.join(root, "metadata.jsonl"), "w") as f:
        for m in meta:
            f.write(json.dumps(m) + "\n")


def test_train_script_from_a_folder_of_wavs_and_resume(tmp_path, monkeypatch):
    """train.py --tiny --audio-dir: two steps to a finite loss; resumed from the checkpoint of step 1, step 2 cuts the segments --
    and sees the log-mel -- of the uninterrupted run, and ends at the same stream position and cursor"""
    from audioldm_with_lora_amd import data as D
    from audioldm_with_lora_amd.script import train
    clips = str(tmp_path / "clips")
    _write_clips(clips)
    seen = []
    collate = D.ClipLoader.collate

    def spy(self, take):
        batch = collate(self, take)
        seen.append((list(take), self.last["random_start"].cpu().tolist(), batch["log_mel_spec"].clone()))
        return batch

    monkeypatch.setattr(D.ClipLoader, "collate", spy)
    common = ["--tiny", "--audio-dir", clips, "--duration", "0.64", "--train-batch-size", "2", "--device-noise", "--max-train-steps", "2",
              "--checkpointing-steps", "1", "--learning-rate", "1e-3", "--seed", "3"]
    out_a, out_b = str(tmp_path / "a"), str(tmp_path / "b")
    loss = train.main(common + ["--output-dir", out_a])
    assert loss == loss and 0.0 < loss < 10.0
    whole, seen[:] = list(seen), []
    assert len(whole) == 2 and whole[0][2].shape == (2, 1, 64, 64) and torch.isfinite(whole[0][2]).all()
    assert whole[0][0] != whole[1][0]
    state_1, state_2 = (torch.load(os.path.join(out_a, f"checkpoint-{k}", "data.bin")) for k in (1, 2))
    assert state_1["loader"] == {"epoch": 0, "cursor": 2, "seed": 4} and state_2["loader"]["cursor"] == 4      # --data-seed: --seed + 1
    assert state_2["front_end"]["ordinal"] == state_1["front_end"]["ordinal"] + 1 and state_1["front_end"]["seed"] == 4
    loss_b = train.main(common + ["--output-dir", out_b, "--resume-from-checkpoint", os.path.join(out_a, "checkpoint-1")])
    assert loss_b == loss_b and 0.0 < loss_b < 10.0
    assert len(seen) == 1
    assert seen[0][0] == whole[1][0] and seen[0][1] == whole[1][1] and torch.equal(seen[0][2], whole[1][2])
    assert torch.load(os.path.join(out_b, "checkpoint-2", "data.bin")) == state_2


@pytest.mark.parametrize("device_noise", [True, False])
def test_train_script_crosses_an_epoch_with_a_short_last_batch(tmp_path, device_noise):
    """five clips at batch 2 are batches of 2, 2 and 1, then the next epoch: four steps take the short batch and the wrap, with the noise
    drawn on the device (step_from_batch) and on the host (encode_batch, timesteps sized by the batch at hand)"""
    from audioldm_with_lora_amd.script import train
    clips, out = str(tmp_path / "clips"), str(tmp_path / "out")
    _write_clips(clips)
    loss = train.main(["--tiny", "--audio-dir", clips, "--duration", "0.64", "--train-batch-size", "2", "--max-train-steps", "4",
                       "--learning-rate", "1e-3", "--seed", "3", "--output-dir", out] + (["--device-noise"] if device_noise else []))
    assert loss == loss and 0.0 < loss < 10.0
    state = torch.load(os.path.join(out, "checkpoint-4", "data.bin"))
    assert state["loader"] == {"epoch": 1, "cursor": 2, "seed": 4}
