"""GPU: BS.1770 loudness metering and normalisation (csrc/loudness.hip, loudness.py) -- hop energies and the gated loudness against the
float64 restatement, the peak, the normalisation gain and its ceiling, the chain in a replayed graph, and the option in the pipelines
and the scripts."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loudness_restatement as LR  # noqa: E402
import resample_restatement as RR  # noqa: E402
from audioldm_with_lora_amd import loudness as L  # noqa: E402
from audioldm_with_lora_amd import resample as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = L.CHUNK
RATES = (16000, 44100, 48000)
INPUTS = ("dc", "white", "sine", "impulse")
ENERGY_BOUND = 1e-9       # relative, per hop: the float64 ordering floor (1e-12, test_loudness_host) x 1000
LUFS_BOUND = 1e-3         # two orders under EBU Tech 3341's +-0.1 LU


def _lengths(fs):
    H = fs // 10
    return {"4H-1": 4 * H - 1, "4H": 4 * H, "4H+1": 4 * H + 1, "C-1": C - 1, "C": C, "C+1": C + 1, "2C+1": 2 * C + 1, "3s": 3 * fs + 37}


# the three ragged lengths of every input's batch; together they cover the whole list at every rate
BATCH_LENGTHS = {"dc": ("3s", "4H-1", "C+1"), "white": ("4H+1", "C-1", "2C+1"), "sine": ("4H", "C", "3s"), "impulse": ("4H+1", "3s", "2C+1")}


def _signal(name, n, fs, row):
    if name == "dc":
        return LR.dc_case(n, fs, seed=10 + row)
    if name == "white":
        return LR.white(n, seed=20 + row)
    if name == "sine":
        return LR.sine(fs, n / fs)[:n]
    H = fs // 10
    if row == 1:                                                    # the last sample of the last chunk that has a successor
        pos = ((n // H * H - 1) // C) * C - 1
    else:                                                           # the last sample of the first chunk
        pos = C - 1
    return LR.impulse_at(n, pos)


@functools.lru_cache(maxsize=None)
def _batch(fs, name):
    """(x fp32 [3, T] host, lens, reference hop energies per row, reference loudness per row); junk behind every row's length"""
    lens = [_lengths(fs)[k] for k in BATCH_LENGTHS[name]]
    T = max(lens)
    x = np.random.RandomState(7).uniform(-1.0, 1.0, (3, T)).astype(np.float32)          # the junk
    for b, n in enumerate(lens):
        x[b, :n] = _signal(name, n, fs, b).astype(np.float32)
    ref_e = [LR.hop_energies(x[b, :n].astype(np.float64), fs) for b, n in enumerate(lens)]
    ref_l = [LR.loudness(e, fs // 10) for e in ref_e]
    return x, lens, ref_e, ref_l


def test_lengths_cover_the_list():
    assert set(k for v in BATCH_LENGTHS.values() for k in v) == set(_lengths(16000))
    for fs in RATES:                                                # an impulse really sits on a chunk's last sample, inside a counted hop
        x, lens, ref_e, _ = _batch(fs, "impulse")
        for b, n in enumerate(lens):
            (pos,) = np.nonzero(x[b, :n])
            assert pos.size == 1 and (pos[0] + 1) % C == 0
        assert ref_e[1].size == 30 and ref_e[1][:-1].max() == 0.0 and ref_e[1][-1] > 0.1


@pytest.mark.parametrize("fs", RATES)
def test_hop_energies_against_the_restatement(fs):
    import conftest
    m = L.meter(fs, DEV)
    worst = 0.0
    for name in INPUTS:
        x, lens, ref_e, _ = _batch(fs, name)
        e = m.hop_energies(torch.from_numpy(x).to(DEV), lens)
        assert e.dtype == torch.float64 and e.shape == (3, x.shape[1] // (fs // 10))
        e = e.cpu().numpy()
        for b, want in enumerate(ref_e):
            err = LR.rel_err(e[b, :want.size], want)
            print(f"{fs} {name} row {b} len {lens[b]}: worst relative hop-energy error {err:.3e}")
            assert err <= ENERGY_BOUND, (fs, name, b, err)
            assert not e[b, want.size:].any()                        # hops past the clip are exactly 0
            worst = max(worst, err)
    conftest.record(worst, "hop_energy_rel_err")


@functools.lru_cache(maxsize=None)
def _host_cases():
    """the three host cases of test_loudness_host: (fs, fp32 samples, reference loudness)"""
    out = []
    for fs, x in ((48000, LR.sine(48000, 5.0)), (16000, LR.sine(16000, 5.0)), (16000, LR.two_level(16000, -50.0)),
                  (16000, LR.two_level(16000, None))):
        x = x.astype(np.float32)
        out.append((fs, x, LR.integrated(x.astype(np.float64), fs)))
    return out


def test_integrated_loudness_host_cases():
    import conftest
    worst = 0.0
    want_about = (-3.0103, -2.9700, -23.186, -23.186)
    for (fs, x, ref), about in zip(_host_cases(), want_about):
        got = L.integrated_loudness(torch.from_numpy(x).to(DEV), fs)
        assert got.dtype == torch.float64 and got.shape == (1,) and got.is_cuda
        err = abs(float(got[0]) - ref)
        print(f"{fs}: {float(got[0]):.6f} LUFS, reference {ref:.6f}")
        assert err <= LUFS_BOUND and abs(ref - about) <= 1e-3
        worst = max(worst, err)
    conftest.record(worst, "lufs_abs_err")


@pytest.mark.parametrize("fs", RATES)
def test_integrated_loudness_ragged_batches(fs):
    import conftest
    m = L.meter(fs, DEV)
    worst = 0.0
    n_inf = 0
    for name in INPUTS:
        x, lens, _, ref_l = _batch(fs, name)
        xg = torch.from_numpy(x).to(DEV)
        got = m.measure(xg, lens)
        for b, want in enumerate(ref_l):
            alone = m.measure(xg[b:b + 1, :lens[b]].contiguous())
            assert torch.equal(alone, got[b:b + 1]), (fs, name, b)      # a clip of a batch is the clip alone, bitwise
            if np.isinf(want):
                n_inf += 1
                assert float(got[b]) == -np.inf                         # (torch.equal above: the same bits alone)
            else:
                worst = max(worst, abs(float(got[b]) - want))
                assert abs(float(got[b]) - want) <= LUFS_BOUND, (fs, name, b, float(got[b]), want)
    assert n_inf >= 3                                                   # 4H - 1, C - 1, C, C + 1 ...: shorter than a block
    conftest.record(worst, "lufs_abs_err")


def test_peak():
    from audioldm_with_lora_amd import ops
    m = L.meter(16000, DEV)
    x, lens, _, _ = _batch(16000, "white")
    xg = torch.from_numpy(x).to(DEV)
    p1, p4 = m.peak(xg, lens, oversample=1), m.peak(xg, lens, oversample=4)
    up, out_lens = ops.resample_poly(xg, 4, 1, lens)
    assert p1.dtype == p4.dtype == torch.float32 and p1.shape == p4.shape == (3,)
    for b, n in enumerate(lens):
        assert out_lens[b] == 4 * n
        assert torch.equal(p1[b], xg[b, :n].abs().max())
        assert torch.equal(p4[b], up[b, :4 * n].abs().max())
        assert float(p4[b]) >= float(p1[b])                             # phase 0 of the interpolation is the samples themselves, nearly
    planted = xg.clone()
    for b, n in enumerate(lens):
        if n < planted.shape[1]:
            planted[b, n] = 1e6                                          # behind the clip: counts for nothing
    assert torch.equal(m.peak(planted, lens, oversample=1), p1) and torch.equal(m.peak(planted, lens, oversample=4), p4)
    assert torch.equal(m.peak(xg[0], None, oversample=1), xg[0].abs().max()[None])                       # 1-D: a batch of one
    assert float(m.peak(xg, [0, 0, 0], oversample=4).abs().max()) == 0.0


def _normalise_batch():
    """16 kHz, five ragged rows: quiet noise (gain up, ceiling idle), the full-scale sine (gain down), an impulse train (the ceiling
    binds), a clip shorter than a block and a silent one (loudness -inf)"""
    fs, H = 16000, 1600
    lens = [16000 + 37, 16000, 16000, 4 * H - 1, 8000]
    T = max(lens) + 100
    x = np.random.RandomState(9).uniform(-1.0, 1.0, (5, T)).astype(np.float32)           # junk behind the lengths
    x[0, :lens[0]] = 0.1 * LR.white(lens[0], seed=30)
    x[1, :lens[1]] = LR.sine(fs, 1.0)
    x[2, :lens[2]] = 0.0
    x[2, 100:lens[2]:400] = 0.5
    x[3, :lens[3]] = 0.3 * LR.white(lens[3], seed=31)
    x[4, :lens[4]] = 0.0
    return fs, x, lens


def test_normalize():
    import conftest
    fs, x, lens = _normalise_batch()
    target, ceiling = -14.0, -1.0
    cap = 10.0 ** (ceiling / 20.0)
    m = L.meter(fs, DEV)
    xg = torch.from_numpy(x).to(DEV)
    y, info = L.normalize_loudness(xg, fs, target, ceiling, lens=lens)
    assert y.shape == xg.shape and y.dtype == torch.float32
    assert set(info) == {"lufs_in", "gain_db", "peak_in"} and all(v.is_cuda and v.shape == (5,) for v in info.values())
    assert torch.equal(info["lufs_in"], m.measure(xg, lens)) and torch.equal(info["peak_in"], m.peak(xg, lens, 4))
    after = m.measure(y, lens).cpu().numpy()
    peak_after = m.peak(y, lens, 4).cpu().numpy().astype(np.float64)
    lufs_in, gain_db, peak_in = (info[k].cpu().numpy().astype(np.float64) for k in ("lufs_in", "gain_db", "peak_in"))
    gain = (y[2, 100] / xg[2, 100]).item()
    worst_db = 0.0
    for b, n in enumerate(lens):
        assert not y[b, n:].any()                                        # zeros behind the clip
        assert peak_after[b] <= cap * (1.0 + 2.0 ** -23), (b, peak_after[b])     # the ceiling, within one fp32 ulp
        ref_l = LR.integrated(x[b, :n].astype(np.float64), fs)
        os_peak = float(np.max(np.abs(RR.restate(x[b, :n], 4, 1)[0]))) if np.isfinite(ref_l) else 0.0
        ref_gain = LR.gain(ref_l, os_peak, target, ceiling)
        worst_db = max(worst_db, abs(gain_db[b] - 20.0 * np.log10(ref_gain)))
        assert abs(gain_db[b] - 20.0 * np.log10(ref_gain)) <= 1e-3, (b, gain_db[b], ref_gain)
        if not np.isfinite(ref_l):
            assert lufs_in[b] == -np.inf and gain_db[b] == 0.0 and torch.equal(y[b, :n], xg[b, :n])     # unchanged, bitwise
        elif ref_gain * os_peak < cap * (1.0 - 1e-6):
            assert abs(after[b] - target) <= 2e-3, (b, after[b])         # the ceiling did not bind: on target
        else:
            assert b == 2 and after[b] < target - 1.0                    # the impulse train: held under the ceiling, below target
            want = np.float32(cap / peak_in[b])
            assert abs(gain - want) <= np.spacing(want), (gain, want)
    assert np.isinf(lufs_in[[3, 4]]).all() and np.isfinite(lufs_in[:3]).all()
    conftest.record(worst_db, "gain_db_abs_err")
    # without a ceiling the impulse train reaches the target too; oversample=1 caps on the sample peak
    y2, info2 = L.normalize_loudness(xg, fs, target, None, lens=lens)
    assert abs(float(m.measure(y2, lens)[2]) - target) <= 2e-3
    y3, info3 = L.normalize_loudness(xg, fs, target, ceiling, lens=lens, oversample=1)
    assert torch.equal(info3["peak_in"], m.peak(xg, lens, 1)) and float(m.peak(y3, lens, 1)[2]) <= cap * (1.0 + 2.0 ** -23)
    one, info1 = L.normalize_loudness(xg[1, :lens[1]], fs, target, ceiling)                              # 1-D: a batch of one
    assert one.shape == (lens[1],) and torch.equal(one, y[1, :lens[1]]) and torch.equal(info1["gain_db"], info["gain_db"][1:2])


def test_chain_in_a_replayed_graph():
    """measure -> oversample -> peak -> gain captured once (nothing in it copies from or waits for the host), replayed on two inputs
    written into the same buffers: the eager results, bitwise"""
    fs, x, lens = _normalise_batch()
    m = L.meter(fs, DEV)
    inputs = [torch.from_numpy(x).to(DEV), torch.from_numpy(np.ascontiguousarray(x[::-1] * np.float32(0.5))).to(DEV)]
    lens_in = [torch.tensor(lens, dtype=torch.int32, device=DEV), torch.tensor(lens[::-1], dtype=torch.int32, device=DEV)]
    eager = [m.normalize(xi, -14.0, -1.0, lens=li) for xi, li in zip(inputs, lens_in)]
    sx, sl = torch.zeros_like(inputs[0]), torch.zeros_like(lens_in[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gy, ginfo = m.normalize(sx, -14.0, -1.0, lens=sl)
    for xi, li, (ey, einfo) in zip(inputs, lens_in, eager):
        sx.copy_(xi)
        sl.copy_(li)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gy, ey)
        for k in ("lufs_in", "gain_db", "peak_in"):
            assert torch.equal(ginfo[k], einfo[k]), k


def test_bad_arguments():
    from audioldm_with_lora_amd import _lib, ops
    from audioldm_with_lora_amd._lib import AldmError
    x = torch.zeros(2, 8000, device=DEV)
    with pytest.raises(ValueError):
        L.integrated_loudness(x, 11025)
    with pytest.raises(ValueError):
        L.integrated_loudness(x, 4000)
    with pytest.raises(ValueError):
        L.integrated_loudness(x, 16000, lens=[8001, 1])
    with pytest.raises(AldmError):
        L.normalize_loudness(x.cpu(), 16000)
    m = L.meter(16000, DEV)
    lib, p = _lib.load(), ops._p
    assert lib.aldm_loudness_chunk() == L.CHUNK
    lens = torch.tensor([8000, 8000], dtype=torch.int32, device=DEV)
    e = torch.zeros(2, 5, dtype=torch.float64, device=DEV)
    ws = torch.zeros(lib.aldm_kweight_energy_workspace_doubles(2, 8000), dtype=torch.float64, device=DEV)
    good = [p(x), p(lens), 2, 8000, 1600, p(m.coef), p(m.mpow), L.CHUNK, p(ws), p(e), None]
    for pos, bad in ((0, None), (1, None), (5, None), (6, None), (8, None), (9, None), (2, 0), (3, 0), (4, 799), (7, 512)):
        args = list(good)
        args[pos] = bad
        assert lib.aldm_kweight_energy(*args) == -1, (pos, bad)
        assert b"kweight_energy" in lib.aldm_last_error()
    assert lib.aldm_kweight_energy(*good) == 0
    assert lib.aldm_loudness_gate(p(e), None, 2, 8000, 1600, p(e), None) == -1
    assert lib.aldm_peak_abs(p(x), p(lens), 2, 8000, 0, 1, p(x), None) == -1
    assert lib.aldm_loudness_gain(p(x), p(lens), 2, 8000, p(e), None, -14.0, -1.0, 1, p(x), p(e), p(x), None) == -1
    torch.cuda.synchronize()


# ---- pipelines ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_pipe():
    from test_gpu_audio2audio import _tiny
    return _tiny()[0]


def _check_delivery(out, base, rate, target, ceiling=-1.0):
    """out: the normalised call, base: the same call without the option (both output_type="pt")"""
    cap = 10.0 ** (ceiling / 20.0)
    assert out.sampling_rate == base.sampling_rate == rate and out.audios.shape == base.audios.shape
    assert set(out.loudness) == {"lufs_in", "gain_db", "peak_in"}
    assert getattr(base, "loudness", "missing") is None
    m = L.meter(rate, DEV)
    after, peak = m.measure(out.audios).cpu().numpy(), m.peak(out.audios, None, 4).cpu().numpy()
    assert torch.equal(out.loudness["lufs_in"], m.measure(base.audios))      # measured at the delivered rate
    for b in range(out.audios.shape[0]):
        print(f"clip {b} at {rate} Hz: {float(out.loudness['lufs_in'][b]):.3f} LUFS in, {after[b]:.4f} out, peak {peak[b]:.4f}")
        # on target, or held at the ceiling (the peak of gain x through the 21-tap interpolator, (21 + 2) fp32 roundings off gain * peak)
        assert abs(after[b] - target) <= 2e-3 or abs(peak[b] - cap) <= cap * 23 * 2.0 ** -24, (b, after[b], peak[b])
        assert peak[b] <= cap * (1.0 + 2.0 ** -23)
        i = int(base.audios[b].abs().argmax())
        ratio_db = 20.0 * np.log10(float(out.audios[b, i].double() / base.audios[b, i].double()))
        assert abs(float(out.loudness["gain_db"][b]) - ratio_db) <= 1e-4, (b, ratio_db)


def test_pipeline_loudness(tiny_pipe):
    from test_gpu_audio2audio import _inputs
    pipe = tiny_pipe
    pe, ne, _ = _inputs()
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio_length_in_s=0.64, num_inference_steps=4, guidance_scale=2.5, output_type="pt")
    gen = lambda: torch.Generator().manual_seed(11)  # noqa: E731
    base = pipe(generator=gen(), **call)
    same = pipe(generator=gen(), loudness_lufs=None, **call)
    assert torch.equal(base.audios, same.audios) and same.loudness is None
    _check_delivery(pipe(generator=gen(), loudness_lufs=-16.0, **call), base, 16000, -16.0)
    base48 = pipe(generator=gen(), output_sampling_rate=48000, **call)
    _check_delivery(pipe(generator=gen(), output_sampling_rate=48000, loudness_lufs=-16.0, **call), base48, 48000, -16.0)
    as_np = pipe(generator=gen(), loudness_lufs=-16.0, **dict(call, output_type="np"))
    assert isinstance(as_np.audios, np.ndarray) and as_np.loudness["gain_db"].is_cuda
    with pytest.raises(ValueError):
        pipe(generator=gen(), loudness_lufs=-16.0, output_sampling_rate=11025, **call)


def test_audio_to_audio_and_windowed_loudness(tiny_pipe):
    from test_gpu_audio2audio import _a2a, _inputs
    a2a = _a2a(tiny_pipe)
    pe, ne, audio = _inputs()
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio=audio, strength=0.5, num_inference_steps=4, guidance_scale=2.5, output_type="pt")
    gen = lambda: torch.Generator().manual_seed(12)  # noqa: E731
    base = a2a(generator=gen(), **call)
    _check_delivery(a2a(generator=gen(), loudness_lufs=-16.0, **call), base, 16000, -16.0)
    with pytest.raises(ValueError):
        a2a(generator=gen(), loudness_lufs=-16.0, **dict(call, output_type="latent"))
    pe1, ne1, _ = _inputs(B=1)
    wcall = dict(prompt_embeds=pe1, negative_prompt_embeds=ne1, audio_length_in_s=2.88, window_length_in_s=1.28, window_overlap_in_s=0.32,
                 num_inference_steps=4, guidance_scale=2.5, output_type="pt")
    wbase = tiny_pipe(generator=gen(), **wcall)
    wout = tiny_pipe(generator=gen(), loudness_lufs=-16.0, **wcall)
    assert wout.plan.K > 1 and wbase.loudness is None
    _check_delivery(wout, wbase, 16000, -16.0)


# ---- scripts --------------------------------------------------------------------------------------------------------------------
def test_inference_script_loudness(tmp_path):
    from scipy.io import wavfile
    import synth_checkpoint
    from audioldm_with_lora_amd.script import inference
    root = str(tmp_path / "m")
    synth_checkpoint.write_model_dir(root)
    out = str(tmp_path / "out.wav")
    inference.main(["--model-dir", root, "--no-lora", "--steps", "4", "--guidance-scale", "2.5", "--audio-length", "1.28", "--output", out,
                    "--seed", "1", "--loudness", "-14", "--peak-ceiling", "12"])
    sr, wav = wavfile.read(out)
    assert sr == 16000 and wav.shape == (20480,)
    got = LR.integrated(np.asarray(wav, dtype=np.float64), sr)
    print(f"the written file reads {got:.4f} LUFS")
    assert abs(got - (-14.0)) <= 0.01
    with pytest.raises(SystemExit):
        inference.parse_args(["--model-dir", root, "--peak-ceiling", "-1"])


def test_evaluate_script_normalizes_both_folders(tmp_path, capsys):
    """Scaling one folder by 0.1 moves the CLAP score and KAD; with --normalize-loudness the folder and its scaled copy give the same
    numbers, within ten times what two runs of the same un-normalised pair differ by (and never less than the CLAP rows' bf16 step,
    2^-8: the scaled copy's samples differ from the original's in their last fp32 bit after normalisation)."""
    import conftest
    from scipy.io import wavfile
    import clap_audio_weights as W
    from test_clap_audio_host import write_clap_dir
    from audioldm_with_lora_amd.script import evaluate
    gold = np.load(os.path.join(HERE, "golden", "clap_audio.npz"))
    clap_dir = str(tmp_path / "clap")
    write_clap_dir(clap_dir, "fused")
    clips = W.clips16k()
    for sub in ("gen", "gen_quiet", "ref"):
        os.makedirs(tmp_path / sub)
    for i in (0, 1):
        wavfile.write(str(tmp_path / "gen" / f"clip{i}.wav"), 16000, clips[i])
        wavfile.write(str(tmp_path / "gen_quiet" / f"clip{i}.wav"), 16000, (clips[i] * np.float32(0.1)).astype(np.float32))
    for i in (2, 3):
        wavfile.write(str(tmp_path / "ref" / f"clip{i}.wav"), 16000, clips[i])
    prompt = ",".join(str(int(t)) for t in gold["prompt_ids"])

    def run(gen, *extra):
        res = evaluate.main(["--clap-dir", clap_dir, "--gen-dir", str(tmp_path / gen), "--ref-dir", str(tmp_path / "ref"),
                             "--prompt", prompt, "--batch", "2", *extra])
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
        return res

    def distance(a, b):
        return max(abs(a["clap_score_mean"] - b["clap_score_mean"]), abs(a["kad"] - b["kad"]))

    plain, again, quiet = run("gen"), run("gen"), run("gen_quiet")
    assert "loudness" not in plain
    run_to_run = distance(plain, again)
    conftest.record(run_to_run, "clap_run_to_run")
    tol = max(10.0 * run_to_run, 2.0 ** -8)
    moved = distance(plain, quiet)
    conftest.record(moved, "moved_by_scaling")
    norm, norm_quiet = run("gen", "--normalize-loudness", "-23"), run("gen_quiet", "--normalize-loudness", "-23")
    apart = distance(norm, norm_quiet)
    conftest.record(apart, "apart_once_normalised")
    print(f"run to run {run_to_run:.3e}, moved by the 0.1 scale {moved:.3e}, apart once normalised {apart:.3e}")
    assert moved > tol
    assert apart <= tol
    for res, shift in ((norm, 0.0), (norm_quiet, -20.0)):
        ld = res["loudness"]
        assert ld["target_lufs"] == -23.0 and set(ld["gen"]) >= {"mean", "std", "min", "max", "n_unmeasured"}
        want = np.mean([LR.integrated(clips[i].astype(np.float64), 16000) for i in (0, 1)]) + shift
        assert abs(ld["gen"]["mean"] - want) <= 2e-3
        assert abs(ld["ref"]["mean"] - np.mean([LR.integrated(clips[i].astype(np.float64), 16000) for i in (2, 3)])) <= 2e-3
