"""GPU: the polyphase resampler (csrc/resample.hip, resample.py) -- every output against the float64 restatement at the derived fp32
bound, the 64-bit index case, agreement with the CLAP front end's 3 : 1 kernel, ragged batches, determinism, and the resampler
inside the pipelines and the scripts."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import resample_restatement as RR  # noqa: E402
from audioldm_with_lora_amd import resample as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t_in_for(n_out, up, down):
    """an input length whose output length ceil(T up / down) is exactly n_out, or None when no length gives it"""
    T = n_out * down // up
    for t in (T, T + 1):
        if t >= 1 and R.output_length(t, up, down) == n_out:
            return t
    return None


def _check(got, x, up, down, idx=None, length=None, factor=1.0):
    """got: the kernel's outputs at idx (all when None) -> the worst |error| / bound; asserts the bound at every one of them"""
    want, S, Kn = RR.restate(x, up, down, idx=idx, length=length)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape
    err, lim = np.abs(got - want), RR.bound(S, Kn, factor)
    worst = int(np.argmax(err / lim))
    assert (err <= lim).all(), (up, down, len(x), worst, err[worst], lim[worst])
    return float(err[worst] / lim[worst])


@pytest.mark.parametrize("rate_in,rate_out,T", RR.PAIRS)
def test_parity_with_restatement(rate_in, rate_out, T):
    """Every output of the listed length, of T_in = 1 and 7 (shorter than the filter: both ends of the sum clipped at once), and of
    the lengths of 512 / 513 and 1024 / 1025 outputs -- the last two end exactly on and one past the edge of a workgroup's run of
    1024 -- where the ratio reaches them (an interpolating ratio skips output lengths), and in any case of the longest input that
    still fits one workgroup's run and the next longer one.  Bound per output: (Kn + 2) 2^-24 S[n] + 1e-30 (resample_restatement.py)."""
    import conftest
    from audioldm_with_lora_amd import ops
    up, down = R.ratio(rate_in, rate_out)
    edges = [t for t in (_t_in_for(n, up, down) for n in (512, 513, 1024, 1025)) if t is not None]
    assert edges, (up, down)
    if down > up:
        assert len(edges) == 4                                      # a decimating ratio reaches every output length
    t_one = 1024 * down // up
    assert R.output_length(t_one, up, down) <= 1024 < R.output_length(t_one + 1, up, down)
    edges = sorted(set(edges) | {t_one, t_one + 1})
    worst = 0.0
    for i, t_in in enumerate([T, 1, 7] + edges):
        x = RR.clip(t_in, 100 + i)
        y, out_lens = ops.resample_poly(torch.from_numpy(x)[None].to(DEV), up, down)
        n_out = R.output_length(t_in, up, down)
        assert y.shape == (1, n_out) and y.dtype == torch.float32 and out_lens.tolist() == [n_out]
        worst = max(worst, _check(y[0].cpu().numpy(), x, up, down))
        r = R.Resampler(rate_in, rate_out, DEV)
        assert torch.equal(r(torch.from_numpy(x).to(DEV)), y[0]) and torch.equal(R.resample(torch.from_numpy(x)[None].to(DEV), rate_in, rate_out), y)
    conftest.record(worst, "max_err_over_bound")


@pytest.mark.parametrize("up,down,T", [(3, 50, 30011), (1, 2048, 300 * 2048 + 5), (1280, 147, 301)])
def test_ratios_beyond_the_staged_forms(up, down, T):
    """the kernel's other two forms: an input span too long for LDS (down / up > 15: everything read from global memory) and a phase
    table too large for it (up > ~700: only the input staged); same definition, same bound, every output"""
    import conftest
    from audioldm_with_lora_amd import ops
    x = RR.clip(T, 120)
    y, out_lens = ops.resample_poly(torch.from_numpy(x)[None].to(DEV), up, down)
    assert y.shape == (1, R.output_length(T, up, down)) and out_lens.tolist() == [y.shape[1]]
    conftest.record(_check(y[0].cpu().numpy(), x, up, down), "max_err_over_bound")


def test_indices_past_2_pow_31():
    """1999 : 2000 on 1.1 M samples: the last output's n down + half is 2 198 918 000 > 2^31.  The last 512 outputs and 512 seeded
    random ones against the restatement (Python integers) at the same bound."""
    import conftest
    from audioldm_with_lora_amd import ops
    T, up, down = 1_100_000, 1999, 2000
    x = RR.clip(T, 5)
    n_out = R.output_length(T, up, down)
    assert (n_out - 1) * down + 10 * down == 2_198_918_000 > 2 ** 31
    y, out_lens = ops.resample_poly(torch.from_numpy(x)[None].to(DEV), up, down)
    assert y.shape == (1, n_out) and out_lens.tolist() == [n_out]
    idx = np.concatenate([np.arange(n_out - 512, n_out), np.sort(np.random.default_rng(6).choice(n_out - 512, 512, replace=False))])
    got = y[0].cpu().numpy()
    assert np.isfinite(got).all()
    conftest.record(_check(got[idx], x, up, down, idx=idx), "max_err_over_bound")


def test_agrees_with_the_clap_front_end_kernel():
    """ops.resample_poly(x, 3, 1) and ClapAudioFrontEnd.resample_16k_to_48k both meet the bound against the exact value, so they
    agree within twice the bound."""
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.clap_audio import ClapAudioFrontEnd
    x = RR.clip(1001, 103)
    xg = torch.from_numpy(x)[None].to(DEV)
    y, _ = ops.resample_poly(xg, 3, 1)
    z, lens = ClapAudioFrontEnd(DEV).resample_16k_to_48k(xg, torch.tensor([x.shape[0]], dtype=torch.int32))
    assert y.shape == z.shape and int(lens[0]) == y.shape[1]
    _, S, Kn = RR.restate(x, 3, 1)
    assert (np.abs(y[0].double().cpu().numpy() - z[0].double().cpu().numpy()) <= RR.bound(S, Kn, 2.0)).all()
    _check(z[0].cpu().numpy(), x, 3, 1)


def test_ragged_batch_rows_are_independent():
    from audioldm_with_lora_amd import ops
    up, down = R.ratio(44100, 16000)
    lens = (5003, 1, 2500)
    x = torch.from_numpy(np.stack([RR.clip(5003, 200 + b) for b in range(3)])).to(DEV)       # (samples behind lens[b] are junk)
    y, out_lens = ops.resample_poly(x, up, down, lens=torch.tensor(lens))
    n_out = R.output_length(5003, up, down)
    assert y.shape == (3, n_out) and out_lens.dtype == torch.int32
    assert out_lens.tolist() == [R.output_length(n, up, down) for n in lens] == [1816, 1, 908]
    for b, n in enumerate(lens):
        alone, _ = ops.resample_poly(x[b:b + 1, :n].contiguous(), up, down)
        m = int(out_lens[b])
        assert alone.shape == (1, m) and torch.equal(y[b, :m], alone[0])
        assert not y[b, m:].any()
        _check(y[b, :m].cpu().numpy(), x[b].cpu().numpy(), up, down, length=n)
    via, via_lens = R.Resampler(44100, 16000, DEV)(x, lens)
    assert torch.equal(via, y) and via_lens.tolist() == out_lens.tolist()


def test_two_calls_bitwise_equal():
    from audioldm_with_lora_amd import ops
    x = torch.from_numpy(np.stack([RR.clip(5003, 300), RR.clip(5003, 301)])).to(DEV)
    for up, down in ((160, 441), (441, 160)):
        a, _ = ops.resample_poly(x, up, down)
        b, _ = ops.resample_poly(x, up, down)
        assert torch.equal(a, b)


def test_c_abi_rejects_bad_arguments():
    from audioldm_with_lora_amd import _lib
    from audioldm_with_lora_amd._lib import AldmError
    from audioldm_with_lora_amd import ops
    x = torch.zeros(1, 100, device=DEV)
    with pytest.raises(ValueError):
        ops.resample_poly(x, 2049, 1)
    with pytest.raises(ValueError):
        ops.resample_poly(x, 3, 1, table=torch.zeros(3, 20, device=DEV))
    with pytest.raises(AldmError):
        ops.resample_poly(x.cpu(), 3, 1)
    lib = _lib.load()
    t, lens, y = R.device_table(3, 1, x.device), torch.tensor([100], dtype=torch.int32, device=DEV), torch.zeros(1, 300, device=DEV)
    p = ops._p
    good = [p(x), p(lens), 1, 100, p(t), 3, 1, 21, 30, p(y), 300, None]
    for pos, bad in ((0, None), (4, None), (9, None), (2, 0), (3, 0), (10, 299), (7, 20), (8, 31), (5, 2049), (6, 0)):
        args = list(good)
        args[pos] = bad
        assert lib.aldm_resample_poly(*args) == -1, (pos, bad)
        assert b"resample_poly" in lib.aldm_last_error()
    assert lib.aldm_resample_poly(*good) == 0
    torch.cuda.synchronize()


# ---- pipelines ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_pipe():
    from test_gpu_audio2audio import _tiny
    return _tiny()[0]


def _recording_44k(n16, B, seed):
    """[B, n44] fp32 on the GPU whose 16 kHz form has exactly n16 samples"""
    up, down = R.ratio(44100, 16000)
    n44 = _t_in_for(n16, up, down)
    return torch.from_numpy(np.stack([RR.clip(n44, seed + b) for b in range(B)])).to(DEV)


def test_audio_to_audio_resamples_the_recording(tiny_pipe):
    from test_gpu_audio2audio import _a2a, _inputs
    a2a = _a2a(tiny_pipe)
    pe, ne, _ = _inputs()
    x44 = _recording_44k(20480, 2, 400)
    x16 = R.resample(x44, 44100, 16000)
    assert x16.shape == (2, 20480)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, strength=0.5, num_inference_steps=4, guidance_scale=2.5, output_type="pt")
    gen = lambda: torch.Generator().manual_seed(9)  # noqa: E731
    got = a2a(audio=x44, sampling_rate=44100, resample=True, generator=gen(), **call)
    want = a2a(audio=x16, sampling_rate=16000, generator=gen(), **call)
    assert got.audios.shape == want.audios.shape == (2, 20480) and torch.equal(got.audios, want.audios)
    assert got.sampling_rate == want.sampling_rate == 16000
    assert torch.equal(a2a(audio=x44.cpu().numpy(), sampling_rate=44100, resample=True, generator=gen(), **call).audios, want.audios)
    with pytest.raises(ValueError, match="resample=True"):
        a2a(audio=x44, sampling_rate=44100, **call)
    with pytest.raises(ValueError):
        a2a(audio=x44, sampling_rate=44100.5, resample=True, **call)
    # the other end: the 16 kHz result leaves at 48 kHz
    out = a2a(audio=x16, generator=gen(), output_sampling_rate=48000, **call)
    assert out.sampling_rate == 48000 and torch.equal(out.audios, R.resample(want.audios, 16000, 48000))
    with pytest.raises(ValueError):
        a2a(audio=x16, output_sampling_rate=48000, **dict(call, output_type="latent"))


def test_windowed_audio_to_audio_resamples_the_recording(tiny_pipe):
    from test_gpu_audio2audio import _a2a, _inputs
    a2a = _a2a(tiny_pipe)
    pe, ne, _ = _inputs(B=1)
    x44 = _recording_44k(46080, 1, 410)                                # 2.88 s: three windows of 1.28 s
    x16 = R.resample(x44, 44100, 16000)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, strength=0.5, num_inference_steps=4, guidance_scale=2.5, output_type="pt",
                window_length_in_s=1.28, window_overlap_in_s=0.32)
    gen = lambda: torch.Generator().manual_seed(10)  # noqa: E731
    got = a2a(audio=x44, sampling_rate=44100, resample=True, generator=gen(), **call)
    want = a2a(audio=x16, sampling_rate=16000, generator=gen(), **call)
    assert got.plan.K > 1 and got.audios.shape == want.audios.shape and abs(got.audios.shape[1] - 46080) <= 1 and torch.equal(got.audios, want.audios)


def test_pipeline_output_sampling_rate(tiny_pipe):
    from test_gpu_audio2audio import _inputs
    pipe = tiny_pipe
    pe, ne, _ = _inputs()
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, audio_length_in_s=0.64, num_inference_steps=4, guidance_scale=2.5)
    gen = lambda: torch.Generator().manual_seed(11)  # noqa: E731
    base = pipe(generator=gen(), output_type="pt", **call)
    n = base.audios.shape[1]
    assert n == 10240 and base.sampling_rate == 16000
    up = pipe(generator=gen(), output_type="pt", output_sampling_rate=48000, **call)
    assert up.sampling_rate == 48000 and up.audios.shape == (2, 3 * n)
    assert torch.equal(up.audios, R.resample(base.audios, 16000, 48000))
    as_np = pipe(generator=gen(), output_sampling_rate=44100, **call)
    assert as_np.sampling_rate == 44100 and isinstance(as_np.audios, np.ndarray) and as_np.audios.shape == (2, -(-n * 441 // 160))
    assert np.array_equal(as_np.audios, R.resample(base.audios, 16000, 44100).cpu().numpy())
    with pytest.raises(ValueError):
        pipe(generator=gen(), output_sampling_rate=0, **call)


# ---- scripts --------------------------------------------------------------------------------------------------------------------
def test_inference_script_resamples_in_and_out(tmp_path, capsys):
    from scipy.io import wavfile
    import synth_checkpoint
    from audioldm_with_lora_amd.script import inference
    root = str(tmp_path / "m")
    synth_checkpoint.write_model_dir(root)
    src, out = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    n_in = 28224                                                        # 1.28 s at 22.05 kHz
    wavfile.write(src, 22050, (0.3 * np.sin(2 * np.pi * 330 * np.arange(n_in) / 22050)).astype(np.float32))
    inference.main(["--model-dir", root, "--no-lora", "--steps", "5", "--guidance-scale", "2.5", "--init-audio", src, "--output", out,
                    "--seed", "1", "--strength", "0.6", "--output-sampling-rate", "44100"])
    assert "22050 Hz -> 16000 Hz" in capsys.readouterr().out
    sr, wav = wavfile.read(out)
    n = int(n_in / 22050.0 * 16000)                                     # the 16 kHz clip the pipeline trims to
    assert n == 20480
    assert sr == 44100 and wav.dtype == np.float32 and wav.shape == (-(-n * 441 // 160),) and np.isfinite(wav).all()


def test_evaluate_script_resamples_a_44k_reference_folder(tmp_path, capsys):
    """a reference folder written at 44.1 kHz gives the JSON of the same clips resampled beforehand with resample() and written at
    16 kHz; the 16 kHz generated folder takes the untouched path in both runs"""
    from scipy.io import wavfile
    import clap_audio_weights as W
    from test_clap_audio_host import write_clap_dir
    from audioldm_with_lora_amd.script import evaluate
    gold = np.load(os.path.join(HERE, "golden", "clap_audio.npz"))
    clap_dir = str(tmp_path / "clap")
    write_clap_dir(clap_dir, "fused")
    clips = W.clips16k()
    for sub in ("gen", "ref44", "ref16"):
        os.makedirs(tmp_path / sub)
    for i in (0, 1):
        wavfile.write(str(tmp_path / "gen" / f"clip{i}.wav"), 16000, clips[i])
    for i in (2, 3):                                                   # the same samples, declared a 44.1 kHz recording
        wavfile.write(str(tmp_path / "ref44" / f"clip{i}.wav"), 44100, clips[i])
        pre = R.resample(torch.from_numpy(clips[i]).to(DEV), 44100, 16000)
        wavfile.write(str(tmp_path / "ref16" / f"clip{i}.wav"), 16000, pre.cpu().numpy())
    prompt = ",".join(str(int(t)) for t in gold["prompt_ids"])
    res = {}
    for ref in ("ref44", "ref16"):
        res[ref] = evaluate.main(["--clap-dir", clap_dir, "--gen-dir", str(tmp_path / "gen"), "--ref-dir", str(tmp_path / ref),
                                  "--prompt", prompt, "--batch", "2"])
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res[ref]
    assert res["ref44"] == res["ref16"] and np.isfinite(res["ref44"]["kad"])
