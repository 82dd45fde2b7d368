"""CPU side of the CLAP audio tower: the golden fixture, the host tables (mel banks, resampler taps), the KAD / median
statistics against a transcription of both reference variants, checkpoint key mapping, and the unsupported options."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLDEN = os.path.join(HERE, "golden", "clap_audio.npz")
GOLDEN_MIXED = os.path.join(HERE, "golden", "clap_audio_mixed.npz")


def test_fixture_exists_and_is_small():
    assert os.path.isfile(GOLDEN) and os.path.getsize(GOLDEN) < 1024 * 1024


def test_fixture_regenerates_from_transformers():
    pytest.importorskip("transformers")
    pytest.importorskip("scipy")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden_clap_audio as mk
    new = mk.build()
    old = np.load(GOLDEN)
    assert sorted(new) == sorted(old.files)
    for k in old.files:
        if old[k].dtype.kind in "bi":
            np.testing.assert_array_equal(new[k], old[k], err_msg=k)
        else:
            np.testing.assert_allclose(new[k], old[k], rtol=1e-4, atol=1e-4, err_msg=k)
    new, old = mk.build_mixed(), np.load(GOLDEN_MIXED)
    assert sorted(new) == sorted(old.files) and os.path.getsize(GOLDEN_MIXED) < 1024 * 1024
    for k in old.files:
        if old[k].dtype.kind in "bi":
            np.testing.assert_array_equal(new[k], old[k], err_msg=k)
        else:
            np.testing.assert_allclose(new[k], old[k], rtol=1e-4, atol=1e-4, err_msg=k)
    assert old["is_longer"].tolist() == [True, False, True] and old["audio_embeds"].shape == (3, 512)


@pytest.mark.parametrize("norm,scale,fmin,fmax", [(None, "htk", 0, 14000), ("slaney", "slaney", 0, 14000), (None, "htk", 50, 12000)])
def test_mel_banks_match_transformers(norm, scale, fmin, fmax):
    au = pytest.importorskip("transformers.audio_utils")
    from audioldm_with_lora_amd.clap_audio import mel_filter_bank
    want = au.mel_filter_bank(num_frequency_bins=513, num_mel_filters=64, min_frequency=fmin, max_frequency=fmax,
                              sampling_rate=48000, norm=norm, mel_scale=scale)
    np.testing.assert_allclose(mel_filter_bank(513, 64, fmin, fmax, 48000, norm=norm, mel_scale=scale), want, rtol=1e-10, atol=1e-12)


def test_resample_taps_match_scipy():
    sig = pytest.importorskip("scipy.signal")
    from audioldm_with_lora_amd.clap_audio import resample_taps
    h = resample_taps(3)
    assert h.shape == (61,)
    np.testing.assert_allclose(h, sig.firwin(61, 1 / 3, window=("kaiser", 5.0)) * 3, rtol=1e-12, atol=1e-15)
    # the index arithmetic the kernel uses, on the host, against resample_poly itself
    x = np.random.RandomState(0).randn(200)
    y = np.array([sum(x[j] * h[n + 30 - 3 * j] for j in range(200) if 0 <= n + 30 - 3 * j < 61) for n in range(600)])
    np.testing.assert_allclose(y, sig.resample_poly(x, 3, 1), rtol=1e-10, atol=1e-12)


def test_periodic_hann_matches_transformers():
    au = pytest.importorskip("transformers.audio_utils")
    np.testing.assert_allclose(np.hanning(1025)[:-1], au.window_function(1024, "hann"), atol=1e-15)


# ---- the reference's statistics, transcribed in torch (train_audioldm_lora.py:247-294, inference.py:19-53) -------------------
def _ref_median(x):
    return torch.median(torch.pdist(torch.as_tensor(np.asarray(x), dtype=torch.float32))).item()


def _ref_kad(x, y, bandwidth=None, kernel="gaussian", eps=1e-8, scale=1.0):
    x, y = torch.as_tensor(np.asarray(x), dtype=torch.float32), torch.as_tensor(np.asarray(y), dtype=torch.float32)
    if bandwidth is None:
        bandwidth = _ref_median(y)
        if bandwidth < 1e-6 or np.isnan(bandwidth):
            bandwidth = 1.0
    gamma = 1 / (2 * bandwidth ** 2 + eps)
    k = {"gaussian": lambda a: torch.exp(-gamma * a), "iq": lambda a: 1 / (1 + gamma * a),
         "imq": lambda a: 1 / torch.sqrt(1 + gamma * a)}[kernel]
    xx = x @ x.T
    xs = torch.diagonal(xx)
    kxx = k(xs[:, None] + xs[None, :] - 2 * xx)
    kxx = kxx - torch.diag(torch.diagonal(kxx))
    yy = y @ y.T
    ys = torch.diagonal(yy)
    kyy = k(ys[:, None] + ys[None, :] - 2 * yy)
    kyy = kyy - torch.diag(torch.diagonal(kyy))
    kxy = k(xs[:, None] + ys[None, :] - 2 * x @ y.T)
    r = kxx.sum() / (x.shape[0] * (x.shape[0] - 1)) + kyy.sum() / (y.shape[0] * (y.shape[0] - 1)) - 2 * kxy.mean()
    return float(r) * scale


def _emb(n, seed, shift=0.0):
    e = np.random.RandomState(seed).randn(n, 512) + shift
    return e / np.linalg.norm(e, axis=1, keepdims=True)


@pytest.mark.parametrize("n", [2, 5, 8])
def test_median_pairwise_distance_matches_reference(n):
    from audioldm_with_lora_amd.metrics import median_pairwise_distance
    x = _emb(n, n)
    assert abs(median_pairwise_distance(x) - _ref_median(x)) < 1e-5


@pytest.mark.parametrize("kernel", ["gaussian", "iq", "imq"])
def test_kad_training_variant(kernel):
    from audioldm_with_lora_amd.metrics import kernel_audio_distance
    ref, gen = _emb(6, 1), _emb(5, 2, shift=0.05)
    want = _ref_kad(ref, gen, kernel=kernel, scale=100.0)            # calc_kernel_audio_distance(ref, gen) * SCALE_FACTOR
    assert abs(kernel_audio_distance(ref, gen, kernel=kernel, scale=100.0) - want) < 1e-3 * max(1.0, abs(want))


def test_kad_inference_variant():
    from audioldm_with_lora_amd.metrics import kernel_audio_distance
    gen, ref = _emb(4, 3, shift=0.1), _emb(7, 4)
    want = _ref_kad(gen, ref, bandwidth=1)
    assert abs(kernel_audio_distance(gen, ref, bandwidth=1.0) - want) < 1e-5
    assert abs(kernel_audio_distance(ref, ref, bandwidth=1.0) - _ref_kad(ref, ref, bandwidth=1)) < 1e-5


def test_kad_rejects_unknown_kernel():
    from audioldm_with_lora_amd.metrics import kernel_audio_distance
    with pytest.raises(ValueError):
        kernel_audio_distance(_emb(3, 0), _emb(3, 1), kernel="laplace")


# ---- checkpoint loading ----------------------------------------------------------------------------------------------------------
def write_clap_dir(d, audio="fused"):
    """A laion/clap-htsat-* style directory with the recipe's weights: config.json (text_config / audio_config),
    model.safetensors with transformers' ClapModel key names, preprocessor_config.json."""
    from safetensors.torch import save_file
    import clap_audio_weights as W
    os.makedirs(d, exist_ok=True)
    sd = dict(W.audio_state_dict(audio))
    sd.update(W.text_state_dict())
    sd["logit_scale_a"] = torch.tensor(np.log(10.0), dtype=torch.float32)
    sd["logit_scale_t"] = torch.tensor(np.log(1 / 0.07), dtype=torch.float32)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(d, "model.safetensors"))
    cfg = {"model_type": "clap", "projection_dim": 512, "text_config": dict(W.TEXT), "audio_config": W.audio_config(audio)}
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    json.dump({"feature_extractor_type": "ClapFeatureExtractor", "frequency_min": 0, "frequency_max": 14000, "hop_length": 480,
               "truncation": "fusion" if W.CONFIGS[audio]["enable_fusion"] else "rand_trunc"},
              open(os.path.join(d, "preprocessor_config.json"), "w"))
    return sd


@pytest.mark.parametrize("audio", ["fused", "unfused"])
def test_from_pretrained_maps_every_key(tmp_path, audio):
    from audioldm_with_lora_amd.clap_audio import ClapModel
    sd = write_clap_dir(str(tmp_path), audio)
    m = ClapModel.from_pretrained(str(tmp_path))
    got = {("audio." + k): v for k, v in m.audio.state_dict().items()}
    got.update({("text." + k): v for k, v in m.text.state_dict().items()})
    for k, v in sd.items():
        if k.endswith(("position_ids", "token_type_ids")):
            continue
        if k.startswith("logit_scale"):
            assert torch.equal(getattr(m, k).detach(), v), k
            continue
        pre = "audio." if k.startswith("audio_") else "text."
        assert torch.equal(got[pre + k], v), k
    assert abs(float(m.logit_scale_a.detach()) - np.log(10.0)) < 1e-6
    assert m.front_end_config["truncation"] == ("fusion" if audio == "fused" else "rand_trunc")


def test_from_pretrained_rejects_unknown_keys(tmp_path):
    from safetensors.torch import load_file, save_file
    from audioldm_with_lora_amd.clap_audio import ClapModel
    write_clap_dir(str(tmp_path))
    f = os.path.join(str(tmp_path), "model.safetensors")
    sd = load_file(f)
    sd["audio_model.audio_encoder.extra.weight"] = torch.zeros(3)
    save_file(sd, f)
    with pytest.raises((KeyError, RuntimeError)):
        ClapModel.from_pretrained(str(tmp_path))


def test_hub_id_raises():
    from audioldm_with_lora_amd.clap_audio import ClapModel
    with pytest.raises(FileNotFoundError):
        ClapModel.from_pretrained("laion/clap-htsat-fused")


# ---- unsupported options / no CPU fallback ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("over,word", [(dict(enable_fusion=True, fusion_type="channel_map"), "fusion_type"),
                                       (dict(spec_size=512), "spec_size"), (dict(window_size=16), "window_size"),
                                       (dict(num_attention_heads=[3, 6, 12, 24]), "head dim")])
def test_unsupported_options_raise(over, word):
    from audioldm_with_lora_amd.clap_audio import ClapAudioModelWithProjection
    with pytest.raises(NotImplementedError, match=word):
        ClapAudioModelWithProjection(**over)


def test_no_cpu_fallback():
    from audioldm_with_lora_amd._lib import AldmError
    from audioldm_with_lora_amd.clap_audio import ClapAudioModelWithProjection
    m = ClapAudioModelWithProjection(enable_fusion=True, fusion_type="aff_2d")
    with pytest.raises(AldmError):
        m(torch.zeros(1, 4, 1001, 64), torch.ones(1, 1, dtype=torch.bool))
    with pytest.raises(AldmError):
        m.plan()


def test_front_end_options():
    from audioldm_with_lora_amd.clap_audio import ClapAudioFrontEnd
    with pytest.raises(NotImplementedError, match="padding"):
        ClapAudioFrontEnd("cpu", padding="pad")
    with pytest.raises(NotImplementedError, match="truncation"):
        ClapAudioFrontEnd("cpu", truncation="channel_map")
    from audioldm_with_lora_amd._lib import AldmError
    with pytest.raises(AldmError):
        ClapAudioFrontEnd("cpu")(torch.zeros(1, 16000), sampling_rate=16000)
