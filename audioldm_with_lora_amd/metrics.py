"""CLAP score and kernel audio distance (KAD) over CLAP audio embeddings.

Embedding is the only GPU work (ClapModel on the HIP kernels); the statistics below are host numpy float64 over the
[n, 512] embeddings, which the reference L2-normalises first [REF script/train/train_audioldm_lora.py:131-141, 304-316].

Two KAD variants exist in the reference, and both are kept:
  training   calc_kernel_audio_distance(ref, gen): bandwidth = median pairwise distance of `y` = gen, result * 100
             [REF script/train/train_audioldm_lora.py:71, 247-294]  ->  kernel_audio_distance(ref, gen, scale=100.0)
  inference  calc_kernel_audio_distance(gen, ref, bandwidth=1), no scale  [REF script/inference/inference.py:22-76]
             ->  kernel_audio_distance(gen, ref, bandwidth=1.0)
"""
import numpy as np
import torch


def _normalize(e):
    e = np.asarray(e, dtype=np.float64)
    return e / np.maximum(np.linalg.norm(e, axis=-1, keepdims=True), 1e-12)     # F.normalize(eps=1e-12)


def median_pairwise_distance(x):
    """Median of the n (n - 1) / 2 Euclidean distances between the rows of x (torch.median of torch.pdist: the lower median)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    i, j = np.triu_indices(n, k=1)
    d = np.sqrt(((x[i] - x[j]) ** 2).sum(1))
    return float(np.sort(d)[(d.size - 1) // 2])


def kernel_audio_distance(x, y, bandwidth=None, kernel="gaussian", scale=1.0, eps=1e-8):
    """Unbiased MMD^2 of x [n, d] and y [m, d] under a Gaussian / inverse-quadratic / inverse-multiquadric kernel, times
    `scale`.  bandwidth None: the median pairwise distance of y (1.0 if that is < 1e-6 or NaN)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if bandwidth is None:
        bandwidth = median_pairwise_distance(y)
        if bandwidth < 1e-6 or np.isnan(bandwidth):
            bandwidth = 1.0
    gamma = 1.0 / (2.0 * bandwidth ** 2 + eps)
    if kernel == "gaussian":
        k = lambda a: np.exp(-gamma * a)
    elif kernel == "iq":
        k = lambda a: 1.0 / (1.0 + gamma * a)
    elif kernel == "imq":
        k = lambda a: 1.0 / np.sqrt(1.0 + gamma * a)
    else:
        raise ValueError(f"kernel must be gaussian / iq / imq, got {kernel!r}")

    def d2(a, b):
        return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T

    n, m = x.shape[0], y.shape[0]
    kxx = k(d2(x, x))
    kyy = k(d2(y, y))
    kxy = k(d2(x, y))
    kxx_mean = (kxx.sum() - np.trace(kxx)) / (n * (n - 1))
    kyy_mean = (kyy.sum() - np.trace(kyy)) / (m * (m - 1))
    return float((kxx_mean + kyy_mean - 2.0 * kxy.mean()) * scale)


def embed_audio(audios_16k, clap, front_end=None, batch=8):
    """16 kHz clips (1-D tensors / arrays, any device, <= 10 s) -> L2-normalised CLAP audio embeddings, float64 [n, d]."""
    dev = clap.audio.audio_model.audio_encoder.norm.weight.device
    fe = front_end or clap.front_end(dev)
    out = []
    for i in range(0, len(audios_16k), batch):
        clips = [torch.as_tensor(np.asarray(a, dtype=np.float32) if not isinstance(a, torch.Tensor) else a).to(dev, torch.float32)
                 for a in audios_16k[i:i + batch]]
        f = fe(clips, sampling_rate=16000)
        out.append(clap.get_audio_features(f.input_features, f.is_longer).double().cpu().numpy())
    return _normalize(np.concatenate(out))


def embed_text(text, clap):
    """A prompt (str: needs clap.tokenizer) or its input_ids -> the L2-normalised CLAP text embedding, float64 [1, d]."""
    dev = clap.text.text_model.pooler.dense.weight.device
    if isinstance(text, str):
        if clap.tokenizer is None:
            raise ValueError("clap has no tokenizer (no tokenizer files in its directory): pass input_ids instead of a string")
        tok = clap.tokenizer(text, return_tensors="pt", padding=True)
        ids, mask = tok["input_ids"], tok["attention_mask"]
    else:
        ids = torch.as_tensor(text).reshape(1, -1)
        mask = torch.ones_like(ids)
    L = ids.shape[1]
    Lp = (L + 7) // 8 * 8                          # the text tower's attention takes key lengths in 8-token granules
    if Lp != L:                                    # right-pad with the pad token; the mask keeps the padding out of every key
        pad = clap.text.cfg["pad_token_id"]
        ids = torch.cat([ids, torch.full((1, Lp - L), pad, dtype=ids.dtype)], 1)
        mask = torch.cat([mask, torch.zeros(1, Lp - L, dtype=mask.dtype)], 1)
    return _normalize(clap.get_text_features(ids.to(dev), mask.to(dev)).double().cpu().numpy())


def clap_score(audios_16k, text, clap, front_end=None, batch=8):
    """(cos(audio, text) + 1) / 2 per clip, float64 [n]  [REF script/train/train_audioldm_lora.py:131-141]."""
    a = embed_audio(audios_16k, clap, front_end, batch)
    t = embed_text(text, clap)
    return (a @ t[0] + 1.0) / 2.0
