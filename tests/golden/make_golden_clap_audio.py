"""Regenerates tests/golden/clap_audio.npz from live transformers (ClapFeatureExtractor, ClapAudioModelWithProjection,
ClapModel) and scipy.signal.resample_poly, with the seeded weights and clips of tests/clap_audio_weights.py.

Every clip takes the reference's path: resample_poly(16 kHz -> 48 kHz), then ONE extractor call per clip (so a fused clip is
always is_longer), then the tower.  Stored per config (fused / unfused / narrow): pooler_output and audio_embeds of every
clip; the fused and unfused input_features of clip 0 (one channel); is_longer; the narrow config's patch-embedding output
for the first 512 tokens of clip 0.  Also the resample_poly output of a short clip and the CLAP text embedding of PROMPT_IDS
under the tiny text tower of the recipe.
Run:  python tests/golden/make_golden_clap_audio.py

With --mixed it writes tests/golden/clap_audio_mixed.npz instead: the narrow fused tower on a batch of three whose four mel channels per
item are the extractor's spectrograms of four DIFFERENT clips (clap_audio_weights.MIXED_CLIPS) with is_longer = [True, False, True].
Stored are the clips' (seconds, seed) pairs, is_longer, audio_embeds and pooler_output; the features are rebuilt from the seeds.
Run:  python tests/golden/make_golden_clap_audio.py --mixed
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def build():
    from scipy.signal import resample_poly
    from transformers import ClapAudioConfig, ClapAudioModelWithProjection, ClapFeatureExtractor, ClapTextConfig
    from transformers import ClapTextModelWithProjection
    import clap_audio_weights as W
    torch.manual_seed(0)
    out = {}
    clips = W.clips16k()
    clips48 = [resample_poly(c, 3, 1).astype(np.float32) for c in clips]
    out["resample_in"] = W.wave16k(0.1, 99)
    out["resample_out"] = resample_poly(out["resample_in"], 3, 1).astype(np.float32)
    for name in W.CONFIGS:
        cfg = ClapAudioConfig(**W.audio_config(name))
        m = ClapAudioModelWithProjection(cfg).eval()
        m.load_state_dict(W.audio_state_dict(name), strict=True)
        trunc = "fusion" if cfg.enable_fusion else "rand_trunc"
        fe = ClapFeatureExtractor(truncation=trunc)
        pooled, embeds, longer = [], [], []
        for i, c in enumerate(clips48):
            np.random.seed(0)
            f = fe(c, sampling_rate=48000, return_tensors="pt")
            feats = f["input_features"].float()
            with torch.no_grad():
                o = m(input_features=feats, is_longer=f["is_longer"], output_hidden_states=False)
                po = m.audio_model(input_features=feats, is_longer=f["is_longer"]).pooler_output
            pooled.append(po[0].numpy())
            embeds.append(o.audio_embeds[0].numpy())
            longer.append(bool(f["is_longer"].reshape(-1)[0]))
            if i == 0 and name in ("fused", "unfused"):
                out[f"{name}_input_features"] = feats[0, 0].numpy()
            if i == 0 and name == "narrow":
                enc = m.audio_model.audio_encoder
                with torch.no_grad():
                    x = enc.batch_norm(feats.transpose(1, 3)).transpose(1, 3)
                    pe = enc.patch_embed(enc.reshape_mel2img(x), torch.where(f["is_longer"].reshape(-1))[0])
                out["narrow_patch_embed"] = pe[0, :512].numpy()
        out[f"{name}_pooler_output"] = np.stack(pooled)
        out[f"{name}_audio_embeds"] = np.stack(embeds)
        out[f"{name}_is_longer"] = np.array(longer)
    tm = ClapTextModelWithProjection(ClapTextConfig(**W.TEXT)).eval()
    tm.load_state_dict(W.text_state_dict(), strict=True)
    ids = torch.tensor([W.PROMPT_IDS])
    with torch.no_grad():
        out["text_embeds"] = tm(input_ids=ids, attention_mask=torch.ones_like(ids)).text_embeds[0].numpy()
    out["prompt_ids"] = np.array(W.PROMPT_IDS, dtype=np.int64)
    return out


def build_mixed():
    from scipy.signal import resample_poly
    from transformers import ClapAudioConfig, ClapAudioModelWithProjection, ClapFeatureExtractor
    import clap_audio_weights as W
    torch.manual_seed(0)
    cfg = ClapAudioConfig(**W.audio_config("narrow"))
    m = ClapAudioModelWithProjection(cfg).eval()
    m.load_state_dict(W.audio_state_dict("narrow"), strict=True)
    fe = ClapFeatureExtractor(truncation="fusion")
    chans = []
    for seconds, seed in W.MIXED_CLIPS:
        np.random.seed(0)
        f = fe(resample_poly(W.wave16k(seconds, seed), 3, 1).astype(np.float32), sampling_rate=48000, return_tensors="pt")
        chans.append(f["input_features"].float()[0, 0])                     # a clip of <= 10 s: four identical channels
    feats = torch.stack(chans).reshape(len(W.MIXED_LONGER), 4, 1001, 64)
    longer = torch.tensor(W.MIXED_LONGER)[:, None]
    with torch.no_grad():
        o = m(input_features=feats, is_longer=longer)
        po = m.audio_model(input_features=feats, is_longer=longer).pooler_output
    return {"clips": np.array(W.MIXED_CLIPS, dtype=np.float64), "is_longer": np.array(W.MIXED_LONGER),
            "audio_embeds": o.audio_embeds.numpy(), "pooler_output": po.numpy()}


if __name__ == "__main__":
    mixed = "--mixed" in sys.argv[1:]
    data = build_mixed() if mixed else build()
    path = os.path.join(HERE, "clap_audio_mixed.npz" if mixed else "clap_audio.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
