"""CLAP audio tower, its front end and the two-tower CLAP model on the HIP kernels.

The reference scores a LoRA with the CLAP audio tower of `laion/clap-htsat-fused`: the CLAP score and KAD of
`log_validation` / `compute_clap_kad_from_audio_lists` [REF script/train/train_audioldm_lora.py:97-321] and of
`script/inference/inference.py`.  Each clip goes through `librosa.resample(16 kHz -> 48 kHz)`, then one
`ClapProcessor(audios=clip, sampling_rate=48000)` call, then `ClapModel.get_audio_features`.

  ClapAudioFrontEnd              ClapFeatureExtractor on the device: resample_up3 (16 kHz input only), clap_log_mel
  ClapAudioModelWithProjection   transformers' HTSAT-Swin tower under transformers' parameter names
  ClapModel                      from_pretrained(local dir) -> get_audio_features / get_text_features

Launch sequence of the tower (bf16 rows, fp32 accumulation / statistics), B clips:
    clap_input                     BatchNorm over mel bins + bicubic 1001 -> 1024 frames + reshape_mel2img, as im2col rows
    proj GEMM (K 16)               patch_embed.proj, 4 x 4 / stride 4
    [fused] mel_conv2d GEMM (K 48), aff_sum_pool, 2 + 2 small GEMMs (BatchNorms folded), aff_combine
    LayerNorm                      patch_embed.norm
    per block: LayerNorm -> QKV GEMM -> window_attention -> out GEMM + residual -> LayerNorm -> GEMM + GELU -> GEMM + residual
    per stage 1-3: patch_merge_gather -> LayerNorm(4C) -> reduction GEMM (no bias)
    LayerNorm -> token_mean -> linear + ReLU -> linear (fp32)
The head's frequency-group regroup (ClapAudioEncoder.forward) only permutes the 64 final tokens before AdaptiveAvgPool1d
averages all of them, so the pool is a plain token mean.
"""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import ACT_GELU, ACT_LRELU, AldmError
from .ops import _p, _require_gpu, _stream, check
from . import _lib

# transformers.ClapAudioConfig defaults; laion/clap-htsat-fused overrides enable_fusion / fusion_type
CLAP_AUDIO = dict(window_size=8, num_mel_bins=64, spec_size=256, hidden_act="gelu", patch_size=4, patch_stride=[4, 4],
                  hidden_size=768, projection_dim=512, depths=[2, 2, 6, 2], num_attention_heads=[4, 8, 16, 32],
                  enable_fusion=False, fusion_type=None, patch_embed_input_channels=1, flatten_patch_embeds=True,
                  patch_embeds_hidden_size=96, enable_patch_layer_norm=True, qkv_bias=True, mlp_ratio=4.0, aff_block_r=4,
                  projection_hidden_act="relu", layer_norm_eps=1e-5)

# transformers.ClapFeatureExtractor defaults
CLAP_FEATURES = dict(feature_size=64, sampling_rate=48000, hop_length=480, max_length_s=10, fft_window_size=1024,
                     frequency_min=0, frequency_max=14000, truncation="fusion", padding="repeatpad")


# ---- host-side tables ------------------------------------------------------------------------------------------------------------
def resample_taps(up=3):
    """The FIR of scipy.signal.resample_poly(x, up, 1): firwin(20 up + 1, 1/up, window=("kaiser", 5.0)) * up, in numpy."""
    half = 10 * up
    n = np.arange(2 * half + 1, dtype=np.float64) - half
    cutoff = 1.0 / up
    h = cutoff * np.sinc(cutoff * n) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def _hz_to_mel(f, scale):
    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    logstep = 27.0 / np.log(6.4)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-10) / 1000.0) * logstep, 3.0 * f / 200.0)


def _mel_to_hz(m, scale):
    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (np.power(10.0, m / 2595.0) - 1.0)
    logstep = np.log(6.4) / 27.0
    return np.where(m >= 15.0, 1000.0 * np.exp(logstep * (m - 15.0)), 200.0 * m / 3.0)


def mel_filter_bank(num_frequency_bins, num_mel_filters, min_frequency, max_frequency, sampling_rate, norm=None, mel_scale="htk"):
    """transformers.audio_utils.mel_filter_bank (triangles in Hz space): [num_frequency_bins, num_mel_filters] float64."""
    mel_freqs = np.linspace(_hz_to_mel(min_frequency, mel_scale), _hz_to_mel(max_frequency, mel_scale), num_mel_filters + 2)
    filter_freqs = _mel_to_hz(mel_freqs, mel_scale)
    fft_freqs = np.linspace(0, sampling_rate // 2, num_frequency_bins)
    diff = np.diff(filter_freqs)
    slopes = filter_freqs[None, :] - fft_freqs[:, None]
    down = -slopes[:, :-2] / diff[:-1]
    up = slopes[:, 2:] / diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    if norm == "slaney":
        fb *= (2.0 / (filter_freqs[2:num_mel_filters + 2] - filter_freqs[:num_mel_filters]))[None, :]
    return fb


# ---- front end -----------------------------------------------------------------------------------------------------------------
class ClapAudioFrontEnd:
    """ClapFeatureExtractor on the device.  `fe(audios, sampling_rate)` -> SimpleNamespace(input_features, is_longer).

    audios: fp32 [B, T] on the GPU (every clip T samples), or a list of 1-D GPU tensors of different lengths.  16 kHz audio
    is resampled to 48 kHz first (resample_up3: scipy.signal.resample_poly's FIR, not the soxr resampler librosa calls).

    is_longer -- the reference embeds ONE clip per processor call, and transformers marks a random clip of a batch as
    "longer" when none is; a lone clip is therefore always fused.  This front end gives every clip of a batch the result it
    gets alone: with truncation="fusion" every clip (<= max_length_s) is is_longer=True and its four mel channels are the
    same spectrogram (a stride-0 view, no copy).  truncation="rand_trunc" (unfused checkpoints): one channel, Slaney bank,
    is_longer=False.  Clips longer than max_length_s need transformers' random crops and raise NotImplementedError."""

    def __init__(self, device="cuda", **over):
        unknown = set(over) - set(CLAP_FEATURES)
        if unknown:
            raise TypeError(f"ClapAudioFrontEnd: unknown options {sorted(unknown)}")
        c = dict(CLAP_FEATURES)
        c.update(over)
        if c["truncation"] not in ("fusion", "rand_trunc"):
            raise NotImplementedError(f"ClapAudioFrontEnd: truncation={c['truncation']!r} (fusion / rand_trunc only)")
        if c["padding"] != "repeatpad":
            raise NotImplementedError(f"ClapAudioFrontEnd: padding={c['padding']!r} (repeatpad only)")
        if c["fft_window_size"] != 1024:
            raise NotImplementedError(f"ClapAudioFrontEnd: fft_window_size={c['fft_window_size']} (1024 only)")
        self.cfg = c
        self.device = torch.device(device)
        self.max_len = int(c["max_length_s"] * c["sampling_rate"])
        nbins = c["fft_window_size"] // 2 + 1
        fusion = c["truncation"] == "fusion"
        fb = mel_filter_bank(nbins, c["feature_size"], c["frequency_min"], c["frequency_max"], c["sampling_rate"],
                             norm=None if fusion else "slaney", mel_scale="htk" if fusion else "slaney")
        basis = np.ascontiguousarray(fb.T).astype(np.float32)
        rng = np.zeros((c["feature_size"], 2), dtype=np.int32)
        for m, row in enumerate(basis):
            nz = np.nonzero(row)[0]
            rng[m] = (nz.min(), nz.max() + 1) if nz.size else (0, 0)
        n = c["fft_window_size"]
        win = np.hanning(n + 1)[:-1]                                   # window_function(n, "hann"): periodic
        self.basis = torch.from_numpy(basis).to(self.device)
        self.ranges = torch.from_numpy(rng).to(self.device)
        self.window = torch.from_numpy(win.astype(np.float32)).to(self.device)
        self.taps = torch.from_numpy(resample_taps(3).astype(np.float32)).to(self.device)

    @classmethod
    def from_pretrained(cls, path, device="cuda", **over):
        """Reads frequency_min / frequency_max (and the other extractor settings) from preprocessor_config.json if present."""
        f = os.path.join(path, "preprocessor_config.json")
        raw = json.load(open(f)) if os.path.isfile(f) else {}
        kw = {k: raw[k] for k in CLAP_FEATURES if k in raw}
        kw.update(over)
        return cls(device, **kw)

    @staticmethod
    def _stack(audios):
        if isinstance(audios, torch.Tensor):
            if audios.dim() == 1:
                audios = audios[None]
            _require_gpu(audios)
            w = audios.to(torch.float32).contiguous()
            return w, torch.full((w.shape[0],), w.shape[1], dtype=torch.int32)
        if not audios:
            raise ValueError("ClapAudioFrontEnd: no clips")
        for a in audios:
            _require_gpu(a)
            if a.dim() != 1:
                raise ValueError("ClapAudioFrontEnd: every clip of a list must be 1-D (mono)")
        lens = torch.tensor([a.shape[0] for a in audios], dtype=torch.int32)
        w = torch.zeros(len(audios), int(lens.max()), dtype=torch.float32, device=audios[0].device)
        for i, a in enumerate(audios):
            w[i, :a.shape[0]] = a
        return w, lens

    def resample_16k_to_48k(self, w, lens):
        """w fp32 [B, T] on the GPU holding lens[b] samples -> ([B, 3 T], 3 lens)."""
        B, T = w.shape
        out = torch.empty(B, 3 * T, dtype=torch.float32, device=w.device)
        dl = lens.to(w.device)
        check(_lib.load().aldm_resample_up3(_p(w), _p(dl), B, T, _p(self.taps), self.taps.numel(), _p(out), 3 * T, _stream()),
              "aldm_resample_up3")
        return out, lens * 3

    def __call__(self, audios, sampling_rate=48000):
        w, lens = self._stack(audios)
        if int(lens.min()) < 1:
            raise ValueError("ClapAudioFrontEnd: empty clip")
        if sampling_rate == 16000:
            w, lens = self.resample_16k_to_48k(w, lens)
        elif sampling_rate != self.cfg["sampling_rate"]:
            raise ValueError(f"ClapAudioFrontEnd: sampling_rate {sampling_rate} (48000, or 16000 to resample here)")
        if int(lens.max()) > self.max_len:
            raise NotImplementedError(f"ClapAudioFrontEnd: clips longer than {self.cfg['max_length_s']} s need transformers' random "
                                      "fusion crops (np.random); cut them first")
        B, T = w.shape
        c = self.cfg
        hop, nm = c["hop_length"], c["feature_size"]
        frames = 1 + self.max_len // hop
        mel = torch.empty(B, frames, nm, dtype=torch.float32, device=w.device)
        dl = lens.to(w.device)
        check(_lib.load().aldm_clap_log_mel(_p(w), _p(dl), B, T, self.max_len, c["fft_window_size"], hop, _p(self.window),
                                            _p(self.basis), _p(self.ranges), nm, _p(mel), _stream()), "aldm_clap_log_mel")
        fusion = c["truncation"] == "fusion"
        feats = mel[:, None].expand(B, 4, frames, nm) if fusion else mel[:, None]
        is_longer = torch.full((B, 1), fusion, dtype=torch.bool, device=w.device)
        return SimpleNamespace(input_features=feats, is_longer=is_longer)


# ---- the tower (parameter containers under transformers' names) ----------------------------------------------------------------
class _AFF(nn.Module):
    def __init__(self, c, r):
        super().__init__()
        i = int(c // r)
        self.local_att = nn.Sequential(nn.Conv2d(c, i, 1), nn.BatchNorm2d(i), nn.ReLU(), nn.Conv2d(i, c, 1), nn.BatchNorm2d(c))
        self.global_att = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(c, i, 1), nn.BatchNorm2d(i), nn.ReLU(), nn.Conv2d(i, c, 1),
                                        nn.BatchNorm2d(c))


class _PatchEmbed(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        c, p = cfg["patch_embeds_hidden_size"], cfg["patch_size"]
        self.proj = nn.Conv2d(cfg["patch_embed_input_channels"], c, p, p)
        self.norm = nn.LayerNorm(c) if cfg["enable_patch_layer_norm"] else nn.Identity()
        if cfg["enable_fusion"]:
            self.fusion_model = _AFF(c, cfg["aff_block_r"])
            self.mel_conv2d = nn.Conv2d(cfg["patch_embed_input_channels"], c, (p, 3 * p), (p, 3 * p))


def _rel_index(w):
    coords = torch.stack(torch.meshgrid([torch.arange(w), torch.arange(w)], indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += w - 1
    rel[:, :, 1] += w - 1
    rel[:, :, 0] *= 2 * w - 1
    return rel.sum(-1)


class _SelfAttn(nn.Module):
    def __init__(self, c, heads, w, bias):
        super().__init__()
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * w - 1) ** 2, heads))
        self.register_buffer("relative_position_index", _rel_index(w))
        self.query, self.key, self.value = nn.Linear(c, c, bias=bias), nn.Linear(c, c, bias=bias), nn.Linear(c, c, bias=bias)


class _Dense(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.dense = nn.Linear(cin, cout)


class _Attn(nn.Module):
    def __init__(self, c, heads, w, bias):
        super().__init__()
        self.self = _SelfAttn(c, heads, w, bias)
        self.output = _Dense(c, c)


class _Layer(nn.Module):
    def __init__(self, c, heads, cfg):
        super().__init__()
        eps, hid = cfg["layer_norm_eps"], int(cfg["mlp_ratio"] * c)
        self.layernorm_before = nn.LayerNorm(c, eps=eps)
        self.attention = _Attn(c, heads, cfg["window_size"], cfg["qkv_bias"])
        self.layernorm_after = nn.LayerNorm(c, eps=eps)
        self.intermediate = _Dense(c, hid)
        self.output = _Dense(hid, c)


class _Merge(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.reduction = nn.Linear(4 * c, 2 * c, bias=False)
        self.norm = nn.LayerNorm(4 * c)


class _Stage(nn.Module):
    def __init__(self, c, depth, heads, cfg, down):
        super().__init__()
        self.blocks = nn.ModuleList([_Layer(c, heads, cfg) for _ in range(depth)])
        self.downsample = _Merge(c) if down else None


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        n = len(cfg["depths"])
        c0 = cfg["patch_embeds_hidden_size"]
        self.patch_embed = _PatchEmbed(cfg)
        self.layers = nn.ModuleList([_Stage(c0 * 2 ** i, cfg["depths"][i], cfg["num_attention_heads"][i], cfg, i < n - 1)
                                     for i in range(n)])
        self.batch_norm = nn.BatchNorm2d(cfg["num_mel_bins"])
        self.norm = nn.LayerNorm(c0 * 2 ** (n - 1))


class _AudioModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.audio_encoder = _Encoder(cfg)


class _Projection(nn.Module):
    def __init__(self, c, p):
        super().__init__()
        self.linear1, self.linear2 = nn.Linear(c, p), nn.Linear(p, p)


def _bn_fold(conv, bn, pad_out=None, pad_in=None):
    """1x1 conv followed by eval BatchNorm -> (weight [N, K], bias [N]) fp32, optionally zero-padded to pad_out rows / pad_in cols."""
    s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    w = conv.weight.detach().float().reshape(conv.weight.shape[0], -1) * s[:, None]
    b = (conv.bias.detach().float() - bn.running_mean.detach().float()) * s + bn.bias.detach().float()
    n, k = w.shape
    wp = torch.zeros(pad_out or n, pad_in or k, device=w.device)
    wp[:n, :k] = w
    bp = torch.zeros(pad_out or n, device=w.device)
    bp[:n] = b
    return wp, bp


def _ln(m):
    return (m.weight.detach().float().contiguous(), m.bias.detach().float().contiguous(), m.eps)


class ClapAudioModelWithProjection(nn.Module):
    """transformers.ClapAudioModelWithProjection (eval) on the HIP kernels.  forward(input_features, is_longer) ->
    SimpleNamespace(audio_embeds fp32 [B, projection_dim], pooler_output fp32 [B, hidden_size]).  No CPU fallback."""

    def __init__(self, **over):
        super().__init__()
        cfg = dict(CLAP_AUDIO)
        cfg.update({k: v for k, v in over.items() if k in CLAP_AUDIO})
        for k in ("depths", "num_attention_heads", "patch_stride"):
            cfg[k] = list(cfg[k]) if isinstance(cfg[k], (list, tuple)) else [cfg[k]] * (2 if k == "patch_stride" else 1)
        self._check(cfg)
        self.cfg = cfg
        self.config = SimpleNamespace(**cfg)
        self.audio_model = _AudioModel(cfg)
        self.audio_projection = _Projection(cfg["hidden_size"], cfg["projection_dim"])
        self.eval()
        self._plan = None

    @staticmethod
    def _check(cfg):
        n = len(cfg["depths"])
        c0 = cfg["patch_embeds_hidden_size"]
        if cfg["enable_fusion"] and cfg["fusion_type"] not in ("aff_2d", None):
            raise NotImplementedError(f"ClapAudioModelWithProjection: fusion_type={cfg['fusion_type']!r} (aff_2d only)")
        if cfg["spec_size"] != 256:
            raise NotImplementedError(f"ClapAudioModelWithProjection: spec_size={cfg['spec_size']} (256 only)")
        if cfg["window_size"] != 8:
            raise NotImplementedError(f"ClapAudioModelWithProjection: window_size={cfg['window_size']} (8 only)")
        for i in range(n):
            c, h = c0 * 2 ** i, cfg["num_attention_heads"][i]
            if c % h or c // h != 24:
                raise NotImplementedError(f"ClapAudioModelWithProjection: head dim {c}/{h} at stage {i} (num_attention_heads must "
                                          "give head dim 24)")
        if cfg["num_mel_bins"] != 64 or cfg["patch_size"] != 4 or list(cfg["patch_stride"]) != [4, 4] or n != 4:
            raise NotImplementedError("ClapAudioModelWithProjection: num_mel_bins 64, patch_size / patch_stride 4 and 4 stages only")
        if cfg["patch_embed_input_channels"] != 1 or not cfg["flatten_patch_embeds"] or cfg["hidden_act"] != "gelu":
            raise NotImplementedError("ClapAudioModelWithProjection: patch_embed_input_channels 1, flattened patches, gelu only")
        if cfg["projection_hidden_act"] != "relu" or cfg["hidden_size"] != c0 * 2 ** (n - 1):
            raise NotImplementedError("ClapAudioModelWithProjection: relu projection, hidden_size = last stage width only")

    @classmethod
    def from_config_dict(cls, raw):
        return cls(**{k: raw[k] for k in CLAP_AUDIO if k in raw})

    def _apply(self, fn, *a, **k):
        self._plan = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._plan = None
        return super().load_state_dict(*a, **k)

    def plan(self):
        if self._plan is not None:
            return self._plan
        enc = self.audio_model.audio_encoder
        if enc.norm.weight.device.type != "cuda":
            raise AldmError("ClapAudioModelWithProjection runs on the MI355X only: call .to('cuda') first (no CPU fallback)")
        cfg = self.cfg
        bn = enc.batch_norm
        s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        pe = enc.patch_embed
        P = SimpleNamespace(bn_scale=s.contiguous(), bn_shift=(bn.bias.detach().float() - bn.running_mean.detach().float() * s).contiguous(),
                            proj=ops.pack_linear(pe.proj.weight.reshape(pe.proj.weight.shape[0], -1), pe.proj.bias),   # K = kh 4 + kw
                            pe_norm=_ln(pe.norm) if cfg["enable_patch_layer_norm"] else None, fusion=None, stages=[])
        if cfg["enable_fusion"]:
            fm = pe.fusion_model
            inter = fm.local_att[0].weight.shape[0]
            ip = (inter + 15) // 16 * 16                  # inter channels padded with zero rows / columns (GEMM K % 8)
            l1w, l1b = _bn_fold(fm.local_att[0], fm.local_att[1], pad_out=ip)
            l2w, l2b = _bn_fold(fm.local_att[3], fm.local_att[4], pad_in=ip)
            g1w, g1b = _bn_fold(fm.global_att[1], fm.global_att[2], pad_out=ip)
            g2w, g2b = _bn_fold(fm.global_att[4], fm.global_att[5], pad_in=ip)
            P.fusion = SimpleNamespace(mel=ops.pack_linear(pe.mel_conv2d.weight.reshape(pe.mel_conv2d.weight.shape[0], -1), pe.mel_conv2d.bias),
                                       l1=ops.pack_linear(l1w, l1b), l2=ops.pack_linear(l2w, l2b),
                                       g1=ops.pack_linear(g1w, g1b), g2=ops.pack_linear(g2w, g2b))
        for i, st in enumerate(enc.layers):
            res = 64 >> i
            blocks = []
            for j, blk in enumerate(st.blocks):
                sa = blk.attention.self
                heads = sa.relative_position_bias_table.shape[1]
                bias = sa.relative_position_bias_table.detach().float()[sa.relative_position_index.reshape(-1)]
                bias = bias.view(64, 64, heads).permute(2, 0, 1).contiguous()
                qb = None if sa.query.bias is None else torch.cat([sa.query.bias, sa.key.bias, sa.value.bias])
                blocks.append(SimpleNamespace(
                    heads=heads, shift=(cfg["window_size"] // 2 if (j % 2 == 1 and res > cfg["window_size"]) else 0), bias=bias,
                    ln1=_ln(blk.layernorm_before), qkv=ops.pack_linear(torch.cat([sa.query.weight, sa.key.weight, sa.value.weight]), qb),
                    ao=ops.pack_linear(blk.attention.output.dense.weight, blk.attention.output.dense.bias), ln2=_ln(blk.layernorm_after),
                    ff1=ops.pack_linear(blk.intermediate.dense.weight, blk.intermediate.dense.bias),
                    ff2=ops.pack_linear(blk.output.dense.weight, blk.output.dense.bias)))
            down = None
            if st.downsample is not None:
                down = SimpleNamespace(ln=_ln(st.downsample.norm), red=ops.pack_linear(st.downsample.reduction.weight, None))
            P.stages.append(SimpleNamespace(res=res, blocks=blocks, down=down))
        P.norm = _ln(enc.norm)
        P.p1 = ops.pack_linear(self.audio_projection.linear1.weight, self.audio_projection.linear1.bias)
        P.p2 = ops.pack_linear(self.audio_projection.linear2.weight, self.audio_projection.linear2.bias)
        self._plan = P
        return P

    @torch.no_grad()
    def forward(self, input_features=None, is_longer=None, return_dict=True, **kw):
        P, cfg = self.plan(), self.cfg
        f = input_features
        _require_gpu(f)
        f = f.float()
        if f.dim() != 4 or f.shape[3] != 64 or f.stride(3) != 1 or f.stride(2) != 64:
            raise ValueError(f"input_features must be [B, C, T, 64] with contiguous frames (got {tuple(f.shape)})")
        B, Cm, T = f.shape[:3]
        lib = _lib.load()
        dev = f.device
        fusion = cfg["enable_fusion"]
        if fusion and Cm != 4:
            raise ValueError(f"a fused tower takes 4 mel channels (truncation='fusion'), got {Cm}")
        if not fusion and Cm != 1:
            raise ValueError(f"an unfused tower takes 1 mel channel (truncation='rand_trunc'), got {Cm}")
        c0 = cfg["patch_embeds_hidden_size"]
        g = torch.empty(B, 64, 64, 16, dtype=torch.bfloat16, device=dev)
        loc = torch.empty(B, 64, 64, 48, dtype=torch.bfloat16, device=dev) if fusion else None
        check(lib.aldm_clap_input(_p(f), f.stride(0), f.stride(1), B, T, 64, _p(P.bn_scale), _p(P.bn_shift), _p(g), _p(loc), _stream()),
              "aldm_clap_input")
        M = B * 4096
        h = ops.linear(g.view(M, 16), P.proj)
        if fusion:
            if is_longer is None:
                raise ValueError("a fused tower needs is_longer (ClapAudioFrontEnd / ClapFeatureExtractor output)")
            longer = is_longer.reshape(-1).to(device=dev, dtype=torch.int32)
            Fz = P.fusion
            r = ops.linear(loc.view(M, 48), Fz.mel)
            a = torch.empty_like(h)
            pooled = torch.empty(B, c0, dtype=torch.bfloat16, device=dev)
            check(lib.aldm_aff_sum_pool(_p(h), _p(r), B, c0, _p(a), _p(pooled), _stream()), "aldm_aff_sum_pool")
            lt = ops.linear(a, Fz.l1, out_act=ACT_LRELU, out_slope=0.0)
            lo = ops.linear(lt, Fz.l2, out_f32=True)
            gt = ops.linear(pooled, Fz.g1, out_act=ACT_LRELU, out_slope=0.0)
            go = ops.linear(gt, Fz.g2, out_f32=True)
            fused = torch.empty_like(h)
            check(lib.aldm_aff_combine(_p(h), _p(r), _p(lo), _p(go), _p(longer), B, c0, _p(fused), _stream()), "aldm_aff_combine")
            h = fused
        x = ops.layernorm(h, *P.pe_norm) if P.pe_norm is not None else h
        for st in P.stages:
            R = st.res
            C = x.shape[1]
            for bp in st.blocks:
                hn = ops.layernorm(x, *bp.ln1)
                qkv = ops.linear(hn, bp.qkv)
                att = window_attention(qkv, B, R, R, bp.heads, bp.shift, bp.bias)
                x = ops.linear(att, bp.ao, res=x)
                hn = ops.layernorm(x, *bp.ln2)
                x = ops.linear(ops.linear(hn, bp.ff1, out_act=ACT_GELU), bp.ff2, res=x)
            if st.down is not None:
                m = patch_merge_gather(x, B, R, R, C)
                x = ops.linear(ops.layernorm(m, *st.down.ln), st.down.red)
        x = ops.layernorm(x, *P.norm)
        N, C = x.shape[0] // B, x.shape[1]
        pooled32 = torch.empty(B, C, dtype=torch.float32, device=dev)
        pooled16 = torch.empty(B, C, dtype=torch.bfloat16, device=dev)
        check(lib.aldm_token_mean(_p(x), B, N, C, _p(pooled32), _p(pooled16), _stream()), "aldm_token_mean")
        t = ops.linear(pooled16, P.p1, out_act=ACT_LRELU, out_slope=0.0)
        emb = ops.linear(t, P.p2, out_f32=True)
        if not return_dict:
            return (emb, x.view(B, N, C))
        return SimpleNamespace(audio_embeds=emb, pooler_output=pooled32, last_hidden_state=x.view(B, N, C))


def window_attention(qkv, B, H, W, heads, shift, bias, head_dim=24, window=8):
    """Swin window attention over the token-major QKV rows qkv [B*H*W, 3C]; returns [B*H*W, C] token-major."""
    _require_gpu(qkv)
    C = heads * head_dim
    out = torch.empty(B * H * W, C, dtype=torch.bfloat16, device=qkv.device)
    check(_lib.load().aldm_window_attention(_p(qkv), qkv.shape[1], B, H, W, heads, head_dim, window, shift, _p(bias),
                                            1.0 / math.sqrt(head_dim), _p(out), C, _stream()), "aldm_window_attention")
    return out


def patch_merge_gather(x, B, H, W, C):
    _require_gpu(x)
    out = torch.empty(B * (H // 2) * (W // 2), 4 * C, dtype=torch.bfloat16, device=x.device)
    check(_lib.load().aldm_patch_merge_gather(_p(x), B, H, W, C, _p(out), _stream()), "aldm_patch_merge_gather")
    return out


# ---- both towers -----------------------------------------------------------------------------------------------------------------
class ClapModel(nn.Module):
    """The two CLAP towers of a `laion/clap-htsat-*` checkpoint: get_audio_features / get_text_features return the projected
    embeddings (not normalised: the metrics normalise, as the reference does).  logit_scale_a / logit_scale_t are loaded and
    not used."""

    def __init__(self, text_config=None, audio_config=None):
        super().__init__()
        from .clap_text import ClapTextModelWithProjection
        from .configs import CLAP_TEXT
        tc = {k: v for k, v in (text_config or {}).items() if k in CLAP_TEXT}
        self.text = ClapTextModelWithProjection(**tc)
        self.audio = ClapAudioModelWithProjection.from_config_dict(audio_config or {})
        self.logit_scale_a = nn.Parameter(torch.tensor(math.log(1 / 0.07)))
        self.logit_scale_t = nn.Parameter(torch.tensor(math.log(1 / 0.07)))
        self.tokenizer = None
        self.front_end_config = {}

    @classmethod
    def from_pretrained(cls, path, **kw):
        f = os.path.join(path, "config.json")
        if not os.path.isfile(f):
            raise FileNotFoundError(f"{f} not found: hub downloads are unavailable, pass a local directory")
        raw = json.load(open(f))
        m = cls(raw.get("text_config", {}), raw.get("audio_config", {}))
        from safetensors.torch import load_file
        m.load_checkpoint_state_dict(load_file(os.path.join(path, "model.safetensors")))
        pf = os.path.join(path, "preprocessor_config.json")
        if os.path.isfile(pf):
            m.front_end_config = {k: v for k, v in json.load(open(pf)).items() if k in CLAP_FEATURES}
        if os.path.isfile(os.path.join(path, "tokenizer.json")) or os.path.isfile(os.path.join(path, "vocab.json")):
            from transformers import RobertaTokenizerFast
            m.tokenizer = RobertaTokenizerFast.from_pretrained(path)
        return m

    def load_checkpoint_state_dict(self, sd):
        """Splits a transformers ClapModel state dict between the towers; every key must land (strict)."""
        text, audio, rest = {}, {}, {}
        for k, v in sd.items():
            if k.startswith(("text_model.", "text_projection.")):
                if not k.endswith(("position_ids", "token_type_ids")):     # persistent index buffers of the text embeddings
                    text[k] = v
            elif k.startswith(("audio_model.", "audio_projection.")):
                audio[k] = v
            else:
                rest[k] = v
        unknown = set(rest) - {"logit_scale_a", "logit_scale_t"}
        if unknown:
            raise KeyError(f"ClapModel: unexpected keys {sorted(unknown)[:8]}")
        self.text.load_state_dict(text, strict=True)
        self.audio.load_state_dict(audio, strict=True)
        with torch.no_grad():
            for k in ("logit_scale_a", "logit_scale_t"):
                if k in rest:
                    getattr(self, k).copy_(rest[k].reshape(()))

    def front_end(self, device="cuda"):
        cfg = dict(self.front_end_config)
        cfg.setdefault("truncation", "fusion" if self.audio.cfg["enable_fusion"] else "rand_trunc")
        return ClapAudioFrontEnd(device, **cfg)

    @torch.no_grad()
    def get_audio_features(self, input_features=None, is_longer=None, **kw):
        return self.audio(input_features, is_longer).audio_embeds

    @torch.no_grad()
    def get_text_features(self, input_ids=None, attention_mask=None, **kw):
        return self.text(input_ids=input_ids, attention_mask=attention_mask).text_embeds
