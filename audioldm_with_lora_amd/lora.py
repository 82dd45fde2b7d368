"""peft-shaped LoRA helpers for the HIP path.

Mirrors the surface the reference uses -- `LoraConfig`, `get_peft_model`, `get_peft_model_state_dict`
[REF script/train/train_audioldm_lora.py:35-36,378-385,578] [REF script/inference/generate_audio.py:8,21-36]
and diffusers' `convert_state_dict_to_diffusers` -- with peft 0.13.2 semantics: in-place
injection by module-name suffix, adapter name "default", state-dict prefix `base_model.model.`,
A ~ N(0, (1/r)^2) / B = 0 for init_lora_weights="gaussian", scaling = lora_alpha / r.

The wrapped layers are parameter containers: the arithmetic y = Wx + (alpha/r) B(Ax) runs fused inside
aldm_igemm (one launch per projection GEMM), never in Python.

Several named adapters can live in one model (peft's `add_adapter` / `load_adapter` / `set_adapter` / `disable_adapter`, and its
mixed-adapter batches: `adapter_names=[...]` with "__base__" for none).  The fused GEMMs hold all of them side by side -- adapter `a`
owns one block of the columns of T = x A_cat^T, the same block in every fused GEMM of the model (`lora_layout`) -- and a per-sample
fp32 gate row multiplies those columns (`AdapterRouting.gate_table`):
    y[b] = W x[b] + sum_a gate[b][a] (alpha_a / r_a) B_a (A_a x[b])
Choosing, weighting, blending or switching adapters off is a change of that small table; only adding, loading or deleting an adapter
repacks the operands.
"""
import contextlib
import json
import math
import os
from dataclasses import dataclass, field
from typing import Sequence

import torch
from torch import nn

BASE = "__base__"          # peft's word for "no adapter" in adapter_names
GATE_COLS = 32             # columns of the gate table = Rp of the persistent / block kernels' LoRA side channel


@dataclass
class LoraConfig:
    r: int = 8
    lora_alpha: int = 8
    target_modules: Sequence[str] = field(default_factory=lambda: ["to_q", "to_v"])
    init_lora_weights: object = True
    lora_dropout: float = 0.0
    bias: str = "none"


class LoraLinear(nn.Module):
    """Container with peft's key layout: base_layer.{weight,bias}, lora_A.<name>.weight [r, in], lora_B.<name>.weight [out, r];
    any number of named adapters, each with its own r / lora_alpha / scaling (`rank`, `alpha`, `scale`, keyed by name)."""

    def __init__(self, base: nn.Linear, cfg: LoraConfig = None, adapter_name: str = "default"):
        super().__init__()
        self.base_layer = base
        self.lora_A = nn.ModuleDict()
        self.lora_B = nn.ModuleDict()
        self.rank, self.alpha, self.scale = {}, {}, {}
        if cfg is not None:
            self.add_adapter(adapter_name, cfg)

    def add_adapter(self, name: str, cfg: LoraConfig):
        assert cfg.lora_dropout == 0.0 and cfg.bias == "none", "reference uses lora_dropout=0, bias='none'"
        if name in self.lora_A:
            raise ValueError(f"adapter {name!r} already exists on this layer")
        base, dev = self.base_layer, self.base_layer.weight.device
        self.lora_A[name] = nn.Linear(base.in_features, cfg.r, bias=False, device=dev)
        self.lora_B[name] = nn.Linear(cfg.r, base.out_features, bias=False, device=dev)
        self.rank[name], self.alpha[name], self.scale[name] = cfg.r, cfg.lora_alpha, cfg.lora_alpha / cfg.r
        if cfg.init_lora_weights == "gaussian":
            nn.init.normal_(self.lora_A[name].weight, std=1.0 / cfg.r)
        else:
            nn.init.kaiming_uniform_(self.lora_A[name].weight, a=5 ** 0.5)
        nn.init.zeros_(self.lora_B[name].weight)

    def delete_adapter(self, name: str):
        if name in self.lora_A:
            del self.lora_A[name], self.lora_B[name], self.rank[name], self.alpha[name], self.scale[name]

    @property
    def adapters(self):
        return list(self.lora_A.keys())

    def _single(self, table):
        """r / lora_alpha / scaling of the layer as scalars: the single-adapter surface ("default" when there are several)."""
        if "default" in table or not table:
            return table.get("default")
        return next(iter(table.values()))

    @property
    def r(self):
        return self._single(self.rank)

    @property
    def lora_alpha(self):
        return self._single(self.alpha)

    @property
    def scaling(self):
        return self._single(self.scale)

    def parts(self):
        """[(adapter name, A [r, in], B [out, r], scaling)] in insertion order: what the weight packers take."""
        return [(n, self.lora_A[n].weight, self.lora_B[n].weight, self.scale[n]) for n in self.lora_A.keys()]

    @property
    def in_features(self):
        return self.base_layer.in_features

    @property
    def out_features(self):
        return self.base_layer.out_features

    def forward(self, *a, **k):
        raise RuntimeError("LoraLinear is a parameter container; the fused HIP GEMM computes it")


def _match(name, targets):
    return any(name == t or name.endswith("." + t) for t in targets)


# ----------------------------------------------------------------------------------------------
# column layout and routing
# ----------------------------------------------------------------------------------------------
QKV = ("to_q", "to_k", "to_v")


def lora_groups(model):
    """The LoRA-wrapped layers of `model` grouped as the fused GEMMs take them: to_q | to_k | to_v of one attention module share one
    GEMM (one side channel, ops.attach_lora); every other wrapped layer is a GEMM of its own."""
    groups = {}
    for name, m in model.named_modules():
        if isinstance(m, LoraLinear):
            parent, _, leaf = name.rpartition(".")
            groups.setdefault(parent + ".qkv" if leaf in QKV else name, []).append(m)
    return list(groups.values())


def adapter_names_of(model):
    """names of the adapters present, in the order they were added"""
    names = []
    for m in model.modules():
        if isinstance(m, LoraLinear):
            names += [n for n in m.lora_A.keys() if n not in names]
    return names


def lora_layout(model, extra=None):
    """{adapter: (first column, width)}: ONE column layout for the whole model.  Adapter `a` owns the same block of the side channel's
    columns in every fused GEMM; its width is the largest combined rank it has in any one of them (r_q + r_k + r_v of an attention
    module, r of an out-projection), blocks in the order the adapters were added.  So one gate table serves every gated launch of a
    step.  With a single adapter this is the layout of the single-adapter packing (columns 0 .. combined rank - 1).
    extra = (name, cfg): the layout the model WOULD have with that adapter added (capacity check before anything is built)."""
    from ._lib import AldmError
    names = adapter_names_of(model)
    width = {n: 0 for n in names}
    for grp in lora_groups(model):
        for n in names:
            width[n] = max(width[n], sum(m.rank.get(n, 0) for m in grp))
    if extra is not None:
        name, cfg = extra
        w = 0
        byparent = {}
        for mname, m in model.named_modules():
            if (isinstance(m, nn.Linear) and not mname.endswith("base_layer") or isinstance(m, LoraLinear)) and _match(mname, cfg.target_modules):
                parent, _, leaf = mname.rpartition(".")
                key = parent + ".qkv" if leaf in QKV else mname
                byparent[key] = byparent.get(key, 0) + cfg.r
        w = max(byparent.values(), default=0)
        names = names + [name]
        width[name] = w
    layout, col = {}, 0
    for n in names:
        layout[n] = (col, width[n])
        col += width[n]
    if len(names) > 1 and col > GATE_COLS:
        raise AldmError(f"the fused LoRA side channel holds a combined rank of {GATE_COLS} columns per GEMM across all adapters; "
                        f"these adapters need {col}: " + ", ".join(f"{n}={width[n]}" for n in names))
    return layout


def _finite(w, what):
    w = float(w)
    if not math.isfinite(w):
        raise ValueError(f"adapter weight for {what!r} is not finite ({w})")
    return w


class AdapterRouting:
    """Routing state of a model that holds LoraLinear layers (mixed into UNet2DConditionModel): which adapters are active, with which
    weights, and the per-sample gate table the fused kernels read.  None of this touches the packed operands."""

    def _routing(self):
        st = self.__dict__.get("_lora_routing")
        if st is None:
            st = self.__dict__["_lora_routing"] = {"active": None, "weights": {}, "disabled": False}
        return st

    def lora_adapters(self):
        return adapter_names_of(self)

    def lora_layout(self):
        return lora_layout(self)

    @property
    def active_adapters(self):
        st, names = self._routing(), adapter_names_of(self)
        if st["active"] is None:            # peft: the first adapter is the active one until set_adapter says otherwise
            return names[:1]
        return [n for n in st["active"] if n in names]

    def set_adapters(self, names, adapter_weights=None):
        """diffusers' set_adapters / peft's set_adapter: the adapters applied to every sample that is not routed explicitly."""
        present = adapter_names_of(self)
        names = [names] if isinstance(names, str) else list(names)
        if adapter_weights is None:
            adapter_weights = [1.0] * len(names)
        elif not isinstance(adapter_weights, (list, tuple)):
            adapter_weights = [adapter_weights] * len(names)
        if len(adapter_weights) != len(names):
            raise ValueError(f"{len(names)} adapter names but {len(adapter_weights)} weights")
        for n in names:
            if n not in present:
                raise ValueError(f"unknown adapter {n!r} (present: {present})")
        st = self._routing()
        st["active"] = names
        st["weights"].update({n: _finite(w, n) for n, w in zip(names, adapter_weights)})

    set_adapter = set_adapters

    def adapter_weight(self, name):
        return self._routing()["weights"].get(name, 1.0)

    def set_lora_enabled(self, on: bool):
        self._routing()["disabled"] = not on

    @property
    def lora_enabled(self):
        return not self._routing()["disabled"]

    def _forget_adapter(self, name):
        st = self._routing()
        st["weights"].pop(name, None)
        if st["active"] is not None:
            st["active"] = [n for n in st["active"] if n != name]

    def _default_spec(self):
        if self._routing()["disabled"]:
            return {}
        return {n: self.adapter_weight(n) for n in self.active_adapters}

    def _spec(self, entry):
        """one adapter_names entry -> {adapter: weight}"""
        present = adapter_names_of(self)
        if entry is None:
            return self._default_spec()
        if isinstance(entry, str):
            entry = [] if entry == BASE else [entry]
        if isinstance(entry, dict):
            spec = {n: _finite(w, n) for n, w in entry.items()}
        else:
            spec = {n: self.adapter_weight(n) for n in entry}
        for n in spec:
            if n not in present:
                raise ValueError(f"unknown adapter {n!r} (present: {present}; {BASE!r} = none)")
        return spec

    def routing_is_plain(self, adapter_names=None):
        """True when the launches need no gate: one adapter present, active, weight 1, nothing routed per sample -- or no adapter at all."""
        present = adapter_names_of(self)
        if not present:
            return True
        return (adapter_names is None and len(present) == 1 and not self._routing()["disabled"] and self.active_adapters == present
                and self.adapter_weight(present[0]) == 1.0)

    def gate_table(self, adapter_names, batch, num_waveforms_per_prompt=1, do_classifier_free_guidance=False):
        """fp32 [batch][GATE_COLS] (host): row b holds sample b's gate for every column of the side channel (lora_layout).
        adapter_names: None (every sample: the active adapters with their set weights) or one entry per prompt -- a name, "__base__",
        a list of names (their set weights) or a dict name -> weight (a blend).  Each entry is repeated over num_waveforms_per_prompt
        like the prompt embeddings; under classifier-free guidance the UNet batch is [uncond; cond] and both halves of a clip carry
        the same gates."""
        layout = lora_layout(self)
        if any(c0 + w > GATE_COLS for c0, w in layout.values()):
            from ._lib import AldmError
            raise AldmError(f"adapter routing needs the model's LoRA columns within {GATE_COLS} (layout {layout})")
        reps = num_waveforms_per_prompt * (2 if do_classifier_free_guidance else 1)
        if batch % reps:
            raise ValueError(f"batch {batch} is not a multiple of num_waveforms_per_prompt x CFG = {reps}")
        nprompt = batch // reps
        if adapter_names is None:
            adapter_names = [None] * nprompt
        if isinstance(adapter_names, (str, dict)) or len(adapter_names) != nprompt:
            raise ValueError(f"adapter_names needs one entry per prompt ({nprompt}), got {adapter_names!r}")
        rows = torch.zeros(nprompt, GATE_COLS, dtype=torch.float32)
        for i, entry in enumerate(adapter_names):
            for n, w in self._spec(entry).items():
                c0, wd = layout[n]
                rows[i, c0:c0 + wd] = w
        rows = rows.repeat_interleave(num_waveforms_per_prompt, dim=0)
        return torch.cat([rows, rows]) if do_classifier_free_guidance else rows


# ----------------------------------------------------------------------------------------------
def _read_adapter_file(path):
    """(state dict, adapter_config dict or None) of a local .safetensors / .bin file or a directory holding one"""
    cfg_json = None
    if os.path.isdir(path):
        d = path
        for fn in ("adapter_model.safetensors", "pytorch_lora_weights.safetensors", "adapter_model.bin", "pytorch_lora_weights.bin"):
            if os.path.exists(os.path.join(d, fn)):
                path = os.path.join(d, fn)
                break
        else:
            raise FileNotFoundError(f"no adapter_model / pytorch_lora_weights (.safetensors / .bin) in {d}")
    cj = os.path.join(os.path.dirname(path), "adapter_config.json")
    if os.path.exists(cj):
        with open(cj) as f:
            cfg_json = json.load(f)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path), cfg_json
    return torch.load(path, map_location="cpu", weights_only=True), cfg_json


def normalize_adapter_state_dict(sd):
    """peft's saved form (`...to_q.lora_A.weight`, with or without the `base_model.model.` prefix, with or without an adapter name)
    or the diffusers form (`...to_q.lora.down.weight`, optional `unet.` prefix) -> {(module path, "A" | "B"): tensor}"""
    out = {}
    for k, v in sd.items():
        k = k.replace(".lora.down.weight", ".lora_A.weight").replace(".lora.up.weight", ".lora_B.weight")
        for pre in ("base_model.model.", "unet."):
            if k.startswith(pre):
                k = k[len(pre):]
        for ab in ("A", "B"):
            tag = f".lora_{ab}."
            if tag in k and k.endswith(".weight"):
                out[(k[:k.index(tag)], ab)] = v
                break
        else:
            raise ValueError(f"not a LoRA tensor: {k}")
    return out


class PeftModel(nn.Module):
    def __init__(self, model, cfg, adapter_name="default"):
        super().__init__()
        self.base_model = nn.Module()
        self.base_model.model = model
        self.peft_config = {} if cfg is None else {adapter_name: cfg}

    def forward(self, *a, **k):
        return self.base_model.model(*a, **k)

    def _repack(self):
        inner = self.base_model.model
        if hasattr(inner, "invalidate_packed"):
            inner.invalidate_packed()

    def load_state_dict(self, *a, **k):
        """[REF script/inference/generate_audio.py:32-33] loads the adapter through the wrapper: the wrapped UNet's packed
        operands (and any captured denoise graph) must follow."""
        out = super().load_state_dict(*a, **k)
        self._repack()
        return out

    # ---- several adapters (peft's surface) ----
    def add_adapter(self, adapter_name, cfg):
        """Inject a new, freshly initialised adapter.  Raises AldmError -- before anything is built -- when the model's adapters
        would no longer fit the kernels' side channel."""
        model = self.base_model.model
        if adapter_name in adapter_names_of(model) or adapter_name == BASE:
            raise ValueError(f"adapter {adapter_name!r} already exists" if adapter_name != BASE else f"{BASE!r} is reserved")
        lora_layout(model, extra=(adapter_name, cfg))
        _inject(model, cfg, adapter_name)
        self.peft_config[adapter_name] = cfg
        self._repack()

    def load_adapter(self, path_or_state_dict, adapter_name, cfg=None):
        """A local .safetensors / .bin file or directory, or a state dict in peft's saved form (get_peft_model_state_dict) or in the
        diffusers form (convert_state_dict_to_diffusers).  Rank and targets are read from the tensors when cfg is not given;
        lora_alpha from an adapter_config.json next to the file, else = r."""
        cfg_json = None
        if isinstance(path_or_state_dict, (str, os.PathLike)):
            sd, cfg_json = _read_adapter_file(os.fspath(path_or_state_dict))
        else:
            sd = path_or_state_dict
        tensors = normalize_adapter_state_dict(sd)
        if not tensors:
            raise ValueError("load_adapter: no LoRA tensors in the state dict")
        model = self.base_model.model
        if cfg is None:
            ranks = {v.shape[0] for (m, ab), v in tensors.items() if ab == "A"}
            if len(ranks) != 1:
                raise ValueError(f"load_adapter: the tensors carry several ranks {sorted(ranks)}; pass cfg")
            r = ranks.pop()
            targets = sorted({m for m, _ in tensors})
            alpha = (cfg_json or {}).get("lora_alpha", r)
            cfg = LoraConfig(r=r, lora_alpha=alpha, target_modules=targets, init_lora_weights="gaussian")
        if adapter_name not in adapter_names_of(model):
            self.add_adapter(adapter_name, cfg)
        for (mname, ab), v in tensors.items():
            mod = model.get_submodule(mname)
            if not isinstance(mod, LoraLinear) or adapter_name not in mod.lora_A:
                raise ValueError(f"load_adapter: {mname} carries no adapter {adapter_name!r}")
            dst = (mod.lora_A if ab == "A" else mod.lora_B)[adapter_name].weight
            if tuple(dst.shape) != tuple(v.shape):
                raise ValueError(f"load_adapter: {mname}.lora_{ab} is {tuple(v.shape)}, the adapter has {tuple(dst.shape)}")
            with torch.no_grad():
                dst.copy_(v)
        self._repack()
        return self

    def delete_adapter(self, adapter_name):
        model = self.base_model.model
        if adapter_name not in adapter_names_of(model):
            raise ValueError(f"unknown adapter {adapter_name!r}")
        for m in model.modules():
            if isinstance(m, LoraLinear):
                m.delete_adapter(adapter_name)
        self.peft_config.pop(adapter_name, None)
        if hasattr(model, "_forget_adapter"):
            model._forget_adapter(adapter_name)
        self._repack()

    def set_adapter(self, name_or_names, adapter_weights=None):
        self.base_model.model.set_adapters(name_or_names, adapter_weights)

    set_adapters = set_adapter

    @property
    def active_adapters(self):
        return self.base_model.model.active_adapters

    @property
    def active_adapter(self):
        a = self.active_adapters
        return a[0] if a else None

    @contextlib.contextmanager
    def disable_adapter(self):
        model = self.base_model.model
        was = model.lora_enabled
        model.set_lora_enabled(False)
        try:
            yield
        finally:
            model.set_lora_enabled(was)

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.base_model.model, name)


def _inject(model, cfg, adapter_name):
    names = [n for n, m in model.named_modules()
             if (isinstance(m, LoraLinear) or (isinstance(m, nn.Linear) and not n.endswith("base_layer") and ".lora_" not in n)) and _match(n, cfg.target_modules)]
    for name in names:
        mod = model.get_submodule(name)
        if isinstance(mod, LoraLinear):
            mod.add_adapter(adapter_name, cfg)
            continue
        parent_name, _, leaf = name.rpartition(".")
        parent = model.get_submodule(parent_name) if parent_name else model
        wrapped = LoraLinear(mod, cfg, adapter_name)
        if leaf.isdigit():
            parent[int(leaf)] = wrapped
        else:
            setattr(parent, leaf, wrapped)


def get_peft_model(model: nn.Module, cfg: LoraConfig, adapter_name: str = "default") -> PeftModel:
    """Freeze the base, wrap every nn.Linear whose name ends with a target.  Mutates `model` in place."""
    for p in model.parameters():
        p.requires_grad_(False)
    lora_layout(model, extra=(adapter_name, cfg))
    _inject(model, cfg, adapter_name)
    if hasattr(model, "invalidate_packed"):
        model.invalidate_packed()
    return PeftModel(model, cfg, adapter_name)


def get_peft_model_state_dict(peft_model, adapter_name="default"):
    tag = f".{adapter_name}.weight"
    return {k[:-len(tag)] + ".weight": v for k, v in peft_model.state_dict().items() if "lora_" in k and k.endswith(tag)}


def convert_state_dict_to_diffusers(sd):
    return {k.replace(".lora_A.weight", ".lora.down.weight").replace(".lora_B.weight", ".lora.up.weight"): v
            for k, v in sd.items()}


def lora_parameters(model):
    return [p for n, p in model.named_parameters() if "lora_" in n]
