"""Test helper: the reference for mixed-adapter batches, restated on the EXISTING fp32 CPU oracle.

For a sample whose gates are g_a, the expected UNet output is `oracle.unet.UNet2DConditionModel` with
    W + sum_a g_a (alpha_a / r_a) B_a A_a
merged into every targeted weight, run on that sample alone.  No adapter code of the package under test is involved: the adapters
are plain dicts of tensors made here, and `peft_state_dict` writes them in peft's saved form for the loaders under test.
"""
import copy

import torch

TARGETS4 = ("to_q", "to_k", "to_v", "to_out.0")


def _match(name, targets):
    return any(name == t or name.endswith("." + t) for t in targets)


def make_adapter(model, r, alpha, targets, seed, b_std=0.05):
    """{'r', 'alpha', 'targets', 'tensors': {module path: (A [r, in], B [out, r])}} for every nn.Linear of `model` whose name ends with a
    target.  lora_B ~ N(0, b_std^2) from Generator(seed) in module order (the recipe of the single-adapter UNet test), lora_A ~ N(0, (1/r)^2)
    (peft's gaussian init) from Generator(seed + 1000)."""
    gb, ga = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed + 1000)
    tensors = {}
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.Linear) and _match(name, targets):
            A = torch.randn(r, m.in_features, generator=ga) / r
            B = torch.randn(m.out_features, r, generator=gb) * b_std
            tensors[name] = (A, B)
    assert tensors, "no module matched the targets"
    return dict(r=r, alpha=alpha, targets=tuple(targets), tensors=tensors)


def peft_state_dict(adapter, prefix="base_model.model."):
    """peft's saved form (get_peft_model_state_dict): keys without the adapter name"""
    sd = {}
    for name, (A, B) in adapter["tensors"].items():
        sd[f"{prefix}{name}.lora_A.weight"] = A.clone()
        sd[f"{prefix}{name}.lora_B.weight"] = B.clone()
    return sd


def merged_oracle(ref, adapters, gates):
    """deep copy of the oracle UNet `ref` with sum_a gates[a] (alpha_a / r_a) B_a A_a added to the targeted weights"""
    m = copy.deepcopy(ref)
    with torch.no_grad():
        for a, g in gates.items():
            ad = adapters[a]
            s = ad["alpha"] / ad["r"]
            for name, (A, B) in ad["tensors"].items():
                m.get_submodule(name).weight += float(g) * s * (B @ A)
    return m.eval()


def gates_of(entry, adapters, weights=None):
    """an adapter_names entry -> {adapter: gate} (the semantics the package documents: name = its set weight, default 1)"""
    weights = weights or {}
    if entry == "__base__":
        return {}
    if isinstance(entry, str):
        return {entry: weights.get(entry, 1.0)}
    if isinstance(entry, dict):
        return dict(entry)
    return {n: weights.get(n, 1.0) for n in entry}


def expected_batch(ref, adapters, routing, x, t, c, weights=None):
    """per-sample oracle outputs of a mixed batch, concatenated: sample b runs through the oracle merged with routing[b]'s gates"""
    outs = []
    with torch.no_grad():
        for b, entry in enumerate(routing):
            m = merged_oracle(ref, adapters, gates_of(entry, adapters, weights))
            tb = t[b:b + 1] if torch.is_tensor(t) and t.dim() > 0 and t.numel() > 1 else t
            outs.append(m(x[b:b + 1], tb, class_labels=c[b:b + 1])[0])
    return torch.cat(outs)
