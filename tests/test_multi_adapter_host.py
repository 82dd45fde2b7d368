"""Host side of multi-adapter LoRA (no GPU): adapter containers and their state-dict forms, the packed column layout, the gate table,
capacity, the inference script's --adapters parser and the ctypes mirrors of the two extended structs."""
import ctypes

import pytest
import torch

import multi_adapter_restatement as mar


def _tiny():
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from oracle import configs
    torch.manual_seed(0)
    return UNet2DConditionModel(**configs.tiny_unet())


def _cfg(ad):
    from audioldm_with_lora_amd.lora import LoraConfig
    return LoraConfig(r=ad["r"], lora_alpha=ad["alpha"], target_modules=list(ad["targets"]), init_lora_weights="gaussian")


def _two(u):
    """adapter a: r = 4 on q / k / v / out; adapter b: r = 2 on q / v only (other rank, other targets)"""
    from audioldm_with_lora_amd import lora as plora
    ads = {"a": mar.make_adapter(u, 4, 8, mar.TARGETS4, seed=4), "b": mar.make_adapter(u, 2, 2, ("to_q", "to_v"), seed=5)}
    pm = plora.get_peft_model(u, _cfg(ads["a"]), adapter_name="a")
    pm.load_adapter(mar.peft_state_dict(ads["a"]), "a")
    pm.load_adapter(mar.peft_state_dict(ads["b"]), "b")                 # rank and targets read from the tensors
    return pm, ads


def test_state_dict_forms_round_trip_and_delete():
    from audioldm_with_lora_amd import lora as plora
    u = _tiny()
    pm, ads = _two(u)
    sd = pm.state_dict()
    q = "base_model.model.down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"
    k = "base_model.model.down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_k"
    assert f"{q}.lora_A.a.weight" in sd and f"{q}.lora_B.b.weight" in sd and f"{q}.base_layer.weight" in sd      # peft's key layout
    assert f"{k}.lora_A.a.weight" in sd and f"{k}.lora_A.b.weight" not in sd          # b does not target to_k: no entry
    assert tuple(sd[f"{q}.lora_A.a.weight"].shape)[0] == 4 and tuple(sd[f"{q}.lora_A.b.weight"].shape)[0] == 2
    assert pm.peft_config["b"].r == 2 and pm.peft_config["b"].lora_alpha == 2 and pm.peft_config["a"].lora_alpha == 8
    m = u.get_submodule(q[len("base_model.model."):])
    assert m.scale == {"a": 2.0, "b": 1.0} and m.rank == {"a": 4, "b": 2}
    for n in "ab":                                                       # what was loaded is what the restatement helper made
        for name, (A, B) in ads[n]["tensors"].items():
            assert torch.equal(sd[f"base_model.model.{name}.lora_A.{n}.weight"], A) and torch.equal(sd[f"base_model.model.{name}.lora_B.{n}.weight"], B)
    # saved form -> load under another name: the tensors exactly
    saved = plora.get_peft_model_state_dict(pm, adapter_name="b")
    assert set(saved) == set(mar.peft_state_dict(ads["b"])) and all(".b." not in key for key in saved)
    nkeys = len(sd)
    pm.load_adapter(saved, "b2")
    # the diffusers form loads to the same tensors
    pm.load_adapter(plora.convert_state_dict_to_diffusers(saved), "b3")
    sd = pm.state_dict()
    for key, v in saved.items():
        for n in ("b2", "b3"):
            assert torch.equal(sd[key.replace(".weight", f".{n}.weight")], v)
    assert pm.peft_config["b2"].r == 2 and sorted(pm.peft_config) == ["a", "b", "b2", "b3"]
    assert plora.get_peft_model_state_dict(pm) == {}                     # there is no adapter called "default" here
    # delete removes exactly its keys
    before = set(sd)
    pm.delete_adapter("b2")
    after = set(pm.state_dict())
    assert before - after == {key.replace(".weight", ".b2.weight") for key in saved} and not after - before
    pm.delete_adapter("b3")
    assert len(pm.state_dict()) == nkeys and u.lora_adapters() == ["a", "b"]
    with pytest.raises(ValueError):
        pm.delete_adapter("nope")
    with pytest.raises(ValueError):
        pm.add_adapter("a", _cfg(ads["a"]))


def test_adapter_file_forms(tmp_path):
    """a local .safetensors file, a directory with adapter_config.json (lora_alpha from it), a .bin file"""
    import json
    from safetensors.torch import save_file
    from audioldm_with_lora_amd import lora as plora
    u = _tiny()
    ad = mar.make_adapter(u, 2, 6, ("to_q", "to_v"), seed=7)
    sd = {k: v.contiguous() for k, v in mar.peft_state_dict(ad).items()}
    f = tmp_path / "one.safetensors"
    save_file(sd, str(f))
    d = tmp_path / "dir"
    d.mkdir()
    save_file(sd, str(d / "adapter_model.safetensors"))
    (d / "adapter_config.json").write_text(json.dumps({"r": 2, "lora_alpha": 6}))
    torch.save(sd, str(tmp_path / "two.bin"))
    pm = plora.PeftModel(u, None)
    pm.load_adapter(str(f), "file")
    pm.load_adapter(str(d), "dir")
    pm.load_adapter(str(tmp_path / "two.bin"), "bin")
    assert pm.peft_config["file"].lora_alpha == 2 and pm.peft_config["dir"].lora_alpha == 6       # else = r / from adapter_config.json
    got = pm.state_dict()
    for key, v in sd.items():
        for n in ("file", "dir", "bin"):
            assert torch.equal(got[key.replace(".weight", f".{n}.weight")], v)


def _unpack(pw):
    return pw.lora_a.float(), pw.lora_b.float()


def test_packed_layout_matches_the_documented_one():
    from audioldm_with_lora_amd import ops
    u = _tiny()
    pm, ads = _two(u)
    layout = u.lora_layout()
    assert layout == {"a": (0, 12), "b": (12, 4)}                        # widths: a = 3 x 4 in the q | k | v GEMM, b = 2 + 2
    bf = lambda t: t.to(torch.bfloat16).float()
    name = "down_blocks.1.attentions.0.transformer_blocks.0.attn1"
    attn = u.get_submodule(name)
    c = attn.to_q.in_features
    g = torch.Generator().manual_seed(1)
    gate = torch.zeros(32)
    gate[0:12], gate[12:16] = 0.75, -1.5
    # q | k | v GEMM (no LayerNorm fold here: pack_linear), parts in module order with their adapters
    pw = ops.pack_linear(torch.randn(3 * c, c, generator=g), None)
    parts = [(i * c, c, A, B, s, n) for i, m in enumerate((attn.to_q, attn.to_k, attn.to_v)) for n, A, B, s in m.parts()]
    ops.attach_lora(pw, parts, layout)
    A_cat, B_ext = _unpack(pw)
    assert pw.Rp == 32 and pw.ranks_used == 16 and tuple(A_cat.shape) == (32, pw.Kpad) and tuple(B_ext.shape) == (3 * c, 32)
    want = torch.zeros(3 * c, pw.Kpad)
    for i, leaf in enumerate(("to_q", "to_k", "to_v")):
        for n, gn in (("a", 0.75), ("b", -1.5)):
            if f"{name}.{leaf}" in ads[n]["tensors"]:
                A, B = ads[n]["tensors"][f"{name}.{leaf}"]
                s = ads[n]["alpha"] / ads[n]["r"]
                want[i * c:(i + 1) * c, :c] += gn * (bf(B * s) @ bf(A))          # to bf16 rounding of the operands
    assert torch.allclose((B_ext * gate[None, :]) @ A_cat, want, rtol=0, atol=1e-6)
    # the out-projection: each adapter at the START of its own block, the rest of the block zero
    pwo = ops.pack_linear(torch.randn(c, c, generator=g), None)
    ops.attach_lora(pwo, [(0, c, A, B, s, n) for n, A, B, s in attn.to_out[0].parts()], layout)
    A_o, B_o = _unpack(pwo)
    Ao, Bo = ads["a"]["tensors"][f"{name}.to_out.0"]
    assert torch.equal(A_o[0:4, :c], bf(Ao)) and torch.equal(B_o[:, 0:4], bf(Bo * 2.0)) and not A_o[4:].any() and not B_o[:, 4:].any()
    assert pwo.ranks_used == 4


def test_single_adapter_packing_is_the_sequential_one():
    """one adapter: columns 0 .. combined rank - 1 in part order, A rounded to bf16, B pre-scaled then rounded; with the folded LayerNorm
    A' = A diag(gamma), sA = row sums of the rounded A', cA = A beta -- pinned against values computed here"""
    from audioldm_with_lora_amd import ops
    g = torch.Generator().manual_seed(2)
    c, r = 64, 4
    w = torch.randn(3 * c, c, generator=g)
    gm, bt = torch.randn(c, generator=g) * 0.3 + 1, torch.randn(c, generator=g) * 0.2
    As = [torch.randn(r, c, generator=g) / r for _ in range(3)]
    Bs = [torch.randn(c, r, generator=g) * 0.05 for _ in range(3)]
    sc = [1.5 * 0.3, 1.5, 1.5]
    A_want, B_want = torch.zeros(32, c, dtype=torch.bfloat16), torch.zeros(3 * c, 32, dtype=torch.bfloat16)
    sa, ca = torch.zeros(32), torch.zeros(32)
    for i in range(3):
        Ap = (As[i] * gm[None, :]).to(torch.bfloat16)
        A_want[i * r:(i + 1) * r] = Ap
        sa[i * r:(i + 1) * r], ca[i * r:(i + 1) * r] = Ap.float().sum(1), As[i] @ bt
        B_want[i * c:(i + 1) * c, i * r:(i + 1) * r] = (Bs[i] * sc[i]).to(torch.bfloat16)
    for parts, layout in (([(i * c, c, As[i], Bs[i], sc[i]) for i in range(3)], None),
                          ([(i * c, c, As[i], Bs[i], sc[i], "default") for i in range(3)], {"default": (0, 12)})):
        pw = ops.pack_linear_ln(w, None, gm, bt)
        ops.attach_lora(pw, parts, layout)
        assert pw.Rp == 32 and pw.ranks_used == 12
        assert torch.equal(pw.lora_a, A_want) and torch.equal(pw.lora_b, B_want)
        assert torch.equal(pw.ln_sa, sa) and torch.equal(pw.ln_ca, ca)
    # and through the model: one adapter called "default" gives the layout {default: (0, 12)}
    from audioldm_with_lora_amd import lora as plora
    u = _tiny()
    plora.get_peft_model(u, plora.LoraConfig(r=4, lora_alpha=8, target_modules=list(mar.TARGETS4), init_lora_weights="gaussian"))
    assert u.lora_layout() == {"default": (0, 12)} and u.routing_is_plain() and u.device_gate(None, 4) is None


def test_gate_table():
    u = _tiny()
    pm, _ = _two(u)
    A, B = slice(0, 12), slice(12, 16)
    t = u.gate_table(["a", "b", "__base__", {"a": 0.5, "b": 0.25}, ["a", "b"]], 5)
    assert t.dtype == torch.float32 and tuple(t.shape) == (5, 32)
    want = torch.zeros(5, 32)
    want[0, A] = 1
    want[1, B] = 1
    want[3, A], want[3, B] = 0.5, 0.25
    want[4, A], want[4, B] = 1, 1
    assert torch.equal(t, want)
    # None = the active adapters (peft: the first one until set_adapter) with their set weights, for every sample
    assert pm.active_adapters == ["a"] and torch.equal(u.gate_table(None, 2), want[[0, 0]])
    pm.set_adapter(["a", "b"], [0.5, 2.0])
    assert pm.active_adapters == ["a", "b"] and not u.routing_is_plain()
    t = u.gate_table(None, 3)
    assert torch.equal(t[:, A], torch.full((3, 12), 0.5)) and torch.equal(t[:, B], torch.full((3, 4), 2.0)) and not t[:, 16:].any()
    t = u.gate_table(["b", ["a"], {"b": 1.0}], 3)                        # a bare name carries its set weight, a dict its own
    assert float(t[0, 12]) == 2.0 and float(t[1, 0]) == 0.5 and float(t[2, 12]) == 1.0
    with pm.disable_adapter():
        assert not u.gate_table(None, 2).any() and not u.lora_enabled
    assert u.lora_enabled
    # repetition over num_waveforms_per_prompt like the prompt embeddings, then the CFG doubling [uncond; cond]
    t = u.gate_table(["a", "__base__"], 8, num_waveforms_per_prompt=2, do_classifier_free_guidance=True)
    rows = [0.5, 0.5, 0.0, 0.0]
    assert [float(v) for v in t[:, 0]] == rows + rows and torch.equal(t[:4], t[4:])
    for bad, exc in ((["a", "nope"], ValueError), (["a"], ValueError), ("a", ValueError), ([{"a": float("nan")}, "a"], ValueError),
                     ([{"a": float("inf")}, "a"], ValueError)):
        with pytest.raises(exc):
            u.gate_table(bad, 2)
    with pytest.raises(ValueError):
        pm.set_adapter("a", float("inf"))
    with pytest.raises(ValueError):
        pm.set_adapter("nope")
    with pytest.raises(ValueError):
        u.gate_table(["a"] * 3, 6, num_waveforms_per_prompt=4)
    # set_adapter and weights never repack
    v = u.plan_version
    pm.set_adapter("b")
    assert u.plan_version == v
    pm.delete_adapter("b")
    assert u.plan_version == v + 1 and pm.active_adapters == []          # (the active adapter is gone: base model until set_adapter)


def test_capacity_is_checked_when_the_adapter_is_added():
    from audioldm_with_lora_amd import lora as plora
    from audioldm_with_lora_amd._lib import AldmError
    u = _tiny()
    cfg = plora.LoraConfig(r=4, lora_alpha=8, target_modules=list(mar.TARGETS4), init_lora_weights="gaussian")
    pm = plora.get_peft_model(u, cfg, adapter_name="a")
    pm.add_adapter("b", cfg)
    assert u.lora_layout() == {"a": (0, 12), "b": (12, 12)}              # 24 of the 32 columns of the q | k | v GEMM
    nkeys = len(pm.state_dict())
    with pytest.raises(AldmError, match=r"32.*a=12, b=12, c=12"):
        pm.add_adapter("c", cfg)
    assert len(pm.state_dict()) == nkeys and u.lora_adapters() == ["a", "b"] and "c" not in pm.peft_config   # nothing was built
    with pytest.raises(AldmError):
        pm.load_adapter(mar.peft_state_dict(mar.make_adapter(_tiny(), 4, 8, mar.TARGETS4, seed=1)), "c")
    # eight adapters of the reference's kind (r = 2 on to_q + to_v) fit exactly; the ninth does not
    u = _tiny()
    ref_cfg = plora.LoraConfig(r=2, lora_alpha=2, target_modules=["to_q", "to_v"], init_lora_weights="gaussian")
    pm = plora.get_peft_model(u, ref_cfg, adapter_name="g0")
    for i in range(1, 8):
        pm.add_adapter(f"g{i}", ref_cfg)
    assert u.lora_layout()["g7"] == (28, 4)
    with pytest.raises(AldmError):
        pm.add_adapter("g8", ref_cfg)


def test_trainer_refuses_several_adapters():
    from audioldm_with_lora_amd import training
    from audioldm_with_lora_amd._lib import AldmError
    u = _tiny()
    pm, _ = _two(u)
    with pytest.raises(AldmError, match="one adapter"):
        training._check_single_adapter(u)
    pm.delete_adapter("b")
    training._check_single_adapter(u)
    pm.set_adapter("a", 0.5)
    with pytest.raises(AldmError, match="routing"):
        training._check_single_adapter(u)


def test_inference_script_adapters_spec():
    from audioldm_with_lora_amd.script.inference import parse_adapters
    assert parse_adapters("boom_bap,trap:0.7,base,a:0.5+b:0.5") == ["boom_bap", {"trap": 0.7}, "__base__", {"a": 0.5, "b": 0.5}]
    assert parse_adapters(" a , __base__ ") == ["a", "__base__"]
    assert parse_adapters("a+b:2") == [{"a": 1.0, "b": 2.0}]
    for bad in ("a,,b", "a:x", "base+a", "a:nan", ":0.5", ""):
        with pytest.raises(ValueError):
            parse_adapters(bad)


def test_ctypes_mirrors_end_with_the_gate_fields():
    from audioldm_with_lora_amd import _lib
    for cls in (_lib.IgemmArgs, _lib.PgemmArgs):
        names = [f[0] for f in cls._fields_]
        assert names[-2:] == ["lora_gate", "gate_rows"]
        assert cls._fields_[-2][1] is ctypes.c_void_p and cls._fields_[-1][1] is ctypes.c_int
        assert getattr(cls, "lora_gate").offset > max(getattr(cls, n).offset for n in names[:-2])
        a = cls()
        assert not a.lora_gate and a.gate_rows == 0                      # zero-initialised = ungated
    assert names.index("vt_dual") == len(names) - 3                      # aldm_pgemm_t: appended right behind its former last field
    assert [f[0] for f in _lib.IgemmArgs._fields_][-3] == "xcd_map"
    for sym in ("aldm_attn_block64_gated", "aldm_attn_block64_fp8_gated", "aldm_attn_block256_gated"):
        assert len(_lib.PROTOTYPES[sym][1]) == len(_lib.PROTOTYPES["aldm_attn_block64"][1]) + 1
