"""GPU: the training recipe around the flat LoRA buffer -- gradient-norm clipping (aldm_sumsq_flat / aldm_clip_flat /
aldm_adamw_flat_clip), min-SNR-gamma loss weighting (aldm_mse_grad_snr), gradient accumulation (aldm_accum_flat) and checkpoint
resume -- from the kernels up to LoraTrainer and the accelerate-shaped facade.  The oracle is torch on the CPU
(torch.optim.AdamW, torch.nn.utils.clip_grad_norm_) and the restatement of diffusers' min-SNR weighting in
tests/train_recipe_restatement.py.  Every model is oracle.configs.tiny_unet() on latents [2, 8, 16, 16]."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_recipe_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _rel(a, b):
    import conftest
    return conftest.record(float((a.double() - b.double()).norm() / b.double().norm()))


def _setup(seed=0, r=4, targets=("to_q", "to_k", "to_v", "to_out.0"), batch=2, lr=1e-3, **trainer_kw):
    """(oracle peft model, product UNet, oracle scheduler, trainer, (latents, noise, timesteps, prompt_embeds)) with equal weights"""
    from audioldm_with_lora_amd import lora as plora
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from audioldm_with_lora_amd.training import LoraTrainer
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from oracle import configs
    from oracle import lora as olora
    from oracle.ddim import DDIMScheduler as ODDIM
    from oracle.unet import UNet2DConditionModel as OUNet
    cfg = configs.tiny_unet()
    torch.manual_seed(seed)
    ref = OUNet(**cfg)
    mine = UNet2DConditionModel(**cfg)
    mine.load_state_dict(ref.state_dict())
    pref = olora.get_peft_model(ref, olora.LoraConfig(r=r, lora_alpha=r, target_modules=list(targets), init_lora_weights="gaussian"))
    pmine = plora.get_peft_model(mine, plora.LoraConfig(r=r, lora_alpha=r, target_modules=list(targets), init_lora_weights="gaussian"))
    g = torch.Generator().manual_seed(seed + 1)
    sd = pref.state_dict()
    for k in sd:
        if "lora_B" in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
    pref.load_state_dict(sd)
    pmine.load_state_dict(sd)
    mine.cuda()
    lat = torch.randn(batch, 8, 16, 16, generator=g) * 0.92
    noise = torch.randn(batch, 8, 16, 16, generator=g)
    t = torch.randint(0, 1000, (batch,), generator=g)
    emb = F.normalize(torch.randn(batch, 64, generator=g), dim=-1)
    trainer = LoraTrainer(mine, DDIMScheduler(), lr=lr, weight_decay=1e-2, max_train_steps=100, **trainer_kw)
    return pref, mine, ODDIM(), trainer, (lat, noise, t, emb)


def _oracle_grads(pref, loss):
    for p in pref.parameters():
        p.grad = None
    loss.backward()
    return {n.replace("base_model.model.", ""): p.grad for n, p in pref.named_parameters() if p.grad is not None}


def _flat_of(want, flat):
    """the oracle's per-tensor gradients laid out like the product's flat buffer"""
    return torch.cat([want[n].reshape(-1) for n in flat.names])


# ---- 1. norm and clip kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10007, 1])
def test_sumsq_flat_and_clip_flat_match_torch(n):
    """n = 10007: odd, so the 16-byte body, the scalar tail and the grid-stride remainder all run; n = 1: tail only."""
    from audioldm_with_lora_amd import ops
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    want = float(torch.linalg.vector_norm(x.double()))
    xd = x.cuda()
    p1 = ops.sumsq_flat(xd).clone()
    p2 = ops.sumsq_flat(xd)
    assert p1.numel() == ops.SUMSQ_PARTS and torch.equal(p1, p2)              # no float atomics: bitwise reproducible
    assert abs(math.sqrt(float(p1.double().sum())) - want) < 1e-5 * want
    for factor, clips in ((0.25, True), (4.0, False)):
        max_norm = factor * want
        p = torch.nn.Parameter(x.clone())
        p.grad = x.clone()
        ref_norm = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
        gd, norm = x.cuda(), torch.zeros(1, device="cuda")
        ops.clip_flat(gd, ops.sumsq_flat(gd), max_norm, norm)
        print(f"n={n} factor={factor}: norm {float(norm):.8g} torch {ref_norm:.8g} float64 {want:.8g}")
        assert abs(float(norm) - want) < 1e-5 * want
        torch.testing.assert_close(gd.cpu(), p.grad, rtol=2e-6, atol=0)
        assert torch.equal(gd.cpu(), x) != clips                                 # left bitwise untouched when the norm is below max_norm


# ---- 2. adamw_flat_clip --------------------------------------------------------------------------------------------------------
def test_adamw_flat_clip_matches_clip_grad_norm_and_torch_adamw():
    from audioldm_with_lora_amd import ops
    n = 10007
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=g)
    scales = [0.5, 2.0, 1.0, 3.0, 0.25]                     # gradient norms ~ sqrt(n) * scale around max_norm = 1.5 sqrt(n)
    grads = [torch.randn(n, generator=g) * s for s in scales]
    max_norm = 1.5 * math.sqrt(n)
    clipped = [float(torch.linalg.vector_norm(x)) > max_norm for x in grads]
    assert clipped == [False, True, False, True, False]                           # some steps clip and some do not
    p, m, v = p0.clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    norm = torch.zeros(1, device="cuda")
    ref = R.clipped_adamw_steps(p0, grads, max_norm, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    for step, (grad, (p_ref, norm_ref)) in enumerate(zip(grads, ref), start=1):
        g4 = (grad * 4).cuda()                               # gradients arrive x4 and go in with grad_scale = 0.25:
        ops.adamw_flat_clip(p, g4, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step, ops.sumsq_flat(g4), max_norm, norm, grad_scale=0.25)
        print(f"step {step}: norm {float(norm):.8g} torch {norm_ref:.8g}")
        assert abs(float(norm) - norm_ref) < 1e-5 * norm_ref                      # ... the norm is the SCALED gradient's
        torch.testing.assert_close(p.cpu(), p_ref, rtol=2e-6, atol=2e-7)


# ---- 3. mse_grad_snr -----------------------------------------------------------------------------------------------------------
def test_mse_grad_snr_matches_the_restatement():
    from audioldm_with_lora_amd import ops
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    B, per, gamma = 3, 280, 5.0                              # 840 elements: 256-thread blocks straddle the sample boundaries
    ac = DDIMScheduler().alphas_cumprod.float()
    t = torch.tensor([0, 500, 999])
    snr = R.compute_snr(ac, t)
    assert float(snr[0]) > 100 * gamma and float(snr[2]) < gamma / 100         # both branches of min(snr, gamma) are hit
    g = torch.Generator().manual_seed(3)
    pred, tgt = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g)
    loss = torch.zeros(1, device="cuda")
    dp = ops.mse_grad_snr(pred.cuda(), tgt.cuda(), loss, ac.cuda(), t.cuda(), gamma)
    want_loss = float(R.min_snr_loss(pred.double(), tgt.double(), ac.double(), t, gamma))
    w = R.min_snr_weights(ac.double(), t, gamma)
    want_dp = 2.0 * w[:, None] * (pred.double() - tgt.double()) / (B * per)
    print(f"loss {float(loss):.8g} restatement {want_loss:.8g}")
    assert abs(float(loss) - want_loss) < 1e-5 * want_loss
    assert dp.dtype == torch.bfloat16 and _rel(dp.float().cpu(), want_dp) < 4e-3
    # every weight 1: the plain kernel's gradient, bit for bit
    big = 1e30
    assert torch.equal(R.min_snr_weights(ac, t, big), torch.ones(B))
    l1, l0 = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    d1 = ops.mse_grad_snr(pred.cuda(), tgt.cuda(), l1, ac.cuda(), t.cuda(), big)
    d0 = ops.mse_grad(pred.cuda(), tgt.cuda(), l0)
    assert torch.equal(d1, d0)
    assert abs(float(l1) - float(l0)) < 1e-6 * float(l0)


# ---- 4. trainer with snr_gamma -------------------------------------------------------------------------------------------------
def test_trainer_min_snr_loss_and_gradients_match_oracle_autograd():
    pref, mine, osched, trainer, (lat, noise, _, emb) = _setup(snr_gamma=5.0)
    t = torch.tensor([10, 900])
    w = R.min_snr_weights(osched.alphas_cumprod, t, 5.0)
    assert float(w[0]) < 1.0 and float(w[1]) == 1.0                              # one sample on each branch
    pred = pref(osched.add_noise(lat, noise, t), t, encoder_hidden_states=None, class_labels=emb)[0]
    loss = R.min_snr_loss(pred, noise, osched.alphas_cumprod, t, 5.0)
    want = _oracle_grads(pref, loss)
    got_loss = float(trainer.loss_and_grads(lat, noise, t, emb))
    print(f"loss {got_loss:.6g} oracle {float(loss):.6g}")
    assert abs(got_loss - float(loss)) < 2e-2 * float(loss) + 1e-4
    f = trainer.flat
    rel = _rel(f.grads[:f.n].cpu(), _flat_of(want, f))
    assert rel < 6e-2, f"flat-gradient relative L2 error {rel:.4g}"


# ---- 5. trainer with max_grad_norm ---------------------------------------------------------------------------------------------
def test_trainer_step_clips_like_clip_grad_norm_and_keeps_the_loss_slot_out_of_the_norm():
    pref, mine, osched, trainer, batch = _setup(seed=2, max_grad_norm=1.0)
    f = trainer.flat
    trainer.loss_and_grads(*batch)                          # no update: only to learn the unclipped norm
    unclipped = float(torch.linalg.vector_norm(f.grads[:f.n].double()))
    assert unclipped > 0
    trainer.max_grad_norm = unclipped / 4
    p0 = f.params.detach().cpu().clone()
    trainer.step(*batch)
    used = f.grads[:f.n].cpu()                               # the gradient the step actually used (atomic scatter order may differ)
    (p_ref, norm_ref), = R.clipped_adamw_steps(p0, [used], trainer.max_grad_norm, lr=trainer.lr(0), betas=(0.9, 0.999),
                                               weight_decay=1e-2, eps=1e-8)
    norm1 = trainer.last_grad_norm.clone()
    print(f"norm {float(norm1):.8g} torch {norm_ref:.8g} max_norm {trainer.max_grad_norm:.8g}")
    assert trainer.last_grad_norm.is_cuda and trainer.last_grad_norm.numel() == 1
    assert abs(float(norm1) - norm_ref) < 1e-5 * norm_ref
    assert norm_ref > 3.9 * trainer.max_grad_norm                                # the step did clip
    torch.testing.assert_close(f.params.detach().cpu(), p_ref, rtol=2e-6, atol=2e-7)
    # the last slot of the buffer is the loss: it must never enter the norm
    f.grads[f.n:].fill_(1.0e4)
    trainer._apply_update(f.grads[f.n:])
    assert torch.equal(trainer.last_grad_norm, norm1)


# ---- 6. accumulation -----------------------------------------------------------------------------------------------------------
def test_accumulated_gradient_is_the_gradient_of_the_concatenated_batch():
    pref, mine, osched, trainer, (lat, noise, t, emb) = _setup(seed=4, batch=4, gradient_accumulation_steps=2, use_graph=False)
    pred = pref(osched.add_noise(lat, noise, t), t, encoder_hidden_states=None, class_labels=emb)[0]
    full = F.mse_loss(pred.float(), noise.float())
    want = _oracle_grads(pref, full)
    f = trainer.flat
    p0 = f.params.clone()
    l0 = float(trainer.step(lat[:2], noise[:2], t[:2], emb[:2]))
    assert trainer.step_count == 0 and torch.equal(f.params, p0)
    l1 = float(trainer.step(lat[2:], noise[2:], t[2:], emb[2:]))
    assert trainer.step_count == 1 and not torch.equal(f.params, p0)
    rel = _rel(f.accum[:f.n].cpu() / 2, _flat_of(want, f))
    assert rel < 6e-2, f"accumulated flat-gradient relative L2 error {rel:.4g}"
    # each call returned its micro-batch's loss; the window's loss slot holds their sum
    assert abs((l0 + l1) / 2 - float(full)) < 2e-2 * float(full) + 1e-4
    assert abs(float(trainer.window_loss) - (l0 + l1) / 2) < 1e-6 * (l0 + l1)


def test_accumulation_steps_every_kth_call_eager_and_graph():
    outs = []
    for use_graph in (False, True):
        pref, mine, osched, trainer, (lat, noise, t, emb) = _setup(seed=5, gradient_accumulation_steps=2, use_graph=use_graph)
        f = trainer.flat
        version = mine.plan_version
        for i in range(6):                                   # two eager warm-ups, one capture, three replays
            before = f.params.clone()
            g = torch.Generator().manual_seed(100 + i)
            trainer.step(lat + 0.01 * i, torch.randn(noise.shape, generator=g), t, emb)
            if i % 2 == 0:
                assert torch.equal(f.params, before), i      # inside the window: bitwise unchanged
            else:
                assert not torch.equal(f.params, before), i
            assert trainer.step_count == (i + 1) // 2 and trainer.micro_step == i + 1
        assert trainer.step_count == 3 and mine.plan_version == version + 3
        assert trainer.lr(trainer.step_count - 1) == (1e-3 - 1e-7) * (1 - 2 / 100) + 1e-7      # the third step ran at lr(2)
        assert (trainer.graph is not None) == use_graph
        outs.append(f.params.clone())
    rel = _rel(outs[1], outs[0])
    assert rel < 1e-3, rel


# ---- 7. the reference-shaped loop through the facade ---------------------------------------------------------------------------
def test_facade_loop_with_accumulation_and_clipping_matches_the_torch_loop():
    from audioldm_with_lora_amd import dp, lora as plora, optim
    from audioldm_with_lora_amd.lora import get_peft_model_state_dict
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from oracle import configs
    from oracle import lora as olora
    from oracle.ddim import DDIMScheduler as ODDIM
    from oracle.unet import UNet2DConditionModel as OUNet
    from transformers.optimization import get_polynomial_decay_schedule_with_warmup
    cfg = configs.tiny_unet()
    torch.manual_seed(0)
    ref, unet = OUNet(**cfg), UNet2DConditionModel(**cfg)
    unet.load_state_dict(ref.state_dict())
    unet.requires_grad_(False); ref.requires_grad_(False)
    conf = dict(r=2, lora_alpha=2, target_modules=["to_q", "to_v"], init_lora_weights="gaussian")
    pref, punet = olora.get_peft_model(ref, olora.LoraConfig(**conf)), plora.get_peft_model(unet, plora.LoraConfig(**conf))
    g = torch.Generator().manual_seed(1)
    sd = pref.state_dict()
    for k in sd:
        if "lora_B" in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
    pref.load_state_dict(sd); punet.load_state_dict(sd)
    K, bsz, lr0, max_train_steps = 2, 2, 1.0e-3, 20
    data = [dict(latents=torch.randn(bsz, 8, 16, 16, generator=g) * 0.92, noise=torch.randn(bsz, 8, 16, 16, generator=g),
                 timesteps=torch.randint(0, 1000, (bsz,), generator=g),
                 prompt_embeds=F.normalize(torch.randn(bsz, 64, generator=g), dim=-1)) for _ in range(4)]

    osched = ODDIM()
    oparams = [p for p in pref.parameters() if p.requires_grad]

    def oracle_loss(batch):
        noisy = osched.add_noise(batch["latents"], batch["noise"], batch["timesteps"])
        pred = pref(noisy, batch["timesteps"], encoder_hidden_states=None, class_labels=batch["prompt_embeds"])[0]
        return F.mse_loss(pred.float(), batch["noise"].float(), reduction="mean")

    pref.train()
    for batch in data[:K]:                                   # the first window's gradient norm sets the scale of max_norm
        (oracle_loss(batch) / K).backward()
    typical = float(torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in oparams])))
    max_norm = 0.5 * typical
    for p in oparams:
        p.grad = None
    oopt = torch.optim.AdamW(oparams, lr=lr0, betas=(0.9, 0.999), weight_decay=1e-5, eps=1e-08)
    olr = get_polynomial_decay_schedule_with_warmup(oopt, 0, max_train_steps, lr_end=1e-7, power=1.0)
    want_losses, want_norms = [], []
    for i, batch in enumerate(data):
        loss = oracle_loss(batch)
        (loss / K).backward()
        want_losses.append(float(loss))
        if (i + 1) % K == 0:
            want_norms.append(float(torch.nn.utils.clip_grad_norm_(oparams, max_norm)))
            oopt.step(); olr.step(); oopt.zero_grad()
    assert want_norms[0] > max_norm                                              # the clip is active

    acc = dp.Accelerator(gradient_accumulation_steps=K, mixed_precision=None)
    ddim = DDIMScheduler()
    unet.to(acc.device, dtype=torch.float32)
    trainable = [p for p in unet.parameters() if p.requires_grad]               # a real parameter list
    optimizer = optim.AdamW(trainable, lr=lr0, betas=(0.9, 0.999), weight_decay=1e-5, eps=1e-08)
    lr_scheduler = optim.get_scheduler("polynomial", optimizer=optimizer, num_warmup_steps=0,
                                       num_training_steps=max_train_steps * acc.num_processes)
    punet, optimizer, lr_scheduler = acc.prepare(punet, optimizer, lr_scheduler)
    got_losses, got_norms, syncs = [], [], []
    punet.train()
    optimizer.zero_grad()
    for batch in data:
        with acc.accumulate(punet):
            x0, eps = batch["latents"].to(acc.device), batch["noise"].to(acc.device)
            t = batch["timesteps"].to(acc.device).long()
            pred = punet(ddim.add_noise(x0, eps, t), t, encoder_hidden_states=None, class_labels=batch["prompt_embeds"].to(acc.device),
                         return_dict=False)[0]
            loss = F.mse_loss(pred.float(), eps.float(), reduction="mean")
            got_losses.append(float(loss))
            acc.backward(loss)
            if acc.sync_gradients:
                norm = acc.clip_grad_norm_(trainable, max_norm)
                assert norm.is_cuda                                              # a device tensor: no host sync in the call
                got_norms.append(float(norm))
            optimizer.step()
            lr_scheduler.step()
            optimizer.zero_grad()
        syncs.append(acc.sync_gradients)
    assert syncs == [False, True, False, True]
    assert optimizer._step == 2 and lr_scheduler.last_epoch == 2
    print("losses", got_losses, want_losses, "norms", got_norms, want_norms)
    for i, (a, b) in enumerate(zip(got_losses, want_losses)):
        assert abs(a - b) < 2e-2 * b + 1e-4, (i, got_losses, want_losses)
    assert abs(lr_scheduler.get_last_lr()[0] - olr.get_last_lr()[0]) < 1e-12
    want = {k.replace(".default", ""): v for k, v in pref.state_dict().items() if "lora_" in k}
    got = get_peft_model_state_dict(acc.unwrap_model(punet))
    assert set(got) == set(want)
    num = sum(float(((got[k].float().cpu() - want[k]) ** 2).sum()) for k in want)
    den = sum(float((want[k] ** 2).sum()) for k in want)
    assert (num / den) ** 0.5 < 2e-2, (num / den) ** 0.5


def test_clip_grad_norm_keeps_quirk_q1_and_the_torch_loop_for_partial_lists():
    from audioldm_with_lora_amd import dp
    pref, mine, osched, trainer, batch = _setup(seed=6, use_graph=False)
    trainer.loss_and_grads(*batch)
    f = trainer.flat
    before = f.grads.clone()
    acc = dp.Accelerator()
    params = [p for p, _, _ in f._plist]
    spent = iter(params)
    list(spent)
    assert float(acc.clip_grad_norm_(spent, 1e-9)) == 0.0 and torch.equal(f.grads, before)     # exhausted iterator: clips nothing
    # a part of the parameters: the per-tensor loop, on those tensors only
    part = params[:3]
    want = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in part)))
    # the oracle is torch's own utility on CPU copies: these gradients are small, so the 1e-6 in max_norm / (total + 1e-6) shows
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in part]
    for c, p in zip(cpu, part):
        c.grad = p.grad.detach().cpu().clone()
    ref = float(torch.nn.utils.clip_grad_norm_(cpu, want / 2))
    got = float(acc.clip_grad_norm_(part, want / 2))
    print(f"partial-list norm {got:.8g} torch {ref:.8g} float64 {want:.8g}")
    assert abs(got - want) < 1e-5 * want and abs(ref - want) < 1e-5 * want
    for c, p in zip(cpu, part):
        assert not torch.equal(p.grad.cpu(), before[f.offset_of(p):f.offset_of(p) + p.numel()].view(p.shape).cpu())    # it did clip
        torch.testing.assert_close(p.grad.cpu(), c.grad, rtol=2e-6, atol=0)
    assert torch.equal(params[3].grad, before[f.offset_of(params[3]):f.offset_of(params[3]) + params[3].numel()].view(params[3].shape))


# ---- 8. resume -----------------------------------------------------------------------------------------------------------------
def test_save_state_load_state_resumes_the_run(tmp_path):
    from audioldm_with_lora_amd import dp

    def batches(lat, noise, t, emb):
        out = []
        for i in range(5):
            g = torch.Generator().manual_seed(200 + i)
            out.append((lat + 0.01 * i, torch.randn(noise.shape, generator=g), t, emb))
        return out

    pref, mine, osched, tr_a, batch = _setup(seed=7, max_grad_norm=1.0)
    data = batches(*batch)
    for b in data[:3]:
        tr_a.step(*b)
    acc = dp.Accelerator()
    ckpt = str(tmp_path / "checkpoint-3")
    acc.save_state(ckpt, tr_a)
    saved = {k: getattr(tr_a.flat, k).detach().cpu().clone() for k in ("params", "m", "v")}
    for b in data[3:]:
        tr_a.step(*b)
    a = tr_a.flat.params.detach().cpu().clone()

    pref, mine_b, osched, tr_b, _ = _setup(seed=7, max_grad_norm=1.0)
    with torch.no_grad():
        tr_b.flat.params.add_(1.0)                           # whatever the fresh adapter holds, the checkpoint replaces it
    version = mine_b.plan_version
    dp.Accelerator().load_state(ckpt, tr_b)
    for k in ("params", "m", "v"):
        assert torch.equal(getattr(tr_b.flat, k).detach().cpu(), saved[k]), k
    assert tr_b.step_count == 3 and tr_b.micro_step == 3 and tr_b.lr(tr_b.step_count) == tr_a.lr(3)
    assert tr_b.flat.intact() and mine_b.plan_version > version
    for b in data[3:]:
        tr_b.step(*b)
    assert tr_b.step_count == tr_a.step_count == 5
    rel = _rel(tr_b.flat.params.detach().cpu(), a)
    assert rel < 1e-3, rel
    assert float((a - saved["params"]).norm()) > 0
