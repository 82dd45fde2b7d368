"""Host side of the training recipe (no GPU): the accumulation window of the accelerate-shaped facade, the min-SNR restatement
(tests/train_recipe_restatement.py) on its own, the LR schedule's state round trip and the driver's new options."""
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_recipe_restatement as R  # noqa: E402


def test_accelerator_accumulation_window_raises_sync_gradients_on_every_kth_entry():
    from audioldm_with_lora_amd import dp
    acc = dp.Accelerator(gradient_accumulation_steps=4)
    assert acc.gradient_accumulation_steps == 4
    seen = []
    for _ in range(8):
        with acc.accumulate(None):
            seen.append(acc.sync_gradients)
    assert seen == [False, False, False, True, False, False, False, True]
    one = dp.Accelerator()                                       # K = 1: always true, as before
    for _ in range(3):
        with one.accumulate(None):
            assert one.sync_gradients


def test_prepared_optimizer_and_schedule_wait_for_sync_gradients():
    from audioldm_with_lora_amd import dp, optim
    acc = dp.Accelerator(gradient_accumulation_steps=2)
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.AdamW([p], lr=1e-3)
    sch = optim.get_scheduler("polynomial", optimizer=opt, num_warmup_steps=0, num_training_steps=10)
    opt, sch = acc.prepare(opt, sch)
    epochs = []
    for _ in range(4):
        with acc.accumulate(None):
            p.grad = torch.ones(3)
            sch.step()
            opt.zero_grad()
            epochs.append((sch.last_epoch, p.grad is None))
    assert epochs == [(0, False), (1, True), (1, False), (2, True)]


def test_min_snr_weights_follow_the_two_branches():
    ac = R.scaled_linear_alphas_cumprod()
    t = torch.tensor([0, 100, 500, 900, 999])
    gamma = 5.0
    snr = R.compute_snr(ac, t)
    assert float(snr[0]) > 100 * gamma and float(snr[-1]) < gamma / 100        # both branches are hit
    w = R.min_snr_weights(ac, t, gamma)
    below = snr <= gamma
    assert below.any() and (~below).any()
    assert torch.equal(w[below], torch.ones(int(below.sum())))
    torch.testing.assert_close(w[~below], gamma / snr[~below], rtol=1e-6, atol=0)
    assert float(w.max()) <= 1.0 and float(w.min()) > 0
    # snr is abar / (1 - abar)
    torch.testing.assert_close(snr, ac[t] / (1 - ac[t]), rtol=1e-5, atol=0)


def test_min_snr_loss_is_plain_mse_when_gamma_is_infinite():
    ac = R.scaled_linear_alphas_cumprod()
    t = torch.tensor([0, 250, 500, 999])
    assert torch.equal(R.min_snr_weights(ac, t, math.inf), torch.ones(4))
    g = torch.Generator().manual_seed(0)
    # small integers, power-of-two sizes: every square, sum and mean below is exact in fp32, so "equal" can be asked for exactly
    pred = torch.randint(-8, 9, (4, 2, 8, 8), generator=g).float()
    target = torch.randint(-8, 9, (4, 2, 8, 8), generator=g).float()
    assert torch.equal(R.min_snr_loss(pred, target, ac, t, math.inf), F.mse_loss(pred, target))
    # ... and on real-valued inputs the two differ by summation order only
    pred, target = torch.randn(4, 8, 16, 16, generator=g), torch.randn(4, 8, 16, 16, generator=g)
    torch.testing.assert_close(R.min_snr_loss(pred, target, ac, t, math.inf), F.mse_loss(pred, target), rtol=1e-6, atol=0)
    # a finite gamma weighs the low-noise samples down
    assert float(R.min_snr_loss(pred, target, ac, t, 5.0)) < float(F.mse_loss(pred, target))


def test_polynomial_lr_state_round_trip():
    from audioldm_with_lora_amd import optim
    def make():
        opt = optim.AdamW([torch.nn.Parameter(torch.zeros(2))], lr=1e-3)
        return opt, optim.get_scheduler("polynomial", optimizer=opt, num_warmup_steps=0, num_training_steps=20)
    opt, sch = make()
    for _ in range(7):
        sch.step()
    sd = sch.state_dict()
    opt2, sch2 = make()
    sch2.load_state_dict(sd)
    assert sch2.last_epoch == 7 and sch2.get_last_lr() == sch.get_last_lr()
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] == sch.lr_at(7)
    sch.step(); sch2.step()
    assert sch2.get_last_lr() == sch.get_last_lr()


def test_adamw_state_round_trip_outside_a_flat_buffer():
    from audioldm_with_lora_amd import optim
    p = torch.nn.Parameter(torch.zeros(2))
    opt = optim.AdamW([p], lr=1e-3)
    opt._step = 3
    opt.state[id(p)] = dict(m=torch.tensor([1.0, 2.0]), v=torch.tensor([3.0, 4.0]))
    opt.param_groups[0]["lr"] = 5e-4
    q = torch.nn.Parameter(torch.zeros(2))
    opt2 = optim.AdamW([q], lr=1e-3)
    opt2.load_state_dict(opt.state_dict())
    assert opt2._step == 3 and opt2.param_groups[0]["lr"] == 5e-4 and opt2.param_groups[0]["params"] == [q]
    assert torch.equal(opt2.state[id(q)]["m"], torch.tensor([1.0, 2.0])) and torch.equal(opt2.state[id(q)]["v"], torch.tensor([3.0, 4.0]))


def test_train_driver_parser_has_the_recipe_options_off_by_default():
    from audioldm_with_lora_amd.script import train
    a = train.build_parser().parse_args([])
    assert a.gradient_accumulation_steps == 1 and a.max_grad_norm is None and a.snr_gamma is None and a.resume_from_checkpoint is None
    a = train.build_parser().parse_args(["--gradient-accumulation-steps", "4", "--max-grad-norm", "1.0", "--snr-gamma", "5",
                                         "--resume-from-checkpoint", "out/checkpoint-100"])
    assert (a.gradient_accumulation_steps, a.max_grad_norm, a.snr_gamma, a.resume_from_checkpoint) == (4, 1.0, 5.0, "out/checkpoint-100")
