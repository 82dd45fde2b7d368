"""GPU: gradient accumulation under data parallelism, two ranks on one GPU over gloo (the pattern of tests/test_gpu_dp_two_ranks.py).

World 2 x gradient_accumulation_steps 2 x micro-batch 1 sees the same four samples per optimiser step as one process with K = 1 on
the batch of 4, and must land on the same parameters: the window is summed locally (aldm_accum_flat), ONE all-reduce per optimiser
step carries it, and AdamW runs with grad_scale = 1 / (world K)."""
import os
import socket
import time

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

STEPS, GLOBAL_B, K, LR0, MAX_STEPS = 2, 4, 2, 1.0e-3, 20
CHILD_TIMEOUT = 240             # seconds for each child process (torch import, engine construction, four tiny steps)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _unet(seed=0):
    from audioldm_with_lora_amd import lora as plora
    from audioldm_with_lora_amd.unet import UNet2DConditionModel
    from oracle import configs
    torch.manual_seed(seed)
    unet = UNet2DConditionModel(**configs.tiny_unet())
    unet.requires_grad_(False)
    punet = plora.get_peft_model(unet, plora.LoraConfig(r=2, lora_alpha=2, target_modules=["to_q", "to_k", "to_v", "to_out.0"],
                                                        init_lora_weights="gaussian"))
    g = torch.Generator().manual_seed(seed + 1)
    sd = punet.state_dict()
    for k in sd:
        if "lora_B" in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
    punet.load_state_dict(sd)
    return punet, unet


def _data():
    g = torch.Generator().manual_seed(11)
    n = STEPS * GLOBAL_B
    return dict(latents=torch.randn(n, 8, 16, 16, generator=g) * 0.92, noise=torch.randn(n, 8, 16, 16, generator=g),
                timesteps=torch.randint(0, 1000, (n,), generator=g), prompt_embeds=F.normalize(torch.randn(n, 64, generator=g), dim=-1))


def _run_trainer(rank, world, k):
    """LoraTrainer.step over this rank's share of every global batch, one micro-batch of GLOBAL_B / (world k) samples per call"""
    import torch.distributed as dist
    from audioldm_with_lora_amd.scheduler import DDIMScheduler
    from audioldm_with_lora_amd.training import LoraTrainer
    punet, unet = _unet()
    unet.to("cuda")
    tr = LoraTrainer(unet, DDIMScheduler(), lr=LR0, max_train_steps=MAX_STEPS, use_graph=False, gradient_accumulation_steps=k)
    calls = [0]
    real = dist.all_reduce

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)
    dist.all_reduce = counted                                   # the trainer calls it through the module
    try:
        d, losses, per = _data(), [], GLOBAL_B // (world * k)
        for s in range(STEPS):
            for j in range(k):
                lo = s * GLOBAL_B + (rank * k + j) * per
                idx = slice(lo, lo + per)
                losses.append(float(tr.step(d["latents"][idx], d["noise"][idx], d["timesteps"][idx], d["prompt_embeds"][idx])))
    finally:
        dist.all_reduce = real
    return dict(params=tr.flat.params.detach().cpu(), losses=losses, lr=tr.lr(tr.step_count), step_count=tr.step_count,
                micro_step=tr.micro_step, all_reduces=calls[0])


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    import torch.distributed as dist
    from audioldm_with_lora_amd import dp
    assert dp.init_from_env(backend="gloo") == world            # gloo over CUDA tensors: both ranks live on the one GPU of this box
    res = _run_trainer(rank, world, K)
    torch.save(res, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def _spawn(tmp_path):
    out = str(tmp_path / "accum.pt")
    ctx = mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=False)
    deadline = time.monotonic() + CHILD_TIMEOUT
    while not ctx.join(timeout=2):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"a rank did not finish within {CHILD_TIMEOUT} s")
    return torch.load(out + ".0"), torch.load(out + ".1")


def test_two_ranks_accumulating_two_micro_batches_equal_one_rank_on_the_whole_batch(tmp_path):
    r0, r1 = _spawn(tmp_path)
    one = _run_trainer(0, 1, 1)                                 # this process: no process group, K = 1, the batch of 4
    assert r0["step_count"] == r1["step_count"] == one["step_count"] == STEPS and r0["micro_step"] == STEPS * K
    # one collective per OPTIMISER step, none inside the window
    assert r0["all_reduces"] == r1["all_reduces"] == STEPS and one["all_reduces"] == 0
    assert torch.equal(r0["params"], r1["params"])
    rel = float((r0["params"] - one["params"]).norm() / one["params"].norm())
    assert rel < 1e-3, rel
    # each call returned its own micro-batch's loss: the four of a step average to the whole batch's
    for s in range(STEPS):
        micro = r0["losses"][s * K:(s + 1) * K] + r1["losses"][s * K:(s + 1) * K]
        a, b = sum(micro) / len(micro), one["losses"][s]
        assert abs(a - b) < 2e-3 * abs(b) + 1e-6, (s, micro, one["losses"])
    assert r0["lr"] == r1["lr"] == one["lr"]
