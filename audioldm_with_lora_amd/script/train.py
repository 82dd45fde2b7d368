"""LoRA fine-tuning driver -- MI355X mirror of  script/train/train_audioldm_lora.py:main  [REF train:324-626].

Same structure and the same default hyper-parameters as the reference's hard-coded literals:
base model cvssp/audioldm-s-full-v2, LoRA r=2 / alpha=2 / gaussian init on to_q,to_v [REF train:378-383], AdamW lr 1e-5
betas (0.9, 0.999) wd 1e-5 eps 1e-8 [REF train:396-403], batch 2 per process [REF train:406], polynomial LR with no
warm-up [REF train:438-443], max 97 000 steps, checkpoint every 19 400 steps [REF train:410-411,574-576].
One process per GPU (torchrun); gradients are all-reduced as ONE flat buffer over RCCL.

Two input contracts:
  --input latents (default)  the north_star boundary: VAE latents [B, 8, 256, 16] and L2-normalised CLAP prompt
                             embeddings [B, 512]; `--latents-file` loads a .pt dict {latents, prompt_embeds}.
  --input mel                the reference's collate_fn batch [REF train:415-420]: {log_mel_spec [B,1,1024,64] fp32,
                             input_ids [B,1,512], attention_mask [B,1,512]}; the loop body then runs, as the reference
                             does, `vae.encode(mel).latent_dist.sample() * scaling_factor` [REF train:495-496] and
                             `normalize(text_encoder(ids, mask).text_embeds)` [REF train:510-524] on the HIP kernels
                             (vae.py, clap_text.py).  `--batches-file` loads a .pt dict of those three tensors.
  --audio-dir DIR            recordings: a folder in the Hugging Face audiofolder layout (wav files of any rate and a
                             metadata.jsonl / metadata.csv with file_name and caption).  data.py decodes them once, keeps them on
                             the device and cuts, resamples, normalises and log-mels each batch there into the
                             `--input mel` batch above; `--duration` is the clip length in seconds, `--data-seed` (default
                             `--seed` + 1) seeds the segment stream and the epoch permutations.  The tokeniser comes from
                             `--model-dir`; `--tiny` without one uses data.ByteTokenizer.  A checkpoint carries the segment stream's
                             position and the loader's (epoch, cursor) in `data.bin`; `--resume-from-checkpoint` restores both
                             (rank 0's: with several processes the resumed run is exact only when the clip count divides by
                             their number; a checkpoint without `data.bin` starts the recordings over, with a warning).
Without a file or a folder the driver trains on synthetic tensors of the same shapes.  The reference's dataset class has its mirror
in data.py (HfAudioDataset for rows already in memory, AudioFolder for a folder); its dead code (trim_wav, mixup, frequency / time
masking) is not built.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m audioldm_with_lora_amd.script.train \
        --max-train-steps 100

Beyond the reference's literals (all off by default): `--gradient-accumulation-steps K` (the optimiser runs on every K-th
micro-batch; `--max-train-steps` counts OPTIMISER steps), `--max-grad-norm` (the clip at 1.0 the reference means to apply, SURVEY
quirk Q1), `--snr-gamma` (min-SNR loss weighting) and `--resume-from-checkpoint DIR` (a `checkpoint-<optimiser step>` directory).
`--device-noise` draws every step's timesteps, diffusion noise and posterior noise on the device from the trainer's Philox stream
(seeded by `--seed`; rank r reads the counters from r * 2^48 on) instead of on the host, inside the step's captured graph; with
`--input mel` the whole loop body then runs as LoraTrainer.step_from_batch.  `--noise-offset X` (diffusers' --noise_offset) needs it.
The checkpoint carries that stream's position, so a resumed `--device-noise` run draws exactly what the uninterrupted run would
have; the host-drawn stream of a resumed run is a fresh one, keyed by the step it resumes from.
"""
import argparse
import json
import os
import time

import torch

from .. import dp
from ..clap_text import ClapTextModelWithProjection
from ..lora import LoraConfig, get_peft_model
from ..scheduler import DDIMScheduler
from ..training import LoraTrainer
from ..unet import UNet2DConditionModel
from ..vae import AutoencoderKL


def encode_batch(vae, text_encoder, batch, generator=None, mel_frontend=None):
    """collate_fn batch -> (latents [B,8,H/4,16], prompt_embeds [B,512]) exactly as [REF train:495-524].  A batch that
    carries `waveform` [B,1,T] instead of `log_mel_spec` goes through the GPU log-mel front end first (mel.py)."""
    dev = vae.post_quant_conv.weight.device
    if "log_mel_spec" in batch:
        mel = batch["log_mel_spec"].to(dev, torch.float32)
    else:
        mel = mel_frontend(batch["waveform"].to(dev, torch.float32).flatten(1))
    latents = vae.encode(mel).latent_dist.sample(generator) * vae.config.scaling_factor
    input_ids = batch["input_ids"].squeeze(1)
    attention_mask = batch["attention_mask"].squeeze(1)
    text_embeds = text_encoder(input_ids=input_ids, attention_mask=attention_mask, return_dict=True).text_embeds
    return latents, torch.nn.functional.normalize(text_embeds, dim=-1)


def synthetic_batch(B, g, vocab=50265, max_len=512, pad=1):
    """Shapes and dtypes of the reference's collate_fn output; captions of 8..64 tokens right-padded to 512."""
    ids = torch.full((B, 1, max_len), pad, dtype=torch.long)
    mask = torch.zeros(B, 1, max_len, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(8, 65, (1,), generator=g))
        ids[b, 0, :n] = torch.randint(3, vocab, (n,), generator=g)
        ids[b, 0, 0], ids[b, 0, n - 1] = 0, 2
        mask[b, 0, :n] = 1
    mel = torch.randn(B, 1, 1024, 64, generator=g) * 2.0 - 5.0          # log-mel-like range
    return {"log_mel_spec": mel, "input_ids": ids, "attention_mask": mask}


def build_audio_data(args, device, rank, world, tokenizer):
    """--audio-dir: the resident dataset, the device front end and the loader (data.py); the seeds come from --data-seed"""
    from ..data import AudioFolder, ClipFrontEnd, ClipLoader
    seed = args.seed + 1 if args.data_seed is None else args.data_seed
    front_end = ClipFrontEnd(device, duration=args.duration, seed=seed, rank=rank)
    return ClipLoader(AudioFolder(args.audio_dir, tokenizer, device), front_end, args.train_batch_size, seed=seed, rank=rank, world=world)


def save_data_state(path, loader):
    torch.save({"front_end": loader.front_end.state_dict(), "loader": loader.state_dict()}, os.path.join(path, "data.bin"))


def load_data_state(path, loader):
    """Restores the data position a checkpoint carries; a checkpoint without one (written without --audio-dir, or before the data
    path existed) leaves the loader at (epoch 0, cursor 0) with a warning.  Returns whether a position was restored."""
    f = os.path.join(path, "data.bin")
    if not os.path.isfile(f):
        print(f"[train] warning: {path} holds no data.bin: the recordings start over at epoch 0 with the stream of --data-seed", flush=True)
        return False
    sd = torch.load(f)
    loader.front_end.load_state_dict(sd["front_end"])
    loader.load_state_dict(sd["loader"])
    return True


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=None, help="local diffusers-format directory of cvssp/audioldm-s-full-v2")
    ap.add_argument("--input", choices=("latents", "mel"), default="latents")
    ap.add_argument("--latents-file", default=None)
    ap.add_argument("--batches-file", default=None)
    ap.add_argument("--audio-dir", default=None, metavar="DIR", help="train from recordings: wav files + metadata.jsonl / metadata.csv")
    ap.add_argument("--duration", type=float, default=10.24, help="clip length in seconds (--audio-dir)")
    ap.add_argument("--data-seed", type=int, default=None, help="segment stream and epoch permutations (default: --seed + 1)")
    ap.add_argument("--output-dir", default="data/LoRA_weight/r2_alpha2")
    ap.add_argument("--rank", type=int, default=2)
    ap.add_argument("--lora-alpha", type=int, default=2)
    ap.add_argument("--target-modules", default="to_q,to_v")
    ap.add_argument("--learning-rate", type=float, default=1.0e-5)
    ap.add_argument("--weight-decay", type=float, default=1e-5)
    ap.add_argument("--train-batch-size", type=int, default=2)
    ap.add_argument("--max-train-steps", type=int, default=97000)
    ap.add_argument("--checkpointing-steps", type=int, default=9700 * 2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="shrunken random-init models of the same topology (smoke tests)")
    ap.add_argument("--gradient-accumulation-steps", type=int, default=1, help="micro-batches per optimiser step")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="clip the gradient 2-norm (off by default)")
    ap.add_argument("--snr-gamma", type=float, default=None, help="min-SNR-gamma loss weighting (5.0 is the usual value)")
    ap.add_argument("--device-noise", action="store_true", help="draw noise and timesteps on the device (Philox stream seeded by --seed)")
    ap.add_argument("--noise-offset", type=float, default=0.0, help="diffusers' noise offset; needs --device-noise")
    ap.add_argument("--resume-from-checkpoint", default=None, metavar="DIR", help="a checkpoint-<step> directory written by this driver")
    return ap


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.noise_offset != 0.0 and not args.device_noise:
        parser.error("--noise-offset applies to noise drawn on the device: add --device-noise")
    if args.audio_dir:
        if args.latents_file or args.batches_file:
            parser.error("--audio-dir replaces --latents-file / --batches-file")
        args.input = "mel"                                        # the loader yields the collate_fn batch

    accelerator = dp.Accelerator(gradient_accumulation_steps=1, mixed_precision=None)     # (the trainer itself accumulates)
    device = accelerator.device
    torch.manual_seed(1234)                                       # identical base weights on every rank
    if args.model_dir:
        unet = UNet2DConditionModel.from_pretrained(args.model_dir, subfolder="unet")
        noise_scheduler = DDIMScheduler.from_pretrained(args.model_dir, subfolder="scheduler")
    elif args.tiny:
        from .. import configs
        unet, noise_scheduler = UNet2DConditionModel(**configs.tiny_unet()), DDIMScheduler()
    else:
        unet, noise_scheduler = UNet2DConditionModel(), DDIMScheduler()
    unet.requires_grad_(False)
    cfg = LoraConfig(r=args.rank, lora_alpha=args.lora_alpha, init_lora_weights="gaussian",
                     target_modules=args.target_modules.split(","))
    peft_unet = get_peft_model(unet, cfg)
    unet.to(device)
    trainer = LoraTrainer(unet, noise_scheduler, lr=args.learning_rate, betas=(0.9, 0.999), weight_decay=args.weight_decay,
                          eps=1e-08, max_train_steps=args.max_train_steps, device=device, max_grad_norm=args.max_grad_norm,
                          gradient_accumulation_steps=args.gradient_accumulation_steps, snr_gamma=args.snr_gamma,
                          noise_seed=(args.seed if args.device_noise else None), noise_offset=args.noise_offset)
    K = args.gradient_accumulation_steps
    if args.resume_from_checkpoint:
        accelerator.load_state(args.resume_from_checkpoint, trainer)

    vae = text_encoder = None
    if args.input == "mel":
        if args.model_dir:
            vae = AutoencoderKL.from_pretrained(args.model_dir, subfolder="vae")
            text_encoder = ClapTextModelWithProjection.from_pretrained(args.model_dir, subfolder="text_encoder")
        elif args.tiny:
            vae = AutoencoderKL(**configs.tiny_vae())
            tiny_text = dict(configs.tiny_clap_text(), max_position_embeddings=514, projection_dim=unet.cfg["class_embed_input_dim"])
            if args.audio_dir:                                    # room for every id of the byte-level stand-in tokeniser
                from ..data import ByteTokenizer
                tiny_text["vocab_size"] = max(tiny_text["vocab_size"], ByteTokenizer.vocab_size)
            text_encoder = ClapTextModelWithProjection(**tiny_text)
        else:
            vae, text_encoder = AutoencoderKL(), ClapTextModelWithProjection()
        vae.requires_grad_(False).to(device)
        text_encoder.requires_grad_(False).to(device)
    data = torch.load(args.latents_file) if args.latents_file else (torch.load(args.batches_file) if args.batches_file else None)
    loader = None
    if args.audio_dir:
        if args.model_dir:
            from transformers import RobertaTokenizerFast          # host-side string -> ids only
            tokenizer = RobertaTokenizerFast.from_pretrained(os.path.join(args.model_dir, "tokenizer"))
        elif args.tiny:
            from ..data import ByteTokenizer
            tokenizer = ByteTokenizer()
        else:
            parser.error("--audio-dir needs the tokeniser of --model-dir (or --tiny)")
        loader = build_audio_data(args, device, accelerator.process_index, accelerator.num_processes, tokenizer)
        if args.resume_from_checkpoint:
            load_data_state(args.resume_from_checkpoint, loader)
    # per-rank noise / timesteps drawn on the host; a resumed run draws a fresh stream, keyed by the step it resumes from.  With
    # --device-noise these generators only pick the data: noise and timesteps come from the trainer's Philox stream, whose position
    # load_state has just restored, so the resumed run continues the saved stream.
    g = torch.Generator().manual_seed(args.seed + 1000 * accelerator.process_index + 7919 * trainer.step_count)
    g_dev = torch.Generator(device=device).manual_seed(args.seed + 1000 * accelerator.process_index + 7919 * trainer.step_count + 1)
    B = args.train_batch_size
    t0, train_loss, first_step = time.time(), 0.0, trainer.step_count + 1
    for micro_step in range(trainer.micro_step + 1, args.max_train_steps * K + 1):
        if args.input == "mel":
            if loader is not None:
                batch = loader.next_batch()
            elif data is not None:
                idx = torch.randint(0, data["log_mel_spec"].shape[0], (B,), generator=g)
                batch = {k: data[k][idx] for k in ("log_mel_spec", "input_ids", "attention_mask")}
            else:
                batch = synthetic_batch(B, g, vocab=text_encoder.cfg["vocab_size"])
            if args.device_noise:
                loss = trainer.step_from_batch(vae, text_encoder, batch, None, None, None)
            else:
                latents, prompt_embeds = encode_batch(vae, text_encoder, batch, g_dev)
        elif data is not None:
            idx = torch.randint(0, data["latents"].shape[0], (B,), generator=g)
            latents, prompt_embeds = data["latents"][idx], data["prompt_embeds"][idx]
        else:
            latents = torch.randn(B, 8, 256, 16, generator=g) * 0.9228
            prompt_embeds = torch.nn.functional.normalize(torch.randn(B, unet.cfg["class_embed_input_dim"], generator=g), dim=-1)
        if not args.device_noise:
            noise = torch.randn(latents.shape, generator=g)
            # (sized by the batch at hand [REF train:501-503]: the last batch of an epoch of recordings may be short)
            timesteps = torch.randint(0, noise_scheduler.config.num_train_timesteps, (latents.shape[0],), generator=g).long()
            loss = trainer.step(latents, noise, timesteps, prompt_embeds)
        elif args.input != "mel":
            loss = trainer.step(latents, None, None, prompt_embeds)
        if micro_step % K:
            continue                                              # inside an accumulation window: no optimiser step yet
        global_step = trainer.step_count
        if global_step % 10 == 0 or global_step == args.max_train_steps:
            train_loss = float(trainer.window_loss if K > 1 else loss)
            if accelerator.is_main_process:
                done = global_step - first_step + 1
                rec = {"step": global_step, "train_loss": train_loss, "lr": trainer.lr(global_step),
                       "clips_per_sec": done * K * B * accelerator.num_processes / (time.time() - t0)}
                if trainer.last_grad_norm is not None:
                    rec["grad_norm"] = float(trainer.last_grad_norm)      # device scalar, read at the logging cadence only
                print(json.dumps(rec), flush=True)
        if global_step % args.checkpointing_steps == 0 and accelerator.is_main_process:
            accelerator.save_state(os.path.join(args.output_dir, f"checkpoint-{global_step}"), trainer)
            if loader is not None:
                save_data_state(os.path.join(args.output_dir, f"checkpoint-{global_step}"), loader)
    accelerator.wait_for_everyone()
    if accelerator.is_main_process:
        accelerator.save_state(os.path.join(args.output_dir, f"checkpoint-{args.max_train_steps}"), trainer)
        if loader is not None:
            save_data_state(os.path.join(args.output_dir, f"checkpoint-{args.max_train_steps}"), loader)
    accelerator.end_training()
    return train_loss


if __name__ == "__main__":
    main()
