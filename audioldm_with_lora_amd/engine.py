"""The DDIM denoising loop as a replayed hipGraph.

AudioLDMPipeline.__call__ step 5 ([REF script/inference/generate_audio.py:47-52], [REF app.py:14]):
    for t in timesteps:  eps = unet(cat[x, x], t, class_labels=[neg | pos]);  eps = eps_u + g (eps_t - eps_u)
                         x = ddim_step(eps, t, x)
One step is ~450 kernel launches of a few microseconds each, so the loop is launch-bound when driven from
the host.  Everything that changes between steps lives in DEVICE memory -- the latent x, the CFG-doubled
bf16 UNet input, the timestep scalar and a step counter that indexes the precomputed DDIM coefficient
table -- so ONE captured graph of a single step replays unchanged for all N steps with no host work
in between.  With a DPMSolverMultistepScheduler the update is the multistep solver's (ops.dpm_step_fused): its coefficient rows
come from the scheduler in the same way, and the previous step's model output lives in one more device buffer.
With a UniPCMultistepScheduler the update is the predictor-corrector's (ops.unipc_step_fused): the last corrected
sample and the previous two model outputs live in one device buffer `state` [3, B, H, W, C], whose two output slots the kernel uses as
a ring turned by the parity of the step counter, so the captured graph stays one step for all N.
Audio-to-audio and inpainting: `begin_index` runs the suffix timesteps[begin:] of the schedule, and `masked`
swaps in the masked fused steps, which blend the known latents back in after every update (x0, noise, mask and the blend rows in
four more device buffers, filled by set_inpaint) -- still one launch behind the UNet, so the loop stays one captured graph.
With an EulerAncestralDiscreteScheduler the update is the ancestral Euler step (ops.euler_a_step_fused), which
draws its noise inside the launch from a Philox stream whose state {seed, draw ordinal} is one more device buffer: the last workgroup
moves the ordinal with the step counter, so every replay draws fresh noise.  In sigma space `x` is the unscaled sample and `x_in` holds
x / sqrt(sigma^2 + 1).
With a RePaintScheduler a masked engine runs RePaint's folded walk: n_steps is the number of UNet calls L, and
the step (ops.repaint_step_fused_masked) draws the known part's noise and the jump's noise inside the launch from the same kind of
Philox state, whose ordinal moves by 2 per step.
Multi-adapter LoRA: a gated engine's UNet launches read a per-sample gate table from one more device buffer
(set_adapters): another routing, other weights or no adapter at all is a copy into that buffer -- no repack, no re-capture.
Long-form generation: WindowedDenoiseEngine keeps ONE long latent [B, rows, W, C] and runs the UNet on K
overlapping windows of the trained length as batch rows; the windowed fused step (ops.*_step_fused_windowed) blends the windows' eps
into the long latent, updates it and scatters the next UNet input back into every window -- still one launch behind the UNet.
Long-form audio-to-audio: WindowedAudioToAudioEngine is that engine on a suffix of the schedule, with the
inpainting blend on the long latent inside the same launch (ops.*_step_fused_windowed_masked).
"""
import torch

from . import ops
from .scheduler import DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, RePaintScheduler, UniPCMultistepScheduler, _fresh_seed


class DenoiseEngine:
    def __init__(self, unet, scheduler, batch, height, width, num_inference_steps, guidance_scale=2.5,
                 device="cuda", use_graph=True, chains=None, begin_index=0, masked=False, gated=False):
        self.unet, self.scheduler = unet, scheduler
        self.B, self.H, self.W = batch, height, width
        self.C = unet.cfg["in_channels"]
        self.cfg = guidance_scale > 1.0
        self.g = float(guidance_scale)
        self.use_graph = use_graph
        dev = torch.device(device)
        self.dev = dev
        scheduler.set_timesteps(num_inference_steps)
        self.dpm = isinstance(scheduler, DPMSolverMultistepScheduler)
        self.euler = isinstance(scheduler, EulerAncestralDiscreteScheduler)
        self.unipc = isinstance(scheduler, UniPCMultistepScheduler)
        self.repaint = isinstance(scheduler, RePaintScheduler)
        self.begin_index, self.masked = int(begin_index), bool(masked)
        if self.repaint and not self.masked:
            raise ValueError("RePaintScheduler needs a mask: RePaint resamples a masked region against the kept one (build the engine "
                             "with masked=True, or call the audio-to-audio pipeline with mask=...)")
        if self.repaint and self.begin_index:
            raise NotImplementedError("begin_index > 0 with a RePaintScheduler: RePaint runs its whole walk (strength 1.0)")
        if not 0 <= self.begin_index < len(scheduler.timesteps):
            raise ValueError(f"begin_index {begin_index} outside the schedule of {len(scheduler.timesteps)} steps")
        # (the defaults keep the full schedule and the scheduler's own table call, launch for launch)
        ts = scheduler.timesteps[self.begin_index:] if self.begin_index else scheduler.timesteps
        self.n_steps = len(ts)
        self.timesteps_f32 = ts.to(torch.float32).to(dev)
        coef = scheduler.coefficient_table(begin_index=self.begin_index) if self.begin_index else scheduler.coefficient_table()
        self.coef = coef.contiguous().to(dev)
        # Optional: independent sub-batches ("chains") captured as parallel branches of the graph (each owns a contiguous
        # slice of the latents and its own CFG-doubled input block [uncond_i | cond_i]).  Measured on MI355X / ROCm 7.2 at
        # batch 4: 1 chain 4.83 ms/step, 2 chains 4.81, 4 chains 5.90 -- the branches do not overlap usefully, so the
        # default stays a single chain.
        if chains is None:
            chains = 1
        if chains > 1 and (self.dpm or self.euler or self.unipc or self.repaint):
            raise NotImplementedError("chains > 1 runs the DDIM update only")
        if chains > 1 and self.masked:
            raise NotImplementedError("chains > 1 runs the unmasked update only")
        assert batch % chains == 0
        self.chains, self.bc = chains, batch // chains
        nbc = 2 * self.bc if self.cfg else self.bc
        self.x = torch.zeros(batch, height, width, self.C, dtype=torch.float32, device=dev)       # latents, NHWC fp32
        self.x_in = [torch.zeros(nbc, height, width, self.C, dtype=torch.bfloat16, device=dev) for _ in range(chains)]
        # DPM-Solver: the previous step's converted model output (read by second-order rows, never by row 0)
        self.hist = torch.zeros_like(self.x) if self.dpm else None
        # UniPC: the last corrected sample and the two previous converted model outputs (each read only by rows that ask for it, none
        # by row 0)
        self.state = torch.zeros(3, *self.x.shape, dtype=torch.float32, device=dev) if self.unipc else None
        # Euler-ancestral: the Philox state {seed_lo, seed_hi, draw_lo, draw_hi} of the in-loop noise (set_seed; set_latents puts the
        # draw ordinal back to 0) and the input scale of the first row, which set_latents applies (the later rows' are in the table)
        # RePaint: the same state; every step uses two draws (the known part's noise, the jump's)
        self.rng = ops.philox_state(_fresh_seed(), 0, dev) if self.euler or self.repaint else None
        self.in_scale0 = float(scheduler.input_scale(self.begin_index)) if self.euler else 1.0
        # masked: the known latents (x0 * scaling_factor), the eps the loop started from (both NHWC fp32), the mask [B, h, w] fp32
        # (1 = regenerate) and the blend rows (a, s) of the suffix [n_steps, 2] -- set_inpaint fills the first three
        self.x0 = self.noise = self.mask = self.blend = None
        if self.masked:
            self.x0, self.noise = torch.zeros_like(self.x), torch.zeros_like(self.x)
            self.mask = torch.ones(batch, height, width, dtype=torch.float32, device=dev)
            self.blend = scheduler.blend_table(self.begin_index).contiguous().to(dev)
        # the single-chain step's last launch (ops.{ddim,dpm,unipc,euler_a}_step_fused[_masked]) and what it takes beside the frame's operands
        self._step = getattr(ops, self._solver_name() + "_step_fused" + ("_masked" if self.masked else ""))
        self._solver_args = (self.rng,) if self.euler or self.repaint else (self.hist,) if self.dpm else (self.state,) if self.unipc else ()
        self._inpaint_args = (self.x0, self.noise, self.mask, self.blend) if self.masked else ()
        self.t_buf = torch.zeros(1, dtype=torch.float32, device=dev)
        self.step_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)      # the fused step's last-workgroup ticket (rests at 0)
        # Multi-adapter routing: [chains][nbc][32] fp32 gate tables the UNet's fused-LoRA launches read.  An engine is GATED when the
        # model needs a gate at construction (more than one adapter, or non-default routing); an engine for a plain single-adapter model
        # passes none and its launches are the ungated ones.
        self.gate = None
        if gated or (hasattr(unet, "routing_is_plain") and not unet.routing_is_plain()):
            self._fill_gate(None, None)
        self.cls = None
        self.temb = None             # [chains][n_steps, nbc, temb_total] fp32: time-embedding projections of every step
        self.rowbias = None          # [chains][nbc, temb_total] fp32: the current step's row (gathered on the device)
        self.graph = None
        self._side = None
        # The captured graph holds raw pointers into the UNet's packed operands (unet.plan()): keep that plan alive for as long
        # as the graph exists and remember its version, so a later state load / LoRA update (which bumps unet.plan_version) is
        # noticed instead of replaying the old weights -- or freed memory.
        self._plan_ref = None
        self.plan_version = None

    def _solver_name(self):
        return "euler_a" if self.euler else "dpm" if self.dpm else "unipc" if self.unipc else "repaint" if self.repaint else "ddim"

    def stale(self):
        """True when the UNet's packed operands changed after this engine captured its graph."""
        return self.plan_version is not None and self.plan_version != self.unet.plan_version

    def _check_fresh(self):
        if self.stale():
            if self.graph is None:                     # eager launches re-plan by themselves
                self._plan_ref, self.plan_version = self.unet.plan(), self.unet.plan_version
                return
            raise ops._lib.AldmError("DenoiseEngine: the UNet's weights changed after this graph was captured "
                                     "(load_state_dict / LoRA update); call capture() again or build a new engine")

    def set_condition(self, prompt_embeds, negative_prompt_embeds=None):
        """[B, D] L2-normalised prompt embeddings (CLAP text_embeds); CFG order is [negative | positive]."""
        pe = prompt_embeds.to(self.dev, torch.float32)
        ne = None
        if self.cfg:
            ne = torch.zeros_like(pe) if negative_prompt_embeds is None else negative_prompt_embeds.to(self.dev, torch.float32)
        new = []
        for i in range(self.chains):
            sl = slice(i * self.bc, (i + 1) * self.bc)
            e = torch.cat([ne[sl], pe[sl]]) if self.cfg else pe[sl]
            new.append(ops.f32_to_bf16(e.contiguous()))
        if self.cls is None:
            self.cls = new
        else:
            for dst, src in zip(self.cls, new):
                dst.copy_(src)
        # everything the UNet derives from (timestep, prompt) alone is computed here once for the whole schedule
        tabs = [self.unet.temb_table(self.timesteps_f32, c) for c in self.cls]
        if self.temb is None:
            self.temb = tabs
            self.rowbias = [torch.empty_like(t[0]) for t in tabs]
        else:
            for dst, src in zip(self.temb, tabs):
                dst.copy_(src)
        self._prime()

    @property
    def gated(self):
        return self.gate is not None

    def set_adapters(self, adapter_names=None, adapter_weights=None):
        """Per-clip adapter routing: adapter_names has one entry per clip of the batch (a name, "__base__", a list or a dict name ->
        weight; None = the model's active adapters with their set weights), adapter_weights an optional factor per clip.  The gate rows
        go into the engine's own device buffer, so a captured graph replays with the new routing; under CFG both halves of a clip get
        the same gates."""
        plain = adapter_weights is None and self.unet.routing_is_plain(adapter_names)
        if self.gate is None:
            if plain:
                return
            if getattr(self, "graph", None) is not None:
                raise ops._lib.AldmError("DenoiseEngine: this graph was captured without a gate table (plain single-adapter model); "
                                         "build a new engine to route adapters per clip")
        self._fill_gate(adapter_names, adapter_weights)

    def _fill_gate(self, adapter_names, adapter_weights):
        g = self.unet.device_gate(adapter_names, self.B, adapter_weights)
        if g is None:                                        # plain routing on a gated engine: the table of the active adapter
            g = self.unet.gate_table(adapter_names, self.B).to(self.dev)
        new = []
        for i in range(self.chains):
            sl = g[i * self.bc:(i + 1) * self.bc]
            new.append((torch.cat([sl, sl]) if self.cfg else sl).contiguous())
        if self.gate is None:
            self.gate = new
        else:
            for dst, src in zip(self.gate, new):
                dst.copy_(src)

    def _gate(self, i):
        return None if self.gate is None else self.gate[i]

    def set_seed(self, seed):
        """Euler-ancestral and RePaint engines: the 64-bit seed of the in-loop noise stream, written into the device state (draw ordinal
        0), so a captured graph replays with the new stream.  Same seed + same latents = the same bits, replayed or eager."""
        if self.rng is None:
            raise ValueError("set_seed needs an engine built with an EulerAncestralDiscreteScheduler or a RePaintScheduler (the other "
                             "updates draw no noise)")
        self.rng.copy_(ops.philox_state(seed, 0, self.dev))

    def set_latents(self, latents_nchw):
        """latents [B, C, H, W] fp32, already multiplied by init_noise_sigma (1 for DDIM / DPM-Solver / UniPC).  Euler-ancestral: the unscaled
        sigma-space sample; the UNet input gets row 0's input scale here, and the noise stream's draw ordinal returns to 0."""
        x = ops.nchw_to_nhwc(latents_nchw.to(self.dev, torch.float32).contiguous(), out_f32=True)
        self.x.copy_(x)
        xb = ops.f32_to_bf16(self.x, self.in_scale0) if self.euler else ops.f32_to_bf16(self.x)
        for i in range(self.chains):
            sl = slice(i * self.bc, (i + 1) * self.bc)
            self.x_in[i][: self.bc].copy_(xb[sl])
            if self.cfg:
                self.x_in[i][self.bc:].copy_(xb[sl])
        self.step_idx.zero_()
        self.t_buf.copy_(self.timesteps_f32[:1])
        if self.hist is not None:
            self.hist.zero_()
        if self.state is not None:
            self.state.zero_()
        if self.rng is not None:
            self.rng[2:].zero_()
        self._prime()

    def set_inpaint(self, x0_nchw, noise_nchw, mask):
        """masked engines: x0 [B, C, H, W] fp32 (the encoded clip times scaling_factor), noise [B, C, H, W] fp32 (the eps the loop
        started from), mask [B, H, W] (1 = regenerate, 0 = keep; fractional values blend).  Copied into the engine's own buffers, so a
        captured graph replays with the new values."""
        if not self.masked:
            raise ValueError("set_inpaint needs an engine built with masked=True")
        if tuple(mask.shape) != tuple(self.mask.shape):
            raise ValueError(f"mask shape {tuple(mask.shape)}, expected {tuple(self.mask.shape)}")
        self.x0.copy_(ops.nchw_to_nhwc(x0_nchw.to(self.dev, torch.float32).contiguous(), out_f32=True))
        self.noise.copy_(ops.nchw_to_nhwc(noise_nchw.to(self.dev, torch.float32).contiguous(), out_f32=True))
        self.mask.copy_(mask.to(self.dev, torch.float32))

    def _prime(self):
        """The single-chain step gathers the NEXT step's time-embedding row at its end (ops.ddim_step_fused); the row of the
        step the counter stands at is put in place here, whenever the counter or the table changes outside the graph.  The fused
        step's last-workgroup ticket is put back to rest as well: a launch that was aborted midway would otherwise leave it non-zero
        for every later replay."""
        self.ticket.zero_()
        if self.temb is not None and self.chains == 1:
            ops.gather_row(self.temb[0], self.step_idx, self.rowbias[0])

    def _chain_step(self, i):
        ops.gather_row(self.temb[i], self.step_idx, self.rowbias[i])
        eps = self.unet.forward_nhwc(self.x_in[i], self.t_buf, self.cls[i], rowbias=self.rowbias[i], gate=self._gate(i))
        ops.cfg_ddim_step(eps, self.x[i * self.bc:(i + 1) * self.bc], self.cfg, self.g, self.coef, self.step_idx, self.x_in[i])

    def _one_step(self):
        if self.chains == 1:
            # one chain: guidance + the scheduler's update, the next step's time-embedding row and the step counter in ONE launch behind the UNet
            eps = self.unet.forward_nhwc(self.x_in[0], self.t_buf, self.cls[0], rowbias=self.rowbias[0], gate=self._gate(0))
            self._step(eps, self.x, self.cfg, self.g, self.coef, self.step_idx, self.x_in[0], *self._solver_args, self.temb[0], self.rowbias[0],
                       self.timesteps_f32, self.t_buf, self.ticket, *self._inpaint_args)
            return
        else:                                   # fork / join: under capture these become parallel graph branches
            cur = torch.cuda.current_stream()
            if self._side is None:
                self._side = [torch.cuda.Stream() for _ in range(self.chains - 1)]
            for s in self._side:
                s.wait_stream(cur)
            self._chain_step(0)
            for i, s in enumerate(self._side):
                with torch.cuda.stream(s):
                    self._chain_step(i + 1)
            for s in self._side:
                cur.wait_stream(s)
        ops.advance_step(self.step_idx, self.timesteps_f32, self.t_buf)

    def capture(self):
        """Warm up (loads code objects, sizes the split-K workspace) and capture one step."""
        self.graph = None
        self._plan_ref, self.plan_version = self.unet.plan(), self.unet.plan_version
        saved = (self.x.clone(), [t.clone() for t in self.x_in], self.step_idx.clone(), self.t_buf.clone())
        saved_hist = self.hist.clone() if self.hist is not None else None
        saved_state = self.state.clone() if self.state is not None else None
        saved_rng = self.rng.clone() if self.rng is not None else None
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._one_step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if self.use_graph:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):   # RCCL's watchdog thread must not void the capture
                self._one_step()
        for dst, src in zip([self.x] + self.x_in + [self.step_idx, self.t_buf], [saved[0]] + saved[1] + [saved[2], saved[3]]):
            dst.copy_(src)
        if saved_hist is not None:
            self.hist.copy_(saved_hist)
        if saved_state is not None:
            self.state.copy_(saved_state)
        if saved_rng is not None:
            self.rng.copy_(saved_rng)
        self._prime()
        torch.cuda.synchronize()

    def step(self):
        self._check_fresh()
        if self.graph is not None:
            self.graph.replay()
        else:
            self._one_step()

    def run(self, steps=None):
        for _ in range(self.n_steps if steps is None else steps):
            self.step()
        return self.x

    def latents_nchw(self):
        return ops.nhwc_to_nchw_f32(self.x)


class WindowedDenoiseEngine(DenoiseEngine):
    """The loop on a LONG latent as K overlapping windows (longform.WindowPlan over the time axis): B clips times K windows are the
    UNet's batch rows, shapes it is tuned for.  x, hist, state and the Philox stream stay in the long layout [B, rows, W, C]; x_in,
    the class labels, the time-embedding table and the gate table have one row per (clip, window): 2 * B * K under CFG, all in ONE
    UNet call (no sub-batching: activation memory grows with K).  A plan of one window is DenoiseEngine, bit
    for bit.  This class starts from noise: chains > 1, masked and begin_index > 0 raise (WindowedAudioToAudioEngine below takes the
    last two)."""
    _AUDIO_TO_AUDIO = False

    def __init__(self, unet, scheduler, batch, plan, width, num_inference_steps, guidance_scale=2.5, device="cuda", use_graph=True,
                 chains=None, begin_index=0, masked=False, gated=False):
        if chains not in (None, 1):
            raise NotImplementedError(f"{type(self).__name__}: chains > 1 is not built (the windows already fill the batch)")
        if (masked or begin_index) and not self._AUDIO_TO_AUDIO:
            raise NotImplementedError("WindowedDenoiseEngine: masked / begun (audio-to-audio) runs on a long latent take a "
                                      "WindowedAudioToAudioEngine")
        self.plan, self.K, self.hw = plan, plan.K, plan.window_rows
        super().__init__(unet, scheduler, batch, plan.rows, width, num_inference_steps, guidance_scale, device=device, use_graph=use_graph,
                         begin_index=begin_index, masked=masked, gated=gated)
        self.bc = batch * self.K                                  # rows per CFG half of everything the UNet sees
        self.x_in = [torch.zeros((2 if self.cfg else 1) * self.bc, self.hw, width, self.C, dtype=torch.bfloat16, device=self.dev)]
        self._win = plan.device(self.dev)                         # offset / cover / weight tables (the plan keeps them alive)
        self._step = getattr(ops, self._solver_name() + "_step_fused_windowed" + ("_masked" if self.masked else ""))

    def _per_window(self, entries, what):
        """one entry per clip, or one per (clip, window) in that order -> one per (clip, window)"""
        if entries is None:
            return None
        entries = list(entries)
        if len(entries) == self.B * self.K:
            return entries
        if len(entries) == self.B:
            return [e for e in entries for _ in range(self.K)]
        raise ValueError(f"{what} needs one entry per clip ({self.B}) or per (clip, window) ({self.B * self.K}), got {len(entries)}")

    def _windows_of(self, e):
        """[B, D] (repeated over the windows) or [B, K, D] (one prompt per window) -> [B * K, D]"""
        if e is None:
            return None
        if e.dim() == 2 and e.shape[0] == self.B:
            e = e[:, None, :].expand(self.B, self.K, e.shape[-1])
        if e.dim() != 3 or tuple(e.shape[:2]) != (self.B, self.K):
            raise ValueError(f"prompt embeddings must be [{self.B}, D] or [{self.B}, {self.K}, D], got {tuple(e.shape)}")
        return e.reshape(self.B * self.K, e.shape[-1])

    def set_condition(self, prompt_embeds, negative_prompt_embeds=None):
        """[B, D] L2-normalised prompt embeddings, the same for every window of a clip, or [B, K, D]: one prompt per window (a prompt
        schedule along the track).  The negative embeddings likewise."""
        super().set_condition(self._windows_of(prompt_embeds), self._windows_of(negative_prompt_embeds))

    def _fill_gate(self, adapter_names, adapter_weights):
        names, weights = self._per_window(adapter_names, "adapter_names"), self._per_window(adapter_weights, "adapter_weights")
        g = self.unet.device_gate(names, self.B * self.K, weights)
        if g is None:
            g = self.unet.gate_table(names, self.B * self.K).to(self.dev)
        new = [(torch.cat([g, g]) if self.cfg else g).contiguous()]
        if self.gate is None:
            self.gate = new
        else:
            self.gate[0].copy_(new[0])

    def set_adapters(self, adapter_names=None, adapter_weights=None):
        """DenoiseEngine.set_adapters with one entry per clip, or one per (clip, window)."""
        names = self._per_window(adapter_names, "adapter_names")
        plain = adapter_weights is None and self.unet.routing_is_plain(names)
        if self.gate is None:
            if plain:
                return
            if self.graph is not None:
                raise ops._lib.AldmError("WindowedDenoiseEngine: this graph was captured without a gate table (plain single-adapter "
                                         "model); build a new engine to route adapters per clip")
        self._fill_gate(adapter_names, adapter_weights)

    def set_latents(self, latents_nchw):
        """latents [B, C, rows, W] fp32 of the LONG clip, already multiplied by init_noise_sigma; the windows of the first UNet input
        are gathered out of it (Euler-ancestral: with row 0's input scale)."""
        self.x.copy_(ops.nchw_to_nhwc(latents_nchw.to(self.dev, torch.float32).contiguous(), out_f32=True))
        xb = ops.window_gather(self.x, self._win, self.in_scale0)
        self.x_in[0][: self.bc].copy_(xb)
        if self.cfg:
            self.x_in[0][self.bc:].copy_(xb)
        self.step_idx.zero_()
        self.t_buf.copy_(self.timesteps_f32[:1])
        if self.hist is not None:
            self.hist.zero_()
        if self.state is not None:
            self.state.zero_()
        if self.rng is not None:
            self.rng[2:].zero_()
        self._prime()

    def _one_step(self):
        # one UNet call on all windows, then the windowed fused step: blend, update, scatter, next row, counter -- one launch
        eps = self.unet.forward_nhwc(self.x_in[0], self.t_buf, self.cls[0], rowbias=self.rowbias[0], gate=self._gate(0))
        self._step(eps, self.x, self.cfg, self.g, self.coef, self.step_idx, self.x_in[0], *self._solver_args, self.temb[0], self.rowbias[0],
                   self.timesteps_f32, self.t_buf, self.ticket, self._win, *self._inpaint_args)


class WindowedAudioToAudioEngine(WindowedDenoiseEngine):
    """WindowedDenoiseEngine that starts from a recording: `begin_index` runs the suffix timesteps[begin:] --
    its coefficient table, timesteps and Euler-ancestral's first input scale exactly as DenoiseEngine derives them -- and `masked`
    swaps in ops.*_step_fused_windowed_masked, whose x0, noise and mask [B, rows, W] are LONG like x (set_inpaint takes the long
    tensors).  A step stays one UNet call on all windows plus one launch, the loop one captured graph; a plan of one window is
    DenoiseEngine(begin_index, masked), bit for bit.  chains > 1 stays refused."""
    _AUDIO_TO_AUDIO = True

    def set_inpaint(self, x0_nchw_long, noise_nchw_long, mask_long):
        """x0 and noise [B, C, rows, W] fp32 and mask [B, rows, W] of the LONG clip (DenoiseEngine.set_inpaint otherwise)."""
        want = (self.B, self.C, self.H, self.W)
        for name, t in (("x0", x0_nchw_long), ("noise", noise_nchw_long)):
            if tuple(t.shape) != want:
                raise ValueError(f"{name} shape {tuple(t.shape)}, expected the long clip's {want}")
        super().set_inpaint(x0_nchw_long, noise_nchw_long, mask_long)
