"""Long-form and loopable generation: the window plan of MultiDiffusion-style windowed denoising.

One long latent [B, rows, W, C] is denoised as K overlapping windows of `window_rows` rows along time -- the length the UNet was
trained on -- whose eps predictions are blended at every step with fixed per-row weights.  This module is the host half: where the
windows lie, which windows cover a long row, and with what weight.  The device half reads the three tables built here
(ops.window_gather, ops.window_blend, ops.*_step_fused_windowed).

The rule, with stride S = window_rows - overlap_rows and 0 <= overlap_rows <= window_rows // 2:
  offsets     open:   0, S, 2S, ... while o + window_rows < rows, then a last window at rows - window_rows (it may overlap its
                      neighbour by more than overlap_rows); rows <= window_rows is ONE window of `rows` rows
              looped: rows % S == 0; offsets 0, S, ..., rows - S, rows taken modulo `rows`, so the last windows wrap over the seam
  profile     over window k's own rows i, with L_k / R_k the overlap in rows with window k - 1 / k + 1 (0 at an open end; looped:
              both overlap_rows for every window), the rising ramp l = min(1, (i + 1) / (L_k + 1)) and the falling ramp
              r = min(1, (hw - i) / (R_k + 1)):   p_k(i) = l + r - 1.
              Where the two ramps of a window do not meet (L_k + R_k <= hw) one of them is 1 and this IS min(1, (i + 1) / (L_k + 1),
              (hw - i) / (R_k + 1)).  They meet only where a shifted last window lands within overlap_rows of the window before it,
              so that three windows lie over a row; there min() would let the profiles sum to more than 1 and the normalisation
              would move the weights by more per row than any ramp does.  l + r - 1 is the difference of two neighbouring
              crossfades (window k's falling ramp is 1 - window k + 1's rising ramp), so the profiles sum to 1 on every row of
              every plan and no weight moves by more than 1 / (overlap_rows + 1) from one row to the next.
  weight      of window k at long row r: p_k / sum of p over the windows that cover r -- float64, stored fp32
"""
import math
from types import SimpleNamespace

import numpy as np

MAX_COVER = 4          # what the launchers accept (csrc/elementwise.hip WIN_MAX_COVER); the rule above never exceeds 3


class WindowPlan:
    def __init__(self, rows, window_rows, overlap_rows, loop=False):
        rows, window_rows, overlap_rows, loop = int(rows), int(window_rows), int(overlap_rows), bool(loop)
        if rows < 1 or window_rows < 1:
            raise ValueError(f"WindowPlan: rows {rows} and window_rows {window_rows} must be positive")
        if not 0 <= overlap_rows <= window_rows // 2:
            raise ValueError(f"WindowPlan: overlap_rows {overlap_rows} outside 0 .. window_rows // 2 = {window_rows // 2}")
        stride = window_rows - overlap_rows
        if loop:
            if rows < window_rows:
                raise ValueError(f"WindowPlan: a looped plan needs rows {rows} >= window_rows {window_rows}")
            if rows % stride != 0:
                raise ValueError(f"WindowPlan: a looped plan needs rows {rows} to be a multiple of the stride {stride}")
            offsets = list(range(0, rows, stride))
        elif rows <= window_rows:
            window_rows, overlap_rows, offsets = rows, 0, [0]          # one window of the clip's own length: nothing overlaps
        else:
            offsets, o = [], 0
            while o + window_rows < rows:
                offsets.append(o)
                o += stride
            offsets.append(rows - window_rows)
        self.rows, self.window_rows, self.overlap_rows, self.loop, self.stride = rows, window_rows, overlap_rows, loop, stride
        self.offsets = offsets
        self.K = K = len(offsets)
        hw = window_rows
        # the profiles
        prof = np.ones((K, hw), dtype=np.float64)
        i = np.arange(hw, dtype=np.float64)
        for k in range(K):
            if loop:
                L = R = overlap_rows if K > 1 else 0
            else:
                L = max(0, offsets[k - 1] + hw - offsets[k]) if k > 0 else 0
                R = max(0, offsets[k] + hw - offsets[k + 1]) if k < K - 1 else 0
            left, right = np.minimum(1.0, (i + 1.0) / (L + 1.0)), np.minimum(1.0, (hw - i) / (R + 1.0))
            # (one ramp at 1: the other one, bit for bit -- the min() form; both below 1: the ramps meet, three windows over the row)
            prof[k] = np.where(np.maximum(left, right) == 1.0, np.minimum(left, right), left - (1.0 - right))
        # who covers a long row, in ascending window order
        cover = [[] for _ in range(rows)]
        for k, o in enumerate(offsets):
            for j in range(hw):
                cover[(o + j) % rows].append((k, j))
        for c in cover:
            c.sort()
        self.KC = KC = max(len(c) for c in cover)
        self.cover = np.full((rows, KC), -1, dtype=np.int32)
        self.weight64 = np.zeros((rows, KC), dtype=np.float64)
        for r, c in enumerate(cover):
            p = np.array([prof[k, j] for k, j in c], dtype=np.float64)
            p = p / p.sum()
            for n, (k, _) in enumerate(c):
                self.cover[r, n] = k
                self.weight64[r, n] = p[n]
        self.weight = self.weight64.astype(np.float32)
        self.offset = np.asarray(offsets, dtype=np.int32)
        self._device = {}

    @property
    def key(self):
        """what tells two plans apart (the pipeline's engine cache key carries it)"""
        return (self.rows, self.window_rows, self.overlap_rows, self.loop)

    def __repr__(self):
        return f"WindowPlan(rows={self.rows}, window_rows={self.window_rows}, overlap_rows={self.overlap_rows}, loop={self.loop}: K={self.K}, KC={self.KC})"

    def scaled(self, f):
        """the same plan at f times the resolution (f = 4: the mel frames under the latent rows)"""
        return WindowPlan(self.rows * f, self.window_rows * f, self.overlap_rows * f, self.loop)

    def device(self, device="cuda"):
        """The three tables on the device: offset int32 [K], cover int32 [rows, KC], weight fp32 [rows, KC] (built once per device and
        kept, so a captured graph's pointers stay valid for the plan's lifetime)."""
        import torch
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        t = self._device.get(dev)
        if t is None:
            t = self._device[dev] = SimpleNamespace(
                offset=torch.from_numpy(self.offset).to(dev), cover=torch.from_numpy(self.cover).contiguous().to(dev),
                weight=torch.from_numpy(self.weight).contiguous().to(dev), K=self.K, KC=self.KC, rows=self.rows, hw=self.window_rows)
        return t


def seconds_to_rows(seconds, seconds_per_frame, vae_scale_factor):
    """Latent rows of a clip of `seconds`: AudioLDMPipeline.geometry's rule (whole mel frames, rounded up to a whole latent row)."""
    frames = int(seconds / seconds_per_frame)
    return max(1, int(math.ceil(frames / vae_scale_factor)))


def plan_for_seconds(audio_s, window_s, overlap_s, seconds_per_frame, vae_scale_factor, loop=False):
    """The plan of a pipeline call.  The clip and the window follow seconds_to_rows, the overlap is rounded to the nearest row.  A
    looped plan rounds the clip UP to a whole number of strides (the caller returns that longer clip)."""
    rows = seconds_to_rows(audio_s, seconds_per_frame, vae_scale_factor)
    hw = seconds_to_rows(window_s, seconds_per_frame, vae_scale_factor)
    ov = int(round(overlap_s / seconds_per_frame / vae_scale_factor))
    if loop:
        stride = hw - ov
        if stride < 1:
            raise ValueError(f"window overlap {overlap_s} s leaves no stride in a window of {window_s} s")
        rows = int(math.ceil(max(rows, hw) / stride)) * stride
    return WindowPlan(rows, hw, ov, loop)
