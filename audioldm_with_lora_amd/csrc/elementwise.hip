// Small fused elementwise kernels of the denoise loop and the training step (gfx950, HBM/latency-bound):
// timestep embedding, SiLU, layout/precision boundary conversions, the fused CFG + DDIM (or DPM-Solver multistep) update with a
// device-side step counter (so one captured hipGraph replays all 200 steps), flat AdamW, and the flat gradient-norm clip /
// gradient accumulation around it.
// [REF script/inference/generate_audio.py:47-52] (AudioLDMPipeline.__call__ loop body)
// [REF script/train/train_audioldm_lora.py:396-403,559-565] (clip_grad_norm_ and torch.optim.AdamW on the LoRA parameters)
#include <initializer_list>

#include "common.h"
#include "philox.h"

namespace {

__global__ void timestep_embedding_kernel(const float* __restrict__ t, int t_stride, int B, int dim, bf16* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * dim) return;
  const int b = idx / dim, i = idx - b * dim;
  const int half = dim >> 1;
  const int kf = i < half ? i : i - half;
  const float freq = expf(-9.210340371976184f * (float)kf / (float)half);  // ln(10000)
  const float arg = t[b * t_stride] * freq;
  out[idx] = (bf16)(i < half ? cosf(arg) : sinf(arg));   // flip_sin_to_cos: [cos | sin]
}

__global__ void silu_kernel(const bf16* __restrict__ x, long long n, bf16* __restrict__ y) {
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i + 8 <= n) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(x + i);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (bf16)silu_f((float)v[k]);
    *reinterpret_cast<bf16x8*>(y + i) = v;
  } else {
    for (long long j = i; j < n; ++j) y[j] = (bf16)silu_f((float)x[j]);
  }
}

__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, int B, int C, int HW, void* __restrict__ y, int y_f32) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // over NHWC output
  if (idx >= (long long)B * C * HW) return;
  const int c = (int)(idx % C);
  const long long t = idx / C;
  const int p = (int)(t % HW), b = (int)(t / HW);
  const float v = x[((long long)b * C + c) * HW + p];
  if (y_f32) reinterpret_cast<float*>(y)[idx] = v; else reinterpret_cast<bf16*>(y)[idx] = (bf16)v;
}

__global__ void nhwc_to_nchw_kernel(const void* __restrict__ x, int x_f32, int B, int C, int HW, float* __restrict__ y) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // over NCHW output
  if (idx >= (long long)B * C * HW) return;
  const int p = (int)(idx % HW);
  const long long t = idx / HW;
  const int c = (int)(t % C), b = (int)(t / C);
  const long long src = ((long long)b * HW + p) * C + c;
  y[idx] = x_f32 ? reinterpret_cast<const float*>(x)[src] : (float)reinterpret_cast<const bf16*>(x)[src];
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ x, long long n, float mul, bf16* __restrict__ y) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = (bf16)(x[i] * mul);
}

// guidance + DDIM update of one element, every fused multiply-add spelled out: the scalar and the vectorised kernels below then
// round identically whatever the compiler would have contracted (tests compare them bit for bit)
__device__ __forceinline__ float ddim_update(float eu, float et, float xv, int cfg, float g, float sa, float sb, float sap, float sbp) {
  const float e = cfg ? fmaf(g, et - eu, eu) : eu;
  const float x0 = fmaf(-sb, e, xv) / sa;
  return fmaf(sap, x0, sbp * e);
}

__global__ void cfg_ddim_step_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n, int cfg,
                                     float g, const float* __restrict__ coef, const int* __restrict__ step_idx,
                                     bf16* __restrict__ x_in) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)B * n;
  if (idx >= total) return;
  const float* cf = coef + 4 * step_idx[0];
  const float sa = cf[0], sb = cf[1], sap = cf[2], sbp = cf[3];
  const float eu = eps[idx], et = cfg ? eps[total + idx] : eu;
  const float xn = ddim_update(eu, et, x[idx], cfg, g, sa, sb, sap, sbp);
  x[idx] = xn;
  if (x_in) {
    x_in[idx] = (bf16)xn;
    if (cfg) x_in[total + idx] = (bf16)xn;
  }
}

// Inpainting / audio-to-audio blend of the masked step kernels (diffusers' legacy inpaint loop): after the scheduler update xn, the
// known latents are noised to the level of the NEXT timestep with the row (a, s) = blend[step_idx[0]] and put back where the mask
// keeps them:   known = a x0 + s noise ;  x' = (1 - m) known + m xn      (m = mask[pixel], broadcast over channels; 1 = regenerate)
// Exact at the ends: m == 1 gives xn, m == 0 gives known, and the last row (1, 0) gives known == x0 (each term is an exact product
// or an exact zero added once).
struct Inpaint {
  const float* x0;       // [B][h][w][C] fp32: the encoded clip times scaling_factor
  const float* noise;    // [B][h][w][C] fp32: the eps the loop started from
  const float* mask;     // [B][h][w] fp32
  const float* blend;    // [n_steps][2] fp32 rows (a, s)
  int C;
};

__device__ __forceinline__ float inpaint_blend(float xn, float x0, float nz, float m, float a, float s) {
  const float known = fmaf(s, nz, a * x0);
  return fmaf(m, xn, (1.f - m) * known);
}

// guidance + DPM-Solver(++) multistep update of one element from a coefficient row {alpha_s, sig_s, A, B, C, convert, reads_hist, -}
// (scheduler.py DPMSolverMultistepScheduler.coefficient_table), every fused multiply-add spelled out as in ddim_update:
//   m0 = convert ? (x - sig_s e) / alpha_s : e ;  x' = A x + B m0 + C (m0 - m1)      (m1 = hist; C == 0 and m1 unread on first-order rows)
__device__ __forceinline__ float dpm_model_output(float eu, float et, float xv, int cfg, float g, float alpha_s, float sig_s, bool convert) {
  const float e = cfg ? fmaf(g, et - eu, eu) : eu;
  return convert ? fmaf(-sig_s, e, xv) / alpha_s : e;
}

__device__ __forceinline__ float dpm_update(float m0, float m1, float xv, float A, float Bc, float Cc) {
  return fmaf(A, xv, fmaf(Bc, m0, Cc * (m0 - m1)));
}

// guidance + Euler-ancestral update of one element from a coefficient row {dt, sigma_up, in_scale_next, sigma_down}
// (scheduler.py EulerAncestralDiscreteScheduler.coefficient_table; dt = sigma_down - sigma_from), every fused multiply-add spelled
// out as in ddim_update:   x' = x + e dt + sigma_up z      (z ~ N(0, 1) from the Philox stream; sigma_up == 0 on the last row)
__device__ __forceinline__ float euler_a_update(float eu, float et, float xv, int cfg, float g, float dt, float sigma_up, float z) {
  const float e = cfg ? fmaf(g, et - eu, eu) : eu;
  return fmaf(sigma_up, z, fmaf(e, dt, xv));
}

// UniPC (predictor-corrector) update of one element from a coefficient row {alpha_s, sig_s, Ac, Bc, Cc, Dc, Ap, Bp, Cp, convert, corr,
// corr_reads_m1, pred_reads_m0, -, -, -} (scheduler.py UniPCMultistepScheduler.coefficient_table), every fused multiply-add spelled
// out as in ddim_update; m_t is dpm_model_output of the UNCORRECTED sample:
//   xc = corr ? Ac last + Bc m0 + Cc (m1 - m0) + Dc (m_t - m0) : x ;  x' = Ap xc + Bp m_t + Cp (m_t - m0)
// (m0, m1: the previous two converted outputs; Cc == 0 / Cp == 0 and m1 / m0 unread where the corrector / the predictor is first order)
__device__ __forceinline__ float unipc_correct(float last, float m0, float m1, float mt, float Ac, float Bc, float Cc, float Dc) {
  return fmaf(Ac, last, fmaf(Bc, m0, fmaf(Cc, m1 - m0, Dc * (mt - m0))));
}

__device__ __forceinline__ float unipc_predict(float xc, float m0, float mt, float Ap, float Bp, float Cp) {
  return fmaf(Ap, xc, fmaf(Bp, mt, Cp * (mt - m0)));
}

// ---- the fused scheduler step: one frame (step_fused_body), five solvers ---------------------------------------------------------
// What the frame asks of a scheduler.  ROW: the floats per row of its coefficient table.  TICKET_OPTIONAL: whether its entry points
// take ticket == NULL (the eager scheduler.step: the counter is left alone, and table is NULL there too).  DRAWS_BLEND_NOISE: whether
// the inpainting blend's noise comes from the solver, not from Inpaint::noise (which may then be NULL).  Its one extra kernel
// operand, if any, as the first member (the kernels build the solver from it, UniPC's also from the counter and the element count that
// they hold anyway; every other member starts at zero).  And eight hooks,
// which every thread calls in this order:
//   begin()             before the bounds test: the state that the last workgroup moves, read where the counter is read
//   load<VEC>(cf, idx)  the coefficient row `cf` and whatever else the update of elements [idx, idx + VEC) reads
//   blend_noise<VEC>(noise, idx)  (masked only) the noise of the blend for elements [idx, idx + VEC): Inpaint::noise as it lies in
//                       memory (the identity, requested ahead of load), or, with DRAWS_BLEND_NOISE, what load drew
//   update<VEC>(k, ..)  element k's new latent, through the solver's one-element function above
//   after_blend(k, r)   what becomes of the (blended) latent before it is stored: the identity, but for RePaint's jump
//   unet_input(r)       the value whose bf16 rounding is the next UNet input
//   store<VEC>(idx)     what is stored beside x
//   advance()           what the last workgroup stores beside the counter
template <int VEC>
using fvec_t = float __attribute__((ext_vector_type(VEC)));

struct DdimSolver {
  static constexpr int ROW = 4;
  static constexpr bool TICKET_OPTIONAL = false;
  static constexpr bool DRAWS_BLEND_NOISE = false;
  float sa, sb, sap, sbp;
  __device__ __forceinline__ void begin() {}
  template <int VEC>
  __device__ __forceinline__ void load(const float* __restrict__ cf, long long) {
    sa = cf[0], sb = cf[1], sap = cf[2], sbp = cf[3];
  }
  template <int VEC>
  __device__ __forceinline__ float update(int, float eu, float et, float xv, int cfg, float g) {
    return ddim_update(eu, et, xv, cfg, g, sa, sb, sap, sbp);
  }
  template <int VEC>
  __device__ __forceinline__ fvec_t<VEC> blend_noise(const float* __restrict__ noise, long long idx) const {
    return *reinterpret_cast<const fvec_t<VEC>*>(noise + idx);
  }
  __device__ __forceinline__ float after_blend(int, float r) const { return r; }
  __device__ __forceinline__ float unet_input(float r) const { return r; }
  template <int VEC> __device__ __forceinline__ void store(long long) {}
  __device__ __forceinline__ void advance() {}
};

// history `hist` [B][n] fp32: the previous step's converted model output, read only on rows that ask for it (a first-order row, row 0
// among them, never loads it), then overwritten with this step's -- the unblended m0, as diffusers stores the model output before the
// caller blends
struct DpmSolver {
  static constexpr int ROW = 8;
  static constexpr bool TICKET_OPTIONAL = true;
  static constexpr bool DRAWS_BLEND_NOISE = false;
  float* __restrict__ hist;
  float alpha_s, sig_s, A, Bc, Cc;
  bool convert, second;
  f32x4 m0, m1;                                               // lanes [0, VEC)
  __device__ __forceinline__ void begin() {}
  template <int VEC>
  __device__ __forceinline__ void load(const float* __restrict__ cf, long long idx) {
    alpha_s = cf[0], sig_s = cf[1], A = cf[2], Bc = cf[3], Cc = cf[4];
    convert = cf[5] != 0.f, second = cf[6] != 0.f;
    if (second) {
      const fvec_t<VEC> h = *reinterpret_cast<const fvec_t<VEC>*>(hist + idx);
#pragma unroll
      for (int k = 0; k < VEC; ++k) m1[k] = h[k];
    }
  }
  template <int VEC>
  __device__ __forceinline__ float update(int k, float eu, float et, float xv, int cfg, float g) {
    m0[k] = dpm_model_output(eu, et, xv, cfg, g, alpha_s, sig_s, convert);
    return dpm_update(m0[k], second ? m1[k] : m0[k], xv, A, Bc, Cc);
  }
  template <int VEC>
  __device__ __forceinline__ fvec_t<VEC> blend_noise(const float* __restrict__ noise, long long idx) const {
    return *reinterpret_cast<const fvec_t<VEC>*>(noise + idx);
  }
  __device__ __forceinline__ float after_blend(int, float r) const { return r; }
  __device__ __forceinline__ float unet_input(float r) const { return r; }
  template <int VEC>
  __device__ __forceinline__ void store(long long idx) {
    fvec_t<VEC> v;
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = m0[k];
    *reinterpret_cast<fvec_t<VEC>*>(hist + idx) = v;
  }
  __device__ __forceinline__ void advance() {}
};

// the noise is generated HERE: element i of the [B][n] latents is element i of the current draw of the Philox state `rng` (philox.h:
// no noise tensor in memory, and the same bits as aldm_randn for the same state).  VEC = 4 maps one thread to one Philox block; VEC = 1
// evaluates the element's whole block and keeps its lane.  The latents stay in sigma space (unscaled); the UNet input is
// x' * in_scale_next.  The counter advance moves the DRAW ORDINAL of the state as well, by the same last-workgroup ticket: every
// workgroup reads state[2..3] when it starts, the last one stores ordinal + 1.
struct EulerASolver {
  static constexpr int ROW = 4;
  static constexpr bool TICKET_OPTIONAL = true;
  static constexpr bool DRAWS_BLEND_NOISE = false;
  uint32_t* __restrict__ rng;
  PhiloxState rs;
  float dt, sigma_up, in_scale;
  f32x4 z;                                                    // lanes [0, VEC): the normals of elements idx + k
  __device__ __forceinline__ void begin() { rs = philox_load(rng); }
  template <int VEC>
  __device__ __forceinline__ void load(const float* __restrict__ cf, long long idx) {
    dt = cf[0], sigma_up = cf[1], in_scale = cf[2];
    z = philox_normal4(rs, (unsigned long long)(idx >> 2));
    if constexpr (VEC == 1) {
      const int lane = (int)(idx & 3);
      z[0] = lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3];
    }
  }
  template <int VEC>
  __device__ __forceinline__ float update(int k, float eu, float et, float xv, int cfg, float g) {
    return euler_a_update(eu, et, xv, cfg, g, dt, sigma_up, z[k]);
  }
  template <int VEC>
  __device__ __forceinline__ fvec_t<VEC> blend_noise(const float* __restrict__ noise, long long idx) const {
    return *reinterpret_cast<const fvec_t<VEC>*>(noise + idx);
  }
  __device__ __forceinline__ float after_blend(int, float r) const { return r; }
  __device__ __forceinline__ float unet_input(float r) const { return r * in_scale; }
  template <int VEC> __device__ __forceinline__ void store(long long) {}
  __device__ __forceinline__ void advance() { philox_store_next(rng, rs); }
};

// RePaint (Lugmayr et al., CVPR 2022, Algorithm 1) on a coefficient row {sa, sb, sap, sbp, c1, c2, -, -} (scheduler.py
// RePaintScheduler.coefficient_table): the DDIM update (eta = 0), the inpainting blend with FRESH noise zk for the known part (line 4
// of the algorithm; the legacy loop reuses the eps it started from), then the closed-form jump back up over the row's J levels,
//   x' = c1 xb + c2 zj        ((c1, c2) == (1, 0) on rows without a jump: zj is then not generated and x' = xb)
// Both noises are generated HERE (draw contract: philox.h): zk is element i of draw d, zj element i of draw d + 1, where d is the
// ordinal the launch finds and i the element's index in the [B][n] latents (the long latents when windowed); the last workgroup
// leaves the ordinal at d + 2 on every row.  Only masked entry points exist: without a mask there is nothing to resample towards.
__device__ __forceinline__ float repaint_jump(float xb, float c1, float c2, float zj) { return fmaf(c2, zj, c1 * xb); }

__device__ __forceinline__ f32x4 philox_normal_lanes(const PhiloxState& s, long long idx, int vec) {
  f32x4 z = philox_normal4(s, (unsigned long long)(idx >> 2));
  if (vec == 1) {
    const int lane = (int)(idx & 3);
    z[0] = lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3];
  }
  return z;
}

struct RepaintSolver {
  static constexpr int ROW = 8;
  static constexpr bool TICKET_OPTIONAL = true;
  static constexpr bool DRAWS_BLEND_NOISE = true;
  uint32_t* __restrict__ rng;
  PhiloxState rs;
  float sa, sb, sap, sbp, c1, c2;
  f32x4 zk, zj;                                               // lanes [0, VEC): the normals of elements idx + k
  __device__ __forceinline__ void begin() { rs = philox_load(rng); }
  template <int VEC>
  __device__ __forceinline__ void load(const float* __restrict__ cf, long long idx) {
    sa = cf[0], sb = cf[1], sap = cf[2], sbp = cf[3], c1 = cf[4], c2 = cf[5];
    zk = philox_normal_lanes(rs, idx, VEC);
    if (c2 != 0.f) zj = philox_normal_lanes(philox_at(rs, 1), idx, VEC);   // (uniform over the grid)
  }
  template <int VEC>
  __device__ __forceinline__ fvec_t<VEC> blend_noise(const float* __restrict__, long long) const {
    fvec_t<VEC> v;
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = zk[k];
    return v;
  }
  template <int VEC>
  __device__ __forceinline__ float update(int, float eu, float et, float xv, int cfg, float g) {
    return ddim_update(eu, et, xv, cfg, g, sa, sb, sap, sbp);
  }
  __device__ __forceinline__ float after_blend(int k, float r) const { return c2 != 0.f ? repaint_jump(r, c1, c2, zj[k]) : c1 * r; }
  __device__ __forceinline__ float unet_input(float r) const { return r; }
  template <int VEC> __device__ __forceinline__ void store(long long) {}
  __device__ __forceinline__ void advance() { philox_store_ordinal(rng, philox_at(rs, 2)); }
};

// state [3][B][n] fp32: plane 0 the last corrected sample, planes 1 and 2 the previous two converted model outputs as a RING indexed by
// the parity of the step counter, so that nothing is shifted: step `cur` reads m0 (step cur - 1's output) from slot (cur - 1) & 1 and m1
// (step cur - 2's) from slot cur & 1, then writes m_t over m1's slot.  Every thread reads and writes its own elements only, so the
// ring needs no synchronisation beyond the frame's.  A plane is loaded only where the row's flags ask for it: row 0 (no corrector,
// first-order predictor) reads none, so a replay that wrapped to step 0, at either parity, starts clean.  last and the slots receive
// unblended values (diffusers: the caller blends after scheduler.step); last is the corrected sample, or x itself without corrector.
struct UniPCSolver {
  static constexpr int ROW = 16;
  static constexpr bool TICKET_OPTIONAL = true;
  static constexpr bool DRAWS_BLEND_NOISE = false;
  float* __restrict__ state;
  const int* __restrict__ step_idx;
  long long total;                                            // B * n: the stride between the planes of state
  int slot;                                                   // cur & 1: m1's slot, and where m_t goes
  float alpha_s, sig_s, Ac, Bc, Cc, Dc, Ap, Bp, Cp;
  bool convert, corr, c2, p2;
  f32x4 last, m0, m1, mt, xc;                                 // lanes [0, VEC)
  __device__ __forceinline__ void begin() { slot = step_idx[0] & 1; }
  template <int VEC>
  __device__ __forceinline__ void load(const float* __restrict__ cf, long long idx) {
    alpha_s = cf[0], sig_s = cf[1], Ac = cf[2], Bc = cf[3], Cc = cf[4], Dc = cf[5], Ap = cf[6], Bp = cf[7], Cp = cf[8];
    convert = cf[9] != 0.f, corr = cf[10] != 0.f, c2 = cf[11] != 0.f, p2 = cf[12] != 0.f;
    if (corr) {
      const fvec_t<VEC> v = *reinterpret_cast<const fvec_t<VEC>*>(state + idx);
#pragma unroll
      for (int k = 0; k < VEC; ++k) last[k] = v[k];
    }
    if (corr || p2) {
      const fvec_t<VEC> v = *reinterpret_cast<const fvec_t<VEC>*>(state + (2 - slot) * total + idx);
#pragma unroll
      for (int k = 0; k < VEC; ++k) m0[k] = v[k];
    }
    if (c2) {
      const fvec_t<VEC> v = *reinterpret_cast<const fvec_t<VEC>*>(state + (1 + slot) * total + idx);
#pragma unroll
      for (int k = 0; k < VEC; ++k) m1[k] = v[k];
    }
  }
  template <int VEC>
  __device__ __forceinline__ float update(int k, float eu, float et, float xv, int cfg, float g) {
    mt[k] = dpm_model_output(eu, et, xv, cfg, g, alpha_s, sig_s, convert);
    xc[k] = corr ? unipc_correct(last[k], m0[k], c2 ? m1[k] : m0[k], mt[k], Ac, Bc, Cc, Dc) : xv;
    return unipc_predict(xc[k], p2 ? m0[k] : mt[k], mt[k], Ap, Bp, Cp);
  }
  template <int VEC>
  __device__ __forceinline__ fvec_t<VEC> blend_noise(const float* __restrict__ noise, long long idx) const {
    return *reinterpret_cast<const fvec_t<VEC>*>(noise + idx);
  }
  __device__ __forceinline__ float after_blend(int, float r) const { return r; }
  __device__ __forceinline__ float unet_input(float r) const { return r; }
  template <int VEC>
  __device__ __forceinline__ void store(long long idx) {
    fvec_t<VEC> v, w;
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = xc[k], w[k] = mt[k];
    *reinterpret_cast<fvec_t<VEC>*>(state + idx) = v;
    *reinterpret_cast<fvec_t<VEC>*>(state + (1 + slot) * total + idx) = w;
  }
  __device__ __forceinline__ void advance() {}
};

// Windowed denoising (long-form generation): the latent x [B][rows][wc] (wc = W * C floats per row) is LONG, the
// UNet ran on K windows of hw rows each as batch rows, and three small read-only tables say how they lie (longform.py WindowPlan):
//   offset[K]         the long row of window k's row 0; window k's row i is long row (offset[k] + i) mod rows
//   cover[rows][KC]   the windows over long row r, ascending, -1 behind the last
//   weight[rows][KC]  their blend weights (positive, sum 1)
// Window k of clip b is batch row b * K + k: eps [half][b][k][hw][wc] and the next UNet input x_in have that layout.  The tables are
// plain device memory, never written by a launch that reads them; an entry outside [0, K) or a row outside the window ends the
// row's list, so no table content can send an access out of bounds.
constexpr int WIN_MAX_COVER = 4;

struct Windows {
  const int* offset;
  const int* cover;
  const float* weight;
  int K, KC, rows, hw;
  long long wc;
};

// the element offset of long row r (column c of clip b) inside window k's batch row, or -1 where the window does not hold it
__device__ __forceinline__ long long window_elem(const Windows& w, long long b, int r, long long c, int k) {
  if (k < 0 || k >= w.K) return -1;
  int i = r - w.offset[k];
  if (i < 0) i += w.rows;
  if (i < 0 || i >= w.hw) return -1;
  return ((b * w.K + k) * w.hw + i) * w.wc + c;
}

// One long row's blend of VEC consecutive elements: e = weight[r][0] win_0, then e = fma(weight[r][j], win_j, e) for j = 1 .. in table
// order -- THE order of the contract (a single window of weight 1.0 returns its element bit for bit; the product is rounded on its
// own, never contracted into the caller's arithmetic).  `base[j]` receives window j's element offset (-1 from the end of the list on).
template <int VEC>
__device__ __forceinline__ void window_blend_row(const Windows& w, const float* __restrict__ src, const float* __restrict__ src2,
                                                 long long b, int r, long long c, long long (&base)[WIN_MAX_COVER], fvec_t<VEC>& e,
                                                 fvec_t<VEC>& e2) {
  typedef fvec_t<VEC> fvec;
  const int* cv = w.cover + (long long)r * w.KC;
  const float* wt = w.weight + (long long)r * w.KC;
  bool live = true;
#pragma unroll
  for (int k = 0; k < VEC; ++k) e[k] = 0.f, e2[k] = 0.f;
#pragma unroll
  for (int j = 0; j < WIN_MAX_COVER; ++j) {
    base[j] = -1;
    if (live && j < w.KC) base[j] = window_elem(w, b, r, c, cv[j]);
    live = base[j] >= 0;
    if (live) {
      const float wj = wt[j];
      const fvec v = *reinterpret_cast<const fvec*>(src + base[j]);
      fvec v2 = v;
      if (src2) v2 = *reinterpret_cast<const fvec*>(src2 + base[j]);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (j == 0) {
#pragma clang fp contract(off)
          e[k] = wj * v[k];
          e2[k] = wj * v2[k];
        } else {
          e[k] = fmaf(wj, v[k], e[k]);
          e2[k] = fmaf(wj, v2[k], e2[k]);
        }
      }
    }
  }
}

// The whole per-step bookkeeping of the replayed denoise loop as ONE launch behind the UNet: classifier-free guidance + the solver's
// update (DDIM: as cfg_ddim_step_kernel), the inpainting blend after it (MASKED, see inpaint_blend), the bf16 input of the next UNet
// call, the NEXT step's row of the precomputed time-embedding table gathered into `rowbias`, and the device-side step counter
// advanced.  Every workgroup reads the counter when it starts; the one that finishes LAST (an agent-scope ticket) writes the new
// value, so no workgroup can see the counter move under it -- three launches become one.
// VEC elements per thread (4 when B * n % 4 == 0): a quarter of the workgroups means a quarter of the same-address ticket atomics,
// which were most of this launch's 8.4 us (500 workgroups at one thread per element).
// The eight kernels below keep their own parameter lists (the first 64 bytes, preloaded into SGPRs, hold coef and step_idx, which the
// first dependent load needs; the unmasked ones carry no inpainting operand) and instantiate this frame with their solver.  They form
// the thread index `tix` themselves: read in here, blockDim.x is not folded to the uniform workgroup size, and every wave starts with
// one more dependent load.
// WINDOWED (the *_windowed[_masked] kernels further down): eps and x_in are per window, x and the solver's state long (Windows above);
// with MASKED also x0, noise and the mask, and the scatter takes the blended value.
template <class Solver, int VEC, bool MASKED, bool WINDOWED = false>
__device__ __forceinline__ void step_fused_body(const float* __restrict__ eps, float* __restrict__ x, int B, long long n, int cfg, float g,
                                                const float* __restrict__ coef, int* __restrict__ step_idx, bf16* __restrict__ x_in,
                                                Solver s, const float* __restrict__ table, long long row_elems, float* __restrict__ rowbias,
                                                const float* __restrict__ timesteps, int n_steps, float* __restrict__ t_out,
                                                unsigned* __restrict__ ticket, long long tix, const Inpaint& ip,
                                                const Windows& win = Windows{}) {
  typedef fvec_t<VEC> fvec;
  typedef bf16 bvec __attribute__((ext_vector_type(VEC)));
  const int cur = step_idx[0];
  int nxt = cur + 1;
  if (nxt >= n_steps) nxt = 0;                                // wrap: a replayed graph may run past the schedule (benchmarks)
  s.begin();
  const long long idx = tix * VEC;
  const long long total = (long long)B * n;
  if (idx < total) {
    // (the operands do not depend on the counter: requested before the coefficient row, which does)
    fvec eu, et;
    long long wbase[WIN_MAX_COVER];
    if constexpr (WINDOWED) {
      // x, the solver's state and idx stay in the long layout; eps is per window: both halves blended into the long row first
      const long long pix = idx / win.wc, b = pix / win.rows;
      window_blend_row<VEC>(win, eps, cfg ? eps + (long long)B * win.K * win.hw * win.wc : nullptr, b, (int)(pix - b * win.rows),
                            idx - pix * win.wc, wbase, eu, et);
    } else {
      eu = *reinterpret_cast<const fvec*>(eps + idx), et = eu;
      if (cfg) et = *reinterpret_cast<const fvec*>(eps + total + idx);
    }
    const fvec xv = *reinterpret_cast<const fvec*>(x + idx);
    fvec kx0, knz;
    if constexpr (MASKED) {
      kx0 = *reinterpret_cast<const fvec*>(ip.x0 + idx);
      if constexpr (!Solver::DRAWS_BLEND_NOISE) knz = s.template blend_noise<VEC>(ip.noise, idx);
    }
    s.template load<VEC>(coef + Solver::ROW * cur, idx);
    if constexpr (MASKED && Solver::DRAWS_BLEND_NOISE) knz = s.template blend_noise<VEC>(ip.noise, idx);   // (drawn by load)
    fvec xn;
    bvec xb;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float r = s.template update<VEC>(k, eu[k], et[k], xv[k], cfg, g);
      if constexpr (MASKED)
        r = inpaint_blend(r, kx0[k], knz[k], ip.mask[(unsigned)(idx + k) / (unsigned)ip.C], ip.blend[2 * cur], ip.blend[2 * cur + 1]);
      r = s.after_blend(k, r);
      xn[k] = r;
      xb[k] = (bf16)s.unet_input(r);
    }
    *reinterpret_cast<fvec*>(x + idx) = xn;
    s.template store<VEC>(idx);
    if constexpr (WINDOWED) {
      // the next UNet input goes into EVERY window that holds this row, both CFG halves
      if (x_in) {
#pragma unroll
        for (int j = 0; j < WIN_MAX_COVER; ++j)
          if (wbase[j] >= 0) {
            *reinterpret_cast<bvec*>(x_in + wbase[j]) = xb;
            if (cfg) *reinterpret_cast<bvec*>(x_in + (long long)B * win.K * win.hw * win.wc + wbase[j]) = xb;
          }
      }
    } else if (x_in) {
      *reinterpret_cast<bvec*>(x_in + idx) = xb;
      if (cfg) *reinterpret_cast<bvec*>(x_in + total + idx) = xb;
    }
  }
  if (table && tix * 4 < row_elems)
    *reinterpret_cast<f32x4*>(rowbias + tix * 4) = *reinterpret_cast<const f32x4*>(table + (long long)nxt * row_elems + tix * 4);
  if constexpr (Solver::TICKET_OPTIONAL)
    if (!ticket) return;                                      // (uniform over the grid)
  __syncthreads();                                            // every thread of this workgroup has read the counter and the solver's state
  if (threadIdx.x == 0) {
    // acq_rel at agent scope: the release half orders this workgroup's reads of step_idx[0] before its ticket, the acquire half orders
    // the last workgroup's stores below after every other workgroup's ticket -- by the memory model, not by an incidental s_waitcnt
    const unsigned done = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (done == gridDim.x - 1) {                              // last workgroup: nobody will read step_idx[0] again in this launch
      ticket[0] = 0;
      step_idx[0] = nxt;
      t_out[0] = timesteps[nxt];
      s.advance();
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void ddim_step_fused_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n, int cfg,
                                                              float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                              bf16* __restrict__ x_in, const float* __restrict__ table, long long row_elems,
                                                              float* __restrict__ rowbias, const float* __restrict__ timesteps, int n_steps,
                                                              float* __restrict__ t_out, unsigned* __restrict__ ticket) {
  step_fused_body<DdimSolver, VEC, false>(eps, x, B, n, cfg, g, coef, step_idx, x_in, DdimSolver{}, table, row_elems, rowbias, timesteps,
                                          n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{});
}

template <int VEC>
__global__ __launch_bounds__(256) void ddim_step_fused_masked_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                     int cfg, float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                                     bf16* __restrict__ x_in, const float* __restrict__ table, long long row_elems,
                                                                     float* __restrict__ rowbias, const float* __restrict__ timesteps, int n_steps,
                                                                     float* __restrict__ t_out, unsigned* __restrict__ ticket,
                                                                     const float* __restrict__ x0, const float* __restrict__ noise,
                                                                     const float* __restrict__ mask, const float* __restrict__ blend, int C) {
  step_fused_body<DdimSolver, VEC, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, DdimSolver{}, table, row_elems, rowbias, timesteps,
                                         n_steps, t_out, ticket,
                                         (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{x0, noise, mask, blend, C});
}

template <int VEC>
__global__ __launch_bounds__(256) void dpm_step_fused_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n, int cfg,
                                                             float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                             bf16* __restrict__ x_in, float* __restrict__ hist, const float* __restrict__ table,
                                                             long long row_elems, float* __restrict__ rowbias, const float* __restrict__ timesteps,
                                                             int n_steps, float* __restrict__ t_out, unsigned* __restrict__ ticket) {
  step_fused_body<DpmSolver, VEC, false>(eps, x, B, n, cfg, g, coef, step_idx, x_in, DpmSolver{hist}, table, row_elems, rowbias, timesteps,
                                         n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{});
}

template <int VEC>
__global__ __launch_bounds__(256) void dpm_step_fused_masked_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                    int cfg, float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                                    bf16* __restrict__ x_in, float* __restrict__ hist, const float* __restrict__ table,
                                                                    long long row_elems, float* __restrict__ rowbias,
                                                                    const float* __restrict__ timesteps, int n_steps, float* __restrict__ t_out,
                                                                    unsigned* __restrict__ ticket, const float* __restrict__ x0,
                                                                    const float* __restrict__ noise, const float* __restrict__ mask,
                                                                    const float* __restrict__ blend, int C) {
  step_fused_body<DpmSolver, VEC, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, DpmSolver{hist}, table, row_elems, rowbias, timesteps,
                                        n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{x0, noise, mask, blend, C});
}

template <int VEC>
__global__ __launch_bounds__(256) void euler_a_step_fused_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n, int cfg,
                                                                 float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                                 bf16* __restrict__ x_in, uint32_t* __restrict__ rng,
                                                                 const float* __restrict__ table, long long row_elems, float* __restrict__ rowbias,
                                                                 const float* __restrict__ timesteps, int n_steps, float* __restrict__ t_out,
                                                                 unsigned* __restrict__ ticket) {
  step_fused_body<EulerASolver, VEC, false>(eps, x, B, n, cfg, g, coef, step_idx, x_in, EulerASolver{rng}, table, row_elems, rowbias,
                                            timesteps, n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{});
}

template <int VEC>
__global__ __launch_bounds__(256) void euler_a_step_fused_masked_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                        int cfg, float g, const float* __restrict__ coef,
                                                                        int* __restrict__ step_idx, bf16* __restrict__ x_in,
                                                                        uint32_t* __restrict__ rng, const float* __restrict__ table,
                                                                        long long row_elems, float* __restrict__ rowbias,
                                                                        const float* __restrict__ timesteps, int n_steps, float* __restrict__ t_out,
                                                                        unsigned* __restrict__ ticket, const float* __restrict__ x0,
                                                                        const float* __restrict__ noise, const float* __restrict__ mask,
                                                                        const float* __restrict__ blend, int C) {
  step_fused_body<EulerASolver, VEC, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, EulerASolver{rng}, table, row_elems, rowbias,
                                           timesteps, n_steps, t_out, ticket,
                                           (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{x0, noise, mask, blend, C});
}

// (euler_a_step_fused_masked_kernel's parameter list; `noise` is carried for the shared launcher and never read)
template <int VEC>
__global__ __launch_bounds__(256) void repaint_step_fused_masked_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                        int cfg, float g, const float* __restrict__ coef,
                                                                        int* __restrict__ step_idx, bf16* __restrict__ x_in,
                                                                        uint32_t* __restrict__ rng, const float* __restrict__ table,
                                                                        long long row_elems, float* __restrict__ rowbias,
                                                                        const float* __restrict__ timesteps, int n_steps, float* __restrict__ t_out,
                                                                        unsigned* __restrict__ ticket, const float* __restrict__ x0,
                                                                        const float* __restrict__ noise, const float* __restrict__ mask,
                                                                        const float* __restrict__ blend, int C) {
  step_fused_body<RepaintSolver, VEC, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, RepaintSolver{rng}, table, row_elems, rowbias,
                                            timesteps, n_steps, t_out, ticket,
                                            (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{x0, noise, mask, blend, C});
}

template <int VEC>
__global__ __launch_bounds__(256) void unipc_step_fused_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n, int cfg,
                                                               float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                               bf16* __restrict__ x_in, float* __restrict__ state,
                                                               const float* __restrict__ table, long long row_elems, float* __restrict__ rowbias,
                                                               const float* __restrict__ timesteps, int n_steps, float* __restrict__ t_out,
                                                               unsigned* __restrict__ ticket) {
  step_fused_body<UniPCSolver, VEC, false>(eps, x, B, n, cfg, g, coef, step_idx, x_in, UniPCSolver{state, step_idx, (long long)B * n}, table,
                                           row_elems, rowbias, timesteps, n_steps, t_out, ticket,
                                           (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{});
}

template <int VEC>
__global__ __launch_bounds__(256) void unipc_step_fused_masked_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                      int cfg, float g, const float* __restrict__ coef,
                                                                      int* __restrict__ step_idx, bf16* __restrict__ x_in,
                                                                      float* __restrict__ state, const float* __restrict__ table,
                                                                      long long row_elems, float* __restrict__ rowbias,
                                                                      const float* __restrict__ timesteps, int n_steps, float* __restrict__ t_out,
                                                                      unsigned* __restrict__ ticket, const float* __restrict__ x0,
                                                                      const float* __restrict__ noise, const float* __restrict__ mask,
                                                                      const float* __restrict__ blend, int C) {
  step_fused_body<UniPCSolver, VEC, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, UniPCSolver{state, step_idx, (long long)B * n}, table,
                                          row_elems, rowbias, timesteps, n_steps, t_out, ticket,
                                          (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{x0, noise, mask, blend, C});
}

// The windowed fused steps: the frame above with WINDOWED, the four solvers unchanged.  Their own parameter list -- the plain kernels'
// (coef and step_idx inside the first 64 bytes), then the plan: offset, cover, weight, K, KC, rows, hw, wc.  n = rows * wc.
template <int VEC>
__global__ __launch_bounds__(256) void ddim_step_fused_windowed_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                        int cfg, float g, const float* __restrict__ coef,
                                                                        int* __restrict__ step_idx, bf16* __restrict__ x_in,
                                                                        const float* __restrict__ table, long long row_elems,
                                                                        float* __restrict__ rowbias, const float* __restrict__ timesteps,
                                                                        int n_steps, float* __restrict__ t_out, unsigned* __restrict__ ticket,
                                                                        const int* offset, const int* cover, const float* weight, int K,
                                                                        int KC, int rows, int hw, long long wc) {
  step_fused_body<DdimSolver, VEC, false, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, DdimSolver{}, table, row_elems, rowbias,
                                              timesteps, n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{},
                                              Windows{offset, cover, weight, K, KC, rows, hw, wc});
}

template <int VEC>
__global__ __launch_bounds__(256) void dpm_step_fused_windowed_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                        int cfg, float g, const float* __restrict__ coef,
                                                                        int* __restrict__ step_idx, bf16* __restrict__ x_in,
                                                                        float* __restrict__ hist, const float* __restrict__ table, long long row_elems,
                                                                        float* __restrict__ rowbias, const float* __restrict__ timesteps,
                                                                        int n_steps, float* __restrict__ t_out, unsigned* __restrict__ ticket,
                                                                        const int* offset, const int* cover, const float* weight, int K,
                                                                        int KC, int rows, int hw, long long wc) {
  step_fused_body<DpmSolver, VEC, false, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, DpmSolver{hist}, table, row_elems, rowbias,
                                              timesteps, n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{},
                                              Windows{offset, cover, weight, K, KC, rows, hw, wc});
}

template <int VEC>
__global__ __launch_bounds__(256) void euler_a_step_fused_windowed_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                        int cfg, float g, const float* __restrict__ coef,
                                                                        int* __restrict__ step_idx, bf16* __restrict__ x_in,
                                                                        uint32_t* __restrict__ rng, const float* __restrict__ table, long long row_elems,
                                                                        float* __restrict__ rowbias, const float* __restrict__ timesteps,
                                                                        int n_steps, float* __restrict__ t_out, unsigned* __restrict__ ticket,
                                                                        const int* offset, const int* cover, const float* weight, int K,
                                                                        int KC, int rows, int hw, long long wc) {
  step_fused_body<EulerASolver, VEC, false, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, EulerASolver{rng}, table, row_elems, rowbias,
                                              timesteps, n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{},
                                              Windows{offset, cover, weight, K, KC, rows, hw, wc});
}

template <int VEC>
__global__ __launch_bounds__(256) void unipc_step_fused_windowed_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                        int cfg, float g, const float* __restrict__ coef,
                                                                        int* __restrict__ step_idx, bf16* __restrict__ x_in,
                                                                        float* __restrict__ state, const float* __restrict__ table, long long row_elems,
                                                                        float* __restrict__ rowbias, const float* __restrict__ timesteps,
                                                                        int n_steps, float* __restrict__ t_out, unsigned* __restrict__ ticket,
                                                                        const int* offset, const int* cover, const float* weight, int K,
                                                                        int KC, int rows, int hw, long long wc) {
  step_fused_body<UniPCSolver, VEC, false, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, UniPCSolver{state, step_idx, (long long)B * n}, table, row_elems, rowbias,
                                              timesteps, n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{},
                                              Windows{offset, cover, weight, K, KC, rows, hw, wc});
}

// The windowed MASKED fused steps (audio-to-audio on a long latent): the frame with MASKED and WINDOWED both.
// x0, noise and the mask are LONG like x ([B][rows][W][C] and [B][rows][W]); the blend runs on the long value after the solver's update
// and before the scatter, so every covering window receives the blended value.  Their own parameter list -- the windowed kernels',
// then the inpainting operands behind the plan.
template <int VEC>
__global__ __launch_bounds__(256) void ddim_step_fused_windowed_masked_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                              int cfg, float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                                              bf16* __restrict__ x_in, const float* __restrict__ table,
                                                                              long long row_elems, float* __restrict__ rowbias, const float* __restrict__ timesteps,
                                                                              int n_steps, float* __restrict__ t_out, unsigned* __restrict__ ticket,
                                                                              const int* offset, const int* cover, const float* weight, int K, int KC, int rows,
                                                                              int hw, long long wc, const float* __restrict__ x0, const float* __restrict__ noise,
                                                                              const float* __restrict__ mask, const float* __restrict__ blend, int C) {
  step_fused_body<DdimSolver, VEC, true, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, DdimSolver{}, table, row_elems, rowbias, timesteps,
      n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{x0, noise, mask, blend, C},
      Windows{offset, cover, weight, K, KC, rows, hw, wc});
}

template <int VEC>
__global__ __launch_bounds__(256) void dpm_step_fused_windowed_masked_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                             int cfg, float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                                             bf16* __restrict__ x_in, float* __restrict__ hist, const float* __restrict__ table,
                                                                             long long row_elems, float* __restrict__ rowbias, const float* __restrict__ timesteps,
                                                                             int n_steps, float* __restrict__ t_out, unsigned* __restrict__ ticket,
                                                                             const int* offset, const int* cover, const float* weight, int K, int KC, int rows,
                                                                             int hw, long long wc, const float* __restrict__ x0, const float* __restrict__ noise,
                                                                             const float* __restrict__ mask, const float* __restrict__ blend, int C) {
  step_fused_body<DpmSolver, VEC, true, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, DpmSolver{hist}, table, row_elems, rowbias, timesteps,
      n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{x0, noise, mask, blend, C},
      Windows{offset, cover, weight, K, KC, rows, hw, wc});
}

template <int VEC>
__global__ __launch_bounds__(256) void euler_a_step_fused_windowed_masked_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                                 int cfg, float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                                                 bf16* __restrict__ x_in, uint32_t* __restrict__ rng, const float* __restrict__ table,
                                                                                 long long row_elems, float* __restrict__ rowbias, const float* __restrict__ timesteps,
                                                                                 int n_steps, float* __restrict__ t_out, unsigned* __restrict__ ticket,
                                                                                 const int* offset, const int* cover, const float* weight, int K, int KC, int rows,
                                                                                 int hw, long long wc, const float* __restrict__ x0, const float* __restrict__ noise,
                                                                                 const float* __restrict__ mask, const float* __restrict__ blend, int C) {
  step_fused_body<EulerASolver, VEC, true, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, EulerASolver{rng}, table, row_elems, rowbias, timesteps,
      n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{x0, noise, mask, blend, C},
      Windows{offset, cover, weight, K, KC, rows, hw, wc});
}

template <int VEC>
__global__ __launch_bounds__(256) void repaint_step_fused_windowed_masked_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                                 int cfg, float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                                                 bf16* __restrict__ x_in, uint32_t* __restrict__ rng, const float* __restrict__ table,
                                                                                 long long row_elems, float* __restrict__ rowbias, const float* __restrict__ timesteps,
                                                                                 int n_steps, float* __restrict__ t_out, unsigned* __restrict__ ticket,
                                                                                 const int* offset, const int* cover, const float* weight, int K, int KC, int rows,
                                                                                 int hw, long long wc, const float* __restrict__ x0, const float* __restrict__ noise,
                                                                                 const float* __restrict__ mask, const float* __restrict__ blend, int C) {
  step_fused_body<RepaintSolver, VEC, true, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, RepaintSolver{rng}, table, row_elems, rowbias, timesteps,
      n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{x0, noise, mask, blend, C},
      Windows{offset, cover, weight, K, KC, rows, hw, wc});
}

template <int VEC>
__global__ __launch_bounds__(256) void unipc_step_fused_windowed_masked_kernel(const float* __restrict__ eps, float* __restrict__ x, int B, long long n,
                                                                               int cfg, float g, const float* __restrict__ coef, int* __restrict__ step_idx,
                                                                               bf16* __restrict__ x_in, float* __restrict__ state, const float* __restrict__ table,
                                                                               long long row_elems, float* __restrict__ rowbias, const float* __restrict__ timesteps,
                                                                               int n_steps, float* __restrict__ t_out, unsigned* __restrict__ ticket,
                                                                               const int* offset, const int* cover, const float* weight, int K, int KC, int rows,
                                                                               int hw, long long wc, const float* __restrict__ x0, const float* __restrict__ noise,
                                                                               const float* __restrict__ mask, const float* __restrict__ blend, int C) {
  step_fused_body<UniPCSolver, VEC, true, true>(eps, x, B, n, cfg, g, coef, step_idx, x_in, UniPCSolver{state, step_idx, (long long)B * n}, table, row_elems, rowbias, timesteps,
      n_steps, t_out, ticket, (long long)blockIdx.x * blockDim.x + threadIdx.x, Inpaint{x0, noise, mask, blend, C},
      Windows{offset, cover, weight, K, KC, rows, hw, wc});
}

// windows out of the long tensor: out[b * K + k][i][:] = x[b][(offset[k] + i) mod rows][:] * mul, bf16 (the UNet / VAE input: the
// rounding of f32_to_bf16_kernel) or fp32.  One thread per VEC elements of the output.
template <int VEC>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ x, const int* __restrict__ offset, int B, int K,
                                                            int rows, int hw, long long wc, float mul, void* __restrict__ out, int out_f32) {
  typedef fvec_t<VEC> fvec;
  typedef bf16 bvec __attribute__((ext_vector_type(VEC)));
  const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (idx >= (long long)B * K * hw * wc) return;
  const long long pix = idx / wc, c = idx - pix * wc;
  const long long bk = pix / hw;
  const int i = (int)(pix - bk * hw), k = (int)(bk % K);
  int r = (offset[k] + i) % rows;
  if (r < 0) r += rows;                                       // (whatever the table holds, the source row is a row of x)
  fvec v = *reinterpret_cast<const fvec*>(x + ((bk / K) * rows + r) * wc + c);
  if (out_f32) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = v[e] * mul;
    *reinterpret_cast<fvec*>(reinterpret_cast<float*>(out) + idx) = v;
  } else {
    bvec o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = (bf16)(v[e] * mul);
    *reinterpret_cast<bvec*>(reinterpret_cast<bf16*>(out) + idx) = o;
  }
}

// windows back into the long tensor: out[b][r][:] = sum_j weight[r][j] win[b * K + cover[r][j]][(r - offset) mod rows][:], in the
// order of window_blend_row.  One thread per VEC elements of the output.
template <int VEC>
__global__ __launch_bounds__(256) void window_blend_kernel(const float* __restrict__ win, int B, long long n, float* __restrict__ out,
                                                           const int* offset, const int* cover, const float* weight, int K, int KC,
                                                           int rows, int hw, long long wc) {
  typedef fvec_t<VEC> fvec;
  const long long idx = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (idx >= (long long)B * n) return;
  const Windows w{offset, cover, weight, K, KC, rows, hw, wc};
  const long long pix = idx / wc, b = pix / rows;
  long long base[WIN_MAX_COVER];
  fvec e, unused;
  window_blend_row<VEC>(w, win, nullptr, b, (int)(pix - b * rows), idx - pix * wc, base, e, unused);
  *reinterpret_cast<fvec*>(out + idx) = e;
}

__global__ void advance_step_kernel(int* step_idx, const float* __restrict__ timesteps, int n_steps, float* t_out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int i = step_idx[0] + 1;
    if (i >= n_steps) i = 0;          // wrap: a replayed graph may run past the schedule (benchmarks)
    step_idx[0] = i;
    t_out[0] = timesteps[i];
  }
}

// out[0 .. row_elems) = table[idx[0]][0 .. row_elems): selects the current DDIM step's row of a precomputed per-step table (the
// time-embedding projections of all steps are computed once per prompt, see engine.py) with a DEVICE-side index, so the replayed
// graph needs no host work between steps.
__global__ __launch_bounds__(256) void gather_row_kernel(const float* __restrict__ table, const int* __restrict__ idx,
                                                         long long row_elems, float* __restrict__ out) {
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= row_elems) return;
  const float* src = table + (long long)idx[0] * row_elems + i;
  *reinterpret_cast<f32x4*>(out + i) = *reinterpret_cast<const f32x4*>(src);
}

__global__ void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                  float* __restrict__ v, long long n, float lr, float b1, float b2, float eps, float wd,
                                  float bc1, float bc2_sqrt, float gscale) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // torch.optim.AdamW (decoupled weight decay), single-tensor formulation
  const float grad = g[i] * gscale;
  float pv = p[i] * (1.f - lr * wd);
  const float mv = b1 * m[i] + (1.f - b1) * grad;
  const float vv = b2 * v[i] + (1.f - b2) * grad * grad;
  m[i] = mv; v[i] = vv;
  const float denom = sqrtf(vv) / bc2_sqrt + eps;
  pv -= (lr / bc1) * (mv / denom);
  p[i] = pv;
}

// ---- gradient-norm clipping over the flat LoRA gradient buffer (torch.nn.utils.clip_grad_norm_, 2-norm) ----
// The norm is TWO steps so that no float atomic is needed and the result is bitwise reproducible: sumsq_flat leaves one partial sum of
// squares per workgroup (a fixed grid: which elements a thread sees, and the order it adds them in, depend on n and npart only), and
// every consumer adds the npart partials itself, in index order, so all of them see the same total.
constexpr int FLAT_THREADS = 256;
constexpr int FLAT_MAX_PARTS = 1024;

// Quads [0, nvec) as 16-byte loads, elements [4 nvec, n) one by one (n is no multiple of anything; nvec = 0 for an unaligned buffer).
__global__ __launch_bounds__(FLAT_THREADS) void sumsq_flat_kernel(const float* __restrict__ g, long long n, long long nvec,
                                                                  float* __restrict__ partials) {
  __shared__ float red[FLAT_THREADS / 64];
  const long long stride = (long long)gridDim.x * FLAT_THREADS;
  const long long t0 = (long long)blockIdx.x * FLAT_THREADS + threadIdx.x;
  float s = 0.f;
  for (long long q = t0; q < nvec; q += stride) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(g + 4 * q);
    s += (x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]);
  }
  for (long long i = 4 * nvec + t0; i < n; i += stride) s += g[i] * g[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// total = sqrt(sum of the partials, in index order) * gscale: the 2-norm of the gradient the optimiser will see (g * gscale), and
// coef = min(1, max_norm / (total + 1e-6)) as clip_grad_norm_ forms it (a NaN norm stays a NaN coefficient, as torch.clamp leaves it).
// One thread adds, everybody reads the pair back from LDS: every workgroup of every consumer computes the same two numbers.
__device__ __forceinline__ void clip_coef(const float* __restrict__ partials, int npart, float gscale, float max_norm, float* sh,
                                          float& total, float& coef) {
  if (threadIdx.x == 0) {
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < npart; ++i) s += partials[i];
    const float t = sqrtf(s) * gscale;
    const float c = max_norm / (t + 1e-6f);
    sh[0] = t;
    sh[1] = c > 1.f ? 1.f : c;
  }
  __syncthreads();
  total = sh[0];
  coef = sh[1];
}

// aldm_adamw_flat on g * gscale * coef, the coefficient taken from device memory (nothing about clipping reaches the host)
__global__ __launch_bounds__(FLAT_THREADS) void adamw_flat_clip_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                       float* __restrict__ m, float* __restrict__ v, long long n,
                                                                       long long nvec, float lr, float b1, float b2, float eps,
                                                                       float wd, float bc1, float bc2_sqrt, float gscale,
                                                                       const float* __restrict__ partials, int npart,
                                                                       float max_norm, float* __restrict__ norm_out) {
  __shared__ float sh[2];
  float total, coef;
  clip_coef(partials, npart, gscale, max_norm, sh, total, coef);
  if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = total;
  struct Pmv { float p, m, v; };
  auto update = [&](float p0, float gv, float m0, float v0) {           // the arithmetic of adamw_flat_kernel, term by term
    const float grad = gv * gscale * coef;
    float pv = p0 * (1.f - lr * wd);
    const float mv = b1 * m0 + (1.f - b1) * grad;
    const float vv = b2 * v0 + (1.f - b2) * grad * grad;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pv -= (lr / bc1) * (mv / denom);
    return Pmv{pv, mv, vv};
  };
  const long long stride = (long long)gridDim.x * FLAT_THREADS;
  const long long t0 = (long long)blockIdx.x * FLAT_THREADS + threadIdx.x;
  for (long long q = t0; q < nvec; q += stride) {
    f32x4 pv = *reinterpret_cast<const f32x4*>(p + 4 * q), mv = *reinterpret_cast<const f32x4*>(m + 4 * q);
    f32x4 vv = *reinterpret_cast<const f32x4*>(v + 4 * q);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + 4 * q);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const Pmv r = update(pv[k], gv[k], mv[k], vv[k]);
      pv[k] = r.p; mv[k] = r.m; vv[k] = r.v;
    }
    *reinterpret_cast<f32x4*>(m + 4 * q) = mv;
    *reinterpret_cast<f32x4*>(v + 4 * q) = vv;
    *reinterpret_cast<f32x4*>(p + 4 * q) = pv;
  }
  for (long long i = 4 * nvec + t0; i < n; i += stride) {
    const Pmv r = update(p[i], g[i], m[i], v[i]);
    m[i] = r.m; v[i] = r.v; p[i] = r.p;
  }
}

// g *= coef in place (the autograd-shaped facade: clip_grad_norm_ must leave scaled .grads behind); coef = 1 leaves every bit as it was
__global__ __launch_bounds__(FLAT_THREADS) void clip_flat_kernel(float* __restrict__ g, long long n, long long nvec,
                                                                 const float* __restrict__ partials, int npart, float max_norm,
                                                                 float gscale, float* __restrict__ norm_out) {
  __shared__ float sh[2];
  float total, coef;
  clip_coef(partials, npart, gscale, max_norm, sh, total, coef);
  if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = total;
  const long long stride = (long long)gridDim.x * FLAT_THREADS;
  const long long t0 = (long long)blockIdx.x * FLAT_THREADS + threadIdx.x;
  for (long long q = t0; q < nvec; q += stride) {
    f32x4 x = *reinterpret_cast<const f32x4*>(g + 4 * q);
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] *= coef;
    *reinterpret_cast<f32x4*>(g + 4 * q) = x;
  }
  for (long long i = 4 * nvec + t0; i < n; i += stride) g[i] *= coef;
}

// acc = first ? g : acc + g (gradient accumulation: the micro-batch's flat gradients + loss slot into the window's buffer)
__global__ __launch_bounds__(FLAT_THREADS) void accum_flat_kernel(float* __restrict__ acc, const float* __restrict__ g, long long n,
                                                                  long long nvec, int first) {
  const long long stride = (long long)gridDim.x * FLAT_THREADS;
  const long long t0 = (long long)blockIdx.x * FLAT_THREADS + threadIdx.x;
  for (long long q = t0; q < nvec; q += stride) {
    f32x4 x = *reinterpret_cast<const f32x4*>(g + 4 * q);
    if (!first) x += *reinterpret_cast<const f32x4*>(acc + 4 * q);
    *reinterpret_cast<f32x4*>(acc + 4 * q) = x;
  }
  for (long long i = 4 * nvec + t0; i < n; i += stride) acc[i] = first ? g[i] : acc[i] + g[i];
}

__global__ void add_noise_kernel(const float* __restrict__ x, const float* __restrict__ nz, const float* __restrict__ coef,
                                 int B, long long n, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * n) return;
  const int b = (int)(idx / n);
  out[idx] = coef[2 * b] * x[idx] + coef[2 * b + 1] * nz[idx];
}

// add_noise with the coefficients taken on the device: noisy = sqrt(abar[t_b]) x + sqrt(1 - abar[t_b]) noise  (t int64 per sample)
__global__ void add_noise_t_kernel(const float* __restrict__ x, const float* __restrict__ nz, const float* __restrict__ abar,
                                   const long long* __restrict__ t, int n_train, int B, long long n, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * n) return;
  const int b = (int)(idx / n);
  long long tb = t[b];
  tb = tb < 0 ? 0 : (tb >= n_train ? n_train - 1 : tb);
  const float a = abar[tb];
  out[idx] = sqrtf(a) * x[idx] + sqrtf(1.f - a) * nz[idx];
}

// DiagonalGaussianDistribution.sample(): params NCHW [B][2C][HW] = (mean | logvar), noise / out [B][C][HW]:
// out = mean + exp(0.5 clamp(logvar, -30, 20)) * noise   (vae.encode(x).latent_dist.sample() [REF train:495])
__global__ void gaussian_sample_kernel(const float* __restrict__ params, const float* __restrict__ nz, int B, long long chw,
                                       float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * chw) return;
  const long long b = idx / chw, r = idx - b * chw;
  const float mean = params[b * 2 * chw + r];
  const float lv = fminf(fmaxf(params[b * 2 * chw + chw + r], -30.f), 20.f);
  out[idx] = mean + __expf(0.5f * lv) * nz[idx];
}

// The training step's batch noising as ONE launch (stream contract: philox.h).  It restates, term by term, what the host-noise path
// runs as seven launches -- nhwc_to_nchw of the moments, gaussian_sample_kernel, the multiply by scaling_factor, add_noise_t_kernel and
// the two nchw_to_nhwc of the noisy latents / the noise -- with all randomness drawn HERE from the Philox state:
//   t_b   = __umulhi(word_b of draw d, T)
//   lat   = (mean + exp(0.5 clamp(logvar, -30, 20)) e) scaling_factor      (moments: fp32 NHWC [B][HW][2C] = mean | logvar, e = draw d + 1)
//         = latents[b][c][p]                                                (latents: fp32 NCHW; draw d + 1 is consumed unused)
//   n'    = n + noise_offset o[b][c]                                        (n = draw d + 2, o = draw d + 3; two roundings, no fma)
//   x_in  = bf16(sqrt(abar[t_b]) lat + sqrt(1 - abar[t_b]) n') ,  target = n'        both NHWC [B][HW][C]
// A thread owns VEC consecutive NCHW elements (VEC = 4: one Philox block of e and of n; VEC = 1: the element's block, its lane) and
// maps each to its NHWC slot on its own, so a block may straddle a channel or a sample.  The first B threads of the grid store
// timesteps / t_f32.  The ordinal moves by 4 by the last-workgroup ticket of the fused sampler steps: every workgroup loads the state
// when it starts, the last one through the agent-scope ticket stores d + 4.  ticket == NULL: the ordinal stays.
template <int VEC>
__global__ __launch_bounds__(256) void train_noise_fused_kernel(uint32_t* __restrict__ rng, const float* __restrict__ abar, int n_train,
                                                                const float* __restrict__ moments, const float* __restrict__ latents,
                                                                float sf, float noise_offset, unsigned B, unsigned C, unsigned HW,
                                                                bf16* __restrict__ x_in, float* __restrict__ target,
                                                                long long* __restrict__ t_out, float* __restrict__ t_f32,
                                                                unsigned* __restrict__ ticket) {
  const PhiloxState s0 = philox_load(rng);
  const unsigned tix = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned chw = C * HW, total = B * chw;               // (the entry point checks total < 2^31)
  if (tix < B) {
    const unsigned t = __umulhi(philox_word1(s0, tix), (unsigned)n_train);
    t_out[tix] = (long long)t;
    t_f32[tix] = (float)t;
  }
  const unsigned idx = tix * VEC;
  if (tix < (total + VEC - 1) / VEC) {
    const PhiloxState s1 = philox_at(s0, 1), s2 = philox_at(s0, 2), s3 = philox_at(s0, 3);
    const f32x4 n4 = philox_normal4(s2, (unsigned long long)(idx >> 2));
    f32x4 e4 = {0.f, 0.f, 0.f, 0.f};
    if (moments) e4 = philox_normal4(s1, (unsigned long long)(idx >> 2));
    unsigned pb = ~0u, pbc = ~0u;
    float ca = 0.f, cs = 0.f, o = 0.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const unsigned i = idx + k;
      const int lane = VEC == 4 ? k : (int)(idx & 3);
      const unsigned b = i / chw, r = i - b * chw, c = r / HW, p = r - c * HW;
      if (b != pb) {                                          // (sample boundary inside the thread's elements: look the coefficients up again)
        const float a = abar[__umulhi(philox_word1(s0, b), (unsigned)n_train)];
        ca = sqrtf(a);
        cs = sqrtf(1.f - a);
        pb = b;
      }
      float nz = lane == 0 ? n4[0] : lane == 1 ? n4[1] : lane == 2 ? n4[2] : n4[3];
      if (noise_offset != 0.f) {                              // (uniform over the grid)
        const unsigned bc = b * C + c;
        if (bc != pbc) {
          o = philox_normal1(s3, bc);
          pbc = bc;
        }
        {
#pragma clang fp contract(off)                                  // two roundings, as the two torch ops of the host recipe: no fma
          const float od = noise_offset * o;
          nz = nz + od;
        }
      }
      const unsigned long long pix = (unsigned long long)b * HW + p;
      float lat;
      if (moments) {
        const float* m = moments + pix * 2 * C;
        const float lv = fminf(fmaxf(m[C + c], -30.f), 20.f);
        const float e = lane == 0 ? e4[0] : lane == 1 ? e4[1] : lane == 2 ? e4[2] : e4[3];
        lat = (m[c] + __expf(0.5f * lv) * e) * sf;
      } else {
        lat = latents[i];
      }
      x_in[pix * C + c] = (bf16)(ca * lat + cs * nz);
      target[pix * C + c] = nz;
    }
  }
  if (!ticket) return;                                        // (uniform over the grid)
  __syncthreads();                                            // every thread of this workgroup has read the RNG state
  if (threadIdx.x == 0) {
    // acq_rel at agent scope, as in step_fused_body
    const unsigned done = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (done == gridDim.x - 1) {
      ticket[0] = 0;
      philox_store_ordinal(rng, philox_at(s0, 4));
    }
  }
}

// Holds the stream busy for ~us microseconds (one wave polling the 100 MHz real-time counter).  Measurement aid: lets a
// host that enqueues slower than the GPU executes build up a queue, so per-kernel event pairs time kernels, not host gaps.
__global__ void sleep_kernel(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" int aldm_timestep_embedding(const float* t, int t_stride, int B, int dim, void* out, void* stream) {
  ALDM_CHECK_ARG(t && out && B > 0 && dim > 0 && dim % 2 == 0 && (t_stride == 0 || t_stride == 1), "timestep_embedding: bad args");
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(blocks_for((long long)B * dim, 256)), dim3(256), 0, (hipStream_t)stream, t, t_stride, B, dim, (bf16*)out);
  return aldm_launch_status("timestep_embedding");
}

extern "C" int aldm_silu(const void* x, long long n, void* y, void* stream) {
  ALDM_CHECK_ARG(x && y && n > 0, "silu: bad args");
  hipLaunchKernelGGL(silu_kernel, dim3(blocks_for((n + 7) / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, n, (bf16*)y);
  return aldm_launch_status("silu");
}

extern "C" int aldm_nchw_f32_to_nhwc(const float* x, int B, int C, int HW, void* y, int y_is_f32, void* stream) {
  ALDM_CHECK_ARG(x && y && B > 0 && C > 0 && HW > 0, "nchw_to_nhwc: bad args");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(blocks_for((long long)B * C * HW, 256)), dim3(256), 0, (hipStream_t)stream, x, B, C, HW, y, y_is_f32);
  return aldm_launch_status("nchw_to_nhwc");
}

extern "C" int aldm_nhwc_to_nchw_f32(const void* x, int x_is_f32, int B, int C, int HW, float* y, void* stream) {
  ALDM_CHECK_ARG(x && y && B > 0 && C > 0 && HW > 0, "nhwc_to_nchw: bad args");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(blocks_for((long long)B * C * HW, 256)), dim3(256), 0, (hipStream_t)stream, x, x_is_f32, B, C, HW, y);
  return aldm_launch_status("nhwc_to_nchw");
}

extern "C" int aldm_f32_to_bf16(const float* x, long long n, float mul, void* y, void* stream) {
  ALDM_CHECK_ARG(x && y && n > 0, "f32_to_bf16: bad args");
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n, mul, (bf16*)y);
  return aldm_launch_status("f32_to_bf16");
}

extern "C" int aldm_cfg_ddim_step(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                  const float* coef, const int* step_idx, void* x_in_bf16, void* stream) {
  ALDM_CHECK_ARG(eps && x && coef && step_idx && B > 0 && n_per_sample > 0, "cfg_ddim_step: bad args");
  hipLaunchKernelGGL(cfg_ddim_step_kernel, dim3(blocks_for((long long)B * n_per_sample, 256)), dim3(256), 0, (hipStream_t)stream, eps, x, B, n_per_sample, cfg, guidance, coef, step_idx, (bf16*)x_in_bf16);
  return aldm_launch_status("cfg_ddim_step");
}

// The host half of the fused step's frame (step_fused_body): the argument checks, one thread per VEC elements or per four floats of the
// table row (whichever asks for more), and the VEC dispatch.  `k4` / `k1` are the entry's kernel at VEC = 4 and 1; `op` is the
// solver's extra operand (none for DDIM), which the kernels take between x_in and table; the masked kernels end with the inpainting
// operands (Inpaint above).  The mask is indexed by element / C in 32 bits, so B * n_per_sample must stay below 2^31 there.
template <class Solver, bool MASKED, class Kernel, class... Op>
static int launch_step_fused(const char* name, Kernel k4, Kernel k1, const float* eps, float* x, int B, long long n_per_sample, int cfg,
                             float guidance, const float* coef, int* step_idx, void* x_in_bf16, const float* table, long long row_elems,
                             float* rowbias, const float* timesteps, int n_steps, float* t_out, unsigned* ticket, const Inpaint& ip,
                             void* stream, Op... op) {
  ALDM_CHECK_ARG(eps && x && coef && step_idx && (... && op) && B > 0 && n_per_sample > 0 && n_steps > 0, "%s: bad args", name);
  ALDM_CHECK_ARG(Solver::TICKET_OPTIONAL || ticket, "%s: bad args", name);
  ALDM_CHECK_ARG(!ticket || (timesteps && t_out), "%s: the counter advance needs timesteps and t_out", name);
  ALDM_CHECK_ARG(!table || (ticket && rowbias && row_elems > 0 && row_elems % 4 == 0),
                 "%s: table needs ticket, rowbias and row_elems %% 4 == 0", name);
  if constexpr (MASKED)
    ALDM_CHECK_ARG(ip.x0 && (ip.noise || Solver::DRAWS_BLEND_NOISE) && ip.mask && ip.blend && ip.C > 0 && n_per_sample % ip.C == 0 && (long long)B * n_per_sample < (1ll << 31),
                   "%s: bad inpainting args", name);
  if (!table) row_elems = 0;
  const long long total = (long long)B * n_per_sample;
  const bool v4 = total % 4 == 0;                       // (torch allocations are 16-byte aligned; CFG's second half starts at `total`)
  const long long items = v4 ? total / 4 : total;
  const long long work = items > row_elems / 4 ? items : row_elems / 4;
  auto launch = [&](auto... inpaint) {
    hipLaunchKernelGGL(v4 ? k4 : k1, dim3(blocks_for(work, 256)), dim3(256), 0, (hipStream_t)stream, eps, x, B, n_per_sample, cfg, guidance,
                       coef, step_idx, (bf16*)x_in_bf16, op..., table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, inpaint...);
  };
  if constexpr (MASKED)
    launch(ip.x0, ip.noise, ip.mask, ip.blend, ip.C);
  else
    launch();
  return aldm_launch_status(name);
}

extern "C" int aldm_ddim_step_fused(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance, const float* coef,
                                    int* step_idx, void* x_in_bf16, const float* table, long long row_elems, float* rowbias,
                                    const float* timesteps, int n_steps, float* t_out, unsigned* ticket, void* stream) {
  return launch_step_fused<DdimSolver, false>("ddim_step_fused", ddim_step_fused_kernel<4>, ddim_step_fused_kernel<1>, eps, x, B, n_per_sample,
                                              cfg, guidance, coef, step_idx, x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out,
                                              ticket, Inpaint{}, stream);
}

extern "C" int aldm_dpm_step_fused(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance, const float* coef,
                                   int* step_idx, void* x_in_bf16, float* hist, const float* table, long long row_elems, float* rowbias,
                                   const float* timesteps, int n_steps, float* t_out, unsigned* ticket, void* stream) {
  return launch_step_fused<DpmSolver, false>("dpm_step_fused", dpm_step_fused_kernel<4>, dpm_step_fused_kernel<1>, eps, x, B, n_per_sample,
                                             cfg, guidance, coef, step_idx, x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out,
                                             ticket, Inpaint{}, stream, hist);
}

// the masked launches: the same arguments as their unmasked counterparts, then the inpainting operands
extern "C" int aldm_ddim_step_fused_masked(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance, const float* coef,
                                           int* step_idx, void* x_in_bf16, const float* table, long long row_elems, float* rowbias,
                                           const float* timesteps, int n_steps, float* t_out, unsigned* ticket, const float* x0,
                                           const float* noise, const float* mask, const float* blend, int channels, void* stream) {
  return launch_step_fused<DdimSolver, true>("ddim_step_fused_masked", ddim_step_fused_masked_kernel<4>, ddim_step_fused_masked_kernel<1>, eps,
                                             x, B, n_per_sample, cfg, guidance, coef, step_idx, x_in_bf16, table, row_elems, rowbias, timesteps,
                                             n_steps, t_out, ticket, Inpaint{x0, noise, mask, blend, channels}, stream);
}

extern "C" int aldm_dpm_step_fused_masked(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance, const float* coef,
                                          int* step_idx, void* x_in_bf16, float* hist, const float* table, long long row_elems, float* rowbias,
                                          const float* timesteps, int n_steps, float* t_out, unsigned* ticket, const float* x0,
                                          const float* noise, const float* mask, const float* blend, int channels, void* stream) {
  return launch_step_fused<DpmSolver, true>("dpm_step_fused_masked", dpm_step_fused_masked_kernel<4>, dpm_step_fused_masked_kernel<1>, eps, x,
                                            B, n_per_sample, cfg, guidance, coef, step_idx, x_in_bf16, table, row_elems, rowbias, timesteps,
                                            n_steps, t_out, ticket, Inpaint{x0, noise, mask, blend, channels}, stream, hist);
}

// the Euler-ancestral fused steps: aldm_dpm_step_fused's argument list with the Philox state {seed_lo, seed_hi, draw_lo, draw_hi} in the
// place of the history buffer
extern "C" int aldm_euler_a_step_fused(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance, const float* coef,
                                       int* step_idx, void* x_in_bf16, unsigned* rng_state, const float* table, long long row_elems,
                                       float* rowbias, const float* timesteps, int n_steps, float* t_out, unsigned* ticket, void* stream) {
  return launch_step_fused<EulerASolver, false>("euler_a_step_fused", euler_a_step_fused_kernel<4>, euler_a_step_fused_kernel<1>, eps, x, B,
                                                n_per_sample, cfg, guidance, coef, step_idx, x_in_bf16, table, row_elems, rowbias, timesteps,
                                                n_steps, t_out, ticket, Inpaint{}, stream, rng_state);
}

extern "C" int aldm_euler_a_step_fused_masked(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                              const float* coef, int* step_idx, void* x_in_bf16, unsigned* rng_state, const float* table,
                                              long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                              unsigned* ticket, const float* x0, const float* noise, const float* mask, const float* blend,
                                              int channels, void* stream) {
  return launch_step_fused<EulerASolver, true>("euler_a_step_fused_masked", euler_a_step_fused_masked_kernel<4>,
                                               euler_a_step_fused_masked_kernel<1>, eps, x, B, n_per_sample, cfg, guidance, coef, step_idx,
                                               x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out, ticket,
                                               Inpaint{x0, noise, mask, blend, channels}, stream, rng_state);
}

// the RePaint fused step: aldm_euler_a_step_fused_masked's argument list; `noise` is not read (the blend's noise is drawn in the
// kernel) and may be NULL
extern "C" int aldm_repaint_step_fused_masked(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                              const float* coef, int* step_idx, void* x_in_bf16, unsigned* rng_state, const float* table,
                                              long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                              unsigned* ticket, const float* x0, const float* noise, const float* mask, const float* blend,
                                              int channels, void* stream) {
  return launch_step_fused<RepaintSolver, true>("repaint_step_fused_masked", repaint_step_fused_masked_kernel<4>,
                                                repaint_step_fused_masked_kernel<1>, eps, x, B, n_per_sample, cfg, guidance, coef, step_idx,
                                                x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out, ticket,
                                                Inpaint{x0, noise, mask, blend, channels}, stream, rng_state);
}

// the UniPC fused steps: aldm_dpm_step_fused's argument list with the solver state [3][B][n] (UniPCSolver) in the place of the history
// buffer
extern "C" int aldm_unipc_step_fused(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance, const float* coef,
                                     int* step_idx, void* x_in_bf16, float* state, const float* table, long long row_elems, float* rowbias,
                                     const float* timesteps, int n_steps, float* t_out, unsigned* ticket, void* stream) {
  return launch_step_fused<UniPCSolver, false>("unipc_step_fused", unipc_step_fused_kernel<4>, unipc_step_fused_kernel<1>, eps, x, B,
                                               n_per_sample, cfg, guidance, coef, step_idx, x_in_bf16, table, row_elems, rowbias, timesteps,
                                               n_steps, t_out, ticket, Inpaint{}, stream, state);
}

extern "C" int aldm_unipc_step_fused_masked(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                            const float* coef, int* step_idx, void* x_in_bf16, float* state, const float* table,
                                            long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                            unsigned* ticket, const float* x0, const float* noise, const float* mask, const float* blend,
                                            int channels, void* stream) {
  return launch_step_fused<UniPCSolver, true>("unipc_step_fused_masked", unipc_step_fused_masked_kernel<4>, unipc_step_fused_masked_kernel<1>,
                                              eps, x, B, n_per_sample, cfg, guidance, coef, step_idx, x_in_bf16, table, row_elems, rowbias,
                                              timesteps, n_steps, t_out, ticket, Inpaint{x0, noise, mask, blend, channels}, stream, state);
}

// ---- windowed denoising: the plan's checks, the gather / blend launches and the four windowed fused steps ----
// 0, or the error a plan earns against a long tensor of n_per_sample = rows * wc floats per clip; *wc receives the row width
static int check_window_plan(const char* name, const aldm_window_plan_t* p, int B, long long n_per_sample, bool tables, long long* wc) {
  ALDM_CHECK_ARG(p && p->offset && B > 0 && n_per_sample > 0, "%s: bad args", name);
  ALDM_CHECK_ARG(p->K > 0 && p->rows > 0 && p->hw > 0 && p->hw <= p->rows, "%s: plan needs K > 0 and 0 < hw <= rows (K %d, hw %d, rows %d)",
                 name, p->K, p->hw, p->rows);
  ALDM_CHECK_ARG(p->offset_elems == p->K, "%s: offset holds %lld entries, the plan has K = %d windows", name, p->offset_elems, p->K);
  ALDM_CHECK_ARG(n_per_sample % p->rows == 0, "%s: n_per_sample %lld is no multiple of the plan's %d rows", name, n_per_sample, p->rows);
  if (tables) {
    ALDM_CHECK_ARG(p->cover && p->weight && p->KC >= 1, "%s: bad plan tables", name);
    if (p->KC > WIN_MAX_COVER) {
      aldm_set_error("%s: a row under %d windows; at most %d are supported", name, p->KC, WIN_MAX_COVER);
      return ALDM_E_UNSUPPORTED;
    }
    const long long want = (long long)p->rows * p->KC;
    ALDM_CHECK_ARG(p->cover_elems == want && p->weight_elems == want, "%s: cover / weight hold %lld / %lld entries, rows * KC = %lld", name,
                   p->cover_elems, p->weight_elems, want);
  }
  *wc = n_per_sample / p->rows;
  return ALDM_OK;
}

extern "C" int aldm_window_gather(const float* x, int B, long long n_per_sample, float mul, void* out, int out_is_f32,
                                  const aldm_window_plan_t* plan, void* stream) {
  ALDM_CHECK_ARG(x && out, "window_gather: bad args");
  long long wc;
  if (const int rc = check_window_plan("window_gather", plan, B, n_per_sample, false, &wc)) return rc;
  const long long total = (long long)B * plan->K * plan->hw * wc;
  if (wc % 4 == 0)
    hipLaunchKernelGGL(window_gather_kernel<4>, dim3(blocks_for(total / 4, 256)), dim3(256), 0, (hipStream_t)stream, x, plan->offset, B,
                       plan->K, plan->rows, plan->hw, wc, mul, out, out_is_f32);
  else
    hipLaunchKernelGGL(window_gather_kernel<1>, dim3(blocks_for(total, 256)), dim3(256), 0, (hipStream_t)stream, x, plan->offset, B, plan->K,
                       plan->rows, plan->hw, wc, mul, out, out_is_f32);
  return aldm_launch_status("window_gather");
}

extern "C" int aldm_window_blend(const float* win, int B, long long n_per_sample, float* out, const aldm_window_plan_t* plan, void* stream) {
  ALDM_CHECK_ARG(win && out, "window_blend: bad args");
  long long wc;
  if (const int rc = check_window_plan("window_blend", plan, B, n_per_sample, true, &wc)) return rc;
  const long long total = (long long)B * n_per_sample;
  if (wc % 4 == 0)
    hipLaunchKernelGGL(window_blend_kernel<4>, dim3(blocks_for(total / 4, 256)), dim3(256), 0, (hipStream_t)stream, win, B, n_per_sample, out,
                       plan->offset, plan->cover, plan->weight, plan->K, plan->KC, plan->rows, plan->hw, wc);
  else
    hipLaunchKernelGGL(window_blend_kernel<1>, dim3(blocks_for(total, 256)), dim3(256), 0, (hipStream_t)stream, win, B, n_per_sample, out,
                       plan->offset, plan->cover, plan->weight, plan->K, plan->KC, plan->rows, plan->hw, wc);
  return aldm_launch_status("window_blend");
}

// launch_step_fused for the windowed kernels: the same checks and grid (one thread per VEC long elements or per four floats of the
// table row), VEC = 4 only where a vector stays inside a row (wc % 4 == 0), and the plan behind the frame's operands
template <class Solver, class Kernel, class... Op>
static int launch_step_fused_windowed(const char* name, Kernel k4, Kernel k1, const float* eps, float* x, int B, long long n_per_sample,
                                      int cfg, float guidance, const float* coef, int* step_idx, void* x_in_bf16, const float* table,
                                      long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                      unsigned* ticket, const aldm_window_plan_t* plan, void* stream, Op... op) {
  ALDM_CHECK_ARG(eps && x && coef && step_idx && (... && op) && B > 0 && n_per_sample > 0 && n_steps > 0, "%s: bad args", name);
  ALDM_CHECK_ARG(Solver::TICKET_OPTIONAL || ticket, "%s: bad args", name);
  ALDM_CHECK_ARG(!ticket || (timesteps && t_out), "%s: the counter advance needs timesteps and t_out", name);
  ALDM_CHECK_ARG(!table || (ticket && rowbias && row_elems > 0 && row_elems % 4 == 0),
                 "%s: table needs ticket, rowbias and row_elems %% 4 == 0", name);
  long long wc;
  if (const int rc = check_window_plan(name, plan, B, n_per_sample, true, &wc)) return rc;
  if (!table) row_elems = 0;
  const long long total = (long long)B * n_per_sample;
  const bool v4 = wc % 4 == 0;
  const long long items = v4 ? total / 4 : total;
  const long long work = items > row_elems / 4 ? items : row_elems / 4;
  hipLaunchKernelGGL(v4 ? k4 : k1, dim3(blocks_for(work, 256)), dim3(256), 0, (hipStream_t)stream, eps, x, B, n_per_sample, cfg, guidance, coef,
                     step_idx, (bf16*)x_in_bf16, op..., table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, plan->offset,
                     plan->cover, plan->weight, plan->K, plan->KC, plan->rows, plan->hw, wc);
  return aldm_launch_status(name);
}

extern "C" int aldm_ddim_step_fused_windowed(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                             const float* coef, int* step_idx, void* x_in_bf16, const float* table, long long row_elems,
                                             float* rowbias, const float* timesteps, int n_steps, float* t_out, unsigned* ticket,
                                             const aldm_window_plan_t* plan, void* stream) {
  return launch_step_fused_windowed<DdimSolver>("ddim_step_fused_windowed", ddim_step_fused_windowed_kernel<4>,
                                                ddim_step_fused_windowed_kernel<1>, eps, x, B, n_per_sample, cfg, guidance, coef, step_idx,
                                                x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, plan, stream);
}

extern "C" int aldm_dpm_step_fused_windowed(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                            const float* coef, int* step_idx, void* x_in_bf16, float* hist, const float* table,
                                            long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                            unsigned* ticket, const aldm_window_plan_t* plan, void* stream) {
  return launch_step_fused_windowed<DpmSolver>("dpm_step_fused_windowed", dpm_step_fused_windowed_kernel<4>, dpm_step_fused_windowed_kernel<1>,
                                               eps, x, B, n_per_sample, cfg, guidance, coef, step_idx, x_in_bf16, table, row_elems, rowbias,
                                               timesteps, n_steps, t_out, ticket, plan, stream, hist);
}

extern "C" int aldm_euler_a_step_fused_windowed(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                                const float* coef, int* step_idx, void* x_in_bf16, unsigned* rng_state, const float* table,
                                                long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                                unsigned* ticket, const aldm_window_plan_t* plan, void* stream) {
  return launch_step_fused_windowed<EulerASolver>("euler_a_step_fused_windowed", euler_a_step_fused_windowed_kernel<4>,
                                                  euler_a_step_fused_windowed_kernel<1>, eps, x, B, n_per_sample, cfg, guidance, coef,
                                                  step_idx, x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, plan,
                                                  stream, rng_state);
}

extern "C" int aldm_unipc_step_fused_windowed(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                              const float* coef, int* step_idx, void* x_in_bf16, float* state, const float* table,
                                              long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                              unsigned* ticket, const aldm_window_plan_t* plan, void* stream) {
  return launch_step_fused_windowed<UniPCSolver>("unipc_step_fused_windowed", unipc_step_fused_windowed_kernel<4>,
                                                 unipc_step_fused_windowed_kernel<1>, eps, x, B, n_per_sample, cfg, guidance, coef, step_idx,
                                                 x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, plan, stream, state);
}

// launch_step_fused_windowed for the masked windowed kernels: its checks joined with launch_step_fused<.., true>'s (the inpainting
// operands, n % C == 0, the 32-bit mask index), and the inpainting operands behind the plan.  A rejected call launches nothing.
template <class Solver, class Kernel, class... Op>
static int launch_step_fused_windowed_masked(const char* name, Kernel k4, Kernel k1, const float* eps, float* x, int B, long long n_per_sample,
                                             int cfg, float guidance, const float* coef, int* step_idx, void* x_in_bf16, const float* table,
                                             long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                             unsigned* ticket, const aldm_window_plan_t* plan, const Inpaint& ip, void* stream, Op... op) {
  ALDM_CHECK_ARG(eps && x && coef && step_idx && (... && op) && B > 0 && n_per_sample > 0 && n_steps > 0, "%s: bad args", name);
  ALDM_CHECK_ARG(Solver::TICKET_OPTIONAL || ticket, "%s: bad args", name);
  ALDM_CHECK_ARG(!ticket || (timesteps && t_out), "%s: the counter advance needs timesteps and t_out", name);
  ALDM_CHECK_ARG(!table || (ticket && rowbias && row_elems > 0 && row_elems % 4 == 0),
                 "%s: table needs ticket, rowbias and row_elems %% 4 == 0", name);
  ALDM_CHECK_ARG(ip.x0 && (ip.noise || Solver::DRAWS_BLEND_NOISE) && ip.mask && ip.blend && ip.C > 0 && n_per_sample % ip.C == 0 && (long long)B * n_per_sample < (1ll << 31),
                 "%s: bad inpainting args", name);
  long long wc;
  if (const int rc = check_window_plan(name, plan, B, n_per_sample, true, &wc)) return rc;
  if (!table) row_elems = 0;
  const long long total = (long long)B * n_per_sample;
  const bool v4 = wc % 4 == 0;
  const long long items = v4 ? total / 4 : total;
  const long long work = items > row_elems / 4 ? items : row_elems / 4;
  hipLaunchKernelGGL(v4 ? k4 : k1, dim3(blocks_for(work, 256)), dim3(256), 0, (hipStream_t)stream, eps, x, B, n_per_sample, cfg, guidance, coef,
                     step_idx, (bf16*)x_in_bf16, op..., table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, plan->offset,
                     plan->cover, plan->weight, plan->K, plan->KC, plan->rows, plan->hw, wc, ip.x0, ip.noise, ip.mask, ip.blend, ip.C);
  return aldm_launch_status(name);
}

extern "C" int aldm_ddim_step_fused_windowed_masked(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                                    const float* coef, int* step_idx, void* x_in_bf16, const float* table,
                                                    long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                                    unsigned* ticket, const aldm_window_plan_t* plan, const float* x0, const float* noise,
                                                    const float* mask, const float* blend, int channels, void* stream) {
  return launch_step_fused_windowed_masked<DdimSolver>("ddim_step_fused_windowed_masked", ddim_step_fused_windowed_masked_kernel<4>,
                                                ddim_step_fused_windowed_masked_kernel<1>, eps, x, B, n_per_sample, cfg, guidance, coef,
                                                step_idx, x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, plan,
                                                Inpaint{x0, noise, mask, blend, channels}, stream);
}

extern "C" int aldm_dpm_step_fused_windowed_masked(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                                   const float* coef, int* step_idx, void* x_in_bf16, float* hist, const float* table,
                                                   long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                                   unsigned* ticket, const aldm_window_plan_t* plan, const float* x0, const float* noise,
                                                   const float* mask, const float* blend, int channels, void* stream) {
  return launch_step_fused_windowed_masked<DpmSolver>("dpm_step_fused_windowed_masked", dpm_step_fused_windowed_masked_kernel<4>,
                                                dpm_step_fused_windowed_masked_kernel<1>, eps, x, B, n_per_sample, cfg, guidance, coef,
                                                step_idx, x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, plan,
                                                Inpaint{x0, noise, mask, blend, channels}, stream, hist);
}

extern "C" int aldm_euler_a_step_fused_windowed_masked(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                                       const float* coef, int* step_idx, void* x_in_bf16, unsigned* rng_state, const float* table,
                                                       long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                                       unsigned* ticket, const aldm_window_plan_t* plan, const float* x0, const float* noise,
                                                       const float* mask, const float* blend, int channels, void* stream) {
  return launch_step_fused_windowed_masked<EulerASolver>("euler_a_step_fused_windowed_masked", euler_a_step_fused_windowed_masked_kernel<4>,
                                                euler_a_step_fused_windowed_masked_kernel<1>, eps, x, B, n_per_sample, cfg, guidance, coef,
                                                step_idx, x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, plan,
                                                Inpaint{x0, noise, mask, blend, channels}, stream, rng_state);
}

extern "C" int aldm_repaint_step_fused_windowed_masked(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                                       const float* coef, int* step_idx, void* x_in_bf16, unsigned* rng_state, const float* table,
                                                       long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                                       unsigned* ticket, const aldm_window_plan_t* plan, const float* x0, const float* noise,
                                                       const float* mask, const float* blend, int channels, void* stream) {
  return launch_step_fused_windowed_masked<RepaintSolver>("repaint_step_fused_windowed_masked", repaint_step_fused_windowed_masked_kernel<4>,
                                                repaint_step_fused_windowed_masked_kernel<1>, eps, x, B, n_per_sample, cfg, guidance, coef,
                                                step_idx, x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, plan,
                                                Inpaint{x0, noise, mask, blend, channels}, stream, rng_state);
}

extern "C" int aldm_unipc_step_fused_windowed_masked(const float* eps, float* x, int B, long long n_per_sample, int cfg, float guidance,
                                                     const float* coef, int* step_idx, void* x_in_bf16, float* state, const float* table,
                                                     long long row_elems, float* rowbias, const float* timesteps, int n_steps, float* t_out,
                                                     unsigned* ticket, const aldm_window_plan_t* plan, const float* x0, const float* noise,
                                                     const float* mask, const float* blend, int channels, void* stream) {
  return launch_step_fused_windowed_masked<UniPCSolver>("unipc_step_fused_windowed_masked", unipc_step_fused_windowed_masked_kernel<4>,
                                                unipc_step_fused_windowed_masked_kernel<1>, eps, x, B, n_per_sample, cfg, guidance, coef,
                                                step_idx, x_in_bf16, table, row_elems, rowbias, timesteps, n_steps, t_out, ticket, plan,
                                                Inpaint{x0, noise, mask, blend, channels}, stream, state);
}

extern "C" int aldm_add_noise(const float* x, const float* noise, const float* coef, int B, long long n_per_sample,
                              float* out, void* stream) {
  ALDM_CHECK_ARG(x && noise && coef && out && B > 0 && n_per_sample > 0, "add_noise: bad args");
  hipLaunchKernelGGL(add_noise_kernel, dim3(blocks_for((long long)B * n_per_sample, 256)), dim3(256), 0, (hipStream_t)stream, x, noise, coef, B, n_per_sample, out);
  return aldm_launch_status("add_noise");
}

extern "C" int aldm_add_noise_t(const float* x, const float* noise, const float* alphas_cumprod, const long long* timesteps,
                                int n_train, int B, long long n_per_sample, float* out, void* stream) {
  ALDM_CHECK_ARG(x && noise && alphas_cumprod && timesteps && out && B > 0 && n_per_sample > 0 && n_train > 0, "add_noise_t: bad args");
  hipLaunchKernelGGL(add_noise_t_kernel, dim3(blocks_for((long long)B * n_per_sample, 256)), dim3(256), 0, (hipStream_t)stream, x, noise,
                     alphas_cumprod, timesteps, n_train, B, n_per_sample, out);
  return aldm_launch_status("add_noise_t");
}

extern "C" int aldm_gaussian_sample(const float* params, const float* noise, int B, long long chw, float* out, void* stream) {
  ALDM_CHECK_ARG(params && noise && out && B > 0 && chw > 0, "gaussian_sample: bad args");
  hipLaunchKernelGGL(gaussian_sample_kernel, dim3(blocks_for((long long)B * chw, 256)), dim3(256), 0, (hipStream_t)stream, params, noise,
                     B, chw, out);
  return aldm_launch_status("gaussian_sample");
}

extern "C" int aldm_train_noise_fused(unsigned* rng_state, const float* alphas_cumprod, int n_train, const float* moments,
                                      const float* latents, float scaling_factor, float noise_offset, int B, int C, int H, int W,
                                      void* x_in_bf16, float* target, long long* timesteps, float* t_f32, unsigned* ticket, void* stream) {
  ALDM_CHECK_ARG(rng_state && alphas_cumprod && x_in_bf16 && target && timesteps && t_f32 && n_train > 0, "train_noise_fused: bad args");
  ALDM_CHECK_ARG((moments != nullptr) != (latents != nullptr), "train_noise_fused: give the moments or the latents, not both");
  ALDM_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && (long long)B * C * H * W < (1ll << 31), "train_noise_fused: bad geometry");
  const long long total = (long long)B * C * H * W;
  const int vec = total % 4 == 0 ? 4 : 1;
  const long long work = (total + vec - 1) / vec;
  const unsigned nblk = blocks_for(work > B ? work : (long long)B, 256);     // (the first B threads store the timesteps)
  if (vec == 4)
    hipLaunchKernelGGL(train_noise_fused_kernel<4>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, rng_state, alphas_cumprod, n_train, moments,
                       latents, scaling_factor, noise_offset, (unsigned)B, (unsigned)C, (unsigned)(H * W), (bf16*)x_in_bf16, target, timesteps,
                       t_f32, ticket);
  else
    hipLaunchKernelGGL(train_noise_fused_kernel<1>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, rng_state, alphas_cumprod, n_train, moments,
                       latents, scaling_factor, noise_offset, (unsigned)B, (unsigned)C, (unsigned)(H * W), (bf16*)x_in_bf16, target, timesteps,
                       t_f32, ticket);
  return aldm_launch_status("train_noise_fused");
}

extern "C" int aldm_sleep_us(int us, void* stream) {
  ALDM_CHECK_ARG(us >= 0 && us <= 2000000, "sleep_us: 0 <= us <= 2e6");   // (0: an empty kernel -- bench.py times the graph's kernel boundary with it)
  hipLaunchKernelGGL(sleep_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long)us * 100ull);
  return aldm_launch_status("sleep_us");
}

extern "C" int aldm_advance_step(int* step_idx, const float* timesteps, int n_steps, float* t_out, void* stream) {
  ALDM_CHECK_ARG(step_idx && timesteps && t_out && n_steps > 0, "advance_step: bad args");
  hipLaunchKernelGGL(advance_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step_idx, timesteps, n_steps, t_out);
  return aldm_launch_status("advance_step");
}

extern "C" int aldm_gather_row(const float* table, const int* idx, long long row_elems, float* out, void* stream) {
  ALDM_CHECK_ARG(table && idx && out && row_elems > 0 && row_elems % 4 == 0, "gather_row: bad args (row_elems %% 4 == 0)");
  hipLaunchKernelGGL(gather_row_kernel, dim3(blocks_for(row_elems / 4, 256)), dim3(256), 0, (hipStream_t)stream, table, idx, row_elems, out);
  return aldm_launch_status("gather_row");
}

extern "C" int aldm_adamw_flat(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream) {
  ALDM_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "adamw_flat: bad args");
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
  hipLaunchKernelGGL(adamw_flat_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale);
  return aldm_launch_status("adamw_flat");
}

// quads the flat kernels may take as 16-byte accesses (every buffer 16-byte aligned), and their grid-stride grid
static inline long long flat_nvec(long long n, std::initializer_list<const void*> bufs) {
  for (const void* b : bufs)
    if (reinterpret_cast<uintptr_t>(b) & 15) return 0;
  return n / 4;
}
static inline unsigned flat_grid(long long n, long long nvec) {
  const long long work = nvec > n - 4 * nvec ? nvec : n - 4 * nvec;
  const long long b = (work + FLAT_THREADS - 1) / FLAT_THREADS;
  return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

extern "C" int aldm_sumsq_flat(const float* g, long long n, float* partials, int npart, void* stream) {
  ALDM_CHECK_ARG(g && partials && n > 0 && npart >= 1 && npart <= FLAT_MAX_PARTS, "sumsq_flat: bad args (1 <= npart <= %d)", FLAT_MAX_PARTS);
  hipLaunchKernelGGL(sumsq_flat_kernel, dim3(npart), dim3(FLAT_THREADS), 0, (hipStream_t)stream, g, n, flat_nvec(n, {g}), partials);
  return aldm_launch_status("sumsq_flat");
}

extern "C" int aldm_adamw_flat_clip(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                                    float eps, float weight_decay, int step, float grad_scale, const float* partials, int npart,
                                    float max_norm, float* norm_out, void* stream) {
  ALDM_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "adamw_flat_clip: bad args");
  ALDM_CHECK_ARG(partials && norm_out && npart >= 1 && npart <= FLAT_MAX_PARTS, "adamw_flat_clip: bad partials (1 <= npart <= %d)", FLAT_MAX_PARTS);
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
  const long long nvec = flat_nvec(n, {p, g, m, v});
  hipLaunchKernelGGL(adamw_flat_clip_kernel, dim3(flat_grid(n, nvec)), dim3(FLAT_THREADS), 0, (hipStream_t)stream, p, g, m, v, n, nvec, lr,
                     beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, partials, npart, max_norm, norm_out);
  return aldm_launch_status("adamw_flat_clip");
}

extern "C" int aldm_clip_flat(float* g, long long n, const float* partials, int npart, float max_norm, float grad_scale, float* norm_out,
                              void* stream) {
  ALDM_CHECK_ARG(g && n > 0 && partials && norm_out && npart >= 1 && npart <= FLAT_MAX_PARTS, "clip_flat: bad args (1 <= npart <= %d)", FLAT_MAX_PARTS);
  const long long nvec = flat_nvec(n, {g});
  hipLaunchKernelGGL(clip_flat_kernel, dim3(flat_grid(n, nvec)), dim3(FLAT_THREADS), 0, (hipStream_t)stream, g, n, nvec, partials, npart,
                     max_norm, grad_scale, norm_out);
  return aldm_launch_status("clip_flat");
}

extern "C" int aldm_accum_flat(float* acc, const float* g, long long n, int first, void* stream) {
  ALDM_CHECK_ARG(acc && g && n > 0, "accum_flat: bad args");
  const long long nvec = flat_nvec(n, {acc, g});
  hipLaunchKernelGGL(accum_flat_kernel, dim3(flat_grid(n, nvec)), dim3(FLAT_THREADS), 0, (hipStream_t)stream, acc, g, n, nvec, first);
  return aldm_launch_status("accum_flat");
}

// ---- debugging hook (tools/probe_latency.py), not part of the drop-in boundary: what does a kernel's FIRST memory access cost? ----
// One wave: stamp, dependent loads from up to four addresses (each waited for), stamp after each.  out[0..4] = s_memtime values.
__global__ void latency_probe_kernel(const int* a, const int* b, const int* c, const int* d, unsigned long long* out, int* sink) {
  unsigned long long t0, t1, t2, t3, t4;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
  int va = __builtin_nontemporal_load(a + threadIdx.x);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1) : "v"(va) : "memory");
  int vb = __builtin_nontemporal_load(b + threadIdx.x);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t2) : "v"(vb) : "memory");
  int vc = __builtin_nontemporal_load(c + threadIdx.x);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t3) : "v"(vc) : "memory");
  int vd = __builtin_nontemporal_load(d + threadIdx.x);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t4) : "v"(vd) : "memory");
  if (threadIdx.x == 0) { out[0] = t0; out[1] = t1; out[2] = t2; out[3] = t3; out[4] = t4; }
  if (va + vb + vc + vd == 0x7fffffff) sink[0] = 1;
}
extern "C" int aldm_probe_latency(const void* a, const void* b, const void* c, const void* d, void* out, void* sink, void* stream) {
  hipLaunchKernelGGL(latency_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int*)a, (const int*)b, (const int*)c, (const int*)d,
                     (unsigned long long*)out, (int*)sink);
  return aldm_launch_status("latency_probe");
}
