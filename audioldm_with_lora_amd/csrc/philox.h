// Counter-based device RNG: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
// constants) and the Box-Muller transform to standard normals.  Shared by aldm_randn (rng.hip) and the fused ancestral step
// (elementwise.hip), which must produce the same bits for the same state.
//
// Addressing (independent of the launch shape):  key = the 64-bit seed;  counter = (block_lo, block_hi, draw_lo, draw_hi) with
// block = element_index / 4 and draw the 64-bit ordinal of the tensor-sized draw within the stream.  Element e of draw d is lane
// e % 4 of block e / 4, so a one-element-per-thread kernel and a four-wide one read the same words.
// The state is four 32-bit words in DEVICE memory: {seed_lo, seed_hi, draw_lo, draw_hi}.
//
// Training-step stream contract (aldm_train_noise_fused, elementwise.hip).  A step that finds the ordinal at d uses FOUR draws and
// leaves the ordinal at d + 4 -- always four, whether or not the noise offset is on and whether the latents come from the VAE moments
// or ready-made, so streams stay aligned across option changes:
//   d      B raw words        t_b = __umulhi(word_b, T)                    the timestep of sample b, uniform on [0, T)
//   d + 1  B*C*H*W normals    e, the posterior noise of latent_dist.sample()   (element index = the flat NCHW index)
//   d + 2  B*C*H*W normals    n, the diffusion noise                           (the same indexing)
//   d + 3  B*C normals        o, the noise offset's per-(sample, channel) normal
// Element i of each draw is element i of aldm_philox_u32 / aldm_randn for the same state with the ordinal set to that draw.
//
// RePaint-step stream contract (aldm_repaint_step_fused[_windowed]_masked, elementwise.hip).  A step that finds the ordinal at d uses
// TWO draws and, with a ticket, its last workgroup leaves the ordinal at d + 2 -- always two, on rows without a jump and on the last
// row too, so streams stay aligned whatever the walk:
//   d      B*n normals        zk, the noise of the known part a x0 + s zk      (RePaint Algorithm 1, line 4)
//   d + 1  B*n normals        zj, the noise of the jump back up c1 xb + c2 zj  (line 10; not generated on rows with c2 == 0)
// Element i of the [B][n] latent -- the LONG latent [B][rows][wc] when windowed -- is element i of each draw, and the bits are
// aldm_randn's for the same state with the ordinal set to that draw.  With ticket == NULL the counter and the ordinal stay.
//
// Clip-segment stream contract (aldm_clip_segment, clip_prep.hip).  One LOGICAL batch of recordings that finds the ordinal at d uses
// ONE draw and leaves the ordinal at d + 1 -- always one, and always ten words per row, whether a row is shorter than the segment
// (no word is looked at) or its first candidate already holds a sound (the other nine stay unused), so streams stay aligned whatever
// the recordings hold:
//   d      10 * (rows of the logical batch) raw words     w = element ordinals[b] * 10 + c is candidate c = 0 .. 9 of row b:
//                                                          start_c = ((w >> 8) * (L - S)) >> 24 in 64-bit integers
// Element i is element i of aldm_philox_u32 for the same state.  A logical batch may be split over several calls (one per sampling
// rate), each with its rows' ordinals: they all read draw d, and only the last one passes advance != 0 -- a trailing one-thread
// launch, behind every reader in stream order, stores d + 1.
#pragma once
#include "common.h"

struct PhiloxState { uint32_t seed_lo, seed_hi, draw_lo, draw_hi; };

__device__ __forceinline__ PhiloxState philox_load(const uint32_t* __restrict__ state) {
  return PhiloxState{state[0], state[1], state[2], state[3]};
}

// {draw_lo, draw_hi} += 1 as one 64-bit ordinal: two ordinary global stores by the one thread that owns the advance
__device__ __forceinline__ void philox_store_next(uint32_t* state, const PhiloxState& s) {
  const uint32_t lo = s.draw_lo + 1u;
  state[2] = lo;
  state[3] = s.draw_hi + (lo == 0u ? 1u : 0u);
}

// the state `k` draws further on: {draw_lo, draw_hi} + k as one 64-bit ordinal
__device__ __forceinline__ PhiloxState philox_at(const PhiloxState& s, uint32_t k) {
  const uint32_t lo = s.draw_lo + k;
  return PhiloxState{s.seed_lo, s.seed_hi, lo, s.draw_hi + (lo < k ? 1u : 0u)};
}

// stores the ordinal of `s` (philox_at of what was loaded): two ordinary global stores by the one thread that owns the advance
__device__ __forceinline__ void philox_store_ordinal(uint32_t* state, const PhiloxState& s) {
  state[2] = s.draw_lo;
  state[3] = s.draw_hi;
}

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += W0;
    k1 += W1;
  }
}

// the four raw words of `block` of the state's current draw
__device__ __forceinline__ void philox_block(const PhiloxState& s, unsigned long long block, uint32_t w[4]) {
  w[0] = (uint32_t)block;
  w[1] = (uint32_t)(block >> 32);
  w[2] = s.draw_lo;
  w[3] = s.draw_hi;
  philox4x32_10(w, s.seed_lo, s.seed_hi);
}

// Box-Muller on one word pair, everything in fp32 with the precise library functions:
//   u = w0 2^-32 + 2^-33 in (0, 1]   (the product is exact, so the sum rounds once; u may round to 1, then r = 0)
//   v = w1 (2 pi 2^-32) in [0, 2 pi] ;  r = sqrt(-2 ln u) ;  (r cos v, r sin v)
__device__ __forceinline__ void box_muller(uint32_t w0, uint32_t w1, float& z0, float& z1) {
  const float u = fmaf((float)w0, 0x1p-32f, 0x1p-33f);
  const float v = (float)w1 * (6.28318530717958647692f * 0x1p-32f);
  const float r = sqrtf(-2.f * logf(u));
  z0 = r * cosf(v);
  z1 = r * sinf(v);
}

// the four standard normals of `block` of the state's current draw: lanes 0/1 from (w0, w1), lanes 2/3 from (w2, w3)
__device__ __forceinline__ f32x4 philox_normal4(const PhiloxState& s, unsigned long long block) {
  uint32_t w[4];
  philox_block(s, block, w);
  f32x4 z;
  float a, b;
  box_muller(w[0], w[1], a, b);
  z[0] = a; z[1] = b;
  box_muller(w[2], w[3], a, b);
  z[2] = a; z[3] = b;
  return z;
}

// one element of the current draw: its whole block, then its lane -- the bits a four-wide reader of the same block sees
__device__ __forceinline__ uint32_t philox_word1(const PhiloxState& s, unsigned long long e) {
  uint32_t w[4];
  philox_block(s, e >> 2, w);
  const int lane = (int)(e & 3);
  return lane == 0 ? w[0] : lane == 1 ? w[1] : lane == 2 ? w[2] : w[3];
}

__device__ __forceinline__ float philox_normal1(const PhiloxState& s, unsigned long long e) {
  const f32x4 z = philox_normal4(s, e >> 2);
  const int lane = (int)(e & 3);
  return lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3];
}
