// On-device random numbers (gfx950): raw Philox4x32-10 words and fp32 standard normals from a counter-based stream whose state
// lives in device memory (philox.h), so a captured hipGraph draws fresh numbers on every replay with no host work.
#include "philox.h"

namespace {

// out[e] = lane e % 4 of block first_block + e / 4 (mod 2^64) of the state's current draw; one thread per block, the tail block
// stores its first n % 4 words
__global__ __launch_bounds__(256) void philox_u32_kernel(uint32_t* __restrict__ out, long long n, const uint32_t* __restrict__ state,
                                                         unsigned long long first_block) {
  const long long blk = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long e0 = blk * 4;
  if (e0 >= n) return;
  uint32_t w[4];
  philox_block(philox_load(state), first_block + (unsigned long long)blk, w);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (e0 + k < n) out[e0 + k] = w[k];
}

// VEC = 4: one thread per Philox block, one 16-byte store (n % 4 == 0, out 16-byte aligned).  VEC = 1: one thread per element, which
// evaluates its whole block through the same function and keeps its lane -- the same bits as the four-wide form.
template <int VEC>
__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, long long n, const uint32_t* __restrict__ state) {
  const long long tix = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long e = tix * VEC;
  if (e >= n) return;
  const f32x4 z = philox_normal4(philox_load(state), (unsigned long long)(e >> 2));
  if constexpr (VEC == 4) {
    *reinterpret_cast<f32x4*>(out + e) = z;
  } else {
    const int lane = (int)(e & 3);
    out[e] = lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3];
  }
}

// the follow-up launch of aldm_randn(advance): stream order puts it behind every read of the draw ordinal
__global__ void philox_advance_kernel(uint32_t* state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) philox_store_next(state, philox_load(state));
}

inline unsigned blocks_for(long long work, int per_block) { return (unsigned)((work + per_block - 1) / per_block); }

}  // namespace

extern "C" int aldm_philox_u32(unsigned* out, long long n, const unsigned* state, unsigned long long first_block, void* stream) {
  ALDM_CHECK_ARG(out && state && n > 0 && n < (1ll << 40), "philox_u32: bad args");
  hipLaunchKernelGGL(philox_u32_kernel, dim3(blocks_for((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, out, n, state, first_block);
  return aldm_launch_status("philox_u32");
}

extern "C" int aldm_randn(float* out, long long n, unsigned* state, int advance, void* stream) {
  ALDM_CHECK_ARG(out && state && n > 0 && n < (1ll << 40), "randn: bad args");
  if (n % 4 == 0 && ((uintptr_t)out & 15) == 0)
    hipLaunchKernelGGL(randn_kernel<4>, dim3(blocks_for(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, out, n, state);
  else
    hipLaunchKernelGGL(randn_kernel<1>, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, out, n, state);
  int rc = aldm_launch_status("randn");
  if (rc != ALDM_OK || !advance) return rc;
  hipLaunchKernelGGL(philox_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
  return aldm_launch_status("randn (advance)");
}
