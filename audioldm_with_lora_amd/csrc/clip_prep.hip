// Clip front end of the training data path (gfx950): from resident recordings to the padded, normalised 16 kHz clip the log-mel kernel
// reads -- the dataset's read_hf_audio [REF script/data/datasets.py:174-195,494-522] around the resampler (resample.hip).
//
// aldm_clip_segment: a random, non-silent window of S samples per recording.  For a row of L samples, L <= S: the whole row, start 0.
// Otherwise R = L - S and candidate c = 0 .. 9 starts at
//     start_c = ((w_c >> 8) * R) >> 24        (64-bit integers: int(R * u) with torch's 24-bit uniform u = (w >> 8) 2^-24)
// with w_c element ordinals[b] * 10 + c of the state's current draw (philox.h).  The row takes the first candidate whose window holds a
// sample with |x| > 1e-4f (strictly), the tenth when none does.  The result of a row depends on its ordinal and its samples only: not
// on B, on its place in the batch or on the launch order; no atomics.
//   1. clip_chunk_max   max |x| of every whole or partial chunk of CLIP_CHUNK samples of the rows with L > S (one wave per chunk).  A
//                       recording can be minutes long: ten windows read sample by sample would be ten passes over up to S samples each.
//   2. clip_pick_start  one workgroup per row: a candidate's window is its ragged left edge, whole chunks, its ragged right edge.
//   3. clip_gather      seg[b][i] = x[start + i] for start + i < L, else 0.
//   4. (advance)        one thread moves the draw ordinal by one, behind every reader in stream order.
//
// aldm_clip_normalize: over the first m = min(n[b], target) samples, mean removal and peak normalisation to 0.5, zeros from m on.
//   1. clip_row_stats   P workgroups per row, each over one slice: {sum, max, min} with the sum in float64 (a 163 840-sample fp32 sum
//                       loses the low bits a DC offset needs; float64 holds 2^29 fp32 addends exactly to fp32's eyes).
//   2. clip_apply       every thread adds the P partials in index order (the same value in every workgroup), mean = sum / m in float64,
//                       peak = max(max - mean, mean - min) = max |y - mean|, out = fp32(y - mean) / (peak + 1e-8f) * 0.5f with IEEE
//                       division.  A constant row has mean == y exactly, so it gives exact zeros.
#include "philox.h"

namespace {

constexpr int CLIP_CHUNK = 1024;          // samples per chunk maximum
constexpr int CLIP_CANDIDATES = 10;
constexpr float CLIP_SILENCE = 1e-4f;
constexpr int NORM_MAX_PARTS = 64;

// the row's usable length: lens[b] cut to [0, max_len] and to what the pool holds behind offsets[b] (a bad row reads nothing)
__device__ __forceinline__ int clip_row(const long long* __restrict__ offsets, const int* __restrict__ lens, int b, int max_len,
                                        long long pool_len, long long& off) {
  off = offsets[b];
  int L = lens[b];
  L = L < 0 ? 0 : (L > max_len ? max_len : L);
  if (off < 0 || off > pool_len) {
    off = 0;
    return 0;
  }
  const long long room = pool_len - off;
  return (long long)L > room ? (int)room : L;
}

// grid (ceil(n_chunks / 4), B), 256 threads: wave w of workgroup g owns chunk 4 g + w of row b
__global__ __launch_bounds__(256) void clip_chunk_max_kernel(const float* __restrict__ x, const long long* __restrict__ offsets,
                                                             const int* __restrict__ lens, int S, int max_len, long long pool_len,
                                                             float* __restrict__ cmax, int n_chunks) {
  const int b = blockIdx.y;
  long long off;
  const int L = clip_row(offsets, lens, b, max_len, pool_len, off);
  if (L <= S) return;                                          // (uniform) the whole row is the segment: nothing to choose
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (chunk >= n_chunks) return;
  const long long c0 = (long long)chunk * CLIP_CHUNK;
  if (c0 >= L) return;
  const float* xb = x + off + c0;
  const int n = (long long)L - c0 < CLIP_CHUNK ? (int)(L - c0) : CLIP_CHUNK;
  float m = 0.f;
#pragma unroll 4
  for (int i = lane; i < n; i += 64) m = fmaxf(m, fabsf(xb[i]));
  m = wave_max(m);
  if (lane == 0) cmax[(long long)b * n_chunks + chunk] = m;
}

// grid (B), 256 threads
__global__ __launch_bounds__(256) void clip_pick_start_kernel(const float* __restrict__ x, const long long* __restrict__ offsets,
                                                              const int* __restrict__ lens, const int* __restrict__ ordinals, int S,
                                                              int max_len, long long pool_len, const uint32_t* __restrict__ state,
                                                              const float* __restrict__ cmax, int n_chunks, int* __restrict__ start) {
  __shared__ uint32_t words[CLIP_CANDIDATES];
  const int b = blockIdx.x, tid = threadIdx.x;
  long long off;
  const int L = clip_row(offsets, lens, b, max_len, pool_len, off);
  if (L <= S) {
    if (tid == 0) start[b] = 0;
    return;
  }
  if (tid < CLIP_CANDIDATES)
    words[tid] = philox_word1(philox_load(state), (unsigned long long)(unsigned)ordinals[b] * CLIP_CANDIDATES + (unsigned)tid);
  __syncthreads();
  const float* xb = x + off;
  const float* cm = cmax + (long long)b * n_chunks;
  const unsigned long long R = (unsigned long long)(L - S);
  int s = 0;
  for (int c = 0; c < CLIP_CANDIDATES; ++c) {
    s = (int)(((unsigned long long)(words[c] >> 8) * R) >> 24);                 // < R: s + S < L
    const long long end = (long long)s + S;                                       // window [s, end)
    long long k0 = ((long long)s + CLIP_CHUNK - 1) / CLIP_CHUNK;                  // whole chunks k0 .. k1 - 1
    long long k1 = end / CLIP_CHUNK;
    int hit = 0;
    if (k1 <= k0) {                                                               // no whole chunk inside: sample by sample
      for (long long i = s + tid; i < end; i += 256) hit |= fabsf(xb[i]) > CLIP_SILENCE;
    } else {
      for (long long i = s + tid; i < k0 * CLIP_CHUNK; i += 256) hit |= fabsf(xb[i]) > CLIP_SILENCE;
      for (long long k = k0 + tid; k < k1; k += 256) hit |= cm[k] > CLIP_SILENCE;
      for (long long i = k1 * CLIP_CHUNK + tid; i < end; i += 256) hit |= fabsf(xb[i]) > CLIP_SILENCE;
    }
    if (__syncthreads_or(hit)) break;                                             // (uniform)
  }
  if (tid == 0) start[b] = s;
}

// grid (ceil(S / 1024), B), 256 threads, four samples each
__global__ __launch_bounds__(256) void clip_gather_kernel(const float* __restrict__ x, const long long* __restrict__ offsets,
                                                          const int* __restrict__ lens, int S, int max_len, long long pool_len,
                                                          const int* __restrict__ start, float* __restrict__ seg) {
  const int b = blockIdx.y;
  long long off;
  const int L = clip_row(offsets, lens, b, max_len, pool_len, off);
  int s = start[b];
  s = (s < 0 || L <= S) ? 0 : s;
  const float* xb = x + off;
  float* sb = seg + (long long)b * S;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = blockIdx.x * 1024 + k * 256 + threadIdx.x;
    if (i < S) {
      const long long j = (long long)s + i;
      sb[i] = j < L ? xb[j] : 0.f;
    }
  }
}

__global__ void clip_advance_kernel(uint32_t* state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) philox_store_next(state, philox_load(state));
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ int norm_count(const int* __restrict__ n, int b, int T, int target) {
  int m = n[b];
  m = m > target ? target : m;
  m = m > T ? T : m;
  return m < 0 ? 0 : m;
}

// grid (P, B), 256 threads: workgroup p owns samples [p slice, (p + 1) slice) below m; part[b][p] = {sum, max, min}
__global__ __launch_bounds__(256) void clip_row_stats_kernel(const float* __restrict__ y, const int* __restrict__ n, int T, int target,
                                                             int slice, double* __restrict__ part) {
  __shared__ double s_sum[4];
  __shared__ float s_max[4], s_min[4];
  const int b = blockIdx.y, p = blockIdx.x, tid = threadIdx.x;
  const int m = norm_count(n, b, T, target);
  const long long lo = (long long)p * slice;
  const long long hi = lo + slice < m ? lo + slice : m;
  const float* yb = y + (long long)b * T;
  double sum = 0.0;
  float mx = -INFINITY, mn = INFINITY;
  for (long long i = lo + tid; i < hi; i += 256) {
    const float v = yb[i];
    sum += (double)v;
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
  }
  sum = wave_sum_f64(sum);
  mx = wave_max(mx);
  mn = wave_min(mn);
  if ((tid & 63) == 0) {
    s_sum[tid >> 6] = sum;
    s_max[tid >> 6] = mx;
    s_min[tid >> 6] = mn;
  }
  __syncthreads();
  if (tid == 0) {
    double* o = part + ((long long)b * gridDim.x + p) * 3;
    o[0] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    o[1] = (double)fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    o[2] = (double)fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));
  }
}

// grid (ceil(target / 1024), B), 256 threads, four samples each
__global__ __launch_bounds__(256) void clip_apply_kernel(const float* __restrict__ y, const int* __restrict__ n, int T, int target, int P,
                                                         const double* __restrict__ part, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int m = norm_count(n, b, T, target);
  double mean = 0.0;
  float denom = 1.f;
  if (m > 0) {                                                  // (uniform)
    const double* pb = part + (long long)b * P * 3;
    double sum = 0.0, mx = -INFINITY, mn = INFINITY;
    for (int p = 0; p < P; ++p) {                               // index order: the same bits in every workgroup
      sum += pb[p * 3];
      mx = fmax(mx, pb[p * 3 + 1]);
      mn = fmin(mn, pb[p * 3 + 2]);
    }
    mean = sum / (double)m;
    const float peak = (float)fmax(mx - mean, mean - mn);       // = max_i fp32(y_i - mean): rounding is monotone
    denom = peak + 1e-8f;
  }
  const float* yb = y + (long long)b * T;
  float* ob = out + (long long)b * target;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = blockIdx.x * 1024 + k * 256 + threadIdx.x;
    if (i < target) {
      float v = 0.f;
      if (i < m) v = (float)((double)yb[i] - mean) / denom * 0.5f;
      ob[i] = v;
    }
  }
}

}  // namespace

extern "C" long long aldm_clip_segment_workspace_floats(int B, int max_len) {
  if (B <= 0 || max_len <= 0) return 0;
  return (long long)B * cdivll(max_len, CLIP_CHUNK);
}

extern "C" int aldm_clip_segment(const float* x, long long pool_len, const long long* offsets, const int* lens, const int* ordinals, int B,
                                 int S, int max_len, unsigned* rng_state, int advance, float* workspace, float* seg, int* start,
                                 void* stream) {
  ALDM_CHECK_ARG(x && offsets && lens && ordinals && rng_state && workspace && seg && start, "clip_segment: null pointer");
  ALDM_CHECK_ARG(B > 0 && B <= 65535 && S > 0 && S <= 0x7fffffff - 1024 && max_len > 0 && pool_len > 0,
                 "clip_segment: bad dims (B %d, S %d, max_len %d, pool_len %lld)", B, S, max_len, pool_len);
  hipStream_t st = (hipStream_t)stream;
  const int n_chunks = (int)cdivll(max_len, CLIP_CHUNK);
  if (max_len > S) {
    hipLaunchKernelGGL(clip_chunk_max_kernel, dim3((unsigned)cdiv(n_chunks, 4), (unsigned)B), dim3(256), 0, st, x, offsets, lens, S,
                       max_len, pool_len, workspace, n_chunks);
    int rc = aldm_launch_status("clip_segment (chunk max)");
    if (rc != ALDM_OK) return rc;
  }
  hipLaunchKernelGGL(clip_pick_start_kernel, dim3((unsigned)B), dim3(256), 0, st, x, offsets, lens, ordinals, S, max_len, pool_len,
                     rng_state, workspace, n_chunks, start);
  int rc = aldm_launch_status("clip_segment (pick start)");
  if (rc != ALDM_OK) return rc;
  hipLaunchKernelGGL(clip_gather_kernel, dim3((unsigned)cdiv(S, 1024), (unsigned)B), dim3(256), 0, st, x, offsets, lens, S, max_len,
                     pool_len, start, seg);
  rc = aldm_launch_status("clip_segment (gather)");
  if (rc != ALDM_OK || !advance) return rc;
  hipLaunchKernelGGL(clip_advance_kernel, dim3(1), dim3(1), 0, st, rng_state);
  return aldm_launch_status("clip_segment (advance)");
}

extern "C" int aldm_clip_normalize_parts(int T, int target) {
  if (T <= 0 || target <= 0) return 0;
  const int span = T < target ? T : target;
  const int P = cdiv(span, 2048);
  return P > NORM_MAX_PARTS ? NORM_MAX_PARTS : P;
}

extern "C" int aldm_clip_normalize(const float* y, const int* n, int B, int T, int target, double* workspace, float* out, void* stream) {
  ALDM_CHECK_ARG(y && n && workspace && out, "clip_normalize: null pointer");
  ALDM_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && target > 0 && target <= 0x7fffffff - 1024,
                 "clip_normalize: bad dims (B %d, T %d, target %d)", B, T, target);
  hipStream_t st = (hipStream_t)stream;
  const int P = aldm_clip_normalize_parts(T, target);
  const int span = T < target ? T : target;
  const int slice = cdiv(span, P);
  hipLaunchKernelGGL(clip_row_stats_kernel, dim3((unsigned)P, (unsigned)B), dim3(256), 0, st, y, n, T, target, slice, workspace);
  int rc = aldm_launch_status("clip_normalize (stats)");
  if (rc != ALDM_OK) return rc;
  hipLaunchKernelGGL(clip_apply_kernel, dim3((unsigned)cdiv(target, 1024), (unsigned)B), dim3(256), 0, st, y, n, T, target, P, workspace,
                     out);
  return aldm_launch_status("clip_normalize (apply)");
}
