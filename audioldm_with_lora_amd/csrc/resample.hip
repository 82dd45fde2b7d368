// Rational polyphase FIR resampler on gfx950: scipy.signal.resample_poly(x, up, down) with its default Kaiser(5.0) filter and zero
// padding, for recordings that are not at the vocoder's 16 kHz (44.1 / 48 kHz in, 44.1 / 48 kHz out).
//
// With h the filter of resample.resample_filter (2 half + 1 taps, half = 10 max(up, down)) cut into its `up` phases,
// table[p][k] = h[p + k up] (fp32 [up][K], zero behind the end of h), output n of a clip of L samples is
//     m = n down + half,  p = m mod up,  j1 = m div up
//     y[n] = sum_{k = 0 .. K-1} table[p][k] x[j1 - k]          (x[j] = 0 outside [0, L))
// (scipy's upfirdn with the pre-pad and pre-remove of resample_poly folded into `half`).  One thread owns one output and walks its
// phase row, contiguous in k, with fp32 fmaf in the order k = first .. last tap that meets a sample; a workgroup of 1024 threads owns
// 1024 consecutive outputs of one clip.  No atomics, nothing shared between clips: a clip's result does not depend on its row.
//
// Indices: n down passes 2^31 after five minutes of 44.1 kHz input, so the workgroup's first m is a 64-bit product, divided once
// (uniformly) into q0 = m0 div up and r0 = m0 mod up.  Inside the workgroup t = tid down + r0 < 1025 * 2048 stays in 32 bits:
// p = t mod up, j1 = q0 + t div up.
//
// Staging.  The outputs of a workgroup read the input span x[q0 - (K-1) .. q0 + (1023 down + up - 1) div up], 1023 down / up + K
// samples (2 876 at 44.1 -> 16 kHz), and -- up and down being coprime -- min(up, 1024) different phase rows: neighbouring lanes
// read rows that lie K floats apart, 64 cache lines per load when they come from global memory (measured: 99 us for 60 s of
// 44.1 -> 16 kHz with 256-thread workgroups, the input staged and the rows read from global memory, 17 us now).  Rule, by
// the bytes of LDS a workgroup would need, against RS_LDS_BYTES = 64 KB (two workgroups = all 32 waves of a CU):
//   span + table    fit: both are copied into LDS, coalesced, the table with its rows K | 1 floats apart (an odd stride: rows whose
//                        numbers differ mod 32 start on different banks); every pair of rates with max(up, down) <= 640 and
//                        down / up <= 12 -- all pairs among 8 / 16 / 22.05 / 32 / 44.1 / 48 kHz, and 96 / 192 kHz down to 16 kHz
//   span alone      fits (up > ~700: a table over 58 KB): the input is staged, the rows are read from global memory
//   neither         (down / up > 15: the span is up to 8 MB at 2048 : 1): both are read from global memory
// All three forms run the same sum in the same order, so a clip's samples do not depend on the form either.
#include "common.h"

namespace {

constexpr int RS_BLOCK = 1024;
constexpr int RS_LDS_BYTES = 65536;
constexpr int RS_MAX_RATIO = 2048;

// sum_{k = k0 .. k1} row[k] xr[-k], one fmaf per tap in that order.  Eight taps' loads are issued before their fmafs: left to the
// compiler the loop waits for both loads of every single tap, and eight waves per SIMD do not hide an LDS round trip per tap.
__device__ __forceinline__ float tap_sum(const float* __restrict__ row, const float* __restrict__ xr, int k0, int k1) {
  float acc = 0.f;
  int k = k0;
  for (; k + 7 <= k1; k += 8) {
    float a[8], v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      a[i] = row[k + i];
      v[i] = xr[-(k + i)];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = fmaf(a[i], v[i], acc);
  }
  for (; k <= k1; ++k) acc = fmaf(row[k], xr[-k], acc);
  return acc;
}

template <bool STAGE_X, bool STAGE_T>
__global__ __launch_bounds__(RS_BLOCK) void resample_poly_kernel(const float* __restrict__ x, const int* __restrict__ lens, int T_in,
                                                                 const float* __restrict__ table, int up, int down, int K, int half,
                                                                 int span, AldmDiv div_k, float* __restrict__ y, int T_out) {
  extern __shared__ float lds[];
  float* xs = lds;                                            // [span]
  float* ts = lds + span;                                     // [up][K | 1]
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n0 = blockIdx.x * RS_BLOCK;
  const int n = n0 + tid;
  int L = lens[b];
  L = L < 0 ? 0 : (L > T_in ? T_in : L);
  const long long out_len = ((long long)L * up + down - 1) / down;
  float* yb = y + (long long)b * T_out;
  if (n0 >= out_len) {                                        // (uniform) the whole run lies behind the clip
    if (n < T_out) yb[n] = 0.f;
    return;
  }
  const float* xb = x + (long long)b * T_in;
  const long long m0 = (long long)n0 * down + half;
  long long q0;
  if ((m0 >> 32) == 0) q0 = (unsigned)m0 / (unsigned)up;      // (uniform) the 64-bit division only where it is needed
  else q0 = m0 / up;
  const int r0 = (int)(m0 - q0 * up);
  const unsigned t = (unsigned)tid * (unsigned)down + (unsigned)r0;
  const int dj = (int)(t / (unsigned)up);
  const int p = (int)(t - (unsigned)dj * (unsigned)up);
  const int Kp = K | 1;
  if (STAGE_X) {
    const long long base = q0 - (K - 1);                      // sample index of xs[0]
    for (int i = tid; i < span; i += RS_BLOCK) {
      const long long j = base + i;
      xs[i] = (j >= 0 && j < L) ? xb[j] : 0.f;
    }
    if (STAGE_T) {
      const int n_el = up * K;
      for (int e = tid; e < n_el; e += RS_BLOCK) {
        const int r = aldm_div(e, div_k);
        ts[r * Kp + (e - r * K)] = table[e];
      }
    }
    __syncthreads();
  }
  if (n >= T_out) return;
  float acc = 0.f;
  if (n < out_len) {
    const long long j1 = q0 + dj;
    const long long lo = j1 - (L - 1);                        // taps k with 0 <= j1 - k <= L - 1
    const int k0 = lo > 0 ? (int)lo : 0;
    const int k1 = j1 < K - 1 ? (int)j1 : K - 1;
    const float* row = STAGE_T ? ts + p * Kp : table + (long long)p * K;
    const float* xr = STAGE_X ? xs + dj + (K - 1) : xb + j1;  // xr[-k] = x[j1 - k]
    acc = tap_sum(row, xr, k0, k1);
  }
  yb[n] = acc;
}

}  // namespace

extern "C" int aldm_resample_poly(const float* x, const int* lens, int B, int T_in, const float* table, int up, int down, int K,
                                  int half, float* y, int T_out, void* stream) {
  ALDM_CHECK_ARG(x && lens && table && y, "resample_poly: null pointer");
  ALDM_CHECK_ARG(B > 0 && B <= 65535 && T_in > 0 && T_out > 0 && T_out <= 0x7fffffff - RS_BLOCK && up > 0 && down > 0 && K > 0 && half > 0,
                 "resample_poly: bad dims (B %d, T_in %d, T_out %d, up %d, down %d, K %d, half %d)", B, T_in, T_out, up, down, K, half);
  const int big = up > down ? up : down;
  ALDM_CHECK_ARG(big <= RS_MAX_RATIO, "resample_poly: ratio %d : %d over the cap of %d", up, down, RS_MAX_RATIO);
  ALDM_CHECK_ARG(half == 10 * big && K == (2 * half + 1 + up - 1) / up,
                 "resample_poly: half %d / K %d do not match %d : %d (half = 10 max(up, down), K = ceil((2 half + 1) / up))", half, K,
                 up, down);
  ALDM_CHECK_ARG((long long)T_out == ((long long)T_in * up + down - 1) / down,
                 "resample_poly: T_out %d is not ceil(%d * %d / %d)", T_out, T_in, up, down);
  const long long span = ((long long)(RS_BLOCK - 1) * down + up - 1) / up + K;
  const long long tab = (long long)up * (K | 1);
  const AldmDiv div_k = aldm_make_div((unsigned)K);
  const dim3 grid((unsigned)cdiv(T_out, RS_BLOCK), (unsigned)B), block(RS_BLOCK);
  if ((span + tab) * 4 <= RS_LDS_BYTES)
    hipLaunchKernelGGL((resample_poly_kernel<true, true>), grid, block, (size_t)((span + tab) * 4), (hipStream_t)stream, x, lens, T_in,
                       table, up, down, K, half, (int)span, div_k, y, T_out);
  else if (span * 4 <= RS_LDS_BYTES)
    hipLaunchKernelGGL((resample_poly_kernel<true, false>), grid, block, (size_t)(span * 4), (hipStream_t)stream, x, lens, T_in, table, up,
                       down, K, half, (int)span, div_k, y, T_out);
  else
    hipLaunchKernelGGL((resample_poly_kernel<false, false>), grid, block, 0, (hipStream_t)stream, x, lens, T_in, table, up, down, K, half,
                       0, div_k, y, T_out);
  return aldm_launch_status("resample_poly");
}
