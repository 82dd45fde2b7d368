// ITU-R BS.1770-4 integrated loudness (mono, channel weight 1) and loudness normalisation on gfx950.
//
// aldm_kweight_energy: the K-weighted signal's energy per 100 ms hop, e[b][j] = sum of y^2 over [j H, (j + 1) H), float64, for the
// complete hops inside lens[b]; the filtered signal y is never stored.  K-weighting is two biquads in cascade (a shelf and a high-pass,
// loudness.k_weighting), each in the transposed direct form II that scipy.signal.lfilter runs:
//     y1 = b0 x + s1,   s1 = b1 x - a1 y1 + s2,   s2 = b2 x - a2 y1          coef = {b0, b1, b2, a1, a2, c0, c1, c2, d1, d2}
//     y2 = c0 y1 + t1,  t1 = c1 y1 - d1 y2 + t2,  t2 = c2 y1 - d2 y2         state = (s1, s2, t1, t2), zero at sample 0
// A fourth-order recurrence over up to millions of samples is cut into chunks of LD_CHUNK samples; the state is linear in (state, x):
//   1. ld_chunk_state   one lane per chunk that has a successor: the chunk from a ZERO state, keeping its end state z_c.
//   2. ld_state_scan    one wave per clip: S_0 = 0, S_{c+1} = M S_c + z_c with M = A^LD_CHUNK the cascade's 4x4 state transition over one
//                       chunk (host, exact, handed over as double-double).  64 chunks at a time, as an inclusive Hillis-Steele scan
//                       over the lanes with the table mpow[k] = M^(2^k), k = 0 .. 5; the carry S of the group enters lane 0 as M S.
//                       The last chunk of a clip has no successor, so no power for a shorter length is needed.
//   3. ld_chunk_energy  one lane per chunk: the chunk again from its true state S_c, y2^2 summed into the (at most LD_SLOTS = 3) hops the
//                       chunk meets: part[b][c][slot].
//   4. ld_hop_sum       one lane per hop: the parts of the chunks that meet it, in chunk order.  Hops past the clip's complete ones are 0.
// State and sums are float64: an fp32 recurrence is off by 4e-4 relative per hop on a DC offset with a small tone (the high-pass output
// is the small difference of large states); two float64 orderings of the same arithmetic agree to ~1e-12.  No atomics: a clip's
// energies depend on its samples and its length only, not on B or its row.  No wave runs more than LD_CHUNK dependent steps, the scan
// ceil(chunks / 64) * 6.
//
// aldm_loudness_gate: one workgroup per clip.  Block i = hops i .. i + 3 (400 ms, 75 % overlap), z_i = (e_i + .. + e_{i+3}) / (4 H),
// l_i = -0.691 + 10 log10 z_i; absolute gate l_i > -70; relative gate Gr = -0.691 + 10 log10(mean z over the absolutely gated) - 10;
// L = -0.691 + 10 log10(mean of z_i with l_i > -70 and l_i > Gr); -inf without a block above -70.  Two float64 reductions.
//
// aldm_peak_abs: max |x| over [0, ceil(lens[b] lens_up / lens_down)): the length of a resampled row from that of its source.  |x| >= 0,
// so its bits order like unsigned integers: the workgroups of a row meet in an integer atomic maximum, which does not depend on their
// order.
//
// aldm_loudness_gain: gain = 10^((target - L) / 20), capped at 10^(ceiling / 20) / peak when use_ceiling (rounded towards zero, so the
// product with the peak never passes the ceiling); L = -inf: gain 1.  y = gain x below lens[b], 0 from there on.
#include "common.h"

namespace {

constexpr int LD_CHUNK = 1024;
constexpr int LD_SLOTS = 3;              // hops a chunk can meet: needs H >= LD_CHUNK / 2
constexpr int LD_MIN_HOP = 800;          // fs >= 8000
constexpr int LD_LEVELS = 6;             // mpow[k] = M^(2^k), k = 0 .. 5

struct KCoef {
  double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2;
};
__device__ __forceinline__ KCoef ld_coef(const double* __restrict__ coef) {
  return KCoef{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], coef[8], coef[9]};
}
struct KState {
  double s1, s2, t1, t2;
};
// one sample through the cascade; returns y2
__device__ __forceinline__ double ld_step(const KCoef& k, KState& s, float xf) {
  const double x = (double)xf;
  const double y1 = k.b0 * x + s.s1;
  s.s1 = (k.b1 * x + s.s2) - k.a1 * y1;
  s.s2 = k.b2 * x - k.a2 * y1;
  const double y2 = k.c0 * y1 + s.t1;
  s.t1 = (k.c1 * y1 + s.t2) - k.d1 * y2;
  s.t2 = k.c2 * y1 - k.d2 * y2;
  return y2;
}

// the samples that count: the complete hops inside the clip
__device__ __forceinline__ int ld_samples(const int* __restrict__ lens, int b, int T, int H) {
  int L = lens[b];
  L = L < 0 ? 0 : (L > T ? T : L);
  return L / H * H;
}

// grid (ceil(nc / 64), B), 64 threads: lane -> chunk c; z[b][c] = end state of chunk c from a zero state, for c + 1 < ceil(N / LD_CHUNK)
__global__ __launch_bounds__(64) void ld_chunk_state_kernel(const float* __restrict__ x, const int* __restrict__ lens, int T, int H,
                                                            const double* __restrict__ coef, int nc, double* __restrict__ z) {
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  const int N = ld_samples(lens, b, T, H);
  const int ncb = (N + LD_CHUNK - 1) / LD_CHUNK;
  if (c + 1 >= ncb) return;                                    // (covers c >= nc) a whole chunk below N: every read is inside the row
  const KCoef k = ld_coef(coef);
  const float* xc = x + (long long)b * T + (long long)c * LD_CHUNK;
  KState s{0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < LD_CHUNK; i += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = xc[i + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) ld_step(k, s, v[u]);
  }
  double* o = z + ((long long)b * nc + c) * 4;
  o[0] = s.s1;
  o[1] = s.s2;
  o[2] = s.t1;
  o[3] = s.t2;
}

// One row of M v with M = hi + lo (a double-double table) as a compensated dot product (Ogita, Rump, Oishi: Dot2): the products and the
// running sum keep their rounding errors, which are added back at the end -- the result is the exact sum rounded once, up to
// 2^-105 of sum |m v|.  Needed because M = A^chunk of the nearly double pole of the high-pass is far from normal: the terms of a row
// cancel by many orders of magnitude once a state decays (an impulse's tail), and a plain fp64 row keeps 1e-16 of the TERMS.
__device__ __forceinline__ double ld_row_dd(const double* __restrict__ hi, const double* __restrict__ lo, const double (&v)[4]) {
#pragma clang fp contract(off)
  double s = 0.0, c = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double p = hi[j] * v[j];
    const double pe = __builtin_fma(hi[j], v[j], -p);           // hi v = p + pe exactly
    const double t = s + p;
    const double bb = t - s;
    const double se = (s - (t - bb)) + (p - bb);                // s + p = t + se exactly
    s = t;
    c += (pe + se) + lo[j] * v[j];
  }
  return s + c;
}
// m: [2][16], the 4x4 matrix's leading doubles (row-major), then its trailing ones
__device__ __forceinline__ KState ld_matvec(const double* __restrict__ m, const KState& v) {
  const double a[4] = {v.s1, v.s2, v.t1, v.t2};
  KState r;
  r.s1 = ld_row_dd(m, m + 16, a);
  r.s2 = ld_row_dd(m + 4, m + 20, a);
  r.t1 = ld_row_dd(m + 8, m + 24, a);
  r.t2 = ld_row_dd(m + 12, m + 28, a);
  return r;
}

// grid (B), 64 threads: start[b][0] = 0, start[b][c + 1] = M start[b][c] + z[b][c]
__global__ __launch_bounds__(64) void ld_state_scan_kernel(const int* __restrict__ lens, int T, int H, const double* __restrict__ mpow,
                                                           int nc, const double* __restrict__ z, double* __restrict__ start) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int N = ld_samples(lens, b, T, H);
  const int nz = (N + LD_CHUNK - 1) / LD_CHUNK - 1;             // chunks with an end state
  const double* zb = z + (long long)b * nc * 4;
  double* sb = start + (long long)b * nc * 4;
  if (lane < 4 && N > 0) sb[lane] = 0.0;
  KState carry{0.0, 0.0, 0.0, 0.0};
  for (int g = 0; g * 64 < nz; ++g) {                           // (uniform)
    const int c = g * 64 + lane;
    KState v{0.0, 0.0, 0.0, 0.0};
    if (c < nz) v = KState{zb[c * 4LL], zb[c * 4LL + 1], zb[c * 4LL + 2], zb[c * 4LL + 3]};
    if (lane == 0) {
      const KState m = ld_matvec(mpow, carry);
      v = KState{m.s1 + v.s1, m.s2 + v.s2, m.t1 + v.t1, m.t2 + v.t2};
    }
#pragma unroll
    for (int lv = 0; lv < LD_LEVELS; ++lv) {
      const int d = 1 << lv;
      KState u;
      u.s1 = __shfl_up(v.s1, d, 64);
      u.s2 = __shfl_up(v.s2, d, 64);
      u.t1 = __shfl_up(v.t1, d, 64);
      u.t2 = __shfl_up(v.t2, d, 64);
      const KState m = ld_matvec(mpow + lv * 32, u);
      if (lane >= d) v = KState{m.s1 + v.s1, m.s2 + v.s2, m.t1 + v.t1, m.t2 + v.t2};
    }
    if (c < nz) {                                               // c + 1 <= nz < nc
      double* o = sb + (c + 1) * 4LL;
      o[0] = v.s1;
      o[1] = v.s2;
      o[2] = v.t1;
      o[3] = v.t2;
    }
    carry.s1 = __shfl(v.s1, 63, 64);
    carry.s2 = __shfl(v.s2, 63, 64);
    carry.t1 = __shfl(v.t1, 63, 64);
    carry.t2 = __shfl(v.t2, 63, 64);
  }
}

// grid (ceil(nc / 64), B), 64 threads: lane -> chunk c < ceil(N / LD_CHUNK); part[b][c][slot] = energy of the chunk's samples in hop
// (c LD_CHUNK) div H + slot
__global__ __launch_bounds__(64) void ld_chunk_energy_kernel(const float* __restrict__ x, const int* __restrict__ lens, int T, int H,
                                                             const double* __restrict__ coef, int nc, const double* __restrict__ start,
                                                             double* __restrict__ part) {
  const int b = blockIdx.y, c = blockIdx.x * 64 + threadIdx.x;
  const int N = ld_samples(lens, b, T, H);
  const int ncb = (N + LD_CHUNK - 1) / LD_CHUNK;
  if (c >= ncb) return;
  const KCoef k = ld_coef(coef);
  const long long c0 = (long long)c * LD_CHUNK;
  const int n = N - c0 < LD_CHUNK ? (int)(N - c0) : LD_CHUNK;  // c0 + n <= N <= T
  const long long bound = (c0 / H + 1) * H - c0;                // first hop edge behind the chunk's first sample: in (0, H]
  const int e1 = bound < n ? (int)bound : n;                    // slot 0 = [0, e1), slot 1 = [e1, e2), slot 2 = [e2, n)
  const int e2 = bound + H < n ? (int)(bound + H) : n;
  const float* xc = x + (long long)b * T + c0;
  const double* sp = start + ((long long)b * nc + c) * 4;
  KState s{sp[0], sp[1], sp[2], sp[3]};
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = xc[i + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double y = ld_step(k, s, v[u]);
      const double q = y * y;
      const int t = i + u;
      p0 += t < e1 ? q : 0.0;
      p1 += (t >= e1 && t < e2) ? q : 0.0;
      p2 += t >= e2 ? q : 0.0;
    }
  }
  for (; i < n; ++i) {
    const double y = ld_step(k, s, xc[i]);
    const double q = y * y;
    p0 += i < e1 ? q : 0.0;
    p1 += (i >= e1 && i < e2) ? q : 0.0;
    p2 += i >= e2 ? q : 0.0;
  }
  double* o = part + ((long long)b * nc + c) * LD_SLOTS;
  o[0] = p0;
  o[1] = p1;
  o[2] = p2;
}

// grid (ceil(n_hops / 256), B), 256 threads: lane -> hop j < n_hops = T div H
__global__ __launch_bounds__(256) void ld_hop_sum_kernel(const int* __restrict__ lens, int T, int H, int nc, const double* __restrict__ part,
                                                         double* __restrict__ e, int n_hops) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_hops) return;
  const int N = ld_samples(lens, b, T, H);
  double sum = 0.0;
  const long long lo = (long long)j * H;
  if (lo + H <= N) {
    const int c_lo = (int)(lo / LD_CHUNK), c_hi = (int)((lo + H - 1) / LD_CHUNK);
    const double* pb = part + (long long)b * nc * LD_SLOTS;
    for (int c = c_lo; c <= c_hi; ++c) {
      const int slot = j - (int)((long long)c * LD_CHUNK / H);  // 0 .. LD_SLOTS - 1: the chunk meets hop j
      sum += pb[(long long)c * LD_SLOTS + slot];
    }
  }
  e[(long long)b * n_hops + j] = sum;
}

__device__ __forceinline__ double ld_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the 256 threads, the same value in every thread (lds: 4 doubles)
__device__ __forceinline__ double ld_block_sum(double v, double* lds) {
  v = ld_wave_sum(v);
  __syncthreads();                                              // (the previous reduction's readers are done)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__device__ __forceinline__ double ld_lufs(double z) { return -0.691 + 10.0 * log10(z); }

// grid (B), 256 threads
__global__ __launch_bounds__(256) void ld_gate_kernel(const double* __restrict__ e, const int* __restrict__ lens, int T, int H, int n_hops,
                                                      double* __restrict__ out) {
  __shared__ double lds[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  int L = lens[b];
  L = L < 0 ? 0 : (L > T ? T : L);
  int nh = L / H;
  nh = nh > n_hops ? n_hops : nh;
  const int nb = nh - 3;                                        // blocks
  const double* eb = e + (long long)b * n_hops;
  const double inv = 1.0 / (4.0 * (double)H);
  double sum = 0.0, cnt = 0.0;
  for (int i = tid; i < nb; i += 256) {
    const double z = (((eb[i] + eb[i + 1]) + eb[i + 2]) + eb[i + 3]) * inv;
    if (ld_lufs(z) > -70.0) {
      sum += z;
      cnt += 1.0;
    }
  }
  sum = ld_block_sum(sum, lds);
  cnt = ld_block_sum(cnt, lds);
  if (!(cnt > 0.0)) {                                           // (uniform) no block, or none above the absolute gate
    if (tid == 0) out[b] = -INFINITY;
    return;
  }
  const double gr = ld_lufs(sum / cnt) - 10.0;
  sum = 0.0;
  cnt = 0.0;
  for (int i = tid; i < nb; i += 256) {
    const double z = (((eb[i] + eb[i + 1]) + eb[i + 2]) + eb[i + 3]) * inv;
    const double l = ld_lufs(z);
    if (l > -70.0 && l > gr) {
      sum += z;
      cnt += 1.0;
    }
  }
  sum = ld_block_sum(sum, lds);
  cnt = ld_block_sum(cnt, lds);
  if (tid == 0) out[b] = cnt > 0.0 ? ld_lufs(sum / cnt) : -INFINITY;
}

__global__ void ld_peak_init_kernel(unsigned* __restrict__ peak, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) peak[b] = 0u;
}

// grid (ceil(T / PEAK_SPAN), B), 256 threads: each workgroup PEAK_SPAN consecutive samples
constexpr int PEAK_SPAN = 8192;
__global__ __launch_bounds__(256) void ld_peak_kernel(const float* __restrict__ x, const int* __restrict__ lens, int T, int up, int down,
                                                      unsigned* __restrict__ peak) {
  __shared__ float s_max[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  long long L = lens[b];
  L = L < 0 ? 0 : (L * up + down - 1) / down;                  // the out_lens of a resampled row from the lens of its source
  L = L > T ? T : L;
  const long long lo = (long long)blockIdx.x * PEAK_SPAN;
  if (lo >= L) return;                                          // (uniform)
  const long long hi = lo + PEAK_SPAN < L ? lo + PEAK_SPAN : L;
  const float* xb = x + (long long)b * T;
  float m = 0.f;
#pragma unroll 4
  for (long long i = lo + tid; i < hi; i += 256) m = fmaxf(m, fabsf(xb[i]));
  m = wave_max(m);
  if ((tid & 63) == 0) s_max[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    atomicMax(peak + b, __float_as_uint(m));                    // m >= 0: the bits order like the values
  }
}

// grid (ceil(T / 1024), B), 256 threads, four samples each
__global__ __launch_bounds__(256) void ld_gain_kernel(const float* __restrict__ x, const int* __restrict__ lens, int T,
                                                      const double* __restrict__ lufs, const float* __restrict__ peak, double target,
                                                      double ceiling, int use_ceiling, float* __restrict__ gain,
                                                      double* __restrict__ gain_db, float* __restrict__ y) {
  const int b = blockIdx.y;
  int L = lens[b];
  L = L < 0 ? 0 : (L > T ? T : L);
  const double l = lufs[b];
  float g = 1.f;
  if (l > -INFINITY && l < INFINITY) {                          // (uniform; NaN fails both)
    double gd = pow(10.0, (target - l) / 20.0);
    if (use_ceiling) {
      const double p = (double)peak[b];
      const double cap = pow(10.0, ceiling / 20.0) / p;
      if (p > 0.0 && cap < gd) gd = cap;
    }
    g = __double2float_rz(gd);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    gain[b] = g;
    gain_db[b] = 20.0 * log10((double)g);
  }
  const float* xb = x + (long long)b * T;
  float* yb = y + (long long)b * T;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = blockIdx.x * 1024 + k * 256 + threadIdx.x;
    if (i < T) yb[i] = i < L ? g * xb[i] : 0.f;
  }
}

bool ld_dims_ok(int B, int T, int H) { return B > 0 && B <= 65535 && T > 0 && T <= 0x7fffffff - LD_CHUNK && H >= LD_MIN_HOP; }

}  // namespace

extern "C" int aldm_loudness_chunk(void) { return LD_CHUNK; }

extern "C" long long aldm_kweight_energy_workspace_doubles(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  return (long long)B * cdivll(T, LD_CHUNK) * (4 + 4 + LD_SLOTS);
}

extern "C" int aldm_kweight_energy(const float* x, const int* lens, int B, int T, int hop, const double* coef, const double* mpow,
                                   int chunk, double* workspace, double* energy, void* stream) {
  ALDM_CHECK_ARG(x && lens && coef && mpow && workspace && (energy || (hop > 0 && T / hop == 0)), "kweight_energy: null pointer");
  ALDM_CHECK_ARG(ld_dims_ok(B, T, hop), "kweight_energy: bad dims (B %d, T %d, hop %d; hop >= %d)", B, T, hop, LD_MIN_HOP);
  ALDM_CHECK_ARG(chunk == LD_CHUNK, "kweight_energy: the power table is for chunks of %d samples, the kernels cut %d", chunk, LD_CHUNK);
  const int n_hops = T / hop;
  if (n_hops == 0) return ALDM_OK;                              // energy is [B][0]
  hipStream_t st = (hipStream_t)stream;
  const int nc = (int)cdivll(T, LD_CHUNK);
  double* z = workspace;
  double* start = z + (long long)B * nc * 4;
  double* part = start + (long long)B * nc * 4;
  const dim3 grid((unsigned)cdiv(nc, 64), (unsigned)B);
  hipLaunchKernelGGL(ld_chunk_state_kernel, grid, dim3(64), 0, st, x, lens, T, hop, coef, nc, z);
  int rc = aldm_launch_status("kweight_energy (chunk state)");
  if (rc != ALDM_OK) return rc;
  hipLaunchKernelGGL(ld_state_scan_kernel, dim3((unsigned)B), dim3(64), 0, st, lens, T, hop, mpow, nc, z, start);
  rc = aldm_launch_status("kweight_energy (state scan)");
  if (rc != ALDM_OK) return rc;
  hipLaunchKernelGGL(ld_chunk_energy_kernel, grid, dim3(64), 0, st, x, lens, T, hop, coef, nc, start, part);
  rc = aldm_launch_status("kweight_energy (chunk energy)");
  if (rc != ALDM_OK) return rc;
  hipLaunchKernelGGL(ld_hop_sum_kernel, dim3((unsigned)cdiv(n_hops, 256), (unsigned)B), dim3(256), 0, st, lens, T, hop, nc, part, energy,
                     n_hops);
  return aldm_launch_status("kweight_energy (hop sum)");
}

extern "C" int aldm_loudness_gate(const double* energy, const int* lens, int B, int T, int hop, double* lufs, void* stream) {
  ALDM_CHECK_ARG((energy || (hop > 0 && T / hop == 0)) && lens && lufs, "loudness_gate: null pointer");
  ALDM_CHECK_ARG(ld_dims_ok(B, T, hop), "loudness_gate: bad dims (B %d, T %d, hop %d; hop >= %d)", B, T, hop, LD_MIN_HOP);
  hipLaunchKernelGGL(ld_gate_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, energy, lens, T, hop, T / hop, lufs);
  return aldm_launch_status("loudness_gate");
}

extern "C" int aldm_peak_abs(const float* x, const int* lens, int B, int T, int lens_up, int lens_down, float* peak, void* stream) {
  ALDM_CHECK_ARG(x && lens && peak, "peak_abs: null pointer");
  ALDM_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && lens_up > 0 && lens_down > 0, "peak_abs: bad dims (B %d, T %d, lens %d : %d)", B, T,
                 lens_up, lens_down);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ld_peak_init_kernel, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, st, (unsigned*)peak, B);
  int rc = aldm_launch_status("peak_abs (init)");
  if (rc != ALDM_OK) return rc;
  hipLaunchKernelGGL(ld_peak_kernel, dim3((unsigned)cdiv(T, PEAK_SPAN), (unsigned)B), dim3(256), 0, st, x, lens, T, lens_up,
                     lens_down, (unsigned*)peak);
  return aldm_launch_status("peak_abs");
}

extern "C" int aldm_loudness_gain(const float* x, const int* lens, int B, int T, const double* lufs, const float* peak, double target_lufs,
                                  double ceiling_dbfs, int use_ceiling, float* gain, double* gain_db, float* y, void* stream) {
  ALDM_CHECK_ARG(x && lens && lufs && gain && gain_db && y && (peak || !use_ceiling), "loudness_gain: null pointer");
  ALDM_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && T <= 0x7fffffff - 1024, "loudness_gain: bad dims (B %d, T %d)", B, T);
  ALDM_CHECK_ARG(target_lufs == target_lufs && target_lufs > -200.0 && target_lufs < 200.0 &&
                     (!use_ceiling || (ceiling_dbfs == ceiling_dbfs && ceiling_dbfs > -200.0 && ceiling_dbfs < 200.0)),
                 "loudness_gain: target %g LUFS / ceiling %g dBFS out of range", target_lufs, ceiling_dbfs);
  ALDM_CHECK_ARG(x != y, "loudness_gain: out of place only");
  hipLaunchKernelGGL(ld_gain_kernel, dim3((unsigned)cdiv(T, 1024), (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, lens, T, lufs, peak,
                     target_lufs, ceiling_dbfs, use_ceiling, gain, gain_db, y);
  return aldm_launch_status("loudness_gain");
}
