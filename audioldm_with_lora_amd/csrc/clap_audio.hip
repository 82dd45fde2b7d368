// CLAP audio tower (HTSAT-Swin, transformers' ClapAudioModelWithProjection) and its front end (ClapFeatureExtractor) on gfx950.
//
// What lives here is everything the existing GEMM / LayerNorm launches do not cover:
//   resample_up3        16 kHz -> 48 kHz, integer-3 polyphase FIR (the taps of scipy.signal.resample_poly(x, 3, 1))
//   clap_log_mel        repeatpad to max_len -> reflect pad n_fft/2 -> periodic Hann -> 1024-point LDS FFT -> |X|^2 -> mel bank
//                       -> 10 log10(max(., 1e-10))   (transformers.audio_utils.spectrogram(center=True, pad_mode="reflect"))
//   clap_input          eval BatchNorm over the mel bins + bicubic (align_corners=True) resize of the time axis to 1024 frames +
//                       reshape_mel2img, written straight into the im2col rows of the patch-embedding GEMMs
//   aff_sum_pool /      the non-GEMM parts of ClapAudioAFFBlock: a = global + local, its global average pool, and
//   aff_combine         2 h sigmoid(l + g) + 2 r (1 - sigmoid(l + g))
//   window_attention    Swin (shifted-)window attention over a token-major QKV buffer; roll / partition / reverse in the addressing
//   patch_merge_gather  the 2 x 2 neighbourhood of every output token as one 4C row, transformers' [x0, x1, x2, x3] order
//   token_mean          the head's average pool
// All arithmetic is fp32; activations are bf16 token-major rows, as everywhere in this library.
#include "common.h"

namespace {

constexpr int NFFT = 1024;
constexpr int NBINS = NFFT / 2 + 1;

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// ---- 16 kHz -> 48 kHz ---------------------------------------------------------------------------------------------------------
// y[n] = sum_j x[j] h[n + half - 3 j]  over 0 <= n + half - 3 j < ntaps  (scipy's upfirdn with its pre-pad / pre-remove folded in)
__global__ __launch_bounds__(256) void resample_up3_kernel(const float* __restrict__ x, const int* __restrict__ lens, int T_in,
                                                           const float* __restrict__ taps, int ntaps, float* __restrict__ y,
                                                           int T_out) {
  const int b = blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= T_out) return;
  const int L = lens[b];
  float acc = 0.f;
  if (n < 3 * L) {
    const int half = (ntaps - 1) / 2;
    const int m = n + half;                                   // tap index of sample j: m - 3 j
    int j0 = m - (ntaps - 1);
    j0 = j0 <= 0 ? 0 : (j0 + 2) / 3;
    int j1 = m / 3;
    if (j1 > L - 1) j1 = L - 1;
    const float* xb = x + (long long)b * T_in;
    for (int j = j0; j <= j1; ++j) acc = fmaf(xb[j], taps[m - 3 * j], acc);
  }
  y[(long long)b * T_out + n] = acc;
}

// ---- CLAP log-mel ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clap_log_mel_kernel(const float* __restrict__ wav, const int* __restrict__ lens, int T,
                                                           int max_len, int hop, int n_frames, const float* __restrict__ window,
                                                           const float* __restrict__ mel_basis, const int* __restrict__ mel_range,
                                                           int n_mels, float* __restrict__ out) {
  __shared__ float2 bufA[NFFT], bufB[NFFT], tw[768];
  __shared__ float pw[NBINS + 3];
  const int tid = threadIdx.x;
  const int frame = blockIdx.x, b = blockIdx.y;
  for (int k = tid; k < 768; k += 256) {
    float s, c;
    sincospif(-(float)k * (2.0f / NFFT), &s, &c);
    tw[k] = make_float2(c, s);
  }
  // repeatpad (np.tile(w, max_len // L), then zeros up to max_len) and the centre reflect padding, folded into the index
  const float* w = wav + (long long)b * T;
  const int L = lens[b];
  const int rep_end = (max_len / L) * L;
  for (int i = tid; i < NFFT; i += 256) {
    int src = frame * hop + i - NFFT / 2;
    src = src < 0 ? -src : src;
    src = src >= max_len ? 2 * (max_len - 1) - src : src;
    const float v = src < rep_end ? w[src % L] : 0.f;
    bufA[i] = make_float2(v * window[i], 0.f);
  }
  __syncthreads();
  float2* x = bufA;
  float2* y = bufB;
#pragma unroll
  for (int pass = 0; pass < 5; ++pass) {
    const int s = 1 << (2 * pass), n = NFFT >> (2 * pass), n1 = n >> 2;
    const int p = tid >> (2 * pass), q = tid & (s - 1);
    const float2 a = x[q + s * p], bb = x[q + s * (p + n1)], c = x[q + s * (p + 2 * n1)], d = x[q + s * (p + 3 * n1)];
    const float2 apc = make_float2(a.x + c.x, a.y + c.y), amc = make_float2(a.x - c.x, a.y - c.y);
    const float2 bpd = make_float2(bb.x + d.x, bb.y + d.y);
    const float2 jbmd = make_float2(-(bb.y - d.y), bb.x - d.x);
    const int k1 = p * s;
    y[q + s * (4 * p + 0)] = make_float2(apc.x + bpd.x, apc.y + bpd.y);
    y[q + s * (4 * p + 1)] = cmul(tw[k1], make_float2(amc.x - jbmd.x, amc.y - jbmd.y));
    y[q + s * (4 * p + 2)] = cmul(tw[2 * k1], make_float2(apc.x - bpd.x, apc.y - bpd.y));
    y[q + s * (4 * p + 3)] = cmul(tw[3 * k1], make_float2(amc.x + jbmd.x, amc.y + jbmd.y));
    __syncthreads();
    float2* t = x; x = y; y = t;
  }
  for (int k = tid; k < NBINS; k += 256) pw[k] = x[k].x * x[k].x + x[k].y * x[k].y;
  __syncthreads();
  float* orow = out + ((long long)b * n_frames + frame) * n_mels;
  for (int m0 = 0; m0 < n_mels; m0 += 64) {
    const int m = m0 + (tid >> 2), part = tid & 3;
    float acc = 0.f;
    if (m < n_mels) {
      const int lo = mel_range[2 * m], hi = mel_range[2 * m + 1];
      const float* fr = mel_basis + (long long)m * NBINS;
      for (int k = lo + part; k < hi; k += 4) acc = fmaf(fr[k], pw[k], acc);
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    // the logarithm alone runs in double (64 values per frame) and is rounded once, as the extractor's float64 spectrogram cast to
    // float32 is: the device's log10f is good to ~2 ulp, which at 20 - 30 dB is 4x the fp32 FFT's error in the mel power, and it puts
    // the clamp at -100.00001 dB instead of -100
    if (m < n_mels && part == 0) orow[m] = (float)(10.0 * log10((double)fmaxf(acc, 1e-10f)));
  }
}

// ---- input stage -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float cubic1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }

// value of channel c of the 256 x 256 spectrogram image at (row, col): frame t = (row / 64) * 256 + col of the time axis resized
// to 1024 frames (bicubic, align_corners=True, A = -0.75, clamped taps: torch's upsample_bicubic2d), mel bin f = row % 64,
// BatchNorm'd per bin
__device__ __forceinline__ float image_value(const float* __restrict__ mc, int T, float tscale, int row, int col,
                                             const float* __restrict__ bn_scale, const float* __restrict__ bn_shift) {
  const int f = row & 63;
  const int t = (row >> 6) * 256 + col;
  const float sc = bn_scale[f], sh = bn_shift[f];
  if (T == 1024) return fmaf(mc[(long long)t * 64 + f], sc, sh);
  const float real = tscale * (float)t;
  const int i0 = (int)floorf(real);
  const float u = real - (float)i0;
  const float A = -0.75f;
  const float c[4] = {cubic2(u + 1.f, A), cubic1(u, A), cubic1(1.f - u, A), cubic2(2.f - u, A)};
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int ti = i0 - 1 + k;
    ti = ti < 0 ? 0 : (ti > T - 1 ? T - 1 : ti);
    acc = fmaf(c[k], fmaf(mc[(long long)ti * 64 + f], sc, sh), acc);
  }
  return acc;
}

// one thread per (token, im2col element).  g: [B, 64, 64, 16] (proj, channel 0, 4 x 4 / stride 4);
// l: [B, 64, 64, 48] (mel_conv2d over channels 1..3, 4 x 12 / stride (4, 12): token column w = c * 21 + j, column 63 is padding)
__global__ __launch_bounds__(256) void clap_input_kernel(const float* __restrict__ mel, long long b_stride, long long c_stride, int T,
                                                         float tscale, const float* __restrict__ bn_scale,
                                                         const float* __restrict__ bn_shift, bf16* __restrict__ g,
                                                         bf16* __restrict__ l, int B) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ng = (long long)B * 4096 * 16;
  if (idx < ng) {
    const int e = (int)(idx & 15);
    const long long tok = idx >> 4;
    const int b = (int)(tok >> 12), h = (int)((tok >> 6) & 63), w = (int)(tok & 63);
    const float v = image_value(mel + b * b_stride, T, tscale, 4 * h + (e >> 2), 4 * w + (e & 3), bn_scale, bn_shift);
    g[idx] = (bf16)v;
    return;
  }
  if (l == nullptr) return;
  const long long li = idx - ng;
  if (li >= (long long)B * 4096 * 48) return;
  const int e = (int)(li % 48);
  const long long tok = li / 48;
  const int b = (int)(tok >> 12), h = (int)((tok >> 6) & 63), w = (int)(tok & 63);
  float v = 0.f;
  if (w < 63) {
    const int c = w / 21, j = w % 21, kh = e / 12, kw = e % 12;
    v = image_value(mel + b * b_stride + (1 + c) * c_stride, T, tscale, 4 * h + kh, 12 * j + kw, bn_scale, bn_shift);
  }
  l[li] = (bf16)v;
}

// ---- attentional feature fusion --------------------------------------------------------------------------------------------------
// a = h + r (r's token column 63 is the zero padding of the local branch: the GEMM's bias is not part of it), and mean_tokens(a).
// One workgroup per item; channel groups of 8 per lane, token stripes across the lanes, fixed-order reduction (deterministic).
__global__ __launch_bounds__(256) void aff_sum_pool_kernel(const bf16* __restrict__ hg, const bf16* __restrict__ rl, int C,
                                                           bf16* __restrict__ a, bf16* __restrict__ pooled) {
  __shared__ float part[256][8];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cg = C / 8;
  const int stripes = 256 / cg;                              // C <= 2048 so cg <= 256
  const int g = tid % cg, s = tid / cg;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (s < stripes) {
    for (int t = s; t < 4096; t += stripes) {
      const long long off = ((long long)b * 4096 + t) * C + g * 8;
      const bf16x8 hv = *(const bf16x8*)(hg + off);
      bf16x8 rv = *(const bf16x8*)(rl + off);
      bf16x8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float v = (float)hv[k] + ((t & 63) == 63 ? 0.f : (float)rv[k]);
        o[k] = (bf16)v;
        acc[k] += v;
      }
      *(bf16x8*)(a + off) = o;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) part[tid][k] = acc[k];
  __syncthreads();
  if (tid < cg) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float sum = 0.f;
      for (int q = 0; q < stripes; ++q) sum += part[q * cg + tid][k];
      pooled[(long long)b * C + tid * 8 + k] = (bf16)(sum * (1.f / 4096.f));
    }
  }
}

// out = longer[b] ? 2 h f + 2 r (1 - f), f = sigmoid(loc + glob[b]) : h
__global__ __launch_bounds__(256) void aff_combine_kernel(const bf16* __restrict__ hg, const bf16* __restrict__ rl,
                                                          const float* __restrict__ loc, const float* __restrict__ glob,
                                                          const int* __restrict__ longer, int C, long long n, bf16* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long tok = i / C;
  const int c = (int)(i - tok * C);
  const int b = (int)(tok >> 12);
  const float h = (float)hg[i];
  if (!longer[b]) {
    out[i] = (bf16)h;
    return;
  }
  const float r = (tok & 63) == 63 ? 0.f : (float)rl[i];
  const float f = 1.f / (1.f + expf(-(loc[i] + glob[(long long)b * C + c])));
  out[i] = (bf16)(2.f * h * f + 2.f * r * (1.f - f));
}

// ---- shifted-window attention ----------------------------------------------------------------------------------------------------
// One 64-lane workgroup per (window, head, item), one query token per lane.  K / V of the window are staged in LDS as fp32; every
// lane walks the 64 keys with broadcast LDS reads.  Token (y, x) of the rolled frame is token ((y + s) % H, (x + s) % W) of the
// image both on the way in (roll(-s) + window_partition) and on the way out (window_reverse + roll(+s)).
constexpr int WIN = 8, WT = WIN * WIN, HD = 24;

__global__ __launch_bounds__(64) void window_attention_kernel(const bf16* __restrict__ qkv, int ld, int H, int W, int heads,
                                                              int shift, const float* __restrict__ bias, float scale,
                                                              bf16* __restrict__ out, int ld_out) {
  __shared__ float4 ks[WT][HD / 4], vs[WT][HD / 4];
  const int lane = threadIdx.x;
  const int win = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int nww = W / WIN;
  const int wy = win / nww, wx = win - wy * nww;
  const int y = wy * WIN + (lane >> 3), x = wx * WIN + (lane & 7);           // rolled-frame coordinates of this lane's token
  int sy = y + shift, sx = x + shift;
  sy = sy >= H ? sy - H : sy;
  sx = sx >= W ? sx - W : sx;
  const long long row = (long long)b * H * W + (long long)sy * W + sx;
  const int C = heads * HD;
  const bf16* src = qkv + row * ld + head * HD;
  float q[HD];
#pragma unroll
  for (int c = 0; c < HD / 8; ++c) {
    const bf16x8 qv = *(const bf16x8*)(src + c * 8);
    const bf16x8 kv = *(const bf16x8*)(src + C + c * 8);
    const bf16x8 vv = *(const bf16x8*)(src + 2 * C + c * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) q[c * 8 + k] = (float)qv[k] * scale;
    ks[lane][2 * c] = make_float4((float)kv[0], (float)kv[1], (float)kv[2], (float)kv[3]);
    ks[lane][2 * c + 1] = make_float4((float)kv[4], (float)kv[5], (float)kv[6], (float)kv[7]);
    vs[lane][2 * c] = make_float4((float)vv[0], (float)vv[1], (float)vv[2], (float)vv[3]);
    vs[lane][2 * c + 1] = make_float4((float)vv[4], (float)vv[5], (float)vv[6], (float)vv[7]);
  }
  __syncthreads();
  // shift mask: region id of a rolled-frame coordinate along one axis (0 / 1 / 2: below H - WIN, below H - shift, the rest)
  const int ry = shift ? (y >= H - WIN) + (y >= H - shift) : 0;
  const int rx = shift ? (x >= W - WIN) + (x >= W - shift) : 0;
  const int my_region = ry * 3 + rx;
  const float* brow = bias + ((long long)head * WT + lane) * WT;
  float s[WT];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) {
      const float4 kv = ks[j][c];
      acc = fmaf(q[4 * c], kv.x, acc);
      acc = fmaf(q[4 * c + 1], kv.y, acc);
      acc = fmaf(q[4 * c + 2], kv.z, acc);
      acc = fmaf(q[4 * c + 3], kv.w, acc);
    }
    acc += brow[j];
    if (shift) {
      const int yj = wy * WIN + (j >> 3), xj = wx * WIN + (j & 7);
      const int rj = ((yj >= H - WIN) + (yj >= H - shift)) * 3 + (xj >= W - WIN) + (xj >= W - shift);
      if (rj != my_region) acc += -100.f;                   // transformers' mask value (not -inf)
    }
    s[j] = acc;
    mx = fmaxf(mx, acc);
  }
  float sum = 0.f;
  float o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) o[d] = 0.f;
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    const float p = expf(s[j] - mx);
    sum += p;
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) {
      const float4 vv = vs[j][c];
      o[4 * c] = fmaf(p, vv.x, o[4 * c]);
      o[4 * c + 1] = fmaf(p, vv.y, o[4 * c + 1]);
      o[4 * c + 2] = fmaf(p, vv.z, o[4 * c + 2]);
      o[4 * c + 3] = fmaf(p, vv.w, o[4 * c + 3]);
    }
  }
  const float inv = 1.f / sum;
  bf16* dst = out + row * ld_out + head * HD;
#pragma unroll
  for (int c = 0; c < HD / 8; ++c) {
    bf16x8 ov;
#pragma unroll
    for (int k = 0; k < 8; ++k) ov[k] = (bf16)(o[c * 8 + k] * inv);
    *(bf16x8*)(dst + c * 8) = ov;
  }
}

// ---- patch merging / pooling -----------------------------------------------------------------------------------------------------
// out[b, i, j, q C + c] = x[b, 2 i + (q & 1), 2 j + (q >> 1), c]   (q = 0..3: transformers' x0 (0,0), x1 (1,0), x2 (0,1), x3 (1,1))
__global__ __launch_bounds__(256) void patch_merge_gather_kernel(const bf16* __restrict__ x, int H, int W, int C, long long n8,
                                                                 bf16* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const long long e = i * 8;
  const int C4 = 4 * C;
  const long long tok = e / C4;
  const int col = (int)(e - tok * C4);
  const int q = col / C, c = col - q * C;
  const int Wo = W / 2, Ho = H / 2;
  const int j = (int)(tok % Wo);
  const long long r = tok / Wo;
  const int ii = (int)(r % Ho);
  const int b = (int)(r / Ho);
  const long long src = (((long long)b * H + 2 * ii + (q & 1)) * W + 2 * j + (q >> 1)) * C + c;
  *(bf16x8*)(out + e) = *(const bf16x8*)(x + src);
}

// mean over N tokens of x [B, N, C] -> fp32 and bf16 [B, C]; one lane per channel, fixed order
__global__ __launch_bounds__(256) void token_mean_kernel(const bf16* __restrict__ x, int N, int C, float* __restrict__ out_f32,
                                                         bf16* __restrict__ out_bf16) {
  const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (c >= C) return;
  const bf16* xb = x + (long long)b * N * C + c;
  float acc = 0.f;
  for (int t = 0; t < N; ++t) acc += (float)xb[(long long)t * C];
  acc /= (float)N;
  out_f32[(long long)b * C + c] = acc;
  out_bf16[(long long)b * C + c] = (bf16)acc;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned cdivu(long long a, int b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

extern "C" int aldm_resample_up3(const float* x, const int* lens, int B, int T_in, const float* taps, int ntaps, float* y,
                                 int T_out, void* stream) {
  ALDM_CHECK_ARG(x && lens && taps && y, "resample_up3: null pointer");
  ALDM_CHECK_ARG(B > 0 && T_in > 0 && T_out > 0 && ntaps > 0 && ntaps % 2 == 1, "resample_up3: bad dims");
  hipLaunchKernelGGL(resample_up3_kernel, dim3(cdivu(T_out, 256), B), dim3(256), 0, (hipStream_t)stream, x, lens, T_in, taps,
                     ntaps, y, T_out);
  return aldm_launch_status("resample_up3");
}

extern "C" int aldm_clap_log_mel(const float* wav, const int* lens, int B, int T, int max_len, int n_fft, int hop,
                                 const float* window, const float* mel_basis, const int* mel_range, int n_mels, float* out,
                                 void* stream) {
  ALDM_CHECK_ARG(wav && lens && window && mel_basis && mel_range && out, "clap_log_mel: null pointer");
  if (n_fft != NFFT) {
    aldm_set_error("clap_log_mel: n_fft %d unsupported (the LDS FFT is built for 1024)", n_fft);
    return ALDM_E_UNSUPPORTED;
  }
  ALDM_CHECK_ARG(B > 0 && T > 0 && hop > 0 && n_mels > 0 && max_len > NFFT / 2, "clap_log_mel: bad dims");
  const int n_frames = 1 + max_len / hop;                       // (max_len + n_fft - n_fft) / hop + 1
  hipLaunchKernelGGL(clap_log_mel_kernel, dim3(n_frames, B), dim3(256), 0, (hipStream_t)stream, wav, lens, T, max_len, hop,
                     n_frames, window, mel_basis, mel_range, n_mels, out);
  return aldm_launch_status("clap_log_mel");
}

extern "C" int aldm_clap_input(const float* mel, long long b_stride, long long c_stride, int B, int T, int n_mels,
                               const float* bn_scale, const float* bn_shift, void* g, void* l, void* stream) {
  ALDM_CHECK_ARG(mel && bn_scale && bn_shift && g && B > 0, "clap_input: null pointer / bad B");
  if (n_mels != 64 || T < 2 || T > 1024) {
    aldm_set_error("clap_input: %d frames x %d mel bins unsupported (needs 64 bins and 2..1024 frames: a 256 x 256 image)", T, n_mels);
    return ALDM_E_UNSUPPORTED;
  }
  const float tscale = (float)(T - 1) / (float)(1024 - 1);
  const long long n = (long long)B * 4096 * (16 + (l ? 48 : 0));
  hipLaunchKernelGGL(clap_input_kernel, dim3(cdivu(n, 256)), dim3(256), 0, (hipStream_t)stream, mel, b_stride, c_stride, T, tscale,
                     bn_scale, bn_shift, (bf16*)g, (bf16*)l, B);
  return aldm_launch_status("clap_input");
}

extern "C" int aldm_aff_sum_pool(const void* h, const void* r, int B, int C, void* a, void* pooled, void* stream) {
  ALDM_CHECK_ARG(h && r && a && pooled && B > 0, "aff_sum_pool: null pointer / bad B");
  if (C % 8 || C > 2048) {
    aldm_set_error("aff_sum_pool: C=%d must be a multiple of 8 and <= 2048", C);
    return ALDM_E_UNSUPPORTED;
  }
  if (!al16(h) || !al16(r) || !al16(a)) {
    aldm_set_error("aff_sum_pool: pointers must be 16-byte aligned");
    return ALDM_E_ALIGN;
  }
  hipLaunchKernelGGL(aff_sum_pool_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const bf16*)h, (const bf16*)r, C, (bf16*)a,
                     (bf16*)pooled);
  return aldm_launch_status("aff_sum_pool");
}

extern "C" int aldm_aff_combine(const void* h, const void* r, const float* loc, const float* glob, const int* longer, int B, int C,
                                void* out, void* stream) {
  ALDM_CHECK_ARG(h && r && loc && glob && longer && out && B > 0 && C > 0, "aff_combine: null pointer / bad dims");
  const long long n = (long long)B * 4096 * C;
  hipLaunchKernelGGL(aff_combine_kernel, dim3(cdivu(n, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)h, (const bf16*)r, loc,
                     glob, longer, C, n, (bf16*)out);
  return aldm_launch_status("aff_combine");
}

extern "C" int aldm_window_attention(const void* qkv, int ld, int B, int H, int W, int heads, int head_dim, int window, int shift,
                                     const float* bias, float scale, void* out, int ld_out, void* stream) {
  ALDM_CHECK_ARG(qkv && bias && out && B > 0 && heads > 0, "window_attention: null pointer / bad dims");
  if (head_dim != HD || window != WIN || H % WIN || W % WIN || H <= 0 || W <= 0 || shift < 0 || shift >= WIN) {
    aldm_set_error("window_attention: head dim %d, window %d, %d x %d tokens, shift %d unsupported (head dim 24, 8 x 8 windows tiling "
                   "the image, shift < 8)", head_dim, window, H, W, shift);
    return ALDM_E_UNSUPPORTED;
  }
  ALDM_CHECK_ARG(ld >= 3 * heads * HD && ld_out >= heads * HD, "window_attention: ld %d / ld_out %d too small", ld, ld_out);
  if (ld % 8 || ld_out % 8 || !al16(qkv) || !al16(out)) {
    aldm_set_error("window_attention: rows must be 16-byte aligned (ld %d, ld_out %d)", ld, ld_out);
    return ALDM_E_ALIGN;
  }
  hipLaunchKernelGGL(window_attention_kernel, dim3((H / WIN) * (W / WIN), heads, B), dim3(64), 0, (hipStream_t)stream,
                     (const bf16*)qkv, ld, H, W, heads, shift, bias, scale, (bf16*)out, ld_out);
  return aldm_launch_status("window_attention");
}

extern "C" int aldm_patch_merge_gather(const void* x, int B, int H, int W, int C, void* out, void* stream) {
  ALDM_CHECK_ARG(x && out && B > 0 && H > 0 && W > 0 && C > 0, "patch_merge_gather: null pointer / bad dims");
  if (H % 2 || W % 2 || C % 8) {
    aldm_set_error("patch_merge_gather: %d x %d x %d unsupported (even H, W; C %% 8 == 0)", H, W, C);
    return ALDM_E_UNSUPPORTED;
  }
  if (!al16(x) || !al16(out)) {
    aldm_set_error("patch_merge_gather: pointers must be 16-byte aligned");
    return ALDM_E_ALIGN;
  }
  const long long n8 = (long long)B * H * W * C / 8;
  hipLaunchKernelGGL(patch_merge_gather_kernel, dim3(cdivu(n8, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, H, W, C, n8,
                     (bf16*)out);
  return aldm_launch_status("patch_merge_gather");
}

extern "C" int aldm_token_mean(const void* x, int B, int N, int C, float* out_f32, void* out_bf16, void* stream) {
  ALDM_CHECK_ARG(x && out_f32 && out_bf16 && B > 0 && N > 0 && C > 0, "token_mean: null pointer / bad dims");
  hipLaunchKernelGGL(token_mean_kernel, dim3(cdivu(C, 256), B), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, N, C, out_f32,
                     (bf16*)out_bf16);
  return aldm_launch_status("token_mean");
}
