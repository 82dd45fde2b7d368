// C-ABI entry of the implicit-GEMM family; the kernels live in igemm_core.h and are instantiated per tile shape in
// igemm_t*.hip (separate translation units so the build parallelises).
#include "igemm_core.h"

using namespace aldm_igemm_detail;

extern "C" size_t aldm_igemm_workspace_bytes(const aldm_igemm_t* p) {
  if (!p || p->splits <= 1) return 0;
  const long long M = (long long)p->B * p->OH * p->OW;
  return (size_t)p->splits * M * p->Cout * sizeof(float);
}

// Element offset, inside the workspace of a split-K launch over B images of HW pixels and C channels, of channel n of output row m in
// slab `split` -- the arithmetic of the kernels' slab stores (igemm_slab_index behind the same magic-number division), on the host, so
// that the layouts can be checked without a GPU.  layout: 0 row-major, 1 quad-planar.  -1 for an argument out of range.
extern "C" long long aldm_igemm_slab_offset(int layout, int B, int HW, int C, int split, int m, int n) {
  if (layout < 0 || layout > 1 || B <= 0 || HW <= 0 || C <= 0 || (C & 3) || split < 0 || m < 0 || n < 0 || n >= C ||
      (long long)B * HW > 0x7fffffffll || m >= B * HW)
    return -1;
  const FastDiv fd = make_fastdiv((unsigned)HW);
  const int b = (int)(((((unsigned long long)(unsigned)m * fd.mul) >> 32) + (unsigned)m) >> fd.shift);   // fdiv() without __umulhi
  const int pix = m - b * HW;
  return (long long)split * B * HW * C + (layout ? igemm_slab_index(1, b, pix, n, C, HW) : igemm_slab_index(0, 0, m, n, C, 0));
}

// The kernel arguments of a launch whose variant is selected, up to the grid (what igemm_reduce_kernel gets).  (IgemmDev is what every
// kernel's prologue fetches: host-only state travels in the variant beside it, never in it.)
static void fill_args(const aldm_igemm_t* p, const aldm_igemm_variant_t& v, IgemmDev& d) {
  const int Ctot = p->Cin + p->Cin2;
  const int Ktot = p->KH * p->KW * Ctot;
  const int Cext = p->x3 ? p->Cin3 + (p->x4 ? p->Cin4 : 0) : 0;
  d.x = (const bf16*)p->x; d.x2 = (const bf16*)p->x2; d.w = (const bf16*)p->w;
  d.lora_a = (const bf16*)p->lora_a; d.lora_b = (const bf16*)p->lora_b; d.lora_t_out = (bf16*)p->lora_t_out;
  d.bias = p->bias; d.rowbias = p->rowbias; d.res = (const bf16*)p->res; d.res2 = (const bf16*)p->res2;
  d.out = p->out; d.vt = (bf16*)p->vt; d.ws = p->workspace;
  d.B = p->B; d.IH = p->IH; d.IW = p->IW; d.Cin = p->Cin; d.Cin2 = p->Cin2; d.Ctot = Ctot; d.UH = p->UH; d.UW = p->UW; d.dilate = p->in_dilate;
  d.KH = p->KH; d.KW = p->KW; d.sh = p->stride_h; d.sw = p->stride_w; d.ph = p->pad_h; d.pw = p->pad_w;
  d.dh = p->dil_h; d.dw = p->dil_w;
  d.OH = p->OH; d.OW = p->OW; d.OHW = p->OH * p->OW; d.N = p->Cout; d.M = p->B * p->OH * p->OW; d.Kpad = p->Kpad;
  d.in_act = p->in_act; d.in_slope = p->in_slope;
  d.rowbias_ld = p->rowbias_ld; d.geglu = p->geglu; d.out_act = p->out_act; d.out_slope = p->out_slope;
  d.alpha = p->alpha;
  d.post_act = p->post_act; d.post_slope = p->post_slope; d.out2 = (bf16*)p->out2;
  d.out_f32 = p->out_dtype == ALDM_OUT_F32; d.out_ld = p->out_ld;
  d.out_bs = p->out_batch_stride; d.out_ps = p->out_pix_stride > 0 ? p->out_pix_stride : 1; d.out_po = p->out_pix_offset;
  d.vt_col0 = p->vt_col0; d.vt_ld = p->vt_ld; d.vt_bs = p->vt_batch_stride; d.vt_dual = p->vt ? p->vt_dual : 0;
  d.x3 = (const bf16*)p->x3; d.x4 = (const bf16*)p->x4; d.Cin3 = p->x3 ? p->Cin3 : 0; d.Cin4 = (p->x3 && p->x4) ? p->Cin4 : 0;
  d.C3tot = d.Cin3 + d.Cin4;
  d.nkt = cdiv(Ktot, BK) + d.C3tot / BK;
  d.splits = v.splits; d.kt_per_split = v.kt_per_split;
  d.ws_rows = d.M;
  // slab layout / store policy of a deferred reduce (the in-library reduce reads row-major slabs: flags only with defer_reduce)
  d.ws_mode = (d.splits > 1 && p->defer_reduce) ? (p->defer_reduce >> 1) & 3 : 0;
  if ((long long)p->B * p->OH * p->OW * p->Cout * 4 >= 0x80000000ll) d.ws_mode &= ~2;   // write-through stores take 32-bit byte offsets into a slab
  if (v.direct) d.ws_mode |= 4;
  d.lora_gate = p->lora_gate; d.fd_gate = make_fastdiv((unsigned)(p->lora_gate ? p->gate_rows : 1)); d.gate_m1 = d.M - 1;
  d.tiles_n = 0; d.tiles_m = 0; d.nwg = 0;
  const int xcd_map = p->xcd_map & ~ALDM_EPI_MASK;
  // which operand an XCD's L2 keeps (igemm_work_item).  Measured (round 4, profiles/r04_fetch_xcd_*.json + r04_step_table_xcd_*.txt):
  // weight-stationary more than halves the fabric fetches of the 252- / 64-token levels' launches (21.6 -> 9.8 MiB per launch on the
  // dominant symbol) and the split-K launches among them get ~1 us SLOWER (eight co-scheduled M-tiles of an XCD then ask one L2
  // channel for the same weight lines at the same instant; the re-fetches of the M-major map were Infinity-Cache hits, not HBM
  // traffic); unsplit launches with weights > activations gain (GEGLU at M = 512: 15.8 -> 14.5 us).  So: auto = weight-stationary
  // only for an unsplit launch whose weight matrix is the larger operand.
  const unsigned long long act = 2ull * p->B * p->IH * p->IW * Ctot + 2ull * p->B * p->OH * p->OW * Cext;
  const unsigned long long wgt = 2ull * p->Cout * p->Kpad;
  d.xmap = xcd_map ? xcd_map - 1 : ((wgt > act && p->splits <= 1) ? 1 : 0);
  const unsigned long long xb = 2ull * p->B * p->IH * p->IW * p->Cin, x2b = 2ull * p->B * p->IH * p->IW * p->Cin2;
  const unsigned long long wb = 2ull * p->Cout * p->Kpad, lb = 2ull * p->Rp * p->Kpad;
  const unsigned long long x3b = 2ull * p->B * p->OH * p->OW * d.Cin3, x4b = 2ull * p->B * p->OH * p->OW * d.Cin4;
  d.x3_bytes = (unsigned)x3b; d.x4_bytes = (unsigned)x4b;
  d.x_bytes = xb < 0xFFFFFFFFull ? (unsigned)xb : 0xFFFFFFFFu;
  d.x2_bytes = x2b < 0xFFFFFFFFull ? (unsigned)x2b : 0xFFFFFFFFu;
  d.w_bytes = (unsigned)wb;
  d.la_bytes = (unsigned)lb;
  d.lb_bytes = (unsigned)(2ull * p->Cout * p->Rp);
  d.fd_ohw = make_fastdiv((unsigned)d.OHW); d.fd_ow = make_fastdiv((unsigned)d.OW); d.fd_halo = make_fastdiv((unsigned)d.OW + 2u);
  d.fd_ctot = make_fastdiv((unsigned)d.Ctot); d.fd_kw = make_fastdiv((unsigned)d.KW);
  d.ln_s = p->ln_s; d.ln_sa = p->ln_sa; d.ln_ca = p->ln_ca; d.ln_eps = p->ln_eps;
  d.rowstat = p->rowstat_out; d.ln_parts = p->ln_parts; d.ln_np = p->ln_nparts;
  d.qstat = p->qstat_out; d.qtile = -1;
  d.gi_gamma = p->gnin_gamma; d.gi_beta = p->gnin_beta; d.gi_q1 = p->gnin_q1; d.gi_q2 = p->gnin_q2;
  d.gi_bm1 = p->gnin_bm1; d.gi_tpi1 = p->gnin_tpi1; d.gi_bm2 = p->gnin_bm2; d.gi_tpi2 = p->gnin_tpi2;
  d.gi_groups = p->gnin_groups; d.gi_act = p->gnin_act; d.gi_eps = p->gnin_eps;
#ifdef ALDM_DIAG
  d.diag = (p->splits <= 1) ? (unsigned long long*)p->workspace : nullptr;   // diagnostic build: workspace doubles as the stamp buffer
#else
  d.diag = nullptr;
#endif
}

// ... and what the selected kernel reads about its grid.  The halo kernels take tiles_m as the workgroups of one split and divide by the
// halo image's width (fd_halo) and -- wave-specialised -- by the filter's taps (fd_kw: kt_per_split / taps = chunks per split)
static void place_grid(const aldm_igemm_variant_t& v, IgemmDev& d) {
  if (v.transposed) {
    transpose_conv1d(d);
    d.fd_ow = make_fastdiv(1u);
    d.fd_ohw = make_fastdiv((unsigned)d.OHW);
  }
  d.tiles_n = v.tiles_n; d.fd_tiles_n = make_fastdiv((unsigned)v.tiles_n);
  d.tiles_m = v.tiles_m; d.fd_tiles_m = make_fastdiv((unsigned)v.tiles_m);
  if (v.family == ALDM_IGEMM_HALO_KERNEL) {
    d.fd_halo = make_fastdiv((unsigned)d.OW + 2u);
  } else if (v.family == ALDM_IGEMM_HALO_WS_KERNEL) {
    d.fd_kw = make_fastdiv((unsigned)(d.KH * d.KW));
    d.fd_halo = make_fastdiv((unsigned)(d.OW + (d.KW - 1) * d.dw));
  } else {
    d.fd_splits = make_fastdiv((unsigned)d.splits);
    d.nwg = (int)v.grid;
  }
}

// checks, select the variant, fill the kernel arguments, launch the variant, reduce the slabs unless the consumer does
extern "C" int aldm_igemm(const aldm_igemm_t* p, void* stream) {
  aldm_igemm_variant_t v;
  if (int rc = igemm_check_args(p)) return rc;
  if (int rc = igemm_select(p, &v)) return rc;
  IgemmDev d;
  fill_args(p, v, d);
  IgemmDev dd = d;
  place_grid(v, dd);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = igemm_tile(v.tile)->launch(v, dd, st)) return rc;
  if (d.splits > 1 && !p->defer_reduce) {
    const int ncols = d.geglu ? d.N / 2 : d.N;
    const long long work = (long long)d.M * (ncols / 4);
    hipLaunchKernelGGL(igemm_reduce_kernel, dim3((unsigned)cdivll(work, 256)), dim3(256), 0, st, d);
    return aldm_launch_status("igemm_reduce");
  }
  return ALDM_OK;
}
