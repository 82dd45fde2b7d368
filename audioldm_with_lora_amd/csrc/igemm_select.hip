// Which kernel an aldm_igemm launch runs, with what grid, workgroup and LDS: one pure function of the argument struct and the tile
// table (igemm_select.h).  No device code and no device call in this file: the host queries at its end answer on any machine.
#include <stdio.h>
#include <string.h>

#include "igemm_select.h"

namespace aldm_igemm_detail {

static int pick_tile(int M, int N) {
  auto tiles = [&](int bm, int bn) { return (long long)cdiv(M, bm) * cdiv(N, bn); };
  if (N <= 64) return M >= 4096 ? ALDM_TILE_128x64 : ALDM_TILE_64x64;
  if (tiles(128, 128) >= 224) return ALDM_TILE_128x128;
  if (tiles(128, 64) >= 224) return ALDM_TILE_128x64;
  return ALDM_TILE_64x64;
}

// THE split rule (a consumer that sums a different number of slabs than the launch wrote reads stale data -- or, with planar slabs,
// another image's).  nkt = K-tiles of the whole launch including the fused x3 | x4 segment, nch = 64-channel chunks of the first source
// pair.  Generic clamp first (as every tile), then the halo tiles' per-chunk rule on the clamped count: they split by whole chunks (a
// chunk's halo serves its KH * KW taps in one workgroup).
static void plan_splits(int want, int nkt, int nch, int taps, bool halo, int& splits, int& kt_per_split) {
  splits = want > 1 ? want : 1;
  if (splits > nkt) splits = nkt;
  if (splits < 1) splits = 1;              // (no K at all: the argument checks refuse such a launch)
  kt_per_split = cdiv(nkt, splits);
  if (kt_per_split > 0) splits = cdiv(nkt, kt_per_split);
  if (halo && splits > 1 && nch > 0) {
    const int cps = cdiv(nch, splits > nch ? nch : splits);
    kt_per_split = taps * cps;
    splits = cdiv(nch, cps);
  }
}

// The LDS-DMA path: a scalar K cursor (64-channel K-tiles inside one tap of one source), no gather-side activation and < 2 GiB
// activations (32-bit buffer offsets, 0x80000000 = "padded tap")
static bool lds_dma_path(const aldm_igemm_t* p) {
  return p->in_act == ALDM_ACT_NONE && p->Cin % 64 == 0 && p->Cin2 % 64 == 0 && 2ull * p->B * p->IH * p->IW * p->Cin < 0x80000000ull &&
         2ull * p->B * p->IH * p->IW * p->Cin2 < 0x80000000ull;
}

// Launches that leave through the register-direct epilogue (igemm_epilogue_direct): the plain bf16 standard path -- what the LEAN non-V^T
// instantiations of the LDS-DMA kernels serve -- without a second residual, second output or LayerNorm hand-over, whole quads everywhere
// (8-byte loads / stores), with a row bias at most one image boundary per M-tile (the halo tiles are image-aligned), and a tile whose
// instantiation has the form compiled in (the DIRECT argument of igemm_epilogue: fewer than 16 accumulator blocks a lane, no LoRA side
// channel).  The kernels check none of this.
static bool epilogue_direct(const aldm_igemm_t* p, const IgemmTile* t, int splits) {
  return t && lds_dma_path(p) && splits <= 1 && !p->vt && !p->geglu && !p->ln_s && p->out_act == ALDM_ACT_NONE && p->post_act == ALDM_ACT_NONE &&
         !p->out2 && p->out_dtype == ALDM_OUT_BF16 && !p->res2 && !p->rowstat_out && p->Cout % 8 == 0 && p->out_ld % 4 == 0 &&
         p->out_batch_stride % 4 == 0 && (!p->rowbias || (p->rowbias_ld % 4 == 0 && (t->halo() || p->OH * p->OW >= t->bm))) && t->blocks() < 16 &&
         p->Rp == 0;
}

// The part of the selection that cannot fail, which is all aldm_igemm_epilogue_form and aldm_igemm_effective_splits ask for: the tile,
// the split and the direct-epilogue bit
static const IgemmTile* select_head(const aldm_igemm_t* p, aldm_igemm_variant_t* v) {
  memset(v, 0, sizeof(*v));
  v->tile = p->tile ? p->tile : pick_tile(p->B * p->OH * p->OW, p->Cout);
  const IgemmTile* t = igemm_tile(v->tile);
  const int Ctot = p->Cin + p->Cin2;
  const int nkt = cdiv(p->KH * p->KW * Ctot, BK) + (p->x3 ? (p->Cin3 + (p->x4 ? p->Cin4 : 0)) / BK : 0);
  plan_splits(p->splits, nkt, Ctot / BK, p->KH * p->KW, t && t->halo(), v->splits, v->kt_per_split);
  v->direct = (p->xcd_map & ALDM_EPI_MASK) != ALDM_EPI_LDS && epilogue_direct(p, t, v->splits);
  return t;
}

// EPI of the instantiation: 3 split-K (only the partial-tile store is compiled in), 2 GEGLU-only with a plain bf16 store, 1 LEAN (the
// common case -- standard epilogue, no activation -- and nothing else compiled in), 4 LEAN + GroupNorm statistics, 0 everything.  The
// tile says which of them it has.
static int epilogue_variant(const aldm_igemm_t* p, const IgemmTile& t, int splits, bool vt) {
  const bool act = p->out_act != ALDM_ACT_NONE || p->post_act != ALDM_ACT_NONE;
  auto has = [&](int e) { return (t.epis >> e) & 1u; };
  if (vt) return t.lean_vt && splits <= 1 && !p->geglu && !act ? 1 : 0;
  if (splits > 1) return has(3) ? 3 : 0;
  if (has(2) && p->Rp == 0 && p->geglu && !p->res && !p->res2 && p->out_dtype != ALDM_OUT_F32 && !act && p->alpha == 1.f) return 2;
  if (!p->geglu && !act && !p->ln_s) return p->Rp == 0 && p->qstat_out ? 4 : 1;
  return 0;
}

// S of the instantiation; *rs: the ws tiles' register-staged loaders.  `ring` (2..4) overrides the tile's default where the tile has
// that depth (tuning: tools/bench_igemm.py --ring); never more than the LDS a workgroup can own (ring + LoRA-B image + row statistics)
static int ring_depth(const aldm_igemm_t* p, const IgemmTile& t, bool ext, bool* rs) {
  *rs = t.kind == WS && p->ring == 2;
  if (*rs) return 2;
  if (ext) return 3;                       // the fused-shortcut form runs three halo buffers and a ring of 3
  int S = t.has_kernel_ring(p->ring) ? p->ring : (p->Rp ? t.ring_lora : t.ring0);
  while (!t.halo() && S > 2 && ring_loop_bytes(S, t.bm, t.bn, p->Rp) + stat_rows_bytes(t.bm) > IGEMM_MAX_LDS) --S;
  return S;
}

static int refuse(const char* text) {
  aldm_set_error("%s", text);
  return ALDM_E_UNSUPPORTED;
}

struct Geo { int KH, KW, dh, dw, ph, pw, sh, sw, OH, OW, IH, IW; };

// igemm_kernel / igemm_pipe_kernel / igemm_ws_kernel
static int select_ring(const aldm_igemm_t* p, const IgemmTile& t, aldm_igemm_variant_t* v) {
  const bool fast = lds_dma_path(p), vt = p->vt != nullptr;
  if ((!fast && !t.reg_staged) || !((t.rps >> (p->Rp / 32)) & 1u) || (vt && !t.vt) || (t.kind == WS && (p->ln_s || p->geglu))) return refuse(t.refusal);
  if (!fast && (p->ln_s || p->x3))
    return refuse("igemm: the folded LayerNorm / the fused second-source segment need the LDS-DMA path (Cin % 64 == 0, no gather activation)");
  bool rs = false;
  const int S = fast ? ring_depth(p, t, false, &rs) : 0;
  v->family = !S ? ALDM_IGEMM_KERNEL : t.kind == WS ? ALDM_IGEMM_WS_KERNEL : ALDM_IGEMM_PIPE_KERNEL;
  v->ring = S;
  v->epi = S ? epilogue_variant(p, t, v->splits, vt) : 0;
  const bool ws = t.kind == WS;
  if (ws) { v->nl = t.nl; v->rs = rs; }
  else { v->rp = p->Rp; v->vt = vt; v->gate = p->lora_gate != nullptr; }
  if (!ws && p->qstat_out && !(v->epi == 0 || v->epi == 4)) {
    aldm_set_error("igemm: qstat_out reached an epilogue instantiation without the statistics code (EPI %d)", v->epi);
    return ALDM_E_UNSUPPORTED;
  }
  // the statistics tables and the V^T block are addressed by whole tiles
  const bool whole = p->Cout % t.bn == 0;
  const char* bad = whole ? nullptr
                    : ws ? (p->qstat_out || p->rowstat_out ? "igemm: qstat_out / rowstat_out need Cout %d to be a multiple of the tile width %d" : nullptr)
                    : p->qstat_out ? "igemm: qstat_out needs Cout %d to be a multiple of the tile width %d"
                    : p->rowstat_out ? "igemm: rowstat_out needs Cout %d to be a multiple of the tile width %d" : nullptr;
  if (bad) {
    aldm_set_error(bad, p->Cout, t.bn);
    return ALDM_E_ARG;
  }
  if (vt && p->vt_col0 % t.bn != 0) {
    aldm_set_error("igemm: vt_col0 %d must be a multiple of the tile width %d", p->vt_col0, t.bn);
    return ALDM_E_ARG;
  }
  v->block = !S ? THREADS : 64 * (t.wm * t.wn + t.nl);
  v->lds = (unsigned)ring_lds_bytes(S, t.bm, t.bn, p->Rp);
  return ALDM_OK;
}

// igemm_halo_kernel / igemm_halo_ws_kernel; g: the geometry the kernel will see
static int select_halo(const aldm_igemm_t* p, const IgemmTile& t, Geo& g, aldm_igemm_variant_t* v) {
  const bool ws = t.kind == HALO_WS;
  // (qstat_out is fine with the halo tiles: they are image-aligned, slot 0)
  if (p->Rp || p->vt || p->rowstat_out || (p->x3 && !ws)) return refuse(t.refusal);
  const int Cin3 = p->x3 ? p->Cin3 : 0, C3tot = Cin3 + (p->x3 && p->x4 ? p->Cin4 : 0);
  if (ws && g.KH == 1 && g.OH == 1 && g.IH == 1 && p->UH == 0 && g.ph == 0 && g.dh == 1 && g.sh == 1 && C3tot == 0 && !p->gnin_gamma) {
    transpose_conv1d(g);
    v->transposed = 1;
  }
  const bool same = ws ? (g.KH % 2 == 1 && g.KW % 2 == 1 && 2 * g.ph == (g.KH - 1) * g.dh && 2 * g.pw == (g.KW - 1) * g.dw &&
                          ((g.KH == 3 && g.KW == 3 && g.dh == 1 && g.dw == 1) || (C3tot == 0 && !p->gnin_gamma && p->UH == 0)))
                       : (g.KH == 3 && g.KW == 3 && g.ph == 1 && g.pw == 1 && g.dh == 1 && g.dw == 1);
  const bool ok = same && g.sh == 1 && g.sw == 1 && lds_dma_path(p) && p->in_dilate == 0 && !p->ln_s && !p->geglu &&
                  ((p->UH == 0 && p->UW == 0) || (p->UH > 0 && p->UW > 0)) && g.OH == (p->UH ? p->UH : g.IH) && g.OW == (p->UW ? p->UW : g.IW);
  if (!ok)
    return refuse("igemm_halo: needs a stride-1 'same' convolution on the LDS-DMA path (Cin % 64 == 0, no gather activation): 3x3, or -- wave-specialised tiles -- any odd filter with dilation");
  // halo rows the tile needs: BM / OW image rows and the filter's reach around them.  At 128 rows, three DMA passes (192) cover OW <= 16
  // -- the UNet's latents; the VAE's 64-wide images need 264: five passes, 80 KB for the two halo buffers
  const int rows_pt = t.bm / g.OW;
  const int need = (rows_pt + (g.KH - 1) * g.dh) * (g.OW + (g.KW - 1) * g.dw);
  const bool ext = C3tot > 0;
  if (ext) {                               // the fused 1x1 segment: wave-specialised tiles, the fused form's halo capacity
    const bool fits = p->UH == 0 && C3tot % 64 == 0 && Cin3 % 64 == 0;
    if (!fits || !t.hp_fused || (t.hp_fused < t.hp_max() && need > t.hp_fused * 64))
      return refuse("igemm_halo: the second-source segment needs a wave-specialised halo tile whose halo fits three DMA passes (OW >= 8 at 128 rows)");
    if (p->gnin_gamma) return refuse("igemm_halo: gnin_* launches take no second-source segment");
    v->hp = t.hp_fused;
  } else {
    v->hp = need > t.hp[0] * 64 ? t.hp_max() : t.hp[0];
    if (p->gnin_gamma && v->splits > 1) return refuse("igemm_halo: gnin_* launches are not split");
    if (p->gnin_gamma && (p->out_act != ALDM_ACT_NONE || p->post_act != ALDM_ACT_NONE)) return refuse("igemm_halo: gnin_* launches take no output activation");
  }
  bool rs;
  v->family = ws ? ALDM_IGEMM_HALO_WS_KERNEL : ALDM_IGEMM_HALO_KERNEL;
  v->ring = ring_depth(p, t, ext, &rs);
  v->epi = epilogue_variant(p, t, v->splits, false);
  v->gnin = p->gnin_gamma != nullptr; v->ext = ext;
  if (t.bm % g.OW != 0 || need > v->hp * 64) {
    aldm_set_error("igemm_halo: image width %d / filter %dx%d does not fit the %dx%d halo tile (%d halo rows of %d)", g.OW, g.KH, g.KW, t.bm, t.bn, need, v->hp * 64);
    return ALDM_E_UNSUPPORTED;
  }
  v->block = ws ? 768 : 512;
  v->lds = (unsigned)halo_lds_bytes(v->hp, v->ring, t.bm, t.bn, v->gnin, ext);
  return ALDM_OK;
}

static void variant_name(aldm_igemm_variant_t* v) {
  auto b = [](int x) { return x ? "true" : "false"; };
  char a[96];
  switch (v->family) {
    case ALDM_IGEMM_KERNEL: snprintf(a, sizeof(a), "kernel<%d, %d, %d, %d, %d, %s, %s>", v->bm, v->bn, v->wm, v->wn, v->rp, b(v->vt), b(v->gate)); break;
    case ALDM_IGEMM_PIPE_KERNEL: snprintf(a, sizeof(a), "pipe_kernel<%d, %d, %d, %d, %d, %s, %d, %d, %s>", v->bm, v->bn, v->wm, v->wn, v->rp, b(v->vt), v->ring, v->epi, b(v->gate)); break;
    case ALDM_IGEMM_WS_KERNEL: snprintf(a, sizeof(a), "ws_kernel<%d, %d, %d, %d, %d, %d, %d, %s>", v->bm, v->bn, v->wm, v->wn, v->nl, v->ring, v->epi, b(v->rs)); break;
    case ALDM_IGEMM_HALO_KERNEL: snprintf(a, sizeof(a), "halo_kernel<%d, %d, %d, %d, %d, %d, %d, %s>", v->bm, v->bn, v->wm, v->wn, v->hp, v->ring, v->epi, b(v->gnin)); break;
    default: snprintf(a, sizeof(a), "halo_ws_kernel<%d, %d, %d, %d, %d, %d, %d, %s, %s>", v->bm, v->bn, v->wm, v->wn, v->hp, v->ring, v->epi, b(v->gnin), b(v->ext)); break;
  }
  snprintf(v->name, sizeof(v->name), "void aldm_igemm_detail::igemm_%s(aldm_igemm_detail::IgemmDev)", a);
}

int igemm_check_args(const aldm_igemm_t* p) {
  ALDM_CHECK_ARG(p && p->x && p->w && p->out, "igemm: null x/w/out");
  ALDM_CHECK_ARG(p->B > 0 && p->IH > 0 && p->IW > 0 && p->OH > 0 && p->OW > 0 && p->Cout > 0, "igemm: bad dims");
  ALDM_CHECK_ARG(p->Cin > 0 && p->Cin % 8 == 0 && p->Cin2 >= 0 && p->Cin2 % 8 == 0, "igemm: Cin/Cin2 must be multiples of 8 (got %d,%d)", p->Cin, p->Cin2);
  ALDM_CHECK_ARG(p->Cin2 == 0 || p->x2, "igemm: Cin2 without x2");
  ALDM_CHECK_ARG(p->KH > 0 && p->KW > 0, "igemm: bad filter");
  const int Ktot = p->KH * p->KW * (p->Cin + p->Cin2);
  const int Cext = p->x3 ? p->Cin3 + (p->x4 ? p->Cin4 : 0) : 0;
  ALDM_CHECK_ARG(p->Kpad % BK == 0 && p->Kpad >= Ktot + Cext, "igemm: Kpad %d must be a multiple of 64 and >= %d", p->Kpad, Ktot + Cext);
  ALDM_CHECK_ARG(!p->x3 || (p->Cin3 > 0 && p->Cin3 % 64 == 0 && (!p->x4 || (p->Cin4 > 0 && p->Cin4 % 64 == 0)) && Ktot % 64 == 0 &&
                            p->Cin % 64 == 0 && p->Cin2 % 64 == 0 && p->in_act == ALDM_ACT_NONE && !p->ln_s && !p->vt && !p->geglu &&
                            p->in_dilate == 0 && p->Rp == 0),
                 "igemm: the fused 1x1 second-source segment (x3 | x4) needs the plain LDS-DMA path: every channel count and KH*KW*(Cin+Cin2) a multiple of 64");
  ALDM_CHECK_ARG(p->x3 || !p->x4, "igemm: x4 without x3");
  ALDM_CHECK_ARG(!p->vt_dual || (p->vt && !p->res && !p->res2 && !p->out2 && p->out_act == ALDM_ACT_NONE && p->post_act == ALDM_ACT_NONE &&
                                 p->alpha == 1.f && !p->rowbias && p->out_dtype == ALDM_OUT_BF16),
                 "igemm: vt_dual needs vt and the plain bf16 epilogue (bias only)");
  ALDM_CHECK_ARG(p->Rp == 0 || p->Rp == 32 || p->Rp == 64, "igemm: Rp must be 0/32/64");
  ALDM_CHECK_ARG(p->Rp == 0 || (p->lora_a && p->lora_b), "igemm: Rp without lora_a/lora_b");
  ALDM_CHECK_ARG(!p->lora_gate || p->Rp, "igemm: lora_gate without an adapter");
  ALDM_CHECK_ARG(!p->lora_gate || p->Rp == 32, "igemm: lora_gate needs Rp == 32 (the gate table's width; got %d)", p->Rp);
  ALDM_CHECK_ARG(!p->lora_gate || !p->lora_t_out, "igemm: lora_t_out (the trainer's copy of T) is not combined with lora_gate");
  ALDM_CHECK_ARG(!p->lora_gate || (p->gate_rows > 0 && (p->B * p->OH * p->OW) % p->gate_rows == 0),
                 "igemm: lora_gate needs gate_rows > 0 dividing M (got %d rows per sample, M %d)", p->gate_rows, p->B * p->OH * p->OW);
  ALDM_CHECK_ARG(!p->geglu || (p->Cout % 32 == 0 && !p->rowbias), "igemm: GEGLU needs Cout %% 32 == 0");
  ALDM_CHECK_ARG(!p->vt || (p->vt_col0 % 16 == 0 && p->splits <= 1 && !p->geglu), "igemm: bad vt config");
  ALDM_CHECK_ARG(!p->vt || p->vt_col0 > 0 || p->out, "igemm: out required");
  ALDM_CHECK_ARG(p->splits <= 1 || (p->workspace && p->Cout % 4 == 0), "igemm: split-K needs workspace and Cout %% 4 == 0");
  ALDM_CHECK_ARG(p->out_ld > 0, "igemm: out_ld");
  ALDM_CHECK_ARG(p->defer_reduce >= 0 && p->defer_reduce <= 7 && (!(p->defer_reduce & 6) || (p->defer_reduce & 1)), "igemm: defer_reduce is a set of ALDM_DEFER_* flags");
  ALDM_CHECK_ARG(!p->defer_reduce || (!p->geglu && !p->res2 && !p->out2 && p->out_act == ALDM_ACT_NONE && p->post_act == ALDM_ACT_NONE && p->alpha == 1.f),
                 "igemm: defer_reduce leaves bias / row bias / res to the consumer and supports nothing else in the epilogue");
  ALDM_CHECK_ARG(!(p->geglu && p->out2) || (p->Rp == 0 && p->splits <= 1 && !p->res && !p->res2 && p->out_dtype == ALDM_OUT_BF16 &&
                                            p->out_act == ALDM_ACT_NONE && p->post_act == ALDM_ACT_NONE && p->alpha == 1.f &&
                                            p->in_act == ALDM_ACT_NONE && p->Cin % 64 == 0 && p->Cin2 % 64 == 0 && p->Cout % 32 == 0),
                 "igemm: GEGLU with out2 (pre-activation copy) needs the plain LDS-DMA GEGLU launch (no residual / activation / split-K)");
  ALDM_CHECK_ARG(!p->ln_s || (p->KH == 1 && p->KW == 1 && p->Cin2 == 0 && p->splits <= 1 && (p->Rp == 0 || (p->ln_sa && p->ln_ca))),
                 "igemm: folded LayerNorm needs a 1x1 single-source GEMM without split-K (and ln_sa/ln_ca with LoRA)");
  ALDM_CHECK_ARG(!p->rowstat_out || (!p->vt && p->splits <= 1 && !p->geglu && p->out_dtype == ALDM_OUT_BF16 && p->Cout % 64 == 0 && !p->out2),
                 "igemm: rowstat_out needs the standard bf16 epilogue (no V^T / split-K / GEGLU / out2) and Cout %% 64 == 0");
  ALDM_CHECK_ARG(!p->qstat_out || (!p->vt && p->splits <= 1 && !p->geglu && p->out_dtype == ALDM_OUT_BF16 && p->Cout % 8 == 0 &&
                                   p->out_pix_stride <= 1 && p->Rp == 0 && !p->ln_s && !p->rowstat_out),
                 "igemm: qstat_out needs the standard bf16 epilogue (no V^T / split-K / GEGLU / LoRA / LayerNorm hand-over) and Cout %% 8 == 0");
  ALDM_CHECK_ARG(!p->ln_parts || (p->ln_s && p->ln_nparts > 0 && p->ln_nparts <= 64), "igemm: ln_parts needs ln_s and 1..64 partials per row");
  ALDM_CHECK_ARG(p->ring == 0 || (p->ring >= 2 && p->ring <= 4), "igemm: ring must be 0 (auto) or 2..4");
  ALDM_CHECK_ARG(p->in_dilate == 0 || (p->in_dilate == 2 && p->UH == 0), "igemm: in_dilate must be 0 or 2 (and excludes UH/UW)");
  return ALDM_OK;
}

int igemm_select(const aldm_igemm_t* p, aldm_igemm_variant_t* v) {
  // epilogue form (aldm_igemm_t.xcd_map bits 4-5, epilogue_direct above): the register-direct store where the launch can take it
  const int form = p->xcd_map & ALDM_EPI_MASK;
  ALDM_CHECK_ARG(form == ALDM_EPI_AUTO || form == ALDM_EPI_LDS || form == ALDM_EPI_DIRECT, "igemm: bad epilogue form in xcd_map");
  const IgemmTile* t = select_head(p, v);
  if (form == ALDM_EPI_DIRECT && !v->direct)
    return refuse("igemm: ALDM_EPI_DIRECT asked for a launch the register-direct epilogue cannot take (aldm_igemm_epilogue_form)");
  const int xcd_map = p->xcd_map & ~ALDM_EPI_MASK;
  ALDM_CHECK_ARG(xcd_map >= 0 && xcd_map <= 2, "igemm: xcd_map must be 0 (auto), 1 (activation-stationary) or 2 (weight-stationary)");
  ALDM_CHECK_ARG(2ull * p->Cout * p->Kpad < 0xFFFFFFFFull, "igemm: weight matrix too large for 32-bit offsets");
  ALDM_CHECK_ARG(!p->x3 || (2ull * p->B * p->OH * p->OW * p->Cin3 < 0x80000000ull && (!p->x4 || 2ull * p->B * p->OH * p->OW * p->Cin4 < 0x80000000ull)),
                 "igemm: x3 / x4 too large for 32-bit offsets");
  if (p->gnin_gamma) {
    ALDM_CHECK_ARG(t && t->halo(), "igemm: gnin_* (GroupNorm of the input inside the launch) needs a halo tile");
    const int Ct = p->Cin + p->Cin2;
    ALDM_CHECK_ARG(p->gnin_beta && p->gnin_q1 && (p->Cin2 == 0 || p->gnin_q2) && p->gnin_groups > 0 && p->gnin_groups <= 64 && Ct % p->gnin_groups == 0 &&
                   (Ct / p->gnin_groups) % 4 == 0 && Ct <= 512 && p->UH == 0 &&
                   (p->gnin_tpi1 > 0 || (p->gnin_bm1 > 0 && p->gnin_bm1 <= p->IH * p->IW)) &&
                   (p->Cin2 == 0 || p->gnin_tpi2 > 0 || (p->gnin_bm2 > 0 && p->gnin_bm2 <= p->IH * p->IW)) &&
                   (p->gnin_act == ALDM_ACT_NONE || p->gnin_act == ALDM_ACT_SILU),
                   "igemm: gnin_*: tables for every source, group width a multiple of 4, at most 512 input channels, no up-sampling, act NONE / SILU");
  }
  if (!t) {
    aldm_set_error("igemm: unknown tile %d", v->tile);
    return ALDM_E_UNSUPPORTED;
  }
  v->bm = t->bm; v->bn = t->bn; v->wm = t->wm; v->wn = t->wn;
  Geo g{p->KH, p->KW, p->dil_h, p->dil_w, p->pad_h, p->pad_w, p->stride_h, p->stride_w, p->OH, p->OW, p->IH, p->IW};
  if (int rc = t->halo() ? select_halo(p, *t, g, v) : select_ring(p, *t, v)) return rc;
  // the grid: one-dimensional.  Halo kernels: a tile is BM / OW whole rows of one image, and tiles_m counts the workgroups of a split
  // (the divisor that peels the split off blockIdx.x)
  v->tiles_n = cdiv(p->Cout, t->bn);
  v->tiles_m = t->halo() ? p->B * cdiv(g.OH, t->bm / g.OW) * v->tiles_n : cdiv(p->B * p->OH * p->OW, t->bm);
  v->grid = (unsigned)(v->tiles_m * (t->halo() ? 1 : v->tiles_n) * v->splits);
  variant_name(v);
  return ALDM_OK;
}

}  // namespace aldm_igemm_detail

using namespace aldm_igemm_detail;

extern "C" int aldm_igemm_variant(const aldm_igemm_t* p, aldm_igemm_variant_t* v) {
  ALDM_CHECK_ARG(v, "igemm_variant: null result");
  if (int rc = igemm_check_args(p)) return rc;
  return igemm_select(p, v);
}

extern "C" int aldm_igemm_tile_info(int tile, aldm_igemm_tile_info_t* info) {
  ALDM_CHECK_ARG(info, "igemm_tile_info: null result");
  const IgemmTile* t = igemm_tile(tile);
  if (!t) {
    aldm_set_error("igemm: unknown tile %d", tile);
    return ALDM_E_UNSUPPORTED;
  }
  *info = {t->id, t->kind, t->bm, t->bn, t->wm, t->wn, t->blocks(), t->rings, t->ring0, t->ring_lora, t->hp_max() * 64, t->hp_fused * 64};
  return ALDM_OK;
}

// 1: aldm_igemm would run this launch with the register-direct epilogue, 0: with the LDS walk (tests, tools)
extern "C" int aldm_igemm_epilogue_form(const aldm_igemm_t* p) {
  aldm_igemm_variant_t v;
  if (!p) return 0;
  select_head(p, &v);
  return v.direct;
}

// the split count the launch really uses (and a consumer of its slabs must sum)
extern "C" int aldm_igemm_effective_splits(const aldm_igemm_t* p) {
  aldm_igemm_variant_t v;
  if (!p || p->splits <= 1) return 1;
  select_head(p, &v);
  return v.splits;
}
