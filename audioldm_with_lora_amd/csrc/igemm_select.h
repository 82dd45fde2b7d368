// Host side of the implicit-GEMM dispatch: THE tile table, and the selection of a launch's kernel variant (igemm_select.hip).
// Nothing here needs a device.  aldm_igemm (igemm.hip) selects, then calls the row's launcher with the selected variant; the
// launchers (igemm_core.h, igemm_ws.hip, igemm_halo.hip) map the variant's values to the instantiation and read the same rows at
// compile time to decide which instantiations exist.  A new tile is one row here plus its launcher.
#pragma once
#include "common.h"

namespace aldm_igemm_detail {

constexpr int BK = 64;
constexpr int THREADS = 256;                      // igemm_kernel's workgroup
constexpr size_t IGEMM_MAX_LDS = 160 * 1024;      // what one workgroup can own

struct IgemmDev;
// every family launcher: the kernel arguments are complete, the variant names the instantiation, grid, workgroup and LDS bytes
typedef int IgemmLaunch(const aldm_igemm_variant_t& v, const IgemmDev& d, hipStream_t st);
// one per translation unit that instantiates kernels (igemm_t*.hip, igemm_ws.hip, igemm_halo.hip)
IgemmLaunch igemm_launch_t128x128, igemm_launch_t128x64, igemm_launch_t64x128, igemm_launch_t64x64, igemm_launch_t128x128w8,
    igemm_launch_t256x128w8, igemm_launch_t64w8, igemm_launch_ws, igemm_launch_halo;

template <class... I>
constexpr unsigned bits(I... i) { return ((1u << i) | ... | 0u); }

enum { W4 = ALDM_IGEMM_KIND_W4, W8 = ALDM_IGEMM_KIND_W8, WS = ALDM_IGEMM_KIND_WS, HALO = ALDM_IGEMM_KIND_HALO, HALO_WS = ALDM_IGEMM_KIND_HALO_WS };

struct IgemmTile {
  int id, kind;
  int bm, bn, wm, wn;          // workgroup tile, (compute) waves along M / N
  unsigned rings;              // bit S: LDS-DMA ring depth S can be asked for (igemm_plan.TILES[].rings)
  int ring0, ring_lora;        // the depth ring = 0 gets without / with LoRA (the LoRA rows + B tile cost LDS; chosen so that the
                               // workgroups-per-CU count does not drop, which matters more than depth for the short-K projection GEMMs)
  unsigned rps;                // bit RP / 32: LoRA ranks instantiated
  unsigned epis;               // bit EPI: epilogue forms instantiated
  bool reg_staged;             // igemm_kernel serves what the LDS-DMA path cannot take
  bool vt, lean_vt;            // V^T instantiations, their lean form
  int hp[2], hp_fused;         // halo tiles: DMA passes (64 rows each) of the halo image, smaller first; of the fused-shortcut form (0: none)
  int nl;                      // loader waves (ws)
  IgemmLaunch* launch;
  const char* refusal;         // what the tile answers to a launch it has no instantiation for
  constexpr bool halo() const { return kind == HALO || kind == HALO_WS; }
  constexpr int blocks() const { return (bm / wm / 16) * (bn / wn / 16); }   // 16x16 accumulator blocks per lane
  constexpr int hp_max() const { return hp[1] ? hp[1] : hp[0]; }
  constexpr bool has_ring(int s) const { return s >= 2 && s <= 4 && ((rings >> s) & 1u); }
  // the ring depths with kernels behind them: the loader waves have no 2-deep LDS-DMA ring (ws tiles: ring 2 = register-staged loaders)
  constexpr bool has_kernel_ring(int s) const { return kind == WS ? (s == 2 || has_ring(s)) : kind == HALO_WS ? (s != 2 && has_ring(s)) : has_ring(s); }
};

constexpr unsigned ALL_EPI = bits(0, 1, 2, 3, 4), NO_GEGLU_EPI = bits(0, 1, 3, 4), UNSPLIT_EPI = bits(0, 1, 4);
constexpr const char* W8S_REFUSAL = "igemm: the 8-wave small tiles need the LDS-DMA path, no LoRA side channel and no V^T store";
constexpr const char* WS_REFUSAL = "igemm: the wave-specialised tiles take plain launches only (LDS-DMA path, no LoRA / V^T / folded LayerNorm / GEGLU)";
constexpr const char* HALO_REFUSAL = "igemm: the halo tiles take no LoRA / V^T / row statistics (and a second-source segment only in the wave-specialised forms)";

// ALDM_TILE_32x64 has no row: it cannot be launched
inline constexpr IgemmTile IGEMM_TILES[] = {
    //id                        kind     bm   bn  wm wn  rings          r0 rL rps            epis          reg    vt     lean   hp      fused nl launch
    {ALDM_TILE_128x128,         W4,      128, 128, 2, 2, bits(2, 3, 4), 3, 2, bits(0, 1, 2), ALL_EPI,      true,  true,  true,  {0, 0}, 0, 0, &igemm_launch_t128x128, nullptr},
    {ALDM_TILE_64x64,           W4,      64,  64,  2, 2, bits(2, 3, 4), 4, 3, bits(0, 1, 2), ALL_EPI,      true,  true,  true,  {0, 0}, 0, 0, &igemm_launch_t64x64, nullptr},
    {ALDM_TILE_128x64,          W4,      128, 64,  2, 2, bits(2, 3, 4), 3, 2, bits(0, 1, 2), ALL_EPI,      true,  true,  true,  {0, 0}, 0, 0, &igemm_launch_t128x64, nullptr},
    {ALDM_TILE_64x128,          W4,      64,  128, 2, 2, bits(2, 3, 4), 3, 2, bits(0, 1, 2), ALL_EPI,      true,  true,  true,  {0, 0}, 0, 0, &igemm_launch_t64x128, nullptr},
    {ALDM_TILE_128x128_W8,      W8,      128, 128, 4, 2, bits(2, 3),    2, 2, bits(0, 2),    UNSPLIT_EPI,  false, true,  false, {0, 0}, 0, 0, &igemm_launch_t128x128w8,
     "igemm: the 8-wave tile needs the LDS-DMA path and Rp in {0, 64}"},
    {ALDM_TILE_HALO_128x128,    HALO,    128, 128, 4, 2, bits(2, 3, 4), 3, 3, bits(0),       NO_GEGLU_EPI, false, false, false, {3, 5}, 0, 0, &igemm_launch_halo, HALO_REFUSAL},
    {ALDM_TILE_HALO_64x128,     HALO,    64,  128, 2, 4, bits(2, 3, 4), 3, 3, bits(0),       NO_GEGLU_EPI, false, false, false, {2, 0}, 0, 0, &igemm_launch_halo, HALO_REFUSAL},
    {ALDM_TILE_256x128_W8,      W8,      256, 128, 4, 2, bits(2, 3),    2, 2, bits(0),       UNSPLIT_EPI,  false, false, false, {0, 0}, 0, 0, &igemm_launch_t256x128w8,
     "igemm: the 256x128 tile needs the LDS-DMA path and takes no LoRA / V^T"},
    {ALDM_TILE_64x128_W8,       W8,      64,  128, 2, 4, bits(2, 3, 4), 3, 3, bits(0),       NO_GEGLU_EPI, false, false, false, {0, 0}, 0, 0, &igemm_launch_t64w8, W8S_REFUSAL},
    {ALDM_TILE_128x64_W8,       W8,      128, 64,  4, 2, bits(2, 3, 4), 3, 3, bits(0),       NO_GEGLU_EPI, false, false, false, {0, 0}, 0, 0, &igemm_launch_t64w8, W8S_REFUSAL},
    {ALDM_TILE_256x128_WS,      WS,      256, 128, 4, 2, bits(3),       3, 3, bits(0),       NO_GEGLU_EPI, false, false, false, {0, 0}, 0, 4, &igemm_launch_ws, WS_REFUSAL},
    {ALDM_TILE_64x128_WS,       WS,      64,  128, 2, 2, bits(3, 4),    3, 3, bits(0),       NO_GEGLU_EPI, false, false, false, {0, 0}, 0, 4, &igemm_launch_ws, WS_REFUSAL},
    {ALDM_TILE_128x64_WS,       WS,      128, 64,  2, 2, bits(3, 4),    3, 3, bits(0),       NO_GEGLU_EPI, false, false, false, {0, 0}, 0, 4, &igemm_launch_ws, WS_REFUSAL},
    {ALDM_TILE_HALO_128x128_WS, HALO_WS, 128, 128, 4, 2, bits(2, 3, 4), 3, 3, bits(0),       NO_GEGLU_EPI, false, false, false, {3, 5}, 3, 0, &igemm_launch_halo, HALO_REFUSAL},
    {ALDM_TILE_HALO_64x128_WS,  HALO_WS, 64,  128, 2, 4, bits(2, 3, 4), 3, 3, bits(0),       NO_GEGLU_EPI, false, false, false, {2, 0}, 2, 0, &igemm_launch_halo, HALO_REFUSAL},
};

constexpr const IgemmTile* igemm_tile(int id) {
  for (const IgemmTile& t : IGEMM_TILES)
    if (t.id == id) return &t;
  return nullptr;
}

// ---- LDS of a workgroup -------------------------------------------------------------------------------------------------------------
// the epilogue's fp32 image of the tile, or its transpose for V^T tiles (EpiCfg in igemm_core.h)
constexpr size_t epi_image_bytes(int bm, int bn) { return (size_t)(bm * (bn + 4) > bn * (bm + 4) ? bm * (bn + 4) : bn * (bm + 4)) * 4; }
// K loop of the ring kernels.  S == 0 (igemm_kernel): register-staged double buffer, needed when the gather applies an activation;
// else S stages of the LDS-DMA ring (+ the LoRA-B image)
constexpr size_t ring_loop_bytes(int S, int bm, int bn, int rp) {
  return (size_t)(S ? S : 2) * (bm + bn + rp) * 128 + (S && rp ? (size_t)bn * 128 : 0);
}
constexpr size_t stat_rows_bytes(int bm) { return 2 * bm * sizeof(float); }
constexpr size_t ring_lds_bytes(int S, int bm, int bn, int rp) {
  return (ring_loop_bytes(S, bm, bn, rp) > epi_image_bytes(bm, bn) ? ring_loop_bytes(S, bm, bn, rp) : epi_image_bytes(bm, bn)) + stat_rows_bytes(bm);
}
// halo kernels: two halo images (three in the fused-shortcut form) of hp * 64 rows, S weight stages, the GNIN tables
constexpr size_t halo_lds_bytes(int hp, int S, int bm, int bn, bool gnin, bool ext) {
  const size_t loop = (ext ? 3 : 2) * (size_t)hp * 64 * 128 + (size_t)S * bn * 128 + (gnin ? (1024 + 128) * sizeof(float) : 0);
  return loop > epi_image_bytes(bm, bn) ? loop : epi_image_bytes(bm, bn);
}

// A 1-D convolution (conv1d = KH 1 over a 1 x T image) read as a T x 1 image under a KW x 1 filter -- the halo tile is then BM consecutive
// time steps, its halo BM + (KW - 1) dw rows, the weight layout [(tap, c)] is unchanged.  G: the selection's geometry or IgemmDev.
template <class G>
void transpose_conv1d(G& g) {
  g.KH = g.KW; g.KW = 1; g.dh = g.dw; g.dw = 1; g.ph = g.pw; g.pw = 0;
  g.OH = g.OW; g.OW = 1; g.IH = g.IW; g.IW = 1; g.sh = g.sw; g.sw = 1;
}

// the argument checks that need no tile; then the selection: 0 and *v, or the code and text aldm_igemm answers with
int igemm_check_args(const aldm_igemm_t* p);
int igemm_select(const aldm_igemm_t* p, aldm_igemm_variant_t* v);

}  // namespace aldm_igemm_detail
