// Instantiates the 8-wave (512-thread) 128x128 workgroup tile of the LDS-DMA implicit-GEMM kernel (see igemm_core.h):
// each wave owns 32x64 of the tile, so a wave issues half the DMA instructions per MFMA of the 4-wave 64x64 tile.
#include "igemm_core.h"
namespace aldm_igemm_detail {
int igemm_launch_t128x128w8(const aldm_igemm_variant_t& v, const IgemmDev& d, hipStream_t st) { return launch_ring_tile<ALDM_TILE_128x128_W8>(v, d, st); }
}  // namespace aldm_igemm_detail
