// Instantiates 8-wave (512-thread) forms of the SMALL workgroup tiles of the LDS-DMA implicit-GEMM kernel (see igemm_core.h), for the
// split-K convolutions of the UNet's 252- / 64-token levels: there the grid is about one workgroup per CU, and with four waves (one per
// SIMD) a K-tile's LDS-DMA issue (~50 % of a wave's cycles: the vector-memory path delivers ~70 GB/s per CU), its fragment reads + MFMAs
// (~33 %) and its barrier ADD UP in every wave.  Eight waves halve each wave's DMA instructions per K-tile and put two waves on every
// SIMD, so one wave's MFMAs run under the other's DMA issue.  64x128: 2 x 4 waves of 32x32; 128x64: 4 x 2 waves of 32x32.
#include "igemm_core.h"
namespace aldm_igemm_detail {
int igemm_launch_t64w8(const aldm_igemm_variant_t& v, const IgemmDev& d, hipStream_t st) {
  return with_constant<ALDM_TILE_64x128_W8, ALDM_TILE_128x64_W8>(v.tile, [&](auto tile) { return launch_ring_tile<decltype(tile)::value>(v, d, st); });
}
}  // namespace aldm_igemm_detail
