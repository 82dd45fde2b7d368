// Instantiates the 8-wave (512-thread) 256x128 workgroup tile of the LDS-DMA implicit-GEMM kernel (see igemm_core.h): each wave owns
// 64x64 of the tile = 16 MFMAs per 8 fragment reads per k-step, and a K-tile costs the workgroup 6 DMA passes for 256 x 128 x 64
// MACs (the 128x128 tile: 4 passes for half the work).  For the big-M layers of the VAE and the vocoder (M >= 64k rows, thousands
// of workgroups), where neither launch latency nor workgroup count is the limit.  No LoRA / V^T forms: plain convolutions only.
#include "igemm_core.h"
namespace aldm_igemm_detail {
int igemm_launch_t256x128w8(const aldm_igemm_variant_t& v, const IgemmDev& d, hipStream_t st) { return launch_ring_tile<ALDM_TILE_256x128_W8>(v, d, st); }
}  // namespace aldm_igemm_detail
