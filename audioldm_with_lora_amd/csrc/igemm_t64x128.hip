// Instantiates the implicit-GEMM kernels for the 64x128 workgroup tile (see igemm_core.h).
#include "igemm_core.h"
namespace aldm_igemm_detail {
int igemm_launch_t64x128(const aldm_igemm_variant_t& v, const IgemmDev& d, hipStream_t st) { return launch_ring_tile<ALDM_TILE_64x128>(v, d, st); }
}  // namespace aldm_igemm_detail
