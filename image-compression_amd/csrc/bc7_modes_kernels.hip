// bc7_modes_kernels.hip -- BC7 with the opt-in mode-1 / mode-5 candidates for gfx950 (EXTENSION, include/ic_amd.h
// ICAMD_BC7_MODES_EXTENDED).  FUSED: one kernel reads the source once, encodes the mode-6 block exactly as
// bc7_kernels.hip does, measures it, fits the block's one candidate (mode 1 on opaque blocks, mode 5 on the others) and
// writes whichever is strictly closer.  One 4 x 4 block per lane on the tiles of launch_tiled, as bc7_kernels.hip; integer
// only, everything in registers (no LDS, no scratch, no wave-uniform shortcut: every branch of bc7_modes_block.h is per lane).
#include "bptc_encode_bodies.inc"  // bc7_modes_encode_one
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

extern "C" {
// *_kernel: 256 x 1-block tiles (block grids more than 128 columns wide); *_narrow_kernel: any tile shape
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc7_modes_rgba8_kernel(GridParams P) { bc7_modes_encode_one<4, true>(P, tile_of_launch(P)); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc7_modes_rgb888_kernel(GridParams P) { bc7_modes_encode_one<3, true>(P, tile_of_launch(P)); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc7_modes_rgba8_narrow_kernel(GridParams P) { bc7_modes_encode_one<4, false>(P, tile_of_launch(P)); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc7_modes_rgb888_narrow_kernel(GridParams P) { bc7_modes_encode_one<3, false>(P, tile_of_launch(P)); }
}  // extern "C"

const char *bc7_modes_kernel_name(int comps) {
  return comps == 4 ? "icamd_bc7_modes_rgba8_kernel" : comps == 3 ? "icamd_bc7_modes_rgb888_kernel" : "";
}

hipError_t launch_bc7_modes_encode(int comps, const GridParams &P, hipStream_t stream) {
  if (comps == 4) return launch_tiled(icamd_bc7_modes_rgba8_kernel, icamd_bc7_modes_rgba8_narrow_kernel, P, stream);
  if (comps == 3) return launch_tiled(icamd_bc7_modes_rgb888_kernel, icamd_bc7_modes_rgb888_narrow_kernel, P, stream);
  return hipErrorInvalidValue;
}

}  // namespace icamd
