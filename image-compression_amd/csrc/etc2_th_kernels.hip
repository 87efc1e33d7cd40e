// etc2_th_kernels.hip -- the T / H pass of icamd_encode_etc2_device(ICAMD_ETC2_RGB8, ..., ICAMD_ETC2_MODES_TH) for gfx950
// (EXTENSION, include/ic_amd.h); see etc2_th_block.h for the block math and DESIGN.md 3.17.
//
// A SECOND launch on the stream, after the ETC2 RGB8 kernel of the call's strategy (etc2_rgb8_kernels.hip) has written the word W
// of every block: the same 16 x 16-block tiles and four-wave workgroups, one block per lane, one kernel per source component
// count whatever the strategy.  A lane reads its sixteen texels (the loads of the first launch: same edge replication, same
// padded-grid fetch) and W, measures W through decode_etc2_colour, runs the search and stores 8 bytes ONLY where a T or H word
// is strictly closer -- every other block keeps the first launch's bytes untouched.  The search so stays out of the ETC1 search's
// 128-VGPR budget, and modes 0 launches exactly what icamd_encode_device launches.  No wave-uniform decision: every shortcut of
// etc2_th_block.h is a per-lane branch.
#include "etc2_encode_bodies.inc"  // etc2_th_encode_one: the pass's body, shared with the chain kernels of etc2_mip_kernels.hip
#include "codec_info.h"
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

extern "C" {

__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc2_th_rgb888_kernel(GridParams P) { etc2_th_encode_one<3>(P, tile_of_launch(P)); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc2_th_rgba8_kernel(GridParams P) { etc2_th_encode_one<4>(P, tile_of_launch(P)); }

}  // extern "C"

const char *etc2_th_kernel_name(int comps) {
  return comps == 4 ? "icamd_etc2_th_rgba8_kernel" : comps == 3 ? "icamd_etc2_th_rgb888_kernel" : "";
}

hipError_t launch_etc2_th(int comps, const GridParams &P, hipStream_t stream) {
  typedef void (*Kernel)(GridParams);
  const Kernel k = comps == 4 ? icamd_etc2_th_rgba8_kernel : icamd_etc2_th_rgb888_kernel;
  return launch_tiled(k, k, P, stream, 4u);  // the tiling of launch_etc2_rgb8
}

}  // namespace icamd
