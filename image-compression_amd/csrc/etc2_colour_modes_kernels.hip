// etc2_colour_modes_kernels.hip -- the colour-mode passes of icamd_encode_etc2_colour_device for ICAMD_ETC2_RGBA8 and
// ICAMD_ETC2_RGB8A1 on gfx950 (EXTENSION, include/ic_amd.h); block math in etc2_colour_block.h, etc2_th_block.h and
// etc2_a1_th_block.h, DESIGN.md 3.19.
//
// A SECOND launch on the stream, after the codec's own kernel of the call's strategy (etc2_kernels.hip, etc2_a1_kernels.hip) has
// written every block: the same 16 x 16-block tiles and four-wave workgroups, one block per lane, one kernel whatever the
// strategy -- the form of the T / H pass of ETC2 RGB8 (etc2_th_kernels.hip), for its reasons: the first kernels sit at the
// 128-VGPR limit, and ICAMD_ETC2_COLOUR_DEFAULT launches exactly what icamd_encode_device launches.  A lane reads its sixteen
// texels (the loads of the first launch) and its colour word and stores 8 bytes ONLY where the word changes:
//   ETC2 RGBA8: the ETC1 word at offset 8 of the block becomes ICAMD_ETC2_RGB8's planar choice, then (TH) its T / H choice; the
//     alpha word at offset 0 is never written;
//   ETC2 RGB8A1: nothing (all transparent), the T / H search of ETC2 RGB8 (none transparent) or the masked search.
// No wave-uniform decision: every shortcut is a per-lane branch.
#include "etc2_encode_bodies.inc"  // etc2_rgba8_colour_one, etc2_a1_th_one
#include "codec_info.h"
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

extern "C" {

__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc2_rgba8_planar_kernel(GridParams P) {
  etc2_rgba8_colour_one<false>(P, tile_of_launch(P));
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc2_rgba8_planar_th_kernel(GridParams P) {
  etc2_rgba8_colour_one<true>(P, tile_of_launch(P));
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc2_a1_th_kernel(GridParams P) { etc2_a1_th_one(P, tile_of_launch(P)); }

}  // extern "C"

const char *etc2_colour_modes_kernel_name(int codec, int colour_modes) {
  if (codec == ICAMD_ETC2_RGBA8)
    return colour_modes == ICAMD_ETC2_COLOUR_PLANAR      ? "icamd_etc2_rgba8_planar_kernel"
           : colour_modes == ICAMD_ETC2_COLOUR_PLANAR_TH ? "icamd_etc2_rgba8_planar_th_kernel"
                                                         : "";
  return codec == ICAMD_ETC2_RGB8A1 && colour_modes == ICAMD_ETC2_COLOUR_PLANAR_TH ? "icamd_etc2_a1_th_kernel" : "";
}

hipError_t launch_etc2_colour_modes(int codec, int colour_modes, const GridParams &P, hipStream_t stream) {
  typedef void (*Kernel)(GridParams);
  const Kernel k = codec == ICAMD_ETC2_RGB8A1                     ? icamd_etc2_a1_th_kernel
                   : colour_modes == ICAMD_ETC2_COLOUR_PLANAR_TH ? icamd_etc2_rgba8_planar_th_kernel
                                                                 : icamd_etc2_rgba8_planar_kernel;
  return launch_tiled(k, k, P, stream, 4u);  // the tiling of launch_etc2 and launch_etc2_a1
}

}  // namespace icamd
