// etc2_rgb8_kernels.hip -- ETC2 RGB8 (ETC1 block or planar block, whichever is closer) encode and decode kernels for gfx950
// (EXTENSION, include/ic_amd.h ICAMD_ETC2_RGB8); see etc2_colour_block.h for the block math and DESIGN.md 3.13.
//
// Encode: one block per lane on 16 x 16-block tiles, four-wave workgroups, as the ETC2 RGBA8 kernels.  Phase one is the ETC1
// block routine of etc1_block.h unchanged (same templates, same wave-uniform shortcuts, so an ETC1 outcome is the ETC1
// kernels' word byte for byte).  Phase two -- the ETC1 word's error, the least-squares plane, its error, the choice -- needs the
// sixteen texels again, and the ETC1 search alone fills the 128-VGPR budget: the lane RELOADS its block (the lines were read by
// this wave a few thousand instructions earlier) instead of holding sixteen registers across the search, which keeps every
// strategy at four waves per SIMD and without scratch.  Phase two has no wave-uniform decision.
// The block leaves as one 8-byte store.
// Decode: one block per lane, an 8-byte block load and four 12-byte row stores (RGB888), clipped at the image's edge.
#include "etc2_encode_bodies.inc"  // etc2_rgb8_encode_one: the encode body, shared with the chain kernels of etc2_mip_kernels.hip
#include "codec_info.h"
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

__device__ __forceinline__ void etc2_rgb8_decode_one(const DecodeParams &P, uint32_t k) {
  const auto [img, rem, brow, bcol] = raster_block(P, k);
  const U2 v = load_stream(reinterpret_cast<const U2 *>(P.blocks + (size_t)img * P.src_image_stride + (size_t)rem * 8u));
  uint32_t px[16];
  decode_etc2_colour(v.x, v.y, px);
  uint8_t *dst = P.pixels + (size_t)img * P.dst_image_stride;
  const uint32_t row = brow * 4u, col = bcol * 4u;
  if (row + 4u <= P.height && col + 4u <= P.width) {
#pragma unroll
    for (int y = 0; y < 4; ++y)  // four 3-byte texels as the twelve bytes R G B R | G B R G | B R G B
      store_stream12(dst + (size_t)(row + y) * P.row_stride + (size_t)col * 3u, px[4 * y] | px[4 * y + 1] << 24,
                     px[4 * y + 1] >> 8 | px[4 * y + 2] << 16, px[4 * y + 2] >> 16 | px[4 * y + 3] << 8);
  } else {  // clipped at the image's edge, pixel by pixel
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (row + y < P.height && col + x < P.width) {
          uint8_t *q = dst + (size_t)(row + y) * P.row_stride + (size_t)(col + x) * 3u;
          const uint32_t p = px[4 * y + x];
          q[0] = (uint8_t)p; q[1] = (uint8_t)(p >> 8); q[2] = (uint8_t)(p >> 16);
        }
  }
}

extern "C" {

// (amdgpu_waves_per_eu(4): as the ETC1 kernels -- the colour search must fit 128 VGPRs)
#define ICAMD_ETC2_RGB8_KERNEL(name, comps, strategy)                                                                  \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) __attribute__((amdgpu_waves_per_eu(4))) name(GridParams P) { \
    etc2_rgb8_encode_one<comps, strategy>(P, tile_of_launch(P));                                                                          \
  }
ICAMD_ETC2_RGB8_KERNEL(icamd_etc2_rgb8_rgb888_kernel, 3, 2)            // kSmallerError (the reference's default)
ICAMD_ETC2_RGB8_KERNEL(icamd_etc2_rgb8_rgba8_kernel, 4, 2)
ICAMD_ETC2_RGB8_KERNEL(icamd_etc2_rgb8_rgb888_split_h_kernel, 3, 0)    // kSplitHorizontally
ICAMD_ETC2_RGB8_KERNEL(icamd_etc2_rgb8_rgba8_split_h_kernel, 4, 0)
ICAMD_ETC2_RGB8_KERNEL(icamd_etc2_rgb8_rgb888_split_v_kernel, 3, 1)    // kSplitVertically
ICAMD_ETC2_RGB8_KERNEL(icamd_etc2_rgb8_rgba8_split_v_kernel, 4, 1)
ICAMD_ETC2_RGB8_KERNEL(icamd_etc2_rgb8_rgb888_heuristic_kernel, 3, 3)  // kHeuristic
ICAMD_ETC2_RGB8_KERNEL(icamd_etc2_rgb8_rgba8_heuristic_kernel, 4, 3)
#undef ICAMD_ETC2_RGB8_KERNEL

__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc2_rgb8_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) etc2_rgb8_decode_one(P, k);
}

}  // extern "C"

const char *etc2_rgb8_kernel_name(int comps) {
  return comps == 4 ? "icamd_etc2_rgb8_rgba8_kernel" : comps == 3 ? "icamd_etc2_rgb8_rgb888_kernel" : "";
}

hipError_t launch_etc2_rgb8(int comps, const GridParams &P, hipStream_t stream) {
  typedef void (*Kernel)(GridParams);
  static const Kernel kernels[2][4] = {
    { icamd_etc2_rgb8_rgb888_split_h_kernel, icamd_etc2_rgb8_rgb888_split_v_kernel, icamd_etc2_rgb8_rgb888_kernel,
      icamd_etc2_rgb8_rgb888_heuristic_kernel },
    { icamd_etc2_rgb8_rgba8_split_h_kernel, icamd_etc2_rgb8_rgba8_split_v_kernel, icamd_etc2_rgb8_rgba8_kernel,
      icamd_etc2_rgb8_rgba8_heuristic_kernel } };
  const Kernel k = kernels[comps == 4 ? 1 : 0][P.etc_strategy < 4u ? P.etc_strategy : 2u];  // any other value is kSmallerError
  return launch_tiled(k, k, P, stream, 4u);
}

hipError_t launch_etc2_rgb8_decode(const DecodeParams &P, hipStream_t stream) {
  return launch_raster_decode(icamd_etc2_rgb8_decode_kernel, P, stream);
}

}  // namespace icamd
