// etc2_a1_kernels.hip -- ETC2 RGB8 with punch-through alpha encode and decode kernels for gfx950 (EXTENSION, include/ic_amd.h
// ICAMD_ETC2_RGB8A1); see etc2_a1_block.h for the block math and DESIGN.md 3.16.
//
// Encode: one block per lane on 16 x 16-block tiles, four-wave workgroups, the tiling and the two phases of the ETC2 RGB8
// kernels (etc2_rgb8_kernels.hip).  Phase one is the ETC1 block routine of etc1_block.h unchanged, run by the fully opaque
// lanes only and skipped by a wave that has none.  Phase two RELOADS the block (the ETC1 search alone fills the 128-VGPR budget)
// and makes the choice of etc2_a1_block: the masked differential search D partition by partition in waves where a lane needs
// it, then the planar candidate on the opaque lanes.  Every skip is a wave vote in which only the lanes that use the result
// take part; lanes outside the block grid have left before the first one.  The block leaves as one 8-byte store.
// Decode: one block per lane, an 8-byte block load and four 16-byte row stores (RGBA8), clipped at the image's edge.
#include "etc2_encode_bodies.inc"  // etc2_a1_encode_one: the encode body, shared with the chain kernels of etc2_mip_kernels.hip
#include "codec_info.h"
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

__device__ __forceinline__ void etc2_a1_decode_one(const DecodeParams &P, uint32_t k) {
  const auto [img, rem, brow, bcol] = raster_block(P, k);
  const U2 v = load_stream(reinterpret_cast<const U2 *>(P.blocks + (size_t)img * P.src_image_stride + (size_t)rem * 8u));
  uint32_t px[16];
  decode_etc2_a1(v.x, v.y, P.swap_rb != 0u, px);
  uint8_t *dst = P.pixels + (size_t)img * P.dst_image_stride;
  const uint32_t row = brow * 4u, col = bcol * 4u;
  if (row + 4u <= P.height && col + 4u <= P.width) {
#pragma unroll
    for (int y = 0; y < 4; ++y)
      store_stream16(dst + (size_t)(row + y) * P.row_stride + (size_t)col * 4u, px[4 * y], px[4 * y + 1], px[4 * y + 2],
                     px[4 * y + 3]);
  } else {  // clipped at the image's edge, pixel by pixel
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (row + y < P.height && col + x < P.width) {
          uint8_t *q = dst + (size_t)(row + y) * P.row_stride + (size_t)(col + x) * 4u;
          const uint32_t p = px[4 * y + x];
          q[0] = (uint8_t)p; q[1] = (uint8_t)(p >> 8); q[2] = (uint8_t)(p >> 16); q[3] = (uint8_t)(p >> 24);
        }
  }
}

extern "C" {

// (amdgpu_waves_per_eu(4): as the ETC1 kernels -- the colour search must fit 128 VGPRs)
#define ICAMD_ETC2_A1_KERNEL(name, strategy)                                                                           \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) __attribute__((amdgpu_waves_per_eu(4))) name(GridParams P) { \
    etc2_a1_encode_one<strategy>(P, tile_of_launch(P));                                                                                   \
  }
ICAMD_ETC2_A1_KERNEL(icamd_etc2_rgb8a1_kernel, 2)            // kSmallerError (the reference's default)
ICAMD_ETC2_A1_KERNEL(icamd_etc2_rgb8a1_split_h_kernel, 0)    // kSplitHorizontally
ICAMD_ETC2_A1_KERNEL(icamd_etc2_rgb8a1_split_v_kernel, 1)    // kSplitVertically
ICAMD_ETC2_A1_KERNEL(icamd_etc2_rgb8a1_heuristic_kernel, 3)  // kHeuristic
#undef ICAMD_ETC2_A1_KERNEL

__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc2_rgb8a1_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) etc2_a1_decode_one(P, k);
}

}  // extern "C"

const char *etc2_a1_kernel_name(int comps) { return comps == 4 ? "icamd_etc2_rgb8a1_kernel" : ""; }

hipError_t launch_etc2_a1(const GridParams &P, hipStream_t stream) {
  typedef void (*Kernel)(GridParams);
  static const Kernel kernels[4] = { icamd_etc2_rgb8a1_split_h_kernel, icamd_etc2_rgb8a1_split_v_kernel, icamd_etc2_rgb8a1_kernel,
                                     icamd_etc2_rgb8a1_heuristic_kernel };
  const Kernel k = kernels[P.etc_strategy < 4u ? P.etc_strategy : 2u];  // any other value is kSmallerError, as for ETC1
  return launch_tiled(k, k, P, stream, 4u);
}

hipError_t launch_etc2_a1_decode(const DecodeParams &P, hipStream_t stream) {
  return launch_raster_decode(icamd_etc2_rgb8a1_decode_kernel, P, stream);
}

}  // namespace icamd
