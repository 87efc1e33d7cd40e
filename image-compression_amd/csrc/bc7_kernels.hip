// bc7_kernels.hip -- BC7 (BPTC) for gfx950 (EXTENSION, include/ic_amd.h ICAMD_BC7): the mode-6 encoder and the
// decoder of all eight modes.  One 4 x 4 block per lane; the encoder runs on the tiles of launch_tiled like DXT5 (a wave reads
// 64 consecutive blocks' row segments and writes 64 consecutive 16-byte blocks), the decoder on blocks in raster order like the
// DXT decoders.  Integer only, everything in registers (no LDS, no scratch, no wave-uniform shortcut).  The metric kernels are
// in metric_kernels.hip (metric_bc7_block).
#include "bptc_encode_bodies.inc"  // bc7_encode_one
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

// Blocks in raster order of the images' block grids; RGBA8 rows.  Blocks the image's edge clips are written pixel by pixel.
__device__ __forceinline__ void bc7_decode_one(const DecodeParams &P, uint32_t k) {
  const auto [img, rem, brow, bcol] = raster_block(P, k);
  const U4 v = load_stream(reinterpret_cast<const U4 *>(P.blocks + (size_t)img * P.src_image_stride + (size_t)rem * 16u));
  const uint32_t w[4] = { v.x, v.y, v.z, v.w };
  uint32_t px[16];
  decode_bc7(w, P.swap_rb != 0, px);
  uint8_t *dst = P.pixels + (size_t)img * P.dst_image_stride;
  const uint32_t row = brow * 4, col = bcol * 4;
  if (row + 4 <= P.height && col + 4 <= P.width) {
#pragma unroll
    for (int y = 0; y < 4; ++y)
      store_stream16(dst + (size_t)(row + y) * P.row_stride + (size_t)col * 4u, px[4 * y], px[4 * y + 1], px[4 * y + 2], px[4 * y + 3]);
  } else {
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (row + y < P.height && col + x < P.width) {
          uint8_t *q = dst + (size_t)(row + y) * P.row_stride + (size_t)(col + x) * 4u;
          const uint32_t t = px[4 * y + x];
          q[0] = (uint8_t)t; q[1] = (uint8_t)(t >> 8); q[2] = (uint8_t)(t >> 16); q[3] = (uint8_t)(t >> 24);
        }
  }
}

extern "C" {
// *_kernel: 256 x 1-block tiles (block grids more than 128 columns wide); *_narrow_kernel: any tile shape
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc7_rgba8_kernel(GridParams P) { bc7_encode_one<4, true>(P, tile_of_launch(P)); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc7_rgb888_kernel(GridParams P) { bc7_encode_one<3, true>(P, tile_of_launch(P)); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc7_rgba8_narrow_kernel(GridParams P) { bc7_encode_one<4, false>(P, tile_of_launch(P)); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc7_rgb888_narrow_kernel(GridParams P) { bc7_encode_one<3, false>(P, tile_of_launch(P)); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc7_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) bc7_decode_one(P, k);
}
}  // extern "C"

const char *bc7_kernel_name(int comps) {
  return comps == 4 ? "icamd_bc7_rgba8_kernel" : comps == 3 ? "icamd_bc7_rgb888_kernel" : "";
}

hipError_t launch_bc7_encode(int comps, const GridParams &P, hipStream_t stream) {
  if (comps == 4) return launch_tiled(icamd_bc7_rgba8_kernel, icamd_bc7_rgba8_narrow_kernel, P, stream);
  if (comps == 3) return launch_tiled(icamd_bc7_rgb888_kernel, icamd_bc7_rgb888_narrow_kernel, P, stream);
  return hipErrorInvalidValue;
}

hipError_t launch_bc7_decode(const DecodeParams &P, hipStream_t stream) {
  return launch_raster_decode(icamd_bc7_decode_kernel, P, stream);
}

}  // namespace icamd
