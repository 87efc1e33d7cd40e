// etc2_kernels.hip -- ETC2 RGBA8 (ETC1-compatible colour word + EAC alpha word) encode and decode kernels for gfx950
// (EXTENSION, include/ic_amd.h ICAMD_ETC2_RGBA8); see etc2_block.h for the alpha search and DESIGN.md 3.11.
//
// Encode: one block per lane on 16 x 16-block tiles (a wave = 16 x 4 blocks, the shape the ETC1 encoder's wave-uniform
// decisions are tuned for), four-wave workgroups.  The source is read ONCE: the lane's 16 RGBA texels feed the ETC1 block
// routine of etc1_block.h unchanged (same templates, same wave-uniform shortcuts, so bytes 8..15 are the ETC1 kernels'), the
// alpha bytes wait packed in four dwords and are searched after the colour registers are dead (two phases of one kernel: the
// ETC1 search alone fills the 128-VGPR budget).  Under kSmallerError the colour search leaves no register free: held to 128
// VGPRs the kernel spills 8 bytes (and 24 with the four dwords parked in LDS instead), so that one kernel may take 3 waves per
// SIMD -- it compiles to 132 VGPRs and no scratch; the alpha search, which is most of the time, needs few registers and no
// memory, so three waves keep the SIMD issuing.  Both halves leave as one 16-byte store.
// Decode: one block per lane, a 16-byte block load and four 16-byte row stores (RGBA8), clipped at the image's edge.
#include "etc2_encode_bodies.inc"  // etc2_encode_one: the encode body, shared with the chain kernels of etc2_mip_kernels.hip
#include "codec_info.h"
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

__device__ __forceinline__ void etc2_decode_one(const DecodeParams &P, uint32_t k) {
  const auto [img, rem, brow, bcol] = raster_block(P, k);
  const U4 v = load_stream(reinterpret_cast<const U4 *>(P.blocks + (size_t)img * P.src_image_stride + (size_t)rem * 16u));
  const uint32_t w[4] = { v.x, v.y, v.z, v.w };
  uint32_t px[16];
  decode_etc2_rgba8(w, P.swap_rb != 0u, px);
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

// (amdgpu_waves_per_eu(4): as the ETC1 kernels -- the colour search must fit 128 VGPRs; kSmallerError: 3 or 4, see above)
#define ICAMD_ETC2_KERNEL(name, strategy)                                                                              \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) __attribute__((amdgpu_waves_per_eu(strategy == 2 ? 3 : 4, 4))) name(GridParams P) { \
    etc2_encode_one<strategy>(P, tile_of_launch(P));                                                                                      \
  }
ICAMD_ETC2_KERNEL(icamd_etc2_rgba8_kernel, 2)            // kSmallerError (the reference's default)
ICAMD_ETC2_KERNEL(icamd_etc2_rgba8_split_h_kernel, 0)    // kSplitHorizontally
ICAMD_ETC2_KERNEL(icamd_etc2_rgba8_split_v_kernel, 1)    // kSplitVertically
ICAMD_ETC2_KERNEL(icamd_etc2_rgba8_heuristic_kernel, 3)  // kHeuristic
#undef ICAMD_ETC2_KERNEL

__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc2_rgba8_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) etc2_decode_one(P, k);
}

}  // extern "C"

const char *etc2_kernel_name(int comps) { return comps == 4 ? "icamd_etc2_rgba8_kernel" : ""; }

hipError_t launch_etc2(const GridParams &P, hipStream_t stream) {
  typedef void (*Kernel)(GridParams);
  static const Kernel kernels[4] = { icamd_etc2_rgba8_split_h_kernel, icamd_etc2_rgba8_split_v_kernel, icamd_etc2_rgba8_kernel,
                                     icamd_etc2_rgba8_heuristic_kernel };
  const Kernel k = kernels[P.etc_strategy < 4u ? P.etc_strategy : 2u];  // any other value is kSmallerError, as for ETC1
  return launch_tiled(k, k, P, stream, 4u);
}

hipError_t launch_etc2_decode(const DecodeParams &P, hipStream_t stream) {
  return launch_raster_decode(icamd_etc2_rgba8_decode_kernel, P, stream);
}

}  // namespace icamd
