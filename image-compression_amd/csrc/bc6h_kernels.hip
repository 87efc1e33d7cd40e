// bc6h_kernels.hip -- BC6H (BPTC float) for gfx950 (EXTENSION, include/ic_amd.h icamd_encode_bc6h_device): the
// one-subset encoder, the decoder of all fourteen modes and the metric; see bc6h_block.h for the block math.
//
// Encode: one 4 x 4 block per lane on the tiles of launch_tiled like BC7 (a wave reads 64 consecutive blocks' row segments and
// writes 64 consecutive 16-byte blocks).  The fetch is the 16-bit EAC encoder's: four row loads of 8 C bytes at a 64-bit lane
// address (any 2-byte alignment, any even row padding) where the block lies in the image, the clamp-to-edge gather otherwise, so
// GridParams::force_gather is not read.  Integer only, everything in registers (no LDS, no scratch).
// Decode: blocks in raster order like bc7_decode_one; RGBA16F rows, A = 0x3C00: two 16-byte stores per pixel row of a block,
// 8-byte stores per pixel on the blocks the image's edge clips.  Lanes of a wave hold different modes: no wave-uniform shortcut.
// Metric: the walk of metric_walk.inc (blocks in raster order of the images' own grids, four per lane) over Bc6hAcc; sums are
// 64-bit from the lane on, lanes meet by wave shuffles and every wave adds its sums to the image's record.
#include "bptc_encode_bodies.inc"  // bc6h_encode_one
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

#include "metric_walk.inc"

template <bool SIGNED>
__device__ __forceinline__ void bc6h_decode_one(const DecodeParams &P, uint32_t k) {
  const auto [img, rem, brow, bcol] = raster_block(P, k);
  const U4 v = load_stream(reinterpret_cast<const U4 *>(P.blocks + (size_t)img * P.src_image_stride + (size_t)rem * 16u));
  const uint32_t w[4] = { v.x, v.y, v.z, v.w };
  uint32_t rg[16], b[16];
  decode_bc6h<SIGNED>(w, rg, b);
  uint8_t *dst = P.pixels + (size_t)img * P.dst_image_stride;
  const uint32_t row = brow * 4, col = bcol * 4;
  constexpr uint32_t kOne = 0x3c000000u;  // A = 1.0 in the high half
  if (row + 4 <= P.height && col + 4 <= P.width) {
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      uint8_t *q = dst + (size_t)(row + y) * P.row_stride + (size_t)col * 8u;
      store_stream16(q, rg[4 * y], b[4 * y] | kOne, rg[4 * y + 1], b[4 * y + 1] | kOne);
      store_stream16(q + 16, rg[4 * y + 2], b[4 * y + 2] | kOne, rg[4 * y + 3], b[4 * y + 3] | kOne);
    }
  } else {
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (row + y < P.height && col + x < P.width)
          store_stream8(dst + (size_t)(row + y) * P.row_stride + (size_t)(col + x) * 8u, rg[4 * y + x], b[4 * y + x] | kOne);
  }
}

template <int C, bool SIGNED>
__device__ __forceinline__ void bc6h_metric(const MetricParams &P) {
  metric_walk<MetricWideOps<Bc6hAcc, 3>>(P, [&](uint32_t img, uint32_t brow, uint32_t bcol, Bc6hAcc &acc) {
    const uint8_t *blk = P.blocks + (size_t)img * P.blocks_image_stride + ((size_t)brow * P.grid_cols + bcol) * 16u;
    const U4 v = load_stream(reinterpret_cast<const U4 *>(blk));
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    metric_bc6h_block<C, SIGNED>(w, P.src + (size_t)img * P.src_image_stride, P.height, P.width, P.row_stride, brow * 4u, bcol * 4u,
                                 acc);
  });
}

extern "C" {

// *_kernel: 256 x 1-block tiles (block grids more than 128 columns wide); *_narrow_kernel: any tile shape
#define ICAMD_BC6H_KERNELS(X)                                                                                               \
  X(bc6h_uf16_rgb16f, ICAMD_BC6H_UF16, 3, false)                                                                            \
  X(bc6h_uf16_rgba16f, ICAMD_BC6H_UF16, 4, false)                                                                           \
  X(bc6h_sf16_rgb16f, ICAMD_BC6H_SF16, 3, true)                                                                             \
  X(bc6h_sf16_rgba16f, ICAMD_BC6H_SF16, 4, true)

#define ICAMD_BC6H_DEFINE(stem, codec, chans, is_signed)                                                                    \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_##stem##_kernel(GridParams P) {                             \
    bc6h_encode_one<chans, is_signed, true>(P, tile_of_launch(P));                                                                             \
  }                                                                                                                         \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_##stem##_narrow_kernel(GridParams P) {                      \
    bc6h_encode_one<chans, is_signed, false>(P, tile_of_launch(P));                                                                            \
  }                                                                                                                         \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_metric_##stem##_kernel(MetricParams P) {                    \
    bc6h_metric<chans, is_signed>(P);                                                                                       \
  }
ICAMD_BC6H_KERNELS(ICAMD_BC6H_DEFINE)
#undef ICAMD_BC6H_DEFINE

__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc6h_uf16_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) bc6h_decode_one<false>(P, k);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc6h_sf16_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) bc6h_decode_one<true>(P, k);
}

}  // extern "C"

namespace {
struct Bc6hKernel {
  int codec, chans;
  void (*wide)(GridParams);
  void (*narrow)(GridParams);
  void (*metric)(MetricParams);
  const char *name, *metric_name;
};
#define ICAMD_BC6H_ENTRY(stem, codec, chans, is_signed) \
  { codec, chans, icamd_##stem##_kernel, icamd_##stem##_narrow_kernel, icamd_metric_##stem##_kernel, "icamd_" #stem "_kernel", \
    "icamd_metric_" #stem "_kernel" },
const Bc6hKernel kBc6hKernels[] = { ICAMD_BC6H_KERNELS(ICAMD_BC6H_ENTRY) };
#undef ICAMD_BC6H_ENTRY
const Bc6hKernel *find_bc6h(int codec, int chans) {
  for (const Bc6hKernel &k : kBc6hKernels)
    if (k.codec == codec && k.chans == chans) return &k;
  return nullptr;
}
}  // namespace
#undef ICAMD_BC6H_KERNELS

const char *bc6h_kernel_name(int codec, int chans) {
  const Bc6hKernel *k = find_bc6h(codec, chans);
  return k ? k->name : "";
}
const char *bc6h_metric_kernel_name(int codec, int chans) {
  const Bc6hKernel *k = find_bc6h(codec, chans);
  return k ? k->metric_name : "";
}

hipError_t launch_bc6h_encode(int codec, int chans, const GridParams &P, hipStream_t stream) {
  const Bc6hKernel *k = find_bc6h(codec, chans);
  if (!k) return hipErrorInvalidValue;
  return launch_tiled(k->wide, k->narrow, P, stream);
}

hipError_t launch_bc6h_decode(int codec, const DecodeParams &P, hipStream_t stream) {
  if (codec != ICAMD_BC6H_UF16 && codec != ICAMD_BC6H_SF16) return hipErrorInvalidValue;
  return launch_raster_decode(codec == ICAMD_BC6H_SF16 ? icamd_bc6h_sf16_decode_kernel : icamd_bc6h_uf16_decode_kernel, P, stream);
}

hipError_t launch_bc6h_metric(int codec, int chans, const MetricParams &P, hipStream_t stream) {
  const Bc6hKernel *k = find_bc6h(codec, chans);
  if (!k) return hipErrorInvalidValue;
  return launch_metric_walk(k->metric, P, stream);
}

}  // namespace icamd
