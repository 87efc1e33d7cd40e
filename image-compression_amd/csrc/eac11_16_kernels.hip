// eac11_16_kernels.hip -- 16-bit and signed EAC R11 / RG11 for gfx950 (EXTENSION, include/ic_amd.h
// icamd_encode_eac11_16_device): encode, decode and metric kernels; see eac11_16_block.h for the block math and DESIGN.md 3.20.
//
// Encode: one block per lane on the 16 x 16-block tiles of eac11_kernels.hip (a wave = 16 x 4 blocks = 64 x 16 pixels: the
// search's wave-uniform exit wants lanes with alike content), four-wave workgroups.  The search is 192 candidates per channel
// and the kernels are bound by instruction issue, so the fetch only has to be correct and simple: four row loads of 8 C bytes
// at a 64-bit lane address (any 2-byte alignment, any even row padding) where the block lies in the image, the clamp-to-edge
// gather otherwise.  RG11 runs both searches in ONE lane, R then G (G's sixteen samples wait in eight registers), and stores
// 16 bytes once.  One body, templated on the channel count, RG and signedness.
// Decode: the lane groups of lane_groups.h with 16 bytes of blocks per lane (K = 2 R11 blocks, or one RG11 block) and 16-byte
// row stores of 16-bit samples.
// Metric: the walk of metric_walk.inc (blocks in raster order of the images' own grids, four per lane) over Eac16Acc; sums are
// 64-bit from the lane on, lanes meet by wave shuffles and every wave adds its sums to the image's record.
#include "eac11_16_block.h"
#include "codec_info.h"
#include "ic_launch.h"
#include "lane_groups.h"
#include "ic_amd.h"

namespace icamd {

#include "metric_walk.inc"

namespace {
constexpr bool codec_rg(int codec) { return codec == ICAMD_EAC_RG11 || codec == ICAMD_EAC_SIGNED_RG11; }
constexpr bool codec_signed(int codec) { return codec == ICAMD_EAC_SIGNED_R11 || codec == ICAMD_EAC_SIGNED_RG11; }
}  // namespace

template <int C, bool RG, bool SIGNED>
__device__ __forceinline__ void eac11_16_encode_one(const GridParams &P) {
  const TileCoord t = locate_tile<false>(P);
  if (!t.valid) return;
  uint32_t r[8], g[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
  eac11_16_fetch<C, RG>(P.src + (uint64_t)t.img * P.src_image_stride, P.height, P.width, P.row_stride, t.brow * 4u, t.bcol * 4u,
                        r, g);
  const Out8 a = encode_eac11_16<SIGNED>(r);
  if (RG) {
    const Out8 b = encode_eac11_16<SIGNED>(g);
    store_stream16(tile_dst<16>(P, t), a.lo, a.hi, b.lo, b.hi);
  } else {
    store_stream8(tile_dst<8>(P, t), a.lo, a.hi);
  }
}

// 16 bytes of blocks per lane: two R11 words (TWO = false) or one RG11 pair; out[y] = the 16 bytes of pixel row y.
template <bool TWO, bool SIGNED>
__device__ __forceinline__ void eac11_16_decode(const Bc45DecodeParams &P) {
  constexpr uint32_t K = TWO ? 1u : 2u, BYTES = TWO ? 16u : 8u, C = TWO ? 2u : 1u;
  const LaneGroup g = locate_lane_group(P.log2_tile_cols, P.tile_row0, K, P.block_rows, P.block_cols);
  if (!g.valid) return;
  const uint8_t *src = P.blocks + (uint64_t)blockIdx.z * P.src_image_stride + ((uint64_t)g.brow * P.block_cols + g.bcol) * BYTES;
  uint8_t *dst = P.pixels + (uint64_t)blockIdx.z * P.dst_image_stride + (uint64_t)(g.brow * 4u) * P.row_stride +
                 (uint64_t)g.bcol * (8u * C);
  uint32_t w[4];
  if (g.bcol + K <= P.block_cols) {
    const U4 v = load_stream(reinterpret_cast<const U4 *>(src));
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {  // (R11 only: the row's last, single block)
    const U2 v = load_stream(reinterpret_cast<const U2 *>(src));
    w[0] = v.x; w[1] = v.y; w[2] = w[3] = 0u;
  }
  uint32_t a[4][2], b[4][2], out[4][4];
  decode_eac11_16<SIGNED>(w[0], w[1], a);
  decode_eac11_16<SIGNED>(w[2], w[3], b);
#pragma unroll
  for (int y = 0; y < 4; ++y) {
    if (TWO) {  // R0 G0 | R1 G1 | R2 G2 | R3 G3
      out[y][0] = perm(b[y][0], a[y][0], 0x05040100u); out[y][1] = perm(b[y][0], a[y][0], 0x07060302u);
      out[y][2] = perm(b[y][1], a[y][1], 0x05040100u); out[y][3] = perm(b[y][1], a[y][1], 0x07060302u);
    } else {
      out[y][0] = a[y][0]; out[y][1] = a[y][1]; out[y][2] = b[y][0]; out[y][3] = b[y][1];
    }
  }
  const uint32_t row = g.brow * 4u, col = g.bcol * 4u;
  if (row + 4u <= P.height && (uint64_t)col + 4u * K <= P.width) {
#pragma unroll
    for (int y = 0; y < 4; ++y) store_stream16(dst + (uint64_t)y * P.row_stride, out[y][0], out[y][1], out[y][2], out[y][3]);
  } else {  // clipped at the image's edge
    const uint32_t rows = umin(P.height - row, 4u), bytes = (uint32_t)umin(P.width - col, 4u * K) * (2u * C);
    for (uint32_t y = 0; y < rows; ++y)
      for (uint32_t i = 0; i < bytes; ++i) dst[(uint64_t)y * P.row_stride + i] = (uint8_t)(out[y][i >> 2] >> (8 * (i & 3u)));
  }
}

template <int C, bool RG, bool SIGNED>
__device__ __forceinline__ void eac11_16_metric(const MetricParams &P) {
  metric_walk<MetricWideOps<Eac16Acc, 2>>(P, [&](uint32_t img, uint32_t brow, uint32_t bcol, Eac16Acc &acc) {
    const uint8_t *b = P.blocks + (size_t)img * P.blocks_image_stride + ((size_t)brow * P.grid_cols + bcol) * (RG ? 16u : 8u);
    uint32_t w[4] = { 0u, 0u, 0u, 0u };
    if (RG) {
      const U4 v = load_stream(reinterpret_cast<const U4 *>(b));
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
      const U2 v = load_stream(reinterpret_cast<const U2 *>(b));
      w[0] = v.x; w[1] = v.y;
    }
    metric_eac11_16_block<C, RG, SIGNED>(w, P.src + (size_t)img * P.src_image_stride, P.height, P.width, P.row_stride, brow * 4u,
                                         bcol * 4u, acc);
  });
}

extern "C" {

#define ICAMD_EAC16_KERNELS(X)                                          \
  X(icamd_eac_r11_r16_kernel, ICAMD_EAC_R11, 1)                         \
  X(icamd_eac_r11_rg16_kernel, ICAMD_EAC_R11, 2)                        \
  X(icamd_eac_r11_rgb16_kernel, ICAMD_EAC_R11, 3)                       \
  X(icamd_eac_r11_rgba16_kernel, ICAMD_EAC_R11, 4)                      \
  X(icamd_eac_rg11_rg16_kernel, ICAMD_EAC_RG11, 2)                      \
  X(icamd_eac_rg11_rgb16_kernel, ICAMD_EAC_RG11, 3)                     \
  X(icamd_eac_rg11_rgba16_kernel, ICAMD_EAC_RG11, 4)                    \
  X(icamd_eac_signed_r11_r16_kernel, ICAMD_EAC_SIGNED_R11, 1)           \
  X(icamd_eac_signed_r11_rg16_kernel, ICAMD_EAC_SIGNED_R11, 2)          \
  X(icamd_eac_signed_r11_rgb16_kernel, ICAMD_EAC_SIGNED_R11, 3)         \
  X(icamd_eac_signed_r11_rgba16_kernel, ICAMD_EAC_SIGNED_R11, 4)        \
  X(icamd_eac_signed_rg11_rg16_kernel, ICAMD_EAC_SIGNED_RG11, 2)        \
  X(icamd_eac_signed_rg11_rgb16_kernel, ICAMD_EAC_SIGNED_RG11, 3)       \
  X(icamd_eac_signed_rg11_rgba16_kernel, ICAMD_EAC_SIGNED_RG11, 4)
#define ICAMD_EAC16_METRIC_KERNELS(X)                                          \
  X(icamd_metric_eac_r11_r16_kernel, ICAMD_EAC_R11, 1)                         \
  X(icamd_metric_eac_r11_rg16_kernel, ICAMD_EAC_R11, 2)                        \
  X(icamd_metric_eac_r11_rgb16_kernel, ICAMD_EAC_R11, 3)                       \
  X(icamd_metric_eac_r11_rgba16_kernel, ICAMD_EAC_R11, 4)                      \
  X(icamd_metric_eac_rg11_rg16_kernel, ICAMD_EAC_RG11, 2)                      \
  X(icamd_metric_eac_rg11_rgb16_kernel, ICAMD_EAC_RG11, 3)                     \
  X(icamd_metric_eac_rg11_rgba16_kernel, ICAMD_EAC_RG11, 4)                    \
  X(icamd_metric_eac_signed_r11_r16_kernel, ICAMD_EAC_SIGNED_R11, 1)           \
  X(icamd_metric_eac_signed_r11_rg16_kernel, ICAMD_EAC_SIGNED_R11, 2)          \
  X(icamd_metric_eac_signed_r11_rgb16_kernel, ICAMD_EAC_SIGNED_R11, 3)         \
  X(icamd_metric_eac_signed_r11_rgba16_kernel, ICAMD_EAC_SIGNED_R11, 4)        \
  X(icamd_metric_eac_signed_rg11_rg16_kernel, ICAMD_EAC_SIGNED_RG11, 2)        \
  X(icamd_metric_eac_signed_rg11_rgb16_kernel, ICAMD_EAC_SIGNED_RG11, 3)       \
  X(icamd_metric_eac_signed_rg11_rgba16_kernel, ICAMD_EAC_SIGNED_RG11, 4)

#define ICAMD_EAC16_ENCODE(name, codec, chans)                                    \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(GridParams P) {    \
    eac11_16_encode_one<chans, codec_rg(codec), codec_signed(codec)>(P);          \
  }
ICAMD_EAC16_KERNELS(ICAMD_EAC16_ENCODE)
#undef ICAMD_EAC16_ENCODE
#define ICAMD_EAC16_METRIC(name, codec, chans)                                    \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(MetricParams P) {  \
    eac11_16_metric<chans, codec_rg(codec), codec_signed(codec)>(P);              \
  }
ICAMD_EAC16_METRIC_KERNELS(ICAMD_EAC16_METRIC)
#undef ICAMD_EAC16_METRIC

__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_eac_r11_decode16_kernel(Bc45DecodeParams P) {
  eac11_16_decode<false, false>(P);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_eac_rg11_decode16_kernel(Bc45DecodeParams P) {
  eac11_16_decode<true, false>(P);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_eac_signed_r11_decode16_kernel(Bc45DecodeParams P) {
  eac11_16_decode<false, true>(P);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_eac_signed_rg11_decode16_kernel(Bc45DecodeParams P) {
  eac11_16_decode<true, true>(P);
}

}  // extern "C"

namespace {
struct Eac16Kernel {
  int codec, chans;
  void (*fn)(GridParams);
  const char *name;
};
struct Eac16MetricKernel {
  int codec, chans;
  void (*fn)(MetricParams);
  const char *name;
};
#define ICAMD_EAC16_ENTRY(fn, codec, chans) { codec, chans, fn, #fn },
const Eac16Kernel kEac16Kernels[] = { ICAMD_EAC16_KERNELS(ICAMD_EAC16_ENTRY) };
const Eac16MetricKernel kEac16MetricKernels[] = { ICAMD_EAC16_METRIC_KERNELS(ICAMD_EAC16_ENTRY) };
#undef ICAMD_EAC16_ENTRY
template <typename K, size_t N>
const K *find_eac16(const K (&list)[N], int codec, int chans) {
  for (const K &k : list)
    if (k.codec == codec && k.chans == chans) return &k;
  return nullptr;
}
}  // namespace
#undef ICAMD_EAC16_KERNELS
#undef ICAMD_EAC16_METRIC_KERNELS

const char *eac11_16_kernel_name(int codec, int chans) {
  const Eac16Kernel *k = find_eac16(kEac16Kernels, codec, chans);
  return k ? k->name : "";
}
const char *eac11_16_metric_kernel_name(int codec, int chans) {
  const Eac16MetricKernel *k = find_eac16(kEac16MetricKernels, codec, chans);
  return k ? k->name : "";
}

hipError_t launch_eac11_16_encode(int codec, int chans, const GridParams &P, hipStream_t stream) {
  const Eac16Kernel *k = find_eac16(kEac16Kernels, codec, chans);
  if (!k) return hipErrorInvalidValue;
  return launch_tiled(k->fn, k->fn, P, stream, 4u);
}

hipError_t launch_eac11_16_decode(int codec, uint32_t n_images, const Bc45DecodeParams &P, hipStream_t stream) {
  void (*fn)(Bc45DecodeParams);
  switch (codec) {
    case ICAMD_EAC_R11: fn = icamd_eac_r11_decode16_kernel; break;
    case ICAMD_EAC_RG11: fn = icamd_eac_rg11_decode16_kernel; break;
    case ICAMD_EAC_SIGNED_R11: fn = icamd_eac_signed_r11_decode16_kernel; break;
    case ICAMD_EAC_SIGNED_RG11: fn = icamd_eac_signed_rg11_decode16_kernel; break;
    default: return hipErrorInvalidValue;
  }
  const uint32_t K = codec_rg(codec) ? 1u : 2u;
  const uint32_t groups = (uint32_t)(((uint64_t)P.block_cols + K - 1u) / K);
  return launch_lane_groups(fn, P, n_images, groups, stream, &Bc45DecodeParams::blocks, P.src_image_stride,
                            &Bc45DecodeParams::pixels, P.dst_image_stride);
}

hipError_t launch_eac11_16_metric(int codec, int chans, const MetricParams &P, hipStream_t stream) {
  const Eac16MetricKernel *k = find_eac16(kEac16MetricKernels, codec, chans);
  if (!k) return hipErrorInvalidValue;
  return launch_metric_walk(k->fn, P, stream);
}

}  // namespace icamd
