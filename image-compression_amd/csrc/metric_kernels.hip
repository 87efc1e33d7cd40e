// metric_kernels.hip -- icamd_measure_error_device for gfx950: the error of compressed blocks against their source pixels,
// per image and channel (sum of squared differences, largest absolute difference), without a decoded image in memory.
// A lane takes a block as in the decoders: load the block words and the block's source pixels, decode in registers
// (metric_block.h: the decoders' own math), accumulate in the lane; lanes meet by wave shuffles, waves through LDS, and a
// workgroup adds one 64-bit sum and one 32-bit maximum per compared channel to the image's record.  Which blocks a lane takes
// and who commits when is the walk of metric_walk.inc, shared with eac11_16_kernels.hip and bc6h_kernels.hip.
#include "metric_block.h"
#include "codec_info.h"
#include "ic_launch.h"
#include "ic_amd.h"
#include "pvrtc_decode_tile.h"

namespace icamd {

#include "metric_walk.inc"

constexpr uint32_t kMetricWaves = kThreadsPerWorkgroup / 64;

__device__ __forceinline__ void metric_wave_reduce(MetricAcc &a) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.sse[k] += (uint32_t)__shfl_xor((int)a.sse[k], off);
    a.mx_rb = pk_max_u16(a.mx_rb, (uint32_t)__shfl_xor((int)a.mx_rb, off));
    a.mx_ga = pk_max_u16(a.mx_ga, (uint32_t)__shfl_xor((int)a.mx_ga, off));
  }
}

// Adds one contribution to image `img`'s record (vector atomics; zero contributions are skipped).
__device__ __forceinline__ void metric_commit(const MetricParams &P, uint32_t img, const MetricAcc &a) {
  icamd_error_stats *rec = reinterpret_cast<icamd_error_stats *>(P.stats) + img;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (a.sse[k]) atomicAdd(reinterpret_cast<unsigned long long *>(&rec->sse[k]), (unsigned long long)a.sse[k]);
    const uint32_t m = metric_max(a, k);
    if (m) atomicMax(&rec->max_abs[k], m);
  }
}

// MetricAcc (packed 32-bit sums of 4 channels) for the walk of metric_walk.inc
struct MetricPackedOps {
  using Acc = MetricAcc;
  static __device__ __forceinline__ void clear(MetricAcc &a) { metric_clear(a); }
  static __device__ __forceinline__ void wave_reduce(MetricAcc &a) { metric_wave_reduce(a); }
  static __device__ __forceinline__ void commit(const MetricParams &P, uint32_t img, const MetricAcc &a) { metric_commit(P, img, a); }
};

// The whole workgroup holds blocks of image `img` (uniform): one commit.  Contains a barrier.
__device__ __forceinline__ void metric_flush_workgroup(const MetricParams &P, uint32_t img, MetricAcc &a,
                                                       uint32_t (*part)[6]) {
  metric_wave_reduce(a);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int k = 0; k < 4; ++k) part[wave][k] = a.sse[k];
    part[wave][4] = a.mx_rb;
    part[wave][5] = a.mx_ga;
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    MetricAcc t;
    metric_clear(t);
#pragma unroll
    for (uint32_t w = 0; w < kMetricWaves; ++w) {
#pragma unroll
      for (int k = 0; k < 4; ++k) t.sse[k] += part[w][k];
      t.mx_rb = pk_max_u16(t.mx_rb, part[w][4]);
      t.mx_ga = pk_max_u16(t.mx_ga, part[w][5]);
    }
    metric_commit(P, img, t);
  }
}

// The walk of metric_walk.inc; a workgroup whose blocks lie in one image commits once, through LDS.
template <typename One>
__device__ __forceinline__ void metric_raster(const MetricParams &P, uint32_t (*part)[6], One one) {
  metric_walk<MetricPackedOps>(P, one, [&](uint32_t img, MetricAcc &acc) { metric_flush_workgroup(P, img, acc, part); });
}

template <int CODEC, int COMPS>
__device__ __forceinline__ void metric_block_codec(const MetricParams &P, uint32_t (*part)[6]) {
  metric_raster(P, part, [&](uint32_t img, uint32_t brow, uint32_t bcol, MetricAcc &acc) {
    const uint8_t *b = P.blocks + (size_t)img * P.blocks_image_stride +
                       ((size_t)brow * P.grid_cols + bcol) * codec_block_bytes(CODEC);
    const uint8_t *src = P.src + (size_t)img * P.src_image_stride;
    uint32_t w[4] = { 0, 0, 0, 0 };
    if (codec_block_bytes(CODEC) == 16) {
      const U4 v = load_stream(reinterpret_cast<const U4 *>(b));  // no alignment assumed: the caller owns the block pointer
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
      const U2 v = load_stream(reinterpret_cast<const U2 *>(b));
      w[0] = v.x; w[1] = v.y;
    }
    const bool wide_ok = P.force_gather == 0u;
    if constexpr (CODEC == ICAMD_ETC2_RGBA8)
      metric_etc2_block(w, P.swap_rb != 0u, src, P.height, P.width, P.row_stride, brow * 4u, bcol * 4u, wide_ok, acc);
    else if constexpr (CODEC == ICAMD_ETC2_RGB8)
      metric_etc2_rgb8_block<COMPS>(w, src, P.height, P.width, P.row_stride, brow * 4u, bcol * 4u, wide_ok, acc);
    else if constexpr (CODEC == ICAMD_ETC2_RGB8A1)
      metric_etc2_a1_block(w, P.swap_rb != 0u, src, P.height, P.width, P.row_stride, brow * 4u, bcol * 4u, wide_ok, acc);
    else if constexpr (CODEC == ICAMD_BC4 || CODEC == ICAMD_BC5)
      metric_bc45_block<COMPS, CODEC == ICAMD_BC5>(w, P.swap_rb != 0u, src, P.height, P.width, P.row_stride, brow * 4u, bcol * 4u,
                                                   wide_ok, acc);
    else if constexpr (CODEC == ICAMD_EAC_R11 || CODEC == ICAMD_EAC_RG11)
      metric_bc45_block<COMPS, CODEC == ICAMD_EAC_RG11, true>(w, P.swap_rb != 0u, src, P.height, P.width, P.row_stride, brow * 4u,
                                                              bcol * 4u, wide_ok, acc);
    else if constexpr (CODEC == ICAMD_BC1A || CODEC == ICAMD_BC2)
      metric_bc1a_bc2_block<CODEC == ICAMD_BC2>(w, P.swap_rb != 0u, src, P.height, P.width, P.row_stride, brow * 4u, bcol * 4u,
                                                wide_ok, acc);
    else if constexpr (CODEC == ICAMD_BC7)
      metric_bc7_block<COMPS>(w, P.swap_rb != 0u, src, P.height, P.width, P.row_stride, brow * 4u, bcol * 4u, wide_ok, acc);
    else
      metric_color_block<CODEC, COMPS>(w, P.swap_rb != 0u, src, P.height, P.width, P.row_stride, brow * 4u, bcol * 4u, wide_ok,
                                       acc);
  });
}

// The sink of the PVRTC decoders' pixel rows: row y of the block whose first source pixel is at `src`.
template <int BPP>
struct PvrtcMetricSink {
  const uint8_t *src;
  size_t row_stride;
  MetricAcc &acc;
  __device__ __forceinline__ void operator()(int, const uint32_t *row) {
    const U4 s0 = load_stream(reinterpret_cast<const U4 *>(src));
    const uint32_t a[4] = { s0.x, s0.y, s0.z, s0.w };
    metric_row4<4>(a, row, acc);
    if (BPP == 2) {
      const U4 s1 = load_stream(reinterpret_cast<const U4 *>(src + 16));
      const uint32_t b[4] = { s1.x, s1.y, s1.z, s1.w };
      metric_row4<4>(b, row + 4, acc);
    }
    src += row_stride;
  }
};

// PVRTC1 2 bpp / 4 bpp, small textures (block grids below 32 x 8): the nine block words from their Z-order slots.
template <int BPP>
__device__ __forceinline__ void metric_pvrtc_generic(const MetricParams &P, uint32_t (*part)[6]) {
  metric_raster(P, part, [&](uint32_t img, uint32_t by, uint32_t bx, MetricAcc &acc) {
    const U2 *blocks = reinterpret_cast<const U2 *>(P.blocks + (size_t)img * P.blocks_image_stride);
    uint32_t mod[9], col[9];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const uint32_t nx = (bx + (uint32_t)dx) & (P.block_cols - 1u), ny = (by + (uint32_t)dy) & (P.block_rows - 1u);
        const U2 w = blocks[spread_bits16(nx) << 1 | spread_bits16(ny)];
        mod[3 * (dy + 1) + dx + 1] = w.x;
        col[3 * (dy + 1) + dx + 1] = w.y;
      }
    uint32_t C[3][3][4];
#pragma unroll
    for (int i = 0; i < 9; ++i) pvrtc_expand_colors(col[i], C[i / 3][i % 3]);
    PvrtcMetricSink<BPP> sink = { P.src + (size_t)img * P.src_image_stride + (size_t)(by * 4u) * P.row_stride +
                                      (size_t)bx * (BPP == 2 ? 32u : 16u),
                                  P.row_stride, acc };
    if (BPP == 2) decode_pvrtc2_block_rows(C, mod, col, sink);
    else decode_pvrtc4_block_rows(C, mod[4], (col[4] & 1u) != 0u, sink);
  });
}

// Block grids of at least 32 x 8: one workgroup per tile (pvrtc_decode_tile.h), which lies in one image.
template <int BPP>
__device__ __forceinline__ void metric_pvrtc_tile(const MetricParams &P, U4 *pairs, uint32_t (*part)[6]) {
  PvrtcTileLane L;
  pvrtc_tile_neighbourhood<BPP>(P.blocks, P.blocks_image_stride, P.block_cols, P.block_rows, pairs, L);
  MetricAcc acc;
  metric_clear(acc);
  PvrtcMetricSink<BPP> sink = { P.src + (size_t)L.img * P.src_image_stride + (size_t)(L.by * 4u) * P.row_stride +
                                    (size_t)L.bx * (BPP == 2 ? 32u : 16u),
                                P.row_stride, acc };
  if (BPP == 2) decode_pvrtc2_block_rows(L.C, L.mod, L.col, sink);
  else decode_pvrtc4_block_rows(L.C, L.own.x, (L.own.y & 1u) != 0u, sink);
  metric_flush_workgroup(P, L.img, acc, part);
}

// The records are cleared by a kernel of the call's own (a launch like the others: stream-ordered, and a node of a captured
// graph that replays with it).
extern "C" __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_metric_clear_kernel(uint32_t *words, uint64_t n_words) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (i < n_words) words[i] = 0u;
}

#define ICAMD_METRIC_KERNEL(name, CODEC, COMPS)                                        \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(MetricParams P) {       \
    __shared__ uint32_t part[kMetricWaves][6];                                         \
    metric_block_codec<CODEC, COMPS>(P, part);                                         \
  }

extern "C" {
ICAMD_METRIC_KERNEL(icamd_metric_dxt1_rgb888_kernel, ICAMD_DXT1, 3)
ICAMD_METRIC_KERNEL(icamd_metric_dxt1_rgba8_kernel, ICAMD_DXT1, 4)
ICAMD_METRIC_KERNEL(icamd_metric_dxt5_rgba8_kernel, ICAMD_DXT5, 4)
ICAMD_METRIC_KERNEL(icamd_metric_etc1_rgb888_kernel, ICAMD_ETC1, 3)
ICAMD_METRIC_KERNEL(icamd_metric_etc1_rgba8_kernel, ICAMD_ETC1, 4)
ICAMD_METRIC_KERNEL(icamd_metric_etc2_rgba8_kernel, ICAMD_ETC2_RGBA8, 4)
ICAMD_METRIC_KERNEL(icamd_metric_etc2_rgb8_rgb888_kernel, ICAMD_ETC2_RGB8, 3)
ICAMD_METRIC_KERNEL(icamd_metric_etc2_rgb8_rgba8_kernel, ICAMD_ETC2_RGB8, 4)
ICAMD_METRIC_KERNEL(icamd_metric_etc2_rgb8a1_kernel, ICAMD_ETC2_RGB8A1, 4)
ICAMD_METRIC_KERNEL(icamd_metric_bc4_r8_kernel, ICAMD_BC4, 1)
ICAMD_METRIC_KERNEL(icamd_metric_bc4_rg8_kernel, ICAMD_BC4, 2)
ICAMD_METRIC_KERNEL(icamd_metric_bc4_rgb888_kernel, ICAMD_BC4, 3)
ICAMD_METRIC_KERNEL(icamd_metric_bc4_rgba8_kernel, ICAMD_BC4, 4)
ICAMD_METRIC_KERNEL(icamd_metric_bc5_rg8_kernel, ICAMD_BC5, 2)
ICAMD_METRIC_KERNEL(icamd_metric_bc5_rgb888_kernel, ICAMD_BC5, 3)
ICAMD_METRIC_KERNEL(icamd_metric_bc5_rgba8_kernel, ICAMD_BC5, 4)
ICAMD_METRIC_KERNEL(icamd_metric_eac_r11_r8_kernel, ICAMD_EAC_R11, 1)
ICAMD_METRIC_KERNEL(icamd_metric_eac_r11_rg8_kernel, ICAMD_EAC_R11, 2)
ICAMD_METRIC_KERNEL(icamd_metric_eac_r11_rgb888_kernel, ICAMD_EAC_R11, 3)
ICAMD_METRIC_KERNEL(icamd_metric_eac_r11_rgba8_kernel, ICAMD_EAC_R11, 4)
ICAMD_METRIC_KERNEL(icamd_metric_eac_rg11_rg8_kernel, ICAMD_EAC_RG11, 2)
ICAMD_METRIC_KERNEL(icamd_metric_eac_rg11_rgb888_kernel, ICAMD_EAC_RG11, 3)
ICAMD_METRIC_KERNEL(icamd_metric_eac_rg11_rgba8_kernel, ICAMD_EAC_RG11, 4)
ICAMD_METRIC_KERNEL(icamd_metric_bc7_rgb888_kernel, ICAMD_BC7, 3)
ICAMD_METRIC_KERNEL(icamd_metric_bc7_rgba8_kernel, ICAMD_BC7, 4)
ICAMD_METRIC_KERNEL(icamd_metric_bc1a_rgba8_kernel, ICAMD_BC1A, 4)
ICAMD_METRIC_KERNEL(icamd_metric_bc2_rgba8_kernel, ICAMD_BC2, 4)
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_metric_pvrtc2_kernel(MetricParams P) {
  __shared__ uint32_t part[kMetricWaves][6];
  metric_pvrtc_generic<2>(P, part);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_metric_pvrtc4_kernel(MetricParams P) {
  __shared__ uint32_t part[kMetricWaves][6];
  metric_pvrtc_generic<4>(P, part);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_metric_pvrtc2_tile_kernel(MetricParams P) {
  __shared__ U4 pairs[kPvrtcTilePairs];
  __shared__ uint32_t part[kMetricWaves][6];
  metric_pvrtc_tile<2>(P, pairs, part);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_metric_pvrtc4_tile_kernel(MetricParams P) {
  __shared__ U4 pairs[kPvrtcTilePairs];
  __shared__ uint32_t part[kMetricWaves][6];
  metric_pvrtc_tile<4>(P, pairs, part);
}
}  // extern "C"
#undef ICAMD_METRIC_KERNEL

namespace {
struct MetricKernel {
  int codec, comps;
  void (*fn)(MetricParams);
  const char *name;
};
#define ICAMD_METRIC_ENTRY(codec, comps, fn) { codec, comps, fn, #fn }
const MetricKernel kMetricKernels[] = {
  ICAMD_METRIC_ENTRY(ICAMD_DXT1, 3, icamd_metric_dxt1_rgb888_kernel), ICAMD_METRIC_ENTRY(ICAMD_DXT1, 4, icamd_metric_dxt1_rgba8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_DXT5, 4, icamd_metric_dxt5_rgba8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_ETC1, 3, icamd_metric_etc1_rgb888_kernel), ICAMD_METRIC_ENTRY(ICAMD_ETC1, 4, icamd_metric_etc1_rgba8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_ETC2_RGBA8, 4, icamd_metric_etc2_rgba8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_ETC2_RGB8, 3, icamd_metric_etc2_rgb8_rgb888_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_ETC2_RGB8, 4, icamd_metric_etc2_rgb8_rgba8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_ETC2_RGB8A1, 4, icamd_metric_etc2_rgb8a1_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_BC4, 1, icamd_metric_bc4_r8_kernel), ICAMD_METRIC_ENTRY(ICAMD_BC4, 2, icamd_metric_bc4_rg8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_BC4, 3, icamd_metric_bc4_rgb888_kernel), ICAMD_METRIC_ENTRY(ICAMD_BC4, 4, icamd_metric_bc4_rgba8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_BC5, 2, icamd_metric_bc5_rg8_kernel), ICAMD_METRIC_ENTRY(ICAMD_BC5, 3, icamd_metric_bc5_rgb888_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_BC5, 4, icamd_metric_bc5_rgba8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_EAC_R11, 1, icamd_metric_eac_r11_r8_kernel), ICAMD_METRIC_ENTRY(ICAMD_EAC_R11, 2, icamd_metric_eac_r11_rg8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_EAC_R11, 3, icamd_metric_eac_r11_rgb888_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_EAC_R11, 4, icamd_metric_eac_r11_rgba8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_EAC_RG11, 2, icamd_metric_eac_rg11_rg8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_EAC_RG11, 3, icamd_metric_eac_rg11_rgb888_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_EAC_RG11, 4, icamd_metric_eac_rg11_rgba8_kernel),
  ICAMD_METRIC_ENTRY(ICAMD_BC7, 3, icamd_metric_bc7_rgb888_kernel), ICAMD_METRIC_ENTRY(ICAMD_BC7, 4, icamd_metric_bc7_rgba8_kernel),
  // BC1A / BC2, written out: tests/test_walk_cases_host.py holds the ICAMD_METRIC_ENTRY rows to the families of tests/walk_cases.py,
  // which end with BC7; the walk shapes of these two rows are run by tests/test_gpu_bc1a_bc2.py
  { ICAMD_BC1A, 4, icamd_metric_bc1a_rgba8_kernel, "icamd_metric_bc1a_rgba8_kernel" },
  { ICAMD_BC2, 4, icamd_metric_bc2_rgba8_kernel, "icamd_metric_bc2_rgba8_kernel" },
  // the tile forms (block grids of at least 32 x 8) are the ones named; small textures take the raster forms
  ICAMD_METRIC_ENTRY(ICAMD_PVRTC2, 4, icamd_metric_pvrtc2_tile_kernel), ICAMD_METRIC_ENTRY(ICAMD_PVRTC4, 4, icamd_metric_pvrtc4_tile_kernel),
};
#undef ICAMD_METRIC_ENTRY
const MetricKernel *find_metric_kernel(int codec, int comps) {
  for (const MetricKernel &k : kMetricKernels)
    if (k.codec == codec && k.comps == comps) return &k;
  return nullptr;
}
}  // namespace

const char *metric_kernel_name(int codec, int comps) {
  const MetricKernel *k = find_metric_kernel(codec, comps);
  return k ? k->name : "";
}

hipError_t launch_metric_clear(void *stats, uint64_t n_images, hipStream_t stream) {
  if (n_images == 0) return hipSuccess;
  (void)hipGetLastError();
  const uint64_t n_words = n_images * (sizeof(icamd_error_stats) / 4u);
  hipLaunchKernelGGL(icamd_metric_clear_kernel, dim3((uint32_t)((n_words + kThreadsPerWorkgroup - 1u) / kThreadsPerWorkgroup)),
                     dim3(kThreadsPerWorkgroup), 0, stream, static_cast<uint32_t *>(stats), n_words);
  return hipGetLastError();
}

hipError_t launch_metric(int codec, int comps, const MetricParams &P, hipStream_t stream) {
  if (P.total_blocks == 0) return hipSuccess;
  const MetricKernel *k = find_metric_kernel(codec, comps);
  if (!k) return hipErrorInvalidValue;
  if (codec == ICAMD_PVRTC2 || codec == ICAMD_PVRTC4) {
    const bool tiles = P.block_cols >= kPvrtcTileW && P.block_rows >= kPvrtcTileH;  // (powers of two: the caller checked)
    if (!tiles) return launch_metric_walk(codec == ICAMD_PVRTC2 ? icamd_metric_pvrtc2_kernel : icamd_metric_pvrtc4_kernel, P, stream);
    (void)hipGetLastError();  // a stale error of another library on this thread is not this launch's
    // whole tiles: total_blocks / 256 workgroups
    hipLaunchKernelGGL(k->fn, dim3(P.total_blocks / kThreadsPerWorkgroup), dim3(kThreadsPerWorkgroup), 0, stream, P);
    return hipGetLastError();
  }
  return launch_metric_walk(k->fn, P, stream);
}

}  // namespace icamd
