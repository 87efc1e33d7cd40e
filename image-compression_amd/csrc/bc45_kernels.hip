// bc45_kernels.hip -- BC4 / BC5 (RGTC) encode and decode kernels for gfx950 (extension, include/ic_amd.h ICAMD_BC4).
//
// A lane owns K horizontally adjacent blocks of one block row (the lane groups of lane_groups.h).  K is chosen so that a lane's row access is 16 bytes and its block store at least 16 bytes:
//   BC4 <- R8: K = 4 (a block row is one dword; 16-byte row loads, 32-byte stores)
//   BC4 / BC5 <- RG8: K = 2 (16-byte row loads, 16 / 32-byte stores)
//   BC4 / BC5 <- RGB888 / RGBA8: K = 1 (the DXT loads: 12 / 16 bytes per row), the DXT5 alpha search on bytes 0 / 1 / 2
//   decoders: K = 4 (BC4 -> R8) and 2 (BC5 -> RG8): 32-byte block loads, 16-byte row stores, so that a wave's store
//   instruction writes 1 KiB of one pixel row (whole lines), not 64 partial segments of 4 bytes.
// Addresses are 64-bit per lane (a lane's K blocks amortise them); any geometry that fits the C ABI runs.
#include "bc45_block.h"
#include "codec_info.h"
#include "ic_launch.h"
#include "lane_groups.h"
#include "ic_amd.h"

namespace icamd {

template <int COMPS>
constexpr uint32_t bc45_encode_lane_blocks() { return COMPS == 1 ? 4u : COMPS == 2 ? 2u : 1u; }

// One channel (byte `ch` of each COMPS-byte pixel) of the block at pixel (row, col), clamped to the image (edge replication,
// pixel4x4.cc:23-59): the reference's gather, byte by byte.
template <int COMPS>
__device__ __forceinline__ void gather_channel_rows(const uint8_t *img, const GridParams &P, uint32_t row, uint32_t col,
                                                    uint32_t ch, uint32_t r[4]) {
#pragma unroll
  for (int y = 0; y < 4; ++y) {
    const uint8_t *line = img + (uint64_t)umin(row + (uint32_t)y, P.height - 1u) * P.row_stride + ch;
    uint32_t v = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) v |= (uint32_t)line[(uint64_t)umin(col + (uint32_t)x, P.width - 1u) * COMPS] << (8 * x);
    r[y] = v;
  }
}

template <int BYTES>
__device__ __forceinline__ void store_block(uint8_t *p, const Out8 &a, const Out8 &b) {
  if (BYTES == 16) store_stream16(p, a.lo, a.hi, b.lo, b.hi);
  else store_stream8(p, a.lo, a.hi);
}

// BC4 (BC5 = false) or BC5 of a COMPS-byte source; rch = byte of R (0, or 2 for a swapped 3 / 4-byte source), G = byte 1.
template <int COMPS, bool BC5>
__device__ __forceinline__ void bc45_encode(const GridParams &P) {
  constexpr uint32_t K = bc45_encode_lane_blocks<COMPS>();
  constexpr int BYTES = BC5 ? 16 : 8;
  const LaneGroup g = locate_lane_group(P.log2_tile_cols, P.tile_row0, K, P.block_rows, P.block_cols);
  if (!g.valid) return;
  const uint8_t *img = P.src + (uint64_t)blockIdx.z * P.src_image_stride;
  uint8_t *out = P.dst + (uint64_t)blockIdx.z * P.dst_image_stride + ((uint64_t)g.brow * P.block_cols + g.bcol) * BYTES;
  const uint32_t row = g.brow * 4u;
  const bool full = g.bcol + K <= P.block_cols;  // all K blocks exist: one wide store
  Out8 a[K], b[K];
  if (COMPS <= 2) {
    const bool interior = (uint64_t)(g.bcol + K) * 4u <= P.width && row + 4u <= P.height;
    uint32_t rows[4][4];  // rows[y] = the 16 source bytes of pixel row y of the lane's K blocks
    if (interior) {
      const uint8_t *p = img + (uint64_t)row * P.row_stride + (uint64_t)g.bcol * (4u * COMPS);
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const U4 v = load_stream(reinterpret_cast<const U4 *>(p + (uint64_t)y * P.row_stride));
        rows[y][0] = v.x; rows[y][1] = v.y; rows[y][2] = v.z; rows[y][3] = v.w;
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
      const uint32_t bcol = g.bcol + k;
      if (!full && bcol >= P.block_cols) break;
      const bool one_pixel = bcol * 4u >= P.width && row >= P.height;
      uint32_t r[4], gr[4];
      if (interior) {
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          if (COMPS == 1) {
            r[y] = rows[y][k];
          } else {
            r[y] = rg_row_r(rows[y][2 * k], rows[y][2 * k + 1]);
            gr[y] = rg_row_g(rows[y][2 * k], rows[y][2 * k + 1]);
          }
        }
      } else {
        gather_channel_rows<COMPS>(img, P, row, bcol * 4u, 0u, r);
        if (BC5) gather_channel_rows<COMPS>(img, P, row, bcol * 4u, 1u, gr);
      }
      a[k] = encode_bc4_rows(r, one_pixel);
      if (BC5) b[k] = encode_bc4_rows(gr, one_pixel);
    }
  } else {
    // the DXT5 loads and the DXT5 alpha search on byte 0 / 2 (R) and byte 1 (G); rows of more than a third of 4 GiB take the
    // byte gather (load_block's wide path steps rows with 32-bit offsets)
    uint32_t px[16];
    load_block<COMPS>(img, P.height, P.width, P.row_stride, row, g.bcol * 4u, px, (uint64_t)P.row_stride * 3u + 16u < (1ull << 32));
    const bool one_pixel = g.bcol * 4u >= P.width && row >= P.height;
    a[0] = P.swap_rb ? encode_dxt5_alpha_block<2>(px, one_pixel) : encode_dxt5_alpha_block<0>(px, one_pixel);
    if (BC5) b[0] = encode_dxt5_alpha_block<1>(px, one_pixel);
  }
  if (full && K * BYTES == 32) {
    if (BC5) {
      store_stream16(out, a[0].lo, a[0].hi, b[0].lo, b[0].hi);
      store_stream16(out + 16, a[1 % K].lo, a[1 % K].hi, b[1 % K].lo, b[1 % K].hi);
    } else {
      store_stream16(out, a[0].lo, a[0].hi, a[1 % K].lo, a[1 % K].hi);
      store_stream16(out + 16, a[2 % K].lo, a[2 % K].hi, a[3 % K].lo, a[3 % K].hi);
    }
  } else if (full && K * BYTES == 16 && !BC5) {
    store_stream16(out, a[0].lo, a[0].hi, a[1 % K].lo, a[1 % K].hi);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < K; ++k)
      if (g.bcol + k < P.block_cols) store_block<BYTES>(out + k * BYTES, a[k], b[k]);
  }
}

// Decoders: the shared lane-group decoder (lane_groups.h) over decode_bc4_rows.
struct Bc4Rows {
  __device__ __forceinline__ void operator()(uint32_t w0, uint32_t w1, uint32_t rows[4]) const { decode_bc4_rows(w0, w1, rows); }
};
template <bool BC5>
__device__ __forceinline__ void bc45_decode(const Bc45DecodeParams &P) { plane_decode<BC5>(P, Bc4Rows()); }

extern "C" {
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc4_r8_kernel(GridParams P) { bc45_encode<1, false>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc4_rg8_kernel(GridParams P) { bc45_encode<2, false>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc4_rgb888_kernel(GridParams P) { bc45_encode<3, false>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc4_rgba8_kernel(GridParams P) { bc45_encode<4, false>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc5_rg8_kernel(GridParams P) { bc45_encode<2, true>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc5_rgb888_kernel(GridParams P) { bc45_encode<3, true>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc5_rgba8_kernel(GridParams P) { bc45_encode<4, true>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc4_decode_kernel(Bc45DecodeParams P) { bc45_decode<false>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc5_decode_kernel(Bc45DecodeParams P) { bc45_decode<true>(P); }
}  // extern "C"

const char *bc45_kernel_name(int codec, int comps) {
  if (codec == ICAMD_BC4) {
    switch (comps) {
      case 1: return "icamd_bc4_r8_kernel";
      case 2: return "icamd_bc4_rg8_kernel";
      case 3: return "icamd_bc4_rgb888_kernel";
      case 4: return "icamd_bc4_rgba8_kernel";
    }
  } else if (codec == ICAMD_BC5) {
    switch (comps) {
      case 2: return "icamd_bc5_rg8_kernel";
      case 3: return "icamd_bc5_rgb888_kernel";
      case 4: return "icamd_bc5_rgba8_kernel";
    }
  }
  return "";
}

hipError_t launch_bc45_encode(int codec, int comps, const GridParams &P, hipStream_t stream) {
  void (*k)(GridParams) = nullptr;
  if (codec == ICAMD_BC4)
    k = comps == 1 ? icamd_bc4_r8_kernel : comps == 2 ? icamd_bc4_rg8_kernel : comps == 3 ? icamd_bc4_rgb888_kernel
      : comps == 4 ? icamd_bc4_rgba8_kernel : nullptr;
  else if (codec == ICAMD_BC5)
    k = comps == 2 ? icamd_bc5_rg8_kernel : comps == 3 ? icamd_bc5_rgb888_kernel : comps == 4 ? icamd_bc5_rgba8_kernel : nullptr;
  if (!k) return hipErrorInvalidValue;
  const uint32_t K = comps == 1 ? 4u : comps == 2 ? 2u : 1u;
  const uint32_t groups = (uint32_t)(((uint64_t)P.block_cols + K - 1u) / K);
  // GridParams::src is const uint8_t *, dst uint8_t *
  return launch_lane_groups(k, P, P.n_images, groups, stream, &GridParams::src, P.src_image_stride, &GridParams::dst,
                            P.dst_image_stride);
}

hipError_t launch_bc45_decode(int codec, uint32_t n_images, const Bc45DecodeParams &P, hipStream_t stream) {
  if (codec != ICAMD_BC4 && codec != ICAMD_BC5) return hipErrorInvalidValue;
  const uint32_t K = codec == ICAMD_BC5 ? 2u : 4u;
  const uint32_t groups = (uint32_t)(((uint64_t)P.block_cols + K - 1u) / K);
  return launch_lane_groups(codec == ICAMD_BC5 ? icamd_bc5_decode_kernel : icamd_bc4_decode_kernel, P, n_images, groups, stream,
                            &Bc45DecodeParams::blocks, P.src_image_stride, &Bc45DecodeParams::pixels, P.dst_image_stride);
}

}  // namespace icamd
