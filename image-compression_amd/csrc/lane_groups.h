// lane_groups.h -- the lane-group launch shape of the one- and two-channel codecs (BC4 / BC5: bc45_kernels.hip, EAC R11 / RG11:
// eac11_kernels.hip) and the decoder both families share.
//
// A lane owns K horizontally adjacent blocks of one block row, 256 lanes per workgroup, one workgroup per tile of
// 2^log2_tile_cols lane groups x (256 >> log2_tile_cols) block rows (the tile shapes of launch_tiled, ic_launch.h), images in
// grid.z.  Addresses are 64-bit per lane (a lane's K blocks amortise them); any geometry that fits the C ABI runs.
#ifndef ICAMD_LANE_GROUPS_H_
#define ICAMD_LANE_GROUPS_H_

#include "bc45_block.h"  // interleave_rg_row
#include "ic_launch.h"

namespace icamd {

struct LaneGroup {
  uint32_t brow, bcol;  // first block of the lane's K
  bool valid;
};
__device__ __forceinline__ LaneGroup locate_lane_group(uint32_t log2_tile_cols, uint32_t tile_row0, uint32_t K,
                                                       uint32_t block_rows, uint32_t block_cols) {
  LaneGroup g;
  const uint32_t lx = threadIdx.x & ((1u << log2_tile_cols) - 1u), ly = threadIdx.x >> log2_tile_cols;
  g.bcol = ((blockIdx.x << log2_tile_cols) + lx) * K;
  g.brow = (blockIdx.y + tile_row0) * (256u >> log2_tile_cols) + ly;
  g.valid = g.bcol < block_cols && g.brow < block_rows;
  return g;
}

// Decoder of 8-byte one-channel words to R8 rows (TWO = false, K = 4 blocks per lane) or of 16-byte word pairs to RG8 rows
// (TWO = true, K = 2): 32-byte block loads, 16-byte row stores, so that a wave's store instruction writes 1 KiB of one pixel
// row (whole lines), not 64 partial segments of 4 bytes.  decode(w0, w1, rows): one word -> its four pixel rows, byte x of
// rows[y] = pixel (x, y).
template <bool TWO, typename DecodeRows>
__device__ __forceinline__ void plane_decode(const Bc45DecodeParams &P, DecodeRows decode) {
  constexpr uint32_t K = TWO ? 2u : 4u, BYTES = TWO ? 16u : 8u, C = TWO ? 2u : 1u;
  const LaneGroup g = locate_lane_group(P.log2_tile_cols, P.tile_row0, K, P.block_rows, P.block_cols);
  if (!g.valid) return;
  const uint8_t *src = P.blocks + (uint64_t)blockIdx.z * P.src_image_stride + ((uint64_t)g.brow * P.block_cols + g.bcol) * BYTES;
  uint8_t *dst = P.pixels + (uint64_t)blockIdx.z * P.dst_image_stride + (uint64_t)(g.brow * 4u) * P.row_stride +
                 (uint64_t)g.bcol * (4u * C);
  const bool full = g.bcol + K <= P.block_cols;
  uint32_t w[8];  // K * BYTES = 32 bytes of blocks
  if (full) {
    const U4 v0 = load_stream(reinterpret_cast<const U4 *>(src)), v1 = load_stream(reinterpret_cast<const U4 *>(src + 16));
    w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w; w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {  // block k is w[k * BYTES / 4 ...]
      const uint32_t i = k * (BYTES / 4u);
      if (g.bcol + k < P.block_cols) {
        const U2 v = load_stream(reinterpret_cast<const U2 *>(src + k * BYTES));
        w[i] = v.x; w[i + 1] = v.y;
        if (TWO) {
          const U2 u = load_stream(reinterpret_cast<const U2 *>(src + k * BYTES + 8));
          w[i + 2] = u.x; w[i + 3] = u.y;
        }
      } else {
        w[i] = w[i + 1] = 0u;
        if (TWO) w[i + 2] = w[i + 3] = 0u;
      }
    }
  }
  uint32_t out[4][4];  // out[y] = the 16 output bytes of pixel row y
  if (TWO) {
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      uint32_t r[4], gr[4];
      decode(w[4 * k], w[4 * k + 1], r);
      decode(w[4 * k + 2], w[4 * k + 3], gr);
#pragma unroll
      for (int y = 0; y < 4; ++y) interleave_rg_row(r[y], gr[y], &out[y][2 * k]);
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      uint32_t r[4];
      decode(w[2 * k], w[2 * k + 1], r);
#pragma unroll
      for (int y = 0; y < 4; ++y) out[y][k] = r[y];
    }
  }
  const uint32_t row = g.brow * 4u, col = g.bcol * 4u;
  if (row + 4u <= P.height && (uint64_t)col + 4u * K <= P.width) {
#pragma unroll
    for (int y = 0; y < 4; ++y) store_stream16(dst + (uint64_t)y * P.row_stride, out[y][0], out[y][1], out[y][2], out[y][3]);
  } else {  // clipped at the image's edge (helper.h:218-262)
    const uint32_t rows = umin(P.height - row, 4u), bytes = (uint32_t)umin(P.width - col, 4u * K) * C;
    for (uint32_t y = 0; y < rows; ++y)
      for (uint32_t i = 0; i < bytes; ++i) dst[(uint64_t)y * P.row_stride + i] = (uint8_t)(out[y][i >> 2] >> (8 * (i & 3u)));
  }
}

// Grid of lane-group tiles over block_rows x groups, images in grid.z; images and tile rows in chunks of at most 65 535.
template <typename Params, typename Kernel>
hipError_t launch_lane_groups(Kernel kernel, Params P, uint32_t n_images, uint32_t groups, hipStream_t stream,
                              const uint8_t *Params::*src, uint64_t src_image_stride, uint8_t *Params::*dst,
                              uint64_t dst_image_stride) {
  if (n_images == 0 || groups == 0 || P.block_rows == 0) return hipSuccess;
  P.log2_tile_cols = tile_log2_cols(groups);
  const uint32_t cols = 1u << P.log2_tile_cols, rows = 256u >> P.log2_tile_cols;
  const uint32_t gx = (groups + cols - 1u) / cols, gy = (uint32_t)(((uint64_t)P.block_rows + rows - 1u) / rows);
  (void)hipGetLastError();  // a stale error of another library on this thread is not this launch's
  for (uint32_t first = 0; first < n_images; first += 65535u) {
    const uint32_t count = n_images - first < 65535u ? n_images - first : 65535u;
    for (uint32_t row0 = 0; row0 < gy; row0 += 65535u) {
      Params Q = P;
      Q.*src = P.*src + (uint64_t)first * src_image_stride;
      Q.*dst = P.*dst + (uint64_t)first * dst_image_stride;
      Q.tile_row0 = row0;
      hipLaunchKernelGGL(kernel, dim3(gx, gy - row0 < 65535u ? gy - row0 : 65535u, count), dim3(kThreadsPerWorkgroup), 0,
                         stream, Q);
    }
  }
  return hipGetLastError();
}

}  // namespace icamd
#endif  // ICAMD_LANE_GROUPS_H_
