// decode_kernels.hip -- DXT1 / DXT5 / ETC1 decode kernels for gfx950 ("next" row 8f.1): one block per
// lane, 8/16-byte coalesced block loads, 12/16-byte row-segment stores (Compressor4x4Helper::Decompress,
// internal/compressor4x4_helper.h:218-262: blocks past the image edge are clipped).  BC1A and BC2 (extensions, bc1a_block.h)
// decode here too, to RGBA8 rows.
#include "bc1a_block.h"      // decode_bc1a, decode_bc2
#include "blockops_block.h"  // decode_block.h + the palette-plane row decoders
#include "codec_info.h"
#include "ic_launch.h"
#include "ic_amd.h"
#include "pvrtc_decode_tile.h"

namespace icamd {

template <int CODEC>
__device__ __forceinline__ void decode_one(const DecodeParams &P, uint32_t k) {
  constexpr int COMPS = CODEC == ICAMD_DXT5 ? 4 : 3;
  const auto [img, rem, brow, bcol] = raster_block(P, k);
  const uint8_t *src = P.blocks + (size_t)img * P.src_image_stride + (size_t)rem * codec_block_bytes(CODEC);
  const bool swap = P.swap_rb != 0;
  uint32_t w[4] = { 0, 0, 0, 0 };
  if (CODEC == ICAMD_DXT5) {
    const U4 v = load_stream(reinterpret_cast<const U4 *>(src));  // no alignment assumed: the caller owns the block pointer
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
    const U2 v = load_stream(reinterpret_cast<const U2 *>(src));
    w[0] = v.x; w[1] = v.y;
  }
  uint8_t *dst = P.pixels + (size_t)img * P.dst_image_stride;
  const uint32_t row = brow * 4, col = bcol * 4;
  if (row + 4 <= P.height && col + 4 <= P.width) {
    // whole block inside the image: rows straight in memory order from the palette planes (blockops_block.h)
    uint32_t rows[4][4];
    decode_block_rows<CODEC>(w, swap, rows);
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      uint8_t *q = dst + (size_t)(row + y) * P.row_stride + (size_t)col * COMPS;
      // r05: non-temporal -- a wave's store instruction writes whole lines (64 x 16 or 12 contiguous bytes), each byte once
      if (COMPS == 4) store_stream16(q, rows[y][0], rows[y][1], rows[y][2], rows[y][3]);
      else store_stream12(q, rows[y][0], rows[y][1], rows[y][2]);
    }
  } else {  // clipped at the image's edge (helper.h:218-262): pixel by pixel
    uint32_t px[16];
    if (CODEC == ICAMD_DXT5) {
      decode_dxt_colors(w[2], w[3], swap, true, px);
      decode_dxt5_alpha(w[0], w[1], px);
    } else if (CODEC == ICAMD_DXT1) {
      decode_dxt_colors(w[0], w[1], swap, false, px);
    } else {
      decode_etc1(w[0], w[1], px);
    }
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (row + y < P.height && col + x < P.width) {
          uint8_t *q = dst + (size_t)(row + y) * P.row_stride + (size_t)(col + x) * COMPS;
          const uint32_t v = px[4 * y + x];
          q[0] = (uint8_t)v; q[1] = (uint8_t)(v >> 8); q[2] = (uint8_t)(v >> 16);
          if (COMPS == 4) q[3] = (uint8_t)(v >> 24);
        }
  }
}

// BC1A (8-byte blocks) and BC2 (16-byte blocks) as the formats define them (bc1a_block.h): four 16-byte row stores (RGBA8),
// clipped at the image's edge.
template <int CODEC>
__device__ __forceinline__ void bc1a_bc2_decode_one(const DecodeParams &P, uint32_t k) {
  const auto [img, rem, brow, bcol] = raster_block(P, k);
  const uint8_t *src = P.blocks + (size_t)img * P.src_image_stride + (size_t)rem * codec_block_bytes(CODEC);
  uint32_t px[16];
  if (CODEC == ICAMD_BC2) {
    const U4 v = load_stream(reinterpret_cast<const U4 *>(src));  // no alignment assumed: the caller owns the block pointer
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    decode_bc2(w, P.swap_rb != 0u, px);
  } else {
    const U2 v = load_stream(reinterpret_cast<const U2 *>(src));
    decode_bc1a(v.x, v.y, P.swap_rb != 0u, px);
  }
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
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc1a_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) bc1a_bc2_decode_one<ICAMD_BC1A>(P, k);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc2_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) bc1a_bc2_decode_one<ICAMD_BC2>(P, k);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_dxt1_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) decode_one<ICAMD_DXT1>(P, k);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_dxt5_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) decode_one<ICAMD_DXT5>(P, k);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc1_decode_kernel(DecodeParams P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k < P.total_blocks) decode_one<ICAMD_ETC1>(P, k);
}
}  // extern "C"

// PVRTC1 2 bpp / 4 bpp (extensions, see decode_block.h): one block (8 x 4 / 4 x 4 pixels) per lane, lanes in raster order of the
// block grid; the nine block words come from their Z-order slots.  Small textures (block grids below 32 x 8).
template <int BPP>
__device__ __forceinline__ void pvrtc_decode_generic(const DecodeParams &P) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k >= P.total_blocks) return;
  const auto [img, rem, by, bx] = raster_block(P, k);  // block_cols = width / 8 (2 bpp), / 4 (4 bpp)
  const U2 *blocks = reinterpret_cast<const U2 *>(P.blocks + (size_t)img * P.src_image_stride);
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
  uint8_t *dst = P.pixels + (size_t)img * P.dst_image_stride + (size_t)(by * 4u) * P.row_stride + (size_t)bx * (BPP == 2 ? 32u : 16u);
  if (BPP == 2) {
    uint32_t px[32];
    decode_pvrtc2_block(mod, col, px);
#pragma unroll
    for (int y = 0; y < 4; ++y) {  // (one 64-bit product above; the rows advance by additions)
      U4 v0 = { px[8 * y], px[8 * y + 1], px[8 * y + 2], px[8 * y + 3] };
      U4 v1 = { px[8 * y + 4], px[8 * y + 5], px[8 * y + 6], px[8 * y + 7] };
      *reinterpret_cast<U4 *>(dst) = v0;
      *reinterpret_cast<U4 *>(dst + 16) = v1;
      dst += P.row_stride;
    }
  } else {
    uint32_t px[16];
    decode_pvrtc4_block(mod[4], col, px);
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      U4 v0 = { px[4 * y], px[4 * y + 1], px[4 * y + 2], px[4 * y + 3] };
      *reinterpret_cast<U4 *>(dst) = v0;
      dst += P.row_stride;
    }
  }
}
// The same for block grids of at least 32 x 8: one workgroup per TILE of 32 x 8 blocks (pvrtc_decode_tile.h gathers the lane's
// neighbourhood through LDS); the decoded pixel rows are stored from here.
template <int BPP>
__device__ __forceinline__ void pvrtc_decode_tile(const DecodeParams &P, U4 *pairs, U4 (*turn)[128]) {
  PvrtcTileLane L;
  pvrtc_tile_neighbourhood<BPP>(P.blocks, P.src_image_stride, P.block_cols, P.block_rows, pairs, L);
  const uint32_t img = L.img, bx0 = L.bx0, by0 = L.by0, bx = L.bx, by = L.by;
  const U2 own = L.own;
  const uint32_t (&mod)[9] = L.mod, (&col)[9] = L.col;
  const uint32_t (&C)[3][3][4] = L.C;
  const size_t row_stride = P.row_stride;
  if (BPP == 4) {
    // a lane's 16 bytes of a pixel row are one store: lanes 0-31 / 32-63 of a wave write 512 contiguous bytes (whole lines) of
    // the two block rows they hold; non-temporal, row by row as the rows are finished
    uint8_t *dst = P.pixels + (size_t)img * P.dst_image_stride + (size_t)(by * 4u) * row_stride + (size_t)bx * 16u;
    decode_pvrtc4_block_rows(C, own.x, (own.y & 1u) != 0u, [&](int y, const uint32_t row[4]) {
      store_stream16(dst, row[0], row[1], row[2], row[3]);
      dst += row_stride;
    });
    return;
  }
  // r05: a lane's 32 bytes of a pixel row leave as two 16-byte stores, and with the lanes' own data those would each fill every
  // other 16 bytes of the lines they touch (measured: this store pattern ALONE took 0.30 ms per 16 x 4096^2, the arithmetic 0.21).
  // Each wave therefore turns its row segment round in 2 KiB of LDS -- lane i writes pieces 2 i and 2 i + 1, reads pieces i and
  // 64 + i -- so that one store instruction writes one whole kilobyte of ONE pixel row (lanes 0-31 hold block row 2 w of the
  // tile, lanes 32-63 block row 2 w + 1), non-temporal: 0.166 ms for the same bytes.  No barrier: LDS is in order within a wave.
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  U4 *const mine = turn[wave];
  uint8_t *dst = P.pixels + (size_t)img * P.dst_image_stride + (size_t)((by0 + 2u * wave) * 4u) * row_stride + (size_t)bx0 * 32u + lane * 16u;
  const size_t next_block_row = 4u * row_stride;
  decode_pvrtc2_block_rows(C, mod, col, [&](int y, const uint32_t row[8]) {  // (one 64-bit product above; the rows advance by additions)
    const U4 v0 = { row[0], row[1], row[2], row[3] }, v1 = { row[4], row[5], row[6], row[7] };
    mine[2u * lane] = v0;
    mine[2u * lane + 1u] = v1;
    __builtin_amdgcn_wave_barrier();
    const U4 a = mine[lane], b = mine[64u + lane];
    __builtin_amdgcn_wave_barrier();
    store_stream16(dst, a.x, a.y, a.z, a.w);
    store_stream16(dst + next_block_row, b.x, b.y, b.z, b.w);
    dst += row_stride;
  });
}

extern "C" {
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_pvrtc2_decode_kernel(DecodeParams P) { pvrtc_decode_generic<2>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_pvrtc4_decode_kernel(DecodeParams P) { pvrtc_decode_generic<4>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_pvrtc2_decode_tile_kernel(DecodeParams P) {
  __shared__ U4 pairs[kPvrtcTilePairs];
  __shared__ U4 turn[kThreadsPerWorkgroup / 64][128];
  pvrtc_decode_tile<2>(P, pairs, turn);
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_pvrtc4_decode_tile_kernel(DecodeParams P) {
  __shared__ U4 pairs[kPvrtcTilePairs];
  pvrtc_decode_tile<4>(P, pairs, nullptr);
}
}  // extern "C"

hipError_t launch_decode(int codec, const DecodeParams &P, hipStream_t stream) {
  if (P.total_blocks == 0) return hipSuccess;
  // PVRTC block grids of whole tiles: one workgroup per tile, total_blocks / 256 of them, which is the raster decoders' grid
  const bool tiles = P.block_cols >= kPvrtcTileW && P.block_rows >= kPvrtcTileH && (P.block_cols & (P.block_cols - 1u)) == 0u &&
                     (P.block_rows & (P.block_rows - 1u)) == 0u;
  void (*kernel)(DecodeParams);
  if (codec == ICAMD_DXT1) kernel = icamd_dxt1_decode_kernel;
  else if (codec == ICAMD_DXT5) kernel = icamd_dxt5_decode_kernel;
  else if (codec == ICAMD_ETC1) kernel = icamd_etc1_decode_kernel;
  else if (codec == ICAMD_BC1A) kernel = icamd_bc1a_decode_kernel;
  else if (codec == ICAMD_BC2) kernel = icamd_bc2_decode_kernel;
  else if (codec == ICAMD_PVRTC2) kernel = tiles ? icamd_pvrtc2_decode_tile_kernel : icamd_pvrtc2_decode_kernel;
  else if (codec == ICAMD_PVRTC4) kernel = tiles ? icamd_pvrtc4_decode_tile_kernel : icamd_pvrtc4_decode_kernel;
  else return hipErrorInvalidValue;
  return launch_raster_decode(kernel, P, stream);
}

}  // namespace icamd
