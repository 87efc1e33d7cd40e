// pvrtc_decode_tile.h -- the tile form of the PVRTC1 2 bpp / 4 bpp decoders up to the point where a lane holds everything
// its block's pixels depend on; what happens to the decoded pixel rows (decode_pvrtc2_block_rows / decode_pvrtc4_block_rows
// hand them to a sink) is the caller's: decode_kernels.hip stores them, metric_kernels.hip compares them with source pixels.
//
// Block grids of at least 32 x 8: one workgroup per TILE of 32 x 8 blocks.  Every lane expands its own block's
// colour word once (the packed-field -> channel-pair expansion is a quarter of the per-block work when each lane does it for all
// nine neighbours), the 84 blocks of the one-block ring around the tile are expanded by the first 84 lanes, the pairs (16 B per
// block) meet in LDS, one barrier.  The modulation / mode words of the four orthogonal neighbours (2 bpp only: its unstored
// pixels look at them) still come from memory (L1 hits).
#ifndef ICAMD_PVRTC_DECODE_TILE_H_
#define ICAMD_PVRTC_DECODE_TILE_H_

#include "decode_block.h"

namespace icamd {

constexpr uint32_t kPvrtcTileW = 32, kPvrtcTileH = 8;
constexpr uint32_t kPvrtcTilePairs = (kPvrtcTileH + 2) * (kPvrtcTileW + 2);  // U4 entries of LDS a tile kernel provides

// What a lane of a tile workgroup knows about its block after pvrtc_tile_neighbourhood.
struct PvrtcTileLane {
  uint32_t img;        // workgroup-uniform
  uint32_t bx0, by0;   // first block of the tile (uniform)
  uint32_t bx, by;     // this lane's block
  U2 own;              // its two words (modulation, colours)
  uint32_t mod[9], col[9];  // own words at 4; 2 bpp: the orthogonal neighbours' at 1, 3, 5, 7; the rest 0
  uint32_t C[3][3][4];      // expanded colours of the 3 x 3 block neighbourhood
};

// blocks: first image's Z-order block words; block_cols / block_rows: powers of two, at least the tile.  One barrier inside.
template <int BPP>
__device__ __forceinline__ void pvrtc_tile_neighbourhood(const uint8_t *all_blocks, uint64_t src_image_stride, uint32_t block_cols,
                                                         uint32_t block_rows, U4 *pairs, PvrtcTileLane &L) {
  const uint32_t log2_cols = 31u - (uint32_t)__builtin_clz(block_cols), log2_rows = 31u - (uint32_t)__builtin_clz(block_rows);
  const uint32_t tiles_x = block_cols >> 5, log2_tx = log2_cols - 5u, log2_tiles = log2_tx + log2_rows - 3u;
  const uint32_t img = blockIdx.x >> log2_tiles, tile = blockIdx.x & ((1u << log2_tiles) - 1u);
  const uint32_t bx0 = (tile & (tiles_x - 1u)) << 5, by0 = (tile >> log2_tx) << 3;
  const uint32_t cmask = block_cols - 1u, rmask = block_rows - 1u;
  const U2 *blocks = reinterpret_cast<const U2 *>(all_blocks + (size_t)img * src_image_stride);
  const uint32_t lx = threadIdx.x & 31u, ly = threadIdx.x >> 5;
  const uint32_t bx = bx0 + lx, by = by0 + ly;
  auto word_at = [&](uint32_t x, uint32_t y) { return blocks[spread_bits16(x & cmask) << 1 | spread_bits16(y & rmask)]; };
  // the four orthogonal neighbours step in the Z-order domain itself: x lives on the odd bits, y on the even ones; filling
  // the other coordinate's bits with ones lets a carry run across them, zeros let a borrow, and the spread grid mask wraps
  const uint32_t mx = spread_bits16(cmask) << 1, my = spread_bits16(rmask);
  auto publish = [&](uint32_t cell, uint32_t colour_word) {
    uint32_t e[4];
    pvrtc_expand_colors(colour_word, e);
    const U4 v = { e[0], e[1], e[2], e[3] };
    pairs[cell] = v;
  };
  const uint32_t sx = spread_bits16(bx) << 1, sy = spread_bits16(by);
  const U2 own = blocks[sx | sy];
  publish((ly + 1u) * (kPvrtcTileW + 2u) + lx + 1u, own.y);
  if (threadIdx.x < 2u * (kPvrtcTileW + 2u) + 2u * kPvrtcTileH) {  // the ring: top row, bottom row, left column, right column
    const uint32_t t = threadIdx.x;
    uint32_t cx, cy;  // cell coordinates in the (W + 2) x (H + 2) array
    if (t < kPvrtcTileW + 2u) { cx = t; cy = 0u; }
    else if (t < 2u * (kPvrtcTileW + 2u)) { cx = t - (kPvrtcTileW + 2u); cy = kPvrtcTileH + 1u; }
    else if (t < 2u * (kPvrtcTileW + 2u) + kPvrtcTileH) { cx = 0u; cy = t - 2u * (kPvrtcTileW + 2u) + 1u; }
    else { cx = kPvrtcTileW + 1u; cy = t - 2u * (kPvrtcTileW + 2u) - kPvrtcTileH + 1u; }
    publish(cy * (kPvrtcTileW + 2u) + cx, word_at(bx0 + cx - 1u, by0 + cy - 1u).y);
  }
  ICAMD_UNROLL
  for (int i = 0; i < 9; ++i) L.mod[i] = L.col[i] = 0u;
  L.mod[4] = own.x; L.col[4] = own.y;
  if (BPP == 2) {
    { const U2 w = blocks[sx | ((sy - 1u) & my)]; L.mod[1] = w.x; L.col[1] = w.y; }
    { const U2 w = blocks[((sx - 2u) & mx) | sy]; L.mod[3] = w.x; L.col[3] = w.y; }
    { const U2 w = blocks[(((sx | 0x55555555u) + 2u) & mx) | sy]; L.mod[5] = w.x; L.col[5] = w.y; }
    { const U2 w = blocks[sx | (((sy | 0xaaaaaaaau) + 1u) & my)]; L.mod[7] = w.x; L.col[7] = w.y; }
  }
  __syncthreads();
  ICAMD_UNROLL
  for (int r = 0; r < 3; ++r)
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) {
      const U4 v = pairs[(ly + (uint32_t)r) * (kPvrtcTileW + 2u) + lx + (uint32_t)c];
      L.C[r][c][0] = v.x; L.C[r][c][1] = v.y; L.C[r][c][2] = v.z; L.C[r][c][3] = v.w;
    }
  L.img = img; L.bx0 = bx0; L.by0 = by0; L.bx = bx; L.by = by; L.own = own;
}

}  // namespace icamd
#endif  // ICAMD_PVRTC_DECODE_TILE_H_
