// etc2_encode_bodies.inc -- what one workgroup of an ETC2-family encode kernel does with its tile: ETC2 RGBA8, ETC2 RGB8 (and its
// T / H pass), ETC2 RGB8A1 (and the colour-mode passes of the two), EAC R11 / RG11.  Kernel text for gfx950, included by the kernel translation units only -- not a header
// of block math: it has no host emulation (the block routines these call live in the *_block.h headers, which have one, and the
// workgroup -> tile -> block walk is emulated in tests/host_emul/etc2_mip_emul.cc).
//
// Every body takes the launch's GridParams and the tile as a TileAt (ic_device.h) and has two callers:
//   the per-level kernels (etc2_kernels.hip, etc2_rgb8_kernels.hip, etc2_th_kernels.hip, etc2_a1_kernels.hip,
//     etc2_colour_modes_kernels.hip, eac11_kernels.hip),
//     whose grid is launch_tiled's: tile_of_launch(P);
//   the chain kernels (etc2_mip_kernels.hip), one launch over every level of a mip chain: P is the level's view and the tile
//     comes from the level table.
// So a level of a chain is byte for byte what the per-level kernel writes for it: the same loads, the same block routines, the
// same lanes in every wave vote.  The comments on registers and phases are those of the per-level files, where they were measured.
#ifndef ICAMD_ETC2_ENCODE_BODIES_H_
#define ICAMD_ETC2_ENCODE_BODIES_H_

#include "etc1_block.h"
#include "etc2_block.h"
#include "etc2_colour_block.h"
#include "etc2_a1_block.h"
#include "etc2_th_block.h"
#include "etc2_a1_th_block.h"
#include "eac11_block.h"
#include "metric_block.h"  // metric_gather_channel: the clamp-to-edge gather of one channel

namespace icamd {

// ---- ETC2 RGBA8 (etc2_kernels.hip) ----
template <int STRATEGY>
__device__ __forceinline__ void etc2_encode_one(const GridParams &P, const TileAt &at) {
  const TileCoord t = locate_tile<false>(P, at.col, at.row, at.img);
  if (!t.valid) return;
  uint32_t px[16];
  load_tile_block<4>(P, t, px);
  uint32_t al[4];  // row y's four alpha bytes, byte x = texel (x, y)
#pragma unroll
  for (int y = 0; y < 4; ++y)
    al[y] = perm(px[4 * y + 1], px[4 * y], 0x0c0c0703u) | perm(px[4 * y + 3], px[4 * y + 2], 0x07030c0cu);
  Out8 c;
  if (STRATEGY == 3) {
    c = encode_etc1_block<false>(px, 3u);
  } else {
    const uint32_t spread = etc1_block_spread(px);
    c = etc1_encode_classified<STRATEGY>(px, etc1_constant_block(px, spread), spread >= ICAMD_ETC1_BUSY_SPREAD);
  }
  uint32_t a[16];
#pragma unroll
  for (int p = 0; p < 16; ++p) a[p] = bfe(al[p >> 2], 8 * (p & 3), 8);
  const Out8 e = encode_eac_alpha(a);
  store_stream16(tile_dst<16>(P, t), e.lo, e.hi, c.lo, c.hi);
}

// ---- ETC2 RGB8 (etc2_rgb8_kernels.hip) ----
template <int COMPS, int STRATEGY>
__device__ __forceinline__ void etc2_rgb8_encode_one(const GridParams &P, const TileAt &at) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // uniform: a scalar register
  Out8 c;
  {
    const TileCoord t = locate_tile_lane(P, threadIdx.x, at.col, at.row, at.img);
    if (!t.valid) return;
    uint32_t px[16];
    load_tile_block<COMPS>(P, t, px);
    if (STRATEGY == 3) {
      c = encode_etc1_block<false>(px, 3u);
    } else {
      const uint32_t spread = etc1_block_spread(px);
      c = etc1_encode_classified<STRATEGY>(px, etc1_constant_block(px, spread), spread >= ICAMD_ETC1_BUSY_SPREAD);
    }
  }
  // Phase two holds NO vector register across the search: the lane index comes from the hardware (mbcnt) and the wave's from
  // a scalar register, the block's coordinates and addresses are derived again from them, and the texels are read again (the
  // compiler barrier keeps the second read apart from the first).  With as little as the lane index kept alive the RGBA8
  // kSmallerError kernel spills 8 bytes at 128 VGPRs.  (P and `at` are workgroup-uniform in both callers: scalar registers.)
  asm volatile("" ::: "memory");
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const TileCoord t = locate_tile_lane(P, lane + 64u * wave, at.col, at.row, at.img);
  if (!t.valid) return;  // (the same lanes as above; the store below is bounded by THIS coordinate)
  uint32_t px[16];
  load_tile_block<COMPS>(P, t, px);
  const Out8 o = etc2_rgb8_choose(px, c);
  store_stream8(tile_dst<8>(P, t), o.lo, o.hi);
}

// ---- the T / H pass of ETC2 RGB8 (etc2_th_kernels.hip) ----
template <int COMPS>
__device__ __forceinline__ void etc2_th_encode_one(const GridParams &P, const TileAt &at) {
  const TileCoord t = locate_tile_lane(P, threadIdx.x, at.col, at.row, at.img);
  if (!t.valid) return;  // (the load and the store below are bounded by this coordinate, as in the first launch)
  uint32_t px[16];
  load_tile_block<COMPS>(P, t, px);
  uint8_t *dst = tile_dst<8>(P, t);
  const U2 v = load_stream(reinterpret_cast<const U2 *>(dst));
  const Out8 w = { v.x, v.y };
  Out8 o;
  if (etc2_th_choose(px, w, &o)) store_stream8(dst, o.lo, o.hi);
}

// ---- the colour-mode passes of ETC2 RGBA8 and ETC2 RGB8A1 (etc2_colour_modes_kernels.hip) ----
// ETC2 RGBA8: the lane's colour word (bytes 8..15 of its block, an ETC1 word) becomes ICAMD_ETC2_RGB8's planar choice and, with TH,
// its T / H choice; 8 bytes are stored only where the word changed, the alpha word never.
template <bool TH>
__device__ __forceinline__ void etc2_rgba8_colour_one(const GridParams &P, const TileAt &at) {
  const TileCoord t = locate_tile_lane(P, threadIdx.x, at.col, at.row, at.img);
  if (!t.valid) return;  // (the load and the store below are bounded by this coordinate, as in the first launch)
  uint32_t px[16];
  load_tile_block<4>(P, t, px);
  uint8_t *dst = tile_dst<16>(P, t) + 8;
  const U2 v = load_stream(reinterpret_cast<const U2 *>(dst));
  const Out8 e = { v.x, v.y };
  const Out8 o = etc2_rgba8_colour_choose<TH>(px, e);
  if (o.lo != e.lo || o.hi != e.hi) store_stream8(dst, o.lo, o.hi);
}

// ETC2 RGB8A1: the T / H choice of the lane's block by its class (etc2_a1_th_block.h); stored only where the word changed.
__device__ __forceinline__ void etc2_a1_th_one(const GridParams &P, const TileAt &at) {
  const TileCoord t = locate_tile_lane(P, threadIdx.x, at.col, at.row, at.img);
  if (!t.valid) return;
  uint32_t px[16];
  load_tile_block<4>(P, t, px);
  uint8_t *dst = tile_dst<8>(P, t);
  const U2 v = load_stream(reinterpret_cast<const U2 *>(dst));
  const Out8 w = { v.x, v.y };
  Out8 o;
  if (etc2_a1_th_choose(px, w, &o)) store_stream8(dst, o.lo, o.hi);
}

// ---- ETC2 RGB8A1 (etc2_a1_kernels.hip) ----
template <int STRATEGY>
__device__ __forceinline__ void etc2_a1_encode_one(const GridParams &P, const TileAt &at) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // uniform: a scalar register
  Out8 c = { 0u, 0u };
  {
    const TileCoord t = locate_tile_lane(P, threadIdx.x, at.col, at.row, at.img);
    if (!t.valid) return;
    uint32_t px[16];
    load_tile_block<4>(P, t, px);
    uint32_t all = px[0];
    ICAMD_UNROLL
    for (int p = 1; p < 16; ++p) all &= px[p];
    const bool opaque = (all >> 31) != 0u;  // every byte 3 >= 128
    if (!wave_all(!opaque)) {
      if (opaque) {
        if (STRATEGY == 3) {
          c = encode_etc1_block<false>(px, 3u);
        } else {
          const uint32_t spread = etc1_block_spread(px);
          c = etc1_encode_classified<STRATEGY>(px, etc1_constant_block(px, spread), spread >= ICAMD_ETC1_BUSY_SPREAD);
        }
      }
    }
  }
  // Phase two holds only the ETC1 word across the search, as the ETC2 RGB8 kernels do: lane and wave index come from the
  // hardware, the coordinates are derived again and the texels read again.
  asm volatile("" ::: "memory");
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const TileCoord t = locate_tile_lane(P, lane + 64u * wave, at.col, at.row, at.img);
  if (!t.valid) return;  // (the same lanes as above; the store below is bounded by THIS coordinate)
  uint32_t px[16];
  load_tile_block<4>(P, t, px);
  const Out8 o = etc2_a1_block<STRATEGY>(px, c);
  store_stream8(tile_dst<8>(P, t), o.lo, o.hi);
}

// ---- EAC R11 / RG11 (eac11_kernels.hip) ----
struct __attribute__((packed, aligned(1))) EacU1 { uint32_t x; };

// r[y] byte x = R of texel (x, y) of the lane's block, g likewise (RG only): R = byte 0, or byte 2 of a swapped 3- / 4-byte
// source; G = byte 1.  Texels outside the image replicate its last row / column, also on a padded grid.
template <int COMPS, bool RG>
__device__ __forceinline__ void eac11_fetch(const GridParams &P, const TileCoord &t, uint32_t r[4], uint32_t g[4]) {
  if constexpr (COMPS >= 3) {
    uint32_t px[16];
    load_tile_block<COMPS>(P, t, px);
    const uint32_t lo = P.swap_rb ? 0x0c0c0602u : 0x0c0c0400u, hi = P.swap_rb ? 0x06020c0cu : 0x04000c0cu;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      r[y] = perm(px[4 * y + 1], px[4 * y], lo) | perm(px[4 * y + 3], px[4 * y + 2], hi);
      if (RG) g[y] = perm(px[4 * y + 1], px[4 * y], 0x0c0c0501u) | perm(px[4 * y + 3], px[4 * y + 2], 0x05010c0cu);
    }
  } else {
    const uint8_t *img = P.src + (uint64_t)t.img * P.src_image_stride;
    const uint32_t row = t.brow * 4u, col = t.bcol * 4u;
    if ((uint64_t)row + 4u <= P.height && (uint64_t)col + 4u <= P.width) {
      const uint8_t *p = img + (uint64_t)row * P.row_stride + (uint64_t)col * COMPS;
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const uint8_t *line = p + (uint64_t)y * P.row_stride;
        if (COMPS == 1) {
          r[y] = reinterpret_cast<const EacU1 *>(line)->x;
        } else {
          const U2 v = load_stream(reinterpret_cast<const U2 *>(line));
          r[y] = rg_row_r(v.x, v.y);
          if (RG) g[y] = rg_row_g(v.x, v.y);
        }
      }
    } else {
      metric_gather_channel<COMPS>(img, P.height, P.width, P.row_stride, row, col, 0u, r);
      if (RG) metric_gather_channel<COMPS>(img, P.height, P.width, P.row_stride, row, col, 1u, g);
    }
  }
}

template <int COMPS, bool RG>
__device__ __forceinline__ void eac11_encode_one(const GridParams &P, const TileAt &at) {
  const TileCoord t = locate_tile<false>(P, at.col, at.row, at.img);
  if (!t.valid) return;
  uint32_t r[4], g[4] = { 0u, 0u, 0u, 0u };
  eac11_fetch<COMPS, RG>(P, t, r, g);
  const Out8 a = encode_eac11_rows(r);
  if (RG) {
    const Out8 b = encode_eac11_rows(g);
    store_stream16(tile_dst<16>(P, t), a.lo, a.hi, b.lo, b.hi);
  } else {
    store_stream8(tile_dst<8>(P, t), a.lo, a.hi);
  }
}

}  // namespace icamd
#endif  // ICAMD_ETC2_ENCODE_BODIES_H_
