// bptc_encode_bodies.inc -- what one workgroup of a BC7 or BC6H encode kernel does with its tile: BC7 mode 6, BC7 with the
// mode-1 / mode-5 candidates, BC6H one-subset, BC6H with the two-subset candidate.  Kernel text for gfx950, included by the kernel
// translation units only -- not a header of block math (the block routines these call live in bc7_block.h, bc7_modes_block.h,
// bc6h_block.h and bc6h_modes_block.h, which have a host emulation).
//
// Every body takes the launch's GridParams and the tile as a TileAt (ic_device.h) and has two callers:
//   the per-level kernels (bc7_kernels.hip, bc7_modes_kernels.hip, bc6h_kernels.hip, bc6h_modes_kernels.hip), whose grid is
//     launch_tiled's: tile_of_launch(P);
//   the chain kernels (bptc_mip_kernels.hip), one launch over every level of a mip chain: P is the level's view and the tile comes
//     from the level table.
// So a level of a chain is byte for byte what the per-level kernel writes for it.  WIDE = the tile is 256 x 1 blocks.
#ifndef ICAMD_BPTC_ENCODE_BODIES_H_
#define ICAMD_BPTC_ENCODE_BODIES_H_

#include "bc7_modes_block.h"
#include "bc6h_modes_block.h"

namespace icamd {

// ---- BC7 mode 6 (bc7_kernels.hip) ----
template <int COMPS, bool WIDE>
__device__ __forceinline__ void bc7_encode_one(const GridParams &P, const TileAt &at) {
  const TileCoord t = locate_tile<WIDE>(P, at.col, at.row, at.img);
  if (!t.valid) return;
  uint32_t px[16], out[4];
  load_tile_block<COMPS>(P, t, px);
  encode_bc7<COMPS>(px, P.swap_rb != 0, out);
  store_stream16(tile_dst<16>(P, t), out[0], out[1], out[2], out[3]);
}

// ---- BC7 with the mode-1 / mode-5 candidates (bc7_modes_kernels.hip) ----
template <int COMPS, bool WIDE>
__device__ __forceinline__ void bc7_modes_encode_one(const GridParams &P, const TileAt &at) {
  const TileCoord t = locate_tile<WIDE>(P, at.col, at.row, at.img);
  if (!t.valid) return;
  uint32_t px[16], out[4];
  load_tile_block<COMPS>(P, t, px);
  encode_bc7_modes<COMPS>(px, P.swap_rb != 0, out);
  store_stream16(tile_dst<16>(P, t), out[0], out[1], out[2], out[3]);
}

// ---- BC6H one-subset (bc6h_kernels.hip) ----
template <int C, bool SIGNED, bool WIDE>
__device__ __forceinline__ void bc6h_encode_one(const GridParams &P, const TileAt &at) {
  const TileCoord t = locate_tile<WIDE>(P, at.col, at.row, at.img);
  if (!t.valid) return;
  uint32_t rg[16], b[16], out[4];
  bc6h_fetch<C>(P.src + (uint64_t)t.img * P.src_image_stride, P.height, P.width, P.row_stride, t.brow * 4u, t.bcol * 4u, rg, b);
  encode_bc6h<SIGNED>(rg, b, out);
  store_stream16(tile_dst<16>(P, t), out[0], out[1], out[2], out[3]);
}

// ---- BC6H with the two-subset candidate (bc6h_modes_kernels.hip) ----
template <int C, bool SIGNED, bool WIDE>
__device__ __forceinline__ void bc6h_modes_encode_one(const GridParams &P, const TileAt &at) {
  const TileCoord t = locate_tile<WIDE>(P, at.col, at.row, at.img);
  if (!t.valid) return;
  uint32_t rg[16], b[16], out[4];
  bc6h_fetch<C>(P.src + (uint64_t)t.img * P.src_image_stride, P.height, P.width, P.row_stride, t.brow * 4u, t.bcol * 4u, rg, b);
  encode_bc6h_modes<SIGNED>(rg, b, out);
  store_stream16(tile_dst<16>(P, t), out[0], out[1], out[2], out[3]);
}

}  // namespace icamd
#endif  // ICAMD_BPTC_ENCODE_BODIES_H_
