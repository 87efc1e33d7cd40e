// dxt_plan.h -- which launch form a DXT1 / DXT5 encode gets (launch_dxt, dxt_kernels.hip).
//
// Host-only arithmetic on a handful of integers: no HIP header, no runtime call.  launch_dxt asks dxt_launch_form once per call
// and hands the answer to launch_tiled; tests/host_emul/dxt_plan_driver.cc runs the same function with g++.
#ifndef ICAMD_DXT_PLAN_H_
#define ICAMD_DXT_PLAN_H_

#include <cstdint>

#include "etc2_mip_plan.h"  // encode_tile_shape

namespace icamd {

struct DxtLaunchForm {
  uint32_t log2_tile_cols;  // encode_tile_shape: 8 = the wide kernels (256 x wide_rows tiles), less = the narrow kernels
  uint32_t wide_rows;       // block rows of a wide tile = blocks per lane (2: DXT1 from RGB888)
  bool wave_workgroups;     // every wave of a wide tile is its own 64-lane workgroup of 64 x wide_rows blocks
  uint32_t lanes, grid_x;   // workgroup size and workgroups per row of tiles (launch_tiled: grid.y = tile rows, grid.z = images)
};

// One-wave workgroups (r08): a workgroup's wave slots are refilled only when its LAST wave has ended, and the
// waves of a DXT tile share nothing -- no barrier, the stash is per lane, the votes are per wave.  Launched one wave per
// workgroup, a slot is free again as soon as ITS wave ends.  A kernel has the form where its own A/B showed a gain
// (profiles/r08_ab_dxt_wave_workgroups.log): DXT1 from RGBA8 does (- 2.6 % per step at 16 x 4096^2, - 1 % at 64 x 1024^2, one
// 4096^2 image per call not slower: no line by launch size); DXT1 from RGB888 (+ 3.4 %) and DXT5 (+ 1.5 %) do not and keep
// 256 lanes, as do the narrow kernels (block grids of at most 128 columns).  The kernels of dxt_kernels.hip are compiled for
// the workgroup size this function gives them.
inline bool dxt_wave_workgroups(int codec, int comps) { return codec == ICAMD_DXT1 && comps == 4; }

// codec: ICAMD_DXT1 / ICAMD_DXT5; comps: source bytes per pixel; the block grid's width and the source's row stride in bytes.
inline DxtLaunchForm dxt_launch_form(int codec, int comps, uint32_t block_cols, uint32_t row_stride) {
  DxtLaunchForm f;
  f.log2_tile_cols = encode_tile_shape(block_cols, row_stride, 8u).log2_tile_cols;
  f.wide_rows = codec == ICAMD_DXT1 && comps == 3 ? 2u : 1u;
  f.wave_workgroups = f.log2_tile_cols == 8u && dxt_wave_workgroups(codec, comps);
  f.lanes = f.wave_workgroups ? 64u : 256u;
  const uint32_t cols = f.wave_workgroups ? 64u : 1u << f.log2_tile_cols;
  // (whole 256-block tiles either way: a one-wave workgroup beyond the last block column returns at once)
  const uint32_t tiles = (uint32_t)(((uint64_t)block_cols + (1u << f.log2_tile_cols) - 1u) >> f.log2_tile_cols);
  f.grid_x = tiles * ((1u << f.log2_tile_cols) / cols);
  return f;
}

}  // namespace icamd
#endif  // ICAMD_DXT_PLAN_H_
