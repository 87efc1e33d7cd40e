// dxt_kernels.hip -- DXT1 / DXT5 encode kernels for gfx950 (MI355X).
//
// One 4x4 block per lane, 256 lanes per workgroup, one workgroup per tile of consecutive blocks of a
// block row (locate_tile, ic_device.h; the wide DXT1 <- RGBA8 kernels: the same waves, each its own 64-lane
// workgroup, dxt_plan.h): consecutive lanes read consecutive 16-byte (RGBA8) or 12-byte
// (RGB888) row segments -- a wave's four row loads are 1 KiB / 768 B contiguous each -- and write
// consecutive 8/16-byte blocks (reference raster order, internal/compressor4x4_helper.h:202-214).
// 4.5 / 3.5 / 5 algorithmic bytes per pixel (DXT1 from RGBA8 / RGB888, DXT5) and 255 / 276 / 614 integer VALU
// instructions per block (r01): DXT1 from RGBA8 streams at the practical HBM rate, the other two are bound by
// instruction issue (see dxt_block.h).
#include "dxt_block.h"
#include "dxt_plan.h"
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

// THROUGH (DXT1): the 8-byte blocks are written through to memory (store_through8), which needs an 8-byte aligned output;
// launch_dxt takes the non-temporal form (store_stream8) for any other output pointer or image stride.
// LANES (wide kernels): 256, or 64 = one-wave workgroups -- the tile's four waves as four workgroups of 64 x 1 blocks
// (dxt_plan.h; blockIdx.x counts 64-block pieces, and full / interior / the stash are the wave's own: 4 KiB of LDS).
// (r08: fetching every kernel-argument field of the fast path in ONE round in front of the validity branch -- the compiler
// takes two, with nothing of the wave in flight -- was tried on the one-wave form: 0.1842 against 0.1820 ms in one call, 0.1823
// against 0.1826 in the next; not shown to be "not slower", not kept.  profiles/r08_ab_dxt_wave_workgroups.log)
template <int COMPS, bool DXT5, bool WIDE, bool THROUGH = false, uint32_t LANES = kThreadsPerWorkgroup>
__device__ __forceinline__ void dxt_encode_one(const GridParams &P) {
  const TileCoord t = locate_tile<WIDE, 1, LANES>(P);
  if (!t.valid) return;
  uint32_t px[16];
  load_tile_block<COMPS>(P, t, px);
  const bool swap = P.swap_rb != 0;
  __shared__ uint32_t lds_px[4][LANES][4];
  BlockStashRows<LANES * 4> stash;
  stash.base = &lds_px[0][threadIdx.x][0];
  if (DXT5) {
    // has_one_pixel: block entirely right of AND below the image (pixel4x4.cc:58)
    const bool one_pixel = (t.bcol * 4 >= P.width) && (t.brow * 4 >= P.height);
    const Out8 a = encode_dxt5_alpha_block(px, one_pixel);
    const Out8 c = encode_dxt_color_block(px, swap, true, stash);
    // alpha block then colour block, dxtc.cc:94-96
    store_stream16(tile_dst<16>(P, t), a.lo, a.hi, c.lo, c.hi);
  } else {
    const Out8 c = encode_dxt_color_block(px, swap, false, stash);
    if (THROUGH) store_through8(tile_dst<8>(P, t), c.lo, c.hi);
    else store_stream8(tile_dst<8>(P, t), c.lo, c.hi);
  }
}

// Two vertically adjacent blocks per lane (256 x 2-block tiles): all eight row loads are issued before the first
// block is encoded (twice the bytes in flight per wave: the 12-byte-per-lane loads of a 3-byte source keep a quarter
// less in flight than RGBA8's), and the tile prologue (coordinates, 64-bit bases) is paid once for two blocks.
template <int COMPS, bool DXT5, bool THROUGH>
__device__ __forceinline__ void dxt_encode_two(const GridParams &P) {
  const TileCoord t = locate_tile<true, 2>(P);
  __shared__ uint32_t lds_px[4][kThreadsPerWorkgroup][4];
  BlockStash stash;
  stash.base = &lds_px[0][threadIdx.x][0];
  const bool swap = P.swap_rb != 0;
  TileCoord tr[2];
  uint32_t px[2][16];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    tr[r] = t;
    tr[r].brow0 = t.brow0 + (uint32_t)r;
    tr[r].brow = tr[r].brow0;
    tr[r].valid = t.full || (t.bcol < P.block_cols && tr[r].brow < P.block_rows);
    if (tr[r].valid) load_tile_block<COMPS>(P, tr[r], px[r]);
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (!tr[r].valid) continue;
    if (DXT5) {
      const bool one_pixel = (tr[r].bcol * 4 >= P.width) && (tr[r].brow * 4 >= P.height);
      const Out8 a = encode_dxt5_alpha_block(px[r], one_pixel);
      const Out8 c = encode_dxt_color_block(px[r], swap, true, stash);
      store_stream16(tile_dst<16>(P, tr[r]), a.lo, a.hi, c.lo, c.hi);
    } else {
      const Out8 c = encode_dxt_color_block(px[r], swap, false, stash);
      if (THROUGH) store_through8(tile_dst<8>(P, tr[r]), c.lo, c.hi);
      else store_stream8(tile_dst<8>(P, tr[r]), c.lo, c.hi);
    }
  }
}

extern "C" {

// (r03: two HORIZONTALLY adjacent blocks per lane -- 24 contiguous bytes per row as a 16-byte + an 8-byte load, one
// 16-byte store, 512 x 1-block tiles -- measured 10 % slower than this kernel on every content,
// profiles/r03_ab_rgb888_hpair.log; the variant is in the history at commit "DXT colour index search in O(1)".)
// 3-byte sources only (r02 A/B, 16 x 4096^2, ms per launch, one block vs two blocks per lane): RGB888 0.183 -> 0.175
// (noise), 0.190 -> 0.183 (flat), 0.174 -> 0.172 (smooth); RGBA8 0.190 -> 0.201 and DXT5 0.253 -> 0.259 got slower
// (67-71 VGPRs instead of 51-54) and keep one block per lane.
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_dxt1_rgb888_x2_kernel(GridParams P) { dxt_encode_two<3, false, true>(P); }
// (r04: the same two-block form for RGBA8 launches of one 4096^2 image or less was 1.1-1.3 us slower per call, not shipped;
// profiles/r04_single_image_timeline.txt, section c)

// *_kernel: 256 x 1-block tiles (block grids more than 128 columns wide); *_narrow_kernel: any tile shape.  The wide DXT1
// kernels write through (store_through8); *_nt_kernel: the same with non-temporal stores, for outputs not 8-byte aligned.
// (r07 A/B, 16 x 4096^2, ms per step: RGBA8 0.195 -> 0.187, RGB888 0.158 -> 0.144; profiles/r07_ab_dxt1_store_policy.log)
// The wide DXT1 <- RGBA8 kernels are launched one wave per workgroup (64 lanes, dxt_plan.h).  r08 A/B, ms per step, 256 -> 64 lanes:
// RGBA8 0.1868 -> 0.1820 (16 x 4096^2), 0.0508 -> 0.0502 (64 x 1024^2); RGB888 0.1467 -> 0.1516 and DXT5 (4 x 8192^2) 0.2107 ->
// 0.2138 got slower and keep 256 lanes; profiles/r08_ab_dxt_wave_workgroups.log
__global__ void __launch_bounds__(64) icamd_dxt1_rgba8_kernel(GridParams P) { dxt_encode_one<4, false, true, true, 64>(P); }
__global__ void __launch_bounds__(64) icamd_dxt1_rgba8_nt_kernel(GridParams P) { dxt_encode_one<4, false, true, false, 64>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_dxt1_rgb888_x2_nt_kernel(GridParams P) { dxt_encode_two<3, false, false>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_dxt5_rgba8_kernel(GridParams P) { dxt_encode_one<4, true, true>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_dxt1_rgba8_narrow_kernel(GridParams P) { dxt_encode_one<4, false, false>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_dxt1_rgb888_narrow_kernel(GridParams P) { dxt_encode_one<3, false, false>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_dxt5_rgba8_narrow_kernel(GridParams P) { dxt_encode_one<4, true, false>(P); }

}  // extern "C"

const char *dxt_kernel_name(int codec, int comps) {
  if (codec == ICAMD_DXT5) return "icamd_dxt5_rgba8_kernel";
  return comps == 4 ? "icamd_dxt1_rgba8_kernel" : "icamd_dxt1_rgb888_x2_kernel";
}

hipError_t launch_dxt(int codec, int comps, const GridParams &P, hipStream_t stream) {
  // the wide kernels above are compiled for the workgroup size dxt_launch_form gives them (dxt_plan.h)
  const DxtLaunchForm form = dxt_launch_form(codec, comps, P.block_cols, P.row_stride);
  if (codec == ICAMD_DXT5) {
    if (comps != 4) return hipErrorInvalidValue;
    return launch_tiled(icamd_dxt5_rgba8_kernel, icamd_dxt5_rgba8_narrow_kernel, P, stream, 8, form.wide_rows, form.wave_workgroups);
  }
  // every block is 8-byte aligned iff the output base and the image stride are (block offsets are multiples of 8)
  const bool through = (((uintptr_t)P.dst | P.dst_image_stride) & 7u) == 0;
  if (comps == 4)
    return launch_tiled(through ? icamd_dxt1_rgba8_kernel : icamd_dxt1_rgba8_nt_kernel, icamd_dxt1_rgba8_narrow_kernel, P, stream, 8,
                        form.wide_rows, form.wave_workgroups);
  return launch_tiled(through ? icamd_dxt1_rgb888_x2_kernel : icamd_dxt1_rgb888_x2_nt_kernel, icamd_dxt1_rgb888_narrow_kernel, P,
                      stream, 8, form.wide_rows, form.wave_workgroups);
}

}  // namespace icamd
