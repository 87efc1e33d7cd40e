// bc1a_bc2_kernels.hip -- BC1 with punch-through alpha and BC2 encode kernels for gfx950 (EXTENSIONS, include/ic_amd.h
// ICAMD_BC1A, ICAMD_BC2); see bc1a_block.h for the block math and DESIGN.md 3.26.
//
// One 4 x 4 block per lane, 256 lanes per workgroup, launched as DXT5 is (dxt_kernels.hip): *_kernel on 256 x 1-block tiles for
// block grids more than 128 columns wide, *_narrow_kernel on any other tile shape; RGBA8 sources only.  The colour block is
// encode_dxt_color_block of dxt_block.h with its LDS stash; BC1A adds the masked three-colour path in the waves that hold a
// transparent texel (a wave vote, bc1a_block.h), BC2 the sixteen roundings of its alpha word.  The blocks leave as one
// non-temporal 8-byte (BC1A) or 16-byte (BC2: alpha word, then colour word) store.  The decode and metric kernels are in
// decode_kernels.hip and metric_kernels.hip.
#include "bc1a_block.h"
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

template <bool BC2, bool WIDE>
__device__ __forceinline__ void bc1a_bc2_encode_one(const GridParams &P) {
  const TileCoord t = locate_tile<WIDE>(P);
  if (!t.valid) return;
  uint32_t px[16];
  load_tile_block<4>(P, t, px);
  const bool swap = P.swap_rb != 0;
  __shared__ uint32_t lds_px[4][kThreadsPerWorkgroup][4];
  BlockStash stash;
  stash.base = &lds_px[0][threadIdx.x][0];
  if (BC2) {
    const Out8 a = encode_bc2_alpha_block(px);
    const Out8 c = encode_dxt_color_block(px, swap, true, stash);
    store_stream16(tile_dst<16>(P, t), a.lo, a.hi, c.lo, c.hi);
  } else {
    const Out8 c = encode_bc1a_block(px, swap, stash);
    store_stream8(tile_dst<8>(P, t), c.lo, c.hi);
  }
}

extern "C" {

__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc1a_rgba8_kernel(GridParams P) { bc1a_bc2_encode_one<false, true>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc1a_rgba8_narrow_kernel(GridParams P) { bc1a_bc2_encode_one<false, false>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc2_rgba8_kernel(GridParams P) { bc1a_bc2_encode_one<true, true>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_bc2_rgba8_narrow_kernel(GridParams P) { bc1a_bc2_encode_one<true, false>(P); }

}  // extern "C"

const char *bc1a_bc2_kernel_name(int codec, int comps) {
  if (comps != 4) return "";
  return codec == ICAMD_BC1A ? "icamd_bc1a_rgba8_kernel" : codec == ICAMD_BC2 ? "icamd_bc2_rgba8_kernel" : "";
}

hipError_t launch_bc1a_bc2_encode(int codec, const GridParams &P, hipStream_t stream) {
  if (codec == ICAMD_BC1A) return launch_tiled(icamd_bc1a_rgba8_kernel, icamd_bc1a_rgba8_narrow_kernel, P, stream, 8);
  if (codec == ICAMD_BC2) return launch_tiled(icamd_bc2_rgba8_kernel, icamd_bc2_rgba8_narrow_kernel, P, stream, 8);
  return hipErrorInvalidValue;
}

}  // namespace icamd
