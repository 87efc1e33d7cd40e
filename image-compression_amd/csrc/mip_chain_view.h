// mip_chain_view.h -- the kernel argument of a chain kernel (etc2_mip_kernels.hip, bptc_mip_kernels.hip) and the view of one
// level it gives the per-level encode body: device code, shared by the two translation units.  The table is etc2_mip_plan.h's.
#ifndef ICAMD_MIP_CHAIN_VIEW_H_
#define ICAMD_MIP_CHAIN_VIEW_H_

#include "etc2_mip_plan.h"
#include "ic_device.h"

namespace icamd {

struct Etc2MipParams {
  const uint8_t *src, *pyramid;  // image 0 of this launch: the caller's source, its pixel pyramid in the workspace
  uint8_t *dst;                  // and its chain
  uint64_t src_image_stride, pyramid_image_stride, dst_image_stride;
  uint32_t swap_rb, etc_strategy;
  Etc2MipTable table;
};
static_assert(sizeof(Etc2MipParams) <= 4096, "the kernel argument segment holds 4 KiB");

// The level's view: what the per-level kernel is given for level L.level of the chain (n_images is the launcher's: not read).
__device__ __forceinline__ GridParams etc2_mip_view(const Etc2MipParams &M, const Etc2MipLevel &L) {
  const bool top = L.level == 0u;
  GridParams P;
  P.src = (top ? M.src : M.pyramid) + L.pix_offset;
  P.dst = M.dst + L.dst_offset;
  P.src_image_stride = top ? M.src_image_stride : M.pyramid_image_stride;
  P.dst_image_stride = M.dst_image_stride;
  P.height = L.height;
  P.width = L.width;
  P.block_rows = L.block_rows;
  P.block_cols = L.block_cols;
  P.row_stride = L.row_stride;
  P.n_images = 0u;
  P.swap_rb = M.swap_rb;
  P.etc_strategy = M.etc_strategy;
  P.log2_tile_cols = L.log2_tile_cols;
  P.tile_row0 = 0u;
  P.force_gather = L.force_gather;
  return P;
}

}  // namespace icamd
#endif  // ICAMD_MIP_CHAIN_VIEW_H_
