// bptc_mip_plan.h -- what icamd_encode_bc7_mips_device and icamd_encode_bc6h_mips_device launch: the pixel-pyramid passes
// (mip_plan.h's, into the workspace: the 8-bit kernels for BC7, the half-float kernel of mip_f16_kernels.hip for BC6H), and ONE
// encode launch over every level of every image, whose workgroups find their level in the table of etc2_mip_plan.h (DESIGN.md
// 3.25).
//
// Host-only arithmetic on a handful of integers: no HIP header, no runtime call, no allocation.  ic_capi.hip makes one plan per
// call and walks it; bptc_mip_kernels.hip defines its kernels from the list below and looks a workgroup up with etc2_mip_locate
// -- the same function tests/host_emul/bptc_mip_plan_driver.cc runs with g++ over every workgroup of a grid of shapes.
#ifndef ICAMD_BPTC_MIP_PLAN_H_
#define ICAMD_BPTC_MIP_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "codec_info.h"
#include "etc2_mip_plan.h"
#include "mip_plan.h"

namespace icamd {

// ---- the kernel list: X(chain kernel, per-level twin, codec, channels, modes) ----
// One chain form per BC7 / BC6H encode kernel.  The twin is the per-level kernel's narrow form, whose body (any tile shape,
// 256 x 1 included) the chain kernel runs; channels are bytes (BC7) or halves (BC6H) per source pixel; modes 0 = DEFAULT,
// 1 = EXTENDED (ICAMD_BC7_MODES_*, ICAMD_BC6H_MODES_*).
#define ICAMD_BPTC_MIP_KERNELS(X)                                                                                         \
  X(icamd_bc7_mip_rgb888_kernel, icamd_bc7_rgb888_narrow_kernel, ICAMD_BC7, 3, 0)                                         \
  X(icamd_bc7_mip_rgba8_kernel, icamd_bc7_rgba8_narrow_kernel, ICAMD_BC7, 4, 0)                                           \
  X(icamd_bc7_modes_mip_rgb888_kernel, icamd_bc7_modes_rgb888_narrow_kernel, ICAMD_BC7, 3, 1)                             \
  X(icamd_bc7_modes_mip_rgba8_kernel, icamd_bc7_modes_rgba8_narrow_kernel, ICAMD_BC7, 4, 1)                               \
  X(icamd_bc6h_mip_uf16_rgb16f_kernel, icamd_bc6h_uf16_rgb16f_narrow_kernel, ICAMD_BC6H_UF16, 3, 0)                       \
  X(icamd_bc6h_mip_uf16_rgba16f_kernel, icamd_bc6h_uf16_rgba16f_narrow_kernel, ICAMD_BC6H_UF16, 4, 0)                     \
  X(icamd_bc6h_mip_sf16_rgb16f_kernel, icamd_bc6h_sf16_rgb16f_narrow_kernel, ICAMD_BC6H_SF16, 3, 0)                       \
  X(icamd_bc6h_mip_sf16_rgba16f_kernel, icamd_bc6h_sf16_rgba16f_narrow_kernel, ICAMD_BC6H_SF16, 4, 0)                     \
  X(icamd_bc6h_modes_mip_uf16_rgb16f_kernel, icamd_bc6h_modes_uf16_rgb16f_narrow_kernel, ICAMD_BC6H_UF16, 3, 1)           \
  X(icamd_bc6h_modes_mip_uf16_rgba16f_kernel, icamd_bc6h_modes_uf16_rgba16f_narrow_kernel, ICAMD_BC6H_UF16, 4, 1)         \
  X(icamd_bc6h_modes_mip_sf16_rgb16f_kernel, icamd_bc6h_modes_sf16_rgb16f_narrow_kernel, ICAMD_BC6H_SF16, 3, 1)           \
  X(icamd_bc6h_modes_mip_sf16_rgba16f_kernel, icamd_bc6h_modes_sf16_rgba16f_narrow_kernel, ICAMD_BC6H_SF16, 4, 1)

inline bool bptc_mip_codec(int codec) { return codec == ICAMD_BC7 || codec == ICAMD_BC6H_UF16 || codec == ICAMD_BC6H_SF16; }
// Bytes of a source pixel: `chans` bytes (BC7) or halves (BC6H).
inline uint32_t bptc_mip_pixel_bytes(int codec, int chans) { return (uint32_t)chans * (codec == ICAMD_BC7 ? 1u : 2u); }
// A row's place in ICAMD_BPTC_MIP_KERNELS, or -1: the index of bptc_mip_kernels.hip's pointer table.
inline int bptc_mip_kernel_index(int codec, int chans, int modes) {
  int i = 0;
#define ICAMD_BPTC_MIP_MATCH(name, twin, c, n, m) \
  if (codec == (c) && chans == (n) && modes == (m)) return i; \
  ++i;
  ICAMD_BPTC_MIP_KERNELS(ICAMD_BPTC_MIP_MATCH)
#undef ICAMD_BPTC_MIP_MATCH
  return -1;
}
inline const char *bptc_mip_kernel_form(int codec, int chans, int modes) {  // "" where there is no kernel
#define ICAMD_BPTC_MIP_NAME(name, twin, c, n, m) #name,
  static const char *const kNames[] = { ICAMD_BPTC_MIP_KERNELS(ICAMD_BPTC_MIP_NAME) };
#undef ICAMD_BPTC_MIP_NAME
  const int i = bptc_mip_kernel_index(codec, chans, modes);
  return i >= 0 ? kNames[i] : "";
}

// One image's encoded chain, as mip_chain_bytes (which must keep answering 0 for these codecs): its bytes, level l at offsets[l]
// (levels + 1 entries; may be null).
inline size_t bptc_mip_chain_bytes(int codec, uint32_t h, uint32_t w, uint32_t levels, size_t *offsets) {
  if (!bptc_mip_codec(codec) || levels == 0 || levels > mip_max_levels(h, w)) return 0;
  size_t total = 0;
  for (uint32_t l = 0; l < levels; ++l) {
    if (offsets) offsets[l] = total;
    total += mip_level_blocks(codec, h, w, l);
  }
  if (offsets) offsets[levels] = total;
  return total;
}

// ---- the plan ----
struct BptcMipIn {
  int codec, chans, filter, modes;  // filter: ICAMD_MIP_FILTER_* of the 8-bit pyramid (BC7); 0 for BC6H
  uint32_t height, width, levels, n_images;
  uint32_t row_stride;                          // of the source
  uint64_t src_image_stride, dst_image_stride;  // the caller's
};
struct BptcMipPlan {
  int form;                // MipForm: kMipRefused (no such chain, or a grid.x of 2^31 and more), kMipNothing (no image), kMipLaunch
  size_t workspace_bytes;  // the pixel pyramid of every image, whenever the chain exists
  uint64_t pyramid_image_stride;  // bytes between the images' pyramids in the workspace
  size_t chain_bytes;
  // the pixel pyramid into the workspace: pyramid.pass[0 .. pyramid.n_passes); the passes of mip_plan_passes with the pixel's
  // bytes (3 / 4 for BC7, 6 / 8 for BC6H) in place of the component count
  MipChainPlan pyramid;
  // the encode launch: grid.x = the table's workgroups of one image, largest level first; images in grid.y, in pieces of at most
  // kMipGridLimitYZ (mip_piece)
  Etc2MipTable table;
  uint32_t grid_x, n_images;
};

inline BptcMipPlan bptc_mip_plan(const BptcMipIn &in) {
  BptcMipPlan plan = {};
  plan.form = kMipRefused;
  if (bptc_mip_kernel_index(in.codec, in.chans, in.modes) < 0 || in.levels == 0 || in.levels > mip_max_levels(in.height, in.width))
    return plan;
  const int pixel_bytes = (int)bptc_mip_pixel_bytes(in.codec, in.chans);
  size_t block_off[kMipMaxLevels + 1], pixel_off[kMipMaxLevels + 1];
  plan.chain_bytes = bptc_mip_chain_bytes(in.codec, in.height, in.width, in.levels, block_off);
  plan.pyramid_image_stride = mip_pyramid_bytes(in.height, in.width, in.levels, pixel_bytes, pixel_off);
  plan.workspace_bytes = (size_t)plan.pyramid_image_stride * in.n_images;
  plan.n_images = in.n_images;
  if (in.levels > 1) {
    const MipChainIn pyr = { kMipPyramidMode, pixel_bytes, in.filter, in.height, in.width, in.levels, in.n_images, in.row_stride,
                             in.src_image_stride, plan.pyramid_image_stride };
    (void)mip_plan_passes(pyr, false, kMipWorkspace, plan.pyramid_image_stride, nullptr, pixel_off, plan.pyramid);
  }
  // the tile rule launch_tiled applies to these codecs: up to 256 x 1 blocks
  plan.grid_x = etc2_mip_fill_table(plan.table, in.height, in.width, in.levels, kEtc2MipLargestFirst, in.row_stride,
                                    (uint32_t)pixel_bytes, pixel_off, block_off, 8u);
  const bool pyramid_kernel = in.codec != ICAMD_BC7 || mip_kernel_form(kMipPyramidMode, in.chans, in.filter).exists;
  plan.form = plan.grid_x == 0 || !pyramid_kernel ? kMipRefused : in.n_images == 0 ? kMipNothing : kMipLaunch;
  if (plan.form != kMipLaunch) plan.pyramid.n_passes = 0;
  return plan;
}

}  // namespace icamd
#endif  // ICAMD_BPTC_MIP_PLAN_H_
