// mip_plan.h -- what a mip-chain call launches: the levels of every pass, where each pass reads and writes, the workspace, the
// grid pieces of every launch, and which (mode, components, filter) has a kernel and what it is called.
//
// Host-only arithmetic on a handful of integers: no HIP header, no runtime call, no allocation.  ic_capi.hip makes one plan per
// call (mip_chain_plan) and walks it; mip_kernels.hip launches a planned pass; the three mip translation units define their
// kernels from the lists below.  tests/test_mip_plan_host.py compiles this header with g++ and pins the answers over a grid of
// inputs (tests/golden/mip_plan.txt).
#ifndef ICAMD_MIP_PLAN_H_
#define ICAMD_MIP_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "codec_info.h"

namespace icamd {

constexpr int kMipPyramidMode = -1;         // `mode` of the pixel-pyramid kernels (no encoder)
constexpr uint32_t kMipTile = 128;          // input pixels per tile side: one workgroup per tile
constexpr uint32_t kMipGridLimitYZ = 65535; // workgroups in a grid's y (tile rows) and z (images)
constexpr uint32_t kMipMaxLevels = 32;
constexpr uint32_t kMipMaxPasses = 6;       // 32 levels at six per pass
constexpr uint32_t kMipFilters = 5;         // ICAMD_MIP_FILTER_*: 0 .. 4

// ---- the kernel list: X(kernel name, mode, source components, filter) ----
// mip_kernels.hip (box filter)
#define ICAMD_MIP_BOX_KERNELS(X)                                \
  X(icamd_mip_dxt1_rgb888_kernel, ICAMD_DXT1, 3, 0)             \
  X(icamd_mip_dxt1_rgba8_kernel, ICAMD_DXT1, 4, 0)              \
  X(icamd_mip_dxt5_rgba8_kernel, ICAMD_DXT5, 4, 0)              \
  X(icamd_mip_bc4_r8_kernel, ICAMD_BC4, 1, 0)                   \
  X(icamd_mip_bc4_rg8_kernel, ICAMD_BC4, 2, 0)                  \
  X(icamd_mip_bc4_rgb888_kernel, ICAMD_BC4, 3, 0)               \
  X(icamd_mip_bc4_rgba8_kernel, ICAMD_BC4, 4, 0)                \
  X(icamd_mip_bc5_rg8_kernel, ICAMD_BC5, 2, 0)                  \
  X(icamd_mip_bc5_rgb888_kernel, ICAMD_BC5, 3, 0)               \
  X(icamd_mip_bc5_rgba8_kernel, ICAMD_BC5, 4, 0)                \
  X(icamd_mip_pyramid_r8_kernel, kMipPyramidMode, 1, 0)         \
  X(icamd_mip_pyramid_rg8_kernel, kMipPyramidMode, 2, 0)        \
  X(icamd_mip_pyramid_rgb888_kernel, kMipPyramidMode, 3, 0)     \
  X(icamd_mip_pyramid_rgba8_kernel, kMipPyramidMode, 4, 0)
// mip_filter_kernels.hip (ICAMD_MIP_FILTER_SRGB = 1, ICAMD_MIP_FILTER_ALPHA_WEIGHTED = 2, both = 3)
#define ICAMD_MIP_FILTER_KERNELS(X)                                     \
  X(icamd_fmip_srgb_dxt1_rgb888_kernel, ICAMD_DXT1, 3, 1)               \
  X(icamd_fmip_srgb_dxt1_rgba8_kernel, ICAMD_DXT1, 4, 1)                \
  X(icamd_fmip_srgb_dxt5_rgba8_kernel, ICAMD_DXT5, 4, 1)                \
  X(icamd_fmip_srgb_pyramid_rgb888_kernel, kMipPyramidMode, 3, 1)       \
  X(icamd_fmip_srgb_pyramid_rgba8_kernel, kMipPyramidMode, 4, 1)        \
  X(icamd_fmip_alpha_dxt1_rgba8_kernel, ICAMD_DXT1, 4, 2)               \
  X(icamd_fmip_alpha_dxt5_rgba8_kernel, ICAMD_DXT5, 4, 2)               \
  X(icamd_fmip_alpha_pyramid_rgba8_kernel, kMipPyramidMode, 4, 2)       \
  X(icamd_fmip_srgb_alpha_dxt1_rgba8_kernel, ICAMD_DXT1, 4, 3)          \
  X(icamd_fmip_srgb_alpha_dxt5_rgba8_kernel, ICAMD_DXT5, 4, 3)          \
  X(icamd_fmip_srgb_alpha_pyramid_rgba8_kernel, kMipPyramidMode, 4, 3)
// mip_normal_kernels.hip (ICAMD_MIP_FILTER_NORMAL = 4)
#define ICAMD_MIP_NORMAL_KERNELS(X)                             \
  X(icamd_nmip_bc5_rg8_kernel, ICAMD_BC5, 2, 4)                 \
  X(icamd_nmip_bc5_rgb888_kernel, ICAMD_BC5, 3, 4)              \
  X(icamd_nmip_bc5_rgba8_kernel, ICAMD_BC5, 4, 4)               \
  X(icamd_nmip_pyramid_rg8_kernel, kMipPyramidMode, 2, 4)
#define ICAMD_MIP_KERNELS(X) ICAMD_MIP_BOX_KERNELS(X) ICAMD_MIP_FILTER_KERNELS(X) ICAMD_MIP_NORMAL_KERNELS(X)

// A row's place in ICAMD_MIP_KERNELS, or -1: the index of mip_kernels.hip's pointer table.
inline int mip_kernel_index(int mode, int comps, int filter) {
  int i = 0;
#define ICAMD_MIP_MATCH(name, m, c, f) \
  if (mode == (m) && comps == (c) && filter == (f)) return i; \
  ++i;
  ICAMD_MIP_KERNELS(ICAMD_MIP_MATCH)
#undef ICAMD_MIP_MATCH
  return -1;
}
struct MipKernelForm {
  bool exists;
  const char *name;  // "" where there is no kernel
};
inline MipKernelForm mip_kernel_form(int mode, int comps, int filter) {
#define ICAMD_MIP_NAME(name, m, c, f) #name,
  static const char *const kNames[] = { ICAMD_MIP_KERNELS(ICAMD_MIP_NAME) };
#undef ICAMD_MIP_NAME
  const int i = mip_kernel_index(mode, comps, filter);
  return { i >= 0, i >= 0 ? kNames[i] : "" };
}

// ---- levels, sizes and offsets of one image ----
inline uint32_t mip_dim(uint32_t v, uint32_t l) { return l >= 32u ? 1u : (v >> l) ? v >> l : 1u; }
inline uint32_t mip_max_levels(uint32_t h, uint32_t w) {
  if (h == 0 || w == 0) return 0;
  uint32_t m = h > w ? h : w, l = 0;
  while (m >>= 1) ++l;
  return l + 1u;
}
inline bool mip_codec(int codec) {
  return codec == ICAMD_DXT1 || codec == ICAMD_DXT5 || codec == ICAMD_ETC1 || codec == ICAMD_BC4 || codec == ICAMD_BC5;
}
// bytes of level l's pixels, tight rows (COMPS bytes per pixel)
inline size_t mip_level_pixels(uint32_t h, uint32_t w, uint32_t l, int comps) { return (size_t)mip_dim(h, l) * mip_dim(w, l) * (size_t)comps; }
// bytes of level l's blocks
inline size_t mip_level_blocks(int codec, uint32_t h, uint32_t w, uint32_t l) {
  return (size_t)((mip_dim(h, l) + 3u) / 4u) * ((mip_dim(w, l) + 3u) / 4u) * codec_block_bytes(codec);
}
// One image's encoded chain: its bytes, level l at offsets[l] (levels + 1 entries, the last is the total; may be null).
// 0 where the codec has no chain or `levels` is not 1 .. mip_max_levels.
inline size_t mip_chain_bytes(int codec, uint32_t h, uint32_t w, uint32_t levels, size_t *offsets) {
  if (!mip_codec(codec) || levels == 0 || levels > mip_max_levels(h, w)) return 0;
  size_t total = 0;
  for (uint32_t l = 0; l < levels; ++l) {
    if (offsets) offsets[l] = total;
    total += mip_level_blocks(codec, h, w, l);
  }
  if (offsets) offsets[levels] = total;
  return total;
}
// One image's pixel pyramid (levels 1 .. levels-1, tight rows, back to back): its bytes, level l at offsets[l] for l = 1 .. levels
// (offsets[levels] is the total; may be null).
inline size_t mip_pyramid_bytes(uint32_t h, uint32_t w, uint32_t levels, int comps, size_t *offsets = nullptr) {
  size_t total = 0;
  for (uint32_t l = 1; l < levels; ++l) {
    if (offsets) offsets[l] = total;
    total += mip_level_pixels(h, w, l, comps);
  }
  if (offsets && levels) offsets[levels] = total;
  return total;
}

// ---- the plan ----
enum MipBase : int { kMipSource = 0, kMipWorkspace, kMipOutput };  // the caller's d_src, d_workspace, d_dst
struct MipRef {
  int base;
  uint64_t offset;  // bytes
};

enum MipForm : int {
  kMipRefused = 0,  // no such chain (mode, components, sizes, level count) or no kernel for (mode, components, filter)
  kMipNothing,      // no image, or a pyramid of level 0 alone: no launch
  kMipLaunch
};

struct MipChainIn {
  int mode;  // ICAMD_DXT1 / DXT5 / ETC1 / BC4 / BC5, or kMipPyramidMode
  int comps, filter;
  uint32_t height, width, levels, n_images;
  uint32_t row_stride;                          // of the source
  uint64_t src_image_stride, dst_image_stride;  // the caller's; the destination is the chain, or the pyramid
};

// One pass = one kernel over every tile of every image: levels [l0, l0 + n) from level l0's pixels.  A pass over more than one
// tile reaches local level 5 in blocks (6 with pixels only); `handoff`: further levels follow, from level l0 + 6's pixels, which
// this pass writes.  Everything MipParams (ic_launch.h) needs, pointers as MipRef.
struct MipPassPlan {
  uint32_t l0, n;
  bool handoff;
  MipRef in;
  uint32_t in_row_stride;
  uint64_t in_image_stride;
  uint32_t height, width;  // of the input level
  uint64_t level_off[8];   // blocks of local level j, from the image's chain in kMipOutput (bit j of enc_mask)
  uint64_t pix_off[8];     // pixels of local level j, from the image's start in `pix` (bit j of pix_mask)
  uint32_t enc_mask, pix_mask;
  MipRef pix;
  uint64_t pix_image_stride, dst_image_stride;
  // the launches: grid.x = tile columns; tile rows in grid.y and images in grid.z, each in pieces of at most kMipGridLimitYZ
  // (mip_piece), images outermost
  uint32_t grid_x, tile_rows, n_images;
};
// One ETC1 level through the ETC1 kernels of icamd_encode_device: n_images images of height x width at `in`, blocks to out_offset
// of each image's chain.
struct MipEncodeCall {
  uint32_t height, width;
  MipRef in;
  uint32_t in_row_stride;
  uint64_t in_image_stride, out_offset;
};
struct MipChainPlan {
  int form;
  size_t workspace_bytes;  // whenever the chain exists, kernel or not
  uint32_t n_passes, n_encodes;
  MipPassPlan pass[kMipMaxPasses];
  // ETC1 chains: encode[0] (level 0, from the source), then the passes (the pixel pyramid into the workspace), then encode[1 ..]
  MipEncodeCall encode[kMipMaxLevels];
};

// Piece i of `total` workgroups in pieces of at most kMipGridLimitYZ.
struct MipPiece {
  uint32_t first, count;
};
inline uint32_t mip_pieces(uint32_t total) { return (uint32_t)(((uint64_t)total + kMipGridLimitYZ - 1u) / kMipGridLimitYZ); }
inline MipPiece mip_piece(uint32_t total, uint32_t i) {
  const uint32_t first = i * kMipGridLimitYZ;
  return { first, total - first < kMipGridLimitYZ ? total - first : kMipGridLimitYZ };
}

// The passes of one chain or pyramid: the fused encode (`encode`) writes every level's blocks to kMipOutput and hands level
// l0 + 6's pixels to the next pass through a region of its own in the workspace, from ws_offset on; the pyramid writes every
// level's pixels to (pix_base, pix_image_stride) and the next pass reads level l0 + 6 where this one wrote it, so its multi-tile
// passes reach one level further.  Returns the workspace bytes the handoffs take.
inline uint64_t mip_plan_passes(const MipChainIn &in, bool encode, int pix_base, uint64_t pix_image_stride, const size_t *block_off,
                                const size_t *pixel_off, MipChainPlan &plan) {
  MipRef next = { kMipSource, 0 };
  uint32_t next_row_stride = in.row_stride;
  uint64_t next_image_stride = in.src_image_stride, ws = 0;
  for (uint32_t l0 = 0;; l0 += 6u) {
    MipPassPlan &P = plan.pass[plan.n_passes++];
    P.l0 = l0;
    P.height = mip_dim(in.height, l0);
    P.width = mip_dim(in.width, l0);
    const uint32_t left = in.levels - l0, most = P.height <= kMipTile && P.width <= kMipTile ? 8u : encode ? 6u : 7u;
    P.n = left < most ? left : most;
    P.handoff = P.n < left;
    P.in = next;
    P.in_row_stride = next_row_stride;
    P.in_image_stride = next_image_stride;
    P.grid_x = (uint32_t)(((uint64_t)P.width + kMipTile - 1u) / kMipTile);
    P.tile_rows = (uint32_t)(((uint64_t)P.height + kMipTile - 1u) / kMipTile);
    P.n_images = in.n_images;
    if (encode) {
      P.enc_mask = (1u << P.n) - 1u;
      P.dst_image_stride = in.dst_image_stride;
      for (uint32_t j = 0; j < P.n; ++j) P.level_off[j] = block_off[l0 + j];
      if (P.handoff) {
        P.pix_mask = 1u << 6;
        P.pix = { kMipWorkspace, ws };
        P.pix_image_stride = mip_level_pixels(in.height, in.width, l0 + 6u, in.comps);
        ws += P.pix_image_stride * in.n_images;
      }
    } else {
      P.pix_mask = ((1u << P.n) - 1u) & ~1u;
      P.pix = { pix_base, 0 };
      P.pix_image_stride = pix_image_stride;
      for (uint32_t j = 1; j < P.n; ++j) P.pix_off[j] = pixel_off[l0 + j];
    }
    if (!P.handoff) return ws;
    next = { P.pix.base, P.pix.offset + P.pix_off[6] };  // level l0 + 6 as this pass writes it: tight rows
    next_row_stride = mip_dim(in.width, l0 + 6u) * (uint32_t)in.comps;
    next_image_stride = P.pix_image_stride;
  }
}

inline MipChainPlan mip_chain_plan(const MipChainIn &in) {
  MipChainPlan plan = {};
  plan.form = kMipRefused;
  const bool pyramid = in.mode == kMipPyramidMode, etc1 = in.mode == ICAMD_ETC1;
  if ((!pyramid && !mip_codec(in.mode)) || in.comps < 1 || in.comps > 4 || in.levels == 0 ||
      in.levels > mip_max_levels(in.height, in.width))
    return plan;
  size_t block_off[kMipMaxLevels + 1], pixel_off[kMipMaxLevels + 1];
  if (!pyramid) (void)mip_chain_bytes(in.mode, in.height, in.width, in.levels, block_off);
  const size_t pyramid_bytes = mip_pyramid_bytes(in.height, in.width, in.levels, in.comps, pixel_off);
  // ETC1: the pixel pyramid into the workspace, images back to back, then the ETC1 kernels (a fused kernel is deferred)
  if (pyramid || etc1) {
    if (in.levels > 1) (void)mip_plan_passes(in, false, etc1 ? kMipWorkspace : kMipOutput, etc1 ? pyramid_bytes : in.dst_image_stride,
                                             nullptr, pixel_off, plan);
    plan.workspace_bytes = etc1 ? pyramid_bytes * in.n_images : 0;
  } else {
    plan.workspace_bytes = mip_plan_passes(in, true, 0, 0, block_off, nullptr, plan);
  }
  if (etc1) {
    plan.encode[plan.n_encodes++] = { in.height, in.width, { kMipSource, 0 }, in.row_stride, in.src_image_stride, 0 };
    for (uint32_t l = 1; l < in.levels; ++l) {
      const uint32_t lw = mip_dim(in.width, l);
      plan.encode[plan.n_encodes++] = { mip_dim(in.height, l), lw, { kMipWorkspace, pixel_off[l] }, lw * (uint32_t)in.comps,
                                        pyramid_bytes, block_off[l] };
    }
  }
  const bool kernel = mip_kernel_form(etc1 ? kMipPyramidMode : in.mode, in.comps, in.filter).exists && !(etc1 && in.comps < 3);
  plan.form = !kernel ? kMipRefused : in.n_images == 0 || plan.n_passes + plan.n_encodes == 0 ? kMipNothing : kMipLaunch;
  if (plan.form != kMipLaunch) plan.n_passes = plan.n_encodes = 0;
  return plan;
}

}  // namespace icamd
#endif  // ICAMD_MIP_PLAN_H_
