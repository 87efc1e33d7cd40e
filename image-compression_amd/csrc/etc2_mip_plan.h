// etc2_mip_plan.h -- what icamd_encode_etc2_mips_device launches: the pixel-pyramid passes (mip_plan.h's, into the workspace), and
// ONE encode launch over every level of every image, whose workgroups find their level in a table.
//
// Host-only arithmetic on a handful of integers: no HIP header, no runtime call, no allocation.  ic_capi.hip makes one plan per
// call and walks it; etc2_mip_kernels.hip defines its kernels from the list below, fills the kernel argument from the plan's
// table and looks a workgroup up with etc2_mip_locate -- the same function tests/host_emul/etc2_mip_plan_driver.cc and
// etc2_mip_emul.cc run with g++, over every workgroup of a grid of shapes.
#ifndef ICAMD_ETC2_MIP_PLAN_H_
#define ICAMD_ETC2_MIP_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "codec_info.h"
#include "mip_plan.h"

#if defined(__HIPCC__)
#define ICAMD_PLAN_HD __host__ __device__
#else
#define ICAMD_PLAN_HD
#endif

namespace icamd {

// ---- the tile shape of the block encoders (launch_tiled, ic_launch.h) ----
// The smallest power of two that covers a block row, at most 256.
inline uint32_t tile_log2_cols(uint32_t block_cols) {
  uint32_t l = 0;
  while (l < 8 && (1u << l) < block_cols) ++l;
  return l;
}
// A workgroup covers 2^log2_tile_cols x (256 >> log2_tile_cols) blocks: tile_log2_cols, at most max_log2_cols (4 for the ETC2
// family: 16 x 16).  A lane addresses its block with a 32-bit offset from the tile's (64-bit, uniform) origin: up to 4 * 256 - 1
// rows of stride in a 1 x 256 tile.  Rows of 4 MiB and more (or grids of 2^20 block columns and more, for the output offset) get
// 256 x 1 tiles, where the offset is at most three rows; rows of more than a third of 4 GiB take the 64-bit clamp-to-edge gather
// for every block (GridParams::force_gather).
struct TileShape {
  uint32_t log2_tile_cols, force_gather;
};
inline TileShape encode_tile_shape(uint32_t block_cols, uint32_t row_stride, uint32_t max_log2_cols) {
  TileShape s;
  s.log2_tile_cols = tile_log2_cols(block_cols);
  if (s.log2_tile_cols > max_log2_cols) s.log2_tile_cols = max_log2_cols;
  if ((uint64_t)row_stride * 1024u >= (1ull << 32) || (uint64_t)block_cols * 4096u >= (1ull << 32)) s.log2_tile_cols = 8;
  s.force_gather = (uint64_t)row_stride * 3u + 8192u >= (1ull << 32) ? 1u : 0u;
  return s;
}

// ---- the kernel list: X(kernel name, per-level twin, codec, source components, strategy, T/H pass) ----
// One chain form per ETC2-family encode kernel; strategy as icamd_encode_device reads it (0 split horizontally, 1 split
// vertically, 2 smaller error, 3 heuristic; any other value is 2), -1 where the codec does not read it.
#define ICAMD_ETC2_MIP_KERNELS(X)                                                                                         \
  X(icamd_etc2_mip_rgb8_rgb888_split_h_kernel, icamd_etc2_rgb8_rgb888_split_h_kernel, ICAMD_ETC2_RGB8, 3, 0, 0)           \
  X(icamd_etc2_mip_rgb8_rgb888_split_v_kernel, icamd_etc2_rgb8_rgb888_split_v_kernel, ICAMD_ETC2_RGB8, 3, 1, 0)           \
  X(icamd_etc2_mip_rgb8_rgb888_kernel, icamd_etc2_rgb8_rgb888_kernel, ICAMD_ETC2_RGB8, 3, 2, 0)                           \
  X(icamd_etc2_mip_rgb8_rgb888_heuristic_kernel, icamd_etc2_rgb8_rgb888_heuristic_kernel, ICAMD_ETC2_RGB8, 3, 3, 0)       \
  X(icamd_etc2_mip_rgb8_rgba8_split_h_kernel, icamd_etc2_rgb8_rgba8_split_h_kernel, ICAMD_ETC2_RGB8, 4, 0, 0)             \
  X(icamd_etc2_mip_rgb8_rgba8_split_v_kernel, icamd_etc2_rgb8_rgba8_split_v_kernel, ICAMD_ETC2_RGB8, 4, 1, 0)             \
  X(icamd_etc2_mip_rgb8_rgba8_kernel, icamd_etc2_rgb8_rgba8_kernel, ICAMD_ETC2_RGB8, 4, 2, 0)                             \
  X(icamd_etc2_mip_rgb8_rgba8_heuristic_kernel, icamd_etc2_rgb8_rgba8_heuristic_kernel, ICAMD_ETC2_RGB8, 4, 3, 0)         \
  X(icamd_etc2_mip_th_rgb888_kernel, icamd_etc2_th_rgb888_kernel, ICAMD_ETC2_RGB8, 3, -1, 1)                              \
  X(icamd_etc2_mip_th_rgba8_kernel, icamd_etc2_th_rgba8_kernel, ICAMD_ETC2_RGB8, 4, -1, 1)                                \
  X(icamd_etc2_mip_rgba8_split_h_kernel, icamd_etc2_rgba8_split_h_kernel, ICAMD_ETC2_RGBA8, 4, 0, 0)                      \
  X(icamd_etc2_mip_rgba8_split_v_kernel, icamd_etc2_rgba8_split_v_kernel, ICAMD_ETC2_RGBA8, 4, 1, 0)                      \
  X(icamd_etc2_mip_rgba8_kernel, icamd_etc2_rgba8_kernel, ICAMD_ETC2_RGBA8, 4, 2, 0)                                      \
  X(icamd_etc2_mip_rgba8_heuristic_kernel, icamd_etc2_rgba8_heuristic_kernel, ICAMD_ETC2_RGBA8, 4, 3, 0)                  \
  X(icamd_etc2_mip_rgb8a1_split_h_kernel, icamd_etc2_rgb8a1_split_h_kernel, ICAMD_ETC2_RGB8A1, 4, 0, 0)                   \
  X(icamd_etc2_mip_rgb8a1_split_v_kernel, icamd_etc2_rgb8a1_split_v_kernel, ICAMD_ETC2_RGB8A1, 4, 1, 0)                   \
  X(icamd_etc2_mip_rgb8a1_kernel, icamd_etc2_rgb8a1_kernel, ICAMD_ETC2_RGB8A1, 4, 2, 0)                                   \
  X(icamd_etc2_mip_rgb8a1_heuristic_kernel, icamd_etc2_rgb8a1_heuristic_kernel, ICAMD_ETC2_RGB8A1, 4, 3, 0)               \
  X(icamd_etc2_mip_r11_r8_kernel, icamd_eac_r11_r8_kernel, ICAMD_EAC_R11, 1, -1, 0)                                       \
  X(icamd_etc2_mip_r11_rg8_kernel, icamd_eac_r11_rg8_kernel, ICAMD_EAC_R11, 2, -1, 0)                                     \
  X(icamd_etc2_mip_r11_rgb888_kernel, icamd_eac_r11_rgb888_kernel, ICAMD_EAC_R11, 3, -1, 0)                               \
  X(icamd_etc2_mip_r11_rgba8_kernel, icamd_eac_r11_rgba8_kernel, ICAMD_EAC_R11, 4, -1, 0)                                 \
  X(icamd_etc2_mip_rg11_rg8_kernel, icamd_eac_rg11_rg8_kernel, ICAMD_EAC_RG11, 2, -1, 0)                                  \
  X(icamd_etc2_mip_rg11_rgb888_kernel, icamd_eac_rg11_rgb888_kernel, ICAMD_EAC_RG11, 3, -1, 0)                            \
  X(icamd_etc2_mip_rg11_rgba8_kernel, icamd_eac_rg11_rgba8_kernel, ICAMD_EAC_RG11, 4, -1, 0)

inline bool etc2_mip_codec(int codec) {
  return codec == ICAMD_ETC2_RGBA8 || codec == ICAMD_ETC2_RGB8 || codec == ICAMD_ETC2_RGB8A1 || codec == ICAMD_EAC_R11 ||
         codec == ICAMD_EAC_RG11;
}
// A row's place in ICAMD_ETC2_MIP_KERNELS, or -1: the index of etc2_mip_kernels.hip's pointer table.  th: the T / H pass.
inline int etc2_mip_kernel_index(int codec, int comps, int etc_strategy, bool th) {
  const bool eac = codec == ICAMD_EAC_R11 || codec == ICAMD_EAC_RG11;
  const int strategy = eac || th ? -1 : etc_strategy >= 0 && etc_strategy < 4 ? etc_strategy : 2;
  int i = 0;
#define ICAMD_ETC2_MIP_MATCH(name, twin, c, n, s, t) \
  if (codec == (c) && comps == (n) && strategy == (s) && th == ((t) != 0)) return i; \
  ++i;
  ICAMD_ETC2_MIP_KERNELS(ICAMD_ETC2_MIP_MATCH)
#undef ICAMD_ETC2_MIP_MATCH
  return -1;
}
inline const char *etc2_mip_kernel_form(int codec, int comps, int etc_strategy, bool th) {  // "" where there is no kernel
#define ICAMD_ETC2_MIP_NAME(name, twin, c, n, s, t) #name,
  static const char *const kNames[] = { ICAMD_ETC2_MIP_KERNELS(ICAMD_ETC2_MIP_NAME) };
#undef ICAMD_ETC2_MIP_NAME
  const int i = etc2_mip_kernel_index(codec, comps, etc_strategy, th);
  return i >= 0 ? kNames[i] : "";
}

// One image's encoded chain, as mip_chain_bytes (which knows the DXT / ETC1 / BC4 / BC5 chains only and must keep answering 0
// for these codecs): its bytes, level l at offsets[l] (levels + 1 entries; may be null).
inline size_t etc2_mip_chain_bytes(int codec, uint32_t h, uint32_t w, uint32_t levels, size_t *offsets) {
  if (!etc2_mip_codec(codec) || levels == 0 || levels > mip_max_levels(h, w)) return 0;
  size_t total = 0;
  for (uint32_t l = 0; l < levels; ++l) {
    if (offsets) offsets[l] = total;
    total += mip_level_blocks(codec, h, w, l);
  }
  if (offsets) offsets[levels] = total;
  return total;
}

// ---- the level table: what the encode kernel receives (by value, in the kernel argument: scalar data) ----
// Entry k is the k-th level IN LAUNCH ORDER: its workgroups are [first_wg[k], first_wg[k + 1]) of grid.x, tile t of the level
// (row-major over its tile grid) at first_wg[k] + t.
struct Etc2MipLevel {
  uint64_t pix_offset;   // its pixels: bytes from the source (level 0) or from the image's pyramid in the workspace
  uint64_t dst_offset;   // its blocks: bytes from the image's chain
  uint32_t level;        // which level this is (0: read from the source, with the source's strides)
  uint32_t row_stride;   // bytes between its pixel rows
  uint32_t height, width, block_rows, block_cols;
  uint32_t log2_tile_cols, force_gather;  // encode_tile_shape
  uint32_t tiles_per_row, n_tiles;
  uint32_t div_mul, div_shift;  // t / tiles_per_row = (umulhi(t, div_mul) + t) >> div_shift for t < 2^31
};
struct Etc2MipTable {
  uint32_t n_levels;
  uint32_t bulk_entry, bulk_first, bulk_tiles;  // the entry of level 0, its first_wg and n_tiles: etc2_mip_locate's first look
  uint32_t first_wg[kMipMaxLevels + 1];  // first_wg[n_levels] = grid.x
  Etc2MipLevel level[kMipMaxLevels];
};
// Where a workgroup works: the entry of its level and its tile there.
struct Etc2MipSpot {
  uint32_t entry, tile_col, tile_row;
};
// wg < first_wg[n_levels].  Every operand is workgroup-uniform in the kernel (blockIdx.x and the kernel argument), so the search
// and the division run on the scalar unit.
ICAMD_PLAN_HD inline Etc2MipSpot etc2_mip_locate(const Etc2MipTable &T, uint32_t wg) {
  // Three workgroups in four belong to level 0, wherever it stands in the order: one comparison finds them, the others search.
  uint32_t k = T.bulk_entry;
  if (wg - T.bulk_first >= T.bulk_tiles) {
    k = 0;
    while (k + 1u < T.n_levels && T.first_wg[k + 1u] <= wg) ++k;
  }
  const Etc2MipLevel &L = T.level[k];
  const uint32_t t = wg - T.first_wg[k];
  Etc2MipSpot s;
  s.entry = k;
  s.tile_row = ((uint32_t)(((uint64_t)t * L.div_mul) >> 32) + t) >> L.div_shift;
  s.tile_col = t - s.tile_row * L.tiles_per_row;
  return s;
}

// ---- the plan ----
enum Etc2MipOrder : int { kEtc2MipSmallestFirst = 0, kEtc2MipLargestFirst = 1 };  // of the levels inside grid.x

struct Etc2MipIn {
  int codec, comps, filter, modes;  // modes: ICAMD_ETC2_MODES_*
  uint32_t height, width, levels, n_images;
  uint32_t row_stride;                          // of the source
  uint64_t src_image_stride, dst_image_stride;  // the caller's
  int order;                                    // Etc2MipOrder
};
struct Etc2MipPlan {
  int form;                // MipForm: kMipRefused (no such chain, or a grid.x of 2^31 and more), kMipNothing (no image), kMipLaunch
  size_t workspace_bytes;  // the pixel pyramid of every image, whenever the chain exists
  uint64_t pyramid_image_stride;  // bytes between the images' pyramids in the workspace
  size_t chain_bytes;
  // the pixel pyramid into the workspace: pyramid.pass[0 .. pyramid.n_passes), exactly the passes of an ETC1 chain
  MipChainPlan pyramid;
  // the encode launch: grid.x = the table's workgroups of one image; images in grid.y, in pieces of at most kMipGridLimitYZ
  // (mip_piece); with `th` a second launch of the same grid, the T / H pass
  Etc2MipTable table;
  uint32_t grid_x, n_images;
  bool th;
};

// Fills the table for `levels` levels of a height x width image in the given order and returns the workgroups of one image
// (grid.x), or 0 where they are 2^31 and more (an image of some 2^43 pixels): the table is then filled up to the level that
// crossed the limit.  Level 0 has the source's row stride, the others tight rows of pixel_bytes per pixel at pixel_off[l] of the
// image's pyramid; every level gets the tile shape launch_tiled gives it alone (encode_tile_shape with max_log2_cols).
inline uint32_t etc2_mip_fill_table(Etc2MipTable &T, uint32_t height, uint32_t width, uint32_t levels, int order, uint32_t row_stride,
                                    uint32_t pixel_bytes, const size_t *pixel_off, const size_t *block_off, uint32_t max_log2_cols) {
  T.n_levels = levels;
  uint64_t wg = 0;
  for (uint32_t k = 0; k < levels; ++k) {
    const uint32_t l = order == kEtc2MipLargestFirst ? k : levels - 1u - k;
    Etc2MipLevel &L = T.level[k];
    L.level = l;
    L.height = mip_dim(height, l);
    L.width = mip_dim(width, l);
    L.block_rows = (uint32_t)(((uint64_t)L.height + 3u) / 4u);
    L.block_cols = (uint32_t)(((uint64_t)L.width + 3u) / 4u);
    L.pix_offset = l == 0 ? 0 : pixel_off[l];
    L.row_stride = l == 0 ? row_stride : L.width * pixel_bytes;
    L.dst_offset = block_off[l];
    const TileShape shape = encode_tile_shape(L.block_cols, L.row_stride, max_log2_cols);
    L.log2_tile_cols = shape.log2_tile_cols;
    L.force_gather = shape.force_gather;
    const uint32_t cols = 1u << L.log2_tile_cols, rows = 256u >> L.log2_tile_cols;
    L.tiles_per_row = (uint32_t)(((uint64_t)L.block_cols + cols - 1u) / cols);
    const uint64_t tile_rows = ((uint64_t)L.block_rows + rows - 1u) / rows;
    const uint64_t n_tiles = tile_rows * L.tiles_per_row;
    // the division by tiles_per_row (ic_device.h make_fastdiv): exact for a dividend below 2^31
    uint32_t s = 0;
    while ((1ull << s) < L.tiles_per_row) ++s;
    L.div_shift = s;
    L.div_mul = (uint32_t)(((1ull << 32) * ((1ull << s) - L.tiles_per_row)) / L.tiles_per_row + 1u);
    T.first_wg[k] = (uint32_t)wg;
    if (l == 0) {
      T.bulk_entry = k;
      T.bulk_first = (uint32_t)wg;
      T.bulk_tiles = (uint32_t)n_tiles;  // (below 2^31, or the plan is refused below)
    }
    wg += n_tiles;
    if (wg >= (1ull << 31)) return 0;  // more workgroups than a grid's x holds
    L.n_tiles = (uint32_t)n_tiles;
  }
  T.first_wg[levels] = (uint32_t)wg;
  return (uint32_t)wg;
}

inline Etc2MipPlan etc2_mip_plan(const Etc2MipIn &in) {
  Etc2MipPlan plan = {};
  plan.form = kMipRefused;
  if (!etc2_mip_codec(in.codec) || in.comps < 1 || in.comps > 4 || in.levels == 0 || in.levels > mip_max_levels(in.height, in.width))
    return plan;
  size_t block_off[kMipMaxLevels + 1], pixel_off[kMipMaxLevels + 1];
  plan.chain_bytes = etc2_mip_chain_bytes(in.codec, in.height, in.width, in.levels, block_off);
  plan.pyramid_image_stride = mip_pyramid_bytes(in.height, in.width, in.levels, in.comps, pixel_off);
  plan.workspace_bytes = (size_t)plan.pyramid_image_stride * in.n_images;
  plan.th = in.modes != 0;
  plan.n_images = in.n_images;
  if (in.levels > 1) {
    const MipChainIn pyr = { kMipPyramidMode, in.comps, in.filter, in.height, in.width, in.levels, in.n_images, in.row_stride,
                             in.src_image_stride, plan.pyramid_image_stride };
    (void)mip_plan_passes(pyr, false, kMipWorkspace, plan.pyramid_image_stride, nullptr, pixel_off, plan.pyramid);
  }
  plan.grid_x = etc2_mip_fill_table(plan.table, in.height, in.width, in.levels, in.order, in.row_stride, (uint32_t)in.comps, pixel_off,
                                    block_off, 4u);
  if (plan.grid_x == 0) {
    plan.pyramid.n_passes = 0;
    return plan;
  }
  const bool kernels = mip_kernel_form(kMipPyramidMode, in.comps, in.filter).exists &&
                       etc2_mip_kernel_index(in.codec, in.comps, 2, false) >= 0 &&
                       (!plan.th || etc2_mip_kernel_index(in.codec, in.comps, 2, true) >= 0);
  plan.form = !kernels ? kMipRefused : in.n_images == 0 ? kMipNothing : kMipLaunch;
  if (plan.form != kMipLaunch) plan.pyramid.n_passes = 0;
  return plan;
}

}  // namespace icamd
#endif  // ICAMD_ETC2_MIP_PLAN_H_
