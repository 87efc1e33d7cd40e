// bptc_mip_plan_driver.cc -- prints the plans of image-compression_amd/csrc/bptc_mip_plan.h over a grid of inputs, for
// tests/test_bptc_mip_plan_host.py.  Built with g++ against the header alone (no HIP); the test also builds it with
// -fsanitize=address,undefined and runs it once.
//
// Per case:
//   # codec chans filter modes h w levels n_images row_stride src_image_stride dst_image_stride
//   = form workspace pyramid_image_stride chain_bytes grid_x n_images n_passes
//   P l0 n handoff in_base in_offset in_row_stride height width pix_mask pix_base pix_image_stride grid_x tile_rows   per pyramid pass
//   L k level pix_offset dst_offset row_stride h w block_rows block_cols log2_tile_cols force_gather tiles_per_row n_tiles first_wg
//   C covered blocks max_hits   every workgroup of grid.x located with etc2_mip_locate, every lane mapped to its block as
//                               locate_tile does ON THE TILE SHAPE encode_tile_shape(block_cols, row_stride, 8) GIVES THAT LEVEL
//                               ALONE (not the table's copy of it): blocks hit, blocks there are, the most hits on one block
// Exit status 1 where a located workgroup lies outside its level's tile grid.
#include <cstdio>
#include <vector>

#include "bptc_mip_plan.h"

using namespace icamd;

static int g_bad = 0;

static void coverage(const BptcMipPlan &plan) {
  unsigned long long covered = 0, blocks = 0;
  unsigned max_hits = 0;
  std::vector<std::vector<unsigned char>> hits(plan.table.n_levels);
  for (uint32_t k = 0; k < plan.table.n_levels; ++k) {
    const Etc2MipLevel &L = plan.table.level[k];
    hits[k].assign((size_t)L.block_rows * L.block_cols, 0);
    blocks += (unsigned long long)L.block_rows * L.block_cols;
  }
  for (uint32_t wg = 0; wg < plan.grid_x; ++wg) {
    const Etc2MipSpot s = etc2_mip_locate(plan.table, wg);
    if (s.entry >= plan.table.n_levels) {
      ++g_bad;
      continue;
    }
    const Etc2MipLevel &L = plan.table.level[s.entry];
    const TileShape shape = encode_tile_shape(L.block_cols, L.row_stride, 8u);  // what launch_tiled gives the level alone
    const uint32_t cols = 1u << shape.log2_tile_cols, rows = 256u >> shape.log2_tile_cols;
    if ((uint64_t)s.tile_col * cols >= L.block_cols || (uint64_t)s.tile_row * rows >= L.block_rows) ++g_bad;
    for (uint32_t tid = 0; tid < 256u; ++tid) {  // locate_tile of ic_device.h
      const uint32_t bcol = s.tile_col * cols + (tid & (cols - 1u)), brow = s.tile_row * rows + (tid >> shape.log2_tile_cols);
      if (bcol < L.block_cols && brow < L.block_rows) {
        unsigned char &h = hits[s.entry][(size_t)brow * L.block_cols + bcol];
        if (h < 255) ++h;
      }
    }
  }
  for (const auto &level : hits)
    for (unsigned char h : level) {
      covered += h != 0;
      if (h > max_hits) max_hits = h;
    }
  printf("C %llu %llu %u\n", covered, blocks, max_hits);
}

static void one(int codec, int chans, int filter, int modes, uint32_t h, uint32_t w, uint32_t levels, uint32_t n) {
  const bool pad = n == 3;
  const uint32_t row_stride = w * bptc_mip_pixel_bytes(codec, chans) + (pad ? 6u : 0u);
  const uint64_t src_image_stride = (uint64_t)row_stride * h + (pad ? 40u : 0u);
  const uint64_t dst_image_stride = bptc_mip_chain_bytes(codec, h, w, levels, nullptr) + (pad ? 32u : 0u);
  const BptcMipIn in = { codec, chans, filter, modes, h, w, levels, n, row_stride, src_image_stride, dst_image_stride };
  const BptcMipPlan plan = bptc_mip_plan(in);
  printf("# %d %d %d %d %u %u %u %u %u %llu %llu\n", codec, chans, filter, modes, h, w, levels, n, row_stride,
         (unsigned long long)src_image_stride, (unsigned long long)dst_image_stride);
  printf("= %d %llu %llu %llu %u %u %u\n", plan.form, (unsigned long long)plan.workspace_bytes,
         (unsigned long long)plan.pyramid_image_stride, (unsigned long long)plan.chain_bytes, plan.grid_x, plan.n_images,
         plan.pyramid.n_passes);
  if (plan.form != kMipLaunch) return;
  for (uint32_t k = 0; k < plan.pyramid.n_passes; ++k) {
    const MipPassPlan &p = plan.pyramid.pass[k];
    printf("P %u %u %d %d %llu %u %u %u %u %d %llu %u %u\n", p.l0, p.n, (int)p.handoff, p.in.base, (unsigned long long)p.in.offset,
           p.in_row_stride, p.height, p.width, p.pix_mask, p.pix.base, (unsigned long long)p.pix_image_stride, p.grid_x, p.tile_rows);
  }
  for (uint32_t k = 0; k < plan.table.n_levels; ++k) {
    const Etc2MipLevel &L = plan.table.level[k];
    printf("L %u %u %llu %llu %u %u %u %u %u %u %u %u %u %u\n", k, L.level, (unsigned long long)L.pix_offset,
           (unsigned long long)L.dst_offset, L.row_stride, L.height, L.width, L.block_rows, L.block_cols, L.log2_tile_cols,
           L.force_gather, L.tiles_per_row, L.n_tiles, plan.table.first_wg[k]);
  }
  if ((uint64_t)plan.grid_x * 256u <= (1ull << 22)) coverage(plan);
}

int main() {
  static const uint32_t kShapes[][2] = { { 1, 1 }, { 4, 4 }, { 37, 21 }, { 8, 516 }, { 516, 8 }, { 4, 2056 }, { 64, 64 }, { 300, 200 },
                                         { 4096, 4096 }, { 4, 1u << 20 } };
  static const struct { int codec, chans, filter, modes; } kForms[] = {
    { ICAMD_BC7, 3, 0, 0 }, { ICAMD_BC7, 4, 3, 0 }, { ICAMD_BC7, 3, 1, 1 }, { ICAMD_BC7, 4, 0, 1 },
    { ICAMD_BC6H_UF16, 3, 0, 0 }, { ICAMD_BC6H_UF16, 4, 0, 1 }, { ICAMD_BC6H_SF16, 3, 0, 1 }, { ICAMD_BC6H_SF16, 4, 0, 0 },
    // refused: a codec outside the three, channels without a kernel, modes outside 0 / 1, a filter without a pyramid kernel
    { ICAMD_ETC1, 3, 0, 0 }, { ICAMD_BC7, 2, 0, 0 }, { ICAMD_BC6H_UF16, 2, 0, 0 }, { ICAMD_BC7, 4, 0, 2 }, { ICAMD_BC7, 3, 2, 0 } };
  static const uint32_t kImages[] = { 0, 1, 3, 65537 };
  for (const auto &f : kForms)
    for (const auto &s : kShapes) {
      const uint32_t top = mip_max_levels(s[0], s[1]);
      const uint32_t levels[] = { 1, 3, 7, 8, top, top + 1 };
      for (uint32_t l : levels) {
        if (l != top && l != top + 1 && l >= top) continue;
        for (uint32_t n : kImages) one(f.codec, f.chans, f.filter, f.modes, s[0], s[1], l, n);
      }
    }
  return g_bad ? 1 : 0;
}
