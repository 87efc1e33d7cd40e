// etc2_mip_plan_driver.cc -- prints the plans of image-compression_amd/csrc/etc2_mip_plan.h over a grid of inputs, for
// tests/test_etc2_mip_plan_host.py.  Built with g++ against the header alone (no HIP).
//
// Per case:
//   # codec comps filter modes h w levels n_images row_stride src_image_stride dst_image_stride order
//   = form workspace pyramid_image_stride chain_bytes grid_x n_images th n_passes
//   P ...   one line per pyramid pass (the fields tests/host_emul/mip_plan_driver.cc prints, without the grid pieces)
//   R ...   the same line of the plan mip_chain_plan makes for the pixel pyramid of that geometry into a buffer of the same image
//           stride (ICAMD_ETC1 where it has a chain: 3 and 4 components)
//   L k level pix_offset dst_offset row_stride h w block_rows block_cols log2_tile_cols force_gather tiles_per_row n_tiles first_wg
//   Y first+count ...   the pieces of grid.y
//   C covered blocks max_hits   every workgroup of grid.x located with etc2_mip_locate, every lane mapped to its block as
//                               locate_tile does: blocks hit, blocks there are, the most hits on one block (printed for plans of at most 2^22 lanes)
#include <cstdio>
#include <vector>

#include "etc2_mip_plan.h"

using namespace icamd;

static void print_pass(char tag, const MipPassPlan &p) {
  printf("%c %u %u %d %d %llu %u %llu %u %u %u %u %d %llu %llu", tag, p.l0, p.n, (int)p.handoff, p.in.base, (unsigned long long)p.in.offset,
         p.in_row_stride, (unsigned long long)p.in_image_stride, p.height, p.width, p.enc_mask, p.pix_mask, p.pix.base,
         (unsigned long long)p.pix.offset, (unsigned long long)p.pix_image_stride);
  for (int j = 0; j < 8; ++j) printf(" %llu", (unsigned long long)p.pix_off[j]);
  printf(" %u %u %u\n", p.grid_x, p.tile_rows, p.n_images);
}

static void coverage(const Etc2MipPlan &plan) {
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
    const Etc2MipLevel &L = plan.table.level[s.entry];
    const uint32_t cols = 1u << L.log2_tile_cols, rows = 256u >> L.log2_tile_cols;
    for (uint32_t tid = 0; tid < 256u; ++tid) {  // locate_tile / locate_tile_lane of ic_device.h
      const uint32_t bcol = s.tile_col * cols + (tid & (cols - 1u)), brow = s.tile_row * rows + (tid >> L.log2_tile_cols);
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

static void one(int codec, int comps, int filter, int modes, uint32_t h, uint32_t w, uint32_t levels, uint32_t n, int order) {
  const bool pad = n == 3;
  const uint32_t row_stride = w * (uint32_t)comps + (pad ? 5u : 0u);
  const uint64_t src_image_stride = (uint64_t)row_stride * h + (pad ? 40u : 0u);
  const uint64_t dst_image_stride = etc2_mip_chain_bytes(codec, h, w, levels, nullptr) + (pad ? 24u : 0u);
  const Etc2MipIn in = { codec, comps, filter, modes, h, w, levels, n, row_stride, src_image_stride, dst_image_stride, order };
  const Etc2MipPlan plan = etc2_mip_plan(in);
  printf("# %d %d %d %d %u %u %u %u %u %llu %llu %d\n", codec, comps, filter, modes, h, w, levels, n, row_stride,
         (unsigned long long)src_image_stride, (unsigned long long)dst_image_stride, order);
  printf("= %d %llu %llu %llu %u %u %d %u\n", plan.form, (unsigned long long)plan.workspace_bytes,
         (unsigned long long)plan.pyramid_image_stride, (unsigned long long)plan.chain_bytes, plan.grid_x, plan.n_images, (int)plan.th,
         plan.pyramid.n_passes);
  if (plan.form != kMipLaunch) return;
  for (uint32_t k = 0; k < plan.pyramid.n_passes; ++k) print_pass('P', plan.pyramid.pass[k]);
  const MipChainIn ref_in = { comps >= 3 ? ICAMD_ETC1 : kMipPyramidMode, comps, filter, h, w, levels, n, row_stride, src_image_stride,
                              comps >= 3 ? dst_image_stride : plan.pyramid_image_stride };
  const MipChainPlan ref = mip_chain_plan(ref_in);
  for (uint32_t k = 0; k < ref.n_passes; ++k) print_pass('R', ref.pass[k]);
  for (uint32_t k = 0; k < plan.table.n_levels; ++k) {
    const Etc2MipLevel &L = plan.table.level[k];
    printf("L %u %u %llu %llu %u %u %u %u %u %u %u %u %u %u\n", k, L.level, (unsigned long long)L.pix_offset,
           (unsigned long long)L.dst_offset, L.row_stride, L.height, L.width, L.block_rows, L.block_cols, L.log2_tile_cols,
           L.force_gather, L.tiles_per_row, L.n_tiles, plan.table.first_wg[k]);
  }
  printf("Y");
  for (uint32_t i = 0; i < mip_pieces(plan.n_images); ++i) {
    const MipPiece p = mip_piece(plan.n_images, i);
    printf(" %u+%u", p.first, p.count);
  }
  printf("\n");
  if ((uint64_t)plan.grid_x * 256u <= (1ull << 22)) coverage(plan);
}

int main() {
  static const uint32_t kShapes[][2] = { { 1, 1 }, { 1, 37 }, { 37, 21 }, { 516, 8 }, { 8, 516 }, { 64, 64 }, { 256, 256 }, { 300, 200 },
                                         { 4096, 4096 }, { 16384, 4 }, { 4, 16384 }, { 1, 1u << 31 }, { 8388608, 2 } };
  static const struct { int codec, comps, filter, modes; } kForms[] = {
    { ICAMD_ETC2_RGBA8, 4, 0, 0 }, { ICAMD_ETC2_RGB8, 3, 0, 0 }, { ICAMD_ETC2_RGB8, 4, 3, 1 }, { ICAMD_ETC2_RGB8A1, 4, 2, 0 },
    { ICAMD_EAC_R11, 1, 0, 0 }, { ICAMD_EAC_RG11, 2, 4, 0 }, { ICAMD_EAC_RG11, 3, 0, 0 },
    // refused: a codec outside the family, components the codec has no kernel for, modes without a T / H kernel
    { ICAMD_ETC1, 3, 0, 0 }, { ICAMD_ETC2_RGBA8, 3, 0, 0 }, { ICAMD_EAC_RG11, 1, 0, 0 }, { ICAMD_EAC_R11, 1, 0, 1 } };
  static const uint32_t kImages[] = { 0, 1, 3, 65537 };
  for (const auto &f : kForms)
    for (const auto &s : kShapes) {
      const uint32_t top = mip_max_levels(s[0], s[1]);
      const uint32_t levels[] = { 1, 7, 8, top, top + 1 };
      for (uint32_t l : levels) {
        if (l != top && l != top + 1 && l >= top) continue;
        for (uint32_t n : kImages)
          for (int order = 0; order < 2; ++order) one(f.codec, f.comps, f.filter, f.modes, s[0], s[1], l, n, order);
      }
    }
  return 0;
}
