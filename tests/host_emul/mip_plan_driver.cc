// mip_plan_driver.cc -- prints what image-compression_amd/csrc/mip_plan.h answers over the grid of tests/test_mip_plan_host.py,
// every field of every plan.  Built with g++ alone: the header needs nothing from HIP.
//
// Output:
//   "K name mode comps filter" per row of the kernel list, then "k mode comps filter exists name" for every combination asked;
//   "S codec h w levels : chain offsets" and "Q comps h w levels : pyramid offsets" for one image's sizes;
//   "# label mode comps filter h w levels n_images row_stride src_image_stride dst_image_stride" per input (label: the line of the
//   golden file the input is hashed under), then
//   "= form workspace_bytes n_passes n_encodes", and per pass
//   "P l0 n handoff in.base in.offset in_row_stride in_image_stride height width enc_mask pix_mask pix.base pix.offset
//      pix_image_stride dst_image_stride L level_off x 8 X pix_off x 8 G grid_x tile_rows n_images Y first+count ... Z first+count ..."
//   (the launches: every Z piece, and within it every Y piece), and per ETC1 encode call
//   "E height width in.base in.offset in_row_stride in_image_stride out_offset".
#include <cstdio>

#include "mip_plan.h"

using namespace icamd;

typedef unsigned long long ull;

static const int kModes[] = { ICAMD_DXT1, ICAMD_DXT5, ICAMD_ETC1, ICAMD_BC4, ICAMD_BC5, kMipPyramidMode };
static const char *const kModeNames[] = { "dxt1", "dxt5", "etc1", "bc4", "bc5", "pyramid" };
static const uint32_t kShapes[][2] = { {1, 1}, {1, 7}, {2, 3}, {61, 59}, {128, 128}, {129, 127}, {129, 1}, {256, 256}, {257, 255},
                                       {1, 8192}, {1, 16384}, {16385, 3}, {4096, 4096}, {16384, 16384}, {65536, 65536},
                                       {8388481, 1}, {8388480, 1}, {1, 1u << 31} };
static const uint32_t kLevels[] = { 1, 6, 7, 8, 12, 13, 14, 0 };  // 0: the full chain
static const uint32_t kImages[] = { 0, 1, 3, 65535, 65536, 70000 };

static void emit(const char *label, const MipChainIn &in) {
  printf("# %s %d %d %d %u %u %u %u %u %llu %llu\n", label, in.mode, in.comps, in.filter, in.height, in.width, in.levels, in.n_images,
         in.row_stride, (ull)in.src_image_stride, (ull)in.dst_image_stride);
  const MipChainPlan p = mip_chain_plan(in);
  printf("= %d %llu %u %u\n", p.form, (ull)p.workspace_bytes, p.n_passes, p.n_encodes);
  for (uint32_t i = 0; i < p.n_passes; ++i) {
    const MipPassPlan &P = p.pass[i];
    printf("P %u %u %d %d %llu %u %llu %u %u %u %u %d %llu %llu %llu L", P.l0, P.n, (int)P.handoff, P.in.base, (ull)P.in.offset,
           P.in_row_stride, (ull)P.in_image_stride, P.height, P.width, P.enc_mask, P.pix_mask, P.pix.base, (ull)P.pix.offset,
           (ull)P.pix_image_stride, (ull)P.dst_image_stride);
    for (int j = 0; j < 8; ++j) printf(" %llu", (ull)P.level_off[j]);
    printf(" X");
    for (int j = 0; j < 8; ++j) printf(" %llu", (ull)P.pix_off[j]);
    printf(" G %u %u %u Y", P.grid_x, P.tile_rows, P.n_images);
    for (uint32_t y = 0; y < mip_pieces(P.tile_rows); ++y) printf(" %u+%u", mip_piece(P.tile_rows, y).first, mip_piece(P.tile_rows, y).count);
    printf(" Z");
    for (uint32_t z = 0; z < mip_pieces(P.n_images); ++z) printf(" %u+%u", mip_piece(P.n_images, z).first, mip_piece(P.n_images, z).count);
    printf("\n");
  }
  for (uint32_t i = 0; i < p.n_encodes; ++i) {
    const MipEncodeCall &E = p.encode[i];
    printf("E %u %u %d %llu %u %llu %llu\n", E.height, E.width, E.in.base, (ull)E.in.offset, E.in_row_stride, (ull)E.in_image_stride,
           (ull)E.out_offset);
  }
}

int main() {
#define ROW(name, mode, comps, filter) printf("K %s %d %d %d\n", #name, (int)(mode), comps, filter);
  ICAMD_MIP_KERNELS(ROW)
#undef ROW
  for (int mode : kModes)
    for (int comps = 0; comps <= 5; ++comps)
      for (int filter = -1; filter <= 5; ++filter) {
        const MipKernelForm f = mip_kernel_form(mode, comps, filter);
        printf("k %d %d %d %d %s\n", mode, comps, filter, (int)f.exists, f.exists ? f.name : "-");
      }
  size_t offsets[kMipMaxLevels + 2];
  for (const auto &s : kShapes) {
    const uint32_t top = mip_max_levels(s[0], s[1]);
    for (uint32_t lv : kLevels) {
      const uint32_t levels = lv ? lv : top;
      if (levels > top || (lv && lv == top)) continue;
      for (int mode : kModes) {
        if (mode == kMipPyramidMode) continue;
        printf("S %d %u %u %u : %llu :", mode, s[0], s[1], levels, (ull)mip_chain_bytes(mode, s[0], s[1], levels, offsets));
        for (uint32_t l = 0; l <= levels; ++l) printf(" %llu", (ull)offsets[l]);
        printf("\n");
      }
      for (int comps = 1; comps <= 4; ++comps) {
        printf("Q %d %u %u %u : %llu :", comps, s[0], s[1], levels, (ull)mip_pyramid_bytes(s[0], s[1], levels, comps, offsets));
        for (uint32_t l = 1; l <= levels; ++l) printf(" %llu", (ull)offsets[l]);
        printf("\n");
      }
    }
  }
  char label[64];
  for (size_t m = 0; m < sizeof kModes / sizeof kModes[0]; ++m)
    for (int comps = 1; comps <= 4; ++comps)
      for (int filter = 0; filter < (int)kMipFilters; ++filter) {
        snprintf(label, sizeof label, "%s/c%d/f%d", kModeNames[m], comps, filter);
        for (const auto &s : kShapes) {
          const uint32_t top = mip_max_levels(s[0], s[1]);
          for (uint32_t lv : kLevels) {
            const uint32_t levels = lv ? lv : top;
            if (levels > top || (lv && lv == top)) continue;
            for (uint32_t n : kImages) {
              // the caller's strides: rows padded by 5 bytes and images 40 / 24 bytes wider than an image where n is 3, tight otherwise
              const uint64_t row = (uint64_t)s[1] * (uint32_t)comps + (n == 3 ? 5u : 0u);
              const uint64_t out = kModes[m] == kMipPyramidMode ? mip_pyramid_bytes(s[0], s[1], levels, comps)
                                                                : mip_chain_bytes(kModes[m], s[0], s[1], levels, nullptr);
              const MipChainIn in = { kModes[m], comps, filter, s[0], s[1], levels, n, (uint32_t)row,
                                      row * s[0] + (n == 3 ? 40u : 0u), out + (n == 3 ? 24u : 0u) };
              emit(label, in);
            }
          }
        }
      }
  return 0;
}
