// pvrtc_plan_driver.cc -- prints what image-compression_amd/csrc/pvrtc_plan.h answers over the grid of
// tests/test_pvrtc_plan_host.py, every field of every plan.  Built with g++ alone: the header needs nothing from HIP.
//
// Output: a "# bpp log2_size n_images compute_units aligned region_first region_blocks" line per input, then one line per
// (mode, strip) below it: "mode strip <plan>", where <plan> is
//   R                                                    refused
//   path rx0 ry0 log2_rw log2_rh z_first log2_strip stage_stores log2_wgc lanes workgroups lds_bytes lds_opt_in_bytes
//        group workspace_bytes encode F <chunk> T <chunk>      chunk: count total_blocks total_strips morph grid_x grid_y encode_grid, or - (none)
//   =                                                    every field as on the line above
#include <cstdio>
#include <string>
#include <vector>

#include "pvrtc_plan.h"

using namespace icamd;

static const int kModes[][2] = { {0, -1}, {0, 4}, {1, -1}, {2, -1}, {2, 0}, {2, 1}, {2, 2}, {2, 4}, {2, 6}, {2, 9}, {2, 20} };
static const uint32_t kImages[] = { 1, 2, 3, 5, 16, 64, 257, 4096, 65536 };
static const uint32_t kComputeUnits[] = { 32, 256, 304 };

static std::string chunk_text(const PvrtcPairChunk &c) {
  if (c.count == 0) return "-";
  char b[160];
  snprintf(b, sizeof b, "%llu %u %u %d %u %u %u", (unsigned long long)c.count, c.total_blocks, c.total_strips, c.morph, c.morph_grid_x,
           c.morph_grid_y, c.encode_grid);
  return b;
}
static std::string plan_text(const PvrtcPlan &p) {
  if (p.path == kPvrtcRefused) return "R";
  char b[320];
  snprintf(b, sizeof b, "%d %u %u %u %u %u %u %u %u %u %u %zu %zu %llu %zu %d F ", p.path, p.rx0, p.ry0, p.log2_rw, p.log2_rh, p.z_first,
           p.log2_strip, p.stage_stores, p.log2_wgc, p.lanes, p.workgroups, p.lds_bytes, p.lds_opt_in_bytes,
           (unsigned long long)p.group, p.workspace_bytes, p.encode);
  return std::string(b) + chunk_text(p.full) + " T " + chunk_text(p.tail);
}

static void emit(uint32_t bpp, uint32_t log2_size, uint32_t n_images, uint32_t first, uint32_t blocks) {
  for (uint32_t cu : kComputeUnits)
    for (int aligned = 0; aligned < 2; ++aligned) {
      printf("# %u %u %u %u %d %u %u\n", bpp, log2_size, n_images, cu, aligned, first, blocks);
      std::string prev;
      for (const auto &ms : kModes) {
        const PvrtcPlanIn in = { bpp, log2_size, n_images, first, blocks, ms[0], ms[1], cu, aligned != 0 };
        const std::string t = plan_text(pvrtc_plan(in));
        printf("%d %d %s\n", ms[0], ms[1], t == prev ? "=" : t.c_str());
        prev = t;
      }
    }
}

int main() {
  // whole textures
  for (uint32_t bpp = 2; bpp <= 4; bpp += 2)
    for (uint32_t log2_size = 3; log2_size <= 15; ++log2_size)
      for (uint32_t n : kImages) emit(bpp, log2_size, n, 0, 0);
  // regions of one 2 bpp texture
  static const uint32_t kRegionSizes[] = { 3, 6, 10, 12, 13 };
  for (uint32_t log2_size : kRegionSizes) {
    const uint32_t log2_bpi = 2 * log2_size - 5, bpi = 1u << log2_bpi;
    for (uint32_t m = 0; m <= log2_bpi; ++m) {
      const uint32_t blocks = 1u << m;
      // the first range, the last, one in the middle; a start that is no multiple of the size; a range past the image's end
      std::vector<uint32_t> firsts = { 0, bpi - blocks, (bpi / blocks / 2) * blocks, (bpi / blocks / 2) * blocks + blocks / 2, bpi };
      for (size_t i = 0; i < firsts.size(); ++i) {
        bool seen = false;
        for (size_t j = 0; j < i; ++j) seen = seen || firsts[j] == firsts[i];
        if (!seen) emit(2, log2_size, 1, firsts[i], blocks);
      }
    }
    emit(2, log2_size, 1, 0, 3);  // no power of two
    emit(2, log2_size, 2, 0, 1);  // a region of more than one image
  }
  emit(4, 10, 1, 0, 64);  // 4 bpp has no regions
  return 0;
}
