// blockops_plan_driver.cc -- prints what image-compression_amd/csrc/blockops_plan.h answers over the grid of
// tests/test_blockops_plan_host.py, every field of every plan.  Built with g++ alone: the header needs nothing from HIP.
//
// Output: a "# label op codec in_rows in_cols out_rows out_cols src_height src_width n_images" line per input (op: P pad,
// D downsample; label: the line of the golden file the input is hashed under), then one line per (strategy, quad switch):
//   "strategy quad form kernel_strategy out_per_image border border_lanes_per_image group F <group> T <group>"
//   group: count form total_out border_lanes border_wgs L <launch> L <launch>, or - (none)
//   launch: kernel grid_x grid_y grid_z lanes items items_per_image lanes_per_item, or - (none)
// and "= label what total ..." lines for the chunked launches: every launch of the loop, as the .hip file runs it.
#include <cstdio>
#include <string>

#include "blockops_plan.h"

using namespace icamd;

static std::string launch_text(const BlockOpLaunch &l) {
  if (l.kernel == kNoKernel) return "-";
  char b[160];
  snprintf(b, sizeof b, "%d %u %u %u %u %u %u %u", l.kernel, l.grid_x, l.grid_y, l.grid_z, l.lanes, l.items, l.items_per_image, l.lanes_per_item);
  return b;
}
static std::string group_text(const BlockOpGroup &g) {
  if (g.count == 0) return "-";
  char b[120];
  snprintf(b, sizeof b, "%u %d %u %u %u L ", g.count, g.form, g.total_out, g.border_lanes, g.border_wgs);
  return std::string(b) + launch_text(g.launch[0]) + " L " + launch_text(g.launch[1]);
}

static const uint32_t kStrategies[] = { 0, 1, 2, 3, 7 };  // 7: out of range, the reference's default: label

static void emit(const char *label, char op, int codec, uint32_t in_rows, uint32_t in_cols, uint32_t out_rows, uint32_t out_cols,
                 uint32_t src_height, uint32_t src_width, uint32_t n_images) {
  printf("# %s %c %d %u %u %u %u %u %u %u\n", label, op, codec, in_rows, in_cols, out_rows, out_cols, src_height, src_width, n_images);
  for (uint32_t strategy : kStrategies)
    for (int quad = 0; quad < 2; ++quad) {
      const BlockOpIn in = { codec, strategy, in_rows, in_cols, out_rows, out_cols, src_height, src_width, n_images, quad != 0 };
      const BlockOpPlan p = op == 'P' ? pad_plan(in) : downsample_plan(in);
      printf("%u %d %d %u %u %llu %u %llu F %s T %s\n", strategy, quad, p.form, p.strategy, p.out_per_image, (unsigned long long)p.border,
             p.border_lanes_per_image, (unsigned long long)p.group, group_text(p.full).c_str(), group_text(p.tail).c_str());
    }
}
static void emit_pad(const char *label, int codec, uint32_t in_rows, uint32_t in_cols, uint32_t out_rows, uint32_t out_cols, uint32_t n) {
  emit(label, 'P', codec, in_rows, in_cols, out_rows, out_cols, in_rows * 4u, in_cols * 4u, n);
}
// a Downsample of n images of h x w pixels: the grids as the entry point derives them
static void emit_down(const char *label, int codec, uint32_t h, uint32_t w, uint32_t n) {
  emit(label, 'D', codec, (h + 3) / 4, (w + 3) / 4, ((h + 1) / 2 + 3) / 4, ((w + 1) / 2 + 3) / 4, h, w, n);
}

int main() {
  static const char *const kCodecNames[] = { "dxt1", "dxt5", "etc1" };
  static const uint32_t kPadIn[][2] = { {1, 1}, {2, 3}, {16, 32}, {64, 1024}, {1024, 1024} };
  static const uint32_t kPadExtra[][2] = { {0, 0}, {0, 1}, {1, 0}, {2, 3}, {0, 64} };
  static const uint32_t kPadImages[] = { 1, 3, 257, 70000 };
  char label[64];
  for (int codec = 0; codec < 3; ++codec) {
    for (const auto &g : kPadIn) {
      snprintf(label, sizeof label, "pad/%s/%ux%u", kCodecNames[codec], g[0], g[1]);
      for (const auto &e : kPadExtra)
        for (uint32_t n : kPadImages) emit_pad(label, codec, g[0], g[1], g[0] + e[0], g[1] + e[1], n);
    }
    // both sides of border x 4 x images = 2^31 (64 pad blocks per image)
    snprintf(label, sizeof label, "pad/%s/quad-lanes-2^31", kCodecNames[codec]);
    emit_pad(label, codec, 1, 1, 1, 65, (1u << 23) - 1);
    emit_pad(label, codec, 1, 1, 1, 65, 1u << 23);
    // images x blocks per image across 2^31 - 1: one group, then two
    snprintf(label, sizeof label, "pad/%s/groups", kCodecNames[codec]);
    emit_pad(label, codec, 1024, 1024, 1024, 1024, 2047);
    emit_pad(label, codec, 1024, 1024, 1024, 1024, 2048);
    emit_pad(label, codec, 2, 3, 4, 6, 89478485);
    emit_pad(label, codec, 2, 3, 4, 6, 89478486);
    emit_pad(label, codec, 1, 1, 1, 1, 0xffffffffu);
    // one image of 2^31 - 32 768 blocks, and one of 2^31: refused
    snprintf(label, sizeof label, "pad/%s/image-2^31", kCodecNames[codec]);
    emit_pad(label, codec, 1, 1, 32768, 65535, 1);
    emit_pad(label, codec, 1, 1, 32768, 65536, 1);
    emit_pad(label, codec, 1, 1, 32768, 65536, 3);
    emit_pad(label, codec, 1, 1, 1, 1, 0);
  }

  static const uint32_t kDownImages[] = { 1, 2, 65535, 65536 };
  struct Size { const char *name; uint32_t h, w; };
  static const Size kDownSizes[] = {
    { "block", 1, 1 }, { "block", 1, 2 }, { "block", 1, 4 }, { "block", 2, 1 }, { "block", 2, 2 }, { "block", 2, 4 }, { "block", 4, 1 },
    { "block", 4, 2 }, { "block", 4, 4 },
    { "1x2-2x1-2x2", 4, 8 }, { "1x2-2x1-2x2", 8, 4 }, { "1x2-2x1-2x2", 8, 8 },
    // out-columns on both sides of a row tile, two block rows and one
    { "cols-255", 16, 2040 }, { "cols-256", 16, 2048 }, { "cols-257", 16, 2056 }, { "cols-255", 4, 2040 }, { "cols-256", 4, 2048 },
    { "cols-257", 4, 2056 }, { "cols-256", 8, 2048 }, { "cols-257", 8, 2056 },
    // 36 864 output blocks, the most of the quad form, and the next sizes up
    { "quad-max", 1536, 1536 }, { "quad-max", 1536, 1544 }, { "quad-max", 1544, 1536 },
    // 65 535 and 65 536 output rows of 256 columns
    { "rows-65535", 524280, 2048 }, { "rows-65536", 524288, 2048 },
  };
  for (int codec = 0; codec < 3; ++codec)
    for (const Size &s : kDownSizes) {
      snprintf(label, sizeof label, "down/%s/%s", kCodecNames[codec], s.name);
      for (uint32_t n : kDownImages) emit_down(label, codec, s.h, s.w, n);
    }
  for (int codec = 0; codec < 3; ++codec) {  // one image of 2^31 output blocks: refused
    snprintf(label, sizeof label, "down/%s/image-2^31", kCodecNames[codec]);
    emit(label, 'D', codec, 65536, 131072, 32768, 65536, 262144, 524288, 1);
    emit(label, 'D', codec, 65536, 131070, 32768, 65535, 262144, 524280, 2);
  }

  // CopySubimage: rows and images in chunks of kGridLimitYZ
  static const uint32_t kCounts[] = { 1, 65534, 65535, 65536, 131071 };
  static const uint32_t kCols[] = { 1, 256, 257 };
  for (uint32_t rows : kCounts)
    for (uint32_t images : kCounts)
      for (uint32_t cols : kCols) {
        printf("= copy_subimage rows %u images %u cols %u grid_x %u :", rows, images, cols, copy_subimage_grid_x(cols));
        for_chunks(images, kGridLimitYZ, [&](uint64_t img0, uint64_t nz) {
          for_chunks(rows, kGridLimitYZ, [&](uint64_t row0, uint64_t ny) {
            printf(" z%llu+%llu/y%llu+%llu", (unsigned long long)img0, (unsigned long long)nz, (unsigned long long)row0, (unsigned long long)ny);
          });
        });
        printf("\n");
      }
  // the fills on both sides of each workgroup cap
  static const uint64_t kFillBlocks[] = { 1, 256, 257, 4194303, 4194304, 4194305, 4196352, 1ull << 33 };
  for (uint64_t n : kFillBlocks) printf("= fill blocks %llu workgroups %u\n", (unsigned long long)n, fill_workgroups(n));
  static const uint32_t kBatchImages[] = { 1, 64, 65, 70 };
  static const uint32_t kBatchBlocks[] = { 1, 256, 257, 32768, 32769, 37056, 349440, 349696, 349697, 2097152, 2097153 };
  for (uint32_t images : kBatchImages)
    for (uint32_t bpi : kBatchBlocks) {
      printf("= fill_batch images %u blocks_per_image %u :", images, bpi);
      for_chunks(images, kFillBatch, [&](uint64_t first, uint64_t n) {
        printf(" %llu+%llu/%u", (unsigned long long)first, (unsigned long long)n, fill_batch_workgroups(bpi, (uint32_t)n));
      });
      printf("\n");
    }
  static const uint64_t kTranscodeBlocks[] = { 1, 1ull << 30, (1ull << 30) + 1, (1ull << 31) + 5 };
  for (uint64_t n : kTranscodeBlocks) {
    printf("= transcode blocks %llu :", (unsigned long long)n);
    for_chunks(n, kTranscodeChunk, [&](uint64_t first, uint64_t count) {
      printf(" %llu+%llu/%llu", (unsigned long long)first, (unsigned long long)count, (unsigned long long)((count + kBlockOpLanes - 1) / kBlockOpLanes));
    });
    printf("\n");
  }
  return 0;
}
