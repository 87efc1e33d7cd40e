// transcode_family_plan_driver.cc -- prints how image-compression_amd/csrc/blockops_plan.h cuts the in-place ETC2-family
// transcodes into launches, for tests/test_transcode_family_host.py.  Built with g++ alone: the header needs nothing from HIP.
//
// Per (n_bytes, block_bytes, lanes): "= n_bytes block_bytes lanes blocks launches", then one line per launch -- all of them
// where there are at most four, else the first two and the last two --: "i first_block byte_offset blocks grid_x lanes".
#include <cstdio>

#include "blockops_plan.h"

using namespace icamd;

int main() {
  static const struct { uint32_t block, lanes; } kKinds[] = { { 8, kBlockOpLanes }, { 8, kSearchLanes }, { 16, kSearchLanes } };
  for (const auto &k : kKinds) {
    const uint64_t chunk_bytes = kTranscodeFamilyChunk * k.block;
    const uint64_t sizes[] = { 0, k.block - 1, k.block, k.block + 1, chunk_bytes - 1, chunk_bytes, chunk_bytes + k.block - 1,
                               chunk_bytes + k.block, 1ull << 40, (1ull << 40) + 7 };
    for (uint64_t n_bytes : sizes) {
      const uint64_t blocks = transcode_blocks(n_bytes, k.block), launches = transcode_launches(blocks);
      printf("= %llu %u %u %llu %llu\n", (unsigned long long)n_bytes, k.block, k.lanes, (unsigned long long)blocks,
             (unsigned long long)launches);
      for (uint64_t i = 0; i < launches; ++i) {
        if (launches > 4 && i >= 2 && i + 2 < launches) continue;
        const TranscodeLaunch l = transcode_launch(blocks, k.block, k.lanes, i);
        printf("%llu %llu %llu %u %u %u\n", (unsigned long long)i, (unsigned long long)l.first_block,
               (unsigned long long)l.byte_offset, l.blocks, l.grid_x, l.lanes);
      }
    }
  }
  return 0;
}
