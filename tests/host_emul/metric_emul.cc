// TEST INFRASTRUCTURE ONLY.  The per-block error accumulation of image-compression_amd/csrc/metric_block.h compiled for the
// HOST (g++ -DICAMD_HOST_EMULATION, like emul.cc) so that the CPU tier checks it against the definition computed with the
// oracle's decoders (tests/test_metric_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "metric_block.h"
#include "emul_violations.h"

using namespace icamd;

namespace {
template <int CODEC, int COMPS>
void one_block(const uint32_t *w, bool swap, const uint8_t *src, uint32_t h, uint32_t wd, uint32_t stride, uint32_t row,
               uint32_t col, bool wide_ok, MetricAcc &a) {
  if (CODEC == 5 || CODEC == 6) metric_bc45_block<COMPS, CODEC == 6>(w, swap, src, h, wd, stride, row, col, wide_ok, a);
  else metric_color_block<(CODEC > 2 ? 0 : CODEC), (COMPS >= 3 ? COMPS : 4)>(w, swap, src, h, wd, stride, row, col, wide_ok, a);
}
typedef void (*OneBlock)(const uint32_t *, bool, const uint8_t *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, bool,
                         MetricAcc &);
OneBlock pick(int codec, int comps) {
  switch (codec * 8 + comps) {
    case 0 * 8 + 3: return one_block<0, 3>;
    case 0 * 8 + 4: return one_block<0, 4>;
    case 1 * 8 + 4: return one_block<1, 4>;
    case 2 * 8 + 3: return one_block<2, 3>;
    case 2 * 8 + 4: return one_block<2, 4>;
    case 5 * 8 + 1: return one_block<5, 1>;
    case 5 * 8 + 2: return one_block<5, 2>;
    case 5 * 8 + 3: return one_block<5, 3>;
    case 5 * 8 + 4: return one_block<5, 4>;
    case 6 * 8 + 2: return one_block<6, 2>;
    case 6 * 8 + 3: return one_block<6, 3>;
    case 6 * 8 + 4: return one_block<6, 4>;
  }
  return nullptr;
}
}  // namespace

// One image as the kernels walk it: the blocks that cover the h x w image out of a grid of max(h, gh) x max(w, gw) pixels,
// each lane-accumulator flushed into 64-bit sums after `blocks_per_flush` blocks (the kernels: 4 per lane).  gather = 1 forces
// the 64-bit gather of every block.  Returns 0 for a codec / component pair the C ABI refuses.
extern "C" int metric_emul_measure(int codec, int comps, int swap, int gather, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw,
                                   uint32_t stride, const uint8_t *src, const uint8_t *blocks, uint64_t sse[4],
                                   uint32_t max_abs[4]) {
  const OneBlock f = pick(codec, comps);
  if (!f || (swap && comps < 3)) return 0;
  const uint32_t grid_cols = (std::max(w, gw) + 3) / 4, bytes = (codec == 1 || codec == 6) ? 16 : 8;
  for (int k = 0; k < 4; ++k) { sse[k] = 0; max_abs[k] = 0; }
  MetricAcc a;
  metric_clear(a);
  uint32_t held = 0;
  auto flush = [&]() {
    for (int k = 0; k < 4; ++k) {
      sse[k] += a.sse[k];
      max_abs[k] = std::max(max_abs[k], metric_max(a, k));
    }
    metric_clear(a);
    held = 0;
  };
  for (uint32_t br = 0; br < (h + 3) / 4; ++br)
    for (uint32_t bc = 0; bc < (w + 3) / 4; ++bc) {
      uint32_t wd[4] = { 0, 0, 0, 0 };
      memcpy(wd, blocks + ((size_t)br * grid_cols + bc) * bytes, bytes);
      f(wd, swap != 0, src, h, w, stride, br * 4, bc * 4, gather == 0, a);
      if (++held == 4) flush();
    }
  flush();
  return 1;
}
