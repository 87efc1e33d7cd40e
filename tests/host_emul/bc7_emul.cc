// TEST INFRASTRUCTURE ONLY.  The BC7 block math of image-compression_amd/csrc/bc7_block.h compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION, like eac11_16_emul.cc) so that the CPU tier checks it against the numpy definition and the
// fixture (tests/test_bc7_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "metric_block.h"  // bc7_block.h + metric_bc7_block
#include "emul_violations.h"

using namespace icamd;

template <int COMPS>
static void encode_image(int swap, uint32_t h, uint32_t w, uint32_t rows, uint32_t cols, uint32_t stride, const uint8_t *src,
                         uint8_t *out) {
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t px[16], o[4];
      load_block<COMPS>(src, h, w, stride, br * 4, bc * 4, px);
      encode_bc7<COMPS>(px, swap != 0, o);
      memcpy(out + ((size_t)br * cols + bc) * 16, o, 16);
    }
}

// The encoder as the kernels run it (bc7_kernels.hip), one block at a time, over the grid max(h, gh) x max(w, gw).
extern "C" int bc7_emul_encode(int comps, int swap, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride,
                               const uint8_t *src, uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  if (comps == 3) encode_image<3>(swap, h, w, rows, cols, stride, src, out);
  else if (comps == 4) encode_image<4>(swap, h, w, rows, cols, stride, src, out);
  else return 0;
  return 1;
}

// The decoder's block math (decode_bc7): h rows of w RGBA8 pixels + pad bytes; the pad bytes are left alone.
extern "C" int bc7_emul_decode(int swap, uint32_t h, uint32_t w, uint32_t pad, const uint8_t *blocks, uint8_t *out) {
  const uint32_t cols = (w + 3) / 4;
  const size_t stride = (size_t)w * 4u + pad;
  for (uint32_t br = 0; br < (h + 3) / 4; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t wd[4], px[16];
      memcpy(wd, blocks + ((size_t)br * cols + bc) * 16, 16);
      decode_bc7(wd, swap != 0, px);
      for (uint32_t y = 0; y < 4 && br * 4 + y < h; ++y)
        for (uint32_t x = 0; x < 4 && bc * 4 + x < w; ++x) memcpy(out + (br * 4 + y) * stride + (size_t)(bc * 4 + x) * 4u, &px[4 * y + x], 4);
    }
  return 1;
}

template <int COMPS>
static void metric_image(int swap, uint32_t h, uint32_t w, uint32_t grid_cols, uint32_t stride, const uint8_t *src,
                         const uint8_t *blocks, uint64_t *out) {
  for (uint32_t br = 0; br < (h + 3) / 4; ++br)
    for (uint32_t bc = 0; bc < (w + 3) / 4; ++bc) {
      uint32_t wd[4];
      MetricAcc acc;
      metric_clear(acc);
      memcpy(wd, blocks + ((size_t)br * grid_cols + bc) * 16, 16);
      metric_bc7_block<COMPS>(wd, swap != 0, src, h, w, stride, br * 4, bc * 4, true, acc);
      for (int k = 0; k < 4; ++k) {
        out[k] += acc.sse[k];
        out[4 + k] = std::max<uint64_t>(out[4 + k], metric_max(acc, k));
      }
    }
}

// The metric's block math over one image: out[0..3] = sse of bytes 0..3, out[4..7] = the largest absolute differences.
// grid_w: the width of the grid the blocks lie in.
extern "C" int bc7_emul_metric(int comps, int swap, uint32_t h, uint32_t w, uint32_t grid_w, uint32_t stride, const uint8_t *src,
                               const uint8_t *blocks, uint64_t *out) {
  const uint32_t gc = (std::max(w, grid_w) + 3) / 4;
  for (int k = 0; k < 8; ++k) out[k] = 0;
  if (comps == 3) metric_image<3>(swap, h, w, gc, stride, src, blocks, out);
  else if (comps == 4) metric_image<4>(swap, h, w, gc, stride, src, blocks, out);
  else return 0;
  return 1;
}
