// TEST INFRASTRUCTURE ONLY.  The EAC R11 / RG11 block math of image-compression_amd/csrc/eac11_block.h compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION, like etc2_emul.cc) so that the CPU tier checks it against the numpy definition
// (tests/test_eac11_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "eac11_block.h"
#include "metric_block.h"  // metric_gather_channel, the kernels' clamp-to-edge gather
#include "emul_violations.h"

using namespace icamd;

template <int COMPS>
static void encode_image(bool two, uint32_t rch, uint32_t h, uint32_t w, uint32_t rows, uint32_t cols, uint32_t stride,
                         const uint8_t *src, uint8_t *out) {
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t r[4];
      uint8_t *o = out + ((size_t)br * cols + bc) * (two ? 16 : 8);
      metric_gather_channel<COMPS>(src, h, w, stride, br * 4, bc * 4, rch, r);
      const Out8 a = encode_eac11_rows(r);
      memcpy(o, &a, 8);
      if (two) {
        metric_gather_channel<COMPS>(src, h, w, stride, br * 4, bc * 4, 1u, r);
        const Out8 b = encode_eac11_rows(r);
        memcpy(o + 8, &b, 8);
      }
    }
}

// The encoder as the kernels run it (eac11_kernels.hip), one block at a time: the channel's sixteen bytes, fetched with
// clamp-to-edge replication over the grid max(h, gh) x max(w, gw), through encode_eac_alpha.  two: RG11.
extern "C" int eac11_emul_encode(int two, int comps, int swap, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride,
                                 const uint8_t *src, uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  const uint32_t rch = (swap && comps >= 3) ? 2u : 0u;
  switch (comps) {
    case 1: if (two) return 0; encode_image<1>(false, rch, h, w, rows, cols, stride, src, out); return 1;
    case 2: encode_image<2>(two != 0, rch, h, w, rows, cols, stride, src, out); return 1;
    case 3: encode_image<3>(two != 0, rch, h, w, rows, cols, stride, src, out); return 1;
    case 4: encode_image<4>(two != 0, rch, h, w, rows, cols, stride, src, out); return 1;
  }
  return 0;
}

// The decoder's block math (decode_eac11): h rows of w (R11) / 2 w (RG11) + pad bytes; the pad bytes are left alone.
extern "C" int eac11_emul_decode(int two, uint32_t h, uint32_t w, uint32_t pad, const uint8_t *blocks, uint8_t *out) {
  const uint32_t cols = (w + 3) / 4, c = two ? 2u : 1u;
  const size_t stride = (size_t)w * c + pad;
  for (uint32_t br = 0; br < (h + 3) / 4; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc)
      for (uint32_t k = 0; k < c; ++k) {
        uint32_t wd[2], r[4];
        memcpy(wd, blocks + ((size_t)br * cols + bc) * (8 * c) + 8 * k, 8);
        decode_eac11(wd[0], wd[1], r);
        for (uint32_t y = 0; y < 4 && br * 4 + y < h; ++y)
          for (uint32_t x = 0; x < 4 && bc * 4 + x < w; ++x)
            out[(br * 4 + y) * stride + (size_t)(bc * 4 + x) * c + k] = (uint8_t)(r[y] >> (8 * x));
      }
  return 1;
}
