// TEST INFRASTRUCTURE ONLY.  The 16-bit and signed EAC R11 / RG11 block math of image-compression_amd/csrc/eac11_16_block.h
// compiled for the HOST (g++ -DICAMD_HOST_EMULATION, like eac11_emul.cc) so that the CPU tier checks it against the numpy
// definition (tests/test_eac11_16_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "eac11_16_block.h"
#include "emul_violations.h"

using namespace icamd;

template <int C, bool RG, bool SIGNED>
static void encode_image(uint32_t h, uint32_t w, uint32_t rows, uint32_t cols, uint32_t stride, const uint8_t *src, uint8_t *out) {
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t r[8], g[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
      uint8_t *o = out + ((size_t)br * cols + bc) * (RG ? 16 : 8);
      eac11_16_fetch<C, RG>(src, h, w, stride, br * 4, bc * 4, r, g);
      const Out8 a = encode_eac11_16<SIGNED>(r);
      memcpy(o, &a, 8);
      if (RG) {
        const Out8 b = encode_eac11_16<SIGNED>(g);
        memcpy(o + 8, &b, 8);
      }
    }
}

template <bool RG, bool SIGNED>
static int encode_chans(int chans, uint32_t h, uint32_t w, uint32_t rows, uint32_t cols, uint32_t stride, const uint8_t *src,
                        uint8_t *out) {
  switch (chans) {
    case 1: if (RG) return 0; encode_image<1, false, SIGNED>(h, w, rows, cols, stride, src, out); return 1;
    case 2: encode_image<2, RG, SIGNED>(h, w, rows, cols, stride, src, out); return 1;
    case 3: encode_image<3, RG, SIGNED>(h, w, rows, cols, stride, src, out); return 1;
    case 4: encode_image<4, RG, SIGNED>(h, w, rows, cols, stride, src, out); return 1;
  }
  return 0;
}

// The encoder as the kernels run it (eac11_16_kernels.hip), one block at a time, over the grid max(h, gh) x max(w, gw).
// two: RG11; sgn: the signed codecs; stride in bytes.
extern "C" int eac11_16_emul_encode(int two, int sgn, int chans, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride,
                                    const uint8_t *src, uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  if (two) return sgn ? encode_chans<true, true>(chans, h, w, rows, cols, stride, src, out)
                      : encode_chans<true, false>(chans, h, w, rows, cols, stride, src, out);
  return sgn ? encode_chans<false, true>(chans, h, w, rows, cols, stride, src, out)
             : encode_chans<false, false>(chans, h, w, rows, cols, stride, src, out);
}

// The decoder's block math (decode_eac11_16): h rows of w (R11) / 2 w (RG11) 16-bit samples + pad bytes; the pad bytes are
// left alone.
extern "C" int eac11_16_emul_decode(int two, int sgn, uint32_t h, uint32_t w, uint32_t pad, const uint8_t *blocks, uint8_t *out) {
  const uint32_t cols = (w + 3) / 4, c = two ? 2u : 1u;
  const size_t stride = (size_t)w * c * 2u + pad;
  for (uint32_t br = 0; br < (h + 3) / 4; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc)
      for (uint32_t k = 0; k < c; ++k) {
        uint32_t wd[2], r[4][2];
        memcpy(wd, blocks + ((size_t)br * cols + bc) * (8 * c) + 8 * k, 8);
        if (sgn) decode_eac11_16<true>(wd[0], wd[1], r);
        else decode_eac11_16<false>(wd[0], wd[1], r);
        for (uint32_t y = 0; y < 4 && br * 4 + y < h; ++y)
          for (uint32_t x = 0; x < 4 && bc * 4 + x < w; ++x) {
            const uint16_t v = (uint16_t)(r[y][x >> 1] >> (16 * (x & 1)));
            memcpy(out + (br * 4 + y) * stride + ((size_t)(bc * 4 + x) * c + k) * 2u, &v, 2);
          }
      }
  return 1;
}

template <int C, bool RG, bool SIGNED>
static void metric_image(uint32_t h, uint32_t w, uint32_t grid_cols, uint32_t stride, const uint8_t *src, const uint8_t *blocks,
                         Eac16Acc &acc) {
  for (uint32_t br = 0; br < (h + 3) / 4; ++br)
    for (uint32_t bc = 0; bc < (w + 3) / 4; ++bc) {
      uint32_t wd[4] = { 0, 0, 0, 0 };
      memcpy(wd, blocks + ((size_t)br * grid_cols + bc) * (RG ? 16 : 8), RG ? 16 : 8);
      metric_eac11_16_block<C, RG, SIGNED>(wd, src, h, w, stride, br * 4, bc * 4, acc);
    }
}

// The metric's block math over one image (2-channel sources only: the layouts differ in the fetch, which the encoder covers):
// out[0..1] = sse of R, G; out[2..3] = the largest absolute differences.  grid_w: the width of the grid the blocks lie in.
extern "C" int eac11_16_emul_metric(int two, int sgn, uint32_t h, uint32_t w, uint32_t grid_w, uint32_t stride, const uint8_t *src,
                                    const uint8_t *blocks, uint64_t *out) {
  Eac16Acc acc;
  eac16_clear(acc);
  const uint32_t gc = (std::max(w, grid_w) + 3) / 4;
  if (two && sgn) metric_image<2, true, true>(h, w, gc, stride, src, blocks, acc);
  else if (two) metric_image<2, true, false>(h, w, gc, stride, src, blocks, acc);
  else if (sgn) metric_image<2, false, true>(h, w, gc, stride, src, blocks, acc);
  else metric_image<2, false, false>(h, w, gc, stride, src, blocks, acc);
  out[0] = acc.sse[0]; out[1] = acc.sse[1]; out[2] = acc.mx[0]; out[3] = acc.mx[1];
  return 1;
}
