// TEST INFRASTRUCTURE ONLY.  The BC6H block math of image-compression_amd/csrc/bc6h_block.h compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION, like bc7_emul.cc) so that the CPU tier checks it against the numpy definition and the
// fixtures (tests/test_bc6h_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "bc6h_block.h"
#include "emul_violations.h"

using namespace icamd;

template <int C, bool SIGNED>
static void encode_image(uint32_t h, uint32_t w, uint32_t rows, uint32_t cols, uint32_t stride, const uint8_t *src, uint8_t *out) {
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t rg[16], b[16], o[4];
      bc6h_fetch<C>(src, h, w, stride, br * 4, bc * 4, rg, b);
      encode_bc6h<SIGNED>(rg, b, o);
      memcpy(out + ((size_t)br * cols + bc) * 16, o, 16);
    }
}

// The encoder as the kernels run it (bc6h_kernels.hip), one block at a time, over the grid max(h, gh) x max(w, gw).
extern "C" int bc6h_emul_encode(int is_signed, int chans, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride,
                                const uint8_t *src, uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  if (chans == 3 && !is_signed) encode_image<3, false>(h, w, rows, cols, stride, src, out);
  else if (chans == 3) encode_image<3, true>(h, w, rows, cols, stride, src, out);
  else if (chans == 4 && !is_signed) encode_image<4, false>(h, w, rows, cols, stride, src, out);
  else if (chans == 4) encode_image<4, true>(h, w, rows, cols, stride, src, out);
  else return 0;
  return 1;
}

// The decoder's block math: h rows of w RGBA16F pixels (A = 0x3C00) + pad bytes; the pad bytes are left alone.
extern "C" int bc6h_emul_decode(int is_signed, uint32_t h, uint32_t w, uint32_t pad, const uint8_t *blocks, uint8_t *out) {
  const uint32_t cols = (w + 3) / 4;
  const size_t stride = (size_t)w * 8u + pad;
  for (uint32_t br = 0; br < (h + 3) / 4; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t wd[4], rg[16], b[16];
      memcpy(wd, blocks + ((size_t)br * cols + bc) * 16, 16);
      if (is_signed) decode_bc6h<true>(wd, rg, b);
      else decode_bc6h<false>(wd, rg, b);
      for (uint32_t y = 0; y < 4 && br * 4 + y < h; ++y)
        for (uint32_t x = 0; x < 4 && bc * 4 + x < w; ++x) {
          const uint32_t px[2] = { rg[4 * y + x], (b[4 * y + x] & 0xffffu) | 0x3c000000u };
          memcpy(out + (br * 4 + y) * stride + (size_t)(bc * 4 + x) * 8u, px, 8);
        }
    }
  return 1;
}

template <int C, bool SIGNED>
static void metric_image(uint32_t h, uint32_t w, uint32_t grid_cols, uint32_t stride, const uint8_t *src, const uint8_t *blocks,
                         uint64_t *out) {
  for (uint32_t br = 0; br < (h + 3) / 4; ++br)
    for (uint32_t bc = 0; bc < (w + 3) / 4; ++bc) {
      uint32_t wd[4];
      Bc6hAcc acc;
      bc6h_clear(acc);
      memcpy(wd, blocks + ((size_t)br * grid_cols + bc) * 16, 16);
      metric_bc6h_block<C, SIGNED>(wd, src, h, w, stride, br * 4, bc * 4, acc);
      for (int k = 0; k < 3; ++k) {
        out[k] += acc.sse[k];
        out[3 + k] = std::max<uint64_t>(out[3 + k], acc.mx[k]);
      }
    }
}

// The metric's block math over one image: out[0..2] = sse of R, G, B in the t domain, out[3..5] = the largest absolute
// differences.  grid_w: the width of the grid the blocks lie in.
extern "C" int bc6h_emul_metric(int is_signed, int chans, uint32_t h, uint32_t w, uint32_t grid_w, uint32_t stride,
                                const uint8_t *src, const uint8_t *blocks, uint64_t *out) {
  const uint32_t gc = (std::max(w, grid_w) + 3) / 4;
  for (int k = 0; k < 6; ++k) out[k] = 0;
  if (chans == 3 && !is_signed) metric_image<3, false>(h, w, gc, stride, src, blocks, out);
  else if (chans == 3) metric_image<3, true>(h, w, gc, stride, src, blocks, out);
  else if (chans == 4 && !is_signed) metric_image<4, false>(h, w, gc, stride, src, blocks, out);
  else if (chans == 4) metric_image<4, true>(h, w, gc, stride, src, blocks, out);
  else return 0;
  return 1;
}

// Step 2 as the kernels run it (the closed-form guess +- 1), and D(q).
extern "C" int32_t bc6h_emul_quantise(int is_signed, int32_t T) { return is_signed ? bc6h_quantise<true>(T) : bc6h_quantise<false>(T); }
extern "C" int32_t bc6h_emul_endpoint_value(int is_signed, int32_t q) {
  return is_signed ? bc6h_endpoint_value<true>(q) : bc6h_endpoint_value<false>(q);
}
