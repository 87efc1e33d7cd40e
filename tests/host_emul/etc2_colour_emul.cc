// TEST INFRASTRUCTURE ONLY.  The ETC2 colour-word block math of image-compression_amd/csrc/etc2_colour_block.h (five-mode decode,
// planar fit / pack / choice) and the ETC1 routines it is fused with, compiled for the HOST (g++ -DICAMD_HOST_EMULATION, like
// etc2_emul.cc) so that the CPU tier checks it against the numpy definition (tests/test_etc2_colour_host.py).  Never linked
// into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "etc1_block.h"
#include "etc2_block.h"
#include "etc2_colour_block.h"
#include "emul_violations.h"

using namespace icamd;

template <int COMPS>
static void encode_image(uint32_t st, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride, const uint8_t *src,
                         uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t px[16];
      load_block<COMPS>(src, h, w, stride, br * 4, bc * 4, px);
      Out8 c;
      if (st == 3u) {
        c = encode_etc1_block<false>(px, 3u);
      } else {
        const uint32_t spread = etc1_block_spread(px);
        const bool constant = etc1_constant_block(px, spread), busy = spread >= ICAMD_ETC1_BUSY_SPREAD;
        c = st == 0u ? etc1_encode_classified<0>(px, constant, busy)
            : st == 1u ? etc1_encode_classified<1>(px, constant, busy) : etc1_encode_classified<2>(px, constant, busy);
      }
      const Out8 o = etc2_rgb8_choose(px, c);
      memcpy(out + ((size_t)br * cols + bc) * 8, &o, 8);
    }
}

// The ICAMD_ETC2_RGB8 encoder as the kernels run it (etc2_rgb8_kernels.hip): the ETC1 word through the routines the kernel of
// `strategy` uses (a "wave" is one block here), then the planar candidate and the choice.
extern "C" int etc2c_emul_encode(int strategy, int comps, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride,
                                 const uint8_t *src, uint8_t *out) {
  const uint32_t st = (uint32_t)strategy < 4u ? (uint32_t)strategy : 2u;
  if (comps == 3) encode_image<3>(st, h, w, gh, gw, stride, src, out);
  else if (comps == 4) encode_image<4>(st, h, w, gh, gw, stride, src, out);
  else return 0;
  return 1;
}

// n colour words -> n x 16 texels in raster order (4 y + x), three bytes each
extern "C" void etc2c_emul_decode_words(uint32_t n, const uint8_t *words, uint8_t *rgb) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t w[2], px[16];
    memcpy(w, words + (size_t)i * 8, 8);
    decode_etc2_colour(w[0], w[1], px);
    for (int p = 0; p < 16; ++p) memcpy(rgb + ((size_t)i * 16 + p) * 3, &px[p], 3);
  }
}

// the mode of n colour words: 0 ETC1-compatible, 1 T, 2 H, 3 planar
extern "C" void etc2c_emul_modes(uint32_t n, const uint8_t *words, uint8_t *mode) {
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t *b = words + (size_t)i * 8;
    mode[i] = (uint8_t)etc2_colour_mode((uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | b[3]);
  }
}

// n x 9 codes -> n planar words, and the nine fields read back from each word
extern "C" void etc2c_emul_planar_pack(uint32_t n, const uint32_t *codes, uint8_t *words, uint32_t *fields) {
  for (uint32_t i = 0; i < n; ++i) {
    const Out8 o = etc2_planar_pack(codes + (size_t)i * 9);
    memcpy(words + (size_t)i * 8, &o, 8);
    etc2_planar_codes(perm(0u, o.lo, 0x00010203u), perm(0u, o.hi, 0x00010203u), fields + (size_t)i * 9);
  }
}

// n blocks of 16 texels in raster order (three bytes each) -> n x 9 codes of the least-squares plane
extern "C" void etc2c_emul_planar_fit(uint32_t n, const uint8_t *rgb, uint32_t *codes) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t px[16];
    for (int p = 0; p < 16; ++p) {
      const uint8_t *q = rgb + ((size_t)i * 16 + p) * 3;
      px[p] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
    }
    etc2_planar_fit(px, codes + (size_t)i * 9);
  }
}

// ETC2 RGBA8 blocks with any colour word (decode_etc2_rgba8): h rows of 4 w + pad bytes; the pad bytes are left alone.
extern "C" int etc2c_emul_decode_rgba8(int swap, uint32_t h, uint32_t w, uint32_t pad, const uint8_t *blocks, uint8_t *out) {
  const uint32_t cols = (w + 3) / 4;
  const size_t stride = (size_t)w * 4 + pad;
  for (uint32_t br = 0; br < (h + 3) / 4; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t wd[4], px[16];
      memcpy(wd, blocks + ((size_t)br * cols + bc) * 16, 16);
      decode_etc2_rgba8(wd, swap != 0, px);
      for (uint32_t y = 0; y < 4 && br * 4 + y < h; ++y)
        for (uint32_t x = 0; x < 4 && bc * 4 + x < w; ++x) memcpy(out + (br * 4 + y) * stride + (size_t)(bc * 4 + x) * 4, &px[4 * y + x], 4);
    }
  return 1;
}
