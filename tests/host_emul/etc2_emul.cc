// TEST INFRASTRUCTURE ONLY.  The ETC2 RGBA8 block math of image-compression_amd/csrc/etc2_block.h (and the ETC1 colour half of
// etc1_block.h it is fused with) compiled for the HOST (g++ -DICAMD_HOST_EMULATION, like emul.cc) so that the CPU tier checks
// it against the numpy definition (tests/test_etc2_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "etc1_block.h"
#include "etc2_block.h"
#include "emul_violations.h"

using namespace icamd;

// The encoder as the kernels run it (etc2_kernels.hip): one RGBA8 block, the colour half through the ETC1 routines the kernel
// of `strategy` uses (a "wave" is one block here), the alpha bytes through the EAC search.
extern "C" int etc2_emul_encode(int strategy, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride,
                                const uint8_t *src, uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  const uint32_t st = (uint32_t)strategy < 4u ? (uint32_t)strategy : 2u;
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t px[16], a[16];
      load_block<4>(src, h, w, stride, br * 4, bc * 4, px);
      Out8 c;
      if (st == 3u) {
        c = encode_etc1_block<false>(px, 3u);
      } else {
        const uint32_t spread = etc1_block_spread(px);
        const bool constant = etc1_constant_block(px, spread), busy = spread >= ICAMD_ETC1_BUSY_SPREAD;
        c = st == 0u ? etc1_encode_classified<0>(px, constant, busy)
            : st == 1u ? etc1_encode_classified<1>(px, constant, busy) : etc1_encode_classified<2>(px, constant, busy);
      }
      for (int p = 0; p < 16; ++p) a[p] = px[p] >> 24;
      const Out8 e = encode_eac_alpha(a);
      uint8_t *o = out + ((size_t)br * cols + bc) * 16;
      memcpy(o, &e, 8);
      memcpy(o + 8, &c, 8);
    }
  return 1;
}

// The decoder's block math (decode_etc2_rgba8): h rows of 4 w + pad bytes; the pad bytes are left alone.
extern "C" int etc2_emul_decode(int swap, uint32_t h, uint32_t w, uint32_t pad, const uint8_t *blocks, uint8_t *out) {
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

// One EAC word from sixteen alphas in raster order (a[4 y + x]), and back.
extern "C" void etc2_emul_alpha_block(const uint8_t v[16], uint8_t word[8], uint8_t decoded[16]) {
  uint32_t a[16], px[16] = { 0 };
  for (int p = 0; p < 16; ++p) a[p] = v[p];
  const Out8 e = encode_eac_alpha(a);
  memcpy(word, &e, 8);
  decode_eac_alpha(e.lo, e.hi, px);
  for (int p = 0; p < 16; ++p) decoded[p] = (uint8_t)(px[p] >> 24);
}

// M[t][k] as the block math derives it from its packed constants (the table self-checks).
extern "C" int etc2_emul_modifier(int t, int k) {
  const uint32_t g = bfe(eac_mags((uint32_t)t), 8u * ((uint32_t)k & 3u), 8u);
  return k < 4 ? -(int)g : (int)g - 1;
}
