// TEST INFRASTRUCTURE ONLY.  The ETC2 RGB8A1 block math of image-compression_amd/csrc/etc2_a1_block.h (decoder, masked
// differential search, per-block choice) and the ETC1 routines it is fused with, compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION, like etc2_colour_emul.cc) so that the CPU tier checks it against the numpy definition
// (tests/test_etc2_a1_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "etc1_block.h"
#include "etc2_a1_block.h"
#include "emul_violations.h"

using namespace icamd;

template <int ST>
static void encode_image(uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride, const uint8_t *src, uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t px[16];
      load_block<4>(src, h, w, stride, br * 4, bc * 4, px);
      Out8 c = { 0u, 0u };
      if (etc2_a1_opaque_mask(px) == 0xffffu) {  // (a "wave" is one block here: the ETC1 phase runs where the block is opaque)
        if (ST == 3) {
          c = encode_etc1_block<false>(px, 3u);
        } else {
          const uint32_t spread = etc1_block_spread(px);
          c = etc1_encode_classified<ST>(px, etc1_constant_block(px, spread), spread >= ICAMD_ETC1_BUSY_SPREAD);
        }
      }
      const Out8 o = etc2_a1_block<ST>(px, c);
      memcpy(out + ((size_t)br * cols + bc) * 8, &o, 8);
    }
}

// The ICAMD_ETC2_RGB8A1 encoder as the kernels run it (etc2_a1_kernels.hip) on an RGBA8 image.
extern "C" int etc2a1_emul_encode(int strategy, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride,
                                  const uint8_t *src, uint8_t *out) {
  switch ((uint32_t)strategy < 4u ? strategy : 2) {
    case 0: encode_image<0>(h, w, gh, gw, stride, src, out); break;
    case 1: encode_image<1>(h, w, gh, gw, stride, src, out); break;
    case 2: encode_image<2>(h, w, gh, gw, stride, src, out); break;
    default: encode_image<3>(h, w, gh, gw, stride, src, out); break;
  }
  return 1;
}

// n words -> n x 16 texels in raster order (4 y + x), four bytes each
extern "C" void etc2a1_emul_decode_words(uint32_t n, int swap, const uint8_t *words, uint8_t *rgba) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t w[2], px[16];
    memcpy(w, words + (size_t)i * 8, 8);
    decode_etc2_a1(w[0], w[1], swap != 0, px);
    memcpy(rgba + (size_t)i * 64, px, 64);
  }
}
