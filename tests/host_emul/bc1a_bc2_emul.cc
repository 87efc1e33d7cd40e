// TEST INFRASTRUCTURE ONLY.  The BC1A / BC2 block math of image-compression_amd/csrc/bc1a_block.h (both decoders, the masked
// three-colour encoder, the per-block choice, BC2's alpha word) and the DXT colour block it is built on, compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION, like etc2_a1_emul.cc) so that the CPU tier checks it against the numpy definition
// (tests/test_bc1a_bc2_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "bc1a_block.h"
#include "emul_violations.h"

using namespace icamd;

// The ICAMD_BC1A (bc2 == 0) or ICAMD_BC2 encoder as the kernels run it (bc1a_bc2_kernels.hip) on an RGBA8 image; a "wave" is one
// block here.
extern "C" int bc1a_bc2_emul_encode(int bc2, int swap, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride,
                                    const uint8_t *src, uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t px[16];
      load_block<4>(src, h, w, stride, br * 4, bc * 4, px);
      BlockStash stash;
      const size_t k = (size_t)br * cols + bc;
      if (bc2) {
        const Out8 a = encode_bc2_alpha_block(px);
        const Out8 c = encode_dxt_color_block(px, swap != 0, true, stash);
        memcpy(out + k * 16, &a, 8);
        memcpy(out + k * 16 + 8, &c, 8);
      } else {
        const Out8 c = encode_bc1a_block(px, swap != 0, stash);
        memcpy(out + k * 8, &c, 8);
      }
    }
  return 1;
}

// The masked path alone on n blocks of sixteen RGBA texels (64 bytes each): what a lane computes when ANOTHER lane of its wave
// has a transparent texel.  Blocks without one are the caller's to ignore.
extern "C" void bc1a_emul_encode_masked(uint32_t n, int swap, const uint8_t *texels, uint8_t *out) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t px[16];
    memcpy(px, texels + (size_t)i * 64, 64);
    BlockStash stash;
    const Out8 c = encode_bc1a_masked_block(px, swap != 0, stash);
    memcpy(out + (size_t)i * 8, &c, 8);
  }
}

// The constant-colour proof of the header: the DXT1 colour block of sixteen equal opaque texels, for all 2^24 colours, under
// both decoders.  counts[i]: blocks that store index i; returns through bad[0] the blocks the BC1A decoder does not read as
// opaque texels of the DXT1 decoder's RGB, through bad[1] the blocks with c0 == c1 and an index other than 0.
#include "decode_block.h"
extern "C" void bc1a_emul_const_scan(uint64_t counts[4], uint64_t bad[2]) {
  counts[0] = counts[1] = counts[2] = counts[3] = bad[0] = bad[1] = 0;
  for (uint32_t v = 0; v < (1u << 24); ++v) {
    uint32_t px[16], a[16], b[16];
    for (int p = 0; p < 16; ++p) px[p] = v | 0xff000000u;
    BlockStash stash;
    const Out8 c = encode_dxt_color_block(px, false, false, stash);
    ++counts[c.hi & 3u];
    decode_bc1a(c.lo, c.hi, false, a);
    decode_dxt_colors(c.lo, c.hi, false, false, b);
    bool same = true;
    for (int p = 0; p < 16; ++p) same = same && a[p] == (b[p] | 0xff000000u);
    if (!same) ++bad[0];
    if ((c.lo & 0xffffu) == (c.lo >> 16) && c.hi != 0u) ++bad[1];
  }
}

// n blocks -> n x 16 texels in raster order (4 y + x), four bytes each
extern "C" void bc1a_bc2_emul_decode(int bc2, uint32_t n, int swap, const uint8_t *blocks, uint8_t *rgba) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t w[4] = { 0, 0, 0, 0 }, px[16];
    memcpy(w, blocks + (size_t)i * (bc2 ? 16 : 8), bc2 ? 16 : 8);
    if (bc2) decode_bc2(w, swap != 0, px);
    else decode_bc1a(w[0], w[1], swap != 0, px);
    memcpy(rgba + (size_t)i * 64, px, 64);
  }
}
