// TEST INFRASTRUCTURE ONLY.  The T / H search of image-compression_amd/csrc/etc2_th_block.h and the ICAMD_ETC2_RGB8 routines it
// follows, compiled for the HOST (g++ -DICAMD_HOST_EMULATION, like etc2_colour_emul.cc) so that the CPU tier checks it against
// the numpy definition (tests/etc2_th_oracle.py, tests/test_etc2_th_host.py).  Never linked into libic_amd.so; the product has
// no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "etc1_block.h"
#include "etc2_colour_block.h"
#include "etc2_th_block.h"
#include "emul_violations.h"

using namespace icamd;

template <int COMPS>
static void encode_image(uint32_t st, int modes, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride,
                         const uint8_t *src, uint8_t *out) {
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
      Out8 o = etc2_rgb8_choose(px, c), th;  // the first launch's word ...
      if (modes == 1 && etc2_th_choose(px, o, &th)) o = th;  // ... and what the second launch leaves in its place
      memcpy(out + ((size_t)br * cols + bc) * 8, &o, 8);
    }
}

// icamd_encode_etc2_device(ICAMD_ETC2_RGB8, strategy, modes, ...) as the kernels run it, a "wave" being one block.
extern "C" int etc2th_emul_encode(int strategy, int modes, int comps, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw,
                                  uint32_t stride, const uint8_t *src, uint8_t *out) {
  const uint32_t st = (uint32_t)strategy < 4u ? (uint32_t)strategy : 2u;
  if (comps == 3) encode_image<3>(st, modes, h, w, gh, gw, stride, src, out);
  else if (comps == 4) encode_image<4>(st, modes, h, w, gh, gw, stride, src, out);
  else return 0;
  return 1;
}

// n blocks of 16 texels in raster order (three bytes each) -> the search's key per block: err << 6 | order, order = 24 partition
// + 8 candidate + di; 0xffffffff where no partition survives.
extern "C" void etc2th_emul_search(uint32_t n, const uint8_t *rgb, uint32_t *keys) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t s[16], ca, cb;
    for (int p = 0; p < 16; ++p) {
      const uint8_t *q = rgb + ((size_t)i * 16 + p) * 3;
      s[p] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
    }
    keys[i] = etc2_th_search(s, etc2_sum_squares(s), &ca, &cb);
  }
}

// q = (30 S + 255 n) / (510 n) through the routine the kernels use
extern "C" uint32_t etc2th_emul_quantise(uint32_t sum, uint32_t n) { return etc2_th_quantise(sum, n); }
