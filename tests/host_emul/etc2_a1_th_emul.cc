// TEST INFRASTRUCTURE ONLY.  The colour-mode passes of icamd_encode_etc2_colour_device compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION, like etc2_th_emul.cc): the masked T / H search of image-compression_amd/csrc/etc2_a1_th_block.h,
// the ETC2 RGBA8 chaining of etc2_rgb8_choose and etc2_th_choose, and the block walk of both passes -- the first launch's word,
// then what the second launch leaves in its place -- so that the CPU tier checks them against the numpy definition
// (tests/etc2_a1_th_oracle.py, tests/test_etc2_colour_modes_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "etc1_block.h"
#include "etc2_block.h"
#include "etc2_a1_th_block.h"
#include "emul_violations.h"

using namespace icamd;

template <int ST>
static Out8 etc1_word(const uint32_t px[16]) {
  if (ST == 3) return encode_etc1_block<false>(px, 3u);
  const uint32_t spread = etc1_block_spread(px);
  return etc1_encode_classified<ST>(px, etc1_constant_block(px, spread), spread >= ICAMD_ETC1_BUSY_SPREAD);
}

// codec 21: 8 bytes per block; codec 16: 16.  modes: ICAMD_ETC2_COLOUR_*.
template <int ST>
static void encode_image(int codec, int modes, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw, uint32_t stride,
                         const uint8_t *src, uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t px[16];
      load_block<4>(src, h, w, stride, br * 4, bc * 4, px);
      const size_t at = (size_t)br * cols + bc;
      if (codec == 21) {
        Out8 c = { 0u, 0u };
        if (etc2_a1_opaque_mask(px) == 0xffffu) c = etc1_word<ST>(px);  // (a "wave" is one block here)
        Out8 o = etc2_a1_block<ST>(px, c), th;                     // the first launch's word ...
        if (modes == 2 && etc2_a1_th_choose(px, o, &th)) o = th;  // ... and what the second launch leaves in its place
        memcpy(out + at * 8, &o, 8);
      } else {
        uint32_t a[16];
        for (int p = 0; p < 16; ++p) a[p] = px[p] >> 24;  // raster order, as etc2_encode_one hands them over
        const Out8 e = encode_eac_alpha(a);
        Out8 c = etc1_word<ST>(px);
        if (modes == 1) c = etc2_rgba8_colour_choose<false>(px, c);
        if (modes == 2) c = etc2_rgba8_colour_choose<true>(px, c);
        memcpy(out + at * 16, &e, 8);
        memcpy(out + at * 16 + 8, &c, 8);
      }
    }
}

// icamd_encode_etc2_colour_device(codec 16 or 21, strategy, modes, 4, ...) as the kernels run it, a "wave" being one block.
extern "C" int etc2cm_emul_encode(int codec, int strategy, int modes, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw,
                                  uint32_t stride, const uint8_t *src, uint8_t *out) {
  if ((codec != 16 && codec != 21) || modes < 0 || modes > 2) return 0;
  switch ((uint32_t)strategy < 4u ? strategy : 2) {
    case 0: encode_image<0>(codec, modes, h, w, gh, gw, stride, src, out); break;
    case 1: encode_image<1>(codec, modes, h, w, gh, gw, stride, src, out); break;
    case 2: encode_image<2>(codec, modes, h, w, gh, gw, stride, src, out); break;
    default: encode_image<3>(codec, modes, h, w, gh, gw, stride, src, out); break;
  }
  return 1;
}

// n blocks of 16 RGBA texels in raster order -> the masked search's key per block: err << 6 | order, order = 24 partition + 8
// candidate + di; 0xffffffff where no partition survives.  Blocks must have 1..15 transparent texels.
extern "C" void etc2cm_emul_masked_search(uint32_t n, const uint8_t *rgba, uint32_t *keys) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t px[16], s[16], ca, cb, cnt = 0u;
    memcpy(px, rgba + (size_t)i * 64, 64);
    const uint32_t o = etc2_a1_opaque_mask(px);
    for (int p = 0; p < 16; ++p) {
      s[p] = (o >> p) & 1u ? px[p] & 0x00ffffffu : 0u;
      cnt += (o >> p) & 1u;
    }
    keys[i] = etc2_a1_th_search(s, o, cnt, etc2_sum_squares(s), &ca, &cb);
  }
}
