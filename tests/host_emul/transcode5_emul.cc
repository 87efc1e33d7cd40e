// TEST INFRASTRUCTURE ONLY.  The DXT5 -> ETC2 RGBA8 block math of image-compression_amd/csrc/transcode5_block.h compiled for the
// HOST (g++ -DICAMD_HOST_EMULATION, like etc2_emul.cc) so that the CPU tier checks it against the definition
// (tests/transcode5_oracle.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <cstring>

#include "transcode5_block.h"
#include "emul_violations.h"

using namespace icamd;

// The transcode as the kernel runs it: every whole 16-byte block in place, the tail bytes untouched.
extern "C" void transcode5_emul(uint8_t *blocks, size_t n_bytes) {
  for (size_t k = 0; k + 16 <= n_bytes; k += 16) {
    uint32_t w[4], o[4];
    memcpy(w, blocks + k, 16);
    transcode_dxt5_block_to_etc2_rgba8(w, o);
    memcpy(blocks + k, o, 16);
  }
}

// n DXT5 alpha words (8 bytes each) -> n EAC words by the palette-domain search ...
extern "C" void transcode5_emul_alpha_palette(size_t n, const uint8_t *words, uint8_t *out) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[2];
    memcpy(w, words + 8 * i, 8);
    const Out8 e = transcode_dxt5_alpha_to_eac(w[0], w[1]);
    memcpy(out + 8 * i, &e, 8);
  }
}

// ... and by the pixel route: decode_dxt5_alpha's sixteen alphas through encode_eac_alpha (etc2_block.h), the search the ETC2
// RGBA8 encoder runs.
extern "C" void transcode5_emul_alpha_expanded(size_t n, const uint8_t *words, uint8_t *out) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[2], px[16] = { 0 }, a[16];
    memcpy(w, words + 8 * i, 8);
    decode_dxt5_alpha(w[0], w[1], px);
    for (int p = 0; p < 16; ++p) a[p] = px[p] >> 24;
    const Out8 e = encode_eac_alpha(a);
    memcpy(out + 8 * i, &e, 8);
  }
}

// The colour half alone: n 8-byte colour words as the DXT1 -> ETC1 transcoder takes them (always4 = 0) or as a DXT5 block's (1).
extern "C" void transcode5_emul_colour(int always4, size_t n, const uint8_t *words, uint8_t *out) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[2];
    memcpy(w, words + 8 * i, 8);
    const Out8 c = always4 ? transcode_dxt1_block_to_etc1<true>(w[0], w[1]) : transcode_dxt1_block_to_etc1(w[0], w[1]);
    memcpy(out + 8 * i, &c, 8);
  }
}
