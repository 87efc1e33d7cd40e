// TEST INFRASTRUCTURE ONLY.  The block math of image-compression_amd/csrc/transcode_family_block.h (DXT1 -> ETC2 RGB8, BC4 -> EAC
// R11, BC5 -> EAC RG11) compiled for the HOST (g++ -DICAMD_HOST_EMULATION, like transcode5_emul.cc) so that the CPU tier checks
// it against the definition (tests/transcode_family_oracle.py) and against the routines it must agree with.  Never linked into
// libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <cstring>

#include "transcode_family_block.h"
#include "emul_violations.h"

using namespace icamd;

// The transcodes as the kernels run them: every whole block in place, the tail bytes untouched.  kind 0: DXT1 -> ETC2 RGB8,
// 1: BC4 -> EAC R11, 2: BC5 -> EAC RG11.
extern "C" void transcode_family_emul(int kind, uint8_t *blocks, size_t n_bytes) {
  const size_t block = kind == 2 ? 16 : 8;
  for (size_t k = 0; k + block <= n_bytes; k += block) {
    uint32_t w[4], o[4];
    memcpy(w, blocks + k, block);
    if (kind == 2) {
      transcode_bc5_block_to_eac_rg11(w, o);
    } else {
      const Out8 r = kind == 0 ? transcode_dxt1_block_to_etc2_rgb8(w[0], w[1]) : transcode_bc4_block_to_eac_r11(w[0], w[1]);
      o[0] = r.lo; o[1] = r.hi;
    }
    memcpy(blocks + k, o, block);
  }
}

// n DXT1 blocks -> what the existing DXT1 -> ETC1 block routine writes for them
extern "C" void transcode_family_emul_dxt1_to_etc1(size_t n, const uint8_t *words, uint8_t *out) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[2];
    memcpy(w, words + 8 * i, 8);
    const Out8 c = transcode_dxt1_block_to_etc1(w[0], w[1]);
    memcpy(out + 8 * i, &c, 8);
  }
}

// n DXT1 blocks by the pixel route: decode_dxt_colors' sixteen pixels through the ETC1 encoder (kHeuristic) and
// etc2_rgb8_choose, the block routine of the ICAMD_ETC2_RGB8 encoder
extern "C" void transcode_family_emul_dxt1_pixels(size_t n, const uint8_t *words, uint8_t *out) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[2], px[16];
    memcpy(w, words + 8 * i, 8);
    decode_dxt_colors(w[0], w[1], false, false, px);
    const Out8 c = etc2_rgb8_choose(px, encode_etc1_block(px, 3u));
    memcpy(out + 8 * i, &c, 8);
  }
}

// n BC4 words as the alpha words of DXT5 blocks (colour words zero) -> bytes 0..7 of the DXT5 -> ETC2 RGBA8 transcoder's output
extern "C" void transcode_family_emul_dxt5_alpha(size_t n, const uint8_t *words, uint8_t *out) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[4] = { 0, 0, 0, 0 }, o[4];
    memcpy(w, words + 8 * i, 8);
    transcode_dxt5_block_to_etc2_rgba8(w, o);
    memcpy(out + 8 * i, o, 8);
  }
}
