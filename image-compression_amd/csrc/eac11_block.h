// eac11_block.h -- EAC R11 / RG11 (EXTENSION, include/ic_amd.h ICAMD_EAC_R11), one block per lane.
//
// An R11 block is one EAC word with the bit layout of the ETC2 RGBA8 alpha word (etc2_block.h): byte 0 = base, byte 1 =
// multiplier << 4 | table, sixteen 3-bit indices, texel i = 4 x + y.  An RG11 block is the word of R, then the word of G.
//
// Encode is encode_eac_alpha of etc2_block.h, unchanged, on the channel's sixteen bytes: the words ARE the alpha half's of
// ICAMD_ETC2_RGBA8 for the same sixteen values, by construction and not by a second copy of the search.
//
// Decode differs from the alpha decoder in precision and at multiplier 0 (Khronos EAC, unsigned 11-bit):
//   v11 = clamp(8 base + 4 + M[table][index] * (multiplier == 0 ? 1 : 8 multiplier), 0, 2047),
// and the byte written is v11 >> 3 (the top byte of the specification's 16-bit expansion v11 << 5 | v11 >> 6).  For a
// multiplier of 1 or more that byte is clamp(base + M multiplier, 0, 255), the alpha decoder's; for multiplier 0 the alpha
// decoder gives `base` and this one base + (4 + M) >> 3, e.g. the word 80 0d 7e 49 24 92 49 24 (base 128, table 13, indices
// 3, 7, 4, 4, ...) decodes to v11 = 1018, 1037, 1028, ... and the bytes 127, 129, 128, ...
#ifndef ICAMD_EAC11_BLOCK_H_
#define ICAMD_EAC11_BLOCK_H_

#include "etc2_block.h"

namespace icamd {

// The EAC word of one channel given as four pixel rows, byte x of r[y] = texel (x, y).
ICAMD_DEV Out8 encode_eac11_rows(const uint32_t r[4]) {
  uint32_t a[16];
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) a[p] = bfe(r[p >> 2], 8 * (p & 3), 8);
  return encode_eac_alpha(a);
}

// w0, w1: the 8 bytes of an EAC word as little-endian dwords.  rows[y] byte x = the decoded byte of texel (x, y): the eight
// values of the word as the bytes of two dwords, and one v_perm_b32 per row whose selector bytes are the row's indices.
ICAMD_DEV void decode_eac11(uint32_t w0, uint32_t w1, uint32_t rows[4]) {
  const uint32_t hi = perm(0u, w0, 0x00010203u), lo = perm(0u, w1, 0x00010203u);
  const uint32_t mul = (hi >> 20) & 15u, mags = eac_mags((hi >> 16) & 15u);
  const int32_t b = (int32_t)(8u * (hi >> 24) + 4u), m = mul == 0u ? 1 : (int32_t)(8u * mul);
  uint32_t tlo = 0u, thi = 0u;  // values 0..3 and 4..7, one byte each
  ICAMD_UNROLL
  for (int k = 0; k < 4; ++k) {
    const int32_t g = (int32_t)bfe(mags, 8 * k, 8);
    tlo |= ((uint32_t)imed3(imad24(-g, m, b), 0, 2047) >> 3) << (8 * k);
    thi |= ((uint32_t)imed3(imad24(g - 1, m, b), 0, 2047) >> 3) << (8 * k);
  }
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    uint32_t sel = 0u;
    ICAMD_UNROLL
    for (int x = 0; x < 4; ++x) {
      sel |= eac_index(hi, lo, 4 * x + y) << (8 * x);
    }
    rows[y] = perm(thi, tlo, sel);
  }
}

}  // namespace icamd
#endif  // ICAMD_EAC11_BLOCK_H_
