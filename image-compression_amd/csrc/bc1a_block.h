// bc1a_block.h -- BC1 with punch-through alpha ("DXT1A") and BC2 ("DXT3") block math (EXTENSIONS, include/ic_amd.h ICAMD_BC1A,
// ICAMD_BC2), one block per lane: the two decoders as the formats define them, the masked three-colour encoder
// of BC1A and the 4-bit alpha word of BC2.  The opaque blocks of BC1A and the colour half of BC2 are encode_dxt_color_block of
// dxt_block.h, called as it is.
#ifndef ICAMD_BC1A_BLOCK_H_
#define ICAMD_BC1A_BLOCK_H_

#include "decode_block.h"  // expand565_packed, blend_packed
#include "dxt_block.h"

namespace icamd {

// ---- decoders.  Texels as dwords in the OUTPUT memory byte order (byte 3 = alpha), texel p = 4 y + x.

// BC1 as the format defines it: c0 > c1 four opaque colours; otherwise -- c0 == c1 included -- three, and index 3 is (0, 0, 0, 0).
// (decode_dxt_colors keeps the reference's c0 == c1 rule and opaque black: that one is ICAMD_DXT1's.)
ICAMD_DEV void decode_bc1a(uint32_t w0, uint32_t bits, bool swap, uint32_t px[16]) {
  const uint32_t c0 = w0 & 0xffffu, c1 = w0 >> 16;
  uint32_t e0 = expand565_packed(c0), e1 = expand565_packed(c1);
  if (swap) {  // stored R goes to the third byte, as for DXT5
    e0 = perm(e0, e0, 0x03000102u);
    e1 = perm(e1, e1, 0x03000102u);
  }
  const bool four = c0 > c1;
  uint32_t col[4];
  col[0] = e0 | 0xff000000u;
  col[1] = e1 | 0xff000000u;
  col[2] = (four ? blend_packed(e0, e1, 2, 1) : blend_packed(e0, e1, 1, 1)) | 0xff000000u;
  col[3] = four ? (blend_packed(e0, e1, 1, 2) | 0xff000000u) : 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint32_t code = (bits >> (2 * p)) & 3u;
    px[p] = code == 0u ? col[0] : code == 1u ? col[1] : code == 2u ? col[2] : col[3];
  }
}

// BC2: w[0..1] the alpha word (nibble p = bits 4p..4p+3, times 17), w[2..3] the colour word, ALWAYS four colours.
ICAMD_DEV void decode_bc2(const uint32_t *w, bool swap, uint32_t px[16]) {
  uint32_t col[4];
  col[0] = expand565_packed(w[2] & 0xffffu);
  col[1] = expand565_packed(w[2] >> 16);
  if (swap) {
    col[0] = perm(col[0], col[0], 0x03000102u);
    col[1] = perm(col[1], col[1], 0x03000102u);
  }
  col[2] = blend_packed(col[0], col[1], 2, 1);
  col[3] = blend_packed(col[0], col[1], 1, 2);
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint32_t code = (w[3] >> (2 * p)) & 3u;
    const uint32_t a = ((p < 8 ? w[0] : w[1]) >> (4 * (p & 7))) & 15u;
    px[p] = (code == 0u ? col[0] : code == 1u ? col[1] : code == 2u ? col[2] : col[3]) | (a * 17u) << 24;
  }
}

// ---- BC2's alpha word: nibble p = Quantize8(alpha_p, 15), i = 15 a + 128, (i + (i >> 8)) >> 8 (the reference's rounding,
// color_util.h:156-164).  Alpha = byte 3 of each texel.  Two texels per instruction: texel q and texel q + 8 share a dword as
// 16-bit lanes (i <= 3953: nothing carries from one lane into the other).
ICAMD_DEV Out8 encode_bc2_alpha_block(const uint32_t px[16]) {
  uint32_t lo = 0u, hi = 0u;
  ICAMD_UNROLL
  for (int q = 7; q >= 0; --q) {
    const uint32_t a2 = perm(px[q + 8], px[q], 0x0c070c03u);  // {alpha(q), 0, alpha(q + 8), 0}
    const uint32_t i2 = pk_mad_u16(a2, 0x000f000fu, 0x00800080u);
    const uint32_t n2 = pk_lshr16(i2 + pk_lshr16(i2, 8), 8);
    lo = lo << 4 | (n2 & 0xffffu);
    hi = hi << 4 | n2 >> 16;
  }
  Out8 o = { lo, hi };
  return o;
}

// True iff a texel of the block is transparent (byte 3 < 128: the dword's top bit is clear).
ICAMD_DEV bool bc1a_has_transparent(const uint32_t px[16]) {
  uint32_t m = umin3(px[0], px[1], px[2]);
  ICAMD_UNROLL
  for (int p = 3; p < 15; p += 2) m = umin3(m, px[p], px[p + 1]);
  return umin(m, px[15]) < 0x80000000u;
}

// ---- BC1A, a block with at least one transparent texel (include/ic_amd.h ICAMD_BC1A, cases 1 and 3).  px[] in memory byte
// order; swap = source is BGRA.
//  * Endpoints: the min / max key trees of encode_dxt_color_block (16 L + p and 16 L + 15 - p, L = 4 R + 8 G + B: "the first
//    texel with the smallest / largest L") with the transparent texels' keys neutralised -- 0xffffffff in the min tree, 0 in the
//    max tree -- so the extremes are taken over the opaque texels alone; both 565 colours through quantize565, stored c0 <= c1.
//  * Palette: the decoder's own, P0 = E(c0), P1 = E(c1), P2 = (P0 + P1) >> 1 per byte (v_lerp_u8).
//  * Indices: argmin_k |t - P_k|^2 = argmin_k (P_k . P_k - 2 t . P_k), the texel's own square being common to the three.  With
//    s_k = t . P_k one v_dot4_u32_u8 (the palette's byte 3 is 0, so the texel's alpha drops out), the key
//    4 (C - P_k . P_k + 2 s_k) + (3 - k), C = 3 * 255^2, is largest for the nearest colour and, among equals, for the smallest k;
//    its low two bits are 3 - k = ~k.  Exact: everything is an integer below 2^22.  A transparent texel's key is 0: index 3.
// A block whose sixteen texels are transparent comes out as 00 00 00 00 ff ff ff ff.
template <typename Stash>
ICAMD_DEV Out8 encode_bc1a_masked_block(const uint32_t px[16], bool swap, Stash &stash) {
  const uint32_t w16 = swap ? 0x00408010u : 0x00108040u;
  uint32_t kmin[16], kmax[16];
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const bool clear = px[p] < 0x80000000u;
    const uint32_t key = udot4(px[p], w16, (uint32_t)p);  // 16 L + p
    kmin[p] = clear ? 0xffffffffu : key;
    kmax[p] = clear ? 0u : key + (uint32_t)(15 - 2 * p);  // 16 L + (15 - p)
  }
  uint32_t lo_key = umin3(kmin[0], kmin[1], kmin[2]);
  uint32_t hi_key = umax3(kmax[0], kmax[1], kmax[2]);
  ICAMD_UNROLL
  for (int p = 3; p < 15; p += 2) {
    lo_key = umin3(lo_key, kmin[p], kmin[p + 1]);
    hi_key = umax3(hi_key, kmax[p], kmax[p + 1]);
  }
  lo_key = umin(lo_key, kmin[15]);
  hi_key = umax(hi_key, kmax[15]);

  stash.put(px);
  const uint32_t lo_raw = stash.get(lo_key & 15u);
  const uint32_t hi_raw = stash.get(15u - (hi_key & 15u));
  const uint32_t sel = swap ? 0x03000102u : 0x03020100u;  // canonical channel order (byte 0 = R, byte 2 = B)
  const uint32_t b0 = perm(lo_raw, lo_raw, sel), b1 = perm(hi_raw, hi_raw, sel);
  const uint32_t qa = quantize565(bfe(b0, 0, 8), bfe(b0, 8, 8), bfe(b0, 16, 8));
  const uint32_t qb = quantize565(bfe(b1, 0, 8), bfe(b1, 8, 8), bfe(b1, 16, 8));
  const uint32_t c0 = umin(qa, qb), c1 = umax(qa, qb);

  // the palette in the texels' memory byte order (a distance does not depend on the order of its channels)
  uint32_t pal[3];
  pal[0] = expand565_packed(c0);
  pal[1] = expand565_packed(c1);
  if (swap) {
    pal[0] = perm(pal[0], pal[0], 0x03000102u);
    pal[1] = perm(pal[1], pal[1], 0x03000102u);
  }
  pal[2] = avg_u8(pal[0], pal[1]);
  uint32_t bias[3];
  ICAMD_UNROLL
  for (int k = 0; k < 3; ++k) bias[k] = 4u * (3u * 255u * 255u - udot4(pal[k], pal[k], 0u)) + (uint32_t)(3 - k);
  uint32_t acc = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint32_t k0 = (udot4(px[p], pal[0], 0u) << 3) + bias[0];
    const uint32_t k1 = (udot4(px[p], pal[1], 0u) << 3) + bias[1];
    const uint32_t k2 = (udot4(px[p], pal[2], 0u) << 3) + bias[2];
    const uint32_t best = px[p] < 0x80000000u ? 0u : umax3(k0, k1, k2);
    acc = alignbit(best, acc, 2);  // shift the winner's low two bits (~index) in from the top
  }
  const bool none_opaque = lo_key == 0xffffffffu;
  Out8 o = { none_opaque ? 0u : (c0 | c1 << 16), ~acc };
  return o;
}

// The ICAMD_BC1A block of the sixteen texels px.  A wave in which no lane has a transparent texel runs the DXT1 colour block
// alone -- a fully opaque image costs what ICAMD_DXT1 from RGBA8 costs plus the vote -- a wave in which every lane has one the
// masked path alone; a mixed wave runs both and each lane keeps its own.
template <typename Stash>
ICAMD_DEV Out8 encode_bc1a_block(const uint32_t px[16], bool swap, Stash &stash) {
  const bool masked = bc1a_has_transparent(px);
  Out8 o = { 0u, 0u };
  if (!wave_all(masked)) o = encode_dxt_color_block(px, swap, false, stash);
  if (!wave_all(!masked)) {
    const Out8 m = encode_bc1a_masked_block(px, swap, stash);
    if (masked) o = m;
  }
  return o;
}

}  // namespace icamd
#endif  // ICAMD_BC1A_BLOCK_H_
