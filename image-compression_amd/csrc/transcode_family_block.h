// transcode_family_block.h -- DXT1 -> ETC2 RGB8, BC4 -> EAC R11 and BC5 -> EAC RG11 in the compressed domain (EXTENSIONS,
// include/ic_amd.h icamd_transcode_dxt1_to_etc2_rgb8 / _bc4_to_eac_r11 / _bc5_to_eac_rg11), one block per lane.
//
// DEFINITIONS: the output bytes are what the target encoder (ICAMD_ETC2_RGB8 kHeuristic on 3 components, ICAMD_EAC_R11 on 1,
// ICAMD_EAC_RG11 on 2; no swap) writes for the 4 x 4 image the source decoder (ICAMD_DXT1, ICAMD_BC4, ICAMD_BC5; no swap)
// produces from the input bytes.
//   * BC4 -> R11: a BC4 word is a DXT5 alpha word and an R11 word is the EAC word of ETC2 RGBA8, so the block is
//     transcode_dxt5_alpha_to_eac (transcode5_block.h) as it stands: the search on the eight palette values weighted by use.
//   * BC5 -> RG11: that, on bytes 0..7 and on bytes 8..15, back to back in one lane (DESIGN.md 3.15 for why).
//   * DXT1 -> ETC2 RGB8: E = transcode_dxt1_block_to_etc1 (blockops_block.h), P = the least-squares planar word of the sixteen
//     decoded texels (etc2_colour_block.h), the result P where its squared error is STRICTLY smaller than E's, else E.  No pixel
//     is assembled: the palette stays in the channel planes the ETC1 transcoder sets up (byte k of P[ch] = channel ch of entry
//     k), a pixel row's four values of a channel are ONE v_perm of the plane through dxt_row_selector, and that dword is what
//     etc2_planar_fit takes its v_dot4 sums from and what the squared errors Sum d^2 - 2 Sum s d + Sum s^2 run on.  E is
//     decoded the same way (etc1_palette_planes / etc1_row_selector), the plane is evaluated per channel row.  Same sums, same
//     quantiser, same packer, same strict comparison as etc2_rgb8_choose on decode_dxt_colors' pixels: the same bytes (checked
//     block by block in tests/host_emul).
#ifndef ICAMD_TRANSCODE_FAMILY_BLOCK_H_
#define ICAMD_TRANSCODE_FAMILY_BLOCK_H_

#include "etc2_colour_block.h"
#include "transcode5_block.h"

namespace icamd {

// Sum s^2 + Sum d^2 - 2 Sum s d over four row dwords of one channel (byte x = texel (x, y)), added to acc.  A channel adds at
// most 16 * 255^2 < 2^21: three of them stay far below 2^31 in either sign.
ICAMD_DEV int32_t family_rows_sse(const uint32_t s[4], const uint32_t d[4], int32_t acc) {
  uint32_t sq = 0u, sd = 0u;
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    sq = udot4(d[y], d[y], udot4(s[y], s[y], sq));
    sd = udot4(s[y], d[y], sd);
  }
  return acc + (int32_t)sq - 2 * (int32_t)sd;
}

// w0, bits: a DXT1 block (c0 | c1 << 16, sixteen 2-bit indices) -> the ICAMD_ETC2_RGB8 block of the pixels it decodes to.
ICAMD_DEV Out8 transcode_dxt1_block_to_etc2_rgb8(uint32_t w0, uint32_t bits) {
  const Out8 e = transcode_dxt1_block_to_etc1(w0, bits);
  uint32_t P[3];
  dxt_palette_planes(w0, false, P);  // (the transcoder's own planes: one computation once both are inlined)
  uint32_t sel[4], esel[4], PE[2][3];
  const bool eflip = etc1_palette_planes(e.lo, PE);
  const uint32_t elo = perm(0u, e.hi, 0x00010203u);
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    sel[y] = dxt_row_selector(bits, y);
    esel[y] = etc1_row_selector(elo, y, eflip);
  }
  uint32_t code[9];
  int32_t sse_e = 0, sse_p = 0;
  ICAMD_UNROLL
  for (int ch = 0; ch < 3; ++ch) {
    uint32_t s[4], d[4];
    int32_t sum = 0, sxv = 0, sy = 0;
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      s[y] = perm(P[ch], P[ch], sel[y]);
      d[y] = perm(PE[1][ch], PE[0][ch], esel[y]);
      const int32_t rs = (int32_t)udot4(s[y], 0x01010101u, 0u);  // etc2_planar_fit's sums, on the same dword
      sum += rs;
      sxv += (int32_t)udot4(s[y], 0x03020100u, 0u);
      sy += (2 * y - 3) * rs;
    }
    sse_e = family_rows_sse(s, d, sse_e);
    const int32_t sx = 2 * sxv - 3 * sum;
    const uint32_t maxcode = ch == 1 ? 127u : 63u;
    const uint32_t co = etc2_planar_code(5 * sum - 3 * sx - 3 * sy, maxcode);
    const uint32_t chh = etc2_planar_code(5 * sum + 5 * sx - 3 * sy, maxcode);
    const uint32_t cv = etc2_planar_code(5 * sum - 3 * sx + 5 * sy, maxcode);
    code[ch] = co; code[3 + ch] = chh; code[6 + ch] = cv;
    // etc2_planar_texels of this channel, a row at a time into the bytes of a dword
    const int32_t o = ch == 1 ? etc2_expand7(co) : etc2_expand6(co);
    const int32_t dx = (ch == 1 ? etc2_expand7(chh) : etc2_expand6(chh)) - o;
    const int32_t dy = (ch == 1 ? etc2_expand7(cv) : etc2_expand6(cv)) - o;
    int32_t row = 4 * o + 2;
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      const uint32_t t0 = clamp255(row >> 2), t1 = clamp255((row + dx) >> 2);
      const uint32_t t2 = clamp255((row + 2 * dx) >> 2), t3 = clamp255((row + 3 * dx) >> 2);
      d[y] = t0 | t1 << 8 | t2 << 16 | t3 << 24;
      row += dy;
    }
    sse_p = family_rows_sse(s, d, sse_p);
  }
  const Out8 pl = etc2_planar_pack(code);
  const bool planar = sse_p < sse_e;  // both carry the same Sum s^2, both are >= 0
  const Out8 o = { planar ? pl.lo : e.lo, planar ? pl.hi : e.hi };
  return o;
}

// A BC4 word -> the EAC R11 word of the sixteen values it decodes to.
ICAMD_DEV Out8 transcode_bc4_block_to_eac_r11(uint32_t w0, uint32_t w1) { return transcode_dxt5_alpha_to_eac(w0, w1); }

// A BC5 block (R word, G word) -> the EAC RG11 block: the two channel searches back to back.
ICAMD_DEV void transcode_bc5_block_to_eac_rg11(const uint32_t w[4], uint32_t out[4]) {
  const Out8 r = transcode_dxt5_alpha_to_eac(w[0], w[1]);
  const Out8 g = transcode_dxt5_alpha_to_eac(w[2], w[3]);
  out[0] = r.lo; out[1] = r.hi; out[2] = g.lo; out[3] = g.hi;
}

}  // namespace icamd
#endif  // ICAMD_TRANSCODE_FAMILY_BLOCK_H_
