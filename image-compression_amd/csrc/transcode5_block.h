// transcode5_block.h -- DXT5 -> ETC2 RGBA8 in the compressed domain (EXTENSION, include/ic_amd.h
// icamd_transcode_dxt5_to_etc2_rgba8), one block per lane.
//
// DEFINITION: the sixteen output bytes are what the ETC2 RGBA8 encoder (kHeuristic, no swap) writes for the 4 x 4 RGBA8 image the
// DXT5 decoder (no swap) produces from the sixteen input bytes.  Both blocks keep alpha in bytes 0..7 and colour in bytes 8..15:
//   * colour: transcode_dxt1_block_to_etc1<true> (blockops_block.h) -- the DXT1 -> ETC1 transcoder on the palette of a DXT5 colour
//     word, which is four colours whatever the order of its endpoints;
//   * alpha: encode_eac_alpha (etc2_block.h) of the decoded alphas, WITHOUT decoding them.  A DXT5 alpha word decodes to at most
//     eight distinct values -- its palette (dxt5_alpha_planes) -- so a candidate's error is a sum over the eight palette entries
//     weighted by how many texels use each, 8 nearest-value searches where encode_eac_alpha runs 16, and the texels' EAC indices
//     are an eight-entry table look-up of their DXT5 codes.  Grouping equal texels changes no sum and no tie: same candidates, same
//     order, same strictly-smaller replacement, same wave-uniform exit, the same bytes (checked block by block in tests/host_emul).
#ifndef ICAMD_TRANSCODE5_BLOCK_H_
#define ICAMD_TRANSCODE5_BLOCK_H_

#include "blockops_block.h"
#include "etc2_block.h"

namespace icamd {

#if defined(ICAMD_HOST_EMULATION)
ICAMD_DEV uint32_t popc32(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
#else
ICAMD_DEV uint32_t popc32(uint32_t v) { return (uint32_t)__popc(v); }  // v_bcnt_u32_b32
#endif

// How many of the sixteen texels use each 3-bit code.  lo24 / hi24: the codes of pixels 0-7 / 8-15.  The three bits of the codes
// as planes -- pixel p's at bit 3 p, pixel 8 + p's at bit 3 p + 1 -- make "code == j" one bit per texel: two ANDs and a bit count.
ICAMD_DEV void dxt5_code_counts(uint32_t lo24, uint32_t hi24, uint32_t count[8]) {
  const uint32_t kLow = 0x249249u, kHigh = kLow << 1, kAll = kLow | kHigh;
  const uint32_t c0 = (lo24 & kLow) | (hi24 & kLow) << 1;
  const uint32_t c1 = ((lo24 >> 1) & kLow) | (hi24 & kHigh);
  const uint32_t c2 = ((lo24 >> 2) & kLow) | ((hi24 >> 1) & kHigh);
  const uint32_t n0 = c0 ^ kAll, n1 = c1 ^ kAll, n2 = c2 ^ kAll;
  ICAMD_UNROLL
  for (int j = 0; j < 8; ++j) count[j] = popc32(((j & 1) ? c0 : n0) & ((j & 2) ? c1 : n1) & ((j & 4) ? c2 : n2));
}

// eac_sse (etc2_block.h) with the texels grouped by value: count[j] texels hold pal[j].  e <= 255 and count <= 16, so e * count
// <= 4 080 and both products are 24-bit multiplies.
ICAMD_DEV uint32_t eac_sse_palette(const uint32_t pal[8], const uint32_t count[8], const int32_t v[8]) {
  uint32_t sse = 0;
  ICAMD_UNROLL
  for (int j = 0; j < 8; ++j) {
    uint32_t e = umin3(sad_u32(pal[j], (uint32_t)v[0], 0u), sad_u32(pal[j], (uint32_t)v[1], 0u), sad_u32(pal[j], (uint32_t)v[2], 0u));
    e = umin3(e, sad_u32(pal[j], (uint32_t)v[3], 0u), sad_u32(pal[j], (uint32_t)v[4], 0u));
    e = umin3(e, sad_u32(pal[j], (uint32_t)v[5], 0u), sad_u32(pal[j], (uint32_t)v[6], 0u));
    e = umin(e, sad_u32(pal[j], (uint32_t)v[7], 0u));
    sse = umad24(umad24(e, count[j], 0u), e, sse);
  }
  return sse;
}

// encode_eac_alpha's search (etc2_block.h) on the palette: table << 12 | multiplier << 8 | base of the winner.  lo and hi are the
// extremes of the entries some texel uses; an entry nobody uses weighs nothing in the error and must not widen the range either.
ICAMD_DEV uint32_t eac_search_palette(const uint32_t pal[8], const uint32_t count[8]) {
  uint32_t lo = 255u, hi = 0u;
  ICAMD_UNROLL
  for (int j = 0; j < 8; ++j) {
    lo = umin(lo, count[j] ? pal[j] : 255u);
    hi = umax(hi, count[j] ? pal[j] : 0u);
  }
  const uint32_t range2 = 2u * (hi - lo), mid2 = lo + hi + 1u;
  uint32_t best_sse = 0xffffffffu, best_tmb = 0u;
  ICAMD_NOUNROLL
  for (int t = 0; t < 16; ++t) {  // wave-uniform: the table's constants are scalars
    const uint32_t mags = eac_mags((uint32_t)t), span = 2u * (mags >> 24) - 1u, recip = eac_recip_of((uint32_t)t);
    const int32_t m0 = imed3((int32_t)(umad24(range2 + span, recip, 0u) >> 16), 1, 15);
    ICAMD_NOUNROLL
    for (int dm = -1; dm <= 1; ++dm) {
      const int32_t m = imed3(m0 + dm, 1, 15);
      const int32_t b0 = (int32_t)((mid2 + (uint32_t)m) >> 1);
      ICAMD_UNROLL
      for (int db = -1; db <= 1; ++db) {
        const int32_t b = imed3(b0 + db, 0, 255);
        int32_t v[8];
        eac_values(mags, m, b, v);
        const uint32_t sse = eac_sse_palette(pal, count, v);
        const bool better = sse < best_sse;
        best_tmb = better ? ((uint32_t)t << 12 | (uint32_t)m << 8 | (uint32_t)b) : best_tmb;
        best_sse = better ? sse : best_sse;
      }
      if (wave_all(best_sse == 0u)) return best_tmb;  // nothing later is strictly smaller than 0 in any lane
    }
  }
  return best_tmb;
}

// eac_pack (etc2_block.h) through the palette: the EAC index of each palette entry once (smallest index on ties), then the
// texels' indices by their DXT5 codes.  A pixel row's four codes select four bytes of the index table in one v_perm (byte x =
// index of texel (x, y)); EAC keeps texel 4 x + y at bits 47 - 3 (4 x + y), so column x is the 12-bit group
// idx(x, 0) << 9 | idx(x, 1) << 6 | idx(x, 2) << 3 | idx(x, 3) at bit 36 - 12 x: even and odd columns are gathered in the 16-bit
// halves of two dwords.
ICAMD_DEV Out8 eac_pack_palette(const uint32_t pal[8], uint32_t lo24, uint32_t hi24, uint32_t t, uint32_t m, uint32_t b) {
  int32_t v[8];
  eac_values(eac_mags(t & 15u), (int32_t)m, (int32_t)b, v);  // (t differs per lane here: per-lane shifts, once per block)
  uint32_t table[2] = { 0u, 0u };  // byte j & 3 of table[j >> 2] = index of palette entry j
  ICAMD_UNROLL
  for (int j = 0; j < 8; ++j) {
    uint32_t best = sad_u32(pal[j], (uint32_t)v[0], 0u), idx = 0u;
    ICAMD_UNROLL
    for (int k = 1; k < 8; ++k) {
      const uint32_t e = sad_u32(pal[j], (uint32_t)v[k], 0u);
      const bool better = e < best;  // strictly: ties keep the smaller index
      idx = better ? (uint32_t)k : idx;
      best = better ? e : best;
    }
    table[j >> 2] |= idx << (8 * (j & 3));
  }
  uint32_t even = 0u, odd = 0u;  // columns (0, 2) and (1, 3) in the 16-bit halves
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    const uint32_t row = perm(table[1], table[0], dxt5_row_alpha_selector(lo24, hi24, y));
    even = even << 3 | perm(0u, row, 0x0c020c00u);
    odd = odd << 3 | perm(0u, row, 0x0c030c01u);
  }
  const uint32_t g0 = even & 0xfffu, g1 = odd & 0xfffu, g2 = even >> 16, g3 = odd >> 16;
  const uint32_t hi = b << 24 | m << 20 | t << 16 | g0 << 4 | g1 >> 8, lo = g1 << 24 | g2 << 12 | g3;
  const Out8 o = { perm(0u, hi, 0x00010203u), perm(0u, lo, 0x00010203u) };  // big-endian words in memory
  return o;
}

// w0, w1: a DXT5 alpha word (a0, a1, sixteen 3-bit codes) -> the EAC word encode_eac_alpha writes for the alphas it decodes to
// (decode_dxt5_alpha: the truncating sevenths / fifths, 0 and 255 in the six-value mode).
ICAMD_DEV Out8 transcode_dxt5_alpha_to_eac(uint32_t w0, uint32_t w1) {
  uint32_t tlo, thi;
  dxt5_alpha_planes(w0, tlo, thi);
  const uint32_t lo24 = w0 >> 16 | (w1 & 0xffu) << 16, hi24 = w1 >> 8;
  uint32_t pal[8], count[8];
  ICAMD_UNROLL
  for (int j = 0; j < 8; ++j) pal[j] = bfe(j < 4 ? tlo : thi, 8u * (uint32_t)(j & 3), 8u);
  dxt5_code_counts(lo24, hi24, count);
  const uint32_t tmb = eac_search_palette(pal, count);
  return eac_pack_palette(pal, lo24, hi24, tmb >> 12, (tmb >> 8) & 15u, tmb & 255u);
}

// A whole block: w[0..1] the alpha word, w[2..3] the colour word, in and out.  Colour first: its registers are dead before the
// alpha search, which is most of the work, starts (as in etc2_kernels.hip).
ICAMD_DEV void transcode_dxt5_block_to_etc2_rgba8(const uint32_t w[4], uint32_t out[4]) {
  const Out8 c = transcode_dxt1_block_to_etc1<true>(w[2], w[3]);
  const Out8 e = transcode_dxt5_alpha_to_eac(w[0], w[1]);
  out[0] = e.lo; out[1] = e.hi; out[2] = c.lo; out[3] = c.hi;
}

}  // namespace icamd
#endif  // ICAMD_TRANSCODE5_BLOCK_H_
