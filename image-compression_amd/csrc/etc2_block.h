// etc2_block.h -- the EAC alpha half of ETC2 RGBA8 (EXTENSION, include/ic_amd.h ICAMD_ETC2_RGBA8), one block per lane.
//
// An ETC2 RGBA8 block is 16 bytes: the 8-byte EAC alpha word, then the 8-byte colour word.  The colour word is what the ETC1
// encoder of etc1_block.h writes (every ETC1 block is a valid ETC2 colour word: etc1_partition_bases never produces the
// overflowing differential bases that select ETC2's T, H and planar modes).  Only the alpha word is defined here.
//
// EAC word, big-endian: byte 0 = base, byte 1 = multiplier << 4 | table, bytes 2..7 = sixteen 3-bit indices, texel
// i = 4 x + y (column-major, like ETC1's pixel indices) in bits 47 - 3 i ... 45 - 3 i.
// Decode (Khronos ETC2 / EAC, 8-bit alpha): alpha = clamp(base + M[table][index] * multiplier, 0, 255); a multiplier of 0
// gives `base`.  M[t][k] = -mag[t][k] for k < 4 and mag[t][k - 4] - 1 for k >= 4: the table below holds the four magnitudes.
//
// Encode is a DEFINITION, the same 144 candidates for every block:
//   lo, hi = min / max of the sixteen alphas, R = hi - lo, span[t] = M[t][7] - M[t][3] = 2 mag[t][3] - 1;
//   for t in 0..15:  m0 = clamp((2 R + span) / (2 span), 1, 15);
//     for m in clamp(m0 - 1 .. m0 + 1, 1, 15):  b0 = (lo + hi + m + 1) >> 1;
//       for b in clamp(b0 - 1 .. b0 + 1, 0, 255):
//         sse = Sum over the texels of min_k (clamp(b + M[t][k] m, 0, 255) - a)^2;
//   the block is the candidate with the lexicographically smallest (sse, t, m, b); every texel takes the smallest index k
//   that reaches its minimum.
// The loops below visit the candidates in ascending (t, m, b) (clamping keeps m and b non-decreasing) and replace the best
// on a strictly smaller sse only, which is that order.  The one candidate skip: once EVERY lane of the wave holds sse = 0
// nothing later can be strictly smaller, so the wave leaves the search (opaque and flat content: the first candidate).
// Integers only; the table loop is wave-uniform, so its modifiers live in scalar registers.
#ifndef ICAMD_ETC2_BLOCK_H_
#define ICAMD_ETC2_BLOCK_H_

#include "decode_block.h"  // decode_etc1
#include "dxt_block.h"     // Out8
#include "etc2_colour_block.h"  // decode_etc2_colour
#include "ic_device.h"

namespace icamd {

// mag[t][0..3] as the four bytes of a dword (low byte = mag[t][0])
#define ICAMD_EAC_MAG(a, b, c, d) ((uint32_t)(a) | (uint32_t)(b) << 8 | (uint32_t)(c) << 16 | (uint32_t)(d) << 24)
constexpr uint32_t kEacMag[16] = {
  ICAMD_EAC_MAG(3, 6, 9, 15), ICAMD_EAC_MAG(3, 7, 10, 13), ICAMD_EAC_MAG(2, 5, 8, 13), ICAMD_EAC_MAG(2, 4, 6, 13),
  ICAMD_EAC_MAG(3, 6, 8, 12), ICAMD_EAC_MAG(3, 7, 9, 11),  ICAMD_EAC_MAG(4, 7, 8, 11), ICAMD_EAC_MAG(3, 5, 8, 11),
  ICAMD_EAC_MAG(2, 6, 8, 10), ICAMD_EAC_MAG(2, 5, 8, 10),  ICAMD_EAC_MAG(2, 4, 8, 10), ICAMD_EAC_MAG(2, 5, 7, 10),
  ICAMD_EAC_MAG(3, 4, 7, 10), ICAMD_EAC_MAG(1, 2, 3, 10),  ICAMD_EAC_MAG(4, 6, 8, 9),  ICAMD_EAC_MAG(3, 5, 7, 9) };
#undef ICAMD_EAC_MAG

// The same tables as immediates for device code: the sixteen tables' k-th magnitudes as the nibbles of one 64-bit constant, and
// the 16-bit reciprocals of 2 span[t] (n / (2 span[t]) for n = 2 R + span[t] <= 510 + 29, checked exhaustively below) four to
// a constant.  A table number that is wave-uniform (the search's loop) makes these scalar shifts; no memory is read.
constexpr uint32_t eac_span(int t) { return 2u * (kEacMag[t] >> 24) - 1u; }
constexpr uint32_t eac_recip(int t) { return (65536u + 2u * eac_span(t) - 1u) / (2u * eac_span(t)); }
constexpr uint64_t eac_nibbles(int k) {
  uint64_t c = 0;
  for (int t = 0; t < 16; ++t) c |= (uint64_t)((kEacMag[t] >> (8 * k)) & 15u) << (4 * t);
  return c;
}
constexpr uint64_t eac_recips(int q) {
  uint64_t c = 0;
  for (int i = 0; i < 4; ++i) c |= (uint64_t)eac_recip(4 * q + i) << (16 * i);
  return c;
}
namespace detail {
constexpr bool check_eac_recip() {
  for (int t = 0; t < 16; ++t)
    for (uint32_t n = 0; n <= 510u + eac_span(t); ++n)
      if (((n * eac_recip(t)) >> 16) != n / (2u * eac_span(t))) return false;
  return true;
}
static_assert(check_eac_recip(), "EAC reciprocal");
}  // namespace detail

// mag[t][0..3] as the four bytes of a dword, t in 0..15
ICAMD_DEV uint32_t eac_mags(uint32_t t) {
  constexpr uint64_t c0 = eac_nibbles(0), c1 = eac_nibbles(1), c2 = eac_nibbles(2), c3 = eac_nibbles(3);
  const uint32_t s = 4u * t;
  return ((uint32_t)(c0 >> s) & 15u) | ((uint32_t)(c1 >> s) & 15u) << 8 | ((uint32_t)(c2 >> s) & 15u) << 16 |
         ((uint32_t)(c3 >> s) & 15u) << 24;
}
ICAMD_DEV uint32_t eac_recip_of(uint32_t t) {
  constexpr uint64_t r0 = eac_recips(0), r1 = eac_recips(1), r2 = eac_recips(2), r3 = eac_recips(3);
  const uint32_t q = t >> 2;
  const uint64_t r = q == 0u ? r0 : q == 1u ? r1 : q == 2u ? r2 : r3;
  return (uint32_t)(r >> (16u * (t & 3u))) & 0xffffu;
}

ICAMD_DEV int32_t imed3(int32_t v, int32_t lo, int32_t hi) { return imin(imax(v, lo), hi); }  // v_med3_i32

// The eight values a (table, multiplier, base) decodes to, in index order.
ICAMD_DEV void eac_values(uint32_t mags, int32_t m, int32_t b, int32_t v[8]) {
  ICAMD_UNROLL
  for (int k = 0; k < 4; ++k) {
    const int32_t g = (int32_t)bfe(mags, 8 * k, 8);
    v[k] = imed3(imad24(-g, m, b), 0, 255);
    v[k + 4] = imed3(imad24(g - 1, m, b), 0, 255);
  }
}

// Sum over the sixteen texels of the squared distance to the nearest of the eight values (at most 16 * 255^2 < 2^21).
ICAMD_DEV uint32_t eac_sse(const uint32_t a[16], const int32_t v[8]) {
  uint32_t sse = 0;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    uint32_t e = umin3(sad_u32(a[p], (uint32_t)v[0], 0u), sad_u32(a[p], (uint32_t)v[1], 0u), sad_u32(a[p], (uint32_t)v[2], 0u));
    e = umin3(e, sad_u32(a[p], (uint32_t)v[3], 0u), sad_u32(a[p], (uint32_t)v[4], 0u));
    e = umin3(e, sad_u32(a[p], (uint32_t)v[5], 0u), sad_u32(a[p], (uint32_t)v[6], 0u));
    e = umin(e, sad_u32(a[p], (uint32_t)v[7], 0u));
    sse = umad24(e, e, sse);
  }
  return sse;
}

// a[4 y + x] = the value of texel (x, y).  The word whose header bits (base, multiplier, table: bits 63..48) are `hi` and whose candidate values, in index order, are v:
// every texel takes the smallest index that reaches its minimum.  a and v below 65536 (sad_u32).
ICAMD_DEV Out8 eac_pack_values(const uint32_t a[16], const int32_t v[8], uint32_t hi) {
  uint32_t lo = 0u;  // the 64-bit big-endian word as (hi, lo)
  ICAMD_UNROLL
  for (int x = 0; x < 4; ++x) {
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      const uint32_t p = a[4 * y + x];
      uint32_t best = sad_u32(p, (uint32_t)v[0], 0u), idx = 0u;
      ICAMD_UNROLL
      for (int k = 1; k < 8; ++k) {
        const uint32_t e = sad_u32(p, (uint32_t)v[k], 0u);
        const bool better = e < best;  // strictly: ties keep the smaller index
        idx = better ? (uint32_t)k : idx;
        best = better ? e : best;
      }
      const int s = 45 - 3 * (4 * x + y);  // the index field's lowest bit in the 64-bit word
      if (s >= 32) hi |= idx << (s - 32);
      else if (s <= 29) lo |= idx << s;
      else { lo |= idx << s; hi |= idx >> (32 - s); }
    }
  }
  const Out8 o = { perm(0u, hi, 0x00010203u), perm(0u, lo, 0x00010203u) };  // big-endian words in memory
  return o;
}
// The EAC word of the chosen (table t, multiplier m, base b): a[4 y + x] = alpha of texel (x, y).
ICAMD_DEV Out8 eac_pack(const uint32_t a[16], uint32_t t, uint32_t m, uint32_t b) {
  int32_t v[8];
  eac_values(eac_mags(t & 15u), (int32_t)m, (int32_t)b, v);  // (t differs per lane here: per-lane shifts, once per block)
  return eac_pack_values(a, v, b << 24 | m << 20 | t << 16);
}

// The 3-bit index of texel i = 4 x + y (a constant at every call site) in the 64-bit big-endian word (hi, lo).
ICAMD_DEV uint32_t eac_index(uint32_t hi, uint32_t lo, int i) {
  const int s = 45 - 3 * i;  // the index field's lowest bit in the 64-bit word
  return (s >= 32 ? hi >> (s - 32) : s <= 29 ? lo >> s : alignbit(hi, lo, (uint32_t)s)) & 7u;
}

// The alpha search.  a[4 y + x] = alpha of texel (x, y), each 0..255.
ICAMD_DEV Out8 encode_eac_alpha(const uint32_t a[16]) {
  uint32_t lo = a[0], hi = a[0];
  ICAMD_UNROLL
  for (int p = 1; p < 16; p += 3) {
    lo = umin3(lo, a[p], a[p + 1]);
    hi = umax3(hi, a[p], a[p + 1]);
    lo = umin(lo, a[p + 2]);
    hi = umax(hi, a[p + 2]);
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
        const uint32_t sse = eac_sse(a, v);
        const bool better = sse < best_sse;
        best_tmb = better ? ((uint32_t)t << 12 | (uint32_t)m << 8 | (uint32_t)b) : best_tmb;
        best_sse = better ? sse : best_sse;
      }
      if (wave_all(best_sse == 0u)) return eac_pack(a, best_tmb >> 12, (best_tmb >> 8) & 15u, best_tmb & 255u);
    }
  }
  return eac_pack(a, best_tmb >> 12, (best_tmb >> 8) & 15u, best_tmb & 255u);
}

// w0, w1: the 8 bytes of an EAC word as little-endian dwords.  Writes the alpha of texel (x, y) into byte 3 of px[4 y + x].
ICAMD_DEV void decode_eac_alpha(uint32_t w0, uint32_t w1, uint32_t px[16]) {
  const uint32_t hi = perm(0u, w0, 0x00010203u), lo = perm(0u, w1, 0x00010203u);
  const int32_t b = (int32_t)(hi >> 24), m = (int32_t)((hi >> 20) & 15u);
  int32_t v[8];
  eac_values(eac_mags((hi >> 16) & 15u), m, b, v);
  ICAMD_UNROLL
  for (int x = 0; x < 4; ++x) {
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      const uint32_t idx = eac_index(hi, lo, 4 * x + y);
      uint32_t al = (uint32_t)v[0];
      ICAMD_UNROLL
      for (int k = 1; k < 8; ++k) al = idx == (uint32_t)k ? (uint32_t)v[k] : al;
      px[4 * y + x] = (px[4 * y + x] & 0x00ffffffu) | al << 24;
    }
  }
}

// A whole ETC2 RGBA8 block (w[0..1] the EAC word, w[2..3] the colour word in any of the five modes: etc2_colour_block.h) as
// R,G,B,A dwords.  swap: stored R goes to the third byte, as the DXT5 decoder's swap does.
ICAMD_DEV void decode_etc2_rgba8(const uint32_t w[4], bool swap, uint32_t px[16]) {
  decode_etc2_colour(w[2], w[3], px);
  decode_eac_alpha(w[0], w[1], px);
  if (swap) {
    ICAMD_UNROLL
    for (int p = 0; p < 16; ++p) px[p] = perm(px[p], px[p], 0x03000102u);
  }
}

}  // namespace icamd
#endif  // ICAMD_ETC2_BLOCK_H_
