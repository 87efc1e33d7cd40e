// etc2_colour_block.h -- the complete ETC2 RGB colour word (EXTENSION, include/ic_amd.h ICAMD_ETC2_RGB8), one
// block per lane: the five-mode decoder that ICAMD_ETC2_RGB8 and ICAMD_ETC2_RGBA8 share, and the planar half of the
// ICAMD_ETC2_RGB8 encoder.  Integers only, no memory tables.
//
// The word is 64 bits, big-endian (bit 63 = top bit of byte 0); `hi` below is bits 63..32, `lo` bits 31..0.
// Mode (Khronos ETC2): diff = bit 33.  diff = 0: individual, as ETC1.  Otherwise s_c = 5-bit base + sign-extended 3-bit delta of
// byte c; s_R outside 0..31: T; else s_G outside: H; else s_B outside: planar; else differential, as ETC1.  The two
// ETC1-compatible modes go through decode_etc1 itself, so those bytes are the ETC1 decoder's.
//   T:      R1 = bits 60-59 : 57-56, G1 = 55-52, B1 = 51-48, R2 = 47-44, G2 = 43-40, B2 = 39-36, di = 35-34 : 32;
//           paint = C1, clamp(C2 + d[di]), C2, clamp(C2 - d[di])                      (C: 4 bits expanded, v * 17)
//   H:      R1 = 62-59, G1 = 58-56 : 52, B1 = 51 : 49-47, R2 = 46-43, G2 = 42-39, B2 = 38-35,
//           di = bit 34 << 2 | bit 32 << 1 | (C1 >= C2 as R << 16 | G << 8 | B);  paint = clamp(C1 +- d[di]), clamp(C2 +- d[di])
//   planar: RO = 62-57, GO = 56 : 54-49, BO = 48 : 44-43 : 41-39, RH = 38-34 : 32, GH = 31-25, BH = 24-19, RV = 18-13,
//           GV = 12-6, BV = 5-0 (6 / 7 / 6 bits, expanded v << 2 | v >> 4 and v << 1 | v >> 6);
//           texel (x, y) = clamp((x (H - O) + y (V - O) + 4 O + 2) >> 2, 0, 255), the shift arithmetic.
// d[0..7] = 3, 6, 11, 16, 23, 32, 41, 64.  In T and H texel (x, y) takes paint k = bit(p) | bit(p + 16) << 1 of `lo`,
// p = 4 x + y: the two bit planes decode_etc1 reads.
//
// The planar candidate of the encoder is a DEFINITION (the least-squares plane, no search): per channel, with v(x, y) the
// sixteen texels, S = Sum v, Sx = Sum (2 x - 3) v, Sy = Sum (2 y - 3) v; the plane's values at (0, 0), (4, 0), (0, 4) times 80
// are N_O = 5 S - 3 Sx - 3 Sy, N_H = 5 S + 5 Sx - 3 Sy, N_V = 5 S - 3 Sx + 5 Sy (Sum (x - 1.5)^2 = 20 over the block); the
// n-bit code is q = (2 clamp(N, 0, 20400) (2^n - 1) + 20400) / 40800, truncating.  The block is the planar word if its summed
// squared error over the 16 texels and 3 channels is STRICTLY smaller than that of the ETC1 word, else the ETC1 word.
#ifndef ICAMD_ETC2_COLOUR_BLOCK_H_
#define ICAMD_ETC2_COLOUR_BLOCK_H_

#include "decode_block.h"  // decode_etc1, clamp255
#include "dxt_block.h"     // Out8
#include "ic_device.h"

namespace icamd {

// 0: an ETC1-compatible mode (individual, or differential without overflow), 1: T, 2: H, 3: planar
ICAMD_DEV uint32_t etc2_colour_mode(uint32_t hi) {
  if (!(hi & 2u)) return 0u;
  uint32_t mode = 0u;
  ICAMD_UNROLL
  for (int ch = 2; ch >= 0; --ch) {  // (R decides before G before B: the last assignment wins)
    const int32_t b5 = (int32_t)((hi >> (27 - 8 * ch)) & 31u), d3 = (int32_t)((hi >> (24 - 8 * ch)) & 7u);
    const int32_t s = b5 + ((d3 ^ 4) - 4);
    mode = (uint32_t)s > 31u ? (uint32_t)ch + 1u : mode;
  }
  return mode;
}

// the three channels (each any int32) clamped to bytes: R | G << 8 | B << 16
ICAMD_DEV uint32_t etc2_pack_clamped(int32_t r, int32_t g, int32_t b) { return clamp255(r) | clamp255(g) << 8 | clamp255(b) << 16; }

// T and H: the four paint colours of the upper half word
ICAMD_DEV void etc2_th_paints(uint32_t hi, bool h_mode, uint32_t paint[4]) {
  int32_t c1[3], c2[3];
  uint32_t di;
  if (h_mode) {
    c1[0] = (int32_t)((hi >> 27) & 15u);
    c1[1] = (int32_t)(((hi >> 24) & 7u) << 1 | ((hi >> 20) & 1u));
    c1[2] = (int32_t)(((hi >> 19) & 1u) << 3 | ((hi >> 15) & 7u));
    c2[0] = (int32_t)((hi >> 11) & 15u);
    c2[1] = (int32_t)((hi >> 7) & 15u);
    c2[2] = (int32_t)((hi >> 3) & 15u);
    di = ((hi >> 2) & 1u) << 2 | (hi & 1u) << 1;
  } else {
    c1[0] = (int32_t)(((hi >> 27) & 3u) << 2 | ((hi >> 24) & 3u));
    c1[1] = (int32_t)((hi >> 20) & 15u);
    c1[2] = (int32_t)((hi >> 16) & 15u);
    c2[0] = (int32_t)((hi >> 12) & 15u);
    c2[1] = (int32_t)((hi >> 8) & 15u);
    c2[2] = (int32_t)((hi >> 4) & 15u);
    di = ((hi >> 2) & 3u) << 1 | (hi & 1u);
  }
  ICAMD_UNROLL
  for (int ch = 0; ch < 3; ++ch) {
    c1[ch] *= 17;
    c2[ch] *= 17;
  }
  if (h_mode) di |= (c1[0] << 16 | c1[1] << 8 | c1[2]) >= (c2[0] << 16 | c2[1] << 8 | c2[2]) ? 1u : 0u;
  const int32_t d = (int32_t)bfe(di < 4u ? (3u | 6u << 8 | 11u << 16 | 16u << 24) : (23u | 32u << 8 | 41u << 16 | 64u << 24),
                                 8u * (di & 3u), 8u);
  const int32_t d1 = h_mode ? d : 0;  // T leaves C1 as it is
  paint[0] = etc2_pack_clamped(c1[0] + d1, c1[1] + d1, c1[2] + d1);
  paint[1] = h_mode ? etc2_pack_clamped(c1[0] - d, c1[1] - d, c1[2] - d) : etc2_pack_clamped(c2[0] + d, c2[1] + d, c2[2] + d);
  paint[2] = h_mode ? etc2_pack_clamped(c2[0] + d, c2[1] + d, c2[2] + d) : etc2_pack_clamped(c2[0], c2[1], c2[2]);
  paint[3] = etc2_pack_clamped(c2[0] - d, c2[1] - d, c2[2] - d);
}

ICAMD_DEV int32_t etc2_expand6(uint32_t v) { return (int32_t)(v << 2 | v >> 4); }
ICAMD_DEV int32_t etc2_expand7(uint32_t v) { return (int32_t)(v << 1 | v >> 6); }

// The sixteen texels of a plane: code[0..2] = RO GO BO, code[3..5] = RH GH BH, code[6..8] = RV GV BV (6 / 7 / 6 bits).
// px[4 y + x] = R | G << 8 | B << 16.
ICAMD_DEV void etc2_planar_texels(const uint32_t code[9], uint32_t px[16]) {
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) px[p] = 0u;
  ICAMD_UNROLL
  for (int ch = 0; ch < 3; ++ch) {
    const int32_t o = ch == 1 ? etc2_expand7(code[ch]) : etc2_expand6(code[ch]);
    const int32_t h = ch == 1 ? etc2_expand7(code[3 + ch]) : etc2_expand6(code[3 + ch]);
    const int32_t v = ch == 1 ? etc2_expand7(code[6 + ch]) : etc2_expand6(code[6 + ch]);
    const int32_t dx = h - o, dy = v - o;
    int32_t row = 4 * o + 2;
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      int32_t t = row;
      ICAMD_UNROLL
      for (int x = 0; x < 4; ++x) {
        px[4 * y + x] |= clamp255(t >> 2) << (8 * ch);
        t += dx;
      }
      row += dy;
    }
  }
}

// The nine codes of a planar word
ICAMD_DEV void etc2_planar_codes(uint32_t hi, uint32_t lo, uint32_t code[9]) {
  code[0] = (hi >> 25) & 63u;
  code[1] = ((hi >> 24) & 1u) << 6 | ((hi >> 17) & 63u);
  code[2] = ((hi >> 16) & 1u) << 5 | ((hi >> 11) & 3u) << 3 | ((hi >> 7) & 7u);
  code[3] = ((hi >> 2) & 31u) << 1 | (hi & 1u);
  code[4] = lo >> 25;
  code[5] = (lo >> 19) & 63u;
  code[6] = (lo >> 13) & 63u;
  code[7] = (lo >> 6) & 127u;
  code[8] = lo & 63u;
}

// Any 8-byte ETC2 RGB colour word (w0, w1: its bytes as little-endian dwords, as decode_etc1 takes them) to sixteen texels,
// px[4 y + x] = R | G << 8 | B << 16.  The mode test is a handful of instructions in front of decode_etc1, and a wave whose
// blocks are all ETC1-compatible -- everything the ETC1 and ETC2 RGBA8 encoders write -- executes nothing else.
ICAMD_DEV void decode_etc2_colour(uint32_t w0, uint32_t w1, uint32_t px[16]) {
  const uint32_t hi = perm(0u, w0, 0x00010203u);
  const uint32_t mode = etc2_colour_mode(hi);
  if (mode == 0u) {
    decode_etc1(w0, w1, px);
    return;
  }
  const uint32_t lo = perm(0u, w1, 0x00010203u);
  if (mode == 3u) {
    uint32_t code[9];
    etc2_planar_codes(hi, lo, code);
    etc2_planar_texels(code, px);
    return;
  }
  uint32_t paint[4];
  etc2_th_paints(hi, mode == 2u, paint);
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    ICAMD_UNROLL
    for (int x = 0; x < 4; ++x) {
      const int p = 4 * x + y;
      const uint32_t k = ((lo >> p) & 1u) | ((lo >> (p + 16)) & 1u) << 1;
      px[4 * y + x] = k == 0u ? paint[0] : k == 1u ? paint[1] : k == 2u ? paint[2] : paint[3];
    }
  }
}

// ---- the planar candidate of the ICAMD_ETC2_RGB8 encoder

// q = (2 c maxcode + 20400) / 40800 for c in 0..20400, maxcode 63 or 127: 40800 = 32 * 1275, the numerator is below 2^23, and
// (n >> 5) / 1275 is one high multiply -- checked for every reachable argument below.
constexpr uint32_t kEtc2Recip1275 = (uint32_t)(((1ull << 32) + 1274u) / 1275u);
constexpr uint32_t etc2_planar_quantise(uint32_t c, uint32_t maxcode) {
  return (uint32_t)(((uint64_t)((2u * c * maxcode + 20400u) >> 5) * kEtc2Recip1275) >> 32);
}
namespace detail {
constexpr bool check_planar_quantise(uint32_t maxcode) {
  for (uint32_t c = 0; c <= 20400u; ++c)
    if (etc2_planar_quantise(c, maxcode) != (2u * c * maxcode + 20400u) / 40800u) return false;
  return true;
}
static_assert(check_planar_quantise(63u), "planar 6-bit code");
static_assert(check_planar_quantise(127u), "planar 7-bit code");
}  // namespace detail
ICAMD_DEV uint32_t etc2_planar_code(int32_t n, uint32_t maxcode) {
  const uint32_t c = (uint32_t)imin(imax(n, 0), 20400);
  return umulhi32(umad24(2u * c, maxcode, 20400u) >> 5, kEtc2Recip1275);
}

// The least-squares plane of the sixteen texels px[4 y + x] (bytes 0..2; byte 3 is ignored) as the nine codes.
ICAMD_DEV void etc2_planar_fit(const uint32_t px[16], uint32_t code[9]) {
  ICAMD_UNROLL
  for (int ch = 0; ch < 3; ++ch) {
    int32_t s = 0, sxv = 0, sy = 0;
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      // the row's four values of the channel as the bytes of a dword, byte x = texel (x, y)
      const uint32_t r = perm(px[4 * y + 1], px[4 * y], 0x0c0c0400u + 0x0101u * (uint32_t)ch) |
                         perm(px[4 * y + 3], px[4 * y + 2], 0x04000c0cu + 0x01010000u * (uint32_t)ch);
      const int32_t rs = (int32_t)udot4(r, 0x01010101u, 0u);
      s += rs;
      sxv += (int32_t)udot4(r, 0x03020100u, 0u);  // Sum x v
      sy += (2 * y - 3) * rs;
    }
    const int32_t sx = 2 * sxv - 3 * s;
    const uint32_t maxcode = ch == 1 ? 127u : 63u;
    code[ch] = etc2_planar_code(5 * s - 3 * sx - 3 * sy, maxcode);
    code[3 + ch] = etc2_planar_code(5 * s + 5 * sx - 3 * sy, maxcode);
    code[6 + ch] = etc2_planar_code(5 * s - 3 * sx + 5 * sy, maxcode);
  }
}

// The planar word of nine codes.  The bits the mode ignores (63, 55, 47-45, 42) are set so that byte 0 and byte 1 do not
// overflow and byte 2 does: bit 63 / 55 = the top bit of the byte's 3-bit delta field (a negative delta gets a base of at
// least 16, a positive one a base below 16); byte 2 with b = BO bits 4-3 and t = BO bits 2-1 is base 28 + b, delta + t
// where b + t >= 4 (>= 32) and base b, delta t - 4 otherwise (< 0).
ICAMD_DEV Out8 etc2_planar_pack(const uint32_t code[9]) {
  const uint32_t ro = code[0], go = code[1], bo = code[2], rh = code[3];
  uint32_t hi = ro << 25 | (go >> 6) << 24 | (go & 63u) << 17 | (bo >> 5) << 16 | ((bo >> 3) & 3u) << 11 | (bo & 7u) << 7 |
                (rh >> 1) << 2 | 2u | (rh & 1u);
  hi |= ((ro >> 1) & 1u) << 31 | ((go >> 1) & 1u) << 23;
  hi |= ((bo >> 3) & 3u) + ((bo >> 1) & 3u) >= 4u ? 7u << 13 : 1u << 10;
  const uint32_t lo = code[4] << 25 | code[5] << 19 | code[6] << 13 | code[7] << 6 | code[8];
  const Out8 o = { perm(0u, hi, 0x00010203u), perm(0u, lo, 0x00010203u) };  // big-endian words in memory
  return o;
}

// Sum over the sixteen texels and three channels of (d - s)^2 = Sum s^2 + Sum d^2 - 2 Sum s d on the texels' bytes; byte 3 of
// every s and d is 0.  ss = Sum s^2.  At most 48 * 255^2 < 2^22.
ICAMD_DEV uint32_t etc2_sum_squares(const uint32_t s[16]) {
  uint32_t ss = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) ss = udot4(s[p], s[p], ss);
  return ss;
}
ICAMD_DEV uint32_t etc2_sse_rgb(const uint32_t s[16], uint32_t ss, const uint32_t d[16]) {
  uint32_t dd = ss, sd = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    dd = udot4(d[p], d[p], dd);
    sd = udot4(s[p], d[p], sd);
  }
  return dd - 2u * sd;
}

// The ICAMD_ETC2_RGB8 block of the sixteen texels px (as the ETC1 block routine was handed them; byte 3 is ignored) whose
// ETC1 word is e: the planar word where it is strictly closer, else e byte for byte.
ICAMD_DEV Out8 etc2_rgb8_choose(const uint32_t px[16], Out8 e) {
  uint32_t s[16], d[16], code[9];
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) s[p] = px[p] & 0x00ffffffu;
  const uint32_t ss = etc2_sum_squares(s);
  decode_etc1(e.lo, e.hi, d);
  const uint32_t sse_e = etc2_sse_rgb(s, ss, d);
  etc2_planar_fit(s, code);
  etc2_planar_texels(code, d);
  const uint32_t sse_p = etc2_sse_rgb(s, ss, d);
  const Out8 pl = etc2_planar_pack(code);
  const bool planar = sse_p < sse_e;
  const Out8 o = { planar ? pl.lo : e.lo, planar ? pl.hi : e.hi };
  return o;
}

}  // namespace icamd
#endif  // ICAMD_ETC2_COLOUR_BLOCK_H_
