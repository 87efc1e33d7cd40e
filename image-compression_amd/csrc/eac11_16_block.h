// eac11_16_block.h -- 16-bit and signed EAC R11 / RG11 (EXTENSION, include/ic_amd.h ICAMD_EAC_SIGNED_R11 and
// icamd_encode_eac11_16_device), one block per lane: the fetch of 16-bit samples, the search in the 11-bit
// domain, the 16-bit decoder and the 16-bit metric.
//
// The word is the EAC word of etc2_block.h; for the signed codecs byte 0 is a two's-complement base.  The search is a
// DEFINITION stated in full in include/ic_amd.h and restated in numpy in tests/eac11_16_oracle.py; in short:
//   target a = u16 >> 5 (unsigned), sign(x) (|x| >> 5) with x = max(s16, -32767) (signed); lo, hi, R = hi - lo;
//   for t in 0..15:  m0 = (2 R + 8 span[t]) / (16 span[t]);
//     for m in (0, clamp(m0 - 1, 1, 15), clamp(m0, 1, 15), clamp(m0 + 1, 1, 15)):  s = m == 0 ? 1 : 8 m, c2 = lo + hi + s,
//         b0 = c2 >> 4 (unsigned), (c2 + 8) >> 4 (signed, floor);
//       for b in clamp(b0 - 1 .. b0 + 1):  sse of the texels' nearest v_k = clamp(B + M[t][k] s, Vmin, Vmax);
//   the first candidate of the smallest sse wins, every texel takes the smallest index at its minimum.
// Both signednesses run ONE body: the signed targets and values are held with 1023 added, which makes them 0 .. 2046 where the
// unsigned ones are 0 .. 2047, so the distance (eac_sse) and the index choice (eac_pack_values) of etc2_block.h serve both; only
// the constants of Eac16 differ.  Shared with the 8-bit codecs: the magnitude table (eac_mags), the reciprocals of 2 span
// (eac_recip_of), eac_sse, eac_pack_values and the index extraction (eac_index).  The candidate loop is this format's own.
#ifndef ICAMD_EAC11_16_BLOCK_H_
#define ICAMD_EAC11_16_BLOCK_H_

#include "etc2_block.h"

namespace icamd {

template <bool SIGNED>
struct Eac16 {
  static constexpr int32_t kBias = SIGNED ? 1023 : 0;      // what targets and values are held above their true value
  static constexpr int32_t kVmax = SIGNED ? 2046 : 2047;   // Vmax + kBias (Vmin + kBias is 0)
  static constexpr int32_t kBase0 = SIGNED ? 1023 : 4;     // B + kBias = 8 b + kBase0
  static constexpr int32_t kBmin = SIGNED ? -127 : 0, kBmax = SIGNED ? 127 : 255;
};

namespace detail {
// (2 R + 8 span) / (16 span) = ((2 R + 8 span) >> 3) / (2 span): the 16-bit reciprocal of 2 span that the 8-bit search uses, on
// this search's larger dividends (R <= 2047), checked exhaustively.
constexpr bool check_eac11_16_recip() {
  for (int t = 0; t < 16; ++t)
    for (uint32_t n = 0; n <= 4094u + 8u * eac_span(t); ++n)
      if ((((n >> 3) * eac_recip(t)) >> 16) != n / (16u * eac_span(t))) return false;
  return true;
}
static_assert(check_eac11_16_recip(), "EAC reciprocal on 11-bit ranges");
}  // namespace detail

// ---- source samples ----
// The block at pixel (row, col) of an image of C little-endian 16-bit samples per pixel: r[i] holds R (sample 0) of texels 2 i
// (low half) and 2 i + 1 (high half) in row-major order p = 4 y + x, g likewise G (sample 1, RG only).  Row loads of 8 C bytes
// at any 2-byte alignment where the block lies inside the image, else the clamp-to-edge gather (also for the blocks of a
// padded grid).  PRECONDITION h, w >= 1.
template <int C, bool RG>
ICAMD_DEV void eac11_16_fetch(const uint8_t *img, uint32_t h, uint32_t w, uint32_t stride, uint32_t row, uint32_t col,
                              uint32_t r[8], uint32_t g[8]) {
  if ((uint64_t)row + 4u <= h && (uint64_t)col + 4u <= w) {
    const uint8_t *p = img + (size_t)row * stride + (size_t)col * (2u * C);
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      const uint8_t *line = p + (size_t)y * stride;
      if (C == 1) {
        const U2 v = load_stream(reinterpret_cast<const U2 *>(line));
        r[2 * y] = v.x; r[2 * y + 1] = v.y;
      } else if (C == 2) {  // R0 G0 | R1 G1 | R2 G2 | R3 G3
        const U4 v = load_stream(reinterpret_cast<const U4 *>(line));
        r[2 * y] = perm(v.y, v.x, 0x05040100u); r[2 * y + 1] = perm(v.w, v.z, 0x05040100u);
        if (RG) { g[2 * y] = perm(v.y, v.x, 0x07060302u); g[2 * y + 1] = perm(v.w, v.z, 0x07060302u); }
      } else if (C == 3) {  // R0 G0 | B0 R1 | G1 B1 | R2 G2 | B2 R3 | G3 B3
        const U4 v = load_stream(reinterpret_cast<const U4 *>(line));
        const U2 u = load_stream(reinterpret_cast<const U2 *>(line + 16));
        r[2 * y] = perm(v.y, v.x, 0x07060100u); r[2 * y + 1] = perm(u.x, v.w, 0x07060100u);
        if (RG) { g[2 * y] = perm(v.z, v.x, 0x05040302u); g[2 * y + 1] = perm(u.y, v.w, 0x05040302u); }
      } else {  // R0 G0 | B0 A0 | R1 G1 | B1 A1 | ...
        const U4 v = load_stream(reinterpret_cast<const U4 *>(line)), u = load_stream(reinterpret_cast<const U4 *>(line + 16));
        r[2 * y] = perm(v.z, v.x, 0x05040100u); r[2 * y + 1] = perm(u.z, u.x, 0x05040100u);
        if (RG) { g[2 * y] = perm(v.z, v.x, 0x07060302u); g[2 * y + 1] = perm(u.z, u.x, 0x07060302u); }
      }
    }
  } else {
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      const uint8_t *line = img + (size_t)umin(row + (uint32_t)y, h - 1u) * stride;
      uint32_t rv[4], gv[4] = { 0u, 0u, 0u, 0u };
      ICAMD_UNROLL
      for (int x = 0; x < 4; ++x) {
        const uint8_t *q = line + (size_t)umin(col + (uint32_t)x, w - 1u) * (2u * C);
        rv[x] = (uint32_t)q[0] | (uint32_t)q[1] << 8;
        if (RG) gv[x] = (uint32_t)q[2] | (uint32_t)q[3] << 8;
      }
      r[2 * y] = rv[0] | rv[1] << 16; r[2 * y + 1] = rv[2] | rv[3] << 16;
      if (RG) { g[2 * y] = gv[0] | gv[1] << 16; g[2 * y + 1] = gv[2] | gv[3] << 16; }
    }
  }
}

// The 11-bit target of one stored sample (its 16 bits in v), plus Eac16::kBias: 0 .. Eac16::kVmax.
template <bool SIGNED>
ICAMD_DEV uint32_t eac11_16_target(uint32_t v) {
  if (!SIGNED) return v >> 5;
  const int32_t x = imax((int32_t)(v << 16) >> 16, -32767);
  const int32_t mag = (x < 0 ? -x : x) >> 5;
  return (uint32_t)((x < 0 ? -mag : mag) + 1023);
}

// The eight values of (table magnitudes, scale s, biased base bb = 8 b + kBase0), in index order, clamped to 0 .. vmax.
ICAMD_DEV void eac11_16_values(uint32_t mags, int32_t s, int32_t bb, int32_t vmax, int32_t v[8]) {
  ICAMD_UNROLL
  for (int k = 0; k < 4; ++k) {
    const int32_t g = (int32_t)bfe(mags, 8 * k, 8);
    v[k] = imed3(imad24(-g, s, bb), 0, vmax);
    v[k + 4] = imed3(imad24(g - 1, s, bb), 0, vmax);
  }
}

// ---- encode ----
// raw: the sixteen stored samples of one channel as eac11_16_fetch leaves them.  The word of the definition.
template <bool SIGNED>
ICAMD_DEV Out8 encode_eac11_16(const uint32_t raw[8]) {
  typedef Eac16<SIGNED> E;
  uint32_t a[16];  // a[4 y + x], biased
  ICAMD_UNROLL
  for (int i = 0; i < 8; ++i) {
    a[2 * i] = eac11_16_target<SIGNED>(raw[i] & 0xffffu);
    a[2 * i + 1] = eac11_16_target<SIGNED>(raw[i] >> 16);
  }
  uint32_t lo = a[0], hi = a[0];
  ICAMD_UNROLL
  for (int p = 1; p < 16; p += 3) {
    lo = umin3(lo, a[p], a[p + 1]);
    hi = umax3(hi, a[p], a[p + 1]);
    lo = umin(lo, a[p + 2]);
    hi = umax(hi, a[p + 2]);
  }
  const uint32_t range2 = 2u * (hi - lo);
  const int32_t mid2 = (int32_t)(lo + hi) - 2 * E::kBias + (SIGNED ? 8 : 0);  // lo + hi of the true values (+ 8: the signed rounding)
  uint32_t best_sse = 0xffffffffu, best_tmb = 0u;  // table << 16 | multiplier << 8 | base byte
  bool done = false;
  ICAMD_NOUNROLL
  for (int t = 0; t < 16 && !done; ++t) {  // wave-uniform: the table's constants are scalars
    const uint32_t mags = eac_mags((uint32_t)t), span = 2u * (mags >> 24) - 1u, recip = eac_recip_of((uint32_t)t);
    const int32_t m0 = (int32_t)(umad24((range2 + 8u * span) >> 3, recip, 0u) >> 16);
    ICAMD_NOUNROLL
    for (int j = 0; j < 4; ++j) {
      const int32_t m = j == 0 ? 0 : imed3(m0 + j - 2, 1, 15);
      const int32_t s = m == 0 ? 1 : 8 * m;
      const int32_t b0 = (mid2 + s) >> 4;  // (arithmetic: floor)
      ICAMD_UNROLL
      for (int db = -1; db <= 1; ++db) {
        const int32_t b = imed3(b0 + db, E::kBmin, E::kBmax);
        int32_t v[8];
        eac11_16_values(mags, s, 8 * b + E::kBase0, E::kVmax, v);
        const uint32_t sse = eac_sse(a, v);  // (at most 16 * 2047^2 < 2^27)
        const bool better = sse < best_sse;
        best_tmb = better ? ((uint32_t)t << 16 | (uint32_t)m << 8 | ((uint32_t)b & 255u)) : best_tmb;
        best_sse = better ? sse : best_sse;
      }
      // once EVERY lane of the wave holds sse 0 nothing later can be strictly smaller
      if (wave_all(best_sse == 0u)) { done = true; break; }
    }
  }
  const uint32_t t = best_tmb >> 16, m = (best_tmb >> 8) & 15u, byte0 = best_tmb & 255u;
  const int32_t b = SIGNED ? (int32_t)(byte0 << 24) >> 24 : (int32_t)byte0;
  int32_t v[8];
  eac11_16_values(eac_mags(t & 15u), m == 0u ? 1 : (int32_t)(8u * m), 8 * b + E::kBase0, E::kVmax, v);
  return eac_pack_values(a, v, byte0 << 24 | m << 20 | t << 16);
}

// ---- decode ----
// w0, w1: the 8 bytes of an EAC word as little-endian dwords.  rows[y]: the four 16-bit values of pixel row y, texel x in
// half x & 1 of rows[y][x >> 1] (uint16, or int16 in two's complement).  The eight values' low and high bytes lie in two dwords
// each, and one v_perm_b32 pair per row picks them by the row's indices, as decode_eac11 does for bytes.
template <bool SIGNED>
ICAMD_DEV void decode_eac11_16(uint32_t w0, uint32_t w1, uint32_t rows[4][2]) {
  const uint32_t hi = perm(0u, w0, 0x00010203u), lo = perm(0u, w1, 0x00010203u);
  const uint32_t mul = (hi >> 20) & 15u, mags = eac_mags((hi >> 16) & 15u);
  const int32_t s = mul == 0u ? 1 : (int32_t)(8u * mul);
  int32_t bb;  // the base term of the true value
  if (SIGNED) bb = 8 * imax((int32_t)hi >> 24, -127);  // (-128 reads as -127)
  else bb = (int32_t)(8u * (hi >> 24) + 4u);
  uint32_t l03 = 0u, l47 = 0u, h03 = 0u, h47 = 0u;  // low / high bytes of values 0..3 and 4..7
  ICAMD_UNROLL
  for (int k = 0; k < 8; ++k) {
    const int32_t g = (int32_t)bfe(mags, 8 * (k & 3), 8);
    uint32_t o;
    if (SIGNED) {
      const int32_t v = imed3(imad24(k < 4 ? -g : g - 1, s, bb), -1023, 1023);
      const int32_t mag = v < 0 ? -v : v, e = (mag << 5) + (mag >> 5);
      o = (uint32_t)(v < 0 ? -e : e) & 0xffffu;
    } else {
      const uint32_t v = (uint32_t)imed3(imad24(k < 4 ? -g : g - 1, s, bb), 0, 2047);
      o = v << 5 | v >> 6;
    }
    if (k < 4) { l03 |= (o & 255u) << (8 * k); h03 |= (o >> 8) << (8 * k); }
    else { l47 |= (o & 255u) << (8 * (k - 4)); h47 |= (o >> 8) << (8 * (k - 4)); }
  }
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    uint32_t sel = 0u;
    ICAMD_UNROLL
    for (int x = 0; x < 4; ++x) sel |= eac_index(hi, lo, 4 * x + y) << (8 * x);
    const uint32_t l = perm(l47, l03, sel), h = perm(h47, h03, sel);
    rows[y][0] = perm(h, l, 0x05010400u);
    rows[y][1] = perm(h, l, 0x07030602u);
  }
}

// ---- metric ----
// Sums of squared differences and largest absolute differences of channel k (0 = R, 1 = G), decoded 16-bit value against
// the stored 16-bit sample.  A squared difference is below 2^32, so a lane's sums are 64-bit.
struct Eac16Acc {
  uint64_t sse[2];
  uint32_t mx[2];
};
ICAMD_DEV void eac16_clear(Eac16Acc &a) {
  a.sse[0] = a.sse[1] = 0u;
  a.mx[0] = a.mx[1] = 0u;
}

// One channel of one block: s, the stored samples (eac11_16_fetch), against the word (w0, w1); only the cols x rows texels
// inside the image count.
template <bool SIGNED, int K>
ICAMD_DEV void metric_eac11_16_plane(const uint32_t s[8], uint32_t w0, uint32_t w1, uint32_t cols, uint32_t rows, Eac16Acc &a) {
  uint32_t d[4][2];
  decode_eac11_16<SIGNED>(w0, w1, d);
  const uint32_t flip = SIGNED ? 0x8000u : 0u;  // int16 -> its order-preserving uint16
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y)
    ICAMD_UNROLL
    for (int x = 0; x < 4; ++x) {
      const uint32_t sv = (bfe(s[2 * y + (x >> 1)], 16 * (x & 1), 16) ^ flip), dv = (bfe(d[y][x >> 1], 16 * (x & 1), 16) ^ flip);
      const uint32_t e = ((uint32_t)x < cols && (uint32_t)y < rows) ? sad_u32(sv, dv, 0u) : 0u;
      a.sse[K] += (uint64_t)(e * e);  // (e <= 65535: the product fits 32 bits)
      a.mx[K] = umax(a.mx[K], e);
    }
}

// The block of words w (2 for R11, 4 for RG11) at pixel (row, col) against the C-sample source pixels there.
// PRECONDITION row < h, col < wd.
template <int C, bool RG, bool SIGNED>
ICAMD_DEV void metric_eac11_16_block(const uint32_t *w, const uint8_t *img, uint32_t h, uint32_t wd, uint32_t stride,
                                     uint32_t row, uint32_t col, Eac16Acc &a) {
  uint32_t sr[8], sg[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
  eac11_16_fetch<C, RG>(img, h, wd, stride, row, col, sr, sg);
  const uint32_t cols = umin(wd - col, 4u), rows = umin(h - row, 4u);
  metric_eac11_16_plane<SIGNED, 0>(sr, w[0], w[1], cols, rows, a);
  if (RG) metric_eac11_16_plane<SIGNED, 1>(sg, w[2], w[3], cols, rows, a);
}

}  // namespace icamd
#endif  // ICAMD_EAC11_16_BLOCK_H_
