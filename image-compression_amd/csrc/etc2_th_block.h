// etc2_th_block.h -- the T / H search of icamd_encode_etc2_device(ICAMD_ETC2_RGB8, ..., ICAMD_ETC2_MODES_TH) (EXTENSION,
// include/ic_amd.h), one block per lane.  Integers only, no memory tables.
//
// A DEFINITION, not a heuristic.  v_p = the sixteen texels the ETC1 block routine is handed (bytes 0..2), W = the word
// icamd_encode_device(ICAMD_ETC2_RGB8) writes for them, err = squared error summed over 16 texels x 3 channels.
//   Partitions into clusters A and B, tried in this order; one with A or B empty is dropped:
//     L: Y_p = R + 2 G + B, p in B iff 16 Y_p > Sum Y.
//     C: c* = the channel with the largest max - min (ties R, G, B), p in B iff 2 v_p[c*] > max + min.
//   Cluster colours: per channel the 4-bit code q = (30 S + 255 n) / (510 n), truncating (n texels, channel sum S), the
//     colour 17 q; a (from A), b (from B).  A partition with equal 12-bit codes is dropped.
//   Candidates of a partition, in order, each with di = 0..7 ascending: T(C1 = a, C2 = b), T(C1 = b, C2 = a), H(a, b); the
//     paints are the decoder's (etc2_colour_block.h), no refinement.  Every texel takes the paint with the smallest squared
//     RGB distance, ties to the smallest paint index; the candidate's error is the sum.
//   The best candidate has the smallest error, ties to the earliest (partition, candidate, di).  The block is its word if its
//     error is STRICTLY smaller than err(W), else W byte for byte.
//   Packing: bit 33 set.  T: with a = R1 >> 2, b = R1 & 3, bits 63-61 = 111 and bit 58 = 0 where a + b >= 4, else 000 and 1 (byte
//     0 overflows).  H: bit 34 = di >> 2, bit 32 = (di >> 1) & 1; where (C1 >= C2) != (di & 1) for (C1, C2) = (a, b) the
//     colours are stored swapped and every index flipped by k ^= 2; bit 63 = G1 bit 3 (byte 0 does not overflow); with
//     a' = (G1 & 1) << 1 | B1 >> 3, b' = (B1 >> 1) & 3, bits 55-53 = 111 and bit 50 = 0 where a' + b' >= 4, else 000 and 1.
//
// How it is computed.  |v - c|^2 = v.v - (2 v.c - c.c): per texel and paint one dot product and one shift-add give the
// closeness t = 2 v.c - c.c, a candidate's error is Sum v.v - Sum_p max_k t, and the index search runs for the winner only.  The
// three candidates of a (partition, di) share their six paints' t.  A candidate is ranked by the key err << 6 | order (err < 2^22,
// order = 24 partition + 8 candidate + di), so "smallest error, earliest on a tie" is one unsigned minimum.
// Shortcuts, each giving the definition's bytes: err(W) == 0 (nothing is strictly smaller); a dropped partition; partition C
// where its cluster B is L's B or L's A (the same two colours: each of its candidates has the error of an L candidate, which
// comes earlier).  All are per-lane branches; none is decided for the wave.
#ifndef ICAMD_ETC2_TH_BLOCK_H_
#define ICAMD_ETC2_TH_BLOCK_H_

#include "etc2_colour_block.h"

namespace icamd {

// q = (30 S + 255 n) / (510 n) = (2 S + 17 n) / (34 n) for n in 1..15, S in 0..255 n: q <= 15, so four steps of restoring
// division, no multiply and no reciprocal table -- checked for every reachable argument below.
constexpr uint32_t etc2_th_quantise(uint32_t sum, uint32_t n) {
  uint32_t num = 2u * sum + 17u * n, q = 0u;
  const uint32_t m = 34u * n;
  if (num >= m << 3) { num -= m << 3; q |= 8u; }
  if (num >= m << 2) { num -= m << 2; q |= 4u; }
  if (num >= m << 1) { num -= m << 1; q |= 2u; }
  if (num >= m) q |= 1u;
  return q;
}
namespace detail {
constexpr bool check_th_quantise(uint32_t n) {
  for (uint32_t s = 0; s <= 255u * n; ++s)
    if (etc2_th_quantise(s, n) != (30u * s + 255u * n) / (510u * n)) return false;
  return true;
}
static_assert(check_th_quantise(1u) && check_th_quantise(2u) && check_th_quantise(3u), "T / H cluster code, n = 1..3");
static_assert(check_th_quantise(4u) && check_th_quantise(5u) && check_th_quantise(6u), "T / H cluster code, n = 4..6");
static_assert(check_th_quantise(7u) && check_th_quantise(8u) && check_th_quantise(9u), "T / H cluster code, n = 7..9");
static_assert(check_th_quantise(10u) && check_th_quantise(11u) && check_th_quantise(12u), "T / H cluster code, n = 10..12");
static_assert(check_th_quantise(13u) && check_th_quantise(14u) && check_th_quantise(15u), "T / H cluster code, n = 13..15");
}  // namespace detail

constexpr uint32_t kEtc2ThNone = 0xffffffffu;  // the key of "no candidate"

// d[di], di < 8 (the table of etc2_th_paints, as two packed constants)
ICAMD_DEV int32_t etc2_th_distance(uint32_t di) {
  return (int32_t)bfe(di < 4u ? (3u | 6u << 8 | 11u << 16 | 16u << 24) : (23u | 32u << 8 | 41u << 16 | 64u << 24), 8u * (di & 3u), 8u);
}

// colour c (R | G << 8 | B << 16) with d added to every channel, clamped
ICAMD_DEV uint32_t etc2_th_shift(uint32_t c, int32_t d) {
  return etc2_pack_clamped((int32_t)bfe(c, 0u, 8u) + d, (int32_t)bfe(c, 8u, 8u) + d, (int32_t)bfe(c, 16u, 8u) + d);
}

// t = 2 v.c - c.c of texel v and paint c (ncc = -c.c): v.v less |v - c|^2, so the nearest paint has the largest t.
// v.c <= 3 * 255^2 < 2^18: one shift-add.
ICAMD_DEV int32_t etc2_th_t(uint32_t v, uint32_t c, int32_t ncc) { return (int32_t)((udot4(v, c, 0u) << 1) + (uint32_t)ncc); }

// The expanded colour (R | G << 8 | B << 16, each 17 q) of a cluster of n texels (1..15) whose channel sums are
// rb = Sum R | Sum B << 16 and g = Sum G.
ICAMD_DEV uint32_t etc2_th_cluster_colour(uint32_t rb, uint32_t g, uint32_t n) {
  return 17u * (etc2_th_quantise(rb & 0xffffu, n) | etc2_th_quantise(g, n) << 8 | etc2_th_quantise(rb >> 16, n) << 16);
}

// The two partitions as masks over the raster index r = 4 y + x: bit r set = texel r is in cluster B.
ICAMD_DEV void etc2_th_partitions(const uint32_t s[16], uint32_t *mask_l, uint32_t *mask_c) {
  uint32_t lum[16], sum_y = 0u, mn[3], mx[3];
  ICAMD_UNROLL
  for (int ch = 0; ch < 3; ++ch) {
    mn[ch] = 255u;
    mx[ch] = 0u;
  }
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    lum[p] = udot4(s[p], 0x00010201u, 0u);
    sum_y += lum[p];
    ICAMD_UNROLL
    for (int ch = 0; ch < 3; ++ch) {
      const uint32_t v = bfe(s[p], 8u * (uint32_t)ch, 8u);
      mn[ch] = umin(mn[ch], v);
      mx[ch] = umax(mx[ch], v);
    }
  }
  const uint32_t range_r = mx[0] - mn[0], range_g = mx[1] - mn[1], range_b = mx[2] - mn[2];
  const uint32_t ch = range_r >= range_g && range_r >= range_b ? 0u : range_g >= range_b ? 1u : 2u;  // ties: R, then G, then B
  const uint32_t mid2 = ch == 0u ? mx[0] + mn[0] : ch == 1u ? mx[1] + mn[1] : mx[2] + mn[2];
  uint32_t ml = 0u, mc = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    ml |= (16u * lum[p] > sum_y ? 1u : 0u) << p;
    mc |= (2u * bfe(s[p], 8u * ch, 8u) > mid2 ? 1u : 0u) << p;
  }
  *mask_l = ml;
  *mask_c = mc;
}

// The cluster colours a (texels outside `mask`) and b (inside) of a partition; false where it is dropped.
ICAMD_DEV bool etc2_th_colours(const uint32_t s[16], uint32_t mask, uint32_t *ca, uint32_t *cb) {
  uint32_t all_rb = 0u, all_g = 0u, b_rb = 0u, b_g = 0u, nb = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint32_t rb = s[p] & 0x00ff00ffu, g = bfe(s[p], 8u, 8u), in_b = bit_mask(mask, (uint32_t)p);
    all_rb += rb;  // (16 * 255 < 2^16: the two sums stay in their halves)
    all_g += g;
    b_rb += rb & in_b;
    b_g += g & in_b;
    nb += in_b & 1u;
  }
  if (nb == 0u || nb == 16u) return false;
  *ca = etc2_th_cluster_colour(all_rb - b_rb, all_g - b_g, 16u - nb);
  *cb = etc2_th_cluster_colour(b_rb, b_g, nb);
  return *ca != *cb;
}

// The smallest key err << 6 | order over the 24 candidates of one partition (cluster colours ca, cb; `first` = the order of its
// first candidate: 0 or 24).  ss = Sum v.v of the texels.
ICAMD_DEV uint32_t etc2_th_partition_best(const uint32_t s[16], uint32_t ss, uint32_t ca, uint32_t cb, uint32_t first) {
  int32_t base[16];  // the nearer of the two unshifted colours: paints 0 and 2 of both T candidates, whatever di
  const int32_t nca = -(int32_t)udot4(ca, ca, 0u), ncb = -(int32_t)udot4(cb, cb, 0u);
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) base[p] = imax(etc2_th_t(s[p], ca, nca), etc2_th_t(s[p], cb, ncb));
  uint32_t best = kEtc2ThNone;
  ICAMD_NOUNROLL
  for (uint32_t di = 0; di < 8u; ++di) {
    const int32_t d = etc2_th_distance(di);
    const uint32_t ap = etc2_th_shift(ca, d), am = etc2_th_shift(ca, -d), bp = etc2_th_shift(cb, d), bm = etc2_th_shift(cb, -d);
    const int32_t nap = -(int32_t)udot4(ap, ap, 0u), nam = -(int32_t)udot4(am, am, 0u);
    const int32_t nbp = -(int32_t)udot4(bp, bp, 0u), nbm = -(int32_t)udot4(bm, bm, 0u);
    int32_t t_ab = 0, t_ba = 0, h = 0;  // Sum_p max_k t: the error is ss less the sum, and never negative
    ICAMD_UNROLL
    for (int p = 0; p < 16; ++p) {
      const int32_t near_a = imax(etc2_th_t(s[p], ap, nap), etc2_th_t(s[p], am, nam));
      const int32_t near_b = imax(etc2_th_t(s[p], bp, nbp), etc2_th_t(s[p], bm, nbm));
      t_ab += imax(base[p], near_b);  // C1 = a, C2 = b: a, b + d, b, b - d
      t_ba += imax(base[p], near_a);
      h += imax(near_a, near_b);
    }
    best = umin(best, (ss - (uint32_t)t_ab) << 6 | (first + di));
    best = umin(best, (ss - (uint32_t)t_ba) << 6 | (first + 8u + di));
    best = umin(best, (ss - (uint32_t)h) << 6 | (first + 16u + di));
  }
  return best;
}

// The word of candidate (kind 0: T(a, b), 1: T(b, a), 2: H(a, b); di) on the cluster colours ca, cb: the colours and di packed,
// the paints read back as the decoder reads them, every texel on its nearest paint.
ICAMD_DEV Out8 etc2_th_word(const uint32_t s[16], uint32_t ca, uint32_t cb, uint32_t kind, uint32_t di) {
  const bool h_mode = kind == 2u;
  uint32_t c1 = kind == 1u ? cb : ca, c2 = kind == 1u ? ca : cb;
  uint32_t flip = 0u;
  if (h_mode) {  // the order of the stored colours carries di's lowest bit
    const uint32_t v1 = perm(0u, c1, 0x0c000102u), v2 = perm(0u, c2, 0x0c000102u);  // R << 16 | G << 8 | B
    if ((v1 >= v2 ? 1u : 0u) != (di & 1u)) {
      const uint32_t t = c1;
      c1 = c2;
      c2 = t;
      flip = 2u;
    }
  }
  const uint32_t r1 = bfe(c1, 4u, 4u), g1 = bfe(c1, 12u, 4u), b1 = bfe(c1, 20u, 4u);  // (a byte 17 q is q << 4 | q)
  const uint32_t r2 = bfe(c2, 4u, 4u), g2 = bfe(c2, 12u, 4u), b2 = bfe(c2, 20u, 4u);
  uint32_t hi;
  if (h_mode) {
    hi = (g1 >> 3) << 31 | r1 << 27 | (g1 >> 1) << 24 | (g1 & 1u) << 20 | (b1 >> 3) << 19 | (b1 & 7u) << 15 | r2 << 11 | g2 << 7 |
         b2 << 3 | (di >> 2) << 2 | 2u | ((di >> 1) & 1u);
    hi |= ((g1 & 1u) << 1 | b1 >> 3) + ((b1 >> 1) & 3u) >= 4u ? 7u << 21 : 1u << 18;
  } else {
    hi = (r1 >> 2) << 27 | (r1 & 3u) << 24 | g1 << 20 | b1 << 16 | r2 << 12 | g2 << 8 | b2 << 4 | (di >> 1) << 2 | 2u | (di & 1u);
    hi |= (r1 >> 2) + (r1 & 3u) >= 4u ? 7u << 29 : 1u << 26;
  }
  uint32_t stored[4];
  etc2_th_paints(hi, h_mode, stored);
  // the paints in the candidate's own order j, and the index k[j] = j ^ flip each is stored under
  uint32_t paint[4], k[4];
  int32_t ncc[4];
  ICAMD_UNROLL
  for (int j = 0; j < 4; ++j) {
    k[j] = (uint32_t)j ^ flip;
    paint[j] = flip ? stored[j ^ 2] : stored[j];
    ncc[j] = -(int32_t)udot4(paint[j], paint[j], 0u);
  }
  uint32_t lo = 0u;
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    ICAMD_UNROLL
    for (int x = 0; x < 4; ++x) {
      const uint32_t v = s[4 * y + x];
      uint32_t best_k = k[0];  // the first nearest
      int32_t best_t = etc2_th_t(v, paint[0], ncc[0]);
      ICAMD_UNROLL
      for (int j = 1; j < 4; ++j) {
        const int32_t t = etc2_th_t(v, paint[j], ncc[j]);
        best_k = t > best_t ? k[j] : best_k;
        best_t = imax(best_t, t);
      }
      const int p = 4 * x + y;
      lo |= (best_k & 1u) << p | (best_k >> 1) << (p + 16);
    }
  }
  const Out8 o = { perm(0u, hi, 0x00010203u), perm(0u, lo, 0x00010203u) };  // big-endian words in memory
  return o;
}

// The smallest key over both partitions of the texels s (bytes 0..2; byte 3 zero) and the winner's cluster colours;
// kEtc2ThNone where no partition survives.  ss = Sum v.v.
ICAMD_DEV uint32_t etc2_th_search(const uint32_t s[16], uint32_t ss, uint32_t *ca, uint32_t *cb) {
  uint32_t mask_l, mask_c, la = 0u, lb = 0u, xa = 0u, xb = 0u;
  etc2_th_partitions(s, &mask_l, &mask_c);
  uint32_t best = kEtc2ThNone;
  if (etc2_th_colours(s, mask_l, &la, &lb)) best = etc2_th_partition_best(s, ss, la, lb, 0u);
  if (mask_c != mask_l && mask_c != (mask_l ^ 0xffffu) && etc2_th_colours(s, mask_c, &xa, &xb))
    best = umin(best, etc2_th_partition_best(s, ss, xa, xb, 24u));
  const bool second = (best & 63u) >= 24u;  // (kEtc2ThNone: order 63, and the colours are not read)
  *ca = second ? xa : la;
  *cb = second ? xb : lb;
  return best;
}

// The block of the sixteen texels px (as the ETC1 block routine was handed them; byte 3 is ignored) whose ICAMD_ETC2_RGB8 word is
// w: true and the T / H word in *o where one is strictly closer, else false (the block stays w).
ICAMD_DEV bool etc2_th_choose(const uint32_t px[16], Out8 w, Out8 *o) {
  uint32_t s[16], ca, cb;
  uint32_t err_w;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) s[p] = px[p] & 0x00ffffffu;
  const uint32_t ss = etc2_sum_squares(s);
  {
    uint32_t d[16];
    decode_etc2_colour(w.lo, w.hi, d);
    err_w = etc2_sse_rgb(s, ss, d);
  }
  if (err_w == 0u) return false;
  const uint32_t best = etc2_th_search(s, ss, &ca, &cb);
  if (best == kEtc2ThNone || (best >> 6) >= err_w) return false;
  const uint32_t order = best & 63u, in_part = order >= 24u ? order - 24u : order;
  *o = etc2_th_word(s, ca, cb, in_part >> 3, in_part & 7u);
  return true;
}

}  // namespace icamd
#endif  // ICAMD_ETC2_TH_BLOCK_H_
