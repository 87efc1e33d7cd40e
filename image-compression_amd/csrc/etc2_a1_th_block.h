// etc2_a1_th_block.h -- the masked T / H search of icamd_encode_etc2_colour_device(ICAMD_ETC2_RGB8A1, ...,
// ICAMD_ETC2_COLOUR_PLANAR_TH) for blocks with 1..15 transparent texels (EXTENSION, include/ic_amd.h), one block
// per lane, on the pieces of etc2_th_block.h.  Integers only, no memory tables.
//
// A DEFINITION, not a heuristic.  O = the opaque texels (byte 3 >= 128), n = |O|, W = the word icamd_encode_device(
// ICAMD_ETC2_RGB8A1) writes for the block, err = squared RGB error summed over O, W read by decode_etc2_a1.
//   Partitions of O into clusters A and B, tried in this order; one with A or B empty is dropped:
//     L: Y_p = R + 2 G + B, p in B iff n Y_p > Sum_O Y.
//     C: c* = the channel with the largest max - min over O (ties R, G, B), p in B iff 2 v_p[c*] > max + min over O.
//   Cluster colours: the rule of etc2_th_block.h over the cluster's m texels; a partition with equal 12-bit codes is dropped.
//   Candidates of a partition, in order, each with di = 0..7 ascending; the paints are the decoder's under Op = 0, where index 2
//   is the transparent texel:
//     T(C1 = a, C2 = b): {0: C1, 1: clamp(C2 + d), 3: clamp(C2 - d)};  T(C1 = b, C2 = a) likewise;
//     H(a, b): (C1, C2) = (a, b) where (a >= b as R << 16 | G << 8 | B) == (di & 1), else (b, a) -- the stored order IS di's low
//       bit; {0: clamp(C1 + d), 1: clamp(C1 - d), 3: clamp(C2 - d)}.  No index is flipped.
//   Every opaque texel takes the allowed index (0, 1, 3) with the smallest squared RGB distance, ties to the smallest index;
//   transparent texels take index 2 and add no error.  The best candidate has the smallest error, ties to the earliest
//   (partition, candidate, di).  The block is its word if its error is STRICTLY smaller than err(W), else W byte for byte.
//   Packing: that of etc2_th_block.h with bit 33 clear.
//
// How it is computed: as etc2_th_block.h -- closeness t = 2 v.c - c.c, a candidate's error is Sum_O v.v - Sum_O max_k t, the key
// err << 6 | order -- on texels whose transparent members are ZEROED: such a texel has t = -c.c for every paint, so a sum over
// all sixteen exceeds the sum over O by (16 - n) max_k (-c.c), which is taken off once per candidate instead of masking every
// term.  Shortcuts, each giving the definition's bytes: err(W) == 0; a dropped partition; partition C where its cluster B is L's
// B or L's A (T(a, b) and T(b, a) exchange places and H depends on the unordered pair only, so each of its candidates has the
// error of an L candidate, which comes earlier).  All are per-lane branches; none is decided for the wave.
#ifndef ICAMD_ETC2_A1_TH_BLOCK_H_
#define ICAMD_ETC2_A1_TH_BLOCK_H_

#include "etc2_a1_block.h"
#include "etc2_th_block.h"

namespace icamd {

// The two partitions of the n opaque texels as masks over the raster index r = 4 y + x: bit r set = texel r is in cluster B.
// s: the texels with the transparent ones zeroed; o: bit r = texel r is opaque.
ICAMD_DEV void etc2_a1_th_partitions(const uint32_t s[16], uint32_t o, uint32_t n, uint32_t *mask_l, uint32_t *mask_c) {
  uint32_t lum[16], sum_y = 0u, mn[3], mx[3];
  ICAMD_UNROLL
  for (int ch = 0; ch < 3; ++ch) {
    mn[ch] = 255u;
    mx[ch] = 0u;
  }
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint32_t out = ~bit_mask(o, (uint32_t)p);
    lum[p] = udot4(s[p], 0x00010201u, 0u);  // (0 for a transparent texel)
    sum_y += lum[p];
    ICAMD_UNROLL
    for (int ch = 0; ch < 3; ++ch) {
      const uint32_t v = bfe(s[p], 8u * (uint32_t)ch, 8u);
      mn[ch] = umin(mn[ch], v | out);
      mx[ch] = umax(mx[ch], v);
    }
  }
  const uint32_t range_r = mx[0] - mn[0], range_g = mx[1] - mn[1], range_b = mx[2] - mn[2];
  const uint32_t ch = range_r >= range_g && range_r >= range_b ? 0u : range_g >= range_b ? 1u : 2u;  // ties: R, then G, then B
  const uint32_t mid2 = ch == 0u ? mx[0] + mn[0] : ch == 1u ? mx[1] + mn[1] : mx[2] + mn[2];
  uint32_t ml = 0u, mc = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    ml |= (umad24(n, lum[p], 0u) > sum_y ? 1u : 0u) << p;
    mc |= (2u * bfe(s[p], 8u * ch, 8u) > mid2 ? 1u : 0u) << p;
  }
  *mask_l = ml & o;
  *mask_c = mc & o;
}

// The cluster colours a (opaque texels outside `mask`) and b (inside) of a partition of the n opaque texels; false where it is
// dropped.  s: the texels with the transparent ones zeroed, so every sum below is a sum over O.
ICAMD_DEV bool etc2_a1_th_colours(const uint32_t s[16], uint32_t mask, uint32_t n, uint32_t *ca, uint32_t *cb) {
  uint32_t all_rb = 0u, all_g = 0u, b_rb = 0u, b_g = 0u, nb = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint32_t rb = s[p] & 0x00ff00ffu, g = bfe(s[p], 8u, 8u), in_b = bit_mask(mask, (uint32_t)p);
    all_rb += rb;
    all_g += g;
    b_rb += rb & in_b;
    b_g += g & in_b;
    nb += in_b & 1u;
  }
  if (nb == 0u || nb == n) return false;
  *ca = etc2_th_cluster_colour(all_rb - b_rb, all_g - b_g, n - nb);
  *cb = etc2_th_cluster_colour(b_rb, b_g, nb);
  return *ca != *cb;
}

// true where H(a, b) stores (C1, C2) = (a, b) at an ODD di: a >= b as R << 16 | G << 8 | B
ICAMD_DEV bool etc2_a1_th_a_first_when_odd(uint32_t ca, uint32_t cb) {
  return perm(0u, ca, 0x0c000102u) >= perm(0u, cb, 0x0c000102u);
}

// The smallest key err << 6 | order over the 24 candidates of one partition (cluster colours ca, cb; `first` = the order of its
// first candidate: 0 or 24).  s: the texels with the transparent ones zeroed, ss = Sum v.v, holes = 16 - n.
ICAMD_DEV uint32_t etc2_a1_th_partition_best(const uint32_t s[16], uint32_t holes, uint32_t ss, uint32_t ca, uint32_t cb,
                                             uint32_t first) {
  int32_t ta[16], tb[16];  // the unshifted colours: paint 0 of the two T candidates, whatever di
  const int32_t nca = -(int32_t)udot4(ca, ca, 0u), ncb = -(int32_t)udot4(cb, cb, 0u);
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    ta[p] = etc2_th_t(s[p], ca, nca);
    tb[p] = etc2_th_t(s[p], cb, ncb);
  }
  const uint32_t odd_ab = etc2_a1_th_a_first_when_odd(ca, cb) ? 1u : 0u;
  const int32_t nh = (int32_t)holes;
  uint32_t best = kEtc2ThNone;
  ICAMD_NOUNROLL
  for (uint32_t di = 0; di < 8u; ++di) {
    const int32_t d = etc2_th_distance(di);
    const uint32_t ap = etc2_th_shift(ca, d), am = etc2_th_shift(ca, -d), bp = etc2_th_shift(cb, d), bm = etc2_th_shift(cb, -d);
    const int32_t nap = -(int32_t)udot4(ap, ap, 0u), nam = -(int32_t)udot4(am, am, 0u);
    const int32_t nbp = -(int32_t)udot4(bp, bp, 0u), nbm = -(int32_t)udot4(bm, bm, 0u);
    // Sum over all sixteen of max_k t, less what the zeroed texels put in: holes * max_k (-c.c)
    int32_t t_ab = -nh * imax(nca, imax(nbp, nbm)), t_ba = -nh * imax(ncb, imax(nap, nam));
    int32_t h_ab = -nh * imax(imax(nap, nam), nbm), h_ba = -nh * imax(imax(nbp, nbm), nam);
    ICAMD_UNROLL
    for (int p = 0; p < 16; ++p) {
      const int32_t tam = etc2_th_t(s[p], am, nam), tbm = etc2_th_t(s[p], bm, nbm);
      const int32_t near_a = imax(etc2_th_t(s[p], ap, nap), tam);
      const int32_t near_b = imax(etc2_th_t(s[p], bp, nbp), tbm);
      t_ab += imax(ta[p], near_b);  // C1 = a, C2 = b: a, b + d, -, b - d
      t_ba += imax(tb[p], near_a);
      h_ab += imax(near_a, tbm);    // C1 = a, C2 = b: a + d, a - d, -, b - d
      h_ba += imax(near_b, tam);
    }
    const int32_t h = (di & 1u) == odd_ab ? h_ab : h_ba;
    best = umin(best, (ss - (uint32_t)t_ab) << 6 | (first + di));
    best = umin(best, (ss - (uint32_t)t_ba) << 6 | (first + 8u + di));
    best = umin(best, (ss - (uint32_t)h) << 6 | (first + 16u + di));
  }
  return best;
}

// The upper half word (bits 63..32) of the T or H word with Op = 0 (bit 33 clear) that stores the expanded colours c1, c2 in this
// order: the fields and overflow patterns of etc2_th_word.  T stores all of di; H stores di >> 1 -- di's lowest bit is the
// order of the two colours.
ICAMD_DEV uint32_t etc2_a1_th_pack_hi(uint32_t c1, uint32_t c2, bool h_mode, uint32_t di) {
  const uint32_t r1 = bfe(c1, 4u, 4u), g1 = bfe(c1, 12u, 4u), b1 = bfe(c1, 20u, 4u);  // (a byte 17 q is q << 4 | q)
  const uint32_t r2 = bfe(c2, 4u, 4u), g2 = bfe(c2, 12u, 4u), b2 = bfe(c2, 20u, 4u);
  uint32_t hi;
  if (h_mode) {
    hi = (g1 >> 3) << 31 | r1 << 27 | (g1 >> 1) << 24 | (g1 & 1u) << 20 | (b1 >> 3) << 19 | (b1 & 7u) << 15 | r2 << 11 | g2 << 7 |
         b2 << 3 | (di >> 2) << 2 | ((di >> 1) & 1u);
    hi |= ((g1 & 1u) << 1 | b1 >> 3) + ((b1 >> 1) & 3u) >= 4u ? 7u << 21 : 1u << 18;
  } else {
    hi = (r1 >> 2) << 27 | (r1 & 3u) << 24 | g1 << 20 | b1 << 16 | r2 << 12 | g2 << 8 | b2 << 4 | (di >> 1) << 2 | (di & 1u);
    hi |= (r1 >> 2) + (r1 & 3u) >= 4u ? 7u << 29 : 1u << 26;
  }
  return hi;
}

// The word of candidate (kind 0: T(a, b), 1: T(b, a), 2: H(a, b); di) on the cluster colours ca, cb under Op = 0: the colours and
// di packed, the paints read back as the decoder reads them, every opaque texel on the nearest of paints 0, 1 and 3, every
// transparent one on index 2.
ICAMD_DEV Out8 etc2_a1_th_word(const uint32_t s[16], uint32_t o, uint32_t ca, uint32_t cb, uint32_t kind, uint32_t di) {
  const bool h_mode = kind == 2u;
  uint32_t c1 = kind == 1u ? cb : ca, c2 = kind == 1u ? ca : cb;
  if (h_mode && (etc2_a1_th_a_first_when_odd(c1, c2) ? 1u : 0u) != (di & 1u)) {  // the stored order carries di's lowest bit
    const uint32_t t = c1;
    c1 = c2;
    c2 = t;
  }
  const uint32_t hi = etc2_a1_th_pack_hi(c1, c2, h_mode, di);
  uint32_t paint[4];
  etc2_th_paints(hi, h_mode, paint);
  const int32_t n0 = -(int32_t)udot4(paint[0], paint[0], 0u), n1 = -(int32_t)udot4(paint[1], paint[1], 0u);
  const int32_t n3 = -(int32_t)udot4(paint[3], paint[3], 0u);
  uint32_t lo = 0u;
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    ICAMD_UNROLL
    for (int x = 0; x < 4; ++x) {
      const uint32_t v = s[4 * y + x];
      const int32_t t0 = etc2_th_t(v, paint[0], n0), t1 = etc2_th_t(v, paint[1], n1), t3 = etc2_th_t(v, paint[3], n3);
      uint32_t k = t1 > t0 ? 1u : 0u;  // the first nearest
      k = t3 > imax(t0, t1) ? 3u : k;
      k = bit_mask(o, (uint32_t)(4 * y + x)) ? k : 2u;
      const int p = 4 * x + y;
      lo |= (k & 1u) << p | (k >> 1) << (p + 16);
    }
  }
  const Out8 out = { perm(0u, hi, 0x00010203u), perm(0u, lo, 0x00010203u) };  // big-endian words in memory
  return out;
}

// The smallest key over both partitions and the winner's cluster colours; kEtc2ThNone where no partition survives.
ICAMD_DEV uint32_t etc2_a1_th_search(const uint32_t s[16], uint32_t o, uint32_t n, uint32_t ss, uint32_t *ca, uint32_t *cb) {
  uint32_t mask_l, mask_c, la = 0u, lb = 0u, xa = 0u, xb = 0u;
  etc2_a1_th_partitions(s, o, n, &mask_l, &mask_c);
  uint32_t best = kEtc2ThNone;
  if (etc2_a1_th_colours(s, mask_l, n, &la, &lb)) best = etc2_a1_th_partition_best(s, 16u - n, ss, la, lb, 0u);
  if (mask_c != mask_l && mask_c != (mask_l ^ o) && etc2_a1_th_colours(s, mask_c, n, &xa, &xb))
    best = umin(best, etc2_a1_th_partition_best(s, 16u - n, ss, xa, xb, 24u));
  const bool second = (best & 63u) >= 24u;  // (kEtc2ThNone: order 63, and the colours are not read)
  *ca = second ? xa : la;
  *cb = second ? xb : lb;
  return best;
}

// A block with 1..15 transparent texels: px its sixteen texels, o its opaque mask (etc2_a1_opaque_mask), w its ICAMD_ETC2_RGB8A1
// word.  true and the T / H word in *out where one is strictly closer over the opaque texels, else false (the block stays w).
ICAMD_DEV bool etc2_a1_th_choose_masked(const uint32_t px[16], uint32_t o, Out8 w, Out8 *out) {
  uint32_t s[16], ca, cb, n = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint32_t in_o = bit_mask(o, (uint32_t)p);
    s[p] = px[p] & 0x00ffffffu & in_o;
    n += in_o & 1u;
  }
  const uint32_t ss = etc2_sum_squares(s);
  uint32_t err_w;
  {
    uint32_t d[16];
    decode_etc2_a1(w.lo, w.hi, false, d);
    ICAMD_UNROLL
    for (int p = 0; p < 16; ++p) d[p] &= 0x00ffffffu & bit_mask(o, (uint32_t)p);
    err_w = etc2_sse_rgb(s, ss, d);
  }
  if (err_w == 0u) return false;
  const uint32_t best = etc2_a1_th_search(s, o, n, ss, &ca, &cb);
  if (best == kEtc2ThNone || (best >> 6) >= err_w) return false;
  const uint32_t order = best & 63u, in_part = order >= 24u ? order - 24u : order;
  *out = etc2_a1_th_word(s, o, ca, cb, in_part >> 3, in_part & 7u);
  return true;
}

// The block of icamd_encode_etc2_colour_device(ICAMD_ETC2_RGB8A1, ..., ICAMD_ETC2_COLOUR_PLANAR_TH) whose ICAMD_ETC2_RGB8A1 word
// is w, by its class: all transparent -- w; none transparent -- the T / H search of ICAMD_ETC2_RGB8 on w (Op = 1); else the masked
// search above.  true and the word in *out where the block changes.
ICAMD_DEV bool etc2_a1_th_choose(const uint32_t px[16], Out8 w, Out8 *out) {
  const uint32_t o = etc2_a1_opaque_mask(px);
  if (o == 0u) return false;
  if (o == 0xffffu) return etc2_th_choose(px, w, out);
  return etc2_a1_th_choose_masked(px, o, w, out);
}

// The colour word of icamd_encode_etc2_colour_device(ICAMD_ETC2_RGBA8, ...) for the block whose ETC1 word is e: ICAMD_ETC2_RGB8's
// planar choice, then (TH) its T / H search.  Alpha (byte 3 of px) never enters.
template <bool TH>
ICAMD_DEV Out8 etc2_rgba8_colour_choose(const uint32_t px[16], Out8 e) {
  Out8 o = etc2_rgb8_choose(px, e), th;
  if (TH && etc2_th_choose(px, o, &th)) o = th;
  return o;
}

}  // namespace icamd
#endif  // ICAMD_ETC2_A1_TH_BLOCK_H_
