// pvrtc4_block.h -- PVRTC1 4 bpp (extension): the 2 bpp rules on 4 x 4-pixel blocks, block form and one-pass strip.
// Part of pvrtc_block.h.
#ifndef ICAMD_PVRTC4_BLOCK_H_
#define ICAMD_PVRTC4_BLOCK_H_

#include "pvrtc_onepass.h"

namespace icamd {

// ---- PVRTC1 4 bpp (r05): EXTENSION, PARITY UNPINNED -- BASELINE.json's config 5 names "PVRTC 4bpp", the reference only
// has 2 bpp (public/pvrtc_compressor.h:15-18).  The 2 bpp rules above with 4 x 4-pixel blocks, exactly as
// oracle/ic_oracle.c (pvrtc4_encode_image) restates them: GetExtremesFast over 16 pixels, the same channel reduction,
// BestModulation against A / B up-sampled with weights (x + 2) & 3, (y + 2) & 3 out of 4 in both directions, every pixel's
// 2-bit value stored at bits 2 (4 y + x), colour word with bit 0 clear.
// GetExtremesFast (pvrtc.cc:255-329) on px[4 y + x]: the keys of pvrtc_extremes with 4-bit indices.
ICAMD_DEV void pvrtc4_extremes(const uint32_t px[16], uint32_t image0, BlockStash &stash, uint32_t &col_a, uint32_t &col_b) {
  uint32_t kmin_l = 0xffffffffu, kmax_l = 0u, kmin_rb = 0xffffffffu, kmax_rb = 0u, kmin_ga = 0xffffffffu, kmax_ga = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; p += 2) {
    uint32_t kl[2];
    ICAMD_UNROLL
    for (int q = 0; q < 2; ++q) {
      const uint32_t c = px[p + q], i = (uint32_t)((p + q) & 3);
      const uint32_t idx4 = (uint32_t)((p + q) & ~3) * 0x01010101u + 0x03020100u;
      const uint32_t up = (uint32_t)(15 - 2 * (p + q)) * 0x00010001u;  // max-side key = value * 256 + (15 - idx)
      kl[q] = perm(udot4(c, 0x001c964du, 0u), idx4, 0x0c0c0500u | i);
      const uint32_t k_rb = perm(c, idx4, 0x06000400u | i | i << 16), k_ga = perm(c, idx4, 0x07000500u | i | i << 16);
      kmin_rb = pk_min_u16(kmin_rb, k_rb);
      kmin_ga = pk_min_u16(kmin_ga, k_ga);
      kmax_rb = pk_max_u16(kmax_rb, k_rb + up);
      kmax_ga = pk_max_u16(kmax_ga, k_ga + up);
    }
    kmin_l = umin3(kmin_l, kl[0], kl[1]);
    kmax_l = umax3(kmax_l, kl[0] + (uint32_t)(15 - 2 * p), kl[1] + (uint32_t)(15 - 2 * (p + 1)));
  }
  const uint32_t kmin[5] = { kmin_l, kmin_rb & 0xffffu, kmin_ga & 0xffffu, kmin_rb >> 16, kmin_ga >> 16 };
  const uint32_t kmax[5] = { kmax_l, kmax_rb & 0xffffu, kmax_ga & 0xffffu, kmax_rb >> 16, kmax_ga >> 16 };
  stash.put(px);
  uint32_t best_diff = 0, best_lo = 0, best_hi = 0;
  ICAMD_UNROLL
  for (int i = 0; i < 5; ++i) {
    const uint32_t lo = stash.get(kmin[i] & 15u);
    const uint32_t hi_block = stash.get(15u - (kmax[i] & 15u));
    const uint32_t hi = (kmax[i] >> 8) == 0u ? image0 : hi_block;  // never-updated max -> image pixel 0 (pvrtc.cc:268-269)
    const uint32_t d = sad_u8(lo, hi, 0u);
    const bool better = (i == 0) || d > best_diff;
    best_lo = better ? lo : best_lo;
    best_hi = better ? hi : best_hi;
    best_diff = better ? d : best_diff;
  }
  const bool swap = udot4(best_hi, 0x01010101u, 0u) < udot4(best_lo, 0x01010101u, 0u);
  col_a = swap ? best_hi : best_lo;
  col_b = swap ? best_lo : best_hi;
}

// The block's 32-bit modulation word from its pixels and the reduced colours of its 3 x 3 block neighbourhood (toroidal wrap
// applied by the caller).  Separable like the 2 bpp walk: per pixel row the three block columns are blended vertically,
// V = 4 ((4 - yw) top + yw bottom), then each half row walks P(xw + 1) = P(xw) + 4 (VR - VL) from P = 8 (VL + VR) (x = 0, 1:
// left | centre, xw = 2, 3) or P = 16 VL (x = 2, 3: centre | right, xw = 0, 1) -- P = 256 x colour on 16-bit lanes
// (<= 65 280), so accumulate_mod's "take the high bytes" is the oracle's sum / 16.
ICAMD_DEV uint32_t pvrtc4_block_data(const uint32_t px[16], const PvrtcColors nb[3][3]) {
  uint32_t C[3][3][4];
  ICAMD_UNROLL
  for (int r = 0; r < 3; ++r)
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) {
      C[r][c][0] = pair_rb(nb[r][c].a); C[r][c][1] = pair_ga(nb[r][c].a);
      C[r][c][2] = pair_rb(nb[r][c].b); C[r][c][3] = pair_ga(nb[r][c].b);
    }
  uint32_t data = 0;
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    const int r0 = y < 2 ? 0 : 1;
    const uint32_t yw = (uint32_t)((y + 2) & 3);
    uint32_t V[3][4];
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c)
      ICAMD_UNROLL
      for (int v = 0; v < 4; ++v) V[c][v] = vblend_pair(yw, C[r0][c][v], C[r0 + 1][c][v]) >> 1;  // 8 x blend -> 4 x blend
    uint32_t acc = 0;
    ICAMD_UNROLL
    for (int h = 0; h < 2; ++h) {
      uint32_t P[4], D[4];
      ICAMD_UNROLL
      for (int v = 0; v < 4; ++v) {
        const uint32_t vl = V[h][v], vr = V[h + 1][v];
        D[v] = (vr - vl) << 2;
        P[v] = h == 0 ? (vl + vr) << 3 : vl << 4;
      }
      acc = opaque(accumulate_mod(px[4 * y + 2 * h], P, 1u << (16 * h), acc));
      ICAMD_UNROLL
      for (int v = 0; v < 4; ++v) P[v] += D[v];
      acc = opaque(accumulate_mod(px[4 * y + 2 * h + 1], P, 1u << (16 * h + 8), acc));
    }
    data |= udot4(acc, 0x40100401u, 0u) << (8 * y);  // bytes (values 0..3) -> four 2-bit fields
  }
  return data;
}

// One-pass form of the 4 bpp encoder (r05), the 2 bpp walk of pvrtc_onepass_strip with 4-pixel rows: one lane = one 4-pixel
// block column of a strip of K blocks.  The vertical structure is the 2 bpp one (blocks are 4 rows tall in both formats: rows
// 2, 3 of block s-1 and rows 0, 1 of block s interpolate between colour rows s-1 and s with weights 0, 1, 2, 3), so a tick
// again hands over pixel row m for the morph and row m - 5 for the modulation.  What falls away: the mode decision and its
// neighbour terms (every pixel's value is stored), hence no deferred finish and no column exchange -- block s-1 is complete
// after its row 3 in segment s.
//   tick(m, mp[4], ep[4]); lookup10 as in pvrtc_keys_finish (indices 0..15); exchange(s, own, left, right): colours only;
//   store(j, data, own).
template <int Q>
ICAMD_DEV void pvrtc4_keys_row(PvrtcMorphKeys &k, const uint32_t px[4]) {
  ICAMD_UNROLL
  for (int x = 0; x < 4; x += 2) {
    uint32_t kl[2];
    ICAMD_UNROLL
    for (int q = 0; q < 2; ++q) {
      const int p = 4 * Q + x + q;
      const uint32_t c = px[x + q], i = (uint32_t)(p & 3);
      const uint32_t idx4 = (uint32_t)(p & ~3) * 0x01010101u + 0x03020100u;
      kl[q] = perm(udot4(c, 0x001c964du, 0u), idx4, 0x0c0c0500u | i);
      const uint32_t k_rb = perm(c, idx4, 0x06000400u | i | i << 16), k_ga = perm(c, idx4, 0x07000500u | i | i << 16);
      k.min_rb = p == 0 ? k_rb : pk_min_u16(k.min_rb, k_rb);
      k.min_ga = p == 0 ? k_ga : pk_min_u16(k.min_ga, k_ga);
      pvrtc_keys_max_step<16>(k, p, k_rb, k_ga);
    }
    const int p = 4 * Q + x;
    k.min_l = p == 0 ? umin(kl[0], kl[1]) : umin3(k.min_l, kl[0], kl[1]);
    k.max_l = p == 0 ? umax(kl[0] + 15u, kl[1] + 13u)
                     : umax3(k.max_l, kl[0] + (uint32_t)(15 - 2 * p), kl[1] + (uint32_t)(15 - 2 * (p + 1)));
  }
  pvrtc_keys_opaque(k);
  ICAMD_SCHED_FENCE();
}
template <typename Lookup10>
ICAMD_DEV void pvrtc4_keys_finish(const PvrtcMorphKeys &k, uint32_t image0, Lookup10 &lookup10, uint32_t &col_a, uint32_t &col_b) {
  uint32_t max_rb, max_ga;
  pvrtc_keys_max_words<16>(k, max_rb, max_ga);
  const uint32_t kmin[5] = { k.min_l, k.min_rb & 0xffffu, k.min_ga & 0xffffu, k.min_rb >> 16, k.min_ga >> 16 };
  const uint32_t kmax[5] = { k.max_l, max_rb & 0xffffu, max_ga & 0xffffu, max_rb >> 16, max_ga >> 16 };
  uint32_t idx[10], v[10];
  ICAMD_UNROLL
  for (int i = 0; i < 5; ++i) {
    idx[2 * i] = kmin[i] & 15u;
    idx[2 * i + 1] = 15u - (kmax[i] & 15u);
  }
  lookup10(idx, v);
  uint32_t best_diff = 0, best_lo = 0, best_hi = 0;
  ICAMD_UNROLL
  for (int i = 0; i < 5; ++i) {
    const uint32_t lo = v[2 * i];
    const uint32_t hi = (kmax[i] >> 8) == 0u ? image0 : v[2 * i + 1];
    const uint32_t d = sad_u8(lo, hi, 0u);
    const bool better = (i == 0) || d > best_diff;
    best_lo = better ? lo : best_lo;
    best_hi = better ? hi : best_hi;
    best_diff = better ? d : best_diff;
  }
  const bool swap = udot4(best_hi, 0x01010101u, 0u) < udot4(best_lo, 0x01010101u, 0u);
  col_a = swap ? best_hi : best_lo;
  col_b = swap ? best_lo : best_hi;
}
// the four values of one pixel row as the row's 8 data bits (pixel x at bits 2 x); the bases as 64-bit pairs (see pvrtc_row_mods_pd64)
ICAMD_DEV uint32_t pvrtc4_row_bits64(const icamd_u64 P0[2], const icamd_u64 D0[2], const icamd_u64 P1[2], const icamd_u64 D1[2],
                                     const uint32_t px[4]) {
  // (one-pixel scans here: at this kernel's four waves per SIMD the compare / select chain is the cheaper one -- the two-pixel
  // form of pvrtc_row_mods_pd64 measured 0.4167 -> 0.4244 ms on 16 x 4096^2)
  uint32_t acc = 0;
  ICAMD_UNROLL
  for (int h = 0; h < 2; ++h) {
    const icamd_u64 *Pb = h ? P1 : P0, *D = h ? D1 : D0;
    icamd_u64 Q[2] = { Pb[0], Pb[1] };
    ICAMD_UNROLL
    for (int j = 0; j < 2; ++j) {
      const uint32_t P[4] = { lo32(Q[0]), hi32(Q[0]), lo32(Q[1]), hi32(Q[1]) };
      acc = opaque(accumulate_mod(px[2 * h + j], P, 1u << (16 * h + 8 * j), acc));
      ICAMD_SCHED_FENCE();
      if (j == 0) {
        Q[0] = add64(Q[0], D[0]);
        Q[1] = add64(Q[1], D[1]);
      }
    }
  }
  return udot4(acc, 0x40100401u, 0u);
}
template <typename Tick, typename Lookup10, typename Exchange, typename BlockStore>
ICAMD_DEV void pvrtc4_onepass_strip(uint32_t k_blocks, uint32_t image0, Tick &tick, Lookup10 &lookup10, Exchange &exchange,
                                    BlockStore &store) {
  const int K = (int)k_blocks;
  PvrtcMorphKeys keys;
  pvrtc_keys_reset(keys);
  uint32_t mp[4], ep[4];
  uint32_t A[3][4];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c)
    ICAMD_UNROLL
    for (int v = 0; v < 4; ++v) A[c][v] = 0u;
  uint32_t data = 0u;
  PvrtcColors own_acc = { 0u, 0u };
  tick(-4, mp, ep); pvrtc4_keys_row<0>(keys, mp);
  tick(-3, mp, ep); pvrtc4_keys_row<1>(keys, mp);
  tick(-2, mp, ep); pvrtc4_keys_row<2>(keys, mp);
  PvrtcColors cc[3] = { { 0u, 0u }, { 0u, 0u }, { 0u, 0u } };
  icamd_u64 P0[2] = { 0u, 0u }, D0[2] = { 0u, 0u }, P1[2] = { 0u, 0u }, D1[2] = { 0u, 0u };  // the walks' bases, carried
  ICAMD_NOUNROLL
  for (int s = -1;; ++s) {
    {
      tick(4 * s + 3, mp, ep);
      pvrtc4_keys_row<3>(keys, mp);
      uint32_t a, c;
      pvrtc4_keys_finish(keys, image0, lookup10, a, c);
      cc[1].a = channel_reduce(a, false);
      cc[1].b = channel_reduce(c, true);
      pvrtc_keys_reset(keys);
    }
    exchange(s, cc[1], cc[0], cc[2]);
    // colour rows (s-1, s): V = 16 A + w * 4 (B - A) for weight w = 0..3; from it the walks' bases and their steps per pixel row:
    //   x = 0, 1: D = 4 (V[1] - V[0]), P = 8 (V[0] + V[1]);   x = 2, 3: D = 4 (V[2] - V[1]), P = 16 V[1]
    // (the bases are carried and stepped a fourth time at the end of the segment, the steps come straight from E = B - A: see
    // pvrtc_onepass_strip; here D = 64 (A1 - A0), P = 128 (A0 + A1) | D = 64 (A2 - A1), P = 256 A1)
    icamd_u64 dP0[2], dD0[2], dP1[2], dD1[2];
    {
      uint32_t ep0[4], ed0[4], ep1[4], ed1[4];
      ICAMD_UNROLL
      for (int v = 0; v < 4; ++v) {
        uint32_t e[3];
        ICAMD_UNROLL
        for (int c = 0; c < 3; ++c) {
          const uint32_t b = v == 0 ? pair_rb(cc[c].a) : v == 1 ? pair_ga(cc[c].a) : v == 2 ? pair_rb(cc[c].b) : pair_ga(cc[c].b);
          e[c] = b - A[c][v];
          A[c][v] = b;
        }
        ed0[v] = (e[1] - e[0]) << 4;
        ep0[v] = (e[0] + e[1]) << 5;
        ed1[v] = (e[2] - e[1]) << 4;
        ep1[v] = e[1] << 6;
      }
      ICAMD_UNROLL
      for (int p = 0; p < 2; ++p) {  // (signed steps: lanes of at most 16 320)
        dD0[p] = pack64_signed(ed0[2 * p], ed0[2 * p + 1]); dD1[p] = pack64_signed(ed1[2 * p], ed1[2 * p + 1]);
        dP0[p] = pack64_signed(ep0[2 * p], ep0[2 * p + 1]); dP1[p] = pack64_signed(ep1[2 * p], ep1[2 * p + 1]);
      }
    }
#define ICAMD_ROW4_STEP()                                                                                    \
  ICAMD_UNROLL                                                                                               \
  for (int p = 0; p < 2; ++p) {                                                                              \
    P0[p] = add64(P0[p], dP0[p]); D0[p] = add64(D0[p], dD0[p]);                                              \
    P1[p] = add64(P1[p], dP1[p]); D1[p] = add64(D1[p], dD1[p]);                                              \
  }
    if (s >= 1) data |= pvrtc4_row_bits64(P0, D0, P1, D1, ep) << 16;  // row 2 of block s-1, weight 0
    ICAMD_ROW4_STEP()
    tick(4 * s + 4, mp, ep);
    pvrtc4_keys_row<0>(keys, mp);
    if (s >= 1) {  // row 3 of block s-1, weight 1: the block is complete
      data |= pvrtc4_row_bits64(P0, D0, P1, D1, ep) << 24;
      store((uint32_t)(s - 1), data, own_acc);
    }
    if (s == K) break;
    ICAMD_ROW4_STEP()
    tick(4 * s + 5, mp, ep);
    pvrtc4_keys_row<1>(keys, mp);
    if (s >= 0) {  // row 0 of block s, weight 2
      own_acc = cc[1];
      data = pvrtc4_row_bits64(P0, D0, P1, D1, ep);
    }
    ICAMD_ROW4_STEP()
    tick(4 * s + 6, mp, ep);
    pvrtc4_keys_row<2>(keys, mp);
    if (s >= 0) data |= pvrtc4_row_bits64(P0, D0, P1, D1, ep) << 8;  // row 1 of block s, weight 3
    ICAMD_ROW4_STEP()  // weight 4 = colour row s itself = the next segment's weight 0
#undef ICAMD_ROW4_STEP
  }
}

}  // namespace icamd
#endif  // ICAMD_PVRTC4_BLOCK_H_
