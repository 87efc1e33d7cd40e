// pvrtc_onepass.h -- PVRTC1 2 bpp, the one-pass strip: the lane that encodes a block column also morphs it, row by row, the
// modulation on the 64-bit walk.  Part of pvrtc_block.h.
#ifndef ICAMD_PVRTC_ONEPASS_H_
#define ICAMD_PVRTC_ONEPASS_H_

#include "pvrtc_walk.h"
#include "pvrtc_pair.h"

namespace icamd {

// ---- one-pass form (r05): the lane that encodes a block column also MORPHS it ----------------------------------------
// GetExtremesFast (pvrtc.cc:255-329) consumed one pixel row at a time: the same keys as pvrtc_extremes, the block's four
// rows arriving in four calls (Q = row inside the block, compile-time), the ten data-dependent pixel look-ups of the final
// scan batched into one call of `lookup10` (on the device: ten ds_read_b32 from the pixel-row ring under one wait).
// The (rb, ga) "first maximum" keys as ONE running pair (r06).  The plain form is max over pixels p of k_p + up_p with
// up_p = (N - 1 - 2 p) per 16-bit lane (N = 32 or 16 pixels): two word adds per pixel.  With M_p = (that maximum up to p) - up_p,
//   M_0 = k_0,   M_p = max(M_(p-1) + 2, k_p)   per lane,
// the SAME constant is added every time, to the running value instead of the new key -- so (M_rb, M_ga) steps as a 64-bit pair
// with one v_lshl_add_u64 (see "the walk on 64-bit register pairs": at two waves per SIMD 4.4 clocks against 2 x 3.5).  Lanes
// stay in 0 .. 65 280 + 2 N: M_p >= k_p >= 0 and the maximum is at most 65 280 + N - 1.  The keys the scan reads are
// M_(N-1) + up_(N-1) = M - (N - 1) per lane (pvrtc_keys_max_words).
struct PvrtcMorphKeys {
  uint32_t min_l, max_l, min_rb, min_ga;
  icamd_u64 max_pair;  // M_rb | M_ga << 32; first assigned by pixel 0 of a block
};
ICAMD_DEV void pvrtc_keys_reset(PvrtcMorphKeys &k) {
  k.min_l = k.min_rb = k.min_ga = 0xffffffffu;
  k.max_l = 0u;
  k.max_pair = 0u;
}
// one pixel's (rb, ga) keys into the running maxima; P = pixel index in the block (compile-time after unrolling), N = pixels
template <int N>
ICAMD_DEV void pvrtc_keys_max_step(PvrtcMorphKeys &k, int P, uint32_t k_rb, uint32_t k_ga) {
  if (P == 0) {
    k.max_pair = pack64(k_rb, k_ga);
  } else {
    const icamd_u64 m = add64(k.max_pair, pack64(0x00020002u, 0x00020002u));
    k.max_pair = pack64(pk_max_u16(lo32(m), k_rb), pk_max_u16(hi32(m), k_ga));
  }
}
template <int N>
ICAMD_DEV void pvrtc_keys_max_words(const PvrtcMorphKeys &k, uint32_t &max_rb, uint32_t &max_ga) {
  max_rb = lo32(k.max_pair) - (uint32_t)(N - 1) * 0x00010001u;
  max_ga = hi32(k.max_pair) - (uint32_t)(N - 1) * 0x00010001u;
}
ICAMD_DEV void pvrtc_keys_opaque(PvrtcMorphKeys &k) {
  k.min_l = opaque(k.min_l); k.max_l = opaque(k.max_l);
  k.min_rb = opaque(k.min_rb); k.min_ga = opaque(k.min_ga);
  k.max_pair = opaque64(k.max_pair);
}
template <int Q>
ICAMD_DEV void pvrtc_keys_row(PvrtcMorphKeys &k, const uint32_t px[8]) {
  ICAMD_UNROLL
  for (int x = 0; x < 8; x += 2) {
    uint32_t kl[2];
    ICAMD_UNROLL
    for (int q = 0; q < 2; ++q) {
      const int p = 8 * Q + x + q;
      const uint32_t c = px[x + q], i = (uint32_t)(p & 3);
      const uint32_t idx4 = (uint32_t)(p & ~3) * 0x01010101u + 0x03020100u;
      kl[q] = perm(udot4(c, 0x001c964du, 0u), idx4, 0x0c0c0500u | i);
      const uint32_t k_rb = perm(c, idx4, 0x06000400u | i | i << 16);
      const uint32_t k_ga = perm(c, idx4, 0x07000500u | i | i << 16);
      // (pixel 0 of a block ASSIGNS the running keys: the reset values -- all ones / zero -- never win against a key)
      k.min_rb = p == 0 ? k_rb : pk_min_u16(k.min_rb, k_rb);
      k.min_ga = p == 0 ? k_ga : pk_min_u16(k.min_ga, k_ga);
      pvrtc_keys_max_step<32>(k, p, k_rb, k_ga);
    }
    const int p = 8 * Q + x;
    k.min_l = p == 0 ? umin(kl[0], kl[1]) : umin3(k.min_l, kl[0], kl[1]);
    k.max_l = p == 0 ? umax(kl[0] + 31u, kl[1] + 29u)
                     : umax3(k.max_l, kl[0] + (uint32_t)(31 - 2 * p), kl[1] + (uint32_t)(31 - 2 * (p + 1)));
  }
  pvrtc_keys_opaque(k);
  ICAMD_SCHED_FENCE();
}
// lookup10(idx[10], out[10]): out[i] = pixel idx[i] (0..31, raster inside the block) of the block whose rows were just consumed
template <typename Lookup10>
ICAMD_DEV void pvrtc_keys_finish(const PvrtcMorphKeys &k, uint32_t image0, Lookup10 &lookup10, uint32_t &col_a, uint32_t &col_b) {
  uint32_t max_rb, max_ga;
  pvrtc_keys_max_words<32>(k, max_rb, max_ga);
  const uint32_t kmin[5] = { k.min_l, k.min_rb & 0xffffu, k.min_ga & 0xffffu, k.min_rb >> 16, k.min_ga >> 16 };
  const uint32_t kmax[5] = { k.max_l, max_rb & 0xffffu, max_ga & 0xffffu, max_rb >> 16, max_ga >> 16 };
  uint32_t idx[10], v[10];
  ICAMD_UNROLL
  for (int i = 0; i < 5; ++i) {
    idx[2 * i] = kmin[i] & 31u;
    idx[2 * i + 1] = 31u - (kmax[i] & 31u);
  }
  lookup10(idx, v);
  uint32_t best_diff = 0, best_lo = 0, best_hi = 0;
  ICAMD_UNROLL
  for (int i = 0; i < 5; ++i) {
    const uint32_t lo = v[2 * i];
    const uint32_t hi = (kmax[i] >> 8) == 0u ? image0 : v[2 * i + 1];  // never-updated max -> image pixel 0 (pvrtc.cc:268-269)
    const uint32_t d = sad_u8(lo, hi, 0u);
    const bool better = (i == 0) || d > best_diff;
    best_lo = better ? lo : best_lo;
    best_hi = better ? hi : best_hi;
    best_diff = better ? d : best_diff;
  }
  const uint32_t s_lo = udot4(best_lo, 0x01010101u, 0u), s_hi = udot4(best_hi, 0x01010101u, 0u);
  const bool swap = s_hi < s_lo;
  col_a = swap ? best_hi : best_lo;
  col_b = swap ? best_lo : best_hi;
}

// One lane = one block column of a strip of K blocks (block rows 0 .. K-1 of the strip), walking pixel rows -4 .. 4 K + 3:
// every row is consumed twice from the same row ring -- by the morph when it arrives (row m) and by the modulation five
// rows later (row e = m - 5): rows 2, 3 of block s-1 and rows 0, 1 of block s interpolate between colour rows s-1 and s
// (pvrtc.cc:216-227), so block s must be morphed (its last row is 4 s + 3) before row 4 s - 2 is modulated.  A "tick"
// hands over both rows.  Per SEGMENT s = -1 .. K+1 (four ticks):
//   tick(4 s + 3):  last row of block s -> its two colours;  exchange(): the colours of the block columns left and right
//                   (neighbour lanes; on the device wave-edge lanes go through LDS, which is where the workgroup's one
//                   barrier per segment sits) and, riding on the same barrier, the column-0 modulation values of the block
//                   right of block s-2 -- which is why a block is finished one segment late (block j in segment j+2):
//                   its last term  sum_y |m(7, y) - m(8, y)|  (pvrtc.cc:426-429) needs the right-hand lane's values;
//   rows 4 s - 2, 4 s - 1 (block s-1 rows 2, 3), 4 s (block s row 0, closes block s-1's vertical differences), 4 s + 1.
// tick(m, mp, ep):       pixel rows m (morph) and m - 5 (modulation) of the strip; wrap and clamping are the caller's.
// lookup10(idx, out):    see pvrtc_keys_finish; refers to the block whose last row the latest tick delivered.
// exchange(s, own, col0, left, right, right_col0): own = colours of block row s of this column, col0 = this lane's column-0
//                        values of block s-2; returns the colours left / right of `own` and the column-0 values of the block
//                        right of block s-2.
// store(j, data, one_bpp, own): block j of the strip is finished.
// K must be >= 1; segments -1 and K+1 only morph / only finish.
template <typename Tick, typename Lookup10, typename Exchange, typename BlockStore>
ICAMD_DEV void pvrtc_onepass_strip(uint32_t k_blocks, uint32_t image0, Tick &tick, Lookup10 &lookup10, Exchange &exchange,
                                   BlockStore &store) {
  const int K = (int)k_blocks;
  PvrtcMorphKeys keys;
  pvrtc_keys_reset(keys);
  uint32_t mp[8], ep[8];
  uint32_t A[3][4];  // colour row s-1 as channel pairs
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c)
    ICAMD_UNROLL
    for (int v = 0; v < 4; ++v) A[c][v] = 0u;
  PvrtcBlockAcc acc = { 0, 0, 0, 0, 0, 0, 0, 0 }, def = { 0, 0, 0, 0, 0, 0, 0, 0 };
  PvrtcColors own_acc = { 0u, 0u }, own_def = { 0u, 0u };
  uint32_t prev[2] = { 0u, 0u };
  tick(-4, mp, ep); pvrtc_keys_row<0>(keys, mp);
  tick(-3, mp, ep); pvrtc_keys_row<1>(keys, mp);
  tick(-2, mp, ep); pvrtc_keys_row<2>(keys, mp);
  PvrtcColors cc[3] = { { 0u, 0u }, { 0u, 0u }, { 0u, 0u } };
  icamd_u64 P0[2] = { 0u, 0u }, D0[2] = { 0u, 0u }, P1[2] = { 0u, 0u }, D1[2] = { 0u, 0u };  // the walks' bases, carried
  ICAMD_NOUNROLL
  for (int s = -1;; ++s) {
    if (s <= K) {
      tick(4 * s + 3, mp, ep);
      pvrtc_keys_row<3>(keys, mp);
      uint32_t a, c;
      pvrtc_keys_finish(keys, image0, lookup10, a, c);
      cc[1].a = channel_reduce(a, false);
      cc[1].b = channel_reduce(c, true);
      pvrtc_keys_reset(keys);
    }
    uint32_t right_col0 = 0u;
    exchange(s, cc[1], def.col0, cc[0], cc[2], right_col0);
    if (s >= 2) {
      def.vc = sad_u8(def.col7, right_col0, def.vc);  // sum_y |m(7, y) - m(8, y)|
      bool one_bpp;
      const uint32_t data = pvrtc_acc_finish(def, &one_bpp);
      store((uint32_t)(s - 2), data, one_bpp, own_def);
    }
    if (s > K) break;
    // colour rows (s-1, s): V = 32 A, dV = 8 (B - A) -- see pvrtc_encode_strip
    // The bases of the horizontal walks and their steps per pixel row, straight from the colour rows A (s-1) and B (s), E = B - A:
    //   left half row:  D = V[1] - V[0] = 32 (A1 - A0),  P = 4 (V[0] + V[1]) = 128 (A0 + A1);   per row + 8 (E1 - E0), + 32 (E0 + E1)
    //   right half row: D = V[2] - V[1] = 32 (A2 - A1),  P = 8 V[1] = 256 A1;                   per row + 8 (E2 - E1), + 64 E1
    // (sums / shifts commute modulo 2^32: the same words as deriving them from V and dV, 15 instead of 19 instructions per
    // channel pair), then as 64-bit pairs (pvrtc_row_mods_pd64) made exact modulo 2^64: the steps are SIGNED quantities below
    // 2^31 in magnitude per word (lanes of at most 16 320), so the pair's high word owes the low word's sign --
    // hi + (lo >> 31, arithmetic); the P bases have non-negative lanes and need nothing.
    // The bases themselves are CARRIED from segment to segment: four row steps lead from colour row s-1 to colour row s, so
    // a fourth row step at the end of the segment leaves exactly the next segment's bases (32 (B1 - B0) = 32 (A1 - A0)
    // + 4 * 8 (E1 - E0), ...; zero before the first segment, like A) -- 8 pair adds instead of deriving them from A again.
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
        ed0[v] = (e[1] - e[0]) << 3;
        ep0[v] = (e[0] + e[1]) << 5;
        ed1[v] = (e[2] - e[1]) << 3;
        ep1[v] = e[1] << 6;
      }
      ICAMD_UNROLL
      for (int p = 0; p < 2; ++p) {
        dD0[p] = pack64_signed(ed0[2 * p], ed0[2 * p + 1]); dD1[p] = pack64_signed(ed1[2 * p], ed1[2 * p + 1]);
        dP0[p] = pack64_signed(ep0[2 * p], ep0[2 * p + 1]); dP1[p] = pack64_signed(ep1[2 * p], ep1[2 * p + 1]);
      }
    }
#define ICAMD_ROW_STEP()                                                                                     \
  ICAMD_UNROLL                                                                                               \
  for (int p = 0; p < 2; ++p) {                                                                              \
    P0[p] = add64(P0[p], dP0[p]); D0[p] = add64(D0[p], dD0[p]);                                              \
    P1[p] = add64(P1[p], dP1[p]); D1[p] = add64(D1[p], dD1[p]);                                              \
  }
    uint32_t row[2];
    if (s >= 1) {  // row 2 of block s-1, weight 0
      pvrtc_row_mods_pd64(P0, D0, P1, D1, ep, row);
      acc.hc = sad_u8(prev[0], row[0], acc.hc);  // "horizontal_count" = sum |m - m(x, y+1)| (pvrtc.cc:426-429)
      acc.hc = sad_u8(prev[1], row[1], acc.hc);
      pvrtc_acc_row<true>(acc, 2, row, 0u);
      prev[0] = row[0]; prev[1] = row[1];
    }
    ICAMD_ROW_STEP()
    ICAMD_SCHED_FENCE();
    tick(4 * s + 4, mp, ep);
    pvrtc_keys_row<0>(keys, mp);
    if (s >= 1) {  // row 3 of block s-1, weight 1
      pvrtc_row_mods_pd64(P0, D0, P1, D1, ep, row);
      acc.hc = sad_u8(prev[0], row[0], acc.hc);
      acc.hc = sad_u8(prev[1], row[1], acc.hc);
      pvrtc_acc_row<true>(acc, 3, row, 0u);
      prev[0] = row[0]; prev[1] = row[1];
    }
    ICAMD_ROW_STEP()
    ICAMD_SCHED_FENCE();
    tick(4 * s + 5, mp, ep);
    pvrtc_keys_row<1>(keys, mp);
    if (s >= 0) {  // row 0 of block s, weight 2 -- for s == K the row below the strip, which only completes block K-1
      pvrtc_row_mods_pd64(P0, D0, P1, D1, ep, row);
      if (s >= 1) {
        acc.hc = sad_u8(prev[0], row[0], acc.hc);
        acc.hc = sad_u8(prev[1], row[1], acc.hc);
        def = acc;  // complete but for the right-hand column: finished in the next segment
        own_def = own_acc;
      }
      own_acc = cc[1];
      acc.hc = acc.vc = acc.d1 = acc.d2 = 0u;
      pvrtc_acc_row<true>(acc, 0, row, 0u);
      prev[0] = row[0]; prev[1] = row[1];
    }
    ICAMD_ROW_STEP()
    ICAMD_SCHED_FENCE();
    tick(4 * s + 6, mp, ep);
    pvrtc_keys_row<2>(keys, mp);
    if (s >= 0 && s < K) {  // row 1 of block s, weight 3
      pvrtc_row_mods_pd64(P0, D0, P1, D1, ep, row);
      acc.hc = sad_u8(prev[0], row[0], acc.hc);
      acc.hc = sad_u8(prev[1], row[1], acc.hc);
      pvrtc_acc_row<true>(acc, 1, row, 0u);
      prev[0] = row[0]; prev[1] = row[1];
    }
    ICAMD_ROW_STEP()  // weight 4 = colour row s itself = the next segment's weight 0
    ICAMD_SCHED_FENCE();
  }
}
#undef ICAMD_ROW_STEP

}  // namespace icamd
#endif  // ICAMD_PVRTC_ONEPASS_H_
