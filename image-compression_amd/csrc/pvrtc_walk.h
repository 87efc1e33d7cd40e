// pvrtc_walk.h -- the horizontal walk of a pixel row on 64-bit register pairs (one-pass kernels).  Part of pvrtc_block.h.
#ifndef ICAMD_PVRTC_WALK_H_
#define ICAMD_PVRTC_WALK_H_

#include "pvrtc_pixel.h"

namespace icamd {

// ---- the walk on 64-bit register pairs (r06) ----------------------------------------------------------------------------
// The four sums of a walk are two (rb, ga) word pairs; as ONE 64-bit integer each -- word v at bits 32 (v & 1) -- a pair steps
// with one v_lshl_add_u64 (4.4 clocks at two waves per SIMD against 2 x 3.5 for two v_add_u32 next to half-rate instructions:
// scripts/ubench_u64.hip).  Exact: every quantity of the walk is a LINEAR function of the colours, 16-bit lanes of a word may be
// negative on the way (steps, differences), so the whole chain is computed modulo 2^64 -- borrows cross the word boundary exactly
// as they cross the lane boundary inside a word in the 32-bit form -- and the values that are READ (the sums at the pixels) have
// all four lanes in 0 .. 65 280, so their words are the 32-bit form's words.
// (A/B against the walk on 32-bit words: profiles/r06_ab_pvrtc_walk64.log, 16 x 4096^2 0.3887 -> 0.3769 ms.)
typedef unsigned long long icamd_u64;
#if defined(ICAMD_HOST_EMULATION)
ICAMD_DEV icamd_u64 pack64(uint32_t lo, uint32_t hi) { return (icamd_u64)hi << 32 | lo; }
ICAMD_DEV uint32_t lo32(icamd_u64 v) { return (uint32_t)v; }
ICAMD_DEV uint32_t hi32(icamd_u64 v) { return (uint32_t)(v >> 32); }
#else
// (as a two-element vector: hipcc then keeps the pair in one aligned register pair whose halves are written in place; the
// shift-and-or form is canonicalised to zext(lo) + (hi << 32) and a pair add becomes v_lshl_add_u64 + v_add_u32)
typedef uint32_t icamd_u32x2 __attribute__((ext_vector_type(2)));
ICAMD_DEV icamd_u64 pack64(uint32_t lo, uint32_t hi) {
  const icamd_u32x2 v = { lo, hi };
  return __builtin_bit_cast(icamd_u64, v);
}
ICAMD_DEV uint32_t lo32(icamd_u64 v) { return __builtin_bit_cast(icamd_u32x2, v).x; }
ICAMD_DEV uint32_t hi32(icamd_u64 v) { return __builtin_bit_cast(icamd_u32x2, v).y; }
#endif
// the pair of two SIGNED words (each below 2^31 in magnitude, given modulo 2^32) as hi * 2^32 + lo modulo 2^64
ICAMD_DEV icamd_u64 pack64_signed(uint32_t lo, uint32_t hi) { return pack64(lo, hi + (uint32_t)((int32_t)lo >> 31)); }
template <int S>
ICAMD_DEV icamd_u64 shl_add64(icamd_u64 a, icamd_u64 b) {  // (a << S) + b, S = 0 .. 4
  static_assert(S >= 0 && S <= 4, "v_lshl_add_u64 shifts by at most 4");
  return (a << S) + b;  // (hipcc selects v_lshl_add_u64 for it on gfx950 and, unlike after an asm, knows which hazards it has)
}
ICAMD_DEV icamd_u64 add64(icamd_u64 a, icamd_u64 b) { return shl_add64<0>(a, b); }
ICAMD_DEV icamd_u64 opaque64(icamd_u64 v) {
#if !defined(ICAMD_HOST_EMULATION)
  asm volatile("" : "+v"(v));
#endif
  return v;
}
// pvrtc_row_mods_v from the walk's own bases (one-pass kernel, r05): P0 / D0 = first value and step of the left half row
// (x_in 0..3, sources left | centre), P1 / D1 of the right half row (centre | right), as pairs: P*[p] = words (2 p, 2 p + 1).
// Both are linear in the vertical weight, so the strip walk steps THEM from pixel row to pixel row instead of stepping the
// three column blends and re-deriving P and D in every row.  The bases are left untouched.
ICAMD_DEV void pvrtc_row_mods_pd64(const icamd_u64 P0[2], const icamd_u64 D0[2], const icamd_u64 P1[2], const icamd_u64 D1[2],
                                   const uint32_t *pixels, uint32_t row[2]) {
  ICAMD_UNROLL
  for (int h = 0; h < 2; ++h) {
    const icamd_u64 *Pb = h ? P1 : P0, *D = h ? D1 : D0;
    icamd_u64 Q[2] = { Pb[0], Pb[1] };
    // pixels (0, 2) and (1, 3) of the half row share their scans: the values land in bytes 0, 2 of one word and, shifted, 1, 3
    uint32_t d[2][4], val[2] = { 0u, 0u };
    ICAMD_UNROLL
    for (int j = 0; j < 4; ++j) {
      const uint32_t P[4] = { lo32(Q[0]), hi32(Q[0]), lo32(Q[1]), hi32(Q[1]) };
      uint32_t c[4];
      modulation_colours(P, c);
      const uint32_t px = pixels[4 * h + j];
      ICAMD_UNROLL
      for (int k = 0; k < 4; ++k) d[j & 1][k] = j < 2 ? sad_u8(px, c[k], 0u) : sad_hi_u8(px, c[k], d[j & 1][k]);
      if (j >= 2) val[j & 1] = opaque(scan_pair(d[j & 1]));
      else {
        ICAMD_UNROLL
        for (int k = 0; k < 4; ++k) d[j][k] = opaque(d[j][k]);
      }
      ICAMD_SCHED_FENCE();
      if (j < 3) {
        Q[0] = add64(Q[0], D[0]);
        Q[1] = add64(Q[1], D[1]);
      }
    }
    row[h] = val[0] | val[1] << 8;
  }
}

}  // namespace icamd
#endif  // ICAMD_PVRTC_WALK_H_
