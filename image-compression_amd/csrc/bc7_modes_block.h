// bc7_modes_block.h -- BC7 with the opt-in mode-1 and mode-5 candidates (EXTENSION, include/ic_amd.h ICAMD_BC7_MODES_EXTENDED;
// DESIGN.md 3.22).  The definition is stated in include/ic_amd.h and restated in tests/bc7_modes_oracle.py.  One block per lane,
// everything in registers, integer only.  The mode-6 block is encode_bc7's (bc7_block.h, untouched); its sse is measured from
// the written bits (bc7_mode6_sse: sixteen interpolations, three dot products each), so the encoder's code stays as it is.
//
// The sub-fit F of the definition is bc7_subfit<NCH, IBITS, Q>: the texels arrive with the channels outside C already cleared
// (bytes NCH..3 zero), so the dot-product distance of bc7_search carries over to the 8- and 4-entry palettes unchanged; the
// texel set S is a 16-bit mask per lane.  The opaque / non-opaque choice, the det = 0 skips, the refit's acceptance and the
// "sse6 == 0: nothing can be strictly closer" return are per-lane branches; there is no wave-uniform shortcut.
#ifndef ICAMD_BC7_MODES_BLOCK_H_
#define ICAMD_BC7_MODES_BLOCK_H_

#include "bc7_block.h"

#if defined(ICAMD_HOST_EMULATION)
#define ICAMD_BC7_NOUNROLL
#else
#define ICAMD_BC7_NOUNROLL _Pragma("nounroll")
#endif

namespace icamd {

enum { kBc7Q1 = 0, kBc7Q5 = 1, kBc7QIdentity = 2 };

// The sse over four channels of the mode-6 block w (as encode_bc7 wrote it) against the texels v.
ICAMD_DEV uint32_t bc7_mode6_sse(const uint32_t v[16], const uint32_t w[4]) {
  const uint64_t lo = (uint64_t)w[0] | (uint64_t)w[1] << 32, hi = (uint64_t)w[2] | (uint64_t)w[3] << 32;
  uint32_t E0 = (uint32_t)(lo >> 63) * 0x01010101u, E1 = ((uint32_t)hi & 1u) * 0x01010101u;
  ICAMD_UNROLL
  for (int c = 0; c < 4; ++c) {
    E0 |= ((uint32_t)(lo >> (7 + 14 * c)) & 127u) << (8 * c + 1);
    E1 |= ((uint32_t)(lo >> (14 + 14 * c)) & 127u) << (8 * c + 1);
  }
  const uint32_t rb0 = E0 & 0x00ff00ffu, ga0 = (E0 >> 8) & 0x00ff00ffu, rb1 = E1 & 0x00ff00ffu, ga1 = (E1 >> 8) & 0x00ff00ffu;
  uint32_t sse = 0;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint32_t k = p == 0 ? ((uint32_t)hi >> 1) & 7u : (uint32_t)(hi >> (4 * p)) & 15u;
    const uint32_t wt = bc7_weight4(k);
    const uint32_t rb = (((64u - wt) * rb0 + wt * rb1 + 0x00200020u) >> 6) & 0x00ff00ffu;
    const uint32_t ga = (((64u - wt) * ga0 + wt * ga1 + 0x00200020u) >> 6) & 0x00ff00ffu;
    const uint32_t pal = rb | ga << 8;
    sse += udot4(v[p], v[p], udot4(pal, pal, 0u)) - 2u * udot4(pal, v[p], 0u);
  }
  return sse;
}

// ---- the quantisers.  A 7-bit x decodes to e7(x) = (x << 1) | (x >> 6): 2 x below 64, 2 x + 1 from 64.  The nearest value of
// each half is a rounding; the lower half wins a tie between the halves (its x are the smaller ones).

// Q1, parity p: the allowed x = 2 q + p decode to 4 q + 2 p (q < 32) and 4 q + 2 p + 1 (q >= 32).  Returns the decoded byte.
ICAMD_DEV uint32_t bc7_near_parity(uint32_t T, uint32_t p) {
  const int32_t t = (int32_t)T - 2 * (int32_t)p;
  const uint32_t elo = 4u * (uint32_t)imin(imax((t + 1) >> 2, 0), 31) + 2u * p;
  const uint32_t ehi = 4u * (uint32_t)imin(imax(t >> 2, 32), 63) + 2u * p + 1u;
  const uint32_t dlo = elo > T ? elo - T : T - elo, dhi = ehi > T ? ehi - T : T - ehi;
  return dhi < dlo ? ehi : elo;
}
// Q5: x in 0..127 decode to 2 x (x < 64) and 2 x + 1 (x >= 64)
ICAMD_DEV uint32_t bc7_near7(uint32_t T) {
  const uint32_t elo = 2u * umin(T >> 1, 63u);
  const uint32_t ehi = 2u * (uint32_t)imin(imax(((int32_t)T - 1) >> 1, 64), 127) + 1u;
  const uint32_t dlo = elo > T ? elo - T : T - elo, dhi = ehi > T ? ehi - T : T - ehi;
  return dhi < dlo ? ehi : elo;
}

// Targets of both endpoints -> the decoded endpoint bytes (bytes NCH..3 zero)
template <int NCH, int Q>
ICAMD_DEV void bc7_quantise_pair(const uint32_t T0[4], const uint32_t T1[4], uint32_t &E0, uint32_t &E1) {
  if (Q == kBc7Q1) {
    uint32_t e0[2] = { 0u, 0u }, e1[2] = { 0u, 0u }, err[2] = { 0u, 0u };
    ICAMD_UNROLL
    for (uint32_t p = 0; p < 2; ++p)
      ICAMD_UNROLL
      for (int c = 0; c < NCH; ++c) {
        const uint32_t a = bc7_near_parity(T0[c], p), b = bc7_near_parity(T1[c], p);
        const int32_t da = (int32_t)a - (int32_t)T0[c], db = (int32_t)b - (int32_t)T1[c];
        err[p] += (uint32_t)(da * da + db * db);
        e0[p] |= a << (8 * c);
        e1[p] |= b << (8 * c);
      }
    const bool one = err[1] < err[0];
    E0 = one ? e0[1] : e0[0];
    E1 = one ? e1[1] : e1[0];
  } else {
    E0 = E1 = 0u;
    ICAMD_UNROLL
    for (int c = 0; c < NCH; ++c) {
      E0 |= (Q == kBc7Q5 ? bc7_near7(T0[c]) : T0[c]) << (8 * c);
      E1 |= (Q == kBc7Q5 ? bc7_near7(T1[c]) : T1[c]) << (8 * c);
    }
  }
}

// bc7_search for a palette of 1 << IBITS entries and the texels of `mask`: inv holds 15 - k_p in nibble p (every texel is
// searched; only those of the mask count towards the sse).
template <int NCH, int IBITS>
ICAMD_DEV uint32_t bc7_search_set(const uint32_t u[16], uint32_t mask, uint32_t E0, uint32_t E1, uint64_t &inv) {
  constexpr int NP = 1 << IBITS;
  const uint32_t rb0 = E0 & 0x00ff00ffu, ga0 = (E0 >> 8) & 0x00ff00ffu, rb1 = E1 & 0x00ff00ffu, ga1 = (E1 >> 8) & 0x00ff00ffu;
  uint32_t pal[NP], bias[NP];
  ICAMD_UNROLL
  for (uint32_t k = 0; k < (uint32_t)NP; ++k) {
    const uint32_t w = (k * 64u + (uint32_t)(NP - 1) / 2u) / (uint32_t)(NP - 1);  // (bc7_detail::weights_ok)
    pal[k] = (((64u - w) * rb0 + w * rb1 + 0x00200020u) >> 6) & 0x00ff00ffu;
    if (NCH > 1) pal[k] |= ((((64u - w) * ga0 + w * ga1 + 0x00200020u) >> 6) & 0x00ff00ffu) << 8;
    bias[k] = (((1u << 19) - udot4(pal[k], pal[k], 0u)) << 4) | (15u - k);
  }
  uint32_t sse = 0;
  inv = 0;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    uint32_t best = 0;
    ICAMD_UNROLL
    for (int k = 0; k < NP; ++k) best = umax(best, (udot4(pal[k], u[p], 0u) << 5) + bias[k]);
    inv |= (uint64_t)(best & 15u) << (4 * p);
    const uint32_t d = udot4(u[p], u[p], 1u << 19) - (best >> 4);
    sse += ((mask >> p) & 1u) ? d : 0u;
  }
  return sse;
}

struct Bc7Fit {
  uint32_t E0, E1, sse;
  uint64_t inv;  // 15 - k_p in nibble p
};

// F(S, C, weights, Q) of the definition: u = the texels with the channels outside C cleared, mask = S (not empty).
template <int NCH, int IBITS, int Q>
ICAMD_DEV Bc7Fit bc7_subfit(const uint32_t u[16], uint32_t mask) {
  const uint32_t n = (uint32_t)__builtin_popcount(mask);
  uint32_t lo[4] = { 0u, 0u, 0u, 0u }, hi[4] = { 0u, 0u, 0u, 0u }, sum[4] = { 0u, 0u, 0u, 0u };
  ICAMD_UNROLL
  for (int c = 0; c < NCH; ++c) {
    lo[c] = 255u;
    hi[c] = sum[c] = 0u;
    ICAMD_UNROLL
    for (int i = 0; i < 16; ++i) {
      const bool in = ((mask >> i) & 1u) != 0u;
      const uint32_t x = bc7_ch(u[i], c);
      lo[c] = umin(lo[c], in ? x : 255u);
      hi[c] = umax(hi[c], in ? x : 0u);
      sum[c] += in ? x : 0u;
    }
  }
  uint32_t cs = 0, widest = hi[0] - lo[0];
  ICAMD_UNROLL
  for (int c = 1; c < NCH; ++c)
    if (hi[c] - lo[c] > widest) {
      widest = hi[c] - lo[c];
      cs = (uint32_t)c;
    }
  uint32_t cross[4] = { 0u, 0u, 0u, 0u };
  if (NCH > 1) {
    ICAMD_UNROLL
    for (int i = 0; i < 16; ++i) {
      const uint32_t star = ((mask >> i) & 1u) ? (u[i] >> (8u * cs)) & 0xffu : 0u;
      ICAMD_UNROLL
      for (int c = 0; c < NCH; ++c) cross[c] += star * bc7_ch(u[i], c);
    }
  }
  const uint32_t sum_star = cs == 0u ? sum[0] : cs == 1u ? sum[1] : sum[2];
  uint32_t T0[4] = { 0u, 0u, 0u, 0u }, T1[4] = { 0u, 0u, 0u, 0u };
  ICAMD_UNROLL
  for (int c = 0; c < NCH; ++c) {
    const int32_t cov = (int32_t)(n * cross[c]) - (int32_t)(sum_star * sum[c]);  // both below 2^25
    const bool flip = NCH > 1 && cov < 0 && (uint32_t)c != cs;
    T0[c] = flip ? hi[c] : lo[c];
    T1[c] = flip ? lo[c] : hi[c];
  }
  Bc7Fit f;
  bc7_quantise_pair<NCH, Q>(T0, T1, f.E0, f.E1);
  f.sse = bc7_search_set<NCH, IBITS>(u, mask, f.E0, f.E1, f.inv);
  // the refit: the mode-6 formulas, the sums over S
  uint32_t a = 0, b = 0, c2 = 0, X[4] = { 0u, 0u, 0u, 0u }, Y[4] = { 0u, 0u, 0u, 0u };
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const bool in = ((mask >> i) & 1u) != 0u;
    const uint32_t wt = bc7_weight(15u - ((uint32_t)(f.inv >> (4 * i)) & 15u), (uint32_t)IBITS);
    const uint32_t w = in ? wt : 0u, m = in ? 64u - wt : 0u;
    a += m * m;
    b += m * w;
    c2 += w * w;
    ICAMD_UNROLL
    for (int c = 0; c < NCH; ++c) {
      X[c] += m * bc7_ch(u[i], c);
      Y[c] += w * bc7_ch(u[i], c);
    }
  }
  const uint32_t det = a * c2 - b * b;  // a + c2 <= 16 * 4096, so a c2 <= 2^30, and >= b^2 (Cauchy-Schwarz)
  if (det != 0u) {
    ICAMD_UNROLL
    for (int c = 0; c < NCH; ++c) {
      const int64_t Xc = (int64_t)X[c], Yc = (int64_t)Y[c];
      const int64_t n0 = 64 * ((int64_t)c2 * Xc - (int64_t)b * Yc), n1 = 64 * ((int64_t)a * Yc - (int64_t)b * Xc);
      const int64_t N0 = 2 * n0 + (int64_t)det, N1 = 2 * n1 + (int64_t)det;
      T0[c] = N0 < 0 ? 0u : bc7_div255((uint64_t)N0, 2ull * det);
      T1[c] = N1 < 0 ? 0u : bc7_div255((uint64_t)N1, 2ull * det);
    }
    Bc7Fit g;
    bc7_quantise_pair<NCH, Q>(T0, T1, g.E0, g.E1);
    g.sse = bc7_search_set<NCH, IBITS>(u, mask, g.E0, g.E1, g.inv);
    if (g.sse < f.sse) f = g;
  }
  return f;
}

// ---- mode 1

// The partition of the smallest within-subset scatter of R, G, B: the largest N_s / d_s, exact, ties to the smaller s.
ICAMD_DEV uint32_t bc7_best_partition(const uint32_t v[16]) {
  uint32_t ch[3][4], tot[3];  // channel c of texels 4 j .. 4 j + 3, one per byte
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    tot[c] = 0u;
    ICAMD_UNROLL
    for (int j = 0; j < 4; ++j) {
      ch[c][j] = bc7_ch(v[4 * j], c) | bc7_ch(v[4 * j + 1], c) << 8 | bc7_ch(v[4 * j + 2], c) << 16 | bc7_ch(v[4 * j + 3], c) << 24;
      tot[c] = udot4(ch[c][j], 0x01010101u, tot[c]);
    }
  }
  uint32_t best = 0, bn = 0, bd = 1;
  ICAMD_BC7_NOUNROLL
  for (uint32_t s = 0; s < 64; ++s) {
    const uint32_t m = kBc7Partitions.w[s][1] & 0xffffu;  // s is the same in every lane: a scalar load
    const uint32_t n1 = (uint32_t)__builtin_popcount(m), n0 = 16u - n1;
    uint32_t q0 = 0, q1 = 0;
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) {
      uint32_t s1 = 0;
      ICAMD_UNROLL
      for (int j = 0; j < 4; ++j) s1 = udot4(ch[c][j], (((m >> (4 * j)) & 15u) * 0x00204081u) & 0x01010101u, s1);
      const uint32_t s0 = tot[c] - s1;
      q0 += s0 * s0;
      q1 += s1 * s1;
    }
    // N < 2^28: n1 * 3 * (255 n0)^2 + n0 * 3 * (255 n1)^2 = 3 * 255^2 * n0 n1 (n0 + n1) <= 3 * 255^2 * 64 * 16
    const uint32_t N = n1 * q0 + n0 * q1, d = n0 * n1;
    if ((uint64_t)N * bd > (uint64_t)bn * d) {
      best = s;
      bn = N;
      bd = d;
    }
  }
  return best;
}

struct Bc7Bits128 {
  uint64_t lo, hi;
};
// val (nbits wide, nbits <= 32) at bit pos of the block; pos is a compile-time constant after unrolling
ICAMD_DEV void bc7_put(Bc7Bits128 &b, int pos, uint64_t val, int nbits) {
  if (pos < 64) {
    b.lo |= val << pos;
    if (pos + nbits > 64) b.hi |= val >> (64 - pos);
  } else {
    b.hi |= val << (pos - 64);
  }
}

// v: opaque texels.  Returns sse1 (over four channels: alpha decodes to 255 exactly).
ICAMD_DEV uint32_t encode_bc7_mode1(const uint32_t v[16], uint32_t out[4]) {
  uint32_t u[16];
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) u[i] = v[i] & 0x00ffffffu;
  const uint32_t part = bc7_best_partition(v);
  const uint32_t entry = kBc7Partitions.w[part][1];
  const uint32_t m1 = entry & 0xffffu, anchor = (entry >> 16) & 15u;
  Bc7Fit f[2] = { bc7_subfit<3, 3, kBc7Q1>(u, m1 ^ 0xffffu), bc7_subfit<3, 3, kBc7Q1>(u, m1) };
  const uint32_t sse = f[0].sse + f[1].sse;
  // anchors: k >= 4 iff 15 - k < 12
  uint64_t k[2];
  ICAMD_UNROLL
  for (int j = 0; j < 2; ++j) {
    const uint32_t at = j == 0 ? 0u : anchor;
    k[j] = ~f[j].inv;  // k_p in the low three bits of nibble p
    if (((uint32_t)(f[j].inv >> (4u * at)) & 15u) < 12u) {
      const uint32_t t = f[j].E0;
      f[j].E0 = f[j].E1;
      f[j].E1 = t;
      k[j] = f[j].inv;  // 7 - k = (15 - k) - 8: the low three bits of 15 - k
    }
  }
  // indices: three bits a texel at 3 p - 1 (texel 0 two bits), then the second anchor's third bit -- clear -- is dropped
  uint64_t idx = 0;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint64_t kk = ((m1 >> p) & 1u) ? k[1] : k[0];
    const uint64_t x = (kk >> (4 * p)) & 7u;
    idx |= p == 0 ? x : x << (3 * p - 1);
  }
  const uint32_t cut = 3u * anchor + 1u;  // the anchor's two stored bits end here
  idx = (idx & ((1ull << cut) - 1ull)) | ((idx >> (cut + 1u)) << cut);
  Bc7Bits128 b = { 2ull | (uint64_t)part << 2, 0ull };
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    bc7_put(b, 8 + 24 * c, bc7_ch(f[0].E0, c) >> 2, 6);
    bc7_put(b, 14 + 24 * c, bc7_ch(f[0].E1, c) >> 2, 6);
    bc7_put(b, 20 + 24 * c, bc7_ch(f[1].E0, c) >> 2, 6);
    bc7_put(b, 26 + 24 * c, bc7_ch(f[1].E1, c) >> 2, 6);
  }
  bc7_put(b, 80, (f[0].E0 >> 1) & 1u, 1);
  bc7_put(b, 81, (f[1].E0 >> 1) & 1u, 1);
  b.hi |= idx << 18;
  out[0] = (uint32_t)b.lo;
  out[1] = (uint32_t)(b.lo >> 32);
  out[2] = (uint32_t)b.hi;
  out[3] = (uint32_t)(b.hi >> 32);
  return sse;
}

// ---- mode 5, rotation 0

// 15 - k_p nibbles -> the 31 index bits of a 2-bit plane, the anchor flip applied; flipped: the endpoints are to be exchanged
ICAMD_DEV uint32_t bc7_mode5_indices(uint64_t inv, bool &flipped) {
  flipped = ((uint32_t)inv & 15u) < 14u;  // k_0 >= 2
  const uint64_t k = flipped ? inv : ~inv;  // 3 - k = (15 - k) - 12: the low two bits of 15 - k
  uint32_t idx = 0;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint32_t x = (uint32_t)(k >> (4 * p)) & 3u;
    idx |= p == 0 ? x : x << (2 * p - 1);
  }
  return idx;
}

ICAMD_DEV uint32_t encode_bc7_mode5(const uint32_t v[16], uint32_t out[4]) {
  uint32_t u[16], al[16];
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    u[i] = v[i] & 0x00ffffffu;
    al[i] = v[i] >> 24;
  }
  Bc7Fit fc = bc7_subfit<3, 2, kBc7Q5>(u, 0xffffu);
  Bc7Fit fa = bc7_subfit<1, 2, kBc7QIdentity>(al, 0xffffu);
  bool flipc, flipa;
  const uint32_t ic = bc7_mode5_indices(fc.inv, flipc), ia = bc7_mode5_indices(fa.inv, flipa);
  const uint32_t C0 = flipc ? fc.E1 : fc.E0, C1 = flipc ? fc.E0 : fc.E1;
  const uint32_t A0 = flipa ? fa.E1 : fa.E0, A1 = flipa ? fa.E0 : fa.E1;
  Bc7Bits128 b = { 1ull << 5, 0ull };
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    bc7_put(b, 8 + 14 * c, bc7_ch(C0, c) >> 1, 7);
    bc7_put(b, 15 + 14 * c, bc7_ch(C1, c) >> 1, 7);
  }
  bc7_put(b, 50, A0 & 0xffu, 8);
  bc7_put(b, 58, A1 & 0xffu, 8);
  bc7_put(b, 66, ic, 31);
  bc7_put(b, 97, ia, 31);
  out[0] = (uint32_t)b.lo;
  out[1] = (uint32_t)(b.lo >> 32);
  out[2] = (uint32_t)b.hi;
  out[3] = (uint32_t)(b.hi >> 32);
  return fc.sse + fa.sse;
}

// ---- the choice

// px as encode_bc7 takes them; out: the block of ICAMD_BC7_MODES_EXTENDED.
template <int COMPS>
ICAMD_DEV void encode_bc7_modes(const uint32_t px[16], bool swap, uint32_t out[4]) {
  encode_bc7<COMPS>(px, swap, out);
  uint32_t v[16], all_a = 0xff000000u;
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    uint32_t t = COMPS == 4 ? px[i] : (px[i] | 0xff000000u);
    if (swap) t = (t & 0xff00ff00u) | ((t >> 16) & 0xffu) | ((t & 0xffu) << 16);
    v[i] = t;
    all_a &= t;
  }
  const uint32_t sse6 = bc7_mode6_sse(v, out);
  if (sse6 == 0u) return;  // no candidate is strictly closer
  uint32_t cand[4], sse;
  if (COMPS == 3 || all_a == 0xff000000u)
    sse = encode_bc7_mode1(v, cand);
  else
    sse = encode_bc7_mode5(v, cand);
  if (sse < sse6) {
    ICAMD_UNROLL
    for (int i = 0; i < 4; ++i) out[i] = cand[i];
  }
}

}  // namespace icamd
#endif  // ICAMD_BC7_MODES_BLOCK_H_
