// bc6h_modes_block.h -- BC6H with the opt-in two-subset candidate (EXTENSION, include/ic_amd.h ICAMD_BC6H_MODES_EXTENDED;
// DESIGN.md 3.24).  The definition is stated in include/ic_amd.h and restated in tests/bc6h_modes_oracle.py.  One block per lane,
// integer only.  The one-subset block and its sse are encode_bc6h_sse's (bc6h_block.h, untouched arithmetic).
//
// The candidate's mode is PER-LANE DATA: the ladder is screened on the quantised first-pass targets alone (bc6h_pick_mode: one
// quantisation of the twelve targets per distinct endpoint width, a uniform loop over the ladder), and what it leaves behind --
// the endpoint bits b, the three delta widths, the table slot -- are registers, not branches: un-quantise takes b as a shift
// amount, so the lanes of a wave, which sit in different modes on real content, run one instruction stream through the sub-fits.
// Both subsets are searched in ONE sweep over the sixteen texels (each texel against its own subset's palette), so a block costs
// two sweeps of 8 palette entries where the one-subset block costs two of 16.  The header is packed from the same rows of
// bc6h_mode_tables.inc that drive the decoder (kBc6hModes): the runs are read at the lane's slot and the fields put where they
// say.  No wave-uniform shortcut anywhere.
#ifndef ICAMD_BC6H_MODES_BLOCK_H_
#define ICAMD_BC6H_MODES_BLOCK_H_

#include "bc6h_block.h"

namespace icamd {

namespace bc6h_modes_detail {
// The ladder: rows of bc6h_mode_tables.inc in the order they are tried (mode fields 00, 01110, 10010, 10110, 11010, 01, 11110).
constexpr int kLadder = 7;
constexpr uint32_t ladder_slot(uint32_t li) { return li == 0u ? 0u : li == 5u ? 1u : li == 6u ? 9u : li + 4u; }
constexpr uint32_t ladder_field(uint32_t li) { return li == 0u ? 0x00u : li == 5u ? 0x01u : li == 6u ? 0x1eu : 0x0eu + 4u * (li - 1u); }
constexpr bool ladder_ok() {
  for (uint32_t i = 0; i < (uint32_t)kLadder; ++i) {
    const bc6h_detail::ModeRow &r = bc6h_detail::kRows[ladder_slot(i)];
    if (r.mode_field != ladder_field(i) || r.subsets != 2 || (r.transformed != 0) != (i + 1u < (uint32_t)kLadder)) return false;
    if (i && r.endpoint_bits > bc6h_detail::kRows[ladder_slot(i - 1u)].endpoint_bits) return false;  // the widths only shrink
    if (r.endpoint_bits > 10 || r.endpoint_bits < 6) return false;
  }
  return true;
}
static_assert(ladder_ok(), "the ladder names rows bc6h_mode_tables.inc does not hold");
}  // namespace bc6h_modes_detail

// What the ladder leaves a lane with.
struct Bc6hLaneMode {
  uint32_t slot, field, field_bits, b, delta[3];
  bool transformed;
};

// ---- the grids

// D_b(q): the t-domain value the b-bit endpoint q decodes to at weight 0
template <bool SIGNED>
ICAMD_DEV int32_t bc6h_endpoint_value_at(int32_t q, uint32_t b) {
  return bc6h_target<SIGNED>(bc6h_finish<SIGNED>(bc6h_unquantise<SIGNED>(q, b)));
}

// Q_b(T): the smallest q that minimises |D_b(q) - T|, 6 <= b <= 10.  Between its ends D_b is (31 q + 15.5) 2^(10 - b)
// (unsigned) or sign(q) (62 |q| + 31) 2^(10 - b) (signed), so the minimum lies within one step of T / (31 * 2^(10 - b)) resp.
// T / (62 * 2^(10 - b)), truncating: three candidates in ascending order, replaced on a strictly smaller distance only.
// tests/test_bc6h_modes_host.py holds this to the definition for every T and b.
template <bool SIGNED>
ICAMD_DEV int32_t bc6h_quantise_at(int32_t T, uint32_t b) {
  const int32_t hi = SIGNED ? (int32_t)(1u << (b - 1u)) - 1 : (int32_t)(1u << b) - 1, lo = SIGNED ? -hi : 0;
  const uint32_t mag = (uint32_t)(T < 0 ? -T : T);
  const int32_t ga = (int32_t)((mag / (SIGNED ? 62u : 31u)) >> (10u - b));
  const int32_t g = T < 0 ? -ga : ga;
  int32_t best_q = 0;
  uint32_t best = 0xffffffffu;
  ICAMD_UNROLL
  for (int d = -1; d <= 1; ++d) {
    const int32_t q = imin(imax(g + d, lo), hi);
    const int32_t e = bc6h_endpoint_value_at<SIGNED>(q, b) - T;
    const uint32_t a = (uint32_t)(e < 0 ? -e : e);
    if (a < best) {
      best = a;
      best_q = q;
    }
  }
  return best_q;
}

// ---- step 1: the partition of the largest N_s / d_s, exact, ties to the smaller s.  The 32 masks are read at a uniform index;
// a subset's sums are the block's totals minus one masked sum.
ICAMD_DEV uint32_t bc6h_best_partition(const int32_t t[16][3]) {
  int32_t tot[3] = { 0, 0, 0 };
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i)
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) tot[c] += t[i][c];
  uint32_t best = 0, bd = 1;
  uint64_t bn = 0;
  ICAMD_NOUNROLL
  for (uint32_t s = 0; s < 32; ++s) {
    const uint32_t m = kBc7Partitions.w[s][1] & 0xffffu;
    const uint32_t n1 = (uint32_t)__builtin_popcount(m), n0 = 16u - n1;
    int32_t s1[3] = { 0, 0, 0 };
    ICAMD_UNROLL
    for (int i = 0; i < 16; ++i) {
      const int32_t bit = (int32_t)((m >> i) & 1u);
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c) s1[c] += bit * t[i][c];
    }
    uint64_t q0 = 0, q1 = 0;  // |S0|^2, |S1|^2: a component is below 2^19, three squares below 2^40
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) {
      const int64_t a = (int64_t)(tot[c] - s1[c]), b = (int64_t)s1[c];
      q0 += (uint64_t)(a * a);
      q1 += (uint64_t)(b * b);
    }
    const uint64_t N = n1 * q0 + n0 * q1;  // (below 2^42; times a d of at most 64: below 2^48)
    const uint32_t d = n0 * n1;
    if (N * bd > bn * d) {
      best = s;
      bn = N;
      bd = d;
    }
  }
  return best;
}

// ---- step 2: step 1 of the one-subset definition over the texels of `mask` (never empty)
ICAMD_DEV void bc6h_subset_targets(const int32_t t[16][3], uint32_t mask, int32_t T0[3], int32_t T1[3]) {
  const int32_t n = (int32_t)__builtin_popcount(mask);
  int32_t lo[3], hi[3], sum[3];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    lo[c] = 0x7fffffff;
    hi[c] = -0x7fffffff;
    sum[c] = 0;
    ICAMD_UNROLL
    for (int i = 0; i < 16; ++i) {
      const bool in = ((mask >> i) & 1u) != 0u;
      lo[c] = imin(lo[c], in ? t[i][c] : 0x7fffffff);
      hi[c] = imax(hi[c], in ? t[i][c] : -0x7fffffff);
      sum[c] += in ? t[i][c] : 0;
    }
  }
  uint32_t cs = 0;
  int32_t widest = hi[0] - lo[0];
  ICAMD_UNROLL
  for (int c = 1; c < 3; ++c)
    if (hi[c] - lo[c] > widest) {
      widest = hi[c] - lo[c];
      cs = (uint32_t)c;
    }
  // (c* picks by masks, not by selects between the texels' registers: those the compiler turns into indexed loads from a
  // copy of t in scratch)
  const int32_t pick[3] = { cs == 0u ? -1 : 0, cs == 1u ? -1 : 0, cs == 2u ? -1 : 0 };
  int64_t cross[3] = { 0, 0, 0 };
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const int32_t v = (t[i][0] & pick[0]) | (t[i][1] & pick[1]) | (t[i][2] & pick[2]);
    const int32_t star = ((mask >> i) & 1u) ? v : 0;
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) cross[c] += (int64_t)star * t[i][c];
  }
  const int32_t sum_star = cs == 0u ? sum[0] : cs == 1u ? sum[1] : sum[2];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    const int64_t cov = (int64_t)n * cross[c] - (int64_t)sum_star * sum[c];
    const bool flip = cov < 0 && (uint32_t)c != cs;
    T0[c] = flip ? hi[c] : lo[c];
    T1[c] = flip ? lo[c] : hi[c];
  }
}

// ---- step 3

// Feasible: both of subset 0's endpoints can be the base of every delta (and, signed format, no endpoint is negative).
template <bool SIGNED>
ICAMD_DEV bool bc6h_feasible(const int32_t E[4][3], const uint32_t delta[3], bool transformed) {
  bool ok = true;
  int32_t least = 0;
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    const int32_t mn = imin(imin(E[0][c], E[1][c]), imin(E[2][c], E[3][c]));
    const int32_t mx = imax(imax(E[0][c], E[1][c]), imax(E[2][c], E[3][c]));
    const int32_t base_lo = imin(E[0][c], E[1][c]), base_hi = imax(E[0][c], E[1][c]);
    const int32_t half = (int32_t)(1u << (delta[c] - 1u));
    ok = ok && mx - base_lo <= half - 1 && mn - base_hi >= -half;
    least = imin(least, mn);
  }
  if (SIGNED) ok = ok && least >= 0;
  return ok || !transformed;
}

// T[0..3] = T0_0, T1_0, T0_1, T1_1 -> the first feasible mode of the ladder and E = Q_b(T) at its b
template <bool SIGNED>
ICAMD_DEV Bc6hLaneMode bc6h_pick_mode(const int32_t T[4][3], int32_t E[4][3]) {
  Bc6hLaneMode mode = { 0u, 0u, 0u, 0u, { 0u, 0u, 0u }, false };
  bool found = false;
  int32_t Q[4][3];
  uint32_t prev_b = 0u;
  ICAMD_NOUNROLL
  for (uint32_t li = 0; li < (uint32_t)bc6h_modes_detail::kLadder; ++li) {
    const uint32_t slot = bc6h_modes_detail::ladder_slot(li);
    const uint32_t info = kBc6hModes.info[slot];  // li is the same in every lane: scalar loads
    const uint32_t b = (info >> 4) & 31u;
    const uint32_t delta[3] = { (info >> 9) & 15u, (info >> 13) & 15u, (info >> 17) & 15u };
    const bool transformed = ((info >> 21) & 1u) != 0u;
    if (b != prev_b) {
      ICAMD_UNROLL
      for (int e = 0; e < 4; ++e)
        ICAMD_UNROLL
        for (int c = 0; c < 3; ++c) Q[e][c] = bc6h_quantise_at<SIGNED>(T[e][c], b);
      prev_b = b;
    }
    if (!found && bc6h_feasible<SIGNED>(Q, delta, transformed)) {
      found = true;
      mode.slot = slot;
      mode.field = bc6h_modes_detail::ladder_field(li);
      mode.field_bits = (info >> 1) & 7u;
      mode.b = b;
      mode.transformed = transformed;
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c) mode.delta[c] = delta[c];
      ICAMD_UNROLL
      for (int e = 0; e < 4; ++e)
        ICAMD_UNROLL
        for (int c = 0; c < 3; ++c) E[e][c] = Q[e][c];
    }
  }
  return mode;  // (the last mode of the ladder is feasible for every block)
}

// ---- step 4

// Both subsets in one sweep: texel p is searched against the palette of its own subset (bit p of m1: subset 1, endpoints E[2],
// E[3]).  k_p in nibble p of idx; sse[j] = the sum of the minima over subset j.  The loop over k stays rolled as in bc6h_search.
template <bool SIGNED>
ICAMD_DEV void bc6h_search_pair(const int32_t t[16][3], uint32_t m1, uint32_t b, const int32_t E[4][3], uint64_t &idx,
                                uint64_t sse[2]) {
  typedef typename Bc6hDist<SIGNED>::type dist_t;
  int32_t U[4][3];
  ICAMD_UNROLL
  for (int e = 0; e < 4; ++e)
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) U[e][c] = bc6h_unquantise<SIGNED>(E[e][c], b);
  dist_t best[16];
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) best[p] = ~(dist_t)0;
  uint32_t lo = 0u, hi = 0u;
  ICAMD_NOUNROLL
  for (uint32_t k = 0; k < 8; ++k) {
    const uint32_t w = (k * 64u + 3u) / 7u;  // (the 3-bit weights: bc7_detail::weights_ok)
    int32_t pal[2][3];
    ICAMD_UNROLL
    for (int j = 0; j < 2; ++j)
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c)
        pal[j][c] = bc6h_target<SIGNED>(bc6h_finish<SIGNED>(bc6h_interp(U[2 * j][c], U[2 * j + 1][c], w)));
    ICAMD_UNROLL
    for (int p = 0; p < 16; ++p) {
      const bool second = ((m1 >> p) & 1u) != 0u;
      dist_t d = 0;
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c) {
        const int32_t e = (second ? pal[1][c] : pal[0][c]) - t[p][c];
        const uint32_t m = (uint32_t)(e < 0 ? -e : e);
        d += (dist_t)umad24(m, m, 0u);
      }
      const bool better = d < best[p];
      best[p] = better ? d : best[p];
      const uint32_t sh = 4u * (uint32_t)(p & 7), mask = ~(15u << sh);
      if (p < 8) lo = better ? (lo & mask) | k << sh : lo;
      else hi = better ? (hi & mask) | k << sh : hi;
    }
  }
  sse[0] = sse[1] = 0;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const bool second = ((m1 >> p) & 1u) != 0u;
    sse[0] += second ? 0u : (uint64_t)best[p];
    sse[1] += second ? (uint64_t)best[p] : 0u;
  }
  idx = (uint64_t)lo | (uint64_t)hi << 32;
}

// One least-squares refit of the subset `mask` from its indices: F = Q_b of the clamped solutions; det = 0: F = E (the second
// search then finds nothing strictly closer, which is "no refit").
template <bool SIGNED>
ICAMD_DEV void bc6h_subset_refit(const int32_t t[16][3], uint32_t mask, uint64_t idx, uint32_t b, const int32_t E0[3],
                                 const int32_t E1[3], int32_t F0[3], int32_t F1[3]) {
  uint32_t a = 0, bb = 0, c2 = 0;
  int32_t Y[3] = { 0, 0, 0 }, sum[3] = { 0, 0, 0 };
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const bool in = ((mask >> i) & 1u) != 0u;
    const uint32_t wt = bc7_weight((uint32_t)(idx >> (4 * i)) & 7u, 3u);
    const uint32_t w = in ? wt : 0u, m = in ? 64u - wt : 0u;
    a += m * m;
    bb += m * w;
    c2 += w * w;
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) {
      Y[c] += (int32_t)w * t[i][c];
      sum[c] += in ? t[i][c] : 0;
    }
  }
  const uint32_t det = a * c2 - bb * bb;
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    const int64_t X = (int64_t)(64 * sum[c] - Y[c]), Yc = (int64_t)Y[c];
    const int64_t n0 = 64 * ((int64_t)c2 * X - (int64_t)bb * Yc), n1 = 64 * ((int64_t)a * Yc - (int64_t)bb * X);
    const uint64_t den = det ? 2ull * det : 2ull;
    const int32_t q0 = bc6h_quantise_at<SIGNED>(bc6h_floor_div_clamped<SIGNED>(2 * n0 + (int64_t)det, den), b);
    const int32_t q1 = bc6h_quantise_at<SIGNED>(bc6h_floor_div_clamped<SIGNED>(2 * n1 + (int64_t)det, den), b);
    F0[c] = det ? q0 : E0[c];
    F1[c] = det ? q1 : E1[c];
  }
}

// bit i of m -> nibble i of the result = 0xF
ICAMD_DEV uint64_t bc6h_nibbles(uint32_t m) {
  uint64_t x = m & 0xffffu;
  x = (x | x << 24) & 0x000000ff000000ffull;
  x = (x | x << 12) & 0x000f000f000f000full;
  x = (x | x << 6) & 0x0303030303030303ull;
  x = (x | x << 3) & 0x1111111111111111ull;
  return x * 15u;
}

struct Bc6hBits128 {
  uint64_t lo, hi;
  uint32_t pos;
};
// v (n bits, n <= 10) at the lane's position
ICAMD_DEV void bc6h_put(Bc6hBits128 &s, uint64_t v, uint32_t n) {
  const uint32_t p = s.pos & 63u;
  if (s.pos < 64u) {
    s.lo |= v << p;
    s.hi |= (v >> 1) >> (63u - p);
  } else {
    s.hi |= v << p;
  }
  s.pos += n;
}

// ---- the candidate: t -> the two-subset block and its sse2
template <bool SIGNED>
ICAMD_DEV uint64_t encode_bc6h_two_subsets(const int32_t t[16][3], uint32_t out[4]) {
  const uint32_t part = bc6h_best_partition(t);
  const uint32_t entry = kBc7Partitions.w[part][1];
  const uint32_t m1 = entry & 0xffffu, m0 = m1 ^ 0xffffu, anchor = (entry >> 16) & 15u;
  int32_t T[4][3], E[4][3], F[4][3];
  bc6h_subset_targets(t, m0, T[0], T[1]);
  bc6h_subset_targets(t, m1, T[2], T[3]);
  const Bc6hLaneMode mode = bc6h_pick_mode<SIGNED>(T, E);
  uint64_t idx_a, idx_b, sse_a[2], sse_b[2];
  bc6h_search_pair<SIGNED>(t, m1, mode.b, E, idx_a, sse_a);
  bc6h_subset_refit<SIGNED>(t, m0, idx_a, mode.b, E[0], E[1], F[0], F[1]);
  bc6h_subset_refit<SIGNED>(t, m1, idx_a, mode.b, E[2], E[3], F[2], F[3]);
  bc6h_search_pair<SIGNED>(t, m1, mode.b, F, idx_b, sse_b);
  // subset 0's refit against subset 1's first pass, then subset 1's against subset 0's final endpoints
  bool take[2];
  ICAMD_UNROLL
  for (int j = 0; j < 2; ++j) {
    int32_t trial[4][3];
    ICAMD_UNROLL
    for (int e = 0; e < 4; ++e)
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c) trial[e][c] = (e >> 1) == j ? F[e][c] : E[e][c];
    take[j] = sse_b[j] < sse_a[j] && bc6h_feasible<SIGNED>(trial, mode.delta, mode.transformed);
    ICAMD_UNROLL
    for (int e = 2 * j; e < 2 * j + 2; ++e)
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c) E[e][c] = take[j] ? F[e][c] : E[e][c];
  }
  const uint64_t sse = (take[0] ? sse_b[0] : sse_a[0]) + (take[1] ? sse_b[1] : sse_a[1]);
  const uint64_t from_b = bc6h_nibbles((take[0] ? m0 : 0u) | (take[1] ? m1 : 0u));
  uint64_t idx = (idx_b & from_b) | (idx_a & ~from_b);
  // step 5
  const bool flip0 = ((uint32_t)idx & 7u) >= 4u, flip1 = ((uint32_t)(idx >> (4u * anchor)) & 7u) >= 4u;
  idx ^= bc6h_nibbles((flip0 ? m0 : 0u) | (flip1 ? m1 : 0u)) & 0x7777777777777777ull;  // 7 - k
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    const int32_t e0 = E[0][c], e2 = E[2][c];
    E[0][c] = flip0 ? E[1][c] : e0;
    E[1][c] = flip0 ? e0 : E[1][c];
    E[2][c] = flip1 ? E[3][c] : e2;
    E[3][c] = flip1 ? e2 : E[3][c];
  }
  // step 6: the fields, endpoint e of colour c in bits 16 e .. 16 e + 15 of acc[c] (as decode_bc6h gathers them)
  uint64_t acc[3];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    const uint32_t dmask = (1u << mode.delta[c]) - 1u;
    acc[c] = (uint64_t)((uint32_t)E[0][c] & ((1u << mode.b) - 1u));
    ICAMD_UNROLL
    for (int e = 1; e < 4; ++e) {
      const uint32_t v = (uint32_t)(mode.transformed ? E[e][c] - E[0][c] : E[e][c]) & dmask;
      acc[c] |= (uint64_t)v << (16 * e);
    }
  }
  Bc6hBits128 s = { mode.field, 0ull, mode.field_bits };
  ICAMD_UNROLL
  for (int j = 0; j < bc6h_detail::kMaxRuns / 4; ++j) {
    const uint64_t four = kBc6hModes.runs[mode.slot][j];
    ICAMD_UNROLL
    for (int k = 0; k < 4; ++k) {
      const uint32_t run = (uint32_t)(four >> (16 * k)) & 0xffffu, dest = run >> 4, count = run & 15u;
      const uint32_t c = dest >> 6;
      const uint64_t src = c == 0u ? acc[0] : c == 1u ? acc[1] : c == 2u ? acc[2] : (uint64_t)part;
      bc6h_put(s, (src >> (dest & 63u)) & ((1ull << count) - 1ull), count);
    }
  }
  // (s.pos == 82.)  Indices: three bits a texel at 3 p - 1 (texel 0 two bits), then subset 1's anchor's third bit -- clear -- is
  // dropped
  uint64_t ib = 0;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    const uint64_t x = (idx >> (4 * p)) & 7u;
    ib |= p == 0 ? x : x << (3 * p - 1);
  }
  const uint32_t cut = 3u * anchor + 1u;
  ib = (ib & ((1ull << cut) - 1ull)) | ((ib >> (cut + 1u)) << cut);
  s.hi |= ib << 18;
  out[0] = (uint32_t)s.lo;
  out[1] = (uint32_t)(s.lo >> 32);
  out[2] = (uint32_t)s.hi;
  out[3] = (uint32_t)(s.hi >> 32);
  return sse;
}

// rg / b as encode_bc6h takes them; out: the block of ICAMD_BC6H_MODES_EXTENDED.
template <bool SIGNED>
ICAMD_DEV void encode_bc6h_modes(const uint32_t rg[16], const uint32_t b[16], uint32_t out[4]) {
  const uint64_t sse1 = encode_bc6h_sse<SIGNED>(rg, b, out);
  int32_t t[16][3];
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    t[i][0] = bc6h_target<SIGNED>(rg[i] & 0xffffu);
    t[i][1] = bc6h_target<SIGNED>(rg[i] >> 16);
    t[i][2] = bc6h_target<SIGNED>(b[i] & 0xffffu);
  }
  uint32_t cand[4];
  const uint64_t sse2 = encode_bc6h_two_subsets<SIGNED>(t, cand);
  if (sse2 < sse1) {
    ICAMD_UNROLL
    for (int i = 0; i < 4; ++i) out[i] = cand[i];
  }
}

}  // namespace icamd
#endif  // ICAMD_BC6H_MODES_BLOCK_H_
