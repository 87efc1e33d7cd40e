// bc6h_block.h -- BC6H (BPTC float) block math (EXTENSION, include/ic_amd.h ICAMD_BC6H_UF16 / ICAMD_BC6H_SF16):
// the decoder of all fourteen modes, the one-subset encoder whose definition is stated in include/ic_amd.h and restated in
// tests/bc6h_oracle.py, the fetch of RGB16F / RGBA16F blocks and the metric.  One block per lane, everything in registers,
// integer only (a half is its 16-bit pattern throughout).  Texel i = 4 y + x.
//
// Tables: the fourteen header layouts are data (bc6h_mode_tables.inc), packed at compile time into 18 rows -- one per mode in
// the table's order and four empty ones for the reserved mode fields -- of six 8-byte words of four 16-bit runs each
// (count | destination << 4) and one info word.  Lanes of a wave hold different modes, so a lane loads ITS row's words at a
// per-lane index (a __device__ const table of 936 bytes that stays in the vector L1, as kBc7Partitions); there is no
// wave-uniform shortcut.  The runs are taken off the block as off a shift register (bc7_take) and land in three 64-bit
// accumulators, one per colour, endpoint e in bits 16 e .. 16 e + 15: the destination selects an accumulator by comparison, never
// by indexing an array, so nothing is spilled to scratch.  Partitions, anchors and weights are BC7's (bc7_block.h).
#ifndef ICAMD_BC6H_BLOCK_H_
#define ICAMD_BC6H_BLOCK_H_

#include "bc7_block.h"

namespace icamd {

namespace bc6h_detail {
enum Field : uint8_t { RW, RX, RY, RZ, GW, GX, GY, GZ, BW, BX, BY, BZ, D };
struct Run {
  uint8_t field, first, count;
};
constexpr int kMaxRuns = 24, kModes = 14, kSlots = 18;
struct ModeRow {
  uint8_t mode_field, mode_bits, endpoint_bits, delta_bits[3], transformed, subsets;
  Run runs[kMaxRuns];
};
constexpr ModeRow kRows[kModes] = {
#define ICAMD_BC6H_TABLE_MODES
#include "bc6h_mode_tables.inc"
#undef ICAMD_BC6H_TABLE_MODES
};
// info: bit 0 = valid, bits 1..3 = mode-field bits, 4..8 = endpoint bits, 9..12 / 13..16 / 17..20 = delta bits of R / G / B,
// bit 21 = transformed, bit 22 = two subsets
struct Packed {
  uint64_t runs[kSlots][kMaxRuns / 4];
  uint32_t info[kSlots];
};
constexpr Packed pack() {
  Packed t = {};
  for (int m = 0; m < kModes; ++m) {
    const ModeRow &r = kRows[m];
    for (int j = 0; j < kMaxRuns; ++j) {
      const uint64_t run = (uint64_t)r.runs[j].count | (uint64_t)(r.runs[j].field * 16u + r.runs[j].first) << 4;
      t.runs[m][j / 4] |= run << (16 * (j % 4));
    }
    t.info[m] = 1u | (uint32_t)r.mode_bits << 1 | (uint32_t)r.endpoint_bits << 4 | (uint32_t)r.delta_bits[0] << 9 |
                (uint32_t)r.delta_bits[1] << 13 | (uint32_t)r.delta_bits[2] << 17 | (uint32_t)r.transformed << 21 |
                (r.subsets == 2 ? 1u << 22 : 0u);
  }
  // the reserved mode fields: no runs, widths of 1 (so that the decoder's arithmetic stays defined), the valid bit clear
  for (int m = kModes; m < kSlots; ++m) t.info[m] = 5u << 1 | 1u << 4 | 1u << 9 | 1u << 13 | 1u << 17;
  return t;
}
// Every row: its slot is what the decoder computes from the mode field, every field bit below the field's width is written
// exactly once, the runs end at bit 82 (two subsets) or 65 (one).
constexpr bool rows_ok() {
  for (int m = 0; m < kModes; ++m) {
    const ModeRow &r = kRows[m];
    const uint32_t f = r.mode_field;
    const uint32_t slot = (f & 2u) ? ((f & 1u) ? 10u : 2u) + ((f >> 2) & 7u) : (f & 1u);
    if (slot != (uint32_t)m || (r.mode_bits != 2 && r.mode_bits != 5) || (r.mode_bits == 2) != (m < 2)) return false;
    uint32_t seen[13] = {}, bits = r.mode_bits;
    for (int j = 0; j < kMaxRuns; ++j)
      for (uint32_t k = 0; k < r.runs[j].count; ++k) {
        const uint32_t bit = 1u << (r.runs[j].first + k);
        if (r.runs[j].count > 10 || (seen[r.runs[j].field] & bit)) return false;
        seen[r.runs[j].field] |= bit;
        ++bits;
      }
    if (bits != (r.subsets == 2 ? 82u : 65u)) return false;
    for (int c = 0; c < 3; ++c) {
      if (seen[4 * c] != (1u << r.endpoint_bits) - 1u || seen[4 * c + 1] != (1u << r.delta_bits[c]) - 1u) return false;
      const uint32_t second = r.subsets == 2 ? (1u << r.delta_bits[c]) - 1u : 0u;
      if (seen[4 * c + 2] != second || seen[4 * c + 3] != second) return false;
    }
    if (seen[D] != (r.subsets == 2 ? 31u : 0u)) return false;
  }
  return true;
}
static_assert(rows_ok(), "bc6h_mode_tables.inc: a row that does not tile its header");
}  // namespace bc6h_detail

#if defined(ICAMD_HOST_EMULATION)
static const bc6h_detail::Packed kBc6hModes = bc6h_detail::pack();
#else
__device__ __attribute__((aligned(8))) const bc6h_detail::Packed kBc6hModes = bc6h_detail::pack();
#endif

// ---- the value pipeline (include/ic_amd.h, "Decode")

// the low `bits` bits of v as a two's-complement number (1 <= bits <= 16)
ICAMD_DEV int32_t bc6h_sext(uint32_t v, uint32_t bits) { return (int32_t)(v << (32u - bits)) >> (32u - bits); }

template <bool SIGNED>
ICAMD_DEV int32_t bc6h_unquantise(int32_t c, uint32_t bits) {
  if (!SIGNED) {
    const uint32_t u = (uint32_t)c, top = (1u << bits) - 1u;
    if (bits >= 15u) return c;
    return u == 0u ? 0 : u == top ? 0xffff : (int32_t)(((u << 16) + 0x8000u) >> bits);
  }
  if (bits >= 16u) return c;
  const uint32_t a = (uint32_t)(c < 0 ? -c : c);
  const int32_t u = a == 0u ? 0 : a >= (1u << (bits - 1u)) - 1u ? 0x7fff : (int32_t)(((a << 15) + 0x4000u) >> (bits - 1u));
  return c < 0 ? -u : u;
}
ICAMD_DEV int32_t bc6h_interp(int32_t a, int32_t b, uint32_t w) { return (a * (int32_t)(64u - w) + b * (int32_t)w) >> 6; }
// the interpolated value -> the half's bit pattern
template <bool SIGNED>
ICAMD_DEV uint32_t bc6h_finish(int32_t x) {
  if (!SIGNED) return ((uint32_t)x * 31u) >> 6;
  return x < 0 ? (((uint32_t)(-x) * 31u) >> 5) | 0x8000u : ((uint32_t)x * 31u) >> 5;
}

// ---- decoder

// Block w[0..3] (its 16 bytes as dwords) -> rg[i] = R | G << 16, b[i] = B (half bit patterns), i = 4 y + x.
template <bool SIGNED>
ICAMD_DEV void decode_bc6h(const uint32_t w[4], uint32_t rg[16], uint32_t b[16]) {
  const uint32_t f = w[0];
  const uint32_t slot = (f & 2u) ? ((f & 1u) ? 10u : 2u) + ((f >> 2) & 7u) : (f & 1u);
  const uint32_t info = kBc6hModes.info[slot];
  const uint32_t keep = (info & 1u) ? 0xffffffffu : 0u;  // a reserved mode field: every lane runs the same code, the texels are 0
  const uint32_t ep = (info >> 4) & 31u;
  const bool transformed = ((info >> 21) & 1u) != 0u, two = ((info >> 22) & 1u) != 0u;
  Bc7Bits s = { (uint64_t)w[0] | (uint64_t)w[1] << 32, (uint64_t)w[2] | (uint64_t)w[3] << 32 };
  (void)bc7_take(s, (info >> 1) & 7u);
  uint64_t acc[3] = { 0u, 0u, 0u };
  uint32_t part = 0u;
  ICAMD_UNROLL
  for (int j = 0; j < bc6h_detail::kMaxRuns / 4; ++j) {
    const uint64_t four = kBc6hModes.runs[slot][j];
    ICAMD_UNROLL
    for (int k = 0; k < 4; ++k) {
      const uint32_t run = (uint32_t)(four >> (16 * k)) & 0xffffu, dest = run >> 4;
      const uint32_t v = bc7_take(s, run & 15u);
      const uint64_t x = (uint64_t)v << (dest & 63u);
      const uint32_t c = dest >> 6;
      acc[0] |= c == 0u ? x : 0u;
      acc[1] |= c == 1u ? x : 0u;
      acc[2] |= c == 2u ? x : 0u;
      part |= c == 3u ? v : 0u;
    }
  }
  int32_t U[3][4];  // [colour][endpoint], un-quantised
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    const uint32_t db = (info >> (9 + 4 * c)) & 15u, mask = (1u << ep) - 1u;
    const uint32_t raw0 = (uint32_t)acc[c] & 0xffffu;
    const int32_t e0 = SIGNED ? bc6h_sext(raw0, ep) : (int32_t)raw0;
    U[c][0] = bc6h_unquantise<SIGNED>(e0, ep);
    ICAMD_UNROLL
    for (int e = 1; e < 4; ++e) {
      const uint32_t raw = (uint32_t)(acc[c] >> (16 * e)) & 0xffffu;
      int32_t v;
      if (transformed) {  // wraps to the endpoint's width; then (signed format) read as a 16-bit number
        const uint32_t t = ((uint32_t)e0 + (uint32_t)bc6h_sext(raw, db)) & mask;
        v = SIGNED ? bc6h_sext(t, 16u) : (int32_t)t;
      } else {
        v = SIGNED ? bc6h_sext(raw, ep) : (int32_t)raw;
      }
      U[c][e] = bc6h_unquantise<SIGNED>(v, ep);
    }
  }
  const uint32_t p2 = two ? kBc7Partitions.w[part][1] : 0u;  // (bits 0..15: the subset of texel i; 16..19: the anchor)
  const uint32_t anchor = two ? (p2 >> 16) & 15u : 0u, ib = two ? 3u : 4u;
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const bool short_index = i == 0 || (uint32_t)i == anchor;
    const uint32_t idx = bc7_take(s, ib - (short_index ? 1u : 0u));
    const uint32_t wt = bc7_weight(idx, ib);
    const bool second = ((p2 >> i) & 1u) != 0u;
    uint32_t h[3];
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c)
      h[c] = bc6h_finish<SIGNED>(bc6h_interp(second ? U[c][2] : U[c][0], second ? U[c][3] : U[c][1], wt));
    rg[i] = (h[0] | h[1] << 16) & keep;
    b[i] = h[2] & keep;
  }
}

// ---- source samples
// The block at pixel (row, col) of an image of C (3 or 4) little-endian halves per pixel: rg[i] = R | G << 16, b[i] = B in the
// low half (the high half is not defined), i = 4 y + x.  Four row loads of 8 C bytes at any 2-byte alignment where the block
// lies inside the image, else the clamp-to-edge gather (also for the blocks of a padded grid).  PRECONDITION h, w >= 1.
template <int C>
ICAMD_DEV void bc6h_fetch(const uint8_t *img, uint32_t h, uint32_t w, uint32_t stride, uint32_t row, uint32_t col,
                          uint32_t rg[16], uint32_t b[16]) {
  if ((uint64_t)row + 4u <= h && (uint64_t)col + 4u <= w) {
    const uint8_t *p = img + (size_t)row * stride + (size_t)col * (2u * C);
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      const uint8_t *line = p + (size_t)y * stride;
      const U4 v = load_stream(reinterpret_cast<const U4 *>(line));
      if (C == 3) {  // R0 G0 | B0 R1 | G1 B1 | R2 G2 | B2 R3 | G3 B3
        const U2 u = load_stream(reinterpret_cast<const U2 *>(line + 16));
        rg[4 * y] = v.x;                          b[4 * y] = v.y;
        rg[4 * y + 1] = alignbit(v.z, v.y, 16u);  b[4 * y + 1] = v.z >> 16;
        rg[4 * y + 2] = v.w;                      b[4 * y + 2] = u.x;
        rg[4 * y + 3] = alignbit(u.y, u.x, 16u);  b[4 * y + 3] = u.y >> 16;
      } else {  // R0 G0 | B0 A0 | R1 G1 | B1 A1 | ...
        const U4 u = load_stream(reinterpret_cast<const U4 *>(line + 16));
        rg[4 * y] = v.x;      b[4 * y] = v.y;
        rg[4 * y + 1] = v.z;  b[4 * y + 1] = v.w;
        rg[4 * y + 2] = u.x;  b[4 * y + 2] = u.y;
        rg[4 * y + 3] = u.z;  b[4 * y + 3] = u.w;
      }
    }
  } else {
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      const uint8_t *line = img + (size_t)umin(row + (uint32_t)y, h - 1u) * stride;
      ICAMD_UNROLL
      for (int x = 0; x < 4; ++x) {
        const uint8_t *q = line + (size_t)umin(col + (uint32_t)x, w - 1u) * (2u * C);
        rg[4 * y + x] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        b[4 * y + x] = (uint32_t)q[4] | (uint32_t)q[5] << 8;
      }
    }
  }
}

// ---- the t domain (include/ic_amd.h, "Encode"): a half's bit pattern (the low 16 bits of h) -> an integer monotone in its value
template <bool SIGNED>
ICAMD_DEV int32_t bc6h_target(uint32_t h) {
  const uint32_t m = h & 0x7fffu;
  const int32_t t = m > 0x7c00u ? 0 : (int32_t)umin(m, 0x7bffu);
  if (!SIGNED) return (h & 0x8000u) ? 0 : t;
  return (h & 0x8000u) ? -t : t;
}

// D(q): the t-domain value the 10-bit endpoint q decodes to at weight 0 (q in 0..1023, or -511..511 in the signed format)
template <bool SIGNED>
ICAMD_DEV int32_t bc6h_endpoint_value(int32_t q) {
  const uint32_t hbits = bc6h_finish<SIGNED>(bc6h_unquantise<SIGNED>(q, 10u));
  return bc6h_target<SIGNED>(hbits);
}

// Step 2: the smallest q that minimises |D(q) - T|.  D is 31 q + 15 (unsigned, 0 < q < 1023) or sign(q) (62 |q| + 31)
// (signed, 0 < |q| < 511), so the minimum lies within one step of T / 31 or T / 62 (truncating): three candidates in ascending
// order, replaced on a strictly smaller distance only.  tests/test_bc6h_host.py holds this to the definition for every T.
template <bool SIGNED>
ICAMD_DEV int32_t bc6h_quantise(int32_t T) {
  const int32_t lo = SIGNED ? -511 : 0, hi = SIGNED ? 511 : 1023;
  const int32_t g = SIGNED ? T / 62 : T / 31;
  int32_t best_q = 0;
  uint32_t best = 0xffffffffu;
  ICAMD_UNROLL
  for (int d = -1; d <= 1; ++d) {
    const int32_t q = imin(imax(g + d, lo), hi);
    const int32_t e = bc6h_endpoint_value<SIGNED>(q) - T;
    const uint32_t a = (uint32_t)(e < 0 ? -e : e);
    if (a < best) {
      best = a;
      best_q = q;
    }
  }
  return best_q;
}

// Widths of step 3: a channel's difference is at most 31743 (unsigned) or 63486 (signed), its square below 2^32 either way;
// a texel's three squares sum to less than 2^32 in the unsigned format (3 * 31743^2 < 2^32) and to more than that in the signed
// one, where the sum is 64-bit.  The block's sse is 64-bit in both.
template <bool SIGNED>
struct Bc6hDist {
  typedef uint32_t type;
};
template <>
struct Bc6hDist<true> {
  typedef uint64_t type;
};

// Step 3.  t[p][c]: the texels' targets.  k_p in nibble p of idx.  The loop over k stays ROLLED (k is only ever arithmetic:
// the weight, the nibble written), the loop over the texels is unrolled, so the sixteen running minima and the 48 targets are
// named registers and the live state stays near 100 VGPRs; unrolling both makes the compiler spill.
template <bool SIGNED>
ICAMD_DEV uint64_t bc6h_search(const int32_t t[16][3], const int32_t E0[3], const int32_t E1[3], uint64_t &idx) {
  typedef typename Bc6hDist<SIGNED>::type dist_t;
  int32_t U0[3], U1[3];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    U0[c] = bc6h_unquantise<SIGNED>(E0[c], 10u);
    U1[c] = bc6h_unquantise<SIGNED>(E1[c], 10u);
  }
  dist_t best[16];
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) best[p] = ~(dist_t)0;
  uint32_t lo = 0u, hi = 0u;  // idx, texels 0..7 and 8..15
  ICAMD_NOUNROLL
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t w = (k * 64u + 7u) / 15u;  // (the 4-bit weights: bc7_detail::weights_ok)
    int32_t pal[3];
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) pal[c] = bc6h_target<SIGNED>(bc6h_finish<SIGNED>(bc6h_interp(U0[c], U1[c], w)));
    ICAMD_UNROLL
    for (int p = 0; p < 16; ++p) {
      dist_t d = 0;
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c) {
        const int32_t e = pal[c] - t[p][c];
        const uint32_t m = (uint32_t)(e < 0 ? -e : e);
        d += (dist_t)umad24(m, m, 0u);  // (m < 2^16.  UNSIGNED: in the signed format m^2 passes 2^31, which a signed product must not)
      }
      const bool better = d < best[p];  // (k ascends: the smallest k among equal distances stays)
      best[p] = better ? d : best[p];
      const uint32_t sh = 4u * (uint32_t)(p & 7), mask = ~(15u << sh);
      if (p < 8) lo = better ? (lo & mask) | k << sh : lo;
      else hi = better ? (hi & mask) | k << sh : hi;
    }
  }
  uint64_t sse = 0;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) sse += best[p];
  idx = (uint64_t)lo | (uint64_t)hi << 32;
  return sse;
}

// floor(N / D) for N >= 0, clamped to 32767: the largest v in 0..32767 with v D <= N, bit by bit.  D < 2^32.
ICAMD_DEV uint32_t bc6h_div15(uint64_t N, uint64_t D) {
  uint32_t v = 0;
  ICAMD_UNROLL
  for (uint32_t bit = 1u << 14; bit; bit >>= 1)
    if ((uint64_t)(v | bit) * D <= N) v |= bit;
  return v;
}
// clamp(floor(N / D), SIGNED ? -0x7BFF : 0, 0x7BFF), D > 0
template <bool SIGNED>
ICAMD_DEV int32_t bc6h_floor_div_clamped(int64_t N, uint64_t D) {
  if (N >= 0) return (int32_t)umin(bc6h_div15((uint64_t)N, D), 0x7bffu);
  if (!SIGNED) return 0;
  return -(int32_t)umin(bc6h_div15((uint64_t)(-N) + D - 1u, D), 0x7bffu);  // floor of a negative quotient = -ceil(|N| / D)
}

// rg / b: the block's sixteen pixels as bc6h_fetch hands them.  out: the 16 bytes of the definition's block.  Returns the
// block's final sse (step 4's; bc6h_modes_block.h compares its candidate with it).
template <bool SIGNED>
ICAMD_DEV uint64_t encode_bc6h_sse(const uint32_t rg[16], const uint32_t b[16], uint32_t out[4]) {
  int32_t t[16][3];
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    t[i][0] = bc6h_target<SIGNED>(rg[i] & 0xffffu);
    t[i][1] = bc6h_target<SIGNED>(rg[i] >> 16);
    t[i][2] = bc6h_target<SIGNED>(b[i] & 0xffffu);
  }
  // step 1
  int32_t lo[3], hi[3], sum[3];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    lo[c] = hi[c] = sum[c] = t[0][c];
    ICAMD_UNROLL
    for (int i = 1; i < 16; ++i) {
      lo[c] = imin(lo[c], t[i][c]);
      hi[c] = imax(hi[c], t[i][c]);
      sum[c] += t[i][c];
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
  int64_t cross[3] = { 0, 0, 0 };
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const int32_t star = cs == 0u ? t[i][0] : cs == 1u ? t[i][1] : t[i][2];
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) cross[c] += (int64_t)star * t[i][c];  // (|product| < 2^30; sixteen of them: 64 bits)
  }
  const int32_t sum_star = cs == 0u ? sum[0] : cs == 1u ? sum[1] : sum[2];
  int32_t T0[3], T1[3];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    const int64_t cov = 16 * cross[c] - (int64_t)sum_star * sum[c];
    const bool flip = cov < 0 && (uint32_t)c != cs;
    T0[c] = flip ? hi[c] : lo[c];
    T1[c] = flip ? lo[c] : hi[c];
  }
  // steps 2, 3
  int32_t E0[3], E1[3];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    E0[c] = bc6h_quantise<SIGNED>(T0[c]);
    E1[c] = bc6h_quantise<SIGNED>(T1[c]);
  }
  uint64_t idx;
  uint64_t sse = bc6h_search<SIGNED>(t, E0, E1, idx);
  // step 4
  uint32_t a = 0, bb = 0, c2 = 0;
  int32_t Y[3] = { 0, 0, 0 };
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const uint32_t w = bc7_weight4((uint32_t)(idx >> (4 * i)) & 15u);
    a += (64u - w) * (64u - w);
    bb += (64u - w) * w;
    c2 += w * w;
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) Y[c] += (int32_t)w * t[i][c];  // (|sum| <= 16 * 64 * 31743 < 2^25)
  }
  const uint32_t det = a * c2 - bb * bb;  // (as BC7: a c <= 2^30 and >= b^2)
  if (det != 0u) {
    int32_t F0[3], F1[3];
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) {
      const int64_t X = (int64_t)(64 * sum[c] - Y[c]), Yc = (int64_t)Y[c];
      const int64_t n0 = 64 * ((int64_t)c2 * X - (int64_t)bb * Yc), n1 = 64 * ((int64_t)a * Yc - (int64_t)bb * X);
      // rdiv(n, det) = floor((2 n + det) / (2 det)), clamped to the format's range
      F0[c] = bc6h_quantise<SIGNED>(bc6h_floor_div_clamped<SIGNED>(2 * n0 + (int64_t)det, 2ull * det));
      F1[c] = bc6h_quantise<SIGNED>(bc6h_floor_div_clamped<SIGNED>(2 * n1 + (int64_t)det, 2ull * det));
    }
    uint64_t idx2;
    const uint64_t sse2 = bc6h_search<SIGNED>(t, F0, F1, idx2);
    if (sse2 < sse) {
      sse = sse2;
      idx = idx2;
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c) {
        E0[c] = F0[c];
        E1[c] = F1[c];
      }
    }
  }
  // step 5
  if ((idx & 15u) >= 8u) {
    idx = ~idx;
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) {
      const int32_t q = E0[c];
      E0[c] = E1[c];
      E1[c] = q;
    }
  }
  // step 6: mode field 00011; rw gw bw rx gx bx, 10 bits each (two's complement); k_0 in 3 bits; k_1..k_15 in 4 bits each
  uint64_t lo64 = 3u;
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    lo64 |= (uint64_t)((uint32_t)E0[c] & 1023u) << (5 + 10 * c);
    lo64 |= (uint64_t)((uint32_t)E1[c] & 1023u) << (35 + 10 * c);
  }
  const uint64_t hi64 = (idx & ~15ull) | (uint64_t)((uint32_t)idx & 7u) << 1 | (((uint32_t)E1[2] >> 9) & 1u);
  out[0] = (uint32_t)lo64;
  out[1] = (uint32_t)(lo64 >> 32);
  out[2] = (uint32_t)hi64;
  out[3] = (uint32_t)(hi64 >> 32);
  return sse;
}
template <bool SIGNED>
ICAMD_DEV void encode_bc6h(const uint32_t rg[16], const uint32_t b[16], uint32_t out[4]) {
  (void)encode_bc6h_sse<SIGNED>(rg, b, out);
}

// ---- metric
// Sums of squared differences and largest absolute differences of channel k (0 = R, 1 = G, 2 = B) in the t domain, decoded half
// against source half.  A squared difference is below 2^32, so a lane's sums are 64-bit.
struct Bc6hAcc {
  uint64_t sse[3];
  uint32_t mx[3];
};
ICAMD_DEV void bc6h_clear(Bc6hAcc &a) {
  ICAMD_UNROLL
  for (int k = 0; k < 3; ++k) {
    a.sse[k] = 0u;
    a.mx[k] = 0u;
  }
}

// The block w at pixel (row, col) against the C-half source pixels there; only the texels inside the image count.
// PRECONDITION row < h, col < wd.
template <int C, bool SIGNED>
ICAMD_DEV void metric_bc6h_block(const uint32_t w[4], const uint8_t *img, uint32_t h, uint32_t wd, uint32_t stride, uint32_t row,
                                 uint32_t col, Bc6hAcc &a) {
  uint32_t srg[16], sb[16], drg[16], db[16];
  bc6h_fetch<C>(img, h, wd, stride, row, col, srg, sb);
  decode_bc6h<SIGNED>(w, drg, db);
  const uint32_t cols = umin(wd - col, 4u), rows = umin(h - row, 4u);
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const bool inside = (uint32_t)(i & 3) < cols && (uint32_t)(i >> 2) < rows;
    ICAMD_UNROLL
    for (int k = 0; k < 3; ++k) {
      const uint32_t sv = k == 0 ? srg[i] & 0xffffu : k == 1 ? srg[i] >> 16 : sb[i] & 0xffffu;
      const uint32_t dv = k == 0 ? drg[i] & 0xffffu : k == 1 ? drg[i] >> 16 : db[i] & 0xffffu;
      const int32_t d = bc6h_target<SIGNED>(dv) - bc6h_target<SIGNED>(sv);
      const uint32_t e = inside ? (uint32_t)(d < 0 ? -d : d) : 0u;
      a.sse[k] += (uint64_t)(e * e);  // (e <= 63486: the product fits 32 bits)
      a.mx[k] = umax(a.mx[k], e);
    }
  }
}

}  // namespace icamd
#endif  // ICAMD_BC6H_BLOCK_H_
