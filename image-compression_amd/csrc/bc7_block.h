// bc7_block.h -- BC7 (BPTC) block math (EXTENSION, include/ic_amd.h ICAMD_BC7): the decoder of all eight modes
// and the mode-6 encoder whose definition is stated in include/ic_amd.h and restated in tests/bc7_oracle.py.  One block per
// lane, everything in registers, integer only.  Texel i = 4 y + x (row-major; the ETC headers use 4 x + y).
//
// Tables: the partition / anchor tables of the specification (bc7_partition_tables.inc, data) are packed at compile time into
// 64 entries of 8 bytes -- the 3-subset row as 16 x 2 bits, the 2-subset row as 16 x 1 bit, the three anchors as nibbles --
// and a lane loads ITS entry with one 8-byte load at a per-lane index (a __device__ const table: 512 bytes, four lines that
// stay in the vector L1; as kDxt5AlphaIndex of dxt_block.h).  LDS staging would cost every workgroup a copy and a barrier for
// one lookup per block.  The weight tables are immediates (bytes of 64-bit constants), selected by shifts.
#ifndef ICAMD_BC7_BLOCK_H_
#define ICAMD_BC7_BLOCK_H_

#include "ic_device.h"

namespace icamd {

namespace bc7_detail {
constexpr uint8_t kP2[64][16] = {
#define ICAMD_BC7_TABLE_P2
#include "bc7_partition_tables.inc"
#undef ICAMD_BC7_TABLE_P2
};
constexpr uint8_t kP3[64][16] = {
#define ICAMD_BC7_TABLE_P3
#include "bc7_partition_tables.inc"
#undef ICAMD_BC7_TABLE_P3
};
constexpr uint8_t kA2[64] = {
#define ICAMD_BC7_TABLE_A2
#include "bc7_partition_tables.inc"
#undef ICAMD_BC7_TABLE_A2
};
constexpr uint8_t kA3A[64] = {
#define ICAMD_BC7_TABLE_A3A
#include "bc7_partition_tables.inc"
#undef ICAMD_BC7_TABLE_A3A
};
constexpr uint8_t kA3B[64] = {
#define ICAMD_BC7_TABLE_A3B
#include "bc7_partition_tables.inc"
#undef ICAMD_BC7_TABLE_A3B
};
// entry s: w[s][0] = 3-subset row, texel i in bits 2 i .. 2 i + 1; w[s][1] = 2-subset row (bit i) | 2-subset anchor << 16 |
// second 3-subset anchor << 20 | third 3-subset anchor << 24
struct Packed {
  uint32_t w[64][2];
};
constexpr Packed pack() {
  Packed t = {};
  for (int s = 0; s < 64; ++s) {
    uint32_t p3 = 0, p2 = 0;
    for (int i = 0; i < 16; ++i) {
      p3 |= (uint32_t)kP3[s][i] << (2 * i);
      p2 |= (uint32_t)kP2[s][i] << i;
    }
    t.w[s][0] = p3;
    t.w[s][1] = p2 | (uint32_t)kA2[s] << 16 | (uint32_t)kA3A[s] << 20 | (uint32_t)kA3B[s] << 24;
  }
  return t;
}
constexpr bool anchors_lie_in_their_subsets() {
  for (int s = 0; s < 64; ++s)
    if (kP2[s][0] != 0 || kP3[s][0] != 0 || kP2[s][kA2[s]] != 1 || kP3[s][kA3A[s]] != 1 || kP3[s][kA3B[s]] != 2) return false;
  return true;
}
static_assert(anchors_lie_in_their_subsets(), "bc7_partition_tables.inc: an anchor outside its subset");
}  // namespace bc7_detail

#if defined(ICAMD_HOST_EMULATION)
static const bc7_detail::Packed kBc7Partitions = bc7_detail::pack();
#else
__device__ __attribute__((aligned(8))) const bc7_detail::Packed kBc7Partitions = bc7_detail::pack();
#endif

// Weight w_idx of the `bits`-bit index (bits 2, 3 or 4): bytes of immediates.
constexpr uint64_t kBc7W2 = 0x402b1500ull, kBc7W3 = 0x40372e251b120900ull;
constexpr uint64_t kBc7W4Lo = 0x1e1a15110d090400ull, kBc7W4Hi = 0x403c37332f2b2622ull;
ICAMD_DEV uint32_t bc7_weight4(uint32_t idx) { return (uint32_t)(((idx & 8u) ? kBc7W4Hi : kBc7W4Lo) >> (8u * (idx & 7u))) & 0xffu; }
ICAMD_DEV uint32_t bc7_weight(uint32_t idx, uint32_t bits) {
  const uint64_t t = bits == 2u ? kBc7W2 : bits == 3u ? kBc7W3 : (idx & 8u) ? kBc7W4Hi : kBc7W4Lo;
  return (uint32_t)(t >> (8u * (idx & 7u))) & 0xffu;
}
namespace bc7_detail {
constexpr bool weights_ok() {
  for (uint32_t i = 0; i < 16; ++i) {
    const uint32_t w4 = (uint32_t)(((i & 8u) ? kBc7W4Hi : kBc7W4Lo) >> (8u * (i & 7u))) & 0xffu;
    if (w4 != (i * 64u + 7u) / 15u) return false;
    if (i < 8 && ((uint32_t)(kBc7W3 >> (8u * i)) & 0xffu) != (i * 64u + 3u) / 7u) return false;
    if (i < 4 && ((uint32_t)(kBc7W2 >> (8u * i)) & 0xffu) != (i * 64u + 1u) / 3u) return false;
  }
  return true;
}
static_assert(weights_ok(), "BC7 weight immediates");
}  // namespace bc7_detail

// ---- decoder

// The block as a 128-bit shift register: take(n) returns the lowest n bits (n = 0..8; 0 takes nothing) and drops them.
struct Bc7Bits {
  uint64_t lo, hi;
};
ICAMD_DEV uint32_t bc7_take(Bc7Bits &b, uint32_t n) {
  const uint32_t v = (uint32_t)b.lo & ((1u << n) - 1u);
  b.lo = (b.lo >> n) | ((b.hi << 1) << (63u - n));
  b.hi >>= n;
  return v;
}
// nibble m of a per-mode constant
ICAMD_DEV uint32_t bc7_mode_field(uint32_t packed, uint32_t mode) { return (packed >> (4u * mode)) & 15u; }

ICAMD_DEV uint32_t bc7_interp(uint32_t e0, uint32_t e1, uint32_t w) { return ((64u - w) * e0 + w * e1 + 32u) >> 6; }

// Block w[0..3] (its 16 bytes as dwords) -> px[i], i = 4 y + x: R | G << 8 | B << 16 | A << 24 (R and B exchanged with swap).
ICAMD_DEV void decode_bc7(const uint32_t w[4], bool swap, uint32_t px[16]) {
  const uint32_t byte0 = w[0] & 0xffu;
  if (byte0 == 0u) {  // reserved
    ICAMD_UNROLL
    for (int i = 0; i < 16; ++i) px[i] = 0u;
    return;
  }
  const uint32_t mode = (uint32_t)__builtin_ctz(byte0);
  // per mode (nibble m): subsets, partition bits, rotation bits, colour bits, alpha bits, index bits, secondary index bits
  const uint32_t ns = bc7_mode_field(0x21112323u, mode), pbits = bc7_mode_field(0x60006664u, mode);
  const uint32_t rbits = bc7_mode_field(0x00220000u, mode), cb = bc7_mode_field(0x57757564u, mode);
  const uint32_t ab = bc7_mode_field(0x57860000u, mode), ib = bc7_mode_field(0x24222233u, mode);
  const uint32_t ib2 = bc7_mode_field(0x00230000u, mode);
  const bool unique_p = ((0xc9u >> mode) & 1u) != 0u, shared_p = mode == 1u;  // modes 0, 3, 6, 7: one p-bit per endpoint
  const uint32_t has_p = (unique_p || shared_p) ? 1u : 0u;
  Bc7Bits b = { (uint64_t)w[0] | (uint64_t)w[1] << 32, (uint64_t)w[2] | (uint64_t)w[3] << 32 };
  (void)bc7_take(b, mode + 1u);
  const uint32_t part = bc7_take(b, pbits), rot = bc7_take(b, rbits), sel = bc7_take(b, mode == 4u ? 1u : 0u);
  const uint32_t ne = 2u * ns;
  uint32_t ep[6][4], pb[6];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c)
    ICAMD_UNROLL
    for (int e = 0; e < 6; ++e) ep[e][c] = bc7_take(b, (uint32_t)e < ne ? cb : 0u);
  ICAMD_UNROLL
  for (int e = 0; e < 6; ++e) ep[e][3] = bc7_take(b, (uint32_t)e < ne ? ab : 0u);
  ICAMD_UNROLL
  for (int e = 0; e < 6; ++e) pb[e] = bc7_take(b, ((uint32_t)e < ne && unique_p) ? 1u : 0u);
  if (shared_p) {  // mode 1: one p-bit per subset
    pb[0] = pb[1] = bc7_take(b, 1u);
    pb[2] = pb[3] = bc7_take(b, 1u);
  }
  uint32_t E[6];
  ICAMD_UNROLL
  for (int e = 0; e < 6; ++e) {
    uint32_t v[4];
    ICAMD_UNROLL
    for (int c = 0; c < 4; ++c) {
      const uint32_t bits = (c == 3 ? ab : cb) + has_p;
      uint32_t x = has_p ? (ep[e][c] << 1 | pb[e]) : ep[e][c];
      x <<= 8u - bits;
      v[c] = (x | x >> bits) & 0xffu;
    }
    if (ab == 0u) v[3] = 255u;
    E[e] = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
  }
  const uint32_t p3 = kBc7Partitions.w[part][0], p2 = kBc7Partitions.w[part][1];
  const uint32_t a1 = ns == 2u ? (p2 >> 16) & 15u : ns == 3u ? (p2 >> 20) & 15u : 0u, a2 = ns == 3u ? (p2 >> 24) & 15u : 0u;
  uint64_t idx1 = 0, idx2 = 0;
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const bool anchor = i == 0 || (uint32_t)i == a1 || (uint32_t)i == a2;
    idx1 |= (uint64_t)bc7_take(b, ib - (anchor ? 1u : 0u)) << (4 * i);
  }
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) idx2 |= (uint64_t)bc7_take(b, ib2 ? ib2 - (i == 0 ? 1u : 0u) : 0u) << (4 * i);
  if (ib2 == 0u) idx2 = idx1;
  const uint32_t bits2 = ib2 ? ib2 : ib;
  const uint32_t cbits = sel ? bits2 : ib, abits = sel ? ib : bits2;
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const uint32_t s = ns == 3u ? (p3 >> (2 * i)) & 3u : ns == 2u ? (p2 >> i) & 1u : 0u;
    const uint32_t e0 = s == 0u ? E[0] : s == 1u ? E[2] : E[4], e1 = s == 0u ? E[1] : s == 1u ? E[3] : E[5];
    const uint32_t i1 = (uint32_t)(idx1 >> (4 * i)) & 15u, i2 = (uint32_t)(idx2 >> (4 * i)) & 15u;
    const uint32_t wc = bc7_weight(sel ? i2 : i1, cbits), wa = bc7_weight(sel ? i1 : i2, abits);
    uint32_t r = bc7_interp(e0 & 0xffu, e1 & 0xffu, wc), g = bc7_interp((e0 >> 8) & 0xffu, (e1 >> 8) & 0xffu, wc);
    uint32_t bl = bc7_interp((e0 >> 16) & 0xffu, (e1 >> 16) & 0xffu, wc), a = bc7_interp(e0 >> 24, e1 >> 24, wa);
    if (rot == 1u) { const uint32_t t = r; r = a; a = t; }
    else if (rot == 2u) { const uint32_t t = g; g = a; a = t; }
    else if (rot == 3u) { const uint32_t t = bl; bl = a; a = t; }
    px[i] = swap ? (bl | g << 8 | r << 16 | a << 24) : (r | g << 8 | bl << 16 | a << 24);
  }
}

// ---- encoder (mode 6; the definition's steps are numbered in include/ic_amd.h)

ICAMD_DEV uint32_t bc7_ch(uint32_t v, int c) { return (v >> (8 * c)) & 0xffu; }

// Step 2: four targets -> the endpoint E (bytes E_c = 2 q_c + p), p shared by the channels.
ICAMD_DEV uint32_t bc7_quantise(const uint32_t T[4]) {
  uint32_t e[2] = { 0u, 0u }, err[2] = { 0u, 0u };
  ICAMD_UNROLL
  for (uint32_t p = 0; p < 2; ++p)
    ICAMD_UNROLL
    for (int c = 0; c < 4; ++c) {
      const uint32_t v = 2u * umin((T[c] - p + 1u) >> 1, 127u) + p;
      const int32_t d = (int32_t)v - (int32_t)T[c];
      err[p] += (uint32_t)(d * d);
      e[p] |= v << (8 * c);
    }
  return err[1] < err[0] ? e[1] : e[0];
}

// Step 3.  sum_c (pal_k[c] - v[c])^2 = |v|^2 + |pal_k|^2 - 2 pal_k . v: per texel the k with the largest
// 2 pal_k . v + (2^19 - |pal_k|^2), both sides exact integers (|pal_k|^2, pal_k . v <= 4 * 255^2 < 2^18); the key holds that
// score above 15 - k, so one unsigned maximum takes the smallest k among equal scores.  inv: 15 - k_p in nibble p.
ICAMD_DEV uint32_t bc7_search(const uint32_t v[16], uint32_t E0, uint32_t E1, uint64_t &inv) {
  const uint32_t rb0 = E0 & 0x00ff00ffu, ga0 = (E0 >> 8) & 0x00ff00ffu, rb1 = E1 & 0x00ff00ffu, ga1 = (E1 >> 8) & 0x00ff00ffu;
  uint32_t pal[16], bias[16];
  ICAMD_UNROLL
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t w = (k * 64u + 7u) / 15u;  // (the 4-bit weights: bc7_detail::weights_ok)
    // two channels per product on 16-bit lanes: 64 * 255 + 32 < 2^16
    const uint32_t rb = (((64u - w) * rb0 + w * rb1 + 0x00200020u) >> 6) & 0x00ff00ffu;
    const uint32_t ga = (((64u - w) * ga0 + w * ga1 + 0x00200020u) >> 6) & 0x00ff00ffu;
    pal[k] = rb | ga << 8;
    bias[k] = (((1u << 19) - udot4(pal[k], pal[k], 0u)) << 4) | (15u - k);
  }
  uint32_t sse = 0;
  inv = 0;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) {
    uint32_t best = 0;
    ICAMD_UNROLL
    for (int k = 0; k < 16; ++k) best = umax(best, (udot4(pal[k], v[p], 0u) << 5) + bias[k]);
    inv |= (uint64_t)(best & 15u) << (4 * p);
    sse += udot4(v[p], v[p], 1u << 19) - (best >> 4);
  }
  return sse;
}

// floor(N / D) for 0 <= N, clamped to 255: the largest t in 0..255 with t D <= N, bit by bit.  D < 2^32.
ICAMD_DEV uint32_t bc7_div255(uint64_t N, uint64_t D) {
  uint32_t t = 0;
  ICAMD_UNROLL
  for (uint32_t bit = 128u; bit; bit >>= 1)
    if ((uint64_t)(t | bit) * D <= N) t |= bit;
  return t;
}

// px: the block's sixteen pixels as load_block hands them (byte k = the source's k-th byte; byte 3 undefined for COMPS = 3).
template <int COMPS>
ICAMD_DEV void encode_bc7(const uint32_t px[16], bool swap, uint32_t out[4]) {
  uint32_t v[16];
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    uint32_t t = COMPS == 4 ? px[i] : (px[i] | 0xff000000u);
    if (swap) t = (t & 0xff00ff00u) | ((t >> 16) & 0xffu) | ((t & 0xffu) << 16);
    v[i] = t;
  }
  // step 1
  uint32_t lo[4], hi[4], sum[4];
  ICAMD_UNROLL
  for (int c = 0; c < 4; ++c) {
    lo[c] = 255u;
    hi[c] = sum[c] = 0u;
    ICAMD_UNROLL
    for (int i = 0; i < 16; ++i) {
      const uint32_t x = bc7_ch(v[i], c);
      lo[c] = umin(lo[c], x);
      hi[c] = umax(hi[c], x);
      sum[c] += x;
    }
  }
  uint32_t cs = 0, widest = hi[0] - lo[0];
  ICAMD_UNROLL
  for (int c = 1; c < 4; ++c)
    if (hi[c] - lo[c] > widest) {
      widest = hi[c] - lo[c];
      cs = (uint32_t)c;
    }
  uint32_t cross[4] = { 0u, 0u, 0u, 0u };
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const uint32_t star = (v[i] >> (8u * cs)) & 0xffu;
    ICAMD_UNROLL
    for (int c = 0; c < 4; ++c) cross[c] += star * bc7_ch(v[i], c);
  }
  const uint32_t sum_star = cs == 0u ? sum[0] : cs == 1u ? sum[1] : cs == 2u ? sum[2] : sum[3];
  uint32_t T0[4], T1[4];
  ICAMD_UNROLL
  for (int c = 0; c < 4; ++c) {
    const int32_t cov = (int32_t)(16u * cross[c]) - (int32_t)(sum_star * sum[c]);  // both below 2^25
    const bool flip = cov < 0 && (uint32_t)c != cs;
    T0[c] = flip ? hi[c] : lo[c];
    T1[c] = flip ? lo[c] : hi[c];
  }
  // steps 2, 3
  uint32_t E0 = bc7_quantise(T0), E1 = bc7_quantise(T1);
  uint64_t inv;
  uint32_t sse = bc7_search(v, E0, E1, inv);
  // step 4
  uint32_t a = 0, b = 0, c2 = 0, Y[4] = { 0u, 0u, 0u, 0u };
  ICAMD_UNROLL
  for (int i = 0; i < 16; ++i) {
    const uint32_t w = bc7_weight4(15u - ((uint32_t)(inv >> (4 * i)) & 15u));
    a += (64u - w) * (64u - w);
    b += (64u - w) * w;
    c2 += w * w;
    ICAMD_UNROLL
    for (int c = 0; c < 4; ++c) Y[c] += w * bc7_ch(v[i], c);
  }
  const uint32_t det = a * c2 - b * b;  // a c <= ((a + c) / 2)^2 <= 2^30, and >= b^2 (Cauchy-Schwarz)
  if (det != 0u) {
    ICAMD_UNROLL
    for (int c = 0; c < 4; ++c) {
      const int64_t X = (int64_t)(64u * sum[c] - Y[c]), Yc = (int64_t)Y[c];
      const int64_t n0 = 64 * ((int64_t)c2 * X - (int64_t)b * Yc), n1 = 64 * ((int64_t)a * Yc - (int64_t)b * X);
      const int64_t N0 = 2 * n0 + (int64_t)det, N1 = 2 * n1 + (int64_t)det;  // rdiv: floor(N / (2 det)), negative -> clamped to 0
      T0[c] = N0 < 0 ? 0u : bc7_div255((uint64_t)N0, 2ull * det);
      T1[c] = N1 < 0 ? 0u : bc7_div255((uint64_t)N1, 2ull * det);
    }
    const uint32_t F0 = bc7_quantise(T0), F1 = bc7_quantise(T1);
    uint64_t inv2;
    const uint32_t sse2 = bc7_search(v, F0, F1, inv2);
    if (sse2 < sse) {
      sse = sse2;
      E0 = F0;
      E1 = F1;
      inv = inv2;
    }
  }
  // step 5: k_0 >= 8 iff 15 - k_0 < 8
  uint64_t k = ~inv;
  if ((inv & 15u) < 8u) {
    const uint32_t t = E0;
    E0 = E1;
    E1 = t;
    k = inv;
  }
  // step 6
  uint64_t lo64 = 0x40u;
  ICAMD_UNROLL
  for (int c = 0; c < 4; ++c) {
    lo64 |= (uint64_t)(bc7_ch(E0, c) >> 1) << (7 + 14 * c);
    lo64 |= (uint64_t)(bc7_ch(E1, c) >> 1) << (14 + 14 * c);
  }
  lo64 |= (uint64_t)(E0 & 1u) << 63;
  const uint64_t hi64 = (k & ~15ull) | (uint64_t)((uint32_t)k & 7u) << 1 | (E1 & 1u);
  out[0] = (uint32_t)lo64;
  out[1] = (uint32_t)(lo64 >> 32);
  out[2] = (uint32_t)hi64;
  out[3] = (uint32_t)(hi64 >> 32);
}

}  // namespace icamd
#endif  // ICAMD_BC7_BLOCK_H_
