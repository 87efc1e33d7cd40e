// etc2_a1_block.h -- ETC2 RGB8 with punch-through alpha (EXTENSION, include/ic_amd.h ICAMD_ETC2_RGB8A1), one
// block per lane: the decoder on top of decode_etc2_colour, the masked differential search D, and the per-block choice of the
// encoder.  Integers only, no memory tables.
//
// The word has the fields of ICAMD_ETC2_RGB8 (etc2_colour_block.h) with bit 33 as the OPAQUE bit Op instead of the diff bit:
// there is no individual mode, s_c = 5-bit base + sign-extended 3-bit delta of byte c decides T / H / planar / differential
// whatever Op.  With Op = 1 a word decodes as the ICAMD_ETC2_RGB8 word with the same bits and alpha 255.  With Op = 0 the
// texels of index k = 2 (differential, T and H; not planar) are (0, 0, 0, 0) and the differential modifiers are {0, +b, -, -b}.
//
// The encoder is a DEFINITION (include/ic_amd.h states it in full).  A texel is transparent iff its byte 3 is < 128.
//   all 16 transparent: 00 00 00 00 ff ff 00 00;
//   none transparent:   C = the ETC1 word E where E is differential, else D(no mask, Op = 1, E's flip bit); the block is
//                       etc2_rgb8_choose(px, C), so wherever E is differential the bytes are ICAMD_ETC2_RGB8's;
//   otherwise:          D(mask, Op = 0) over the partitions of the strategy, the smaller error wins, a tie keeps flip 0.
// D on one partition: per sub-block q5 = floor(sum of the opaque texels / (8 n)) per channel (an empty sub-block takes the
// other's); per channel d = q5(S1) - q5(S0), c = clamp(d, -4, 3), a' = q5(S0) + (d - c) / 2 truncating, the word stores a' and
// c; per sub-block the table t = 0..7 with the smallest summed squared RGB error, every opaque texel at the allowed index
// closest to it (ties: the smallest index, the smallest t), transparent texels at index 2 without error.
#ifndef ICAMD_ETC2_A1_BLOCK_H_
#define ICAMD_ETC2_A1_BLOCK_H_

#include "etc1_block.h"         // kEtcModA_lo ... (the modifier tables a, b)
#include "etc2_colour_block.h"  // decode_etc2_colour, etc2_rgb8_choose
#include "ic_device.h"

namespace icamd {

// The 4 x 4 bit matrices in both halves of v transposed: bit 4 a + b <-> bit 4 b + a (and 16 + ...).
ICAMD_DEV uint32_t etc2_a1_transpose4x4(uint32_t v) {
  return (v & 0x84218421u) | (v & 0x08420842u) << 3 | (v & 0x00840084u) << 6 | (v & 0x00080008u) << 9 |
         ((v >> 3) & 0x08420842u) | ((v >> 6) & 0x00840084u) | ((v >> 9) & 0x00080008u);
}

// ---- decoder

// w0, w1: the 8 block bytes as little-endian dwords.  px[4 y + x] = R | G << 8 | B << 16 | A << 24; swap: stored R goes to the
// third byte, as decode_etc2_rgba8 does.
ICAMD_DEV void decode_etc2_a1(uint32_t w0, uint32_t w1, bool swap, uint32_t px[16]) {
  const uint32_t hi = perm(0u, w0, 0x00010203u) | 2u, lo = perm(0u, w1, 0x00010203u);
  const bool punch = !(w0 & 0x02000000u);         // Op = 0 (bit 33 is bit 1 of byte 3)
  decode_etc2_colour(w0 | 0x02000000u, w1, px);   // Op = 1: the RGB8 word with the same bits
  const uint32_t mode = etc2_colour_mode(hi);
  uint32_t base[2] = { 0u, 0u };  // Op = 0, differential: index 0 is the sub-block's base colour itself
  ICAMD_UNROLL
  for (int ch = 0; ch < 3; ++ch) {
    const uint32_t b5 = (hi >> (27 - 8 * ch)) & 31u, d3 = (hi >> (24 - 8 * ch)) & 7u;
    const uint32_t s5 = (b5 + ((d3 ^ 4u) - 4u)) & 31u;
    base[0] |= (b5 << 3 | b5 >> 2) << (8 * ch);
    base[1] |= (s5 << 3 | s5 >> 2) << (8 * ch);
  }
  const bool differential = mode == 0u, holes = punch && mode != 3u;
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    ICAMD_UNROLL
    for (int x = 0; x < 4; ++x) {
      const int p = 4 * x + y;
      const uint32_t k = ((lo >> p) & 1u) | ((lo >> (p + 16)) & 1u) << 1;
      const bool second = (hi & 1u) ? y >= 2 : x >= 2;
      uint32_t c = px[4 * y + x];
      c = (holes && differential && k == 0u) ? (second ? base[1] : base[0]) : c;
      c |= 0xff000000u;
      c = (holes && k == 2u) ? 0u : c;
      px[4 * y + x] = swap ? perm(c, c, 0x03000102u) : c;
    }
  }
}

// ---- D, the masked differential search

// floor(sum / (8 n)) for n = 1..8 opaque texels and sum <= 255 n as one multiply: recip = ceil(2^20 / (8 n)); n = 8 is ETC1's
// sum >> 6.  Checked for every reachable argument below.
constexpr uint32_t etc2_a1_recip(uint32_t n) { return ((1u << 20) + 8u * n - 1u) / (8u * n); }
namespace detail {
constexpr bool check_a1_q5() {
  for (uint32_t n = 1; n <= 8u; ++n)
    for (uint32_t sum = 0; sum <= 255u * n; ++sum)
      if ((sum * etc2_a1_recip(n)) >> 20 != sum / (8u * n) || sum * etc2_a1_recip(n) >= (1u << 31)) return false;
  return etc2_a1_recip(8u) == 1u << 14;
}
static_assert(check_a1_q5(), "q5 of 1..8 opaque texels");
}  // namespace detail

struct EtcA1Result {
  uint32_t err;     // summed squared RGB error over the opaque texels
  uint32_t hi, lo;  // the word's halves (bits 63..32, 31..0)
};

// One partition.  q[j]: the texels in sub-block order (j < 8: sub-block 0), byte 3 zero; opaque16: bit j = texel j is opaque;
// op: the word's opaque bit (opaque16 is 0xffff then).  Returns hi without the flip bit and lo with bit j / 16 + j = the index
// bits of texel j.
ICAMD_DEV EtcA1Result etc2_a1_search(const uint32_t q[16], uint32_t opaque16, bool op) {
  // bases
  uint32_t q5[2][3], qq[2];
  uint32_t n[2];
  ICAMD_UNROLL
  for (int s = 0; s < 2; ++s) {
    uint32_t rb = 0u, g = 0u, cnt = 0u, sq = 0u;
    ICAMD_UNROLL
    for (int j = 0; j < 8; ++j) {
      const uint32_t v = ((opaque16 >> (8 * s + j)) & 1u) ? q[8 * s + j] : 0u;
      rb += v & 0x00ff00ffu;
      g += (v >> 8) & 0xffu;
      cnt += (opaque16 >> (8 * s + j)) & 1u;
      sq = udot4(v, v, sq);
    }
    uint32_t recip = etc2_a1_recip(8u);
    ICAMD_UNROLL
    for (uint32_t k = 1; k < 8u; ++k) recip = cnt == k ? etc2_a1_recip(k) : recip;
    q5[s][0] = umad24(rb & 0xffffu, recip, 0u) >> 20;
    q5[s][1] = umad24(g, recip, 0u) >> 20;
    q5[s][2] = umad24(rb >> 16, recip, 0u) >> 20;
    n[s] = cnt;
    qq[s] = sq;
  }
  uint32_t hi = op ? 2u : 0u;
  int32_t base[2][3];
  ICAMD_UNROLL
  for (int ch = 0; ch < 3; ++ch) {
    const int32_t q0 = (int32_t)(n[0] == 0u ? q5[1][ch] : q5[0][ch]), q1 = (int32_t)(n[1] == 0u ? q5[0][ch] : q5[1][ch]);
    const int32_t d = q1 - q0, c = imin(imax(d, -4), 3);
    const int32_t a = q0 + (d - c) / 2, b = a + c;  // (C division: truncating toward zero)
    hi |= (uint32_t)a << (27 - 8 * ch) | ((uint32_t)c & 7u) << (24 - 8 * ch);
    base[0][ch] = a << 3 | a >> 2;
    base[1][ch] = b << 3 | b >> 2;
  }
  // tables and indices.  A texel's candidates are compared by key = 4 (|c|^2 - 2 q . c) + k: the squared distance less the
  // texel's own |q|^2, and the index in the low bits, so that the signed minimum is the closest candidate, the smallest index on a
  // tie.  |c|^2 <= 195075 and q . c <= 195075: no key leaves 24 + 3 bits.
  int32_t best_err[2] = { 0x7fffffff, 0x7fffffff };
  uint32_t best_idx[2] = { 0u, 0u }, best_t[2] = { 0u, 0u };
  ICAMD_NOUNROLL
  for (uint32_t t = 0; t < 8u; ++t) {
    const int32_t a = (int32_t)bfe(t < 4u ? kEtcModA_lo : kEtcModA_hi, 8u * (t & 3u), 8u);
    const int32_t b = (int32_t)bfe(t < 4u ? kEtcModB_lo : kEtcModB_hi, 8u * (t & 3u), 8u);
    const int32_t mod[4] = { op ? a : 0, b, -a, -b };
    ICAMD_UNROLL
    for (int s = 0; s < 2; ++s) {
      uint32_t cand[4];
      int32_t cc[4];
      ICAMD_UNROLL
      for (int k = 0; k < 4; ++k) {
        cand[k] = etc2_pack_clamped(base[s][0] + mod[k], base[s][1] + mod[k], base[s][2] + mod[k]);
        cc[k] = (int32_t)(4u * udot4(cand[k], cand[k], 0u)) + k;
      }
      cc[2] = op ? cc[2] : 1 << 28;  // Op = 0: index 2 is the transparent texel, no colour
      int32_t err = (int32_t)qq[s];
      uint32_t idx = 0u;
      ICAMD_UNROLL
      for (int j = 0; j < 8; ++j) {
        const uint32_t v = q[8 * s + j];
        int32_t key = imad24((int32_t)udot4(v, cand[0], 0u), -8, cc[0]);
        ICAMD_UNROLL
        for (int k = 1; k < 4; ++k) key = imin(key, imad24((int32_t)udot4(v, cand[k], 0u), -8, cc[k]));
        key = ((opaque16 >> (8 * s + j)) & 1u) ? key : 2;  // a transparent texel: index 2, no error
        err += key >> 2;
        idx |= ((uint32_t)key & 3u) << (2 * j);
      }
      const bool better = err < best_err[s];  // (ascending t: a tie keeps the smaller table)
      best_err[s] = better ? err : best_err[s];
      best_idx[s] = better ? idx : best_idx[s];
      best_t[s] = better ? t : best_t[s];
    }
  }
  // sixteen (lsb, msb) pairs -> the two bit planes
  const uint32_t z = best_idx[0] | best_idx[1] << 16;
  uint32_t lsb = z & 0x55555555u, msb = (z >> 1) & 0x55555555u;
  lsb = (lsb | lsb >> 1) & 0x33333333u; msb = (msb | msb >> 1) & 0x33333333u;
  lsb = (lsb | lsb >> 2) & 0x0f0f0f0fu; msb = (msb | msb >> 2) & 0x0f0f0f0fu;
  lsb = (lsb | lsb >> 4) & 0x00ff00ffu; msb = (msb | msb >> 4) & 0x00ff00ffu;
  lsb = (lsb | lsb >> 8) & 0x0000ffffu; msb = (msb | msb >> 8) & 0x0000ffffu;
  EtcA1Result r;
  r.err = (uint32_t)(best_err[0] + best_err[1]);
  r.hi = hi | best_t[0] << 5 | best_t[1] << 2;
  r.lo = lsb | msb << 16;
  return r;
}

// D on the partition `flip` of the block px[4 y + x] (bytes 0..2); opaque16: bit 4 y + x = the texel is opaque.  With flip 0 the
// sub-block order j = 4 x + y is the order of the word's index bits; with flip 1 it is the raster order and the planes are
// transposed into place.
ICAMD_DEV EtcA1Result etc2_a1_partition(const uint32_t px[16], uint32_t opaque16, bool op, bool flip) {
  uint32_t q[16];
  ICAMD_UNROLL
  for (int j = 0; j < 16; ++j) q[j] = (flip ? px[j] : px[4 * (j & 3) + (j >> 2)]) & 0x00ffffffu;
  EtcA1Result r = etc2_a1_search(q, flip ? opaque16 : etc2_a1_transpose4x4(opaque16), op);
  r.lo = flip ? etc2_a1_transpose4x4(r.lo) : r.lo;
  r.hi |= flip ? 1u : 0u;
  return r;
}

// ---- the block

// bit 4 y + x = texel (x, y) is opaque (byte 3 >= 128)
ICAMD_DEV uint32_t etc2_a1_opaque_mask(const uint32_t px[16]) {
  uint32_t m = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 16; ++p) m |= (px[p] >> 31) << p;
  return m;
}

// The ICAMD_ETC2_RGB8A1 block of the sixteen texels px.  e: the block's ETC1 word for the strategy, read only where the block
// is fully opaque (the kernels skip the ETC1 search in waves without such a block).  D is skipped, partition by partition,
// in waves where no lane needs it: the votes count only lanes that use the result.
template <int STRATEGY>
ICAMD_DEV Out8 etc2_a1_block(const uint32_t px[16], Out8 e) {
  const uint32_t opaque16 = etc2_a1_opaque_mask(px);
  const bool opaque = opaque16 == 0xffffu, clear = opaque16 == 0u, mixed = !opaque && !clear;
  const uint32_t ehi = perm(0u, e.lo, 0x00010203u);
  const bool need = mixed || (opaque && !(ehi & 2u));  // (an individual E has no counterpart here: D in its place)
  Out8 c = e;
  uint32_t best = 0xffffffffu;
  ICAMD_NOUNROLL
  for (uint32_t f = 0; f < 2u; ++f) {
    const bool by_strategy = STRATEGY == 0 ? f == 1u : STRATEGY == 1 ? f == 0u : true;
    const bool want = need && (mixed ? by_strategy : f == (ehi & 1u));
    if (wave_all(!want)) continue;
    const EtcA1Result r = etc2_a1_partition(px, opaque16, opaque, f != 0u);
    const bool take = want && r.err < best;  // (flip 0 first: a tie keeps it)
    best = take ? r.err : best;
    c.lo = take ? perm(0u, r.hi, 0x00010203u) : c.lo;  // big-endian words in memory
    c.hi = take ? perm(0u, r.lo, 0x00010203u) : c.hi;
  }
  Out8 o = c;
  if (opaque) o = etc2_rgb8_choose(px, c);
  if (clear) {  // 00 00 00 00 ff ff 00 00
    o.lo = 0u;
    o.hi = 0x0000ffffu;
  }
  return o;
}

}  // namespace icamd
#endif  // ICAMD_ETC2_A1_BLOCK_H_
