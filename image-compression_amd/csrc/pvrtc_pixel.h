// pvrtc_pixel.h -- PVRTC1 2 bpp: colour reduction, GetExtremesFast on a whole block (the morph), the bilinear up-sampling and
// the per-pixel modulation scan, the modulation values of one pixel row (pvrtc_row_mods_v).  Part of pvrtc_block.h.
#ifndef ICAMD_PVRTC_PIXEL_H_
#define ICAMD_PVRTC_PIXEL_H_

#include "dxt_block.h"  // pk_lshr16
#include "ic_device.h"

namespace icamd {

// A block's two colours after ApplyColorChannelReduction, expanded to channel pairs.
struct PvrtcAB {
  uint32_t a_rb, a_ga, b_rb, b_ga;
};
// ... and as the two RGBA dwords the morph kernel stores (8 bytes per block).
struct PvrtcColors {
  uint32_t a, b;
};

ICAMD_DEV uint32_t pair_rb(uint32_t c) { return c & 0x00ff00ffu; }
ICAMD_DEV uint32_t pair_ga(uint32_t c) { return (c >> 8) & 0x00ff00ffu; }
ICAMD_DEV uint32_t unpair(uint32_t rb, uint32_t ga) { return rb | ga << 8; }

// ApplyBitDepthReduction (pvrtc.cc:93-106) on one 8-bit channel: keep the top `depth` bits, replicate them downwards.
constexpr uint32_t bit_depth_reduce(uint32_t v, uint32_t depth) {
  const uint32_t e = v & (0xffu << (8 - depth)) & 0xffu;
  return e | e >> depth | (depth <= 3 ? e >> (2 * depth) : 0u);
}

// ApplyColorChannelReduction (pvrtc.cc:337-349), channel by channel as the reference does it:
//   colour A: opaque R5 G5 B4, translucent R4 G4 B3 A3;   colour B: opaque R5 G5 B5, translucent R4 G4 B4 A3.
// Note the alpha 224..254 promotion: a translucent colour whose alpha reduces to 255 keeps its 4/4/3(4)-bit RGB
// but is later stored as opaque (pvrtc_pack_colors tests the REDUCED alpha).
constexpr uint32_t channel_reduce_by_channel(uint32_t c, bool is_b) {
  const uint32_t r = c & 0xffu, g = (c >> 8) & 0xffu, b = (c >> 16) & 0xffu, a = c >> 24;
  return a == 255u ? (bit_depth_reduce(r, 5) | bit_depth_reduce(g, 5) << 8 | bit_depth_reduce(b, is_b ? 5 : 4) << 16 | 255u << 24)
                   : (bit_depth_reduce(r, 4) | bit_depth_reduce(g, 4) << 8 | bit_depth_reduce(b, is_b ? 4 : 3) << 16 |
                      bit_depth_reduce(a, 3) << 24);
}

// The same on all four channels at once (SWAR on the RGBA dword): the shifted copies are masked so that nothing
// crosses a byte boundary.  ~10 integer ops per colour instead of ~45.
constexpr uint32_t channel_reduce(uint32_t c, bool is_b) {
  uint32_t ro = 0, rt = 0;
  if (is_b) {
    const uint32_t eo = c & 0x00f8f8f8u;
    ro = eo | ((eo >> 5) & 0x00070707u);
    const uint32_t et = c & 0xe0f0f0f0u;
    rt = et | ((et >> 4) & 0x000f0f0fu) | ((et >> 3) & 0x1c000000u) | ((et >> 6) & 0x03000000u);
  } else {
    const uint32_t eo = c & 0x00f0f8f8u;
    ro = eo | ((eo >> 5) & 0x00000707u) | ((eo >> 4) & 0x000f0000u);
    const uint32_t et = c & 0xe0e0f0f0u;
    rt = et | ((et >> 4) & 0x00000f0fu) | ((et >> 3) & 0x1c1c0000u) | ((et >> 6) & 0x03030000u);
  }
  return (c >> 24) == 255u ? (ro | 0xff000000u) : rt;
}
// every value of every channel, next to all-zero and all-one neighbours, for both colours and both alpha classes
constexpr bool channel_reduce_matches_reference() {
  for (uint32_t v = 0; v < 256; ++v)
    for (uint32_t sh = 0; sh < 32; sh += 8)
      for (uint32_t bg = 0; bg < 2; ++bg)
        for (uint32_t alpha_ff = 0; alpha_ff < 2; ++alpha_ff) {
          uint32_t c = ((bg ? 0xffffffffu : 0u) & ~(0xffu << sh)) | v << sh;
          if (alpha_ff) c |= 0xff000000u;
          if (channel_reduce(c, false) != channel_reduce_by_channel(c, false)) return false;
          if (channel_reduce(c, true) != channel_reduce_by_channel(c, true)) return false;
        }
  return true;
}
static_assert(channel_reduce_matches_reference(), "SWAR channel reduction differs from the per-channel form");

// Scheduling fence: keeps hipcc from interleaving independent pixels / rows, which would multiply the live
// registers (the encode kernel wants <= 64 VGPRs; thread-level parallelism covers the latency instead).
#if defined(ICAMD_HOST_EMULATION)
#define ICAMD_SCHED_FENCE() ((void)0)
ICAMD_DEV uint32_t popcount_u32(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
#else
#define ICAMD_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
ICAMD_DEV uint32_t popcount_u32(uint32_t v) { return (uint32_t)__popc(v); }
#endif

// Per-lane 32-dword stash (same idea as BlockStash in dxt_block.h): pixel at a data-dependent index.
#if defined(ICAMD_HOST_EMULATION)
struct Stash32 {
  uint32_t v[32];
  void put(const uint32_t px[32]) { for (int i = 0; i < 32; ++i) v[i] = px[i]; }
  uint32_t get(uint32_t idx) const { return v[idx]; }
};
#else
struct Stash32 {
  uint32_t *base;       // the lane's 4 dwords in plane 0
  uint32_t row_dwords;  // distance between the 8 planes
  bool filled = false;  // the kernel already placed the pixels (compile-time constant after inlining)
  __device__ __forceinline__ void put(const uint32_t px[32]) {
    if (filled) return;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      *reinterpret_cast<uint4 *>(base + q * row_dwords) = make_uint4(px[4 * q], px[4 * q + 1], px[4 * q + 2], px[4 * q + 3]);
  }
  __device__ __forceinline__ uint32_t get(uint32_t idx) const { return base[(idx >> 2) * row_dwords + (idx & 3u)]; }
};
#endif

// GetExtremesFast (pvrtc.cc:255-329) on a block's 32 pixels px[4*... raster: idx = 8*y + x].
// image0 = pixel 0 of the whole image: the reference initialises every "max" candidate index to 0
// (an IMAGE index, pvrtc.cc:268-269) and only replaces it when a fitness value > 0 is seen.
// Returns the two extreme colours, ordered so that colour A is not brighter than colour B.
ICAMD_DEV void pvrtc_extremes(const uint32_t px[32], uint32_t image0, Stash32 &stash, uint32_t &col_a, uint32_t &col_b) {
  // keys: value*256 + p (min side) and value*256 + (31-p) (max side): an unsigned min / max over them is the
  // reference's "first pixel with the strictly smallest / largest value".  A key pair is ONE v_perm_b32: the channel
  // byte of the pixel next to an index byte taken from a register that holds four consecutive indices.  The max-side
  // key is the min-side key plus (31 - 2p): one full-rate add.  The lightness axis uses 32-bit keys (byte 1 of the
  // 16-bit dot product is the reference's (77r + 150g + 28b) / 256); the R,B and G,A axes are two 16-bit keys per
  // dword, reduced with v_pk_min/max_u16.
  uint32_t kmin_l = 0xffffffffu, kmax_l = 0u, kmin_rb = 0xffffffffu, kmax_rb = 0u, kmin_ga = 0xffffffffu, kmax_ga = 0u;
  ICAMD_UNROLL
  for (int p = 0; p < 32; p += 2) {
    uint32_t kl[2];
    ICAMD_UNROLL
    for (int q = 0; q < 2; ++q) {
      const uint32_t c = px[p + q], i = (uint32_t)((p + q) & 3);
      const uint32_t idx4 = (uint32_t)((p + q) & ~3) * 0x01010101u + 0x03020100u;  // bytes: 4 consecutive indices
      const uint32_t up = (uint32_t)(31 - 2 * (p + q)) * 0x00010001u;
      // {hi, lo} = {c or dot, idx4}: selector bytes 0..3 pick an index byte, 4..7 a byte of the pixel
      kl[q] = perm(udot4(c, 0x001c964du, 0u), idx4, 0x0c0c0500u | i);              // [idx, lightness, 0, 0]
      const uint32_t k_rb = perm(c, idx4, 0x06000400u | i | i << 16);              // [idx, R, idx, B]
      const uint32_t k_ga = perm(c, idx4, 0x07000500u | i | i << 16);              // [idx, G, idx, A]
      kmin_rb = pk_min_u16(kmin_rb, k_rb);
      kmin_ga = pk_min_u16(kmin_ga, k_ga);
      kmax_rb = pk_max_u16(kmax_rb, k_rb + up);
      kmax_ga = pk_max_u16(kmax_ga, k_ga + up);
    }
    kmin_l = umin3(kmin_l, kl[0], kl[1]);
    kmax_l = umax3(kmax_l, kl[0] + (uint32_t)(31 - 2 * p), kl[1] + (uint32_t)(31 - 2 * (p + 1)));
    if ((p & 6) == 6) {  // one pixel row at a time: stops the optimiser from regrouping the reductions by axis
      kmin_l = opaque(kmin_l); kmax_l = opaque(kmax_l);  // (which keeps ~64 masked pixel values alive)
      kmin_rb = opaque(kmin_rb); kmax_rb = opaque(kmax_rb);
      kmin_ga = opaque(kmin_ga); kmax_ga = opaque(kmax_ga);
      ICAMD_SCHED_FENCE();
    }
  }
  // axis order of the reference: lightness, R, G, B, A (pvrtc.cc:259-266)
  const uint32_t kmin[5] = { kmin_l, kmin_rb & 0xffffu, kmin_ga & 0xffffu, kmin_rb >> 16, kmin_ga >> 16 };
  const uint32_t kmax[5] = { kmax_l, kmax_rb & 0xffffu, kmax_ga & 0xffffu, kmax_rb >> 16, kmax_ga >> 16 };
  stash.put(px);
  uint32_t best_diff = 0, best_lo = 0, best_hi = 0;
  ICAMD_UNROLL
  for (int i = 0; i < 5; ++i) {
    const uint32_t lo = stash.get(kmin[i] & 31u);
    const uint32_t hi_block = stash.get(31u - (kmax[i] & 31u));
    const uint32_t hi = (kmax[i] >> 8) == 0u ? image0 : hi_block;  // never-updated max -> image pixel 0
    const uint32_t d = sad_u8(lo, hi, 0u);
    const bool better = (i == 0) || d > best_diff;  // strict '>' scan from best_pair = 0 (pvrtc.cc:309-316)
    best_lo = better ? lo : best_lo;
    best_hi = better ? hi : best_hi;
    best_diff = better ? d : best_diff;
  }
  // ColorBrightnessOrder (pvrtc.cc:240-243, 323-328): swap only if strictly darker
  const uint32_t s_lo = udot4(best_lo, 0x01010101u, 0u), s_hi = udot4(best_hi, 0x01010101u, 0u);
  const bool swap = s_hi < s_lo;
  col_a = swap ? best_hi : best_lo;
  col_b = swap ? best_lo : best_hi;
}

// One channel pair of GetInterpolatedColor2BPP / Interpolate4_2BPP (pvrtc.cc:173-237):
// ((4-yw)(8-xw) c00 + (4-yw) xw c01 + yw (8-xw) c10 + yw xw c11) / 32 on both 16-bit lanes.
ICAMD_DEV uint32_t bilerp_pair(uint32_t c00, uint32_t c01, uint32_t c10, uint32_t c11, uint32_t xw, uint32_t yw) {
  const uint32_t a = (4u - yw) * (8u - xw), b = (4u - yw) * xw, c = yw * (8u - xw), d = yw * xw;
  return ((a * c00 + b * c01 + c * c10 + d * c11) >> 5) & 0x00ff00ffu;
}

// BestModulation (pvrtc.cc:148-166) for one pixel given the up-sampled A and B colours as pairs.
// Scans mod 0..3 and stops at the first step that does not improve (NOT a full argmin).
ICAMD_DEV uint32_t best_modulation(uint32_t pixel, uint32_t a_rb, uint32_t a_ga, uint32_t b_rb, uint32_t b_ga) {
  const uint32_t c0 = unpair(a_rb, a_ga), c3 = unpair(b_rb, b_ga);
  // ApplyModulation (pvrtc.cc:120-144): (5A+3B)/8 and (3A+5B)/8 per channel; <= 2040 per 16-bit lane
  const uint32_t c1 = unpair(((5u * a_rb + 3u * b_rb) >> 3) & 0x00ff00ffu, ((5u * a_ga + 3u * b_ga) >> 3) & 0x00ff00ffu);
  const uint32_t c2 = unpair(((3u * a_rb + 5u * b_rb) >> 3) & 0x00ff00ffu, ((3u * a_ga + 5u * b_ga) >> 3) & 0x00ff00ffu);
  const uint32_t d0 = sad_u8(pixel, c0, 0u), d1 = sad_u8(pixel, c1, 0u);
  const uint32_t d2 = sad_u8(pixel, c2, 0u), d3 = sad_u8(pixel, c3, 0u);
  const bool s1 = d1 < d0, s2 = s1 && d2 < d1, s3 = s2 && d3 < d2;
  return (uint32_t)s1 + (uint32_t)s2 + (uint32_t)s3;
}

// Modulation value of the pixel at in-block position (XI, YI) of a block whose 3x3 block neighbourhood
// of reduced colours is nb[dy+1][dx+1] (toroidal wrap already applied by the caller).
template <int XI, int YI>
ICAMD_DEV uint32_t pvrtc_pixel_mod(uint32_t pixel, const PvrtcAB nb[3][3]) {
  constexpr int x0 = XI < 4 ? 0 : 1, y0 = YI < 2 ? 0 : 1;      // top-left of the 2x2 sources, pvrtc.cc:216-223
  constexpr uint32_t xw = (XI + 4) & 7, yw = (YI + 2) & 3;      // pvrtc.cc:226-227
  const PvrtcAB &c00 = nb[y0][x0], &c01 = nb[y0][x0 + 1], &c10 = nb[y0 + 1][x0], &c11 = nb[y0 + 1][x0 + 1];
  return best_modulation(pixel,
                         bilerp_pair(c00.a_rb, c01.a_rb, c10.a_rb, c11.a_rb, xw, yw),
                         bilerp_pair(c00.a_ga, c01.a_ga, c10.a_ga, c11.a_ga, xw, yw),
                         bilerp_pair(c00.b_rb, c01.b_rb, c10.b_rb, c11.b_rb, xw, yw),
                         bilerp_pair(c00.b_ga, c01.b_ga, c10.b_ga, c11.b_ga, xw, yw));
}

// 8 * ((4-yw)*top + yw*bot) on a channel pair (both 16-bit lanes; <= 8*4*255 per lane).
ICAMD_DEV uint32_t vblend_pair(uint32_t yw, uint32_t top, uint32_t bot) {
  if (yw == 0u) return top << 5;
  if (yw == 2u) return (top + bot) << 4;
  return (yw == 1u ? 3u * top + bot : top + 3u * bot) << 3;
}

// floor((5a + 3b) / 8) per byte as three nested floor-averages: with m = (a+b)>>1,
//   (b + m) >> 1 = floor((a + 3b) / 4)   and   (a + floor((a + 3b) / 4)) >> 1 = floor((5a + 3b) / 8)
// (an integer can be moved inside a floor, and floor(floor(x/2)/2) = floor(x/4)); checked for all 65 536 pairs.
constexpr bool blend53_is_nested_average() {
  for (unsigned a = 0; a < 256; ++a)
    for (unsigned b = 0; b < 256; ++b) {
      const unsigned m = (a + b) >> 1;
      if (((a + ((b + m) >> 1)) >> 1) != (5 * a + 3 * b) / 8) return false;
    }
  return true;
}
static_assert(blend53_is_nested_average(), "(5a+3b)/8 != avg(a, avg(b, avg(a,b)))");

// Modulation value of one pixel from the horizontally accumulated sums P[] = 256 * (up-sampled A_rb, A_ga,
// B_rb, B_ga) -- the reference's truncated 8-bit channels (pvrtc.cc:228-236, sum / 32) are therefore exactly the
// HIGH BYTES of the four 16-bit lanes, and one v_perm_b32 per colour packs them as R,G,B,A.  The two intermediate
// colours (5A+3B)/8 and (3A+5B)/8 (pvrtc.cc:111-135) are nested byte averages (v_lerp_u8, all four channels per
// instruction), the four L1 distances are v_sad_u8.  The value (0..3) lands in `acc` at the byte whose unit is
// `unit` (1, 1<<8, ...), which is zero on entry: the plain form adds it there, the SDWA form writes the byte (with unit 1 the
// whole dword) -- the same thing inside the precondition below.  Same decisions as best_modulation().
#if !defined(ICAMD_HOST_EMULATION) && !defined(ICAMD_PVRTC_NO_SCAN_SDWA)  // kept: tests/test_isa_guards.py builds the plain form
// The early-exit scan  s1 + (s1 && s2) + (s1 && s2 && s3)  as nested selects  e1 ? (e2 ? (e3 ? 3 : 2) : 1) : 0  on VCC, the
// last select writing byte J of `acc` in place (SDWA dst_sel, the other bytes preserved): 3 v_cmp + 3 v_cndmask and no scalar
// instruction, where the plain expression compiles to 3 v_cmp + 2 s_and_b64 + 2 v_cndmask + v_addc + v_lshl_add (r05: -2 %
// on the one-pass kernel, profiles/r05_ab_pvrtc_onepass.log; -DICAMD_PVRTC_NO_SCAN_SDWA builds the plain form).  The byte of
// `acc` that `unit` addresses must be zero on entry.  PRECONDITION unit is 1, 2^8, 2^16 or 2^24; the byte of `acc` it addresses
// is zero, and with unit 1 the whole of `acc` is zero (only there do this form and the plain one agree).
ICAMD_DEV uint32_t scan_into_byte(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t unit, uint32_t acc) {
  uint32_t x;
  const uint32_t three = 3u, zero = 0u;
#define ICAMD_SCAN_HEAD                                                                                                   \
  "v_cmp_lt_u32_e32 vcc, %[d3], %[d2]\n\tv_cndmask_b32_e32 %[x], 2, %[three], vcc\n\t"                                   \
  "v_cmp_lt_u32_e32 vcc, %[d2], %[d1]\n\tv_cndmask_b32_e32 %[x], 1, %[x], vcc\n\tv_cmp_lt_u32_e32 vcc, %[d1], %[d0]\n\t"
#define ICAMD_SCAN_TAIL(B)                                                                                                \
  "v_cndmask_b32_sdwa %[acc], %[zero], %[x], vcc dst_sel:" B " dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD"
#define ICAMD_SCAN_OPS : [acc] "+v"(acc), [x] "=&v"(x) : [d0] "v"(d0), [d1] "v"(d1), [d2] "v"(d2), [d3] "v"(d3), [three] "v"(three), [zero] "v"(zero) : "vcc"
  if (unit == 1u) asm(ICAMD_SCAN_HEAD "v_cndmask_b32_e32 %[acc], 0, %[x], vcc" ICAMD_SCAN_OPS);  // acc == 0: the whole dword
  else if (unit == 1u << 8) asm(ICAMD_SCAN_HEAD ICAMD_SCAN_TAIL("BYTE_1") ICAMD_SCAN_OPS);
  else if (unit == 1u << 16) asm(ICAMD_SCAN_HEAD ICAMD_SCAN_TAIL("BYTE_2") ICAMD_SCAN_OPS);
  else asm(ICAMD_SCAN_HEAD ICAMD_SCAN_TAIL("BYTE_3") ICAMD_SCAN_OPS);
#undef ICAMD_SCAN_HEAD
#undef ICAMD_SCAN_TAIL
#undef ICAMD_SCAN_OPS
  return acc;
}
#elif defined(ICAMD_HOST_EMULATION)
// (the SDWA form, which is what the kernels run: the value REPLACES the byte `unit` addresses, and unit 1 replaces the whole
// dword; a unit that is none of the four counts as the last, as in the chain of comparisons above -- that case is NOT probed on
// the device, tests/device_probe fixes the unit per op as every caller does)
ICAMD_DEV uint32_t scan_into_byte(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t unit, uint32_t acc, ICAMD_EMUL_SITE) {
  const bool s1 = d1 < d0, s2 = s1 && d2 < d1, s3 = s2 && d3 < d2;  // stop at the first non-improving step
  const uint32_t x = (uint32_t)s1 + (uint32_t)s2 + (uint32_t)s3;
  const uint32_t byte = unit == 1u ? 0u : unit == 1u << 8 ? 1u : unit == 1u << 16 ? 2u : 3u;
  ICAMD_EMUL_DOMAIN((unit == 1u ? acc == 0u : ((acc >> (8u * byte)) & 0xffu) == 0u) && unit == 1u << (8u * byte), "scan_into_byte",
                    unit, acc, x);
  return byte == 0u ? x : (acc & ~(0xffu << (8u * byte))) | x << (8u * byte);
}
#else
ICAMD_DEV uint32_t scan_into_byte(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t unit, uint32_t acc) {
  const bool s1 = d1 < d0, s2 = s1 && d2 < d1, s3 = s2 && d3 < d2;  // stop at the first non-improving step
  return acc + ((uint32_t)s1 + (uint32_t)s2 + (uint32_t)s3) * unit;
}
#endif
// ---- two pixels per scan (r06) ----------------------------------------------------------------------------------------------
// The four L1 distances of a pixel are at most 1 020, so TWO pixels' distances share a dword: v_sad_u8 writes the first pixel's
// into the low half, v_sad_hi_u8 ((sad << 16) + accumulator) adds the second pixel's on top -- still one instruction per distance.
// The early-exit scan then runs on both 16-bit lanes at once: the sign bit of d(k+1) - d(k) (v_pk_sub_u16, |difference| < 2^15)
// is "step k + 1 improves", the chain s1, s1 && s2, s1 && s2 && s3 is two ANDs on the raw differences, and the value 0 .. 3 is
// the sum of the three sign bits -- 9 instructions for two pixels where the compare / select chain takes 12, no VCC, no inline
// asm (hipcc follows every asm statement with an s_nop).  Same decisions as best_modulation().
ICAMD_DEV void modulation_colours(const uint32_t P[4], uint32_t c[4]) {
  const uint32_t kSel = 0x07030501u;  // bytes: lo.b1, hi.b1, lo.b3, hi.b3  = R, G, B, A
  c[0] = perm(P[1], P[0], kSel);
  c[3] = perm(P[3], P[2], kSel);
  const uint32_t m = avg_u8(c[0], c[3]);
  c[1] = avg_u8(c[0], avg_u8(c[3], m));
  c[2] = avg_u8(c[3], avg_u8(c[0], m));
}
// d[k]: distances of two pixels to their own colour k, one per 16-bit lane -> the two modulation values, one per lane
ICAMD_DEV uint32_t scan_pair(const uint32_t d[4]) {
  const uint32_t s1 = pk_sub_u16(d[1], d[0]), s2 = pk_sub_u16(d[2], d[1]), s3 = pk_sub_u16(d[3], d[2]);
  const uint32_t s12 = s1 & s2, s123 = s12 & s3;
  return pk_lshr16(s1, 15) + pk_lshr16(s12, 15) + pk_lshr16(s123, 15);
}
ICAMD_DEV uint32_t accumulate_mod(uint32_t pixel, const uint32_t P[4], uint32_t unit, uint32_t acc) {
  const uint32_t kSel = 0x07030501u;  // bytes: lo.b1, hi.b1, lo.b3, hi.b3  = R, G, B, A
  const uint32_t c0 = perm(P[1], P[0], kSel), c3 = perm(P[3], P[2], kSel);
  const uint32_t m = avg_u8(c0, c3);
  const uint32_t c1 = avg_u8(c0, avg_u8(c3, m)), c2 = avg_u8(c3, avg_u8(c0, m));
  const uint32_t d0 = sad_u8(pixel, c0, 0u), d1 = sad_u8(pixel, c1, 0u);
  const uint32_t d2 = sad_u8(pixel, c2, 0u), d3 = sad_u8(pixel, c3, 0u);
  return scan_into_byte(d0, d1, d2, d3, unit, acc);
}

// The 8 modulation values of one pixel row of a block (bytes of row[0..1], x order), and optionally the value of
// the pixel just right of the row (first pixel of the right-hand block).  top[c] / bot[c], c = 0..2: reduced
// colours of the block columns (left, centre, right) in the two block rows that bracket this pixel row;
// yw = vertical weight of `bot` (0..3).  Separable form of pvrtc.cc:173-237: blend the three block columns
// vertically once ((4-yw)*top + yw*bot), then walk each half row with P(xw+1) = P(xw) + (VR - VL):
//   x_in 0..3: sources (left, centre), xw = 4..7, P(4) = 4 (VL + VR)
//   x_in 4..7: sources (centre, right), xw = 0..3, P(0) = 8 VL
// with everything pre-scaled by 8 (vblend_pair) so that P = 256 * colour: 16-bit lanes, max 65 280, no carries;
//   pixel right of the row = x_in 0 of the next block: sources (centre, right), xw = 4
// (a*c00 + b*c01 + c*c10 + d*c11 with a..d = (4-yw)(8-xw), (4-yw)xw, yw(8-xw), yw*xw is exactly
//  (8-xw)*VL + xw*VR; the division by 32 is accumulate_mod's "take the high byte".)
// V[c][v]: 8 * vertical blend of block column c (left, centre, right), v = a_rb, a_ga, b_rb, b_ga
template <bool WITH_RIGHT>
ICAMD_DEV void pvrtc_row_mods_v(const uint32_t V[3][4], const uint32_t *pixels, uint32_t right_pixel, uint32_t row[2],
                                uint32_t *right_mod) {
  ICAMD_UNROLL
  for (int h = 0; h < 2; ++h) {
    uint32_t P[4], D[4];
    ICAMD_UNROLL
    for (int v = 0; v < 4; ++v) {
      const uint32_t vl = V[h][v], vr = V[h + 1][v];
      D[v] = vr - vl;
      P[v] = h == 0 ? (vl + vr) << 2 : vl << 3;
    }
    uint32_t acc = 0;
    ICAMD_UNROLL
    for (int j = 0; j < 4; ++j) {
      // opaque(): finish this pixel (compares included) before the next one starts, otherwise the optimiser
      // sinks all eight pixels' decisions to the end of the row and keeps their distances alive until then
      acc = opaque(accumulate_mod(pixels[4 * h + j], P, 1u << (8 * j), acc));
      ICAMD_SCHED_FENCE();
      if (j < 3) {
        ICAMD_UNROLL
        for (int v = 0; v < 4; ++v) P[v] += D[v];
      }
    }
    row[h] = acc;
  }
  if (WITH_RIGHT) {
    uint32_t P[4];
    ICAMD_UNROLL
    for (int v = 0; v < 4; ++v) P[v] = (V[1][v] + V[2][v]) << 2;
    *right_mod = accumulate_mod(right_pixel, P, 1u, 0u);
  }
}

}  // namespace icamd
#endif  // ICAMD_PVRTC_PIXEL_H_
