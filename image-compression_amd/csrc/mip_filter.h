// mip_filter.h -- how one pixel of mip level l + 1 is made from its four pixels of level l (include/ic_amd.h, mip-chain
// section): the truncating mean of the bytes (ICAMD_MIP_FILTER_BOX, the reference's Average4Uint8Fast), the mean of the light
// the sRGB codes stand for (ICAMD_MIP_FILTER_SRGB), the alpha-weighted mean (ICAMD_MIP_FILTER_ALPHA_WEIGHTED), or both.
// Integer arithmetic only.  Device code for mip_pass.h; with ICAMD_HOST_EMULATION, plain C++ for tests/host_emul.
#ifndef ICAMD_MIP_FILTER_H_
#define ICAMD_MIP_FILTER_H_

#include "ic_device.h"

namespace icamd {

constexpr int kMipFilterSrgb = 1, kMipFilterAlphaWeighted = 2;  // ICAMD_MIP_FILTER_* (bits)

#if defined(ICAMD_HOST_EMULATION)
#define ICAMD_DEV_TABLE static const
#else
#define ICAMD_DEV_TABLE static __device__ const
#endif

// T[s]: the linear light of sRGB code s in 16 bits (scripts/gen_srgb_table.py).
ICAMD_DEV_TABLE uint16_t kSrgbToLinear[256] = {
#include "srgb_table.inc"
};

// R[A] = floor((2^32 - 1) / A) for A = 1..1020 (the sum of four alpha bytes), R[0] = 0: with q = umulhi(n, R[A]) and
// n < 2^27, n / A - 1 / 16 < n R[A] / 2^32 <= n / A, so q is floor(n / A) or one less, and one correction step settles it.
struct MipRecipTable {
  uint32_t r[1024];
};
constexpr MipRecipTable make_mip_recip_table() {
  MipRecipTable t = {};
  for (uint32_t a = 1; a < 1024u; ++a) t.r[a] = 0xffffffffu / a;
  return t;
}
ICAMD_DEV_TABLE MipRecipTable kMipRecip = make_mip_recip_table();
#undef ICAMD_DEV_TABLE

constexpr uint32_t kMipFilterSrgbTableBytes = 2u * 256u * 2u;   // T and M, 16-bit entries
constexpr uint32_t kMipFilterRecipTableBytes = 1024u * 4u;
constexpr uint32_t mip_filter_table_bytes(int filter) {
  return ((filter & kMipFilterSrgb) ? kMipFilterSrgbTableBytes : 0u) + ((filter & kMipFilterAlphaWeighted) ? kMipFilterRecipTableBytes : 0u);
}

// The tables as the filter reads them: in the kernels, the workgroup's copies in LDS (one ds_read_u16 / ds_read_b32 per look-up).
// to_linear = T; midpoint[k] = (T[k-1] + T[k] + 1) >> 1 for k = 1..255 and midpoint[0] = 0; recip = R.
struct MipFilterTables {
  const uint16_t *to_linear, *midpoint;
  const uint32_t *recip;
};

// Entry i of the table copies, for the loops that fill them (i < 256 for T and M, i < 1024 for R).
ICAMD_DEV uint16_t mip_filter_to_linear_entry(uint32_t i) { return kSrgbToLinear[i]; }
ICAMD_DEV uint16_t mip_filter_midpoint_entry(uint32_t i) {
  return i ? (uint16_t)(((uint32_t)kSrgbToLinear[i - 1u] + kSrgbToLinear[i] + 1u) >> 1) : (uint16_t)0;
}
ICAMD_DEV uint32_t mip_filter_recip_entry(uint32_t i) { return kMipRecip.r[i]; }

// Average4Uint8Fast per byte (color_util.h:335-343): (a + b + c + d) / 4, two bytes at a time in 16-bit lanes.
ICAMD_DEV uint32_t avg4_px(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const uint32_t m = 0x00ff00ffu;
  const uint32_t lo = (a & m) + (b & m) + (c & m) + (d & m);
  const uint32_t hi = ((a >> 8) & m) + ((b >> 8) & m) + ((c >> 8) & m) + ((d >> 8) & m);
  return ((lo >> 2) & m) | (((hi >> 2) & m) << 8);
}

// inv(v), v < 65536: the number of k in 1..255 with M[k] <= v -- the code whose T is nearest to v.  M is strictly increasing
// and M[0] = 0, so that number is the largest k with M[k] <= v: eight halving steps.
ICAMD_DEV uint32_t mip_filter_to_srgb(uint32_t v, const MipFilterTables &t) {
  uint32_t k = 0;
  ICAMD_UNROLL
  for (uint32_t step = 128u; step; step >>= 1)
    if (t.midpoint[k + step] <= v) k += step;
  return k;
}

// (n + (A >> 1)) / A for 1 <= A <= 1020 and n + (A >> 1) < 2^27; 0 or 1 for A == 0 (the caller discards it).
ICAMD_DEV uint32_t mip_filter_weighted_quotient(uint32_t n, uint32_t A, const MipFilterTables &t) {
  n += A >> 1;
  uint32_t q = umulhi32(n, t.recip[A]);
  q += n - umad24(q, A, 0u) >= A ? 1u : 0u;  // q <= 65535, A <= 1020: a 24-bit product
  return q;
}

// One pixel of the next level from p0..p3 (dwords in memory order).  FILTER 0 is avg4_px; otherwise bytes 0..2 follow the
// filter and byte 3 is the truncating mean of the alpha bytes (0 for a 3-byte source, whose byte 3 is undefined on input).
template <int FILTER, int COMPS>
ICAMD_DEV uint32_t mip_filter_px(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, const MipFilterTables &t) {
  if (FILTER == 0) return avg4_px(p0, p1, p2, p3);
  constexpr bool kSrgb = (FILTER & kMipFilterSrgb) != 0, kWeighted = (FILTER & kMipFilterAlphaWeighted) != 0;
  static_assert(!kWeighted || COMPS == 4, "the alpha-weighted filter needs an alpha byte");
  const uint32_t a0 = p0 >> 24, a1 = p1 >> 24, a2 = p2 >> 24, a3 = p3 >> 24, A = a0 + a1 + a2 + a3;
  uint32_t out = COMPS == 4 ? (A >> 2) << 24 : 0u;
  ICAMD_UNROLL
  for (uint32_t k = 0; k < 3u; ++k) {
    uint32_t x0 = bfe(p0, 8u * k, 8u), x1 = bfe(p1, 8u * k, 8u), x2 = bfe(p2, 8u * k, 8u), x3 = bfe(p3, 8u * k, 8u);
    if (kSrgb) {
      x0 = t.to_linear[x0]; x1 = t.to_linear[x1]; x2 = t.to_linear[x2]; x3 = t.to_linear[x3];
    }
    uint32_t v = (x0 + x1 + x2 + x3 + (kSrgb ? 2u : 0u)) >> 2;
    if (kWeighted) {
      const uint32_t n = umad24(a0, x0, umad24(a1, x1, umad24(a2, x2, umad24(a3, x3, 0u))));  // <= 1020 * 65535
      const uint32_t q = mip_filter_weighted_quotient(n, A, t);
      v = A ? q : v;
    }
    out |= (kSrgb ? mip_filter_to_srgb(v, t) : v) << (8u * k);
  }
  return out;
}

}  // namespace icamd
#endif  // ICAMD_MIP_FILTER_H_
