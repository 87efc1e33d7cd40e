// mip_normal.h -- ICAMD_MIP_FILTER_NORMAL (include/ic_amd.h, "normal-map mip filter"): one pixel of mip level l + 1 of a
// tangent-space normal map from its four pixels of level l.  R and G hold x and y of a unit vector (code c stands for
// 2c - 255, unit length 255); z is rebuilt from them, the four vectors are summed and the sum is brought back to unit length.
// The result is exact: the two square roots and the division take a floating-point first guess (v_sqrt_f32 / v_rcp_f32) and
// settle it with integer compare-and-step, so that it does not depend on how the guess was rounded.
// Device code for mip_pass.h; with ICAMD_HOST_EMULATION, plain C++ for tests/host_emul.
#ifndef ICAMD_MIP_NORMAL_H_
#define ICAMD_MIP_NORMAL_H_

#include "mip_filter.h"

#if defined(ICAMD_HOST_EMULATION)
#include <math.h>
#endif

namespace icamd {

constexpr int kMipFilterNormal = 4;  // ICAMD_MIP_FILTER_NORMAL

// floor(sqrt(n)) for n < 2^30 from a first guess s that is at most one off either way: one step down, one step up.
// (s <= 2^15 + 1: 24-bit factors, and the squares fit 32 bits.)
ICAMD_DEV uint32_t normal_isqrt_settle(uint32_t n, uint32_t s) {
  s -= umad24(s, s, 0u) > n ? 1u : 0u;
  s += umad24(s + 1u, s + 1u, 0u) <= n ? 1u : 0u;
  return s;
}

// floor(n / d) for n < 2^23 and 16 <= d < 2^15 (or n == 0, d >= 1) from a first guess q at most one off either way.
ICAMD_DEV uint32_t normal_div_settle(uint32_t n, uint32_t d, uint32_t q) {
  int32_t r = (int32_t)n - (int32_t)umad24(q, d, 0u);  // in [-d, 2d)
  q -= r < 0 ? 1u : 0u;
  r += r < 0 ? (int32_t)d : 0;
  q += r >= (int32_t)d ? 1u : 0u;
  return q;
}

// The first guesses.  n < 2^30 rounds to a float with a relative error of 2^-24 and v_sqrt_f32 / v_rcp_f32 add one ulp, so
// the square root (below 2^15) is off by less than 2^-8 and the quotient (below 2^19) by less than 2^-2 before truncation:
// the truncated guess is the floor or its neighbour.  BIAS (host emulation only) replaces the guess by the exact floor + BIAS,
// clamped at 0: the tests run every case with the guess forced one off in either direction.
// (the raw truncated guesses on their own, so that tests/device_probe measures the expressions the filter runs)
#if defined(ICAMD_HOST_EMULATION)
ICAMD_DEV uint32_t normal_isqrt_guess(uint32_t n) { return (uint32_t)sqrtf((float)n); }
ICAMD_DEV uint32_t normal_div_guess(uint32_t n, uint32_t d) { return (uint32_t)((float)n * (1.0f / (float)d)); }
#else
ICAMD_DEV uint32_t normal_isqrt_guess(uint32_t n) { return (uint32_t)__builtin_amdgcn_sqrtf((float)n); }
ICAMD_DEV uint32_t normal_div_guess(uint32_t n, uint32_t d) { return (uint32_t)((float)n * __builtin_amdgcn_rcpf((float)d)); }
#endif
template <int BIAS>
ICAMD_DEV uint32_t normal_isqrt(uint32_t n) {
#if defined(ICAMD_HOST_EMULATION)
  if (n >= 1u << 30) emul::violate("normal_isqrt", n, 0u, 0u, __FILE__, __LINE__);
  if (BIAS != 0) {
    const int32_t s = (int32_t)sqrt((double)n) + BIAS;
    return normal_isqrt_settle(n, (uint32_t)(s < 0 ? 0 : s));
  }
#else
  static_assert(BIAS == 0, "the biased guess is for the host emulation");
#endif
  return normal_isqrt_settle(n, normal_isqrt_guess(n));
}
template <int BIAS>
ICAMD_DEV uint32_t normal_div(uint32_t n, uint32_t d) {
#if defined(ICAMD_HOST_EMULATION)
  if (!((n < 1u << 23 && d >= 16u && d < 1u << 15) || (n == 0u && d >= 1u))) emul::violate("normal_div", n, d, 0u, __FILE__, __LINE__);
  if (BIAS != 0) {
    const int32_t q = (int32_t)(n / d) + BIAS;
    return normal_div_settle(n, d, (uint32_t)(q < 0 ? 0 : q));
  }
#else
  static_assert(BIAS == 0, "the biased guess is for the host emulation");
#endif
  return normal_div_settle(n, d, normal_div_guess(n, d));
}

// z of one texel: the nearest integer to sqrt(max(0, 255^2 - x^2 - y^2)), x = 2r - 255, y = 2g - 255.
template <int BIAS>
ICAMD_DEV uint32_t normal_z(int32_t x, int32_t y) {
  const int32_t rem = imax(0, 65025 - imad24(x, x, imad24(y, y, 0)));
  return (normal_isqrt<BIAS>((uint32_t)rem << 2) + 1u) >> 1;  // 4 rem <= 260100
}

// Ls = floor(sqrt(N2 << 8)): the length of the summed vector with 4 fraction bits, N2 <= 3 * 1020^2 < 2^22.
template <int BIAS>
ICAMD_DEV uint32_t normal_length16(uint32_t n2) { return normal_isqrt<BIAS>(n2 << 8); }

// The code of one component V (|V| <= 1020) of the summed vector, brought to unit length: m = min(255, (4080 |V| +
// (Ls >> 1)) / Ls) with V's sign, code (v + 256) >> 1.  Ls >= 16 (N2 >= 1).
template <int BIAS>
ICAMD_DEV uint32_t normal_code(int32_t V, uint32_t Ls) {
  const uint32_t a = (uint32_t)(V < 0 ? -V : V);
  const int32_t m = (int32_t)umin(255u, normal_div<BIAS>(umad24(4080u, a, Ls >> 1), Ls));
  return (uint32_t)((V < 0 ? -m : m) + 256) >> 1;
}

// One pixel of the next level from p0..p3 (dwords in memory order).  R is byte 0, or byte 2 when swap (wave-uniform; 3- and
// 4-byte pixels only), G is byte 1; every other byte is the truncating mean of avg4_px.
template <int COMPS, int BIAS = 0>
ICAMD_DEV uint32_t mip_normal_px(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, bool swap) {
  static_assert(COMPS >= 2 && COMPS <= 4, "a normal map has R and G");
  const uint32_t rsh = COMPS >= 3 && swap ? 16u : 0u;
  const uint32_t box = avg4_px(p0, p1, p2, p3);
  const uint32_t p[4] = { p0, p1, p2, p3 };
  int32_t X = 0, Y = 0;
  uint32_t Z = 0;
  ICAMD_UNROLL
  for (int i = 0; i < 4; ++i) {
    const int32_t x = 2 * (int32_t)bfe(p[i], rsh, 8u) - 255, y = 2 * (int32_t)bfe(p[i], 8u, 8u) - 255;
    X += x;
    Y += y;
    Z += normal_z<BIAS>(x, y);
  }
  const uint32_t n2 = (uint32_t)imad24(X, X, imad24(Y, Y, 0)) + umad24(Z, Z, 0u);
  const uint32_t Ls = normal_length16<BIAS>(n2);
  const uint32_t rg = normal_code<BIAS>(X, umax(Ls, 1u)) << rsh | normal_code<BIAS>(Y, umax(Ls, 1u)) << 8;
  const uint32_t mask = 0xffu << rsh | 0xff00u;
  return n2 ? (box & ~mask) | rg : box;  // N2 == 0: the box value
}

}  // namespace icamd
#endif  // ICAMD_MIP_NORMAL_H_
