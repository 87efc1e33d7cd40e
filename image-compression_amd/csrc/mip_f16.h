// mip_f16.h -- the box filter of the half-float pixel pyramid (include/ic_amd.h, "half-float pixel pyramid"): one output sample
// from the four samples above it, as exact integer arithmetic on binary16 bit patterns.  The mean of the four values, rounded to
// nearest even; NaN counts as 0, an infinity as the largest finite half of its sign; -0 is never written.
//
// Plain C++ on 32- and 64-bit integers: the same text runs in mip_f16_kernels.hip and, compiled with g++, in
// tests/host_emul/mip_f16_emul.cc, which tests/test_mip_f16_host.py holds against the float64 restatement.
#ifndef ICAMD_MIP_F16_H_
#define ICAMD_MIP_F16_H_

#include "ic_device.h"

namespace icamd {

// The value of the half h (low 16 bits) in units of 2^-24, after the cleaning of NaN and infinities: |F| < 2^40.
ICAMD_DEV int64_t mip_f16_fixed(uint32_t h) {
  const uint32_t m = h & 0x7fffu;
  const uint32_t c = m > 0x7c00u ? 0u : m == 0x7c00u ? 0x7bffu : m;
  const uint32_t e = c >> 10, f = c & 1023u;
  const int64_t v = e == 0u ? (int64_t)f : (int64_t)(1024u + f) << (e - 1u);
  return (h & 0x8000u) ? -v : v;
}

// The half nearest to (p0 + p1 + p2 + p3) / 4, ties to even.
ICAMD_DEV uint32_t mip_f16_avg(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
  const int64_t sum = mip_f16_fixed(p0) + mip_f16_fixed(p1) + mip_f16_fixed(p2) + mip_f16_fixed(p3);  // |sum| < 2^42
  if (sum == 0) return 0u;
  const uint64_t a = (uint64_t)(sum < 0 ? -sum : sum);
  const uint32_t n = 64u - (uint32_t)__builtin_clzll(a);  // bit length: 1 .. 42
  const uint32_t s = n > 13u ? n - 11u : 2u;              // the sum is four values: two bits go to the division
  uint32_t q = (uint32_t)(a >> s);                        // at most 11 bits
  const uint64_t rem = a & ((1ull << s) - 1u), half = 1ull << (s - 1u);
  if (rem > half || (rem == half && (q & 1u))) ++q;       // a carry into bit 11 runs into the exponent field
  const uint32_t mag = ((s - 2u) << 10) + q;
  return mag == 0u ? 0u : mag | (sum < 0 ? 0x8000u : 0u);  // (a sum that rounds to nothing is +0 like a sum of nothing)
}

// Two samples at once: the halves of each dword are two channels of one pixel.
ICAMD_DEV uint32_t mip_f16_avg2(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
  return mip_f16_avg(p0 & 0xffffu, p1 & 0xffffu, p2 & 0xffffu, p3 & 0xffffu) |
         mip_f16_avg(p0 >> 16, p1 >> 16, p2 >> 16, p3 >> 16) << 16;
}

}  // namespace icamd
#endif  // ICAMD_MIP_F16_H_
