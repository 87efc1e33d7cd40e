// TEST INFRASTRUCTURE ONLY.  The mip-filter math of image-compression_amd/csrc/mip_filter.h compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION, like emul.cc) so that the CPU tier checks it against the definition restated in numpy
// (tests/mip_filter_oracle.py, tests/test_mip_filters_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include "mip_filter.h"
#include "emul_violations.h"

using namespace icamd;

namespace {
// the tables as a workgroup fills them into LDS (mip_pass.h), through the same entry functions
struct Tables {
  uint16_t to_linear[256], midpoint[256];
  uint32_t recip[1024];
  MipFilterTables t;
  Tables() {
    for (uint32_t i = 0; i < 256u; ++i) {
      to_linear[i] = mip_filter_to_linear_entry(i);
      midpoint[i] = mip_filter_midpoint_entry(i);
    }
    for (uint32_t i = 0; i < 1024u; ++i) recip[i] = mip_filter_recip_entry(i);
    t.to_linear = to_linear;
    t.midpoint = midpoint;
    t.recip = recip;
  }
};
const Tables &tables() {
  static const Tables tb;
  return tb;
}
}  // namespace

extern "C" void mip_filter_emul_table(uint16_t out[256]) {
  for (int i = 0; i < 256; ++i) out[i] = tables().to_linear[i];
}

extern "C" void mip_filter_emul_inverse(const uint32_t *v, uint32_t n, uint8_t *out) {
  for (uint32_t i = 0; i < n; ++i) out[i] = (uint8_t)mip_filter_to_srgb(v[i], tables().t);
}

// (num[i] + (A[i] >> 1)) / A[i]
extern "C" void mip_filter_emul_quotient(const uint32_t *num, const uint32_t *A, uint32_t n, uint32_t *out) {
  for (uint32_t i = 0; i < n; ++i) out[i] = mip_filter_weighted_quotient(num[i], A[i], tables().t);
}

// n quads of four pixel dwords each -> n pixel dwords; returns 0 for a filter / component pair the kernels do not have
extern "C" int mip_filter_emul_quads(int filter, int comps, const uint32_t *quads, uint32_t n, uint32_t *out) {
  typedef uint32_t (*Fn)(uint32_t, uint32_t, uint32_t, uint32_t, const MipFilterTables &);
  Fn f = nullptr;
  switch (filter * 8 + comps) {
    case 0 * 8 + 3: f = mip_filter_px<0, 3>; break;
    case 0 * 8 + 4: f = mip_filter_px<0, 4>; break;
    case 1 * 8 + 3: f = mip_filter_px<1, 3>; break;
    case 1 * 8 + 4: f = mip_filter_px<1, 4>; break;
    case 2 * 8 + 4: f = mip_filter_px<2, 4>; break;
    case 3 * 8 + 4: f = mip_filter_px<3, 4>; break;
  }
  if (!f) return 0;
  for (uint32_t i = 0; i < n; ++i) out[i] = f(quads[4 * i], quads[4 * i + 1], quads[4 * i + 2], quads[4 * i + 3], tables().t);
  return 1;
}
