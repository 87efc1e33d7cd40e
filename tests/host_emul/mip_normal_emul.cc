// TEST INFRASTRUCTURE ONLY.  The normal-map mip filter of image-compression_amd/csrc/mip_normal.h compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION, like mip_filter_emul.cc) so that the CPU tier checks it against the definition restated in numpy
// (tests/normal_filter_oracle.py, tests/test_mip_normal_host.py).  `bias` is the first guess of the two square roots and the
// division: 0 the floating-point guess, -1 / +1 the exact floor forced one off.  Never linked into libic_amd.so.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include "mip_normal.h"
#include "emul_violations.h"

using namespace icamd;

#define BY_BIAS(call_m1, call_0, call_p1) (bias < 0 ? (call_m1) : bias > 0 ? (call_p1) : (call_0))

// z of n texels (r[i], g[i])
extern "C" void mip_normal_emul_z(int bias, const uint8_t *r, const uint8_t *g, uint32_t n, uint32_t *out) {
  for (uint32_t i = 0; i < n; ++i) {
    const int32_t x = 2 * r[i] - 255, y = 2 * g[i] - 255;
    out[i] = BY_BIAS(normal_z<-1>(x, y), normal_z<0>(x, y), normal_z<1>(x, y));
  }
}

// Ls for N2 = first .. first + n - 1
extern "C" void mip_normal_emul_length(int bias, uint32_t first, uint32_t n, uint32_t *out) {
  for (uint32_t i = 0; i < n; ++i)
    out[i] = BY_BIAS(normal_length16<-1>(first + i), normal_length16<0>(first + i), normal_length16<1>(first + i));
}

// the output code of component V[i] under length Ls[i]
extern "C" void mip_normal_emul_code(int bias, const int32_t *V, const uint32_t *Ls, uint32_t n, uint32_t *out) {
  for (uint32_t i = 0; i < n; ++i)
    out[i] = BY_BIAS(normal_code<-1>(V[i], Ls[i]), normal_code<0>(V[i], Ls[i]), normal_code<1>(V[i], Ls[i]));
}

// n quads of four pixel dwords each -> n pixel dwords; returns 0 for a component count the kernels do not have
extern "C" int mip_normal_emul_quads(int bias, int comps, int swap, const uint32_t *quads, uint32_t n, uint32_t *out) {
  typedef uint32_t (*Fn)(uint32_t, uint32_t, uint32_t, uint32_t, bool);
  Fn f = nullptr;
  switch (comps) {
    case 2: f = BY_BIAS((mip_normal_px<2, -1>), (mip_normal_px<2, 0>), (mip_normal_px<2, 1>)); break;
    case 3: f = BY_BIAS((mip_normal_px<3, -1>), (mip_normal_px<3, 0>), (mip_normal_px<3, 1>)); break;
    case 4: f = BY_BIAS((mip_normal_px<4, -1>), (mip_normal_px<4, 0>), (mip_normal_px<4, 1>)); break;
  }
  if (!f) return 0;
  for (uint32_t i = 0; i < n; ++i) out[i] = f(quads[4 * i], quads[4 * i + 1], quads[4 * i + 2], quads[4 * i + 3], swap != 0);
  return 1;
}
