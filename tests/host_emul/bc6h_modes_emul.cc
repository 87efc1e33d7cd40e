// TEST INFRASTRUCTURE ONLY.  The BC6H two-subset block math of image-compression_amd/csrc/bc6h_modes_block.h compiled for the
// HOST (g++ -DICAMD_HOST_EMULATION, like bc6h_emul.cc) so that the CPU tier checks it against the numpy definition
// (tests/test_bc6h_modes_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "bc6h_modes_block.h"
#include "emul_violations.h"

using namespace icamd;

template <int C, bool SIGNED>
static void encode_image(int modes, uint32_t h, uint32_t w, uint32_t rows, uint32_t cols, uint32_t stride, const uint8_t *src,
                         uint8_t *out) {
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t rg[16], b[16], o[4];
      bc6h_fetch<C>(src, h, w, stride, br * 4, bc * 4, rg, b);
      if (modes) encode_bc6h_modes<SIGNED>(rg, b, o);
      else encode_bc6h<SIGNED>(rg, b, o);
      memcpy(out + ((size_t)br * cols + bc) * 16, o, 16);
    }
}

// The encoder as the kernels run it (bc6h_modes_kernels.hip; modes 0: bc6h_kernels.hip), one block at a time, over the grid
// max(h, gh) x max(w, gw).
extern "C" int bc6h_modes_emul_encode(int modes, int is_signed, int chans, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw,
                                      uint32_t stride, const uint8_t *src, uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  if (modes != 0 && modes != 1) return 0;
  if (chans == 3 && !is_signed) encode_image<3, false>(modes, h, w, rows, cols, stride, src, out);
  else if (chans == 3) encode_image<3, true>(modes, h, w, rows, cols, stride, src, out);
  else if (chans == 4 && !is_signed) encode_image<4, false>(modes, h, w, rows, cols, stride, src, out);
  else if (chans == 4) encode_image<4, true>(modes, h, w, rows, cols, stride, src, out);
  else return 0;
  return 1;
}

// Q_b as the kernels run it (the closed-form guess +- 1), for every T in [t_lo, t_hi] -> out[T - t_lo]; and D_b(q).
extern "C" void bc6h_modes_emul_quantise(int is_signed, uint32_t b, int32_t t_lo, int32_t t_hi, int32_t *out) {
  for (int32_t T = t_lo; T <= t_hi; ++T) out[T - t_lo] = is_signed ? bc6h_quantise_at<true>(T, b) : bc6h_quantise_at<false>(T, b);
}
extern "C" int32_t bc6h_modes_emul_endpoint_value(int is_signed, uint32_t b, int32_t q) {
  return is_signed ? bc6h_endpoint_value_at<true>(q, b) : bc6h_endpoint_value_at<false>(q, b);
}
