// TEST INFRASTRUCTURE ONLY.  The BC7 mode-1 / mode-5 block math of image-compression_amd/csrc/bc7_modes_block.h compiled for the
// HOST (g++ -DICAMD_HOST_EMULATION, like bc7_emul.cc) so that the CPU tier checks it against the numpy definition
// (tests/test_bc7_modes_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "bc7_modes_block.h"
#include "emul_violations.h"

using namespace icamd;

template <int COMPS>
static void encode_image(int modes, int swap, uint32_t h, uint32_t w, uint32_t rows, uint32_t cols, uint32_t stride,
                         const uint8_t *src, uint8_t *out) {
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      uint32_t px[16], o[4];
      load_block<COMPS>(src, h, w, stride, br * 4, bc * 4, px);
      if (modes) encode_bc7_modes<COMPS>(px, swap != 0, o);
      else encode_bc7<COMPS>(px, swap != 0, o);
      memcpy(out + ((size_t)br * cols + bc) * 16, o, 16);
    }
}

// The encoder as the kernels run it (bc7_modes_kernels.hip; modes 0: bc7_kernels.hip), one block at a time, over the grid
// max(h, gh) x max(w, gw).
extern "C" int bc7_modes_emul_encode(int modes, int comps, int swap, uint32_t h, uint32_t w, uint32_t gh, uint32_t gw,
                                     uint32_t stride, const uint8_t *src, uint8_t *out) {
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4;
  if (modes != 0 && modes != 1) return 0;
  if (comps == 3) encode_image<3>(modes, swap, h, w, rows, cols, stride, src, out);
  else if (comps == 4) encode_image<4>(modes, swap, h, w, rows, cols, stride, src, out);
  else return 0;
  return 1;
}

// The quantisers' roundings: kind 0 / 1 = Q1 with parity 0 / 1, kind 2 = Q5; the decoded byte nearest to T.
extern "C" uint32_t bc7_modes_emul_nearest(int kind, uint32_t T) {
  return kind == 2 ? bc7_near7(T) : bc7_near_parity(T, (uint32_t)kind);
}
