// bc6h_modes_kernels.hip -- BC6H with the opt-in two-subset candidate for gfx950 (EXTENSION, include/ic_amd.h
// ICAMD_BC6H_MODES_EXTENDED).  FUSED: one kernel reads the source once, encodes the one-subset block exactly as
// bc6h_kernels.hip does, fits the block's one two-subset candidate and writes whichever is strictly closer, in one 16-byte store.
// One 4 x 4 block per lane on the tiles of launch_tiled with the GridParams and the fetch of bc6h_kernels.hip; integer only, no
// LDS, no wave-uniform shortcut: a lane's mode is data (bc6h_modes_block.h).
#include "bptc_encode_bodies.inc"  // bc6h_modes_encode_one
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

extern "C" {

// *_kernel: 256 x 1-block tiles (block grids more than 128 columns wide); *_narrow_kernel: any tile shape
#define ICAMD_BC6H_MODES_KERNELS(X)                                                                                         \
  X(bc6h_modes_uf16_rgb16f, ICAMD_BC6H_UF16, 3, false)                                                                      \
  X(bc6h_modes_uf16_rgba16f, ICAMD_BC6H_UF16, 4, false)                                                                     \
  X(bc6h_modes_sf16_rgb16f, ICAMD_BC6H_SF16, 3, true)                                                                       \
  X(bc6h_modes_sf16_rgba16f, ICAMD_BC6H_SF16, 4, true)

#define ICAMD_BC6H_MODES_DEFINE(stem, codec, chans, is_signed)                                                              \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_##stem##_kernel(GridParams P) {                             \
    bc6h_modes_encode_one<chans, is_signed, true>(P, tile_of_launch(P));                                                                       \
  }                                                                                                                         \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_##stem##_narrow_kernel(GridParams P) {                      \
    bc6h_modes_encode_one<chans, is_signed, false>(P, tile_of_launch(P));                                                                      \
  }
ICAMD_BC6H_MODES_KERNELS(ICAMD_BC6H_MODES_DEFINE)
#undef ICAMD_BC6H_MODES_DEFINE

}  // extern "C"

namespace {
struct Bc6hModesKernel {
  int codec, chans;
  void (*wide)(GridParams);
  void (*narrow)(GridParams);
  const char *name;
};
#define ICAMD_BC6H_MODES_ENTRY(stem, codec, chans, is_signed) \
  { codec, chans, icamd_##stem##_kernel, icamd_##stem##_narrow_kernel, "icamd_" #stem "_kernel" },
const Bc6hModesKernel kBc6hModesKernels[] = { ICAMD_BC6H_MODES_KERNELS(ICAMD_BC6H_MODES_ENTRY) };
#undef ICAMD_BC6H_MODES_ENTRY
const Bc6hModesKernel *find_bc6h_modes(int codec, int chans) {
  for (const Bc6hModesKernel &k : kBc6hModesKernels)
    if (k.codec == codec && k.chans == chans) return &k;
  return nullptr;
}
}  // namespace
#undef ICAMD_BC6H_MODES_KERNELS

const char *bc6h_modes_kernel_name(int codec, int chans) {
  const Bc6hModesKernel *k = find_bc6h_modes(codec, chans);
  return k ? k->name : "";
}

hipError_t launch_bc6h_modes_encode(int codec, int chans, const GridParams &P, hipStream_t stream) {
  const Bc6hModesKernel *k = find_bc6h_modes(codec, chans);
  if (!k) return hipErrorInvalidValue;
  return launch_tiled(k->wide, k->narrow, P, stream);
}

}  // namespace icamd
