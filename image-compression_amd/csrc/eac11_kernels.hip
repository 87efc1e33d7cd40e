// eac11_kernels.hip -- EAC R11 / RG11 encode and decode kernels for gfx950 (EXTENSION, include/ic_amd.h ICAMD_EAC_R11); see
// eac11_block.h for the block math and DESIGN.md 3.14.
//
// Encode: one block per lane on 16 x 16-block tiles (a wave = 16 x 4 blocks = 64 x 16 pixels, as ETC2 RGBA8: the search's
// wave-uniform exit wants lanes with alike content), four-wave workgroups.  The search is some 33 k VALU instructions per
// channel, so the kernels are bound by instruction issue and the fetch only has to be correct and simple:
//   RGB888 / RGBA8: the ETC tile path (load_tile_block), then one v_perm_b32 pair per row picks byte 0 / 2 (R) and byte 1 (G);
//   R8 / RG8: four 4- / 8-byte row loads at a 64-bit lane address (any alignment, any row padding) where the block lies in the
//   image, the clamp-to-edge byte gather otherwise.
// RG11 runs both searches in ONE lane, R then G (G's sixteen bytes wait in four registers), and stores 16 bytes once: the
// source is read once, and every vote of a search's wave-uniform exit is taken among lanes that search the same channel.
// Decode: the lane-group decoder of lane_groups.h (K = 4 / 2 blocks per lane, 16-byte row stores), as BC4 / BC5.
#include "etc2_encode_bodies.inc"  // eac11_encode_one: the encode body, shared with the chain kernels of etc2_mip_kernels.hip
#include "codec_info.h"
#include "ic_launch.h"
#include "lane_groups.h"
#include "ic_amd.h"

namespace icamd {

struct Eac11Rows {
  __device__ __forceinline__ void operator()(uint32_t w0, uint32_t w1, uint32_t rows[4]) const { decode_eac11(w0, w1, rows); }
};

extern "C" {

#define ICAMD_EAC11_KERNEL(name, comps, rg) \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(GridParams P) { eac11_encode_one<comps, rg>(P, tile_of_launch(P)); }
ICAMD_EAC11_KERNEL(icamd_eac_r11_r8_kernel, 1, false)
ICAMD_EAC11_KERNEL(icamd_eac_r11_rg8_kernel, 2, false)
ICAMD_EAC11_KERNEL(icamd_eac_r11_rgb888_kernel, 3, false)
ICAMD_EAC11_KERNEL(icamd_eac_r11_rgba8_kernel, 4, false)
ICAMD_EAC11_KERNEL(icamd_eac_rg11_rg8_kernel, 2, true)
ICAMD_EAC11_KERNEL(icamd_eac_rg11_rgb888_kernel, 3, true)
ICAMD_EAC11_KERNEL(icamd_eac_rg11_rgba8_kernel, 4, true)
#undef ICAMD_EAC11_KERNEL

__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_eac_r11_decode_kernel(Bc45DecodeParams P) {
  plane_decode<false>(P, Eac11Rows());
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_eac_rg11_decode_kernel(Bc45DecodeParams P) {
  plane_decode<true>(P, Eac11Rows());
}

}  // extern "C"

namespace {
struct Eac11Kernel {
  int codec, comps;
  void (*fn)(GridParams);
  const char *name;
};
#define ICAMD_EAC11_ENTRY(codec, comps, fn) { codec, comps, fn, #fn }
const Eac11Kernel kEac11Kernels[] = {
  ICAMD_EAC11_ENTRY(ICAMD_EAC_R11, 1, icamd_eac_r11_r8_kernel),     ICAMD_EAC11_ENTRY(ICAMD_EAC_R11, 2, icamd_eac_r11_rg8_kernel),
  ICAMD_EAC11_ENTRY(ICAMD_EAC_R11, 3, icamd_eac_r11_rgb888_kernel), ICAMD_EAC11_ENTRY(ICAMD_EAC_R11, 4, icamd_eac_r11_rgba8_kernel),
  ICAMD_EAC11_ENTRY(ICAMD_EAC_RG11, 2, icamd_eac_rg11_rg8_kernel),  ICAMD_EAC11_ENTRY(ICAMD_EAC_RG11, 3, icamd_eac_rg11_rgb888_kernel),
  ICAMD_EAC11_ENTRY(ICAMD_EAC_RG11, 4, icamd_eac_rg11_rgba8_kernel),
};
#undef ICAMD_EAC11_ENTRY
const Eac11Kernel *find_eac11_kernel(int codec, int comps) {
  for (const Eac11Kernel &k : kEac11Kernels)
    if (k.codec == codec && k.comps == comps) return &k;
  return nullptr;
}
}  // namespace

const char *eac11_kernel_name(int codec, int comps) {
  const Eac11Kernel *k = find_eac11_kernel(codec, comps);
  return k ? k->name : "";
}

hipError_t launch_eac11_encode(int codec, int comps, const GridParams &P, hipStream_t stream) {
  const Eac11Kernel *k = find_eac11_kernel(codec, comps);
  if (!k) return hipErrorInvalidValue;
  return launch_tiled(k->fn, k->fn, P, stream, 4u);
}

hipError_t launch_eac11_decode(int codec, uint32_t n_images, const Bc45DecodeParams &P, hipStream_t stream) {
  if (codec != ICAMD_EAC_R11 && codec != ICAMD_EAC_RG11) return hipErrorInvalidValue;
  const uint32_t K = codec == ICAMD_EAC_RG11 ? 2u : 4u;
  const uint32_t groups = (uint32_t)(((uint64_t)P.block_cols + K - 1u) / K);
  return launch_lane_groups(codec == ICAMD_EAC_RG11 ? icamd_eac_rg11_decode_kernel : icamd_eac_r11_decode_kernel, P, n_images,
                            groups, stream, &Bc45DecodeParams::blocks, P.src_image_stride, &Bc45DecodeParams::pixels,
                            P.dst_image_stride);
}

}  // namespace icamd
