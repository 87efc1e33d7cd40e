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
#include "eac11_block.h"
#include "metric_block.h"  // metric_gather_channel: the clamp-to-edge gather of one channel
#include "codec_info.h"
#include "ic_launch.h"
#include "lane_groups.h"
#include "ic_amd.h"

namespace icamd {

struct __attribute__((packed, aligned(1))) EacU1 { uint32_t x; };

// r[y] byte x = R of texel (x, y) of the lane's block, g likewise (RG only): R = byte 0, or byte 2 of a swapped 3- / 4-byte
// source; G = byte 1.  Texels outside the image replicate its last row / column, also on a padded grid.
template <int COMPS, bool RG>
__device__ __forceinline__ void eac11_fetch(const GridParams &P, const TileCoord &t, uint32_t r[4], uint32_t g[4]) {
  if constexpr (COMPS >= 3) {
    uint32_t px[16];
    load_tile_block<COMPS>(P, t, px);
    const uint32_t lo = P.swap_rb ? 0x0c0c0602u : 0x0c0c0400u, hi = P.swap_rb ? 0x06020c0cu : 0x04000c0cu;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      r[y] = perm(px[4 * y + 1], px[4 * y], lo) | perm(px[4 * y + 3], px[4 * y + 2], hi);
      if (RG) g[y] = perm(px[4 * y + 1], px[4 * y], 0x0c0c0501u) | perm(px[4 * y + 3], px[4 * y + 2], 0x05010c0cu);
    }
  } else {
    const uint8_t *img = P.src + (uint64_t)t.img * P.src_image_stride;
    const uint32_t row = t.brow * 4u, col = t.bcol * 4u;
    if ((uint64_t)row + 4u <= P.height && (uint64_t)col + 4u <= P.width) {
      const uint8_t *p = img + (uint64_t)row * P.row_stride + (uint64_t)col * COMPS;
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const uint8_t *line = p + (uint64_t)y * P.row_stride;
        if (COMPS == 1) {
          r[y] = reinterpret_cast<const EacU1 *>(line)->x;
        } else {
          const U2 v = load_stream(reinterpret_cast<const U2 *>(line));
          r[y] = rg_row_r(v.x, v.y);
          if (RG) g[y] = rg_row_g(v.x, v.y);
        }
      }
    } else {
      metric_gather_channel<COMPS>(img, P.height, P.width, P.row_stride, row, col, 0u, r);
      if (RG) metric_gather_channel<COMPS>(img, P.height, P.width, P.row_stride, row, col, 1u, g);
    }
  }
}

template <int COMPS, bool RG>
__device__ __forceinline__ void eac11_encode_one(const GridParams &P) {
  const TileCoord t = locate_tile<false>(P);
  if (!t.valid) return;
  uint32_t r[4], g[4] = { 0u, 0u, 0u, 0u };
  eac11_fetch<COMPS, RG>(P, t, r, g);
  const Out8 a = encode_eac11_rows(r);
  if (RG) {
    const Out8 b = encode_eac11_rows(g);
    store_stream16(tile_dst<16>(P, t), a.lo, a.hi, b.lo, b.hi);
  } else {
    store_stream8(tile_dst<8>(P, t), a.lo, a.hi);
  }
}

struct Eac11Rows {
  __device__ __forceinline__ void operator()(uint32_t w0, uint32_t w1, uint32_t rows[4]) const { decode_eac11(w0, w1, rows); }
};

extern "C" {

#define ICAMD_EAC11_KERNEL(name, comps, rg) \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(GridParams P) { eac11_encode_one<comps, rg>(P); }
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
