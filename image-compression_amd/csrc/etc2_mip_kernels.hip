// etc2_mip_kernels.hip -- the chain kernels of icamd_encode_etc2_mips_device for gfx950 (EXTENSION, include/ic_amd.h): every level
// of every image of an ETC2-family mip chain in ONE encode launch; see etc2_mip_plan.h for the plan and DESIGN.md 3.18.
//
// One chain form per per-level encode kernel (the list: ICAMD_ETC2_MIP_KERNELS).  The pixel pyramid lies in the workspace when a
// chain kernel starts (the pyramid kernels, earlier on the stream).  grid.x holds the workgroups of one image, level by level,
// grid.y the images.  A workgroup
//   finds its level: one comparison for level 0 (three workgroups in four), else a search of first_wg[] on blockIdx.x, and one
//   division, etc2_mip_locate -- kernel argument and blockIdx only, so scalar loads and scalar arithmetic, the same in every lane;
//   builds that level's GridParams (pointers, strides, sizes, tile shape: what launch_tiled would have passed the per-level kernel
//   for that level), again from scalar data only;
//   and runs the per-level kernel's body (etc2_encode_bodies.inc) on it: the same loads, block routines, wave votes and stores, so
//   a level's bytes are the per-level kernel's.
// A workgroup covers blocks of one level only, on the tiles launch_tiled would use for it.  The view costs scalar registers, not
// vector ones: every chain kernel has the VGPR count and the scratch size of its twin (tests/test_etc2_mip_isa_host.py holds
// them together), and each is declared with its twin's occupancy attribute.
#include "etc2_encode_bodies.inc"
#include "codec_info.h"
#include "ic_launch.h"
#include "ic_amd.h"
#include "mip_chain_view.h"

namespace icamd {

#define ICAMD_ETC2_MIP_BODY(body)                                          \
  const Etc2MipSpot spot = etc2_mip_locate(M.table, blockIdx.x);           \
  const GridParams P = etc2_mip_view(M, M.table.level[spot.entry]);        \
  const TileAt at = { spot.tile_col, spot.tile_row, blockIdx.y };          \
  body(P, at);

extern "C" {

// (the occupancy attributes are the twins': etc2_rgb8_kernels.hip, etc2_kernels.hip, etc2_a1_kernels.hip)
#define ICAMD_ETC2_MIP_RGB8(name, comps, strategy)                                                                          \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) __attribute__((amdgpu_waves_per_eu(4))) name(Etc2MipParams M) {   \
    ICAMD_ETC2_MIP_BODY((etc2_rgb8_encode_one<comps, strategy>))                                                            \
  }
ICAMD_ETC2_MIP_RGB8(icamd_etc2_mip_rgb8_rgb888_split_h_kernel, 3, 0)
ICAMD_ETC2_MIP_RGB8(icamd_etc2_mip_rgb8_rgb888_split_v_kernel, 3, 1)
ICAMD_ETC2_MIP_RGB8(icamd_etc2_mip_rgb8_rgb888_kernel, 3, 2)
ICAMD_ETC2_MIP_RGB8(icamd_etc2_mip_rgb8_rgb888_heuristic_kernel, 3, 3)
ICAMD_ETC2_MIP_RGB8(icamd_etc2_mip_rgb8_rgba8_split_h_kernel, 4, 0)
ICAMD_ETC2_MIP_RGB8(icamd_etc2_mip_rgb8_rgba8_split_v_kernel, 4, 1)
ICAMD_ETC2_MIP_RGB8(icamd_etc2_mip_rgb8_rgba8_kernel, 4, 2)
ICAMD_ETC2_MIP_RGB8(icamd_etc2_mip_rgb8_rgba8_heuristic_kernel, 4, 3)
#undef ICAMD_ETC2_MIP_RGB8

__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc2_mip_th_rgb888_kernel(Etc2MipParams M) {
  ICAMD_ETC2_MIP_BODY(etc2_th_encode_one<3>)
}
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_etc2_mip_th_rgba8_kernel(Etc2MipParams M) {
  ICAMD_ETC2_MIP_BODY(etc2_th_encode_one<4>)
}

#define ICAMD_ETC2_MIP_RGBA8(name, strategy)                                                                                \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) __attribute__((amdgpu_waves_per_eu(strategy == 2 ? 3 : 4, 4)))    \
  name(Etc2MipParams M) {                                                                                                   \
    ICAMD_ETC2_MIP_BODY(etc2_encode_one<strategy>)                                                                          \
  }
ICAMD_ETC2_MIP_RGBA8(icamd_etc2_mip_rgba8_split_h_kernel, 0)
ICAMD_ETC2_MIP_RGBA8(icamd_etc2_mip_rgba8_split_v_kernel, 1)
ICAMD_ETC2_MIP_RGBA8(icamd_etc2_mip_rgba8_kernel, 2)
ICAMD_ETC2_MIP_RGBA8(icamd_etc2_mip_rgba8_heuristic_kernel, 3)
#undef ICAMD_ETC2_MIP_RGBA8

#define ICAMD_ETC2_MIP_A1(name, strategy)                                                                                   \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) __attribute__((amdgpu_waves_per_eu(4))) name(Etc2MipParams M) {   \
    ICAMD_ETC2_MIP_BODY(etc2_a1_encode_one<strategy>)                                                                       \
  }
ICAMD_ETC2_MIP_A1(icamd_etc2_mip_rgb8a1_split_h_kernel, 0)
ICAMD_ETC2_MIP_A1(icamd_etc2_mip_rgb8a1_split_v_kernel, 1)
ICAMD_ETC2_MIP_A1(icamd_etc2_mip_rgb8a1_kernel, 2)
ICAMD_ETC2_MIP_A1(icamd_etc2_mip_rgb8a1_heuristic_kernel, 3)
#undef ICAMD_ETC2_MIP_A1

#define ICAMD_ETC2_MIP_EAC11(name, comps, rg) \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(Etc2MipParams M) { ICAMD_ETC2_MIP_BODY((eac11_encode_one<comps, rg>)) }
ICAMD_ETC2_MIP_EAC11(icamd_etc2_mip_r11_r8_kernel, 1, false)
ICAMD_ETC2_MIP_EAC11(icamd_etc2_mip_r11_rg8_kernel, 2, false)
ICAMD_ETC2_MIP_EAC11(icamd_etc2_mip_r11_rgb888_kernel, 3, false)
ICAMD_ETC2_MIP_EAC11(icamd_etc2_mip_r11_rgba8_kernel, 4, false)
ICAMD_ETC2_MIP_EAC11(icamd_etc2_mip_rg11_rg8_kernel, 2, true)
ICAMD_ETC2_MIP_EAC11(icamd_etc2_mip_rg11_rgb888_kernel, 3, true)
ICAMD_ETC2_MIP_EAC11(icamd_etc2_mip_rg11_rgba8_kernel, 4, true)
#undef ICAMD_ETC2_MIP_EAC11

}  // extern "C"
#undef ICAMD_ETC2_MIP_BODY

hipError_t launch_etc2_mip(int codec, int comps, uint32_t etc_strategy, bool th, bool swap_rb, const Etc2MipPlan &plan,
                           const MipBuffers &buffers, uint64_t src_image_stride, uint64_t dst_image_stride, hipStream_t stream) {
  typedef void (*Kernel)(Etc2MipParams);
#define ICAMD_ETC2_MIP_POINTER(name, twin, c, n, s, t) name,
  static const Kernel kKernels[] = { ICAMD_ETC2_MIP_KERNELS(ICAMD_ETC2_MIP_POINTER) };
#undef ICAMD_ETC2_MIP_POINTER
  const int index = etc2_mip_kernel_index(codec, comps, (int)etc_strategy, th);
  if (index < 0 || plan.form == kMipRefused) return hipErrorInvalidValue;
  if (plan.form != kMipLaunch || plan.grid_x == 0) return hipSuccess;
  Etc2MipParams M;
  M.src_image_stride = src_image_stride;
  M.pyramid_image_stride = plan.pyramid_image_stride;
  M.dst_image_stride = dst_image_stride;
  M.swap_rb = swap_rb ? 1u : 0u;
  M.etc_strategy = etc_strategy;
  M.table = plan.table;
  (void)hipGetLastError();  // do not attribute a stale error of another library on this thread to these launches
  for (uint32_t i = 0; i < mip_pieces(plan.n_images); ++i) {
    const MipPiece images = mip_piece(plan.n_images, i);
    M.src = buffers.src + (uint64_t)images.first * src_image_stride;
    M.pyramid = buffers.workspace + (uint64_t)images.first * plan.pyramid_image_stride;  // (never read for a chain of level 0 alone)
    M.dst = buffers.out + (uint64_t)images.first * dst_image_stride;
    hipLaunchKernelGGL(kKernels[index], dim3(plan.grid_x, images.count), dim3(kThreadsPerWorkgroup), 0, stream, M);
  }
  return hipGetLastError();
}

}  // namespace icamd
