// bptc_mip_kernels.hip -- the chain kernels of icamd_encode_bc7_mips_device and icamd_encode_bc6h_mips_device for gfx950
// (EXTENSION, include/ic_amd.h): every level of every image of a BC7 or BC6H mip chain in ONE encode launch; see bptc_mip_plan.h
// for the plan and DESIGN.md 3.25.
//
// One chain form per per-level encode kernel (the list: ICAMD_BPTC_MIP_KERNELS).  The pixel pyramid lies in the workspace when a
// chain kernel starts (the pyramid kernels, earlier on the stream).  grid.x holds the workgroups of one image, largest level
// first, grid.y the images.  A workgroup finds its level (etc2_mip_locate: kernel argument and blockIdx only, so scalar loads and
// scalar arithmetic), builds that level's GridParams (mip_chain_view.h: what launch_tiled would have passed the per-level kernel
// for that level) and runs the per-level kernel's body (bptc_encode_bodies.inc) on it, so a level's bytes are the per-level
// kernel's.  The tile shape varies inside one launch -- 256 x 1 blocks on a level more than 128 block columns wide, squarer
// below -- so every chain kernel runs the WIDE = false body, which handles every shape (DESIGN.md 3.25 says what that costs).
// The view costs scalar registers, not vector ones: tests/test_bptc_mip_isa_host.py holds every chain kernel's VGPR count and
// scratch size to its twin's.
#include "bptc_encode_bodies.inc"
#include "bptc_mip_plan.h"
#include "codec_info.h"
#include "ic_launch.h"
#include "ic_amd.h"
#include "mip_chain_view.h"

namespace icamd {

#define ICAMD_BPTC_MIP_BODY(body)                                          \
  const Etc2MipSpot spot = etc2_mip_locate(M.table, blockIdx.x);           \
  const GridParams P = etc2_mip_view(M, M.table.level[spot.entry]);        \
  const TileAt at = { spot.tile_col, spot.tile_row, blockIdx.y };          \
  body(P, at);

extern "C" {

#define ICAMD_BPTC_MIP_BC7(name, body, comps) \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(Etc2MipParams M) { ICAMD_BPTC_MIP_BODY((body<comps, false>)) }
ICAMD_BPTC_MIP_BC7(icamd_bc7_mip_rgb888_kernel, bc7_encode_one, 3)
ICAMD_BPTC_MIP_BC7(icamd_bc7_mip_rgba8_kernel, bc7_encode_one, 4)
ICAMD_BPTC_MIP_BC7(icamd_bc7_modes_mip_rgb888_kernel, bc7_modes_encode_one, 3)
ICAMD_BPTC_MIP_BC7(icamd_bc7_modes_mip_rgba8_kernel, bc7_modes_encode_one, 4)
#undef ICAMD_BPTC_MIP_BC7

#define ICAMD_BPTC_MIP_BC6H(name, body, chans, is_signed) \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(Etc2MipParams M) { ICAMD_BPTC_MIP_BODY((body<chans, is_signed, false>)) }
ICAMD_BPTC_MIP_BC6H(icamd_bc6h_mip_uf16_rgb16f_kernel, bc6h_encode_one, 3, false)
ICAMD_BPTC_MIP_BC6H(icamd_bc6h_mip_uf16_rgba16f_kernel, bc6h_encode_one, 4, false)
ICAMD_BPTC_MIP_BC6H(icamd_bc6h_mip_sf16_rgb16f_kernel, bc6h_encode_one, 3, true)
ICAMD_BPTC_MIP_BC6H(icamd_bc6h_mip_sf16_rgba16f_kernel, bc6h_encode_one, 4, true)
ICAMD_BPTC_MIP_BC6H(icamd_bc6h_modes_mip_uf16_rgb16f_kernel, bc6h_modes_encode_one, 3, false)
ICAMD_BPTC_MIP_BC6H(icamd_bc6h_modes_mip_uf16_rgba16f_kernel, bc6h_modes_encode_one, 4, false)
ICAMD_BPTC_MIP_BC6H(icamd_bc6h_modes_mip_sf16_rgb16f_kernel, bc6h_modes_encode_one, 3, true)
ICAMD_BPTC_MIP_BC6H(icamd_bc6h_modes_mip_sf16_rgba16f_kernel, bc6h_modes_encode_one, 4, true)
#undef ICAMD_BPTC_MIP_BC6H

}  // extern "C"
#undef ICAMD_BPTC_MIP_BODY

hipError_t launch_bptc_mip(int codec, int chans, int modes, bool swap_rb, const BptcMipPlan &plan, const MipBuffers &buffers,
                           uint64_t src_image_stride, uint64_t dst_image_stride, hipStream_t stream) {
  typedef void (*Kernel)(Etc2MipParams);
#define ICAMD_BPTC_MIP_POINTER(name, twin, c, n, m) name,
  static const Kernel kKernels[] = { ICAMD_BPTC_MIP_KERNELS(ICAMD_BPTC_MIP_POINTER) };
#undef ICAMD_BPTC_MIP_POINTER
  const int index = bptc_mip_kernel_index(codec, chans, modes);
  if (index < 0 || plan.form == kMipRefused) return hipErrorInvalidValue;
  if (plan.form != kMipLaunch || plan.grid_x == 0) return hipSuccess;
  Etc2MipParams M;
  M.src_image_stride = src_image_stride;
  M.pyramid_image_stride = plan.pyramid_image_stride;
  M.dst_image_stride = dst_image_stride;
  M.swap_rb = swap_rb ? 1u : 0u;
  M.etc_strategy = 0u;
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
