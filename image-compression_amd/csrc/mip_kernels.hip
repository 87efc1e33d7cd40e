// mip_kernels.hip -- fused mip-chain encode (and the plain pixel pyramid) for gfx950 (include/ic_amd.h, mip-chain section) with
// the box filter: the pass of mip_pass.h, which describes it.  The kernels of the other filters: mip_filter_kernels.hip and
// mip_normal_kernels.hip.  Also the one table of all the mip kernels (mip_plan.h's list) and the launcher of a planned pass.
#include "mip_pass.h"

namespace icamd {

extern "C" {
ICAMD_MIP_BOX_KERNELS(ICAMD_MIP_DEFINE_KERNEL)
#define ICAMD_MIP_DECLARE_KERNEL(name, mode, comps, filter) __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(MipParams P);
ICAMD_MIP_FILTER_KERNELS(ICAMD_MIP_DECLARE_KERNEL)
ICAMD_MIP_NORMAL_KERNELS(ICAMD_MIP_DECLARE_KERNEL)
#undef ICAMD_MIP_DECLARE_KERNEL
}  // extern "C"

typedef void (*MipKernel)(MipParams);
#define ICAMD_MIP_POINTER(name, mode, comps, filter) name,
static const MipKernel kMipKernels[] = { ICAMD_MIP_KERNELS(ICAMD_MIP_POINTER) };  // by mip_kernel_index
#undef ICAMD_MIP_POINTER

hipError_t launch_mip_kernel(MipKernel kernel, const MipPassPlan &pass, const MipBuffers &buffers, bool swap_rb, hipStream_t stream) {
  uint8_t *const base[] = { const_cast<uint8_t *>(buffers.src), buffers.workspace, buffers.out };  // by MipBase
  MipParams P = {};
  P.src_image_stride = pass.in_image_stride;
  P.row_stride = pass.in_row_stride;
  P.height = pass.height;
  P.width = pass.width;
  P.enc_mask = pass.enc_mask;
  P.pix_mask = pass.pix_mask;
  P.swap_rb = swap_rb ? 1u : 0u;
  P.dst_image_stride = pass.dst_image_stride;
  P.pix_image_stride = pass.pix_image_stride;
  for (int j = 0; j < 8; ++j) {
    P.level_off[j] = pass.level_off[j];
    P.pix_off[j] = pass.pix_off[j];
  }
  (void)hipGetLastError();  // a stale error of another library on this thread is not this launch's
  for (uint32_t z = 0; z < mip_pieces(pass.n_images); ++z) {
    const MipPiece images = mip_piece(pass.n_images, z);
    P.src = base[pass.in.base] + pass.in.offset + (uint64_t)images.first * pass.in_image_stride;
    P.dst = pass.enc_mask ? buffers.out + (uint64_t)images.first * pass.dst_image_stride : nullptr;
    P.pix = pass.pix_mask ? base[pass.pix.base] + pass.pix.offset + (uint64_t)images.first * pass.pix_image_stride : nullptr;
    for (uint32_t y = 0; y < mip_pieces(pass.tile_rows); ++y) {
      const MipPiece rows = mip_piece(pass.tile_rows, y);
      P.tile_row0 = rows.first;
      hipLaunchKernelGGL(kernel, dim3(pass.grid_x, rows.count, images.count), dim3(kThreadsPerWorkgroup), 0, stream, P);
    }
  }
  return hipGetLastError();
}

hipError_t launch_mip_pass(int mode, int comps, int filter, const MipPassPlan &pass, const MipBuffers &buffers, bool swap_rb,
                           hipStream_t stream) {
  const int k = mip_kernel_index(mode, comps, filter);
  if (k < 0) return hipErrorInvalidValue;
  return launch_mip_kernel(kMipKernels[k], pass, buffers, swap_rb, stream);
}

const char *mip_kernel_name(int mode, int comps, int filter) { return mip_kernel_form(mode, comps, filter).name; }

}  // namespace icamd
