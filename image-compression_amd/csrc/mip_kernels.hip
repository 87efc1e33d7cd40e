// mip_kernels.hip -- fused mip-chain encode (and the plain pixel pyramid) for gfx950 (include/ic_amd.h, mip-chain section) with
// the box filter: the pass of mip_pass.h, which describes it.  The kernels of the other filters: mip_filter_kernels.hip.
#include "mip_pass.h"

namespace icamd {

extern "C" {
#define ICAMD_MIP_KERNEL(name, mode, comps) \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(MipParams P) { mip_pass<mode, comps, 0>(P); }
ICAMD_MIP_KERNEL(icamd_mip_dxt1_rgb888_kernel, ICAMD_DXT1, 3)
ICAMD_MIP_KERNEL(icamd_mip_dxt1_rgba8_kernel, ICAMD_DXT1, 4)
ICAMD_MIP_KERNEL(icamd_mip_dxt5_rgba8_kernel, ICAMD_DXT5, 4)
ICAMD_MIP_KERNEL(icamd_mip_bc4_r8_kernel, ICAMD_BC4, 1)
ICAMD_MIP_KERNEL(icamd_mip_bc4_rg8_kernel, ICAMD_BC4, 2)
ICAMD_MIP_KERNEL(icamd_mip_bc4_rgb888_kernel, ICAMD_BC4, 3)
ICAMD_MIP_KERNEL(icamd_mip_bc4_rgba8_kernel, ICAMD_BC4, 4)
ICAMD_MIP_KERNEL(icamd_mip_bc5_rg8_kernel, ICAMD_BC5, 2)
ICAMD_MIP_KERNEL(icamd_mip_bc5_rgb888_kernel, ICAMD_BC5, 3)
ICAMD_MIP_KERNEL(icamd_mip_bc5_rgba8_kernel, ICAMD_BC5, 4)
ICAMD_MIP_KERNEL(icamd_mip_pyramid_r8_kernel, kMipPyramidMode, 1)
ICAMD_MIP_KERNEL(icamd_mip_pyramid_rg8_kernel, kMipPyramidMode, 2)
ICAMD_MIP_KERNEL(icamd_mip_pyramid_rgb888_kernel, kMipPyramidMode, 3)
ICAMD_MIP_KERNEL(icamd_mip_pyramid_rgba8_kernel, kMipPyramidMode, 4)
#undef ICAMD_MIP_KERNEL
}  // extern "C"

static MipKernel mip_kernel(int mode, int comps) {
  switch (mode) {
    case ICAMD_DXT1: return comps == 3 ? icamd_mip_dxt1_rgb888_kernel : comps == 4 ? icamd_mip_dxt1_rgba8_kernel : nullptr;
    case ICAMD_DXT5: return comps == 4 ? icamd_mip_dxt5_rgba8_kernel : nullptr;
    case ICAMD_BC4:
      return comps == 1 ? icamd_mip_bc4_r8_kernel : comps == 2 ? icamd_mip_bc4_rg8_kernel : comps == 3 ? icamd_mip_bc4_rgb888_kernel
           : comps == 4 ? icamd_mip_bc4_rgba8_kernel : nullptr;
    case ICAMD_BC5:
      return comps == 2 ? icamd_mip_bc5_rg8_kernel : comps == 3 ? icamd_mip_bc5_rgb888_kernel : comps == 4 ? icamd_mip_bc5_rgba8_kernel
           : nullptr;
    case kMipPyramidMode:
      return comps == 1 ? icamd_mip_pyramid_r8_kernel : comps == 2 ? icamd_mip_pyramid_rg8_kernel
           : comps == 3 ? icamd_mip_pyramid_rgb888_kernel : comps == 4 ? icamd_mip_pyramid_rgba8_kernel : nullptr;
  }
  return nullptr;
}

hipError_t launch_mip_pass(int mode, int comps, const MipParams &P, uint32_t n_images, hipStream_t stream) {
  return launch_mip_kernel(mip_kernel(mode, comps), P, n_images, stream);
}

const char *mip_box_kernel_name(int mode, int comps) {
  switch (mode) {
    case ICAMD_DXT1: return comps == 3 ? "icamd_mip_dxt1_rgb888_kernel" : comps == 4 ? "icamd_mip_dxt1_rgba8_kernel" : "";
    case ICAMD_DXT5: return comps == 4 ? "icamd_mip_dxt5_rgba8_kernel" : "";
    case ICAMD_BC4:
      return comps == 1 ? "icamd_mip_bc4_r8_kernel" : comps == 2 ? "icamd_mip_bc4_rg8_kernel" : comps == 3 ? "icamd_mip_bc4_rgb888_kernel"
           : comps == 4 ? "icamd_mip_bc4_rgba8_kernel" : "";
    case ICAMD_BC5:
      return comps == 2 ? "icamd_mip_bc5_rg8_kernel" : comps == 3 ? "icamd_mip_bc5_rgb888_kernel" : comps == 4 ? "icamd_mip_bc5_rgba8_kernel"
           : "";
    case kMipPyramidMode:
      return comps == 1 ? "icamd_mip_pyramid_r8_kernel" : comps == 2 ? "icamd_mip_pyramid_rg8_kernel"
           : comps == 3 ? "icamd_mip_pyramid_rgb888_kernel" : comps == 4 ? "icamd_mip_pyramid_rgba8_kernel" : "";
  }
  return "";
}

}  // namespace icamd
