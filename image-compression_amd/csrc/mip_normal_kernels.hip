// mip_normal_kernels.hip -- the fused mip-chain pass of mip_pass.h with the normal-map filter of mip_normal.h (include/ic_amd.h,
// ICAMD_MIP_FILTER_NORMAL), for BC5 from 2-, 3- and 4-byte pixels and the RG8 pixel pyramid.  No tables: each kernel's LDS is
// its box twin's (mip_kernels.hip).
#include "mip_pass.h"

namespace icamd {

extern "C" {
#define ICAMD_NMIP_KERNEL(name, mode, comps) \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(MipParams P) { mip_pass<mode, comps, kMipFilterNormal>(P); }
ICAMD_NMIP_KERNEL(icamd_nmip_bc5_rg8_kernel, ICAMD_BC5, 2)
ICAMD_NMIP_KERNEL(icamd_nmip_bc5_rgb888_kernel, ICAMD_BC5, 3)
ICAMD_NMIP_KERNEL(icamd_nmip_bc5_rgba8_kernel, ICAMD_BC5, 4)
ICAMD_NMIP_KERNEL(icamd_nmip_pyramid_rg8_kernel, kMipPyramidMode, 2)
#undef ICAMD_NMIP_KERNEL
}  // extern "C"

namespace {
struct NormalKernel {
  int mode, comps;
  MipKernel kernel;
  const char *name;
};
#define ICAMD_NMIP_ROW(mode, comps, name) { mode, comps, name, #name }
const NormalKernel kNormalKernels[] = {
  ICAMD_NMIP_ROW(ICAMD_BC5, 2, icamd_nmip_bc5_rg8_kernel),
  ICAMD_NMIP_ROW(ICAMD_BC5, 3, icamd_nmip_bc5_rgb888_kernel),
  ICAMD_NMIP_ROW(ICAMD_BC5, 4, icamd_nmip_bc5_rgba8_kernel),
  ICAMD_NMIP_ROW(kMipPyramidMode, 2, icamd_nmip_pyramid_rg8_kernel),
};
#undef ICAMD_NMIP_ROW

const NormalKernel *normal_kernel(int mode, int comps) {
  for (const NormalKernel &k : kNormalKernels)
    if (k.mode == mode && k.comps == comps) return &k;
  return nullptr;
}
}  // namespace

hipError_t launch_mip_normal_pass(int mode, int comps, const MipParams &P, uint32_t n_images, hipStream_t stream) {
  const NormalKernel *k = normal_kernel(mode, comps);
  return launch_mip_kernel(k ? k->kernel : nullptr, P, n_images, stream);
}

const char *mip_normal_kernel_name(int mode, int comps) {
  const NormalKernel *k = normal_kernel(mode, comps);
  return k ? k->name : "";
}

}  // namespace icamd
