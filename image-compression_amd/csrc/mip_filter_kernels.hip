// mip_filter_kernels.hip -- the fused mip-chain pass of mip_pass.h with the sRGB, alpha-weighted and combined filters of
// mip_filter.h (include/ic_amd.h, mip-chain section: ICAMD_MIP_FILTER_*), for the colour codecs DXT1 / DXT5 and the pixel
// pyramid (which also serves ETC1 chains, ic_capi.hip).  The box-filter kernels stay in mip_kernels.hip.
#include "mip_pass.h"

namespace icamd {

extern "C" {
#define ICAMD_FMIP_KERNEL(name, mode, comps, filter) \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(MipParams P) { mip_pass<mode, comps, filter>(P); }
ICAMD_FMIP_KERNEL(icamd_fmip_srgb_dxt1_rgb888_kernel, ICAMD_DXT1, 3, 1)
ICAMD_FMIP_KERNEL(icamd_fmip_srgb_dxt1_rgba8_kernel, ICAMD_DXT1, 4, 1)
ICAMD_FMIP_KERNEL(icamd_fmip_srgb_dxt5_rgba8_kernel, ICAMD_DXT5, 4, 1)
ICAMD_FMIP_KERNEL(icamd_fmip_srgb_pyramid_rgb888_kernel, kMipPyramidMode, 3, 1)
ICAMD_FMIP_KERNEL(icamd_fmip_srgb_pyramid_rgba8_kernel, kMipPyramidMode, 4, 1)
ICAMD_FMIP_KERNEL(icamd_fmip_alpha_dxt1_rgba8_kernel, ICAMD_DXT1, 4, 2)
ICAMD_FMIP_KERNEL(icamd_fmip_alpha_dxt5_rgba8_kernel, ICAMD_DXT5, 4, 2)
ICAMD_FMIP_KERNEL(icamd_fmip_alpha_pyramid_rgba8_kernel, kMipPyramidMode, 4, 2)
ICAMD_FMIP_KERNEL(icamd_fmip_srgb_alpha_dxt1_rgba8_kernel, ICAMD_DXT1, 4, 3)
ICAMD_FMIP_KERNEL(icamd_fmip_srgb_alpha_dxt5_rgba8_kernel, ICAMD_DXT5, 4, 3)
ICAMD_FMIP_KERNEL(icamd_fmip_srgb_alpha_pyramid_rgba8_kernel, kMipPyramidMode, 4, 3)
#undef ICAMD_FMIP_KERNEL
}  // extern "C"

namespace {
struct FilterKernel {
  int mode, comps, filter;
  MipKernel kernel;
  const char *name;
};
#define ICAMD_FMIP_ROW(mode, comps, filter, name) { mode, comps, filter, name, #name }
const FilterKernel kFilterKernels[] = {
  ICAMD_FMIP_ROW(ICAMD_DXT1, 3, 1, icamd_fmip_srgb_dxt1_rgb888_kernel),
  ICAMD_FMIP_ROW(ICAMD_DXT1, 4, 1, icamd_fmip_srgb_dxt1_rgba8_kernel),
  ICAMD_FMIP_ROW(ICAMD_DXT5, 4, 1, icamd_fmip_srgb_dxt5_rgba8_kernel),
  ICAMD_FMIP_ROW(kMipPyramidMode, 3, 1, icamd_fmip_srgb_pyramid_rgb888_kernel),
  ICAMD_FMIP_ROW(kMipPyramidMode, 4, 1, icamd_fmip_srgb_pyramid_rgba8_kernel),
  ICAMD_FMIP_ROW(ICAMD_DXT1, 4, 2, icamd_fmip_alpha_dxt1_rgba8_kernel),
  ICAMD_FMIP_ROW(ICAMD_DXT5, 4, 2, icamd_fmip_alpha_dxt5_rgba8_kernel),
  ICAMD_FMIP_ROW(kMipPyramidMode, 4, 2, icamd_fmip_alpha_pyramid_rgba8_kernel),
  ICAMD_FMIP_ROW(ICAMD_DXT1, 4, 3, icamd_fmip_srgb_alpha_dxt1_rgba8_kernel),
  ICAMD_FMIP_ROW(ICAMD_DXT5, 4, 3, icamd_fmip_srgb_alpha_dxt5_rgba8_kernel),
  ICAMD_FMIP_ROW(kMipPyramidMode, 4, 3, icamd_fmip_srgb_alpha_pyramid_rgba8_kernel),
};
#undef ICAMD_FMIP_ROW

const FilterKernel *filter_kernel(int mode, int comps, int filter) {
  for (const FilterKernel &k : kFilterKernels)
    if (k.mode == mode && k.comps == comps && k.filter == filter) return &k;
  return nullptr;
}
}  // namespace

hipError_t launch_mip_filter_pass(int mode, int comps, int filter, const MipParams &P, uint32_t n_images, hipStream_t stream) {
  if (filter == 0) return launch_mip_pass(mode, comps, P, n_images, stream);
  if (filter == kMipFilterNormal) return launch_mip_normal_pass(mode, comps, P, n_images, stream);
  const FilterKernel *k = filter_kernel(mode, comps, filter);
  return launch_mip_kernel(k ? k->kernel : nullptr, P, n_images, stream);
}

const char *mip_kernel_name(int mode, int comps, int filter) {
  if (filter == 0) return mip_box_kernel_name(mode, comps);
  if (filter == kMipFilterNormal) return mip_normal_kernel_name(mode, comps);
  const FilterKernel *k = filter_kernel(mode, comps, filter);
  return k ? k->name : "";
}

}  // namespace icamd
