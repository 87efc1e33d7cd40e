// mip_filter_kernels.hip -- the fused mip-chain pass of mip_pass.h with the sRGB, alpha-weighted and combined filters of
// mip_filter.h (include/ic_amd.h, mip-chain section: ICAMD_MIP_FILTER_*), for the colour codecs DXT1 / DXT5 and the pixel
// pyramid (which also serves ETC1 chains, mip_plan.h).  The box-filter kernels, the kernel table and the launcher: mip_kernels.hip.
#include "mip_pass.h"

namespace icamd {

extern "C" {
ICAMD_MIP_FILTER_KERNELS(ICAMD_MIP_DEFINE_KERNEL)
}  // extern "C"

}  // namespace icamd
