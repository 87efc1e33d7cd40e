// mip_normal_kernels.hip -- the fused mip-chain pass of mip_pass.h with the normal-map filter of mip_normal.h (include/ic_amd.h,
// ICAMD_MIP_FILTER_NORMAL), for BC5 from 2-, 3- and 4-byte pixels and the RG8 pixel pyramid.  No tables: each kernel's LDS is
// its box twin's (mip_kernels.hip, which also holds the kernel table and the launcher).
#include "mip_pass.h"

namespace icamd {

extern "C" {
ICAMD_MIP_NORMAL_KERNELS(ICAMD_MIP_DEFINE_KERNEL)
}  // extern "C"

}  // namespace icamd
