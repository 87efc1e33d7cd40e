// codec_info.h -- per-codec constants shared by the host code and the kernels (no device work).
#ifndef ICAMD_CODEC_INFO_H_
#define ICAMD_CODEC_INFO_H_

#include <stdint.h>

#include "ic_amd.h"

namespace icamd {

// Bytes of one 4 x 4 block (PVRTC included: 8 bytes per 8 x 4 / 4 x 4 block): 16 for DXT5 (alpha half + colour half) and BC5
// (two BC4 halves), ETC2 RGBA8 (EAC alpha word + colour word), EAC RG11 and signed EAC RG11 (two EAC words), 8 for every other
// codec (ETC2 RGB8, ETC2 RGB8A1, EAC R11 and signed EAC R11 among them).  BC7 and BC6H (both formats): 16.  BC1A: 8; BC2: 16 (alpha
// word + colour word).
constexpr uint32_t codec_block_bytes(int codec) {
  return (codec == ICAMD_DXT5 || codec == ICAMD_BC5 || codec == ICAMD_ETC2_RGBA8 || codec == ICAMD_EAC_RG11 ||
          codec == ICAMD_EAC_SIGNED_RG11 || codec == ICAMD_BC7 || codec == ICAMD_BC6H_UF16 || codec == ICAMD_BC6H_SF16 ||
          codec == ICAMD_BC2) ? 16u : 8u;
}

// Bytes of one decoded pixel (icamd_decode_device, icamd_decode_bc6h_device): RGBA8 rows for DXT5, ETC2 RGBA8, ETC2 RGB8A1, BC7,
// BC1A, BC2 and PVRTC, R8 for BC4 and EAC R11, RG8 for BC5 and EAC RG11, RGBA16F for BC6H, RGB888 for DXT1, ETC1 and ETC2 RGB8.
constexpr uint32_t codec_decoded_pixel_bytes(int codec) {
  return (codec == ICAMD_BC6H_UF16 || codec == ICAMD_BC6H_SF16) ? 8u
         : (codec == ICAMD_DXT5 || codec == ICAMD_ETC2_RGBA8 || codec == ICAMD_ETC2_RGB8A1 || codec == ICAMD_BC7 ||
            codec == ICAMD_PVRTC2 || codec == ICAMD_PVRTC4 || codec == ICAMD_BC1A || codec == ICAMD_BC2) ? 4u
         : (codec == ICAMD_BC5 || codec == ICAMD_EAC_RG11) ? 2u
         : (codec == ICAMD_BC4 || codec == ICAMD_EAC_R11) ? 1u : 3u;
}

}  // namespace icamd
#endif  // ICAMD_CODEC_INFO_H_
