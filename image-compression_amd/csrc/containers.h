// containers.h -- file-container framing for the encoders' block streams (host code, no device work).
//
// SURVEY.md §8(f) row 4, tail: "container formats (DDS/KTX/PVR headers) which the reference does not have at all".
// google/image-compression stops at the raw block stream (CompressedImage, compressed_image.h:52-66 carries format +
// dimensions only), so there is NOTHING in the reference to pin these against: parity unpinned by construction.  The
// layouts below are written from the public file-format descriptions:
//   * DDS  -- "DDS " magic + 124-byte DDS_HEADER with a FOURCC pixel format (DXT1 / DXT5, and ATI1 / ATI2 for BC4 / BC5;
//             the legacy header has no code for ETC1 or PVRTC); BC7: FOURCC "DX10" followed by the 20-byte DDS_HEADER_DXT10
//             (dxgiFormat 98 = DXGI_FORMAT_BC7_UNORM, resourceDimension 3 = TEXTURE2D, miscFlag 0, arraySize 1, miscFlags2 0);
//             BC6H: the same two headers with dxgiFormat 95 = DXGI_FORMAT_BC6H_UF16 / 96 = DXGI_FORMAT_BC6H_SF16;
//             BC1A: FOURCC DXT1 with ddspf.dwFlags = DDPF_FOURCC | DDPF_ALPHAPIXELS (0x5), the one field in which its header
//             differs from DXT1's; BC2: FOURCC DXT3;
//   * KTX  -- KTX 1.1: 12-byte identifier, 13 little-endian uint32 fields, then per mip level uint32 imageSize + data
//             (glInternalFormat: COMPRESSED_RGB_S3TC_DXT1_EXT 0x83F0, COMPRESSED_RGBA_S3TC_DXT5_EXT 0x83F3,
//             ETC1_RGB8_OES 0x8D64, COMPRESSED_RGBA_PVRTC_2BPPV1_IMG 0x8C03, COMPRESSED_RED_RGTC1 0x8DBB with base format
//             GL_RED, COMPRESSED_RG_RGTC2 0x8DBD with base format GL_RG, COMPRESSED_RGBA8_ETC2_EAC 0x9278 with GL_RGBA,
//             COMPRESSED_R11_EAC 0x9270 with GL_RED, COMPRESSED_RG11_EAC 0x9272 with GL_RG,
//             COMPRESSED_SIGNED_R11_EAC 0x9271 with GL_RED, COMPRESSED_SIGNED_RG11_EAC 0x9273 with GL_RG,
//             COMPRESSED_RGB8_PUNCHTHROUGH_ALPHA1_ETC2 0x9276 with GL_RGBA, COMPRESSED_RGBA_BPTC_UNORM 0x8E8C with GL_RGBA,
//             COMPRESSED_RGB_BPTC_UNSIGNED_FLOAT 0x8E8F and COMPRESSED_RGB_BPTC_SIGNED_FLOAT 0x8E8E with GL_RGB,
//             COMPRESSED_RGBA_S3TC_DXT1_EXT 0x83F1 (BC1A) and COMPRESSED_RGBA_S3TC_DXT3_EXT 0x83F2 (BC2) with GL_RGBA);
//   * PKM  -- 16-byte big-endian header, exactly one level: "PKM 10" with type 0 for ETC1, "PKM 20" with type 3
//             (ETC2_RGBA_NO_MIPMAPS) for ETC2 RGBA8, type 4 (ETC2_RGBA1_NO_MIPMAPS) for ETC2 RGB8A1, type 5 / 6 (ETC2_R /
//             ETC2_RG _NO_MIPMAPS) for EAC R11 / RG11, type 7 / 8 (ETC2_R_SIGNED / ETC2_RG_SIGNED _NO_MIPMAPS) for the signed two;
//   * PVR  -- PVR v3: 52-byte little-endian header (pixel format 1 = PVRTC 2bpp RGBA, 6 = ETC1, 7 = DXT1, 11 = DXT5,
//             9 = DXT3 (BC2), 12 = BC4, 13 = BC5, 15 = BC7, 23 = ETC2 RGBA, 24 = ETC2 RGB A1, 25 = EAC R11, 26 = EAC RG11; signed EAC R11 / RG11 are
//             formats 25 / 26 with the channel-type field 1, signed byte normalised, where every other codec has 0; PVR has
//             ONE DXT1 code: BC1A is format 7 like DXT1, the reader finds the transparent index in the blocks),
//             no metadata, levels follow largest first.  PVRTC data is stored in the Z-order the encoder already
//             produces (pvrtc_compressor.cc:551-580).
// Mip level l of an h x w texture is max(1, h >> l) x max(1, w >> l) pixels; its block stream is what
// icamd_compress / icamd_downsample produce for that size (compressor4x4_helper.h:594-636 halves the same way).
#ifndef ICAMD_CONTAINERS_H_
#define ICAMD_CONTAINERS_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "codec_info.h"
#include "ic_amd.h"

namespace icamd {

inline void put_le32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}
inline void put_le64(uint8_t *p, uint64_t v) {
  put_le32(p, (uint32_t)v);
  put_le32(p + 4, (uint32_t)(v >> 32));
}
inline void put_be16(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v;
}

inline bool container_bc6h(int codec) { return codec == ICAMD_BC6H_UF16 || codec == ICAMD_BC6H_SF16; }
inline bool container_bc1a_bc2(int codec) { return codec == ICAMD_BC1A || codec == ICAMD_BC2; }  // DDS, KTX, PVR; no PKM

inline size_t container_header_size(int container, int codec) {
  switch (container) {
    case ICAMD_CONTAINER_DDS: return codec == ICAMD_BC7 || container_bc6h(codec) ? 148 : 128;  // BC7, BC6H: + DDS_HEADER_DXT10
    case ICAMD_CONTAINER_KTX: return 64;
    case ICAMD_CONTAINER_PKM: return 16;
    case ICAMD_CONTAINER_PVR: return 52;
    default: return 0;
  }
}

inline bool container_supports(int container, int codec) {
  switch (container) {
    case ICAMD_CONTAINER_DDS:
      return codec == ICAMD_DXT1 || codec == ICAMD_DXT5 || codec == ICAMD_BC4 || codec == ICAMD_BC5 || codec == ICAMD_BC7 ||
             container_bc6h(codec) || container_bc1a_bc2(codec);
    case ICAMD_CONTAINER_KTX:
      if (container_bc6h(codec)) return true;  // (BC6H: DDS and KTX only)
      [[fallthrough]];
    case ICAMD_CONTAINER_PVR:
      return codec == ICAMD_DXT1 || codec == ICAMD_DXT5 || codec == ICAMD_ETC1 || codec == ICAMD_PVRTC2 || codec == ICAMD_BC4 ||
             codec == ICAMD_BC5 || codec == ICAMD_ETC2_RGBA8 || codec == ICAMD_ETC2_RGB8 || codec == ICAMD_EAC_R11 ||
             codec == ICAMD_EAC_RG11 || codec == ICAMD_ETC2_RGB8A1 || codec == ICAMD_EAC_SIGNED_R11 ||
             codec == ICAMD_EAC_SIGNED_RG11 || codec == ICAMD_BC7 || container_bc1a_bc2(codec);
    case ICAMD_CONTAINER_PKM:
      return codec == ICAMD_ETC1 || codec == ICAMD_ETC2_RGBA8 || codec == ICAMD_ETC2_RGB8 || codec == ICAMD_EAC_R11 ||
             codec == ICAMD_EAC_RG11 || codec == ICAMD_ETC2_RGB8A1 || codec == ICAMD_EAC_SIGNED_R11 ||
             codec == ICAMD_EAC_SIGNED_RG11;
    default: return false;
  }
}

// bytes of one mip level's block stream; 0 if the level cannot exist for this codec
inline size_t container_level_bytes(int codec, uint32_t height, uint32_t width, uint32_t level) {
  if (level >= 32) return 0;
  const uint32_t h = (height >> level) ? (height >> level) : 1u, w = (width >> level) ? (width >> level) : 1u;
  if (codec == ICAMD_PVRTC2) {  // the encoder's own domain: square powers of two, 8 x 8 and up (pvrtc.cc:636-652)
    if ((height >> level) < 8 || (width >> level) < 8) return 0;
    return (size_t)w * h / 4;
  }
  return (size_t)((h + 3) / 4) * ((w + 3) / 4) * codec_block_bytes(codec);
}

// framing bytes in front of every level (KTX: the uint32 imageSize)
inline size_t container_level_prefix(int container) { return container == ICAMD_CONTAINER_KTX ? 4 : 0; }

// Writes the header of `container` for `codec` into out (container_header_size bytes).  level0_bytes = size of the first level.
inline void container_write_header(int container, int codec, uint32_t height, uint32_t width, uint32_t levels,
                                   size_t level0_bytes, uint8_t *out) {
  memset(out, 0, container_header_size(container, codec));
  switch (container) {
    case ICAMD_CONTAINER_DDS: {
      memcpy(out, "DDS ", 4);
      put_le32(out + 4, 124);                                                            // dwSize
      put_le32(out + 8, 0x1u | 0x2u | 0x4u | 0x1000u | 0x80000u | (levels > 1 ? 0x20000u : 0u));  // CAPS HEIGHT WIDTH PIXELFORMAT LINEARSIZE [MIPMAPCOUNT]
      put_le32(out + 12, height);
      put_le32(out + 16, width);
      put_le32(out + 20, (uint32_t)level0_bytes);                                        // dwPitchOrLinearSize
      put_le32(out + 28, levels);                                                        // dwMipMapCount
      put_le32(out + 76, 32);                                                            // ddspf.dwSize
      put_le32(out + 80, codec == ICAMD_BC1A ? 0x4u | 0x1u : 0x4u);                      // DDPF_FOURCC [| DDPF_ALPHAPIXELS: BC1A]
      memcpy(out + 84, (codec == ICAMD_DXT1 || codec == ICAMD_BC1A) ? "DXT1" : codec == ICAMD_BC2 ? "DXT3"
                       : codec == ICAMD_DXT5 ? "DXT5" : codec == ICAMD_BC4 ? "ATI1" : codec == ICAMD_BC5 ? "ATI2" : "DX10", 4);
      put_le32(out + 108, 0x1000u | (levels > 1 ? 0x8u | 0x400000u : 0u));               // DDSCAPS_TEXTURE [COMPLEX MIPMAP]
      if (codec == ICAMD_BC7 || container_bc6h(codec)) {  // DDS_HEADER_DXT10
        // dxgiFormat: DXGI_FORMAT_BC7_UNORM, DXGI_FORMAT_BC6H_UF16, DXGI_FORMAT_BC6H_SF16
        put_le32(out + 128, codec == ICAMD_BC7 ? 98 : codec == ICAMD_BC6H_UF16 ? 95 : 96);
        put_le32(out + 132, 3);   // resourceDimension: D3D10_RESOURCE_DIMENSION_TEXTURE2D
        put_le32(out + 136, 0);   // miscFlag
        put_le32(out + 140, 1);   // arraySize
        put_le32(out + 144, 0);   // miscFlags2: alpha mode unknown
      }
      break;
    }
    case ICAMD_CONTAINER_KTX: {
      static const uint8_t id[12] = { 0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A };
      memcpy(out, id, 12);
      put_le32(out + 12, 0x04030201u);  // endianness
      put_le32(out + 16, 0);            // glType (compressed)
      put_le32(out + 20, 1);            // glTypeSize
      put_le32(out + 24, 0);            // glFormat (compressed)
      const uint32_t internal = codec == ICAMD_DXT1 ? 0x83F0u : codec == ICAMD_DXT5 ? 0x83F3u : codec == ICAMD_ETC1 ? 0x8D64u
                                : codec == ICAMD_BC4 ? 0x8DBBu : codec == ICAMD_BC5 ? 0x8DBDu
                                : codec == ICAMD_ETC2_RGBA8 ? 0x9278u : codec == ICAMD_ETC2_RGB8 ? 0x9274u
                                : codec == ICAMD_EAC_R11 ? 0x9270u : codec == ICAMD_EAC_RG11 ? 0x9272u
                                : codec == ICAMD_EAC_SIGNED_R11 ? 0x9271u : codec == ICAMD_EAC_SIGNED_RG11 ? 0x9273u
                                : codec == ICAMD_ETC2_RGB8A1 ? 0x9276u : codec == ICAMD_BC7 ? 0x8E8Cu
                                : codec == ICAMD_BC6H_UF16 ? 0x8E8Fu : codec == ICAMD_BC6H_SF16 ? 0x8E8Eu
                                : codec == ICAMD_BC1A ? 0x83F1u : codec == ICAMD_BC2 ? 0x83F2u : 0x8C03u;
      put_le32(out + 28, internal);
      const uint32_t base = (codec == ICAMD_BC4 || codec == ICAMD_EAC_R11 || codec == ICAMD_EAC_SIGNED_R11) ? 0x1903u     // GL_RED
                            : (codec == ICAMD_BC5 || codec == ICAMD_EAC_RG11 || codec == ICAMD_EAC_SIGNED_RG11) ? 0x8227u  // GL_RG
                            : (codec == ICAMD_DXT5 || codec == ICAMD_PVRTC2 || codec == ICAMD_ETC2_RGBA8 ||
                               codec == ICAMD_ETC2_RGB8A1 || codec == ICAMD_BC7 || container_bc1a_bc2(codec)) ? 0x1908u : 0x1907u;                         // GL_RGBA / GL_RGB
      put_le32(out + 32, base);
      put_le32(out + 36, width);
      put_le32(out + 40, height);
      put_le32(out + 44, 0);            // pixelDepth
      put_le32(out + 48, 0);            // numberOfArrayElements
      put_le32(out + 52, 1);            // numberOfFaces
      put_le32(out + 56, levels);
      put_le32(out + 60, 0);            // bytesOfKeyValueData
      break;
    }
    case ICAMD_CONTAINER_PKM: {
      memcpy(out, codec == ICAMD_ETC1 ? "PKM 10" : "PKM 20", 6);
      // ETC2_RGBA / ETC2_RGB / ETC2_RGBA1 / ETC2_R / ETC2_RG / ETC2_R_SIGNED / ETC2_RG_SIGNED / ETC1_RGB _NO_MIPMAPS
      put_be16(out + 6, codec == ICAMD_ETC2_RGBA8 ? 3 : codec == ICAMD_ETC2_RGB8 ? 1 : codec == ICAMD_ETC2_RGB8A1 ? 4
                        : codec == ICAMD_EAC_R11 ? 5 : codec == ICAMD_EAC_RG11 ? 6 : codec == ICAMD_EAC_SIGNED_R11 ? 7
                        : codec == ICAMD_EAC_SIGNED_RG11 ? 8 : 0);
      put_be16(out + 8, (width + 3u) & ~3u);       // encoded (block-aligned) size
      put_be16(out + 10, (height + 3u) & ~3u);
      put_be16(out + 12, width);                   // original size
      put_be16(out + 14, height);
      break;
    }
    case ICAMD_CONTAINER_PVR: {
      put_le32(out, 0x03525650u);  // "PVR\3"
      put_le32(out + 4, 0);        // flags
      put_le64(out + 8, codec == ICAMD_PVRTC2 ? 1u : codec == ICAMD_ETC1 ? 6u : (codec == ICAMD_DXT1 || codec == ICAMD_BC1A) ? 7u
                        : codec == ICAMD_BC2 ? 9u
                        : codec == ICAMD_BC4 ? 12u : codec == ICAMD_BC5 ? 13u : codec == ICAMD_BC7 ? 15u
                        : codec == ICAMD_ETC2_RGBA8 ? 23u
                        : codec == ICAMD_ETC2_RGB8 ? 22u : codec == ICAMD_ETC2_RGB8A1 ? 24u
                        : (codec == ICAMD_EAC_R11 || codec == ICAMD_EAC_SIGNED_R11) ? 25u
                        : (codec == ICAMD_EAC_RG11 || codec == ICAMD_EAC_SIGNED_RG11) ? 26u : 11u);
      put_le32(out + 16, 0);       // colour space: linear RGB
      // channel type: 0 = unsigned byte, normalised; 1 = signed byte, normalised (what tells signed EAC from unsigned)
      put_le32(out + 20, (codec == ICAMD_EAC_SIGNED_R11 || codec == ICAMD_EAC_SIGNED_RG11) ? 1u : 0u);
      put_le32(out + 24, height);
      put_le32(out + 28, width);
      put_le32(out + 32, 1);       // depth
      put_le32(out + 36, 1);       // surfaces
      put_le32(out + 40, 1);       // faces
      put_le32(out + 44, levels);
      put_le32(out + 48, 0);       // metadata bytes
      break;
    }
    default: break;
  }
}

}  // namespace icamd

#endif  // ICAMD_CONTAINERS_H_
