// In-place DXT1 -> ETC1 transcoding (reference public/dxtc_to_etc_transcoder.h:24): every 8-byte DXT1 block of the
// image data is decoded and re-encoded as ETC1 with the kHeuristic strategy.  Metadata is left untouched.
// MI355X backend: one HIP kernel over the block array.
#ifndef IMAGE_COMPRESSION_PUBLIC_DXTC_TO_ETC_TRANSCODER
#define IMAGE_COMPRESSION_PUBLIC_DXTC_TO_ETC_TRANSCODER

#include "image_compression/public/compressed_image.h"

namespace image_codec_compression {

void TranscodeDxt1ToEtc1(CompressedImage *image);

// EXTENSION (the reference has no such function): in-place DXT5 -> ETC2 RGBA8.  Every 16-byte DXT5 block of the image data becomes
// the ETC2 RGBA8 block (EAC alpha word + ETC1-compatible colour word, kHeuristic) of the pixels it decodes to; see
// icamd_transcode_dxt5_to_etc2_rgba8 in ic_amd.h.  Data only: the metadata, format name included, is left untouched.
void TranscodeDxt5ToEtc2Rgba8(CompressedImage *image);

// EXTENSIONS: the other three textures of a desktop asset set, in place and data only like the one above.  DXT1 blocks become the
// ETC2 RGB8 blocks (ETC1-compatible or planar, kHeuristic) of the pixels they decode to, BC4 blocks the EAC R11 blocks and BC5
// blocks the EAC RG11 blocks of theirs; see icamd_transcode_dxt1_to_etc2_rgb8 / _bc4_to_eac_r11 / _bc5_to_eac_rg11 in ic_amd.h.
void TranscodeDxt1ToEtc2Rgb8(CompressedImage *image);
void TranscodeBc4ToEacR11(CompressedImage *image);
void TranscodeBc5ToEacRg11(CompressedImage *image);

}  // namespace image_codec_compression

#endif  // IMAGE_COMPRESSION_PUBLIC_DXTC_TO_ETC_TRANSCODER
