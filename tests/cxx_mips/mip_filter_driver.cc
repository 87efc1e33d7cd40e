// Test driver (built by tests/test_gpu_mip_filters.py): Compressor::CompressMipChainFiltered on an RGBA image read from a
// file.  usage: mip_filter_driver <rgba file> <height> <width> <padding bytes per row> <out dir>
// For every (class, format, filter) case it writes the levels' data back to back to <out dir>/<case>.bin, which the test
// compares with the oracle's chain, and checks here the levels' metadata, that filter 0 is CompressMipChain, and the refusals.
// Prints one line per case, "OK ..." or "FAIL ...", and exits 1 on any failure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "image_compression/public/compressed_image.h"
#include "image_compression/public/dxtc_compressor.h"
#include "image_compression/public/etc_compressor.h"
#include "image_compression/public/pvrtc_compressor.h"

using namespace image_codec_compression;

static uint32 g_h, g_w, g_pad, g_levels;
static std::vector<uint8> g_rgba;
static std::string g_out;

// the image's rows in `format` (3 or 4 bytes per pixel; the bytes are taken as they are, no channel swap) with g_pad bytes of padding
static std::vector<uint8> rows_of(uint32 c) {
  const size_t stride = (size_t)g_w * c + g_pad;
  std::vector<uint8> src(stride * g_h, 0xa5);
  for (uint32 y = 0; y < g_h; ++y)
    for (uint32 x = 0; x < g_w; ++x) std::memcpy(&src[y * stride + (size_t)x * c], &g_rgba[((size_t)y * g_w + x) * 4], c);
  return src;
}

template <typename C>
static int run(C &comp, const char *name, CompressedImage::Format format, uint32 c, int filter) {
  const std::vector<uint8> src = rows_of(c);
  std::vector<CompressedImage> images(g_levels);
  if (!comp.CompressMipChainFiltered(format, g_h, g_w, g_pad, src.data(), filter, g_levels, images.data())) {
    std::printf("FAIL %s filter %d: CompressMipChainFiltered returned false\n", name, filter);
    return 1;
  }
  int bad = 0;
  std::vector<uint8> chain;
  for (uint32 l = 0; l < g_levels; ++l) {
    const CompressedImage::Metadata &m = images[l].GetMetadata();
    if (m.format != format || m.uncompressed_height != std::max(1u, g_h >> l) || m.uncompressed_width != std::max(1u, g_w >> l) ||
        m.padding_bytes_per_row != (l ? 0u : g_pad)) {
      std::printf("FAIL %s filter %d: metadata of level %u\n", name, filter, l);
      bad = 1;
    }
    chain.insert(chain.end(), images[l].GetData(), images[l].GetData() + images[l].GetDataSize());
  }
  if (filter == 0) {
    std::vector<CompressedImage> plain(g_levels);
    if (!comp.CompressMipChain(format, g_h, g_w, g_pad, src.data(), g_levels, plain.data())) bad = 1;
    for (uint32 l = 0; l < g_levels && !bad; ++l)
      if (plain[l].GetDataSize() != images[l].GetDataSize() || std::memcmp(plain[l].GetData(), images[l].GetData(), plain[l].GetDataSize())) {
        std::printf("FAIL %s: filter 0 differs from CompressMipChain at level %u\n", name, l);
        bad = 1;
      }
  }
  const std::string path = g_out + "/" + name + "_f" + std::to_string(filter) + ".bin";
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(chain.data(), 1, chain.size(), f) != chain.size()) bad = 1;
  if (f) std::fclose(f);
  if (!bad) std::printf("OK %s filter %d: %u levels, %lu bytes\n", name, filter, g_levels, (unsigned long)chain.size());
  return bad;
}

int main(int argc, char **argv) {
  if (argc != 6) return 2;
  g_h = (uint32)std::atoi(argv[2]);
  g_w = (uint32)std::atoi(argv[3]);
  g_pad = (uint32)std::atoi(argv[4]);
  g_out = argv[5];
  g_rgba.resize((size_t)g_h * g_w * 4);
  FILE *f = std::fopen(argv[1], "rb");
  if (!f || std::fread(g_rgba.data(), 1, g_rgba.size(), f) != g_rgba.size()) return 2;
  std::fclose(f);
  for (uint32 m = std::max(g_h, g_w); m; m >>= 1) ++g_levels;
  DxtcCompressor dxtc;
  EtcCompressor etc;
  PvrtcCompressor pvrtc;
  int bad = 0;
  for (int filter = 0; filter <= 3; ++filter) {
    bad |= run(dxtc, "dxtc_rgba", CompressedImage::kRGBA, 4, filter);
    bad |= run(dxtc, "dxtc_bgra", CompressedImage::kBGRA, 4, filter);
    if (filter <= 1) {
      bad |= run(dxtc, "dxtc_rgb", CompressedImage::kRGB, 3, filter);
      bad |= run(etc, "etc_rgb", CompressedImage::kRGB, 3, filter);
    }
  }
  // refusals: the alpha-weighted filter without alpha, filters outside 0 .. 3, PVRTC, ETC from RGBA
  const std::vector<uint8> rgb = rows_of(3), rgba = rows_of(4);
  std::vector<CompressedImage> images(g_levels);
  if (dxtc.CompressMipChainFiltered(CompressedImage::kRGB, g_h, g_w, g_pad, rgb.data(), 2, g_levels, images.data()) ||
      etc.CompressMipChainFiltered(CompressedImage::kRGB, g_h, g_w, g_pad, rgb.data(), 3, g_levels, images.data()) ||
      dxtc.CompressMipChainFiltered(CompressedImage::kRGBA, g_h, g_w, g_pad, rgba.data(), 4, g_levels, images.data()) ||
      dxtc.CompressMipChainFiltered(CompressedImage::kRGBA, g_h, g_w, g_pad, rgba.data(), -1, g_levels, images.data()) ||
      pvrtc.CompressMipChainFiltered(CompressedImage::kRGBA, g_h, g_w, g_pad, rgba.data(), 1, g_levels, images.data()) ||
      etc.CompressMipChainFiltered(CompressedImage::kRGBA, g_h, g_w, g_pad, rgba.data(), 1, g_levels, images.data())) {
    std::printf("FAIL: a refused filter / format combination was accepted\n");
    bad = 1;
  } else {
    std::printf("OK refusals\n");
  }
  return bad;
}
