// Test driver (built by tests/test_gpu_mips.py): Compressor::CompressMipChain against Compress of every level's pixels --
// the 2 x 2 truncating pyramid built here -- for owned and external storage.  Prints one line per case, "OK ..." or
// "FAIL ...", and exits 1 on any failure.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "image_compression/public/compressed_image.h"
#include "image_compression/public/dxtc_compressor.h"
#include "image_compression/public/etc_compressor.h"
#include "image_compression/public/pvrtc_compressor.h"

using namespace image_codec_compression;

static std::vector<uint8> next_level(const std::vector<uint8> &p, uint32 h, uint32 w, uint32 c) {
  const uint32 nh = std::max(1u, h >> 1), nw = std::max(1u, w >> 1);
  std::vector<uint8> out((size_t)nh * nw * c);
  for (uint32 y = 0; y < nh; ++y)
    for (uint32 x = 0; x < nw; ++x) {
      const uint32 y0 = 2 * y, y1 = std::min(2 * y + 1, h - 1), x0 = 2 * x, x1 = std::min(2 * x + 1, w - 1);
      for (uint32 k = 0; k < c; ++k)
        out[((size_t)y * nw + x) * c + k] =
            (uint8)(((int)p[((size_t)y0 * w + x0) * c + k] + p[((size_t)y0 * w + x1) * c + k] + p[((size_t)y1 * w + x0) * c + k] +
                     p[((size_t)y1 * w + x1) * c + k]) / 4);
    }
  return out;
}

static bool same(const CompressedImage &a, const CompressedImage &b) {
  const CompressedImage::Metadata &m = a.GetMetadata(), &n = b.GetMetadata();
  return m.format == n.format && m.compressor_name == n.compressor_name && m.uncompressed_height == n.uncompressed_height &&
         m.uncompressed_width == n.uncompressed_width && m.compressed_height == n.compressed_height &&
         m.compressed_width == n.compressed_width && m.padding_bytes_per_row == n.padding_bytes_per_row &&
         a.GetDataSize() == b.GetDataSize() && std::memcmp(a.GetData(), b.GetData(), a.GetDataSize()) == 0;
}

template <typename C>
static int run(C &comp, const char *name, CompressedImage::Format format, uint32 c, uint32 h, uint32 w, uint32 pad) {
  const size_t stride = (size_t)w * c + pad;
  std::vector<uint8> src(stride * h), tight((size_t)w * c * h);
  for (uint32 y = 0; y < h; ++y)
    for (uint32 i = 0; i < w * c; ++i) {
      const uint8 v = (uint8)((y * 7 + i * 13 + (y * i) % 29 + ((i / c) % 17 < 3 ? 200 : 0)) & 0xff);
      src[y * stride + i] = v;
      tight[(size_t)y * w * c + i] = v;
    }
  uint32 levels = 0;
  for (uint32 m = std::max(h, w); m; m >>= 1) ++levels;
  std::vector<CompressedImage> owned(levels);
  if (!comp.CompressMipChain(format, h, w, pad, src.data(), levels, owned.data())) {
    std::printf("FAIL %s %ux%u: CompressMipChain returned false\n", name, h, w);
    return 1;
  }
  // external storage of the exact sizes: an array of images over caller buffers, built in place
  std::vector<std::vector<uint8> > store(levels);
  for (uint32 l = 0; l < levels; ++l) store[l].resize(owned[l].GetDataSize());
  int bad = 0;
  {
    CompressedImage *arr = static_cast<CompressedImage *>(operator new(sizeof(CompressedImage) * levels));
    for (uint32 l = 0; l < levels; ++l) new (&arr[l]) CompressedImage(store[l].size(), store[l].data());
    if (!comp.CompressMipChain(format, h, w, pad, src.data(), levels, arr)) {
      std::printf("FAIL %s %ux%u: external storage refused\n", name, h, w);
      bad = 1;
    }
    std::vector<uint8> level = tight;
    uint32 lh = h, lw = w;
    for (uint32 l = 0; l < levels && !bad; ++l) {
      CompressedImage want;
      if (!comp.Compress(format, lh, lw, l ? 0 : pad, l ? level.data() : src.data(), &want) || !same(owned[l], want) ||
          !same(arr[l], want)) {
        std::printf("FAIL %s %ux%u level %u\n", name, h, w, l);
        bad = 1;
      }
      level = next_level(level, lh, lw, c);
      lh = std::max(1u, lh >> 1);
      lw = std::max(1u, lw >> 1);
    }
    // a wrongly sized external image is refused, as Compress refuses it
    CompressedImage small(store[0].size() - 1, store[0].data());
    if (comp.CompressMipChain(format, h, w, pad, src.data(), 1, &small)) {
      std::printf("FAIL %s %ux%u: undersized external storage accepted\n", name, h, w);
      bad = 1;
    }
    for (uint32 l = 0; l < levels; ++l) arr[l].~CompressedImage();
    operator delete(arr);
  }
  if (comp.CompressMipChain(format, h, w, pad, src.data(), levels + 1, owned.data()) ||
      comp.CompressMipChain(format, h, w, pad, src.data(), 0, owned.data())) {
    std::printf("FAIL %s %ux%u: level count outside 1 .. L_max accepted\n", name, h, w);
    bad = 1;
  }
  if (!bad) std::printf("OK %s %ux%u pad %u: %u levels\n", name, h, w, pad, levels);
  return bad;
}

int main() {
  DxtcCompressor dxtc;
  EtcCompressor etc;
  PvrtcCompressor pvrtc;
  int bad = 0;
  const uint32 shapes[][3] = { { 61, 59, 5 }, { 300, 200, 0 }, { 1, 9, 3 }, { 130, 2, 1 } };
  for (const auto &s : shapes) {
    bad |= run(dxtc, "dxtc/rgb", CompressedImage::kRGB, 3, s[0], s[1], s[2]);
    bad |= run(dxtc, "dxtc/bgra", CompressedImage::kBGRA, 4, s[0], s[1], s[2]);
    bad |= run(etc, "etc/rgb", CompressedImage::kRGB, 3, s[0], s[1], s[2]);
  }
  std::vector<uint8> buf(64 * 64 * 4);
  std::vector<CompressedImage> imgs(7);
  if (pvrtc.CompressMipChain(CompressedImage::kRGBA, 64, 64, 0, buf.data(), 7, imgs.data()) ||
      etc.CompressMipChain(CompressedImage::kRGBA, 64, 64, 0, buf.data(), 7, imgs.data())) {
    std::printf("FAIL: PVRTC / ETC-from-RGBA chain accepted\n");
    bad = 1;
  } else {
    std::printf("OK refusals\n");
  }
  return bad;
}
