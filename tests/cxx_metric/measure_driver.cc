// TEST PROGRAM for MeasureErrorDevice, the quality-metric member of the C++ classes' device extension (compressor.h; built by
// tests/test_gpu_metric.py against this repo's classes and the HIP runtime API).  For every class and format: the record the
// member leaves in HBM for Compress's own blocks must equal the record of the C ABI's icamd_measure_error_device and of the
// host-buffer icamd_measure_error.  Prints one "OK ..." line per case with the record; exit code 1 on any difference.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "ic_amd.h"
#include "image_compression/public/compressed_image.h"
#include "image_compression/public/dxtc_compressor.h"
#include "image_compression/public/etc_compressor.h"
#include "image_compression/public/pvrtc_compressor.h"

using namespace image_codec_compression;

static int g_bad = 0;

// coarse gradient + noise: varied blocks (pixel bytes only; the row padding is filled with 0xA5)
static std::vector<uint8> MakeImage(uint32 h, uint32 w, uint32 comps, uint32 pad, uint32 seed) {
  std::vector<uint8> v((size_t)h * (w * comps + pad), 0xA5);
  uint32 x = seed * 2654435761u + 12345u;
  for (uint32 yy = 0; yy < h; ++yy)
    for (uint32 i = 0; i < w * comps; ++i) {
      x = x * 1664525u + 1013904223u;
      v[(size_t)yy * (w * comps + pad) + i] = (uint8)(((x >> 24) & 63u) + 3u * (i / comps / 4) + 2u * (yy / 4));
    }
  return v;
}

struct DeviceBuf {
  void *p;
  explicit DeviceBuf(size_t n) : p(nullptr) { if (hipMalloc(&p, n ? n : 1) != hipSuccess) p = nullptr; }
  ~DeviceBuf() { if (p) (void)hipFree(p); }
};

template <typename C>
static void Run(C *c, const char *name, int compressor, int codec, CompressedImage::Format format, uint32 comps, uint32 h,
                uint32 w, uint32 pad, hipStream_t stream) {
  const std::vector<uint8> img = MakeImage(h, w, comps, pad, h * 131u + w);
  CompressedImage host;
  if (!c->Compress(format, h, w, pad, img.data(), &host)) {
    std::printf("BAD %s fmt=%d %ux%u: Compress refused\n", name, (int)format, h, w);
    ++g_bad;
    return;
  }
  const size_t n = host.GetDataSize();
  DeviceBuf d_in(img.size()), d_blocks(n), d_stats(2 * sizeof(icamd_error_stats));
  (void)hipMemcpy(d_in.p, img.data(), img.size(), hipMemcpyHostToDevice);
  (void)hipMemcpy(d_blocks.p, host.GetData(), n, hipMemcpyHostToDevice);
  (void)hipMemset(d_stats.p, 0xEE, 2 * sizeof(icamd_error_stats));  // the call overwrites its record
  icamd_error_stats *recs = static_cast<icamd_error_stats *>(d_stats.p);
  const bool ok = c->MeasureErrorDevice(format, h, w, pad, d_in.p, d_blocks.p, n, recs, stream);
  const int swap = (format == CompressedImage::kBGR || format == CompressedImage::kBGRA) ? 1 : 0;
  const int rc = icamd_measure_error_device(codec, (int)comps, swap, h, w, h, w, w * comps + pad, 1, 0, 0, d_in.p, d_blocks.p,
                                            recs + 1, stream);
  (void)hipStreamSynchronize(stream);
  icamd_error_stats got[2], from_host;
  (void)hipMemcpy(got, d_stats.p, sizeof got, hipMemcpyDeviceToHost);
  const int rc_host = icamd_measure_error(compressor, (int)format, h, w, pad, img.data(), host.GetData(), n, &from_host);
  const bool refused = !c->MeasureErrorDevice(format, h, w, pad, d_in.p, d_blocks.p, n + 8, recs, stream);
  const bool same = ok && rc == ICAMD_OK && rc_host == ICAMD_OK && refused && std::memcmp(&got[0], &got[1], sizeof got[0]) == 0 &&
                    std::memcmp(&got[0], &from_host, sizeof from_host) == 0;
  if (!same) ++g_bad;
  std::printf("%s %s fmt=%d %ux%u pad=%u sse=%llu,%llu,%llu,%llu max=%u,%u,%u,%u\n", same ? "OK" : "BAD", name, (int)format, h, w,
              pad, (unsigned long long)got[0].sse[0], (unsigned long long)got[0].sse[1], (unsigned long long)got[0].sse[2],
              (unsigned long long)got[0].sse[3], got[0].max_abs[0], got[0].max_abs[1], got[0].max_abs[2], got[0].max_abs[3]);
}

int main() {
  hipStream_t stream = nullptr;
  if (hipStreamCreate(&stream) != hipSuccess) {
    std::printf("no HIP device\n");
    return 2;
  }
  DxtcCompressor dxtc;
  EtcCompressor etc;
  PvrtcCompressor pvrtc;
  etc.SetCompressionStrategy(EtcCompressor::kHeuristic);
  Run(&dxtc, "dxtc", ICAMD_COMPRESSOR_DXTC, ICAMD_DXT1, CompressedImage::kRGB, 3, 61, 59, 3, stream);
  Run(&dxtc, "dxtc", ICAMD_COMPRESSOR_DXTC, ICAMD_DXT1, CompressedImage::kBGR, 3, 64, 128, 0, stream);
  Run(&dxtc, "dxtc", ICAMD_COMPRESSOR_DXTC, ICAMD_DXT5, CompressedImage::kRGBA, 4, 37, 130, 5, stream);
  Run(&dxtc, "dxtc", ICAMD_COMPRESSOR_DXTC, ICAMD_DXT5, CompressedImage::kBGRA, 4, 5, 3, 0, stream);
  Run(&etc, "etc", ICAMD_COMPRESSOR_ETC, ICAMD_ETC1, CompressedImage::kRGB, 3, 61, 59, 1, stream);
  Run(&pvrtc, "pvrtc", ICAMD_COMPRESSOR_PVRTC, ICAMD_PVRTC2, CompressedImage::kRGBA, 4, 64, 64, 0, stream);
  Run(&pvrtc, "pvrtc", ICAMD_COMPRESSOR_PVRTC, ICAMD_PVRTC2, CompressedImage::kRGBA, 4, 256, 256, 0, stream);
  (void)hipStreamDestroy(stream);
  std::printf("measure driver: %d bad\n", g_bad);
  return g_bad ? 1 : 0;
}
