// TEST PROGRAM for TranscodeDxt1ToEtc2Rgb8, TranscodeBc4ToEacR11 and TranscodeBc5ToEacRg11 (image_compression/public/
// dxtc_to_etc_transcoder.h; built by tests/test_gpu_transcode_family.py against this repo's classes).  Each function on a
// CompressedImage over caller storage must leave the bytes the C ABI's host form leaves on a copy of them, the trailing bytes
// that are no whole block included.  Prints one "OK ..." / "BAD ..." line per function and a checksum; exit code 1 on any difference.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ic_amd.h"
#include "image_compression/public/compressed_image.h"
#include "image_compression/public/dxtc_to_etc_transcoder.h"

using namespace image_codec_compression;

static std::vector<uint8> MakeBlocks(size_t n_bytes, uint32 seed) {
  std::vector<uint8> v(n_bytes);
  uint32 x = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < n_bytes; ++i) {
    x = x * 1664525u + 1013904223u;
    v[i] = (uint8)(x >> 24);
  }
  return v;
}

static int Run(const char *name, void (*cxx)(CompressedImage *), int (*abi)(uint8_t *, size_t), size_t block, uint32 seed) {
  const size_t n_bytes = 777 * block + block - 3;  // 777 whole blocks and a tail
  const std::vector<uint8> src = MakeBlocks(n_bytes, seed);
  std::vector<uint8> a = src, b = src;
  CompressedImage image(a.size(), a.data());
  cxx(&image);
  const int rc = abi(b.data(), b.size());
  unsigned sum = 0;
  for (size_t i = 0; i < a.size(); ++i) sum = sum * 31u + a[i];
  const bool tail_kept = std::memcmp(a.data() + 777 * block, src.data() + 777 * block, block - 3) == 0;
  const bool ok = rc == ICAMD_OK && a == b && a != src && tail_kept;
  std::printf("%s %s rc=%d bytes=%zu checksum=%08x\n", ok ? "OK" : "BAD", name, rc, n_bytes, sum);
  return ok ? 0 : 1;
}

int main() {
  if (icamd_device_count() <= 0) {
    std::printf("no HIP device\n");
    return 2;
  }
  int bad = 0;
  bad += Run("TranscodeDxt1ToEtc2Rgb8", TranscodeDxt1ToEtc2Rgb8, icamd_transcode_dxt1_to_etc2_rgb8, 8, 1);
  bad += Run("TranscodeBc4ToEacR11", TranscodeBc4ToEacR11, icamd_transcode_bc4_to_eac_r11, 8, 2);
  bad += Run("TranscodeBc5ToEacRg11", TranscodeBc5ToEacRg11, icamd_transcode_bc5_to_eac_rg11, 16, 3);
  std::printf("transcode family driver: %d bad\n", bad);
  return bad ? 1 : 0;
}
