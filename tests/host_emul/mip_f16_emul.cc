// mip_f16_emul.cc -- the half-float pyramid's per-sample routine (image-compression_amd/csrc/mip_f16.h) compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION, like the other *_emul.cc here), for tests/test_mip_f16_host.py: the text the kernels of
// mip_f16_kernels.hip run, against the numpy oracle, and a plain-loop pyramid over it with the kernel's clamping rule.
#include "mip_f16.h"

extern "C" {

// out[i] = mip_f16_avg(q[4 i .. 4 i + 3])
void mip_f16_emul_avg(const uint16_t *q, uint64_t n, uint16_t *out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = (uint16_t)icamd::mip_f16_avg(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
}

// Two channels at once, as the kernel packs them: out[i] = mip_f16_avg2 of four dwords.
void mip_f16_emul_avg2(const uint32_t *q, uint64_t n, uint32_t *out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = icamd::mip_f16_avg2(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
}

// One level from the level above: h x w pixels of c samples, tight rows, to max(1, h / 2) x max(1, w / 2).
void mip_f16_emul_next_level(const uint16_t *in, uint32_t h, uint32_t w, uint32_t c, uint16_t *out) {
  const uint32_t nh = h > 1 ? h >> 1 : 1, nw = w > 1 ? w >> 1 : 1;
  for (uint32_t y = 0; y < nh; ++y)
    for (uint32_t x = 0; x < nw; ++x) {
      const uint32_t y0 = 2 * y, y1 = icamd::umin(2 * y + 1, h - 1), x0 = 2 * x, x1 = icamd::umin(2 * x + 1, w - 1);
      for (uint32_t k = 0; k < c; ++k)
        out[((size_t)y * nw + x) * c + k] =
            (uint16_t)icamd::mip_f16_avg(in[((size_t)y0 * w + x0) * c + k], in[((size_t)y0 * w + x1) * c + k],
                                         in[((size_t)y1 * w + x0) * c + k], in[((size_t)y1 * w + x1) * c + k]);
    }
}

}  // extern "C"
