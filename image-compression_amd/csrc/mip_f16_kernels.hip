// mip_f16_kernels.hip -- the half-float pixel pyramid for gfx950 (EXTENSION, include/ic_amd.h icamd_mip_pyramid_f16_device;
// DESIGN.md 3.25): levels 1 .. of RGB16F / RGBA16F images, each sample the mean of the four above it by the integer definition of
// mip_f16.h.  Pyramid only: BC6H chains encode from it afterwards (bptc_mip_kernels.hip).
//
// The pass is the 8-bit pyramid's (mip_pass.h) with pixels of CH halves, planned by mip_plan_passes with 2 CH bytes per pixel in
// place of the component count:
//  * a 256-lane workgroup owns a 128 x 128-pixel tile of the input level; in four rounds a lane reads the tile's 4 x 4-pixel
//    blocks from global memory (rows of 8 CH bytes as two loads of two pixels, at any 2-byte alignment; the clamp-to-edge gather
//    at the image's edges) and writes each block's 2 x 2 level-1 pixels to LDS, a pixel as two dwords R | G << 16, B | A << 16
//    (64 x 64 x 8 bytes = 32 KiB);
//  * one barrier later the tile's levels 2 .. 6 (7 when the input is one tile) are built in LDS from the level above, one halving
//    per barrier (10.7 KiB more: 43 688 bytes in all);
//  * every level the pass owns is then written as tight rows of 2 CH bytes, consecutive lanes to consecutive pixels; a pass
//    that hands off writes local level 6 where the next pass reads it.
// The next level is built from real pixels only: x1 = min(2 x + 1, w_l - 1), which differs from 2 x + 1 only where w_l == 1; for
// level 0 -> 1 the clamped gather already holds those pixels (mip_pass.h).
#include "mip_f16.h"
#include "mip_pass.h"  // mip_lds_off, mip_level: the tile geometry of the 8-bit pass

namespace icamd {

namespace {

struct Px16 {
  uint32_t x, y;  // R | G << 16, B | A << 16 (RGB16F: B alone)
};
struct __attribute__((packed, aligned(2))) H1 { uint32_t x; };
struct __attribute__((packed, aligned(2))) H2 { uint32_t x, y; };

// Two neighbouring pixels of a row: one 16- or 12-byte load at any alignment (load_stream: every input byte is read once).
template <int CH>
__device__ __forceinline__ void f16_load_pair(const uint8_t *q, Px16 &a, Px16 &b) {
  if (CH == 4) {  // R0 G0 | B0 A0 | R1 G1 | B1 A1
    const U4 v = load_stream(reinterpret_cast<const U4 *>(q));
    a = { v.x, v.y };
    b = { v.z, v.w };
  } else {  // R0 G0 | B0 R1 | G1 B1
    const U3 v = load_stream(reinterpret_cast<const U3 *>(q));
    a = { v.x, v.y & 0xffffu };
    b = { alignbit(v.z, v.y, 16u), v.z >> 16 };
  }
}
template <int CH>
__device__ __forceinline__ Px16 f16_load_px(const uint8_t *q) {
  const uint16_t *s = reinterpret_cast<const uint16_t *>(q);
  Px16 p;
  p.x = (uint32_t)s[0] | (uint32_t)s[1] << 16;
  p.y = CH == 4 ? (uint32_t)s[2] | (uint32_t)s[3] << 16 : (uint32_t)s[2];
  return p;
}
template <int CH>
__device__ __forceinline__ void f16_store_px(uint8_t *q, const Px16 &p) {
  if (CH == 4) {
    H2 v = { p.x, p.y };
    *reinterpret_cast<H2 *>(q) = v;
  } else {
    reinterpret_cast<H1 *>(q)->x = p.x;
    *reinterpret_cast<uint16_t *>(q + 4) = (uint16_t)p.y;
  }
}
template <int CH>
__device__ __forceinline__ Px16 f16_filter_px(const Px16 &a, const Px16 &b, const Px16 &c, const Px16 &d) {
  Px16 r;
  r.x = mip_f16_avg2(a.x, b.x, c.x, d.x);
  r.y = CH == 4 ? mip_f16_avg2(a.y, b.y, c.y, d.y) : mip_f16_avg(a.y, b.y, c.y, d.y);
  return r;
}

template <int CH>
__device__ __forceinline__ void mip_f16_pass(const MipParams &P) {
  constexpr uint32_t kBpp = 2u * CH;
  __shared__ Px16 lds[kMipLdsDwords];
  const uint32_t tid = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y + P.tile_row0;
  const uint8_t *src = P.src + (uint64_t)blockIdx.z * P.src_image_stride;
  const uint32_t mask = P.pix_mask & ~1u;  // local levels this pass writes
  if (!mask) return;
  const uint32_t jmax = 31u - (uint32_t)__builtin_clz(mask);
  // level 1: block i of the tile's 32 x 32 blocks of 4 x 4 pixels, from global memory
#pragma nounroll
  for (uint32_t r = 0; r < 4u; ++r) {
    const uint32_t i = tid + (r << 8), bx = i & 31u, by = i >> 5;
    const uint32_t row = (ty * 32u + by) * 4u, col = (tx * 32u + bx) * 4u;
    if (row >= P.height || col >= P.width) continue;
    const bool inside = P.height - row >= 4u && P.width - col >= 4u;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        Px16 a, b, c, d;
        if (inside) {
          const uint8_t *q = src + (uint64_t)(row + 2u * (uint32_t)dy) * P.row_stride + (uint64_t)(col + 2u * (uint32_t)dx) * kBpp;
          f16_load_pair<CH>(q, a, b);
          f16_load_pair<CH>(q + P.row_stride, c, d);
        } else {
          const uint32_t y0 = umin(row + 2u * (uint32_t)dy, P.height - 1u), y1 = umin(row + 2u * (uint32_t)dy + 1u, P.height - 1u);
          const uint32_t x0 = umin(col + 2u * (uint32_t)dx, P.width - 1u), x1 = umin(col + 2u * (uint32_t)dx + 1u, P.width - 1u);
          const uint8_t *q0 = src + (uint64_t)y0 * P.row_stride, *q1 = src + (uint64_t)y1 * P.row_stride;
          a = f16_load_px<CH>(q0 + (uint64_t)x0 * kBpp);
          b = f16_load_px<CH>(q0 + (uint64_t)x1 * kBpp);
          c = f16_load_px<CH>(q1 + (uint64_t)x0 * kBpp);
          d = f16_load_px<CH>(q1 + (uint64_t)x1 * kBpp);
        }
        lds[(2u * by + (uint32_t)dy) * 64u + 2u * bx + (uint32_t)dx] = f16_filter_px<CH>(a, b, c, d);
      }
  }
  __syncthreads();
  // levels 2 .. jmax from the level above, one barrier per halving
  for (uint32_t j = 2; j <= jmax; ++j) {
    const MipLevel Lp = mip_level(P, j - 1u, tx, ty);
    const uint32_t lg = 7u - j, sp = kMipTile >> (j - 1u);
    const uint32_t sx = Lp.vw >= 2u ? 1u : 0u, sy = Lp.vh >= 2u ? sp : 0u;  // (w_{j-1} == 1: x1 = x0)
    const Px16 *prev = lds + mip_lds_off(j - 1u);
    for (uint32_t p = tid; p < (1u << (2u * lg)); p += kThreadsPerWorkgroup) {
      const uint32_t x = p & ((1u << lg) - 1u), y = p >> lg;
      const Px16 *q = prev + 2u * y * sp + 2u * x;
      lds[mip_lds_off(j) + p] = f16_filter_px<CH>(q[0], q[sx], q[sy], q[sy + sx]);
    }
    __syncthreads();
  }
  // the levels' pixels: tight rows
  for (uint32_t j = 1; j <= jmax; ++j) {
    if (!((mask >> j) & 1u)) continue;
    const MipLevel L = mip_level(P, j, tx, ty);
    const uint32_t lg = 7u - j;
    uint8_t *out = P.pix + (uint64_t)blockIdx.z * P.pix_image_stride + P.pix_off[j];
    for (uint32_t p = tid; p < (1u << (2u * lg)); p += kThreadsPerWorkgroup) {
      const uint32_t x = p & ((1u << lg) - 1u), y = p >> lg;
      if (x >= L.vw || y >= L.vh) continue;
      f16_store_px<CH>(out + ((uint64_t)(L.y0 + y) * L.w + L.x0 + x) * kBpp, lds[mip_lds_off(j) + p]);
    }
  }
}

}  // namespace

extern "C" {
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_mip_pyramid_rgb16f_kernel(MipParams P) { mip_f16_pass<3>(P); }
__global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_mip_pyramid_rgba16f_kernel(MipParams P) { mip_f16_pass<4>(P); }
}  // extern "C"

const char *mip_f16_kernel_name(int chans) {
  return chans == 3 ? "icamd_mip_pyramid_rgb16f_kernel" : chans == 4 ? "icamd_mip_pyramid_rgba16f_kernel" : "";
}

hipError_t launch_mip_f16_pass(int chans, const MipPassPlan &pass, const MipBuffers &buffers, hipStream_t stream) {
  if (chans != 3 && chans != 4) return hipErrorInvalidValue;
  return launch_mip_kernel(chans == 3 ? icamd_mip_pyramid_rgb16f_kernel : icamd_mip_pyramid_rgba16f_kernel, pass, buffers, false, stream);
}

}  // namespace icamd
