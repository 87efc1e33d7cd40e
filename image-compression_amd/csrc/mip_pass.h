// mip_pass.h -- the fused mip-chain pass (and the plain pixel pyramid) for gfx950 (include/ic_amd.h, mip-chain section), shared
// by mip_kernels.hip (the box filter), mip_filter_kernels.hip (the sRGB / alpha-weighted filters, mip_filter.h) and
// mip_normal_kernels.hip (the normal-map filter, mip_normal.h).  Device code only: which passes a call runs, on which grids, and
// which kernels exist is mip_plan.h's.
//
// One pass reads an input level once and writes up to six (eight when the input is a single tile) levels of the chain:
//  * a 256-lane workgroup owns a 128 x 128-pixel tile of the input level; a lane encodes four of its 32 x 32 blocks straight
//    from global memory (rounds 0-3, the gather of icamd_encode_device: rows clamped to the image edge), and writes each
//    block's 2 x 2 filtered pixels -- its level-1 pixels -- to LDS (64 x 64 dwords, 16 KiB);
//  * one barrier later the tile's levels 2..6 are built in LDS from the level above (one halving per barrier, 5.3 KiB);
//  * the tile's blocks of levels 1..5 (256 + 64 + 16 + 4 + 1 = 341) are then encoded from LDS in two more rounds; the
//    second round's 85 blocks fill one wave and a third of another, which waves take them rotates with the workgroup
//    so that the extra round is spread over the four SIMDs;
//  * the tile's 2 x 2 level-6 pixels go to a handoff image (the caller's workspace), which the next pass takes as its input.
// A level's block past the image edge replicates the edge pixels (clamp to h_l - 1 / w_l - 1), exactly as the encoder
// does; the next level is built from real pixels only: in global coordinates x1 = min(2x + 1, w_l - 1), which differs
// from 2x + 1 only when w_l == 1.  For level 0 -> 1 the clamped gather already holds those pixels: a block's column
// 2j + 1 IS pixel min(4 bx + 2j + 1, w - 1).
// The pixel pyramid entry is the same kernel with no encoder: it writes levels 1..6 as tight COMPS-byte rows.
// A fused ETC1 kernel is deferred: ETC1 chains run the pyramid kernel + etc1_kernels.hip per level (ic_capi.hip).
// FILTER 1..3 adds the filter's tables to LDS (mip_filter_table_bytes), filled once per workgroup before the first round;
// FILTER 4 (normals) has no tables.
#ifndef ICAMD_MIP_PASS_H_
#define ICAMD_MIP_PASS_H_

#include "bc45_block.h"
#include "codec_info.h"
#include "dxt_block.h"
#include "ic_amd.h"
#include "ic_launch.h"
#include "mip_filter.h"
#include "mip_normal.h"

namespace icamd {

// dword offset of local level j (1..7) in LDS: level j is (128 >> j)^2 pixel dwords
constexpr uint32_t mip_lds_off(uint32_t j) { return j <= 1 ? 0u : mip_lds_off(j - 1) + (kMipTile >> (j - 1)) * (kMipTile >> (j - 1)); }
constexpr uint32_t kMipLdsDwords = mip_lds_off(8);  // 5461 dwords = 21 844 bytes
static_assert(kMipLdsDwords == 5461u, "LDS plan of the mip kernels");

// Level j of this pass as seen from tile (tx, ty): the level's size, the tile's origin in it and how many of the tile's
// (128 >> j)^2 pixels lie inside the level.
struct MipLevel {
  uint32_t w, h, x0, y0, vw, vh;
};
__device__ __forceinline__ MipLevel mip_level(const MipParams &P, uint32_t j, uint32_t tx, uint32_t ty) {
  MipLevel L;
  const uint32_t side = kMipTile >> j;
  L.w = umax(1u, P.width >> j);
  L.h = umax(1u, P.height >> j);
  // x0 <= w (tile tx starts at pixel 128 tx <= width - 1, so x0 = floor(128 tx / 2^j) <= w); x0 == w happens (width 129,
  // tile 1, level 1: x0 = 64 = w) and then vw == 0: the tile holds none of the level's pixels and reads or writes none of them
  L.x0 = tx * side;
  L.y0 = ty * side;
  L.vw = umin(side, L.w - L.x0);
  L.vh = umin(side, L.h - L.y0);
  return L;
}

struct __attribute__((packed, aligned(1))) U1 { uint32_t x; };

// One pixel of a COMPS-byte row as a dword in memory order (bytes past COMPS are 0 for 1 / 2, undefined for 3).
template <int COMPS>
__device__ __forceinline__ uint32_t load_pixel(const uint8_t *q) {
  uint32_t v = q[0];
  if (COMPS >= 2) v |= (uint32_t)q[1] << 8;
  if (COMPS >= 3) v |= (uint32_t)q[2] << 16;
  if (COMPS == 4) v |= (uint32_t)q[3] << 24;
  return v;
}

// The block at pixel (row, col) of a COMPS-byte image, clamped to its edge (pixel4x4.cc:23-59): four row loads inside the
// image, the byte gather at its edges.  64-bit addresses per lane: any stride the C ABI accepts.
template <int COMPS>
__device__ __forceinline__ void mip_load_block(const uint8_t *img, const MipParams &P, uint32_t row, uint32_t col, uint32_t px[16]) {
  if (P.height - row >= 4u && P.width - col >= 4u) {
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const uint8_t *r = img + (uint64_t)(row + (uint32_t)y) * P.row_stride + (uint64_t)col * COMPS;
      if (COMPS == 4) {
        const U4 v = load_stream(reinterpret_cast<const U4 *>(r));
        px[4 * y + 0] = v.x; px[4 * y + 1] = v.y; px[4 * y + 2] = v.z; px[4 * y + 3] = v.w;
      } else if (COMPS == 3) {
        const U3 v = load_stream(reinterpret_cast<const U3 *>(r));
        px[4 * y + 0] = v.x;
        px[4 * y + 1] = alignbit(v.y, v.x, 24);
        px[4 * y + 2] = alignbit(v.z, v.y, 16);
        px[4 * y + 3] = v.z >> 8;
      } else if (COMPS == 2) {
        const U2 v = load_stream(reinterpret_cast<const U2 *>(r));
        px[4 * y + 0] = v.x & 0xffffu; px[4 * y + 1] = v.x >> 16; px[4 * y + 2] = v.y & 0xffffu; px[4 * y + 3] = v.y >> 16;
      } else {
        const uint32_t v = reinterpret_cast<const U1 *>(r)->x;
        px[4 * y + 0] = v & 0xffu; px[4 * y + 1] = bfe(v, 8, 8); px[4 * y + 2] = bfe(v, 16, 8); px[4 * y + 3] = v >> 24;
      }
    }
  } else {
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const uint8_t *r = img + (uint64_t)umin(row + (uint32_t)y, P.height - 1u) * P.row_stride;
#pragma unroll
      for (int x = 0; x < 4; ++x) px[4 * y + x] = load_pixel<COMPS>(r + (uint64_t)umin(col + (uint32_t)x, P.width - 1u) * COMPS);
    }
  }
}

// The block's bytes through the same per-block encoders as icamd_encode_device (dxt_kernels.hip, bc45_kernels.hip).  No block of a mip level lies wholly outside it, so DXT5's / BC4's one_pixel case never arises.
template <int MODE>
__device__ __forceinline__ void mip_encode_store(const uint32_t px[16], bool swap, BlockStash &stash, uint8_t *out) {
  if (MODE == ICAMD_DXT1) {
    const Out8 c = encode_dxt_color_block(px, swap, false, stash);
    store_stream8(out, c.lo, c.hi);
  } else if (MODE == ICAMD_DXT5) {
    const Out8 a = encode_dxt5_alpha_block(px, false);
    const Out8 c = encode_dxt_color_block(px, swap, true, stash);
    store_stream16(out, a.lo, a.hi, c.lo, c.hi);
  } else if (MODE == ICAMD_BC4) {
    const Out8 a = swap ? encode_dxt5_alpha_block<2>(px, false) : encode_dxt5_alpha_block<0>(px, false);
    store_stream8(out, a.lo, a.hi);
  } else if (MODE == ICAMD_BC5) {
    const Out8 a = swap ? encode_dxt5_alpha_block<2>(px, false) : encode_dxt5_alpha_block<0>(px, false);
    const Out8 b = encode_dxt5_alpha_block<1>(px, false);
    store_stream16(out, a.lo, a.hi, b.lo, b.hi);
  }
}

template <int MODE, int COMPS, int FILTER>
__device__ __forceinline__ void mip_pass(const MipParams &P) {
  constexpr bool kEncode = MODE != kMipPyramidMode;
  constexpr bool kDxt = MODE == ICAMD_DXT1 || MODE == ICAMD_DXT5;
  constexpr uint32_t kBlockBytes = kEncode ? codec_block_bytes(MODE) : 0u;
  __shared__ uint32_t lds[kMipLdsDwords];
  __shared__ uint32_t lds_stash[kDxt ? 4 : 1][kDxt ? kThreadsPerWorkgroup : 1][4];
  BlockStash stash;
  stash.base = &lds_stash[0][kDxt ? threadIdx.x : 0][0];
  const uint32_t tid = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y + P.tile_row0;
  MipFilterTables ft = { nullptr, nullptr, nullptr };
  if constexpr (mip_filter_table_bytes(FILTER) != 0) {
    // the filter's tables, one copy per workgroup (256 lanes: one entry of T and M, four of R each)
    if constexpr ((FILTER & kMipFilterSrgb) != 0) {
      __shared__ uint16_t lds_to_linear[256], lds_midpoint[256];
      lds_to_linear[tid] = mip_filter_to_linear_entry(tid);
      lds_midpoint[tid] = mip_filter_midpoint_entry(tid);
      ft.to_linear = lds_to_linear;
      ft.midpoint = lds_midpoint;
    }
    if constexpr ((FILTER & kMipFilterAlphaWeighted) != 0) {
      __shared__ uint32_t lds_recip[1024];
#pragma unroll
      for (uint32_t i = 0; i < 4u; ++i) lds_recip[tid + 256u * i] = mip_filter_recip_entry(tid + 256u * i);
      ft.recip = lds_recip;
    }
    __syncthreads();
  }
  const uint8_t *src = P.src + (uint64_t)blockIdx.z * P.src_image_stride;
  uint8_t *dst = P.dst + (uint64_t)blockIdx.z * P.dst_image_stride;
  const bool swap = P.swap_rb != 0;
  const uint32_t tail_mask = (P.enc_mask | P.pix_mask) & ~1u;                  // local levels built in LDS
  const uint32_t jmax = tail_mask ? 31u - (uint32_t)__builtin_clz(tail_mask) : 0u;
  // blocks of levels 1..7 this tile encodes from LDS, dealt in rounds of 256
  uint32_t tail = 0;
#pragma unroll
  for (uint32_t j = 1; j <= 7; ++j)
    if ((P.enc_mask >> j) & 1u) tail += umax(1u, (32u >> j) * (32u >> j));
  const uint32_t rounds = 4u + (jmax ? umax(1u, (tail + 255u) >> 8) : 0u);
  // the lane's slot in the LDS rounds: waves rotated by a hash of the workgroup, so that the partial last round lands on
  // different SIMDs in neighbouring workgroups
  const uint32_t wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const uint32_t slot = ((((tid >> 6) + ((wg * 0x9e3779b1u) >> 30)) & 3u) << 6) | (tid & 63u);
  const MipLevel L0 = mip_level(P, 0, tx, ty);
  const uint32_t bw0 = (L0.w + 3u) >> 2;
#pragma nounroll
  for (uint32_t r = 0; r < rounds; ++r) {
    if (r == 4u) {
      // levels 2..jmax from the level above, one barrier per halving, then the pixel outputs (pyramid levels / handoff)
      __syncthreads();
      for (uint32_t j = 2; j <= jmax; ++j) {
        const MipLevel Lp = mip_level(P, j - 1u, tx, ty);
        const uint32_t lg = 7u - j, sp = kMipTile >> (j - 1u);
        const uint32_t sx = Lp.vw >= 2u ? 1u : 0u, sy = Lp.vh >= 2u ? sp : 0u;  // (w_{j-1} == 1: x1 = x0)
        const uint32_t *prev = lds + mip_lds_off(j - 1u);
        for (uint32_t p = tid; p < (1u << (2u * lg)); p += kThreadsPerWorkgroup) {
          const uint32_t x = p & ((1u << lg) - 1u), y = p >> lg;
          const uint32_t *q = prev + 2u * y * sp + 2u * x;
          if constexpr (FILTER == kMipFilterNormal) lds[mip_lds_off(j) + p] = mip_normal_px<COMPS>(q[0], q[sx], q[sy], q[sy + sx], swap);
          else lds[mip_lds_off(j) + p] = mip_filter_px<FILTER, COMPS>(q[0], q[sx], q[sy], q[sy + sx], ft);
        }
        __syncthreads();
      }
      for (uint32_t j = 1; j <= jmax; ++j) {
        if (!((P.pix_mask >> j) & 1u)) continue;
        const MipLevel L = mip_level(P, j, tx, ty);
        const uint32_t lg = 7u - j;
        uint8_t *out = P.pix + (uint64_t)blockIdx.z * P.pix_image_stride + P.pix_off[j];
        for (uint32_t p = tid; p < (1u << (2u * lg)); p += kThreadsPerWorkgroup) {
          const uint32_t x = p & ((1u << lg) - 1u), y = p >> lg;
          if (x >= L.vw || y >= L.vh) continue;
          const uint32_t v = lds[mip_lds_off(j) + p];
          uint8_t *q = out + ((uint64_t)(L.y0 + y) * L.w + L.x0 + x) * COMPS;
          if (COMPS == 4) {
            reinterpret_cast<U1 *>(q)->x = v;
          } else {
#pragma unroll
            for (int c = 0; c < COMPS; ++c) q[c] = (uint8_t)(v >> (8 * c));
          }
        }
      }
    }
    uint32_t px[16];
    bool have;
    uint8_t *out = nullptr;
    if (r < 4u) {
      // level 0: block i of the tile's 32 x 32, from global memory
      const uint32_t i = tid + (r << 8), bx = i & 31u, by = i >> 5;
      const uint32_t row = (ty * 32u + by) * 4u, col = (tx * 32u + bx) * 4u;
      have = row < L0.h && col < L0.w;
      if (have) {
        mip_load_block<COMPS>(src, P, row, col, px);
        if (jmax) {
#pragma unroll
          for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
              const int q = 8 * dy + 2 * dx;
              uint32_t &next = lds[(2u * by + (uint32_t)dy) * 64u + 2u * bx + (uint32_t)dx];
              if constexpr (FILTER == kMipFilterNormal) next = mip_normal_px<COMPS>(px[q], px[q + 1], px[q + 4], px[q + 5], swap);
              else next = mip_filter_px<FILTER, COMPS>(px[q], px[q + 1], px[q + 4], px[q + 5], ft);
            }
        }
        out = dst + P.level_off[0] + ((uint64_t)(row >> 2) * bw0 + (col >> 2)) * kBlockBytes;
      }
      have = have && (P.enc_mask & 1u);
    } else {
      // levels 1..7: the tile's blocks in level order, from LDS
      uint32_t f = slot + ((r - 4u) << 8), j = 0;
      have = f < tail;
#pragma unroll
      for (uint32_t k = 1; k <= 7; ++k) {
        const uint32_t c = umax(1u, (32u >> k) * (32u >> k));
        if (!j && ((P.enc_mask >> k) & 1u)) {
          if (f < c) j = k;
          else f -= c;
        }
      }
      if (have) {
        const MipLevel L = mip_level(P, j, tx, ty);
        const uint32_t lgb = j < 5u ? 5u - j : 0u, bx = f & ((1u << lgb) - 1u), by = f >> lgb;
        const uint32_t side = kMipTile >> j;
        have = bx * 4u < L.vw && by * 4u < L.vh;
        if (have) {
          const uint32_t *lv = lds + mip_lds_off(j);
#pragma unroll
          for (int y = 0; y < 4; ++y) {
            const uint32_t yy = umin(by * 4u + (uint32_t)y, L.vh - 1u) * side;
#pragma unroll
            for (int x = 0; x < 4; ++x) px[4 * y + x] = lv[yy + umin(bx * 4u + (uint32_t)x, L.vw - 1u)];
          }
          const uint32_t bw = (L.w + 3u) >> 2;
          out = dst + P.level_off[j] + ((uint64_t)((L.y0 >> 2) + by) * bw + (L.x0 >> 2) + bx) * kBlockBytes;
        }
      }
    }
    if (kEncode && have) mip_encode_store<MODE>(px, swap, stash, out);
  }
}

// A row of mip_plan.h's kernel list as its kernel: each mip translation unit defines its own sub-list.
#define ICAMD_MIP_DEFINE_KERNEL(name, mode, comps, filter) \
  __global__ void __launch_bounds__(kThreadsPerWorkgroup) name(MipParams P) { mip_pass<mode, comps, filter>(P); }

}  // namespace icamd
#endif  // ICAMD_MIP_PASS_H_
