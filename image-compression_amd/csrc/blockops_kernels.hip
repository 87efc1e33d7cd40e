// blockops_kernels.hip -- Pad / Downsample / DXT1->ETC1, DXT5->ETC2 RGBA8, DXT1->ETC2 RGB8, BC4->EAC R11 and BC5->EAC RG11
// transcode kernels: one output block per lane, coalesced 8/16-byte block loads and stores.  See blockops_block.h for the per-block math and
// blockops_plan.h for which kernel a call gets, with which grid: the launchers at the end of this file run what the plan says.
#include <cstdlib>
#include "blockops_block.h"
#include "transcode5_block.h"
#include "transcode_family_block.h"
#include "ic_launch.h"
#include "ic_amd.h"

namespace icamd {

static_assert(kBlockOpDxt1 == ICAMD_DXT1 && kBlockOpDxt5 == ICAMD_DXT5 && kBlockOpEtc1 == ICAMD_ETC1, "blockops_plan.h codecs");
static_assert(kBlockOpLanes == kThreadsPerWorkgroup, "blockops_plan.h workgroup");

namespace {
constexpr int kWords(int codec) { return codec == ICAMD_DXT5 ? 4 : 2; }
}

// What a Pad kernel's work items are: every output block, pad blocks made on the way (DXT); every output block, only the image's
// own written (the ETC1 copy); the pad blocks alone, one lane each; the pad blocks alone, four lanes each (kSmallerError)
enum PadPart : int { kPadWhole = 0, kPadCopy = 1, kPadBorder = 2, kPadBorderQuad = 3 };

// Border block k of an image -> (r, c): the in_rows x extra columns right of the image first, then the extra rows over the full width
struct RowCol { uint32_t r, c; };
__device__ __forceinline__ RowCol pad_border_rc(const BlockOpParams &P, uint32_t k) {
  const uint32_t dc = P.out_cols - P.in_cols, right = P.in_rows * dc;
  uint32_t r, c;
  if (k < right) { r = k / dc; c = P.in_cols + (k - r * dc); }
  else { const uint32_t j = k - right; r = P.in_rows + j / P.out_cols; c = j - (r - P.in_rows) * P.out_cols; }
  return { r, c };
}

// (r, c) of an output block: the source block it copies / replicates, and whether it is a pad block.
template <int CODEC, int STRATEGY>
__device__ __forceinline__ void pad_block(const BlockOpParams &P, uint32_t img, uint32_t r, uint32_t c, bool copy_interior,
                                          bool make_border) {
  constexpr int W = kWords(CODEC);
  const uint32_t *src = reinterpret_cast<const uint32_t *>(P.src + (size_t)img * P.src_image_stride);
  uint32_t *dst = reinterpret_cast<uint32_t *>(P.dst + (size_t)img * P.dst_image_stride) + ((size_t)r * P.out_cols + c) * W;
  const bool in_rows = r < P.in_rows, in_cols = c < P.in_cols;
  if (in_rows && in_cols ? !copy_interior : !make_border) return;
  const uint32_t sr = in_rows ? r : P.in_rows - 1, sc = in_cols ? c : P.in_cols - 1;
  const uint32_t *s = src + ((size_t)sr * P.in_cols + sc) * W;
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < W; ++i) w[i] = s[i];
  if (in_rows && in_cols) {
#pragma unroll
    for (int i = 0; i < W; ++i) dst[i] = w[i];
    return;
  }
  const int kind = in_rows ? kPadColumn : (in_cols ? kPadRow : kPadCorner);  // helper.h:427-470
  if (CODEC == ICAMD_ETC1) {
    const Out8 o = etc1_pad_block(w[0], w[1], kind, (uint32_t)STRATEGY);  // compile-time strategy: see downsample_one
    dst[0] = o.lo; dst[1] = o.hi;
  } else if (CODEC == ICAMD_DXT1) {
    dst[0] = w[0];
    dst[1] = dxt_pad_color_bits(w[1], kind);
  } else {
    uint32_t lo24 = w[0] >> 16 | (w[1] & 0xffu) << 16, hi24 = w[1] >> 8;
    dxt5_pad_alpha_codes(lo24, hi24, kind);
    dst[0] = (w[0] & 0xffffu) | lo24 << 16;
    dst[1] = lo24 >> 16 | hi24 << 8;
    dst[2] = w[2];
    dst[3] = dxt_pad_color_bits(w[3], kind);
  }
}

// DXT: one pass over the output grid (a pad block is a few bit edits).  ETC1 (r04): a pad block is a decode + re-encode -- up to
// the whole kSmallerError search -- so the copy of the image's own blocks runs as one light kernel over the grid (kPadCopy: 7 VGPRs,
// 8 waves per SIMD) and the pad blocks as a second, small launch over the BORDER only (kPadBorder); in one kernel the searches'
// 121 VGPRs capped the copy at 4 waves per SIMD and every wave that touched the border ran the search (28.6 -> ~7 us per 4096^2
// image padded by 8 pixels).
// Batched launches (icamd_pad_batch_device, r05): n_images equally shaped grids, out_per_image work items each (output blocks;
// kPadBorder: border blocks; kPadBorderQuad: border_lanes_per_image quad lanes).
template <int CODEC, int STRATEGY, int PART>
__device__ __forceinline__ void pad_one(const BlockOpParams &P, uint32_t k) {
  uint32_t img = 0;
  if (P.n_images > 1) {
    if (PART == kPadBorderQuad) {
      img = fastdiv(k, P.div_border_lanes_per_image);
      k -= img * P.border_lanes_per_image;
    } else {
      img = fastdiv(k, P.div_out_per_image);
      k -= img * P.out_per_image;
    }
  }
  if (PART == kPadBorderQuad) {  // kPadBorder with four lanes per pad block (kSmallerError): work item k = 4 * border block + quad lane
    const uint32_t t = k & 3u;
    k >>= 2;
    const RowCol at = pad_border_rc(P, k);
    const uint32_t r = at.r, c = at.c;
    // (its own addressing: sharing pad_block's changed the instruction order of every Pad kernel)
    const bool in_rows = r < P.in_rows, in_cols = c < P.in_cols;
    const uint32_t sr = in_rows ? r : P.in_rows - 1, sc = in_cols ? c : P.in_cols - 1;
    const uint32_t *s = reinterpret_cast<const uint32_t *>(P.src + (size_t)img * P.src_image_stride) + ((size_t)sr * P.in_cols + sc) * 2;
    uint32_t *dst = reinterpret_cast<uint32_t *>(P.dst + (size_t)img * P.dst_image_stride) + ((size_t)r * P.out_cols + c) * 2;
    bool writes = false;
    const Out8 o = etc1_pad_block_quad(s[0], s[1], in_rows ? kPadColumn : (in_cols ? kPadRow : kPadCorner), t, &writes);
    if (writes) { dst[0] = o.lo; dst[1] = o.hi; }
    return;
  }
  if (PART == kPadBorder) {
    const RowCol at = pad_border_rc(P, k);
    pad_block<CODEC, STRATEGY>(P, img, at.r, at.c, false, true);
    return;
  }
  const uint32_t r = fastdiv(k, P.div_out_cols), c = k - r * P.out_cols;
  pad_block<CODEC, STRATEGY>(P, img, r, c, true, PART == kPadWhole);
}

// STRATEGY: the ETC1 re-encode strategy as a compile-time constant (one kernel per strategy, like the encoders: the
// kSmallerError search is not carried along by a kHeuristic downsample and vice versa); ignored for DXT.
// QUAD (ETC1 kSmallerError, small grids -- the low levels of a mip chain): work item k = 4 * output block + quad lane; the four
// lanes build the same sixteen pixels and split the re-encode's searches (etc1_block.h encode_etc1_block_quad).
// (img, r, c): image of a batched launch and the output block's position in its grid; kk = r * out_cols + c
template <int CODEC, int STRATEGY, bool QUAD = false>
__device__ __forceinline__ void downsample_at(const BlockOpParams &P, uint32_t img, uint32_t r, uint32_t c, uint32_t kk,
                                              uint32_t quad_lane, BlockStash &stash) {
  constexpr int W = kWords(CODEC);
  const uint32_t *src = reinterpret_cast<const uint32_t *>(P.src + (size_t)img * P.src_image_stride);
  uint32_t px[16], tmp[16];
  if (P.in_rows > 1 && P.in_cols > 1) {  // DownsampleBlocks2x2
    if (CODEC != ICAMD_ETC1) {
      // the two blocks of a source row are adjacent in memory: one 16-byte (DXT1) / two 16-byte (DXT5) loads per row
      uint32_t w[2][2][W];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t *q = src + ((size_t)(2 * r + i) * P.in_cols + 2 * c) * W;
#pragma unroll
        for (int h = 0; h < 2 * W / 4; ++h) {
          const U4 v = *reinterpret_cast<const U4 *>(q + 4 * h);
          uint32_t *d = &w[0][0][0] + (i * 2 * W + 4 * h);
          d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
      }
      const uint32_t *const s4[2][2] = { { w[0][0], w[0][1] }, { w[1][0], w[1][1] } };
      dxt_downsample_2x2<CODEC>(s4, px);
    } else {
      uint32_t w[2][2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const U4 v = *reinterpret_cast<const U4 *>(src + ((size_t)(2 * r + i) * P.in_cols + 2 * c) * 2);
        w[i][0][0] = v.x; w[i][0][1] = v.y; w[i][1][0] = v.z; w[i][1][1] = v.w;
      }
      const uint32_t *const s4[2][2] = { { w[0][0], w[0][1] }, { w[1][0], w[1][1] } };
      etc1_downsample_2x2(s4, px);
    }
  } else if (P.in_rows > 1) {  // DownsampleBlocks2x1: one block column
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      decode_any<CODEC>(src + (size_t)(2 * r + i) * W, tmp);
      store_downsampled(tmp, 2 * i, 0, px);
      store_downsampled(tmp, 2 * i, 2, px);
    }
  } else if (P.in_cols > 1) {  // DownsampleBlocks1x2: one block row
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      decode_any<CODEC>(src + (size_t)(2 * c + j) * W, tmp);
      store_downsampled(tmp, 0, 2 * j, px);
      store_downsampled(tmp, 2, 2 * j, px);
    }
  } else {  // a single block of 4, 2 or 1 pixels per side: replicate to 4x4 first (helper.h:338-387)
    decode_any<CODEC>(src, tmp);
    if (P.src_width == 1) {
#pragma unroll
      for (int y = 0; y < 4; ++y) tmp[4 * y + 1] = tmp[4 * y + 2] = tmp[4 * y + 3] = tmp[4 * y];
    } else if (P.src_width == 2) {
#pragma unroll
      for (int y = 0; y < 4; ++y) { tmp[4 * y + 2] = tmp[4 * y]; tmp[4 * y + 3] = tmp[4 * y + 1]; }
    }
    if (P.src_height == 1) {
#pragma unroll
      for (int x = 0; x < 4; ++x) tmp[4 + x] = tmp[8 + x] = tmp[12 + x] = tmp[x];
    } else if (P.src_height == 2) {
#pragma unroll
      for (int x = 0; x < 4; ++x) { tmp[8 + x] = tmp[x]; tmp[12 + x] = tmp[4 + x]; }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) store_downsampled(tmp, 2 * i, 2 * j, px);
  }
  uint8_t *dst = P.dst + (size_t)img * P.dst_image_stride + (size_t)kk * (W * 4);
  if (QUAD) {
    bool writes = false;
    const Out8 o = encode_etc1_block_quad(px, quad_lane, &writes);
    if (writes) store_stream8(dst, o.lo, o.hi);
    return;
  }
  uint32_t out[4];
  encode_any<CODEC>(px, CODEC == ICAMD_ETC1 ? (uint32_t)STRATEGY : 0u, stash, out);
  if (W == 4) store_stream16(dst, out[0], out[1], out[2], out[3]);
  else store_stream8(dst, out[0], out[1]);
}
// work item k of a linear launch -> (image, row, column) by two multiply-high divisions
template <int CODEC, int STRATEGY, bool QUAD = false>
__device__ __forceinline__ void downsample_one(const BlockOpParams &P, uint32_t k, BlockStash &stash) {
  const uint32_t quad_lane = QUAD ? (k & 3u) : 0u;
  if (QUAD) k >>= 2;
  uint32_t img = 0, kk = k;
  if (P.n_images > 1) {
    img = fastdiv(k, P.div_out_per_image);
    kk = k - img * P.out_per_image;
  }
  const uint32_t r = fastdiv(kk, P.div_out_cols), c = kk - r * P.out_cols;
  downsample_at<CODEC, STRATEGY, QUAD>(P, img, r, c, kk, quad_lane, stash);
}

// Lanes per workgroup: blockop_lanes (blockops_plan.h), one wave where the kernel runs an ETC1 search per block.
#define ICAMD_PAD_KERNEL(NAME, CODEC, STRATEGY, PART)                                                          \
  extern "C" __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_pad_##NAME##_kernel(BlockOpParams P) { \
    const uint32_t k = blockIdx.x * blockop_lanes(CODEC, STRATEGY, PART == kPadCopy) + threadIdx.x;            \
    if (k < P.total_out) pad_one<CODEC, STRATEGY, PART>(P, k);                                                 \
  }
// the per-lane pixel stash of the Downsample kernels: only the DXT colour encoder uses it
#define ICAMD_DOWNSAMPLE_STASH(CODEC)                                                                          \
  __shared__ uint32_t lds_px[CODEC == ICAMD_ETC1 ? 1 : 4][CODEC == ICAMD_ETC1 ? 1 : kThreadsPerWorkgroup][4];  \
  BlockStash stash;                                                                                            \
  stash.base = CODEC == ICAMD_ETC1 ? &lds_px[0][0][0] : &lds_px[0][threadIdx.x][0];
#define ICAMD_DOWNSAMPLE_KERNEL(NAME, CODEC, STRATEGY)                                                         \
  extern "C" __global__ void __launch_bounds__(kThreadsPerWorkgroup)                                           \
  icamd_downsample_##NAME##_kernel(BlockOpParams P) {                                                          \
    ICAMD_DOWNSAMPLE_STASH(CODEC)                                                                              \
    const uint32_t k = blockIdx.x * blockop_lanes(CODEC, STRATEGY, false) + threadIdx.x;                       \
    if (k < P.total_out) downsample_one<CODEC, STRATEGY>(P, k, stash);                                         \
  }

// ROW TILES (r06; grids of at least 256 output columns, DXT and ETC1 kHeuristic): blockIdx = (column tile, output row, image),
// so image and row are workgroup-uniform -- the two multiply-high divisions, their quarter-rate multiplies back and the 64-bit
// row addressing move to the scalar unit, a lane adds a 32-bit column offset (the encoders' tile form).
#define ICAMD_DOWNSAMPLE_ROWS_KERNEL(NAME, CODEC, STRATEGY)                                                    \
  extern "C" __global__ void __launch_bounds__(kThreadsPerWorkgroup)                                           \
  icamd_downsample_##NAME##_rows_kernel(BlockOpParams P) {                                                     \
    ICAMD_DOWNSAMPLE_STASH(CODEC)                                                                              \
    const uint32_t c = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x, r = blockIdx.y, img = blockIdx.z;      \
    if (c < P.out_cols) downsample_at<CODEC, STRATEGY>(P, img, r, c, r * P.out_cols + c, 0u, stash);           \
  }
ICAMD_PAD_KERNEL(dxt1, ICAMD_DXT1, 0, kPadWhole)
ICAMD_PAD_KERNEL(dxt5, ICAMD_DXT5, 0, kPadWhole)
ICAMD_PAD_KERNEL(etc1_copy, ICAMD_ETC1, 0, kPadCopy)
ICAMD_PAD_KERNEL(etc1_border_split_h, ICAMD_ETC1, 0, kPadBorder)
ICAMD_PAD_KERNEL(etc1_border_split_v, ICAMD_ETC1, 1, kPadBorder)
ICAMD_PAD_KERNEL(etc1_border, ICAMD_ETC1, 2, kPadBorder)
ICAMD_PAD_KERNEL(etc1_border_heuristic, ICAMD_ETC1, 3, kPadBorder)
// kSmallerError (r05): four lanes per pad block, and -- the split search needs 61 VGPRs where the whole one needed 121, so the
// copy no longer loses occupancy to it -- in the SAME launch as the copy of the image's own blocks: the first border_wgs
// workgroups are the pad blocks (they start first and are the long ones), the others copy.  One launch per Pad call.
extern "C" __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_pad_etc1_quad_kernel(BlockOpParams P) {
  if (blockIdx.x < P.border_wgs) {
    const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
    if (k < P.border_lanes) pad_one<ICAMD_ETC1, 2, kPadBorderQuad>(P, k);
  } else {
    const uint32_t k = (blockIdx.x - P.border_wgs) * kThreadsPerWorkgroup + threadIdx.x;
    if (k < P.total_out) pad_one<ICAMD_ETC1, 2, kPadCopy>(P, k);
  }
}
ICAMD_DOWNSAMPLE_KERNEL(dxt1, ICAMD_DXT1, 0)
ICAMD_DOWNSAMPLE_KERNEL(dxt5, ICAMD_DXT5, 0)
ICAMD_DOWNSAMPLE_KERNEL(etc1_split_h, ICAMD_ETC1, 0)
ICAMD_DOWNSAMPLE_KERNEL(etc1_split_v, ICAMD_ETC1, 1)
ICAMD_DOWNSAMPLE_KERNEL(etc1, ICAMD_ETC1, 2)  // kSmallerError (and every value the reference's default: label maps to it)
ICAMD_DOWNSAMPLE_KERNEL(etc1_heuristic, ICAMD_ETC1, 3)
ICAMD_DOWNSAMPLE_ROWS_KERNEL(dxt1, ICAMD_DXT1, 0)
ICAMD_DOWNSAMPLE_ROWS_KERNEL(dxt5, ICAMD_DXT5, 0)
ICAMD_DOWNSAMPLE_ROWS_KERNEL(etc1_heuristic, ICAMD_ETC1, 3)
// kSmallerError on grids of at most kDownsampleQuadMaxBlocks output blocks (r05, blockops_plan.h): four lanes per output block.
extern "C" __global__ void __launch_bounds__(64) icamd_downsample_etc1_quad_kernel(BlockOpParams P) {
  BlockStash stash;
  stash.base = nullptr;  // (only the DXT colour encoder parks pixels)
  const uint32_t k = blockIdx.x * 64u + threadIdx.x;
  if ((k >> 2) < P.total_out) downsample_one<ICAMD_ETC1, 2, true>(P, k, stash);
}

extern "C" __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_dxt1_to_etc1_kernel(uint2 *blocks, uint32_t n) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k >= n) return;
  const uint2 b = blocks[k];
  // DecodeDxt1Block(block, swap = false) + EncodeEtc1Block(..., kHeuristic), without materialising the pixels
  const Out8 o = transcode_dxt1_block_to_etc1(b.x, b.y);
  blocks[k] = make_uint2(o.lo, o.hi);
}

// DXT5 -> ETC2 RGBA8 in place (EXTENSION; transcode5_block.h): one block per lane, one 16-byte load and one
// 16-byte store.  One-wave workgroups, as the kernels that run an ETC1 search (blockops_plan.h runs_etc1_search): the kernel is
// the EAC search -- up to 144 candidates of 139 VALU instructions each as compiled, nothing in LDS, two dwords of state -- whose length depends on
// the content (a wave of flat or 0 / 255 alpha leaves after the first candidates), and a one-wave workgroup gives its slot back
// when it is done instead of waiting for the slowest of four.
extern "C" __global__ void __launch_bounds__(kSearchLanes) icamd_transcode_dxt5_to_etc2_rgba8_kernel(uint4 *blocks, uint32_t n) {
  const uint32_t k = blockIdx.x * kSearchLanes + threadIdx.x;
  if (k >= n) return;
  const uint4 b = blocks[k];
  const uint32_t w[4] = { b.x, b.y, b.z, b.w };
  uint32_t o[4];
  transcode_dxt5_block_to_etc2_rgba8(w, o);
  blocks[k] = make_uint4(o[0], o[1], o[2], o[3]);
}

// DXT1 -> ETC2 RGB8, BC4 -> EAC R11, BC5 -> EAC RG11 in place (EXTENSIONS; transcode_family_block.h): one block
// per lane, one 8- or 16-byte load and one store of the same size.  The DXT1 kernel has no search and keeps the four-wave
// workgroups of the DXT1 -> ETC1 kernel; the two EAC kernels are the palette search of the DXT5 kernel (twice, back to back,
// for BC5) and take its one-wave workgroups for the same reason.
extern "C" __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_transcode_dxt1_to_etc2_rgb8_kernel(uint2 *blocks, uint32_t n) {
  const uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x;
  if (k >= n) return;
  const uint2 b = blocks[k];
  const Out8 o = transcode_dxt1_block_to_etc2_rgb8(b.x, b.y);
  blocks[k] = make_uint2(o.lo, o.hi);
}
extern "C" __global__ void __launch_bounds__(kSearchLanes) icamd_transcode_bc4_to_eac_r11_kernel(uint2 *blocks, uint32_t n) {
  const uint32_t k = blockIdx.x * kSearchLanes + threadIdx.x;
  if (k >= n) return;
  const uint2 b = blocks[k];
  const Out8 o = transcode_bc4_block_to_eac_r11(b.x, b.y);
  blocks[k] = make_uint2(o.lo, o.hi);
}
extern "C" __global__ void __launch_bounds__(kSearchLanes) icamd_transcode_bc5_to_eac_rg11_kernel(uint4 *blocks, uint32_t n) {
  const uint32_t k = blockIdx.x * kSearchLanes + threadIdx.x;
  if (k >= n) return;
  const uint4 b = blocks[k];
  const uint32_t w[4] = { b.x, b.y, b.z, b.w };
  uint32_t o[4];
  transcode_bc5_block_to_eac_rg11(w, o);
  blocks[k] = make_uint4(o[0], o[1], o[2], o[3]);
}

// ICAMD_PAD_BORDER_QUAD=0: one lane per pad block, the r04 form; read once.  Kept: the GPU tests run both forms through it.
static bool pad_border_quad() {
  static const bool on = [] { const char *e = getenv("ICAMD_PAD_BORDER_QUAD"); return !(e && e[0] == '0'); }();
  return on;
}

// The kernels of the plan's BlockOpKernel values
using BlockOpKernelFn = void (*)(BlockOpParams);
static constexpr BlockOpKernelFn kBlockOpKernelFns[kBlockOpKernels] = {
  icamd_pad_dxt1_kernel, icamd_pad_dxt5_kernel, icamd_pad_etc1_copy_kernel, icamd_pad_etc1_border_split_h_kernel,
  icamd_pad_etc1_border_split_v_kernel, icamd_pad_etc1_border_kernel, icamd_pad_etc1_border_heuristic_kernel, icamd_pad_etc1_quad_kernel,
  icamd_downsample_dxt1_kernel, icamd_downsample_dxt5_kernel, icamd_downsample_etc1_split_h_kernel, icamd_downsample_etc1_split_v_kernel,
  icamd_downsample_etc1_kernel, icamd_downsample_etc1_heuristic_kernel, icamd_downsample_dxt1_rows_kernel,
  icamd_downsample_dxt5_rows_kernel, icamd_downsample_etc1_heuristic_rows_kernel, icamd_downsample_etc1_quad_kernel };

// Runs a plan: each group of images, each of its launches, BlockOpParams filled here from the call and the plan.
static hipError_t launch_blockop(const BlockOpCall &call, const BlockOpPlan &plan, hipStream_t stream) {
  if (plan.form == kBlockOpRefused) return hipErrorInvalidValue;
  if (plan.form == kBlockOpNothing) return hipSuccess;
  const BlockOpIn &in = call.in;
  for (uint64_t first = 0; first < in.n_images; first += plan.group) {
    const BlockOpGroup &g = in.n_images - first >= plan.group ? plan.full : plan.tail;
    for (const BlockOpLaunch &l : g.launch) {
      if (l.kernel == kNoKernel) continue;
      BlockOpParams P;
      P.src = call.src + first * call.src_image_stride;
      P.dst = call.dst + first * call.dst_image_stride;
      P.in_rows = in.in_rows; P.in_cols = in.in_cols;
      P.out_rows = in.out_rows; P.out_cols = in.out_cols;
      P.total_out = l.items;
      P.etc_strategy = in.etc_strategy;
      P.src_height = in.src_height; P.src_width = in.src_width;
      P.div_out_cols = make_fastdiv(in.out_cols);
      P.n_images = g.count;
      P.out_per_image = l.items_per_image;
      P.div_out_per_image = make_fastdiv(l.items_per_image);
      P.src_image_stride = call.src_image_stride;
      P.dst_image_stride = call.dst_image_stride;
      if (g.form == kPadQuad) {
        P.border_wgs = g.border_wgs;
        P.border_lanes = g.border_lanes;
        P.border_lanes_per_image = plan.border_lanes_per_image;
        P.div_border_lanes_per_image = make_fastdiv(plan.border_lanes_per_image);
      }
      hipLaunchKernelGGL(kBlockOpKernelFns[l.kernel], dim3(l.grid_x, l.grid_y, l.grid_z), dim3(l.lanes), 0, stream, P);
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

hipError_t launch_pad(BlockOpCall call, hipStream_t stream) {
  if (call.in.codec < ICAMD_DXT1 || call.in.codec > ICAMD_ETC1) return hipErrorInvalidValue;
  call.in.quad = pad_border_quad();
  return launch_blockop(call, pad_plan(call.in), stream);
}

hipError_t launch_downsample(BlockOpCall call, hipStream_t stream) {
  if (call.in.codec < ICAMD_DXT1 || call.in.codec > ICAMD_ETC1) return hipErrorInvalidValue;
  call.in.quad = pad_border_quad();  // (the same A/B switch as the Pad border: ICAMD_PAD_BORDER_QUAD=0)
  return launch_blockop(call, downsample_plan(call.in), stream);
}

hipError_t launch_transcode_dxt1_to_etc1(void *blocks, uint64_t n_blocks, hipStream_t stream) {
  hipError_t err = hipSuccess;
  for_chunks(n_blocks, kTranscodeChunk, [&](uint64_t first, uint64_t count) {
    if (err != hipSuccess) return;
    hipLaunchKernelGGL(icamd_dxt1_to_etc1_kernel, dim3((uint32_t)((count + kThreadsPerWorkgroup - 1) / kThreadsPerWorkgroup)),
                       dim3(kThreadsPerWorkgroup), 0, stream, static_cast<uint2 *>(blocks) + first, (uint32_t)count);
    err = hipGetLastError();
  });
  return err;
}

hipError_t launch_transcode_dxt5_to_etc2_rgba8(void *blocks, uint64_t n_blocks, hipStream_t stream) {
  hipError_t err = hipSuccess;
  for_chunks(n_blocks, kTranscode16Chunk, [&](uint64_t first, uint64_t count) {
    if (err != hipSuccess) return;
    hipLaunchKernelGGL(icamd_transcode_dxt5_to_etc2_rgba8_kernel, dim3((uint32_t)((count + kSearchLanes - 1) / kSearchLanes)),
                       dim3(kSearchLanes), 0, stream, static_cast<uint4 *>(blocks) + first, (uint32_t)count);
    err = hipGetLastError();
  });
  return err;
}

// The launches blockops_plan.h cuts a buffer of n_blocks into (transcode_launch), each with its kernel's lanes per workgroup
template <typename Block>
static hipError_t launch_transcode_family(void (*kernel)(Block *, uint32_t), uint32_t lanes, void *blocks, uint64_t n_blocks,
                                          hipStream_t stream) {
  for (uint64_t i = 0; i < transcode_launches(n_blocks); ++i) {
    const TranscodeLaunch l = transcode_launch(n_blocks, (uint32_t)sizeof(Block), lanes, i);
    hipLaunchKernelGGL(kernel, dim3(l.grid_x), dim3(l.lanes), 0, stream, static_cast<Block *>(blocks) + l.first_block, l.blocks);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}
hipError_t launch_transcode_dxt1_to_etc2_rgb8(void *blocks, uint64_t n_blocks, hipStream_t stream) {
  return launch_transcode_family<uint2>(icamd_transcode_dxt1_to_etc2_rgb8_kernel, kThreadsPerWorkgroup, blocks, n_blocks, stream);
}
hipError_t launch_transcode_bc4_to_eac_r11(void *blocks, uint64_t n_blocks, hipStream_t stream) {
  return launch_transcode_family<uint2>(icamd_transcode_bc4_to_eac_r11_kernel, kSearchLanes, blocks, n_blocks, stream);
}
hipError_t launch_transcode_bc5_to_eac_rg11(void *blocks, uint64_t n_blocks, hipStream_t stream) {
  return launch_transcode_family<uint4>(icamd_transcode_bc5_to_eac_rg11_kernel, kSearchLanes, blocks, n_blocks, stream);
}

// ---- CreateSolidImage / CopySubimage on device-resident block grids (helper.h:522-592) ----

// One block replicated n times: lane i of the grid-stride loop writes block i (8 or 16 bytes, streaming stores; the
// pointer only needs the 4-byte alignment of the other block-domain operations).
struct FillParams {
  uint8_t *dst;
  uint64_t n_blocks;
  uint32_t w[4];
  uint32_t words;  // 2 or 4
};
// n <= kFillBatch images of blocks_per_image blocks each, image i filled with its own block w[i] (icamd_create_solid_batch_device)
struct FillBatchParams {
  uint8_t *dst;
  uint64_t dst_image_stride;
  uint32_t blocks_per_image, words, n;
  uint32_t w[kFillBatch][4];
};
extern "C" __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_fill_blocks_batch_kernel(FillBatchParams P) {
  const uint32_t img = blockIdx.y;
  uint8_t *dst = P.dst + (size_t)img * P.dst_image_stride;
  const uint32_t w0 = P.w[img][0], w1 = P.w[img][1], w2 = P.w[img][2], w3 = P.w[img][3];
  const uint32_t stride = gridDim.x * kThreadsPerWorkgroup;
  for (uint32_t k = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x; k < P.blocks_per_image; k += stride) {
    if (P.words == 4) store_stream16(dst + (size_t)k * 16u, w0, w1, w2, w3);
    else store_stream8(dst + (size_t)k * 8u, w0, w1);
  }
}
extern "C" __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_fill_blocks_kernel(FillParams P) {
  const uint64_t stride = (uint64_t)gridDim.x * kThreadsPerWorkgroup;
  for (uint64_t k = (uint64_t)blockIdx.x * kThreadsPerWorkgroup + threadIdx.x; k < P.n_blocks; k += stride) {
    if (P.words == 4) store_stream16(P.dst + k * 16u, P.w[0], P.w[1], P.w[2], P.w[3]);
    else store_stream8(P.dst + k * 8u, P.w[0], P.w[1]);
  }
}

// Sub-rectangle of a block grid: output block (r, c) = source block (r0 + r, c0 + c); grid = (column chunks, rows),
// consecutive lanes = consecutive blocks of one row (coalesced on both sides).
struct SubimageParams {
  const uint8_t *src;
  uint8_t *dst;
  uint32_t src_cols, r0, c0, rows, cols, words, row_first;
  uint64_t src_image_stride, dst_image_stride;  // blockIdx.z = image (icamd_copy_subimage_batch_device)
};
extern "C" __global__ void __launch_bounds__(kThreadsPerWorkgroup) icamd_copy_subimage_kernel(SubimageParams P) {
  const uint32_t c = blockIdx.x * kThreadsPerWorkgroup + threadIdx.x, r = P.row_first + blockIdx.y;
  if (c >= P.cols) return;
  const size_t so = (size_t)blockIdx.z * P.src_image_stride + ((size_t)(P.r0 + r) * P.src_cols + P.c0 + c) * (P.words * 4u);
  const size_t dof = (size_t)blockIdx.z * P.dst_image_stride + ((size_t)r * P.cols + c) * (P.words * 4u);
  if (P.words == 4) {
    const U4 v = *reinterpret_cast<const U4 *>(P.src + so);
    store_stream16(P.dst + dof, v.x, v.y, v.z, v.w);
  } else {
    const U2 v = *reinterpret_cast<const U2 *>(P.src + so);
    store_stream8(P.dst + dof, v.x, v.y);
  }
}

hipError_t launch_fill_blocks(void *dst, uint64_t n_blocks, int block_bytes, const uint32_t words[4], hipStream_t stream) {
  if (n_blocks == 0) return hipSuccess;
  FillParams P;
  P.dst = static_cast<uint8_t *>(dst);
  P.n_blocks = n_blocks;
  P.words = (uint32_t)block_bytes / 4u;
  for (int i = 0; i < 4; ++i) P.w[i] = words[i];
  (void)hipGetLastError();
  hipLaunchKernelGGL(icamd_fill_blocks_kernel, dim3(fill_workgroups(n_blocks)), dim3(kThreadsPerWorkgroup), 0, stream, P);
  return hipGetLastError();
}

hipError_t launch_fill_blocks_batch(void *dst, uint64_t dst_image_stride, uint32_t blocks_per_image, int block_bytes,
                                    const uint32_t (*words)[4], uint32_t n_images, hipStream_t stream) {
  if (blocks_per_image == 0 || n_images == 0) return hipSuccess;
  (void)hipGetLastError();
  for_chunks(n_images, kFillBatch, [&](uint64_t first, uint64_t count) {
    FillBatchParams P;
    P.n = (uint32_t)count;
    P.dst = static_cast<uint8_t *>(dst) + first * dst_image_stride;
    P.dst_image_stride = dst_image_stride;
    P.blocks_per_image = blocks_per_image;
    P.words = (uint32_t)block_bytes / 4u;
    for (uint32_t i = 0; i < P.n; ++i)
      for (int j = 0; j < 4; ++j) P.w[i][j] = words[first + i][j];
    hipLaunchKernelGGL(icamd_fill_blocks_batch_kernel, dim3(fill_batch_workgroups(blocks_per_image, P.n), P.n),
                       dim3(kThreadsPerWorkgroup), 0, stream, P);
  });
  return hipGetLastError();
}

hipError_t launch_copy_subimage(int block_bytes, const void *src, uint32_t src_cols, uint32_t r0, uint32_t c0,
                                uint32_t rows, uint32_t cols, void *dst, hipStream_t stream, uint32_t n_images,
                                uint64_t src_image_stride, uint64_t dst_image_stride) {
  if (rows == 0 || cols == 0 || n_images == 0) return hipSuccess;
  SubimageParams P;
  P.src = static_cast<const uint8_t *>(src);
  P.dst = static_cast<uint8_t *>(dst);
  P.src_cols = src_cols; P.r0 = r0; P.c0 = c0; P.rows = rows; P.cols = cols;
  P.words = (uint32_t)block_bytes / 4u;
  P.src_image_stride = src_image_stride;
  P.dst_image_stride = dst_image_stride;
  (void)hipGetLastError();
  for_chunks(n_images, kGridLimitYZ, [&](uint64_t img0, uint64_t nz) {
    P.src = static_cast<const uint8_t *>(src) + img0 * src_image_stride;
    P.dst = static_cast<uint8_t *>(dst) + img0 * dst_image_stride;
    for_chunks(rows, kGridLimitYZ, [&](uint64_t row0, uint64_t ny) {
      P.row_first = (uint32_t)row0;
      hipLaunchKernelGGL(icamd_copy_subimage_kernel, dim3(copy_subimage_grid_x(cols), (uint32_t)ny, (uint32_t)nz),
                         dim3(kThreadsPerWorkgroup), 0, stream, P);
    });
  });
  return hipGetLastError();
}

}  // namespace icamd
