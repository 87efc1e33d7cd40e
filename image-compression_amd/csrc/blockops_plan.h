// blockops_plan.h -- which kernels a Pad / Downsample call gets, with which grids, lanes and work items, and how the block copies,
// fills and the transcode are cut into launches.
//
// Host-only arithmetic on a handful of integers: no HIP header, no runtime call, no global, no environment.  blockops_kernels.hip
// asks pad_plan() / downsample_plan() once per call, fills BlockOpParams from the answer and launches what it says;
// tests/test_blockops_plan_host.py compiles this header with g++ and pins the answers over a grid of inputs
// (tests/golden/blockops_plan.txt).  Every limit of a launch is stated here, once.
#ifndef ICAMD_BLOCKOPS_PLAN_H_
#define ICAMD_BLOCKOPS_PLAN_H_

#include <cstddef>
#include <cstdint>

namespace icamd {

enum BlockOpCodec : int { kBlockOpDxt1 = 0, kBlockOpDxt5 = 1, kBlockOpEtc1 = 2 };  // = ICAMD_DXT1 / DXT5 / ETC1 (include/ic_amd.h)

constexpr uint32_t kBlockOpLanes = 256;                // lanes per workgroup: 4 waves, one block per lane
constexpr uint32_t kSearchLanes = 64;                  // ... of the kernels that run an ETC1 search per block
constexpr uint32_t kGridLimitYZ = 65535;               // workgroups in a grid's y and z
constexpr uint64_t kLaunchBlockLimit = 1ull << 31;     // a launch indexes its work items with 32 bits, fewer than 2^31 of them
// kSmallerError on grids of at most kDownsampleQuadMaxBlocks output blocks (r05): four lanes per output block.  A 512^2 level is
// 4 096 output blocks = 64 waves of ~3 000 dependent instructions on 64 of 1 024 SIMDs; the quad form makes it 256 waves of ~1 500.
constexpr uint32_t kDownsampleQuadMaxBlocks = 36864;
constexpr uint32_t kRowTileMinCols = kBlockOpLanes;    // row tiles where an output row fills a workgroup
constexpr uint64_t kTranscodeChunk = 1ull << 30;       // blocks per transcode launch (32-bit block index in the kernel)
// blocks per DXT5 -> ETC2 RGBA8 transcode launch: 16-byte blocks, 32-bit block index in the kernel, 2^24 one-wave workgroups
constexpr uint64_t kTranscode16Chunk = 1ull << 30;
constexpr uint32_t kFillBatch = 64;                    // images per batched fill launch (their blocks travel as kernel arguments)
constexpr uint32_t kFillWorkgroups = 256u * 64u;       // single fill: 8 waves on every SIMD several times over; the loop covers the rest
constexpr uint32_t kFillBatchWorkgroups = 256u * 32u;  // batched fill: ~8 waves on every SIMD over the whole launch

// The ETC1 re-encode strategy as the kernels are built for it: kSplitHorizontally 0, kSplitVertically 1 and kHeuristic 3 as they
// are, everything else kSmallerError 2, as the reference's default: label does.
constexpr uint32_t etc_strategy_kernel(uint32_t strategy) { return strategy == 0u || strategy == 1u || strategy == 3u ? strategy : 2u; }

// Whether a kernel runs an ETC1 codeword SEARCH per block (Downsample and the Pad border with kSplitHorizontally / kSplitVertically /
// kSmallerError): those are launched as one-wave workgroups like the encoders (r05, etc1_kernels.hip etc1_wave_workgroups: the
// search's cost depends on the content, and a four-wave workgroup holds its slots until its slowest wave is done); everything else
// keeps 256 lanes.  copies_only: the kernel writes no re-encoded block (the Pad copy).
constexpr bool runs_etc1_search(int codec, uint32_t strategy, bool copies_only) {
  return codec == kBlockOpEtc1 && strategy != 3u && !copies_only;
}
constexpr uint32_t blockop_lanes(int codec, uint32_t strategy, bool copies_only) {
  return runs_etc1_search(codec, strategy, copies_only) ? kSearchLanes : kBlockOpLanes;
}

// blockops_kernels.hip maps these to its kernels; the ETC1 ones follow the strategy: kPadEtc1Border0 + strategy, kDownEtc1_0 + strategy
enum BlockOpKernel : int {
  kNoKernel = -1,
  kPadDxt1, kPadDxt5, kPadEtc1Copy, kPadEtc1Border0, kPadEtc1Border1, kPadEtc1Border2, kPadEtc1Border3, kPadEtc1Quad,
  kDownDxt1, kDownDxt5, kDownEtc1_0, kDownEtc1_1, kDownEtc1_2, kDownEtc1_3, kDownDxt1Rows, kDownDxt5Rows, kDownEtc1HeuristicRows,
  kDownEtc1Quad,
  kBlockOpKernels
};

enum BlockOpForm : int {
  kBlockOpRefused = 0,  // one image of 2^31 blocks or more
  kBlockOpNothing,      // no image, or an empty grid: no launch
  kPadOnePass,          // DXT: one launch over the output grid
  kPadCopyAndBorder,    // ETC1: the copy over the grid, then (where there is a border) the pad blocks, one lane each
  kPadQuad,             // ETC1 kSmallerError: ONE launch, first the pad blocks' workgroups (four lanes per block), then the copy's
  kDownLinear,          // one work item per output block, (image, row, column) by division
  kDownRows,            // blockIdx = (column tile, output row, image)
  kDownQuad             // ETC1 kSmallerError on small grids: linear, four lanes per output block
};

struct BlockOpIn {
  int codec;
  uint32_t etc_strategy;         // as the caller passed it
  uint32_t in_rows, in_cols;     // source block grid
  uint32_t out_rows, out_cols;   // result block grid
  uint32_t src_height, src_width;  // Downsample: uncompressed pixels of the source (its single-block case)
  uint32_t n_images;
  bool quad;                     // the four-lanes-per-block forms are allowed (ICAMD_PAD_BORDER_QUAD)
};

// One launch: `items` work items (what the kernel compares its index with), items_per_image of them per image,
// lanes_per_item lanes each
struct BlockOpLaunch {
  int kernel;
  uint32_t grid_x, grid_y, grid_z, lanes;
  uint32_t items, items_per_image, lanes_per_item;
};
// The launches of `count` images
struct BlockOpGroup {
  uint32_t count;
  int form;
  uint32_t total_out;  // output blocks
  BlockOpLaunch launch[2];
  // kPadQuad: the first border_wgs workgroups are the pad blocks' quad lanes, border_lanes of them
  uint32_t border_lanes, border_wgs;
};
struct BlockOpPlan {
  int form;           // of the full groups (a shorter last group may take another: see BlockOpGroup::form); kBlockOpRefused
  uint32_t strategy;  // etc_strategy_kernel()
  uint32_t out_per_image;
  uint64_t border;                  // Pad: pad blocks per image, right of the image and below it
  uint32_t border_lanes_per_image;  // kPadQuad
  uint64_t group;                   // images per launch group: as many as the 2^31 limit allows
  BlockOpGroup full, tail;          // groups of `group` images, and the last one where n_images is no multiple (count 0: none)
};

inline bool blockop_image_fits(uint32_t out_rows, uint32_t out_cols) { return (uint64_t)out_rows * out_cols < kLaunchBlockLimit; }

// the frame both plans share: the refusal, the group size, and the groups as group_plan(count) shapes them
template <typename GroupPlan>
inline void blockop_groups(BlockOpPlan &p, const BlockOpIn &in, GroupPlan group_plan) {
  const uint64_t per = (uint64_t)in.out_rows * in.out_cols;
  p.strategy = etc_strategy_kernel(in.etc_strategy);
  if (!blockop_image_fits(in.out_rows, in.out_cols)) return;
  p.form = kBlockOpNothing;
  if (per == 0 || in.n_images == 0) return;
  p.out_per_image = (uint32_t)per;
  p.group = (kLaunchBlockLimit - 1) / per;
  if (p.group < 1) p.group = 1;
  if (p.group > in.n_images) p.group = in.n_images;
  p.full = group_plan((uint32_t)p.group);
  if (in.n_images % p.group) p.tail = group_plan((uint32_t)(in.n_images % p.group));
  p.form = p.full.form;
}

// the work items of one linear launch: `lanes` per workgroup, lanes_per_item of them per item
inline BlockOpLaunch linear_launch(int kernel, uint32_t lanes, uint32_t items, uint32_t items_per_image, uint32_t lanes_per_item = 1) {
  return { kernel, (items * lanes_per_item + lanes - 1) / lanes, 1, 1, lanes, items, items_per_image, lanes_per_item };
}
inline BlockOpGroup blockop_group(const BlockOpPlan &p, uint32_t count) {
  BlockOpGroup g = {};
  g.count = count;
  g.total_out = p.out_per_image * count;
  g.launch[1].kernel = kNoKernel;
  return g;
}

inline BlockOpPlan pad_plan(const BlockOpIn &in) {
  BlockOpPlan p = {};
  p.border = (uint64_t)in.in_rows * (in.out_cols - in.in_cols) + (uint64_t)(in.out_rows - in.in_rows) * in.out_cols;
  p.border_lanes_per_image = p.border * 4u < kLaunchBlockLimit ? (uint32_t)p.border * 4u : 0u;  // (more: no group takes kPadQuad)
  blockop_groups(p, in, [&](uint32_t count) {
    BlockOpGroup g = blockop_group(p, count);
    BlockOpLaunch &l = g.launch[0];
    l = linear_launch(kNoKernel, kBlockOpLanes, g.total_out, p.out_per_image);  // every form starts with one lane per output block
    if (in.codec != kBlockOpEtc1) {
      g.form = kPadOnePass;
      l.kernel = kPadDxt1 + in.codec;
    } else if (p.border && p.strategy == 2u && in.quad && p.border * 4u * count < kLaunchBlockLimit) {
      g.form = kPadQuad;
      g.border_lanes = p.border_lanes_per_image * count;
      g.border_wgs = (g.border_lanes + kBlockOpLanes - 1) / kBlockOpLanes;
      l.kernel = kPadEtc1Quad;
      l.grid_x += g.border_wgs;
    } else {
      g.form = kPadCopyAndBorder;
      l.kernel = kPadEtc1Copy;
      if (p.border)  // the pad blocks only: right of the image, then below it
        g.launch[1] = linear_launch(kPadEtc1Border0 + (int)p.strategy, blockop_lanes(kBlockOpEtc1, p.strategy, false),
                                    (uint32_t)(p.border * count), (uint32_t)p.border);
    }
    return g;
  });
  return p;
}

inline BlockOpPlan downsample_plan(const BlockOpIn &in) {
  BlockOpPlan p = {};
  blockop_groups(p, in, [&](uint32_t count) {
    BlockOpGroup g = blockop_group(p, count);
    const bool etc1 = in.codec == kBlockOpEtc1;
    // row tiles where a row fills a workgroup (small grids keep the linear launch); of the ETC1 kernels, kHeuristic has the form
    const bool rows = in.in_rows > 1 && in.in_cols > 1 && in.out_cols >= kRowTileMinCols && in.out_rows <= kGridLimitYZ &&
                      count <= kGridLimitYZ && (!etc1 || p.strategy == 3u);
    if (rows) {
      g.form = kDownRows;
      g.launch[0] = { etc1 ? kDownEtc1HeuristicRows : kDownDxt1Rows + in.codec, (in.out_cols + kBlockOpLanes - 1) / kBlockOpLanes,
                      in.out_rows, count, kBlockOpLanes, g.total_out, p.out_per_image, 1 };
    } else if (etc1 && p.strategy == 2u && in.quad && g.total_out <= kDownsampleQuadMaxBlocks) {
      g.form = kDownQuad;
      g.launch[0] = linear_launch(kDownEtc1Quad, kSearchLanes, g.total_out, p.out_per_image, 4);
    } else {
      g.form = kDownLinear;
      g.launch[0] = linear_launch(etc1 ? kDownEtc1_0 + (int)p.strategy : kDownDxt1 + in.codec,
                                  blockop_lanes(in.codec, p.strategy, false), g.total_out, p.out_per_image);
    }
    return g;
  });
  return p;
}

// ---- launches that are cut into chunks: launch(first, count) for every [first, first + count) of `total`, at most `limit` at a time
template <typename Launch>
inline void for_chunks(uint64_t total, uint64_t limit, Launch launch) {
  for (uint64_t first = 0; first < total; first += limit) launch(first, total - first < limit ? total - first : limit);
}

// The in-place transcodes of the ETC2 family (DXT1 -> ETC2 RGB8, BC4 -> EAC R11, BC5 -> EAC RG11; transcode_family_block.h): a
// buffer of n_bytes holds n_bytes / block_bytes whole blocks, the rest is left alone; a launch takes at most kTranscodeFamilyChunk
// blocks, which its kernel indexes with 32 bits, one block per lane in workgroups of `lanes`.  Launch i of transcode_launches().
constexpr uint64_t kTranscodeFamilyChunk = 1ull << 30;
struct TranscodeLaunch {
  uint64_t first_block, byte_offset;  // where the launch starts in the buffer
  uint32_t blocks, grid_x, lanes;
};
inline uint64_t transcode_blocks(uint64_t n_bytes, uint32_t block_bytes) { return n_bytes / block_bytes; }
inline uint64_t transcode_launches(uint64_t n_blocks) { return (n_blocks + kTranscodeFamilyChunk - 1) / kTranscodeFamilyChunk; }
inline TranscodeLaunch transcode_launch(uint64_t n_blocks, uint32_t block_bytes, uint32_t lanes, uint64_t i) {
  const uint64_t first = i * kTranscodeFamilyChunk, left = n_blocks - first;
  const uint32_t blocks = (uint32_t)(left < kTranscodeFamilyChunk ? left : kTranscodeFamilyChunk);
  return { first, first * block_bytes, blocks, (blocks + lanes - 1) / lanes, lanes };
}

// CopySubimage: grid = (column chunks of a block row, rows, images), rows and images in chunks of kGridLimitYZ
inline uint32_t copy_subimage_grid_x(uint32_t cols) { return (cols + kBlockOpLanes - 1) / kBlockOpLanes; }
// CreateSolid, one image: a grid-stride loop of at most kFillWorkgroups workgroups
inline uint32_t fill_workgroups(uint64_t n_blocks) {
  const uint64_t wgs = (n_blocks + kBlockOpLanes - 1) / kBlockOpLanes;
  return (uint32_t)(wgs < kFillWorkgroups ? wgs : kFillWorkgroups);
}
// CreateSolid, a launch of n <= kFillBatch images: grid = (workgroups per image, n), each image a grid-stride loop
inline uint32_t fill_batch_workgroups(uint32_t blocks_per_image, uint32_t n) {
  const uint64_t wgs = ((uint64_t)blocks_per_image + kBlockOpLanes - 1) / kBlockOpLanes;
  const uint32_t per_image = (kFillBatchWorkgroups + n - 1) / n;
  return wgs < per_image ? (uint32_t)wgs : per_image;
}

}  // namespace icamd

#endif  // ICAMD_BLOCKOPS_PLAN_H_
