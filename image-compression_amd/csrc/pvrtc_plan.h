// pvrtc_plan.h -- which kernels a PVRTC call gets, and with which grid, LDS size, strip and rectangle.
//
// Host-only arithmetic on a handful of integers: no HIP header, no runtime call, no global, no environment.  pvrtc_kernels.hip asks
// pvrtc_plan() once per call and launches what it answers; tests/test_pvrtc_plan_host.py compiles this header with g++ and pins the
// answers over a grid of inputs (tests/golden/pvrtc_plan.txt).  The sizes the kernels and the plan share (lanes per workgroup,
// LDS per wave) are defined here, and so is compact_even_bits, which the 4 bpp kernels use on the device.
#ifndef ICAMD_PVRTC_PLAN_H_
#define ICAMD_PVRTC_PLAN_H_

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ICAMD_PLAN_HD __host__ __device__ __forceinline__
#else
#define ICAMD_PLAN_HD inline
#endif

namespace icamd {

constexpr int kMorphLanes = 256;
constexpr int kEncodeLanes = 256;
constexpr uint32_t kFullChipLanes = 256u * 4u * 64u * 2u;  // two waves on each of the 1 024 SIMDs
constexpr int kMorphBlocksPerLane = 4;                     // pair, morph kernel (pvrtc_kernels.hip)

// LDS of the one-pass kernels (layout: pvrtc_kernels.hip, at the kernels)
constexpr uint32_t kOnePassRing = 8;
constexpr uint32_t kOnePassChunkSlots = 18;                                  // 4 x 4 blocks in Z order + 2 (16-byte aligned stride)
constexpr uint32_t kOnePassWaveDwords = kOnePassRing * 512u + 16u * kOnePassChunkSlots * 2u;  // ring + tile: 18 688 bytes
constexpr uint32_t kOnePassXchDwords = 8;                                    // per wave and parity: [lo.a lo.b col0 - | hi.a hi.b - -]
constexpr uint32_t kOnePassHaloTableBytes = (64u + 4u) * 8u + (64u + 3u) * 16u + (64u + 3u) * 8u;  // strips of at most 64 blocks
constexpr uint32_t kOnePass4WaveDwords = kOnePassRing * 256u + 256u;  // ring + tile: 9 216 bytes
constexpr uint32_t kOnePass4XchDwords = 4;                            // per wave and parity: lo.a lo.b hi.a hi.b

// inverse of pvrtc_z_index: x from the odd bits (v >> 1), y from the even bits
ICAMD_PLAN_HD uint32_t compact_even_bits(uint32_t v) {
  v &= 0x55555555u;
  v = (v | v >> 1) & 0x33333333u;
  v = (v | v >> 2) & 0x0f0f0f0fu;
  v = (v | v >> 4) & 0x00ff00ffu;
  v = (v | v >> 8) & 0x0000ffffu;
  return v;
}

// images of one launch pair: as many as 4 GiB of pixels (and the 32-bit block index) allow
inline uint64_t pvrtc_group(uint32_t size, uint32_t n_images) {
  const uint64_t image_bytes = (uint64_t)size * size * 4u;
  uint64_t group = image_bytes ? (4096ull << 20) / image_bytes : 1;
  if (group < 1) group = 1;
  if (group > n_images) group = n_images;
  return group;
}
// scratch of the pair between its two kernels: 8 bytes (the two reduced colours) per block of one launch group
inline size_t pvrtc_workspace_bytes(uint32_t bpp, uint32_t size, uint32_t n_images) {
  if (n_images == 0) return 0;
  return (size_t)((uint64_t)(size / (bpp == 4 ? 4 : 8)) * (size / 4) * pvrtc_group(size, n_images) * 8u);
}

enum PvrtcPath : int { kPvrtcRefused = 0, kPvrtcOnePass = 1, kPvrtcOnePassHalo = 2, kPvrtcPair = 3 };
enum PvrtcMorph : int { kPvrtcMorphSmall = 0, kPvrtcMorphDense = 1, kPvrtcMorphPlain = 2, kPvrtcMorphRect = 3 };
enum PvrtcEncode : int { kPvrtcEncodeWide = 0, kPvrtcEncodeNarrow = 1 };

struct PvrtcPlanIn {
  uint32_t bpp;                          // 2 or 4
  uint32_t log2_size, n_images;          // n_images >= 1 square textures of 2^log2_size pixels, log2_size >= 3
  uint32_t region_first, region_blocks;  // region_blocks != 0: that Z-order range of ONE image (2 bpp only)
  int mode, strip;                       // icamd_pvrtc2_tune: 0 auto, 1 always the pair, 2 one pass wherever eligible; strip < 0: auto
  uint32_t compute_units;
  bool dst_aligned16;                    // every image's output is 16-byte aligned
};

// One launch of the pair: `count` images
struct PvrtcPairChunk {
  uint64_t count;
  uint32_t total_blocks, total_strips;
  int morph;
  uint32_t morph_grid_x, morph_grid_y, encode_grid;
};

struct PvrtcPlan {
  int path;
  // the encoded rectangle of each image, in blocks (whole texture: 0, 0, log2_bw, log2_bh, 0) -- 2 bpp
  uint32_t rx0, ry0, log2_rw, log2_rh, z_first;
  uint32_t log2_strip;    // one-pass: block rows per workgroup; pair: blocks per lane of the encode kernel
  uint32_t stage_stores;  // finished blocks leave through LDS as 16-byte stores
  // one-pass forms
  uint32_t log2_wgc;      // halo form: block columns per workgroup (plain form: 0, the kernel does not read it)
  uint32_t lanes, workgroups;
  size_t lds_bytes;         // dynamic LDS of this launch
  size_t lds_opt_in_bytes;  // ... and of the kernel's widest workgroup: what the once-per-device opt-in asks for
  // pair
  uint64_t group;           // images per launch pair
  size_t workspace_bytes;
  int encode;
  PvrtcPairChunk full, tail;  // launches of `group` images, and the last one where n_images is no multiple (count 0: none)
};

// Strip height of a one-pass launch (log2 of the block rows a workgroup walks), or -1 where the morph + encode pair is the better
// choice.  Time model, fitted on an MI355X (profiles/r05_ab_pvrtc_onepass.log, within 5 % of every measured shape from 1 x 512^2 to
// 16 x 4096^2; 4 bpp: profiles/r05_ab_pvrtc4_onepass.log): a workgroup of K-block strips takes 11 + 5.8 K us on a full CU whatever
// its width (its waves walk K + 2 block rows; 4 bpp: the same pixels per CU and block row), a CU holds cu_waves / waves-per-workgroup
// of them, a launch takes prologue_us + ceil(workgroups / slots) such rounds; the pair takes 10 us + pair_us_per_unit x units.
// Mode 2: the best strip height, no comparison; mode 2 with a strip: that strip height, clamped.
struct StripModel {
  uint32_t log2_lanes, max_log2_lanes;  // lanes per workgroup (at least one wave), and the kernel's widest workgroup
  uint32_t log2_rows, min_log2_rows;    // block rows of each image's rectangle, and the fewest the form takes
  uint64_t wgs_per_row;                 // workgroups side by side on one block row
  uint32_t cu_waves;                    // waves a CU holds: 8 (2 bpp: 2 per SIMD) or 16 (4 bpp)
  double prologue_us;                   // halo form: 2 us for the table
  double pair_us_per_unit;              // the pair's cost line: 52.6e-6 per block (2 bpp) or 1.87e-6 per pixel (4 bpp) ...
  uint64_t units;                       // ... and the blocks / pixels of this launch
  uint64_t min_units;  // 4 bpp, 8 Mi pixels: below, neither fills the chip and the pair is as fast or faster (1 x 2048^2: 15 vs 21 us)
  int forced_min, forced_max;           // a forced strip is clamped to these
};
inline int onepass_log2_strip(const StripModel &M, const PvrtcPlanIn &in) {
  const bool always = in.mode == 2;
  const int forced = always ? in.strip : -1;  // (a strip height only counts together with mode 2)
  const uint64_t n_images = in.n_images;
  if (M.log2_lanes < 6u || M.log2_lanes > M.max_log2_lanes || M.log2_rows < M.min_log2_rows) return -1;
  if (forced >= 0) return forced < M.forced_min ? M.forced_min : (forced > M.forced_max ? M.forced_max : forced);
  if (!always && M.units < M.min_units) return -1;  // (a forced strip is not held to the floor, mode 2 alone is not either)
  const uint64_t slots = (uint64_t)in.compute_units * (M.cu_waves >> (M.log2_lanes - 6u));
  int best = -1;
  double best_us = 0.0;
  for (int sb = 2; sb <= 6 && sb <= (int)M.log2_rows; ++sb) {
    const uint64_t wgs = (n_images << (M.log2_rows - (uint32_t)sb)) * M.wgs_per_row;
    const double us = M.prologue_us + (double)((wgs + slots - 1) / slots) * (11.0 + 5.8 * (double)(1u << sb));
    if (best < 0 || us <= best_us) { best_us = us; best = sb; }
  }
  const double pair_us = 10.0 + M.pair_us_per_unit * (double)M.units;
  return always || best_us < 0.97 * pair_us ? best : -1;
}

// Shape of a one-pass launch: strips of 2^sb block rows, workgroups of 2^log2_lanes lanes, 2^log2_wgs of them per image (the caller
// has checked blocks per image x images < 2^31, so the grid fits); LDS per wave and behind the waves, the widest workgroup's waves
inline void onepass_shape(PvrtcPlan &p, const PvrtcPlanIn &in, int sb, uint32_t log2_lanes, uint32_t log2_wgs, size_t wave_bytes,
                          size_t table_bytes, uint32_t max_waves) {
  p.log2_strip = (uint32_t)sb;
  p.lanes = 1u << log2_lanes;
  p.workgroups = (uint32_t)((uint64_t)in.n_images << log2_wgs);
  p.lds_bytes = (p.lanes >> 6) * wave_bytes + table_bytes;
  p.lds_opt_in_bytes = max_waves * wave_bytes + table_bytes;
  // the tile's write-out issues 16-byte stores: only when every image's output is 16-byte aligned (the contract asks for 8)
  p.stage_stores = in.dst_aligned16 ? 1u : 0u;
}

// The 2 bpp one-pass forms on the plan's rectangle: true and the launch where the model prefers the form.  The plain form is the halo
// form with one workgroup per block row of a whole texture, no prologue and no table behind the exchange slots; it does not read
// log2_wgc, and it differs in one more thing, the clamp of a forced strip.
inline bool onepass2(PvrtcPlan &p, const PvrtcPlanIn &in, bool halo) {
  const uint32_t log2_wgc = p.log2_rw < 9u ? p.log2_rw : 9u;
  StripModel M = {};
  M.log2_lanes = halo ? log2_wgc : p.log2_rw;  // plain: a workgroup is one block row wide, 64 ... 512 lanes
  M.max_log2_lanes = 9; M.cu_waves = 8;
  M.log2_rows = p.log2_rh; M.min_log2_rows = 2;  // one 4-block strip (a whole texture that is a wave wide is taller anyway)
  M.wgs_per_row = 1ull << (p.log2_rw - log2_wgc);
  M.prologue_us = halo ? 2.0 : 0.0;
  M.pair_us_per_unit = 52.6e-6; M.units = (uint64_t)in.n_images << (p.log2_rw + p.log2_rh);
  // plain: a forced strip may be as tall as the texture, one workgroup per texture (tests and A/B runs use it);
  // halo: 64 block rows at the most, the table's size
  M.forced_min = 2; M.forced_max = halo && p.log2_rh > 6u ? 6 : (int)p.log2_rh;
  const int sb = onepass_log2_strip(M, in);
  if (sb < 0) return false;
  p.path = halo ? kPvrtcOnePassHalo : kPvrtcOnePass;
  p.log2_wgc = halo ? log2_wgc : 0u;
  onepass_shape(p, in, sb, log2_wgc, p.log2_rh - (uint32_t)sb + p.log2_rw - log2_wgc, (kOnePassWaveDwords + 2u * kOnePassXchDwords) * 4u,
                halo ? kOnePassHaloTableBytes : 0u, 8);
  return true;
}

// The encode kernel of the 2 bpp pair: strip height for `blocks` encoded blocks in one launch, the kernel, the staged stores
inline void pair2_encode(PvrtcPlan &p, const PvrtcPlanIn &in, uint64_t blocks) {
  // strip height: 8 blocks (32 pixel rows) amortise the one halo row per strip to 1/32 of the modulation work
  // while a 4096^2 image still yields 1 024 waves; never more than the rectangle's block rows
  p.log2_strip = p.log2_rh < 3u ? p.log2_rh : 3u;
  // ... and never so tall that a small launch leaves the chip empty: a strip is one long dependent instruction
  // stream (~1 200 per block), so below ~2 waves per SIMD of strips, shorter strips finish sooner
  // (one 1024^2 texture: 40 us with 8-block strips, a quarter of that with 1-block strips)
  // (kFullChipLanes is a 256-CU chip's whatever compute_units says)
  while (p.log2_strip > 0 && (blocks >> p.log2_strip) < kFullChipLanes) --p.log2_strip;
  // the staged write-out issues 16-byte stores: taken only when every image's output is 16-byte aligned (the
  // contract asks for 8); otherwise each block is stored on its own, 8 bytes at its Z-order slot
  p.stage_stores = (p.log2_strip >= 1 && p.log2_rw >= p.log2_strip && in.dst_aligned16) ? 1u : 0u;
  p.encode = p.log2_rw >= 6 ? kPvrtcEncodeWide : kPvrtcEncodeNarrow;
}

inline PvrtcPlan pvrtc_plan(const PvrtcPlanIn &in) {
  PvrtcPlan p = {};  // (path: kPvrtcRefused)
  const bool four = in.bpp == 4;  // 4 x 4-pixel blocks, 8 x 4 otherwise
  const uint32_t size = 1u << in.log2_size, log2_bw = in.log2_size - (four ? 2u : 3u), log2_bh = in.log2_size - 2u;
  const uint32_t log2_bpi = log2_bw + log2_bh;
  const uint64_t bpi = 1ull << log2_bpi;
  const bool onepass_fits = in.mode != 1 && bpi * in.n_images < (1ull << 31);  // (one grid, 32-bit)

  if (in.region_blocks != 0) {
    // One image, blocks [region_first, region_first + region_blocks) of its Z-order output (a power of two of them, the first a
    // multiple of it: a rectangle of the block grid); 4 bpp has no regions
    if (four || in.n_images != 1) return p;
    uint32_t m = 0;
    while (m < 32u && (1ull << m) < in.region_blocks) ++m;
    if ((1ull << m) != in.region_blocks || m > log2_bpi || (in.region_first & (in.region_blocks - 1u)) != 0 ||
        (uint64_t)in.region_first + in.region_blocks > bpi)
      return p;
    p.log2_rw = m / 2;  // x owns the odd bits of the Z index: floor(m/2) of the low m bits
    p.log2_rh = m - p.log2_rw;
    p.rx0 = compact_even_bits(in.region_first >> 1); p.ry0 = compact_even_bits(in.region_first);
    p.z_first = in.region_first;
    // r06: regions at least one wave wide and one 4-block strip tall take the one-pass kernel's halo form where the time model
    // prefers it (one read of the pixels, one launch, no scratch) -- the multi-GPU split of ONE large texture (sharding.pvrtc_region)
    // no longer pays the pair's second pass over the pixels; icamd_pvrtc2_tune(1, ...) keeps the pair for A/B runs and tests
    if (in.mode != 1 && onepass2(p, in, true)) return p;
    // the pair reads the region's pixels and a one-block ring around it only; its workspace is indexed like a whole image's
    p.path = kPvrtcPair;
    p.group = 1;
    p.workspace_bytes = (size_t)8u << log2_bpi;
    pair2_encode(p, in, in.region_blocks);
    PvrtcPairChunk &c = p.full;
    c.count = 1;
    c.total_blocks = 1u << log2_bpi;
    c.total_strips = in.region_blocks >> p.log2_strip;
    c.morph = kPvrtcMorphRect;  // one lane per block of the rectangle and of the ring around it
    c.morph_grid_x = ((1u << p.log2_rw) + 2 + kMorphLanes - 1) / kMorphLanes;
    c.morph_grid_y = (1u << p.log2_rh) + 2;
    c.encode_grid = (c.total_strips + kEncodeLanes - 1) / kEncodeLanes;
    return p;
  }

  if (four && onepass_fits) {
    StripModel M = {};
    M.log2_lanes = M.log2_rows = log2_bw;  // a workgroup is one whole block row of the texture wide: size / 4 lanes
    M.max_log2_lanes = 10; M.wgs_per_row = 1; M.cu_waves = 16;
    M.pair_us_per_unit = 1.87e-6; M.units = (uint64_t)in.n_images << (2u * in.log2_size); M.min_units = 8ull << 20;
    M.forced_min = 1; M.forced_max = (int)log2_bw;  // (the 2 bpp forms: from 2)
    const int sb = onepass_log2_strip(M, in);
    if (sb >= 0) {
      p.path = kPvrtcOnePass;
      onepass_shape(p, in, sb, log2_bw, log2_bw - (uint32_t)sb, (kOnePass4WaveDwords + 2u * kOnePass4XchDwords) * 4u, 0, 16);
      return p;
    }
  }
  if (!four) {
    p.log2_rw = log2_bw; p.log2_rh = log2_bh;
    // whole textures of 512^2 ... 4096^2: the plain form; of 8192^2 and more (r06), whose block row is two or more workgroups wide:
    // the halo form
    if (onepass_fits && (onepass2(p, in, false) || (log2_bw > 9u && onepass2(p, in, true)))) return p;
  }

  // The pair.  Images per launch: every launch boundary costs a drain/fill of ~4 waves per SIMD: measured 0.67 / 0.60 /
  // 0.58 / 0.57 ms per 16 x 4096^2 for groups of 64 MiB / 128 MiB / 512 MiB / 1 GiB of pixels (r01).  So: as many
  // images per launch as the 32-bit block index and a 256 MiB workspace allow.  (r02: hosting the encode workgroups
  // of one image group and the morph workgroups of the next in ONE grid, 1 : 2 interleaved -- the encode role is
  // VALU-bound, the morph role memory-bound -- was measured at 0.55 / 0.59 / 0.68 ms for 2 / 4 / 8 stages against
  // 0.53 ms for the two plain kernels: the shared 167-VGPR allocation and the extra fill/drain phases cost more than
  // the overlap gains.  Removed.)
  p.group = pvrtc_group(size, in.n_images);
  if (bpi * p.group >= (1ull << 31)) { p.group = 0; return p; }
  p.path = kPvrtcPair;
  p.workspace_bytes = pvrtc_workspace_bytes(in.bpp, size, in.n_images);
  if (!four) pair2_encode(p, in, bpi * p.group);  // (4 bpp: one encode kernel, one block per lane, no staged stores)
  auto chunk = [&](uint64_t count) {
    PvrtcPairChunk c = {};
    c.count = count;
    c.total_blocks = (uint32_t)(bpi * count);
    c.total_strips = c.total_blocks >> p.log2_strip;
    // 2 bpp: one block per lane up to AND INCLUDING two waves per SIMD of four-block lanes -- one 4096^2 texture is exactly that:
    // morph 17.0 -> 14.7 us per call (r03, rocprofv3; the memory-bound kernel wants the extra waves in flight)
    const bool small = !four && c.total_blocks <= (uint32_t)kMorphBlocksPerLane * kFullChipLanes;
    const uint32_t per_wg = kMorphLanes * (four || small ? 1 : kMorphBlocksPerLane);  // (4 bpp: one morph kernel, one block per lane)
    c.morph = small ? kPvrtcMorphSmall : !four && log2_bw >= 6 ? kPvrtcMorphDense : kPvrtcMorphPlain;
    c.morph_grid_x = (c.total_blocks + per_wg - 1) / per_wg; c.morph_grid_y = 1;
    c.encode_grid = (c.total_strips + kEncodeLanes - 1) / kEncodeLanes;
    return c;
  };
  p.full = chunk(p.group);
  if (in.n_images % p.group) p.tail = chunk(in.n_images % p.group);
  return p;
}

}  // namespace icamd

#endif  // ICAMD_PVRTC_PLAN_H_
