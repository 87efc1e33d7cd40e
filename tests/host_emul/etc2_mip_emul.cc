// TEST INFRASTRUCTURE ONLY.  The encode launch of icamd_encode_etc2_mips_device as its chain kernels run it
// (image-compression_amd/csrc/etc2_mip_kernels.hip), compiled for the HOST (g++ -DICAMD_HOST_EMULATION, like the other *_emul.cc
// files) so that the CPU tier checks it against the numpy route (tests/test_etc2_mips_host.py).  Never linked into libic_amd.so;
// the product has no CPU path.
//
// What is the product's own code here: the plan and its level table (etc2_mip_plan.h), etc2_mip_locate -- workgroup -> level and
// tile --, load_block's clamp-to-edge fetch and the block routines of the five codecs.  What is restated: the lane -> block
// arithmetic of locate_tile (ic_device.h, device-only) and the view of a level (etc2_mip_view).  A "wave" is one block, as in the
// other emulations: the encoders' wave votes change how a word is found, never which.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <cstring>

#include "etc1_block.h"
#include "etc2_block.h"
#include "etc2_colour_block.h"
#include "etc2_a1_block.h"
#include "etc2_th_block.h"
#include "eac11_block.h"
#include "metric_block.h"  // metric_gather_channel, the EAC kernels' clamp-to-edge gather
#include "etc2_mip_plan.h"
#include "emul_violations.h"

using namespace icamd;

namespace {

template <int ST>
Out8 etc1_word(const uint32_t px[16]) {
  if (ST == 3) return encode_etc1_block<false>(px, 3u);
  const uint32_t spread = etc1_block_spread(px);
  return etc1_encode_classified<ST>(px, etc1_constant_block(px, spread), spread >= ICAMD_ETC1_BUSY_SPREAD);
}

struct Level {  // etc2_mip_view: the GridParams of one level
  const uint8_t *src;
  uint8_t *dst;
  uint32_t h, w, stride, block_cols;
};

template <int COMPS, int ST>
void encode_block(int codec, int modes, int swap, const Level &V, uint32_t brow, uint32_t bcol) {
  const uint32_t bytes = codec_block_bytes(codec);
  uint8_t *o = V.dst + ((size_t)brow * V.block_cols + bcol) * bytes;
  if (codec == ICAMD_EAC_R11 || codec == ICAMD_EAC_RG11) {
    uint32_t r[4];
    metric_gather_channel<COMPS>(V.src, V.h, V.w, V.stride, brow * 4, bcol * 4, (swap && COMPS >= 3) ? 2u : 0u, r);
    const Out8 a = encode_eac11_rows(r);
    memcpy(o, &a, 8);
    if (codec == ICAMD_EAC_RG11) {
      metric_gather_channel<COMPS>(V.src, V.h, V.w, V.stride, brow * 4, bcol * 4, 1u, r);
      const Out8 b = encode_eac11_rows(r);
      memcpy(o + 8, &b, 8);
    }
    return;
  }
  if constexpr (COMPS >= 3) {
    uint32_t px[16];
    load_block<COMPS>(V.src, V.h, V.w, V.stride, brow * 4, bcol * 4, px);
    if (codec == ICAMD_ETC2_RGB8) {
      Out8 w = etc2_rgb8_choose(px, etc1_word<ST>(px)), th;  // the encode launch's word ...
      if (modes == 1 && etc2_th_choose(px, w, &th)) w = th;   // ... and what the T / H launch leaves in its place
      memcpy(o, &w, 8);
    } else if (codec == ICAMD_ETC2_RGBA8) {
      uint32_t a[16];
      for (int p = 0; p < 16; ++p) a[p] = px[p] >> 24;
      const Out8 c = etc1_word<ST>(px), e = encode_eac_alpha(a);
      memcpy(o, &e, 8);
      memcpy(o + 8, &c, 8);
    } else {
      Out8 c = { 0u, 0u };
      if (etc2_a1_opaque_mask(px) == 0xffffu) c = etc1_word<ST>(px);
      const Out8 w = etc2_a1_block<ST>(px, c);
      memcpy(o, &w, 8);
    }
  }
}

template <int COMPS, int ST>
void run(int codec, int modes, int swap, const Etc2MipPlan &plan, const uint8_t *src, const uint8_t *pyramid, uint8_t *out,
         uint32_t *hits) {
  size_t hit_base[kMipMaxLevels + 1] = { 0 };
  for (uint32_t k = 0; k < plan.table.n_levels; ++k)
    hit_base[k + 1] = hit_base[k] + (size_t)plan.table.level[k].block_rows * plan.table.level[k].block_cols;
  for (uint32_t wg = 0; wg < plan.grid_x; ++wg) {  // blockIdx.x
    const Etc2MipSpot spot = etc2_mip_locate(plan.table, wg);
    const Etc2MipLevel &L = plan.table.level[spot.entry];
    const Level V = { (L.level == 0u ? src : pyramid) + L.pix_offset, out + L.dst_offset, L.height, L.width, L.row_stride, L.block_cols };
    const uint32_t cols = 1u << L.log2_tile_cols, rows = 256u >> L.log2_tile_cols;
    for (uint32_t tid = 0; tid < 256u; ++tid) {  // threadIdx.x: locate_tile<false>
      const uint32_t bcol = spot.tile_col * cols + (tid & (cols - 1u)), brow = spot.tile_row * rows + (tid >> L.log2_tile_cols);
      if (!(bcol < L.block_cols && brow < L.block_rows)) continue;
      ++hits[hit_base[spot.entry] + (size_t)brow * L.block_cols + bcol];
      encode_block<COMPS, ST>(codec, modes, swap, V, brow, bcol);
    }
  }
}

template <int COMPS>
void run_strategy(int st, int codec, int modes, int swap, const Etc2MipPlan &plan, const uint8_t *src, const uint8_t *pyramid,
                  uint8_t *out, uint32_t *hits) {
  switch (st) {
    case 0: run<COMPS, 0>(codec, modes, swap, plan, src, pyramid, out, hits); break;
    case 1: run<COMPS, 1>(codec, modes, swap, plan, src, pyramid, out, hits); break;
    case 3: run<COMPS, 3>(codec, modes, swap, plan, src, pyramid, out, hits); break;
    default: run<COMPS, 2>(codec, modes, swap, plan, src, pyramid, out, hits); break;
  }
}

}  // namespace

// One image: `src` rows of row_stride bytes, `pyramid` levels 1 .. levels-1 as icamd_mip_pyramid_device writes them, `out` the
// chain (icamd_etc2_mip_chain_size bytes).  hits: one counter per block, levels in TABLE order, raster inside a level -- how
// often the launch encoded it.  order: 0 smallest level first, 1 largest first.  Returns the launch's grid.x, 0 if refused.
extern "C" uint32_t etc2mip_emul_encode(int codec, int strategy, int modes, int comps, int swap, int order, uint32_t h, uint32_t w,
                                        uint32_t row_stride, uint32_t levels, const uint8_t *src, const uint8_t *pyramid,
                                        uint8_t *out, uint32_t *hits) {
  const Etc2MipPlan plan = etc2_mip_plan({ codec, comps, 0, modes, h, w, levels, 1, row_stride, 0, 0, order });
  if (plan.form != kMipLaunch) return 0;
  const int st = (uint32_t)strategy < 4u ? strategy : 2;
  switch (comps) {
    case 1: run<1, 2>(codec, modes, swap, plan, src, pyramid, out, hits); break;
    case 2: run<2, 2>(codec, modes, swap, plan, src, pyramid, out, hits); break;
    case 3: run_strategy<3>(st, codec, modes, swap, plan, src, pyramid, out, hits); break;
    default: run_strategy<4>(st, codec, modes, swap, plan, src, pyramid, out, hits); break;
  }
  return plan.grid_x;
}
