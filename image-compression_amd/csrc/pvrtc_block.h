// pvrtc_block.h -- PVRTC1 2bpp (8x4-pixel blocks) per-block and per-pixel math.
//
// Bit-exact with internal/pvrtc_compressor.cc (Morph :506-521, Modulate :527-540, Encode :551-580),
// restructured so that a lane owns whole 8x4 blocks with their pixels in VGPRs:
//  * GetExtremesFast (:255-329): the 5 fitness axes' "first minimum / first maximum" become unsigned
//    min / max reductions over keys value*256 + idx  /  value*256 + (31-idx), each key (pair) built by one v_perm_b32:
//    lightness is a v_dot4_u32_u8 with 32-bit keys, the R,B and G,A channels are two 16-bit keys per dword reduced
//    with v_pk_min/max_u16;
//  * ColorDiff (:74-77), an L1 distance over 4 bytes, is one v_sad_u8;
//  * ApplyColorChannelReduction (:337-349) is SWAR on the RGBA dword;
//  * the bilinear up-sampling (:173-237) is separable and incremental on 16-bit channel pairs 0x00RR00BB /
//    0x00GG00AA carried at scale 256 (max 65 280 per lane: no carry between lanes), so the truncated 8-bit
//    channels are the lanes' high bytes; the 5:3 / 3:5 blends (:111-135) are nested v_lerp_u8 byte averages;
//  * pvrtc_encode_strip: one lane walks a vertical strip of blocks, so the row below a block is computed once.
#ifndef ICAMD_PVRTC_BLOCK_H_
#define ICAMD_PVRTC_BLOCK_H_

// The math lives in five headers, included here in the order they build on each other; this file adds the Z-order index and,
// for tests/host_emul, the host drivers over all of them.
#include "pvrtc_pixel.h"    // colour reduction, whole-block extremes, per-pixel modulation, one row's values
#include "pvrtc_walk.h"   // the row walk on 64-bit register pairs
#include "pvrtc_pair.h"     // pair path: block rows, strip form
#include "pvrtc_onepass.h"  // one-pass strip (morph + modulation)
#include "pvrtc4_block.h"   // 4 bpp extension
#if defined(ICAMD_HOST_EMULATION)
#include <string.h>
#endif

namespace icamd {

// FromZOrder inverse (pvrtc.cc:80-86): x occupies the odd bits, y the even bits of the block index.
ICAMD_DEV uint32_t spread_bits16(uint32_t v) {
  v = (v | v << 8) & 0x00ff00ffu;
  v = (v | v << 4) & 0x0f0f0f0fu;
  v = (v | v << 2) & 0x33333333u;
  v = (v | v << 1) & 0x55555555u;
  return v;
}
ICAMD_DEV uint32_t pvrtc_z_index(uint32_t bx, uint32_t by) { return spread_bits16(bx) << 1 | spread_bits16(by); }

#if defined(ICAMD_HOST_EMULATION)
static inline uint32_t spread_bits16_host(uint32_t v) {
  v = (v | v << 8) & 0x00ff00ffu; v = (v | v << 4) & 0x0f0f0f0fu; v = (v | v << 2) & 0x33333333u; v = (v | v << 1) & 0x55555555u;
  return v;
}
// PVRTC 4 bpp (extension): the device math above over a whole image (tests/host_emul only).
static inline int emul_pvrtc4(const uint8_t *src, uint32_t n, uint8_t *out) {
  const uint32_t lw = n / 4;
  const uint32_t *img = reinterpret_cast<const uint32_t *>(src);
  PvrtcColors *col = new PvrtcColors[(size_t)lw * lw];
  for (uint32_t by = 0; by < lw; ++by)
    for (uint32_t bx = 0; bx < lw; ++bx) {
      uint32_t px[16], a, b;
      for (int i = 0; i < 16; ++i) px[i] = img[(size_t)(by * 4 + i / 4) * n + bx * 4 + i % 4];
      BlockStash st;
      pvrtc4_extremes(px, img[0], st, a, b);
      col[by * lw + bx].a = channel_reduce(a, false);
      col[by * lw + bx].b = channel_reduce(b, true);
    }
  for (uint32_t by = 0; by < lw; ++by)
    for (uint32_t bx = 0; bx < lw; ++bx) {
      uint32_t px[16];
      for (int i = 0; i < 16; ++i) px[i] = img[(size_t)(by * 4 + i / 4) * n + bx * 4 + i % 4];
      PvrtcColors nb[3][3];
      for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) nb[dy][dx] = col[((by + lw + dy - 1) % lw) * lw + (bx + lw + dx - 1) % lw];
      uint32_t *o = reinterpret_cast<uint32_t *>(out) + 2 * (size_t)(spread_bits16_host(bx) << 1 | spread_bits16_host(by));
      o[0] = pvrtc4_block_data(px, nb);
      o[1] = pvrtc_pack_colors(nb[1][1].a, nb[1][1].b, true);  // bit 0 clear: standard modulation
    }
  // the one-pass walker (what icamd_pvrtc4_onepass_kernel runs) must reproduce every block for several strip heights
  int ok = 1;
  for (uint32_t k_blocks = 1; k_blocks <= 8 && k_blocks <= lw; k_blocks *= 2)
    for (uint32_t by0 = 0; by0 < lw; by0 += k_blocks)
      for (uint32_t bx = 0; bx < lw; ++bx) {
        int last_m = -100;
        auto tick = [&](int m, uint32_t *mp, uint32_t *ep) {
          last_m = m;
          const uint32_t ym = (by0 * 4 + (uint32_t)m) & (n - 1), ye = (by0 * 4 + (uint32_t)(m - 5)) & (n - 1);
          for (int x = 0; x < 4; ++x) {
            mp[x] = img[(size_t)ym * n + bx * 4 + x];
            ep[x] = img[(size_t)ye * n + bx * 4 + x];
          }
        };
        auto lookup10 = [&](const uint32_t idx[10], uint32_t v[10]) {
          const uint32_t y0 = (by0 * 4 + (uint32_t)(last_m - 3)) & (n - 1);
          for (int i = 0; i < 10; ++i) v[i] = img[(size_t)(y0 + idx[i] / 4) * n + bx * 4 + idx[i] % 4];
        };
        auto exchange = [&](int s, const PvrtcColors &own, PvrtcColors &left, PvrtcColors &right) {
          const size_t row = (size_t)((by0 + lw + (uint32_t)s) % lw) * lw;
          if (own.a != col[row + bx].a || own.b != col[row + bx].b) ok = 0;
          left = col[row + (bx + lw - 1) % lw];
          right = col[row + (bx + 1) % lw];
        };
        uint32_t stored = 0;
        auto store = [&](uint32_t j, uint32_t data, const PvrtcColors &own) {
          const uint32_t *o = reinterpret_cast<const uint32_t *>(out) + 2 * (size_t)(spread_bits16_host(bx) << 1 | spread_bits16_host(by0 + j));
          if (o[0] != data || o[1] != pvrtc_pack_colors(own.a, own.b, true)) ok = 0;
          stored |= 1u << j;
        };
        pvrtc4_onepass_strip(k_blocks, img[0], tick, lookup10, exchange, store);
        if (!ok || stored != (1u << k_blocks) - 1u) { delete[] col; return 0; }
      }
  delete[] col;
  return 1;
}
// Three-pass host driver over the device math above (tests/host_emul only).
template <int XI, int YI>
static inline void emul_mods_xy(const uint32_t px[32], const PvrtcAB nb[3][3], uint8_t mods[32]) {
  mods[8 * YI + XI] = (uint8_t)pvrtc_pixel_mod<XI, YI>(px[8 * YI + XI], nb);
  if constexpr (XI + 1 < 8) emul_mods_xy<XI + 1, YI>(px, nb, mods);
  else if constexpr (YI + 1 < 4) emul_mods_xy<0, YI + 1>(px, nb, mods);
}

static inline int emul_pvrtc2(const uint8_t *src, uint32_t n, uint8_t *out) {
  const uint32_t bw = n / 8, bh = n / 4;
  const uint32_t *img = reinterpret_cast<const uint32_t *>(src);
  PvrtcAB *ab = new PvrtcAB[(size_t)bw * bh];
  uint32_t *ca = new uint32_t[(size_t)bw * bh], *cb = new uint32_t[(size_t)bw * bh];
  uint8_t *mods = new uint8_t[(size_t)n * n];
  uint32_t *self_right = new uint32_t[(size_t)bw * bh], *self_below = new uint32_t[(size_t)2 * bw * bh];
  for (uint32_t by = 0; by < bh; ++by)
    for (uint32_t bx = 0; bx < bw; ++bx) {
      uint32_t px[32];
      for (int i = 0; i < 32; ++i) px[i] = img[(size_t)(by * 4 + i / 8) * n + bx * 8 + i % 8];
      Stash32 st;
      uint32_t a, b;
      pvrtc_extremes(px, img[0], st, a, b);
      a = channel_reduce(a, false);
      b = channel_reduce(b, true);
      ca[by * bw + bx] = a; cb[by * bw + bx] = b;
      PvrtcAB e = { pair_rb(a), pair_ga(a), pair_rb(b), pair_ga(b) };
      ab[by * bw + bx] = e;
    }
  for (uint32_t by = 0; by < bh; ++by)
    for (uint32_t bx = 0; bx < bw; ++bx) {
      uint32_t px[32];
      for (int i = 0; i < 32; ++i) px[i] = img[(size_t)(by * 4 + i / 8) * n + bx * 8 + i % 8];
      PvrtcAB nb[3][3];
      for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx)
          nb[dy][dx] = ab[((by + bh + dy - 1) % bh) * bw + (bx + bw + dx - 1) % bw];
      uint8_t m[32], m2[32];
      emul_mods_xy<0, 0>(px, nb, m);  // generic per-pixel path
      uint32_t rows[4][2], right_px[4], below_px[8], right_col, below[2];
      for (int y = 0; y < 4; ++y) right_px[y] = img[(size_t)(by * 4 + y) * n + ((bx * 8 + 8) & (n - 1))];
      for (int x = 0; x < 8; ++x) below_px[x] = img[(size_t)((by * 4 + 4) & (n - 1)) * n + bx * 8 + x];
      PvrtcColors nbc[3][3];
      for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
          const size_t o = ((by + bh + dy - 1) % bh) * bw + (bx + bw + dx - 1) % bw;
          nbc[dy][dx].a = ca[o];
          nbc[dy][dx].b = cb[o];
        }
      pvrtc_block_mods(px, right_px, below_px, nbc, rows, &right_col, below);  // separable path (what the kernel runs)
      for (int i = 0; i < 32; ++i) m2[i] = (uint8_t)(rows[i / 8][(i % 8) >> 2] >> (8 * (i & 3)));
      if (memcmp(m, m2, 32) != 0) return 0;
      for (int i = 0; i < 32; ++i) mods[(size_t)(by * 4 + i / 8) * n + bx * 8 + i % 8] = m[i];
      self_right[by * bw + bx] = right_col;
      self_below[2 * (by * bw + bx)] = below[0];
      self_below[2 * (by * bw + bx) + 1] = below[1];
    }
  for (uint32_t by = 0; by < bh; ++by)
    for (uint32_t bx = 0; bx < bw; ++bx) {
      uint32_t rows[4][2], right = 0, below[2] = { 0, 0 };
      for (int y = 0; y < 4; ++y)
        for (int h = 0; h < 2; ++h) {
          rows[y][h] = 0;
          for (int x = 0; x < 4; ++x) rows[y][h] |= (uint32_t)mods[(size_t)(by * 4 + y) * n + bx * 8 + 4 * h + x] << (8 * x);
        }
      for (int y = 0; y < 4; ++y) right |= (uint32_t)mods[(size_t)(by * 4 + y) * n + ((bx * 8 + 8) & (n - 1))] << (8 * y);
      for (int x = 0; x < 8; ++x) below[x >> 2] |= (uint32_t)mods[(size_t)((by * 4 + 4) & (n - 1)) * n + bx * 8 + x] << (8 * (x & 3));
      // pvrtc_left_edge_mod (what the encode kernel precomputes for the column right of each wave) == the per-pixel path
      for (uint32_t y = 0; y < 4; ++y) {
        const uint32_t up = (y < 2 ? by + bh - 1 : by) % bh, dn = (up + 1) % bh, lx = (bx + bw - 1) % bw;
        const PvrtcColors ul = { ca[up * bw + lx], cb[up * bw + lx] }, uc = { ca[up * bw + bx], cb[up * bw + bx] };
        const PvrtcColors ll = { ca[dn * bw + lx], cb[dn * bw + lx] }, lc = { ca[dn * bw + bx], cb[dn * bw + bx] };
        if (pvrtc_left_edge_mod(img[(size_t)(by * 4 + y) * n + bx * 8], y, ul, uc, ll, lc) !=
            mods[(size_t)(by * 4 + y) * n + bx * 8]) return 0;
      }
      // the halo values each lane recomputes for itself must equal the neighbours' own values
      if (right != self_right[by * bw + bx] || below[0] != self_below[2 * (by * bw + bx)] ||
          below[1] != self_below[2 * (by * bw + bx) + 1]) return 0;
      bool one_bpp;
      const uint32_t data = pvrtc_block_modulation(rows, right, below, &one_bpp);
      const uint32_t colors = pvrtc_pack_colors(ca[by * bw + bx], cb[by * bw + bx], one_bpp);
      {  // the row-streaming encoder (what the kernel runs) must agree
        PvrtcColors nbc[3][3];
        for (int dy = 0; dy < 3; ++dy)
          for (int dx = 0; dx < 3; ++dx) {
            const size_t o2 = ((by + bh + dy - 1) % bh) * bw + (bx + bw + dx - 1) % bw;
            nbc[dy][dx].a = ca[o2];
            nbc[dy][dx].b = cb[o2];
          }
        auto loader = [&](int r, uint32_t *pixels, uint32_t *right_px) {
          const uint32_t yy = (by * 4 + (uint32_t)r) & (n - 1);
          for (int x = 0; x < 8; ++x) pixels[x] = img[(size_t)yy * n + bx * 8 + x];
          *right_px = img[(size_t)yy * n + ((bx * 8 + 8) & (n - 1))];
        };
        uint32_t data2;
        bool one2;
        pvrtc_encode_block_rows(loader, nbc, &data2, &one2);
        if (data2 != data || one2 != one_bpp) return 0;
      }
      uint32_t *o = reinterpret_cast<uint32_t *>(out) + 2 * (size_t)pvrtc_z_index(bx, by);
      o[0] = data;
      o[1] = colors;
    }
  // the strip encoder (what the kernel runs) must reproduce every block for several strip heights
  for (uint32_t k_blocks = 1; k_blocks <= 8 && k_blocks <= bh; k_blocks *= 2)
    for (uint32_t by0 = 0; by0 < bh; by0 += k_blocks)
      for (uint32_t bx = 0; bx < bw; ++bx) {
        auto load_px = [&](uint32_t r, uint32_t *pixels, uint32_t *right_px) {
          const uint32_t yy = (by0 * 4 + r) & (n - 1);
          for (int x = 0; x < 8; ++x) pixels[x] = img[(size_t)yy * n + bx * 8 + x];
          *right_px = img[(size_t)yy * n + ((bx * 8 + 8) & (n - 1))];
        };
        auto load_colours = [&](int j, PvrtcColors c[3]) {
          const uint32_t yy = (by0 + bh + (uint32_t)j) % bh;
          for (int dx = 0; dx < 3; ++dx) {
            const size_t o2 = (size_t)yy * bw + (bx + bw + dx - 1) % bw;
            c[dx].a = ca[o2];
            c[dx].b = cb[o2];
          }
        };
        int ok = 1;
        auto store = [&](uint32_t j, uint32_t data, bool one_bpp, const PvrtcColors &own) {
          const uint32_t *o = reinterpret_cast<const uint32_t *>(out) + 2 * (size_t)pvrtc_z_index(bx, by0 + j);
          if (o[0] != data || o[1] != pvrtc_pack_colors(own.a, own.b, one_bpp)) ok = 0;
        };
        auto no_right = [&](uint32_t, uint32_t) -> uint32_t { return 0u; };
        pvrtc_encode_strip<false>(k_blocks, load_px, load_colours, store, no_right);
        if (!ok) return 0;
        // EXCHANGE form: the right-hand values come from the neighbouring column (here: the per-pixel reference path)
        auto right_of = [&](uint32_t j, uint32_t col0) -> uint32_t {
          uint32_t own0 = 0, r = 0;
          for (int y = 0; y < 4; ++y) {
            own0 |= (uint32_t)mods[(size_t)((by0 + j) * 4 + y) * n + bx * 8] << (8 * y);
            r |= (uint32_t)mods[(size_t)((by0 + j) * 4 + y) * n + ((bx * 8 + 8) & (n - 1))] << (8 * y);
          }
          if (own0 != col0) ok = 0;  // what the lane hands to its left-hand neighbour
          return r;
        };
        pvrtc_encode_strip<true>(k_blocks, load_px, load_colours, store, right_of);
        if (!ok) return 0;
        // the one-pass walker (r05: what icamd_pvrtc2_onepass_kernel runs): morphs its own column, is handed the neighbour
        // columns' colours and column-0 values (here: the reference values; what it hands out is checked against them)
        int last_m = -100;
        auto tick = [&](int m, uint32_t *mp, uint32_t *ep) {
          last_m = m;
          const uint32_t ym = (by0 * 4 + (uint32_t)m) & (n - 1), ye = (by0 * 4 + (uint32_t)(m - 5)) & (n - 1);
          for (int x = 0; x < 8; ++x) {
            mp[x] = img[(size_t)ym * n + bx * 8 + x];
            ep[x] = img[(size_t)ye * n + bx * 8 + x];
          }
        };
        auto lookup10 = [&](const uint32_t idx[10], uint32_t v[10]) {
          const uint32_t y0 = (by0 * 4 + (uint32_t)(last_m - 3)) & (n - 1);  // first row of the block just consumed
          for (int i = 0; i < 10; ++i) v[i] = img[(size_t)(y0 + idx[i] / 8) * n + bx * 8 + idx[i] % 8];
        };
        auto exchange = [&](int s, const PvrtcColors &own, uint32_t col0, PvrtcColors &left, PvrtcColors &right, uint32_t &right_col0) {
          if (s <= (int)k_blocks) {
            const uint32_t yy = (by0 + bh + (uint32_t)s) % bh;
            const size_t o2 = (size_t)yy * bw;
            if (own.a != ca[o2 + bx] || own.b != cb[o2 + bx]) ok = 0;
            left.a = ca[o2 + (bx + bw - 1) % bw]; left.b = cb[o2 + (bx + bw - 1) % bw];
            right.a = ca[o2 + (bx + 1) % bw]; right.b = cb[o2 + (bx + 1) % bw];
          }
          if (s >= 2) {
            uint32_t own0 = 0, r = 0;
            for (int y = 0; y < 4; ++y) {
              own0 |= (uint32_t)mods[(size_t)((by0 + (uint32_t)s - 2) * 4 + y) * n + bx * 8] << (8 * y);
              r |= (uint32_t)mods[(size_t)((by0 + (uint32_t)s - 2) * 4 + y) * n + ((bx * 8 + 8) & (n - 1))] << (8 * y);
            }
            if (own0 != col0) ok = 0;
            right_col0 = r;
          }
        };
        uint32_t stored = 0;
        auto store1 = [&](uint32_t j, uint32_t data, bool one_bpp, const PvrtcColors &own) {
          store(j, data, one_bpp, own);
          stored |= 1u << j;
        };
        pvrtc_onepass_strip(k_blocks, img[0], tick, lookup10, exchange, store1);
        if (!ok || stored != (k_blocks >= 32 ? 0xffffffffu : (1u << k_blocks) - 1u)) return 0;
      }
  delete[] ab; delete[] ca; delete[] cb; delete[] mods; delete[] self_right; delete[] self_below;
  return 1;
}
#endif

}  // namespace icamd
#endif  // ICAMD_PVRTC_BLOCK_H_
