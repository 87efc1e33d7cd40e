// metric_block.h -- per-block error accumulation of the quality metric (icamd_measure_error_device, include/ic_amd.h):
// decode a block in registers with the decoders' own math (decode_block.h, blockops_block.h, bc45_block.h), compare it with
// the block's source pixels, and add the squared differences / keep the largest absolute difference per channel.  Nothing is
// written per pixel.  Everything is integer, so the sums are exact whatever the order.
//
// Two forms:
//  * pixels as R,G,B,A dwords (DXT1, DXT5, ETC1, PVRTC): |s - d| on 16-bit lanes, two channels per register -- (R, B) and
//    (G, A) -- whose running maximum is one packed instruction each; the four pixels' differences of one channel are then
//    four BYTES of a dword, and their sum of squares is one v_dot4_u32_u8 of that dword with itself;
//  * one-channel rows, byte x = pixel x (BC4, BC5, EAC R11 / RG11 -- the form decode_bc4_rows and decode_eac11 produce): sum d^2 = sum a^2 + sum b^2 -
//    2 sum a b, three v_dot4_u32_u8 per four values, and the maximum on the same 16-bit lanes.
// Range: a squared byte difference is at most 65 025; a lane adds at most 4 blocks x 32 pixels of them, a workgroup 256 lanes:
// 256 * 4 * 32 * 65 025 < 2^32.
#ifndef ICAMD_METRIC_BLOCK_H_
#define ICAMD_METRIC_BLOCK_H_

#include "bc1a_block.h"  // decode_bc1a, decode_bc2
#include "bc45_block.h"  // blockops_block.h (decode_block_rows), decode_block.h, dxt_block.h (packed 16-bit helpers)
#include "bc7_block.h"  // decode_bc7
#include "eac11_block.h"  // decode_eac11
#include "etc2_a1_block.h"  // decode_etc2_a1
#include "etc2_block.h"  // decode_etc2_rgba8, decode_etc2_colour
#include "ic_device.h"

namespace icamd {

struct MetricAcc {
  uint32_t sse[4];        // sum of squared differences of channel k (byte k of a pixel)
  uint32_t mx_rb, mx_ga;  // largest |difference| on 16-bit lanes: (channel 0, channel 2) and (channel 1, channel 3)
};
ICAMD_DEV void metric_clear(MetricAcc &a) {
  a.sse[0] = a.sse[1] = a.sse[2] = a.sse[3] = 0u;
  a.mx_rb = a.mx_ga = 0u;
}
ICAMD_DEV uint32_t metric_max(const MetricAcc &a, int k) {
  const uint32_t v = (k & 1) ? a.mx_ga : a.mx_rb;
  return (k & 2) ? v >> 16 : v & 0xffffu;
}

ICAMD_DEV uint32_t pk_absdiff_u16(uint32_t a, uint32_t b) { return pk_sub_u16(pk_max_u16(a, b), pk_min_u16(a, b)); }

// Four pixels (dwords, byte k = channel k) of the source and of the decoded block.  NCH = 3: byte 3 of either is ignored.
template <int NCH>
ICAMD_DEV void metric_row4(const uint32_t s[4], const uint32_t d[4], MetricAcc &a) {
  uint32_t e_rb[4], e_ga[4];
  ICAMD_UNROLL
  for (int x = 0; x < 4; ++x) {
    e_rb[x] = pk_absdiff_u16(pair_rb(s[x]), pair_rb(d[x]));
    e_ga[x] = NCH == 4 ? pk_absdiff_u16(pair_ga(s[x]), pair_ga(d[x])) : pk_absdiff_u16(bfe(s[x], 8, 8), bfe(d[x], 8, 8));
    a.mx_rb = pk_max_u16(a.mx_rb, e_rb[x]);
    a.mx_ga = pk_max_u16(a.mx_ga, e_ga[x]);
  }
  // differences are below 256: two pixels' lanes share a dword as bytes (c0 p0, c0 p1, c2 p0, c2 p1), two such dwords
  // give each channel's four differences as the four bytes of one operand
  const uint32_t rb01 = e_rb[0] | e_rb[1] << 8, rb23 = e_rb[2] | e_rb[3] << 8;
  const uint32_t ga01 = e_ga[0] | e_ga[1] << 8, ga23 = e_ga[2] | e_ga[3] << 8;
  const uint32_t c0 = perm(rb23, rb01, 0x05040100u), c2 = perm(rb23, rb01, 0x07060302u);
  const uint32_t c1 = perm(ga23, ga01, 0x05040100u);
  a.sse[0] = udot4(c0, c0, a.sse[0]);
  a.sse[1] = udot4(c1, c1, a.sse[1]);
  a.sse[2] = udot4(c2, c2, a.sse[2]);
  if (NCH == 4) {
    const uint32_t c3 = perm(ga23, ga01, 0x07060302u);
    a.sse[3] = udot4(c3, c3, a.sse[3]);
  }
}

// One channel's row of four values (byte x = pixel x) against the decoded row.  K: the channel (0 or 1).
template <int K>
ICAMD_DEV void metric_plane_row(uint32_t s, uint32_t d, MetricAcc &a) {
  a.sse[K] = udot4(s, s, a.sse[K]);
  a.sse[K] = udot4(d, d, a.sse[K]);
  a.sse[K] -= 2u * udot4(s, d, 0u);
  const uint32_t e01 = pk_absdiff_u16(perm(0u, s, 0x0c010c00u), perm(0u, d, 0x0c010c00u));
  const uint32_t e23 = pk_absdiff_u16(perm(0u, s, 0x0c030c02u), perm(0u, d, 0x0c030c02u));
  const uint32_t e = pk_max_u16(e01, e23);
  uint32_t &m = K == 0 ? a.mx_rb : a.mx_ga;  // the channel's maximum lives on the low lane
  m = pk_max_u16(m, pk_max_u16(e & 0xffffu, e >> 16));
}

// DXT1 (CODEC 0), DXT5 (1) or ETC1 (2) block `w` (its 8 / 16 bytes as dwords) of the image at pixel (row, col), against the
// COMPS-byte source pixels there.  Whole blocks decode through the palette planes (decode_block_rows), blocks clipped by the
// image's edge pixel by pixel like the decode kernels; a pixel outside the image compares with itself.
// PRECONDITION row < h, col < wd.
template <int CODEC, int COMPS>
ICAMD_DEV void metric_color_block(const uint32_t *w, bool swap, const uint8_t *img, uint32_t h, uint32_t wd, uint32_t stride,
                                  uint32_t row, uint32_t col, bool wide_ok, MetricAcc &a) {
  uint32_t S[16], D[16];
  load_block<COMPS>(img, h, wd, stride, row, col, S, wide_ok);
  if (row + 4 <= h && col + 4 <= wd) {
    uint32_t rows[4][4];
    decode_block_rows<CODEC>(w, swap, rows);
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      if (CODEC == 1) {
        ICAMD_UNROLL
        for (int x = 0; x < 4; ++x) D[4 * y + x] = rows[y][x];
      } else {  // twelve bytes R G B R | G B R G | B R G B -> one pixel per dword (byte 3: whatever follows)
        D[4 * y + 0] = rows[y][0];
        D[4 * y + 1] = alignbit(rows[y][1], rows[y][0], 24);
        D[4 * y + 2] = alignbit(rows[y][2], rows[y][1], 16);
        D[4 * y + 3] = rows[y][2] >> 8;
      }
    }
  } else {
    if (CODEC == 1) {
      decode_dxt_colors(w[2], w[3], swap, true, D);
      decode_dxt5_alpha(w[0], w[1], D);
    } else if (CODEC == 0) {
      decode_dxt_colors(w[0], w[1], swap, false, D);
    } else {
      decode_etc1(w[0], w[1], D);
    }
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y)
      ICAMD_UNROLL
      for (int x = 0; x < 4; ++x)
        if (row + (uint32_t)y >= h || col + (uint32_t)x >= wd) S[4 * y + x] = D[4 * y + x];
  }
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) metric_row4<CODEC == 1 ? 4 : 3>(&S[4 * y], &D[4 * y], a);
}

// ETC2 RGBA8 block `w` (EXTENSION: EAC alpha word + ETC1-compatible colour word) against the RGBA8 source pixels, four
// channels, with the decoder's own math (decode_etc2_rgba8, swap included); a pixel outside the image compares with itself.
// PRECONDITION row < h, col < wd.
ICAMD_DEV void metric_etc2_block(const uint32_t *w, bool swap, const uint8_t *img, uint32_t h, uint32_t wd, uint32_t stride,
                                 uint32_t row, uint32_t col, bool wide_ok, MetricAcc &a) {
  uint32_t S[16], D[16];
  load_block<4>(img, h, wd, stride, row, col, S, wide_ok);
  decode_etc2_rgba8(w, swap, D);
  if (row + 4 > h || col + 4 > wd) {
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y)
      ICAMD_UNROLL
      for (int x = 0; x < 4; ++x)
        if (row + (uint32_t)y >= h || col + (uint32_t)x >= wd) S[4 * y + x] = D[4 * y + x];
  }
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) metric_row4<4>(&S[4 * y], &D[4 * y], a);
}

// ETC2 RGB8 block `w` (EXTENSION: one colour word in any of the five modes) against the COMPS-byte source pixels, three
// channels, with the decoder's own math (decode_etc2_colour; swap does not enter, as for ETC1); a pixel outside the image
// compares with itself.  PRECONDITION row < h, col < wd.
template <int COMPS>
ICAMD_DEV void metric_etc2_rgb8_block(const uint32_t *w, const uint8_t *img, uint32_t h, uint32_t wd, uint32_t stride,
                                      uint32_t row, uint32_t col, bool wide_ok, MetricAcc &a) {
  uint32_t S[16], D[16];
  load_block<COMPS>(img, h, wd, stride, row, col, S, wide_ok);
  decode_etc2_colour(w[0], w[1], D);
  if (row + 4 > h || col + 4 > wd) {
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y)
      ICAMD_UNROLL
      for (int x = 0; x < 4; ++x)
        if (row + (uint32_t)y >= h || col + (uint32_t)x >= wd) S[4 * y + x] = D[4 * y + x];
  }
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) metric_row4<3>(&S[4 * y], &D[4 * y], a);
}

// ETC2 RGB8A1 block `w` (EXTENSION: one punch-through colour word in any mode, either opaque bit) against the RGBA8 source pixels,
// four channels, with the decoder's own math (decode_etc2_a1, swap included: a transparent texel is (0, 0, 0, 0)); a pixel
// outside the image compares with itself.  PRECONDITION row < h, col < wd.
ICAMD_DEV void metric_etc2_a1_block(const uint32_t *w, bool swap, const uint8_t *img, uint32_t h, uint32_t wd, uint32_t stride,
                                    uint32_t row, uint32_t col, bool wide_ok, MetricAcc &a) {
  uint32_t S[16], D[16];
  load_block<4>(img, h, wd, stride, row, col, S, wide_ok);
  decode_etc2_a1(w[0], w[1], swap, D);
  if (row + 4 > h || col + 4 > wd) {
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y)
      ICAMD_UNROLL
      for (int x = 0; x < 4; ++x)
        if (row + (uint32_t)y >= h || col + (uint32_t)x >= wd) S[4 * y + x] = D[4 * y + x];
  }
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) metric_row4<4>(&S[4 * y], &D[4 * y], a);
}

// BC1A (w[0..1]) or BC2 (w[0..3]) block (EXTENSIONS, bc1a_block.h) against the RGBA8 source pixels, four channels, with the
// decoders' own math (decode_bc1a / decode_bc2, swap included: a transparent BC1A texel is (0, 0, 0, 0), a BC2 alpha is
// nibble x 17); a pixel outside the image compares with itself.  PRECONDITION row < h, col < wd.
template <bool BC2>
ICAMD_DEV void metric_bc1a_bc2_block(const uint32_t *w, bool swap, const uint8_t *img, uint32_t h, uint32_t wd, uint32_t stride,
                                     uint32_t row, uint32_t col, bool wide_ok, MetricAcc &a) {
  uint32_t S[16], D[16];
  load_block<4>(img, h, wd, stride, row, col, S, wide_ok);
  if (BC2) decode_bc2(w, swap, D);
  else decode_bc1a(w[0], w[1], swap, D);
  if (row + 4 > h || col + 4 > wd) {
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y)
      ICAMD_UNROLL
      for (int x = 0; x < 4; ++x)
        if (row + (uint32_t)y >= h || col + (uint32_t)x >= wd) S[4 * y + x] = D[4 * y + x];
  }
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) metric_row4<4>(&S[4 * y], &D[4 * y], a);
}

// BC7 block `w` (EXTENSION: any of the eight modes, or the reserved form) against the COMPS-byte source pixels with the decoder's
// own math (decode_bc7, swap included): four channels for COMPS = 4, R, G, B for COMPS = 3; a pixel outside the image compares
// with itself.  PRECONDITION row < h, col < wd.
template <int COMPS>
ICAMD_DEV void metric_bc7_block(const uint32_t *w, bool swap, const uint8_t *img, uint32_t h, uint32_t wd, uint32_t stride,
                                uint32_t row, uint32_t col, bool wide_ok, MetricAcc &a) {
  uint32_t S[16], D[16];
  load_block<COMPS>(img, h, wd, stride, row, col, S, wide_ok);
  decode_bc7(w, swap, D);
  if (row + 4 > h || col + 4 > wd) {
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y)
      ICAMD_UNROLL
      for (int x = 0; x < 4; ++x)
        if (row + (uint32_t)y >= h || col + (uint32_t)x >= wd) S[4 * y + x] = D[4 * y + x];
  }
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) metric_row4<COMPS>(&S[4 * y], &D[4 * y], a);
}

// Channel `ch` of the COMPS-byte pixels of the block at (row, col), clamped to the image: r[y] byte x = pixel (x, y).
struct __attribute__((packed, aligned(1))) MetricU1 { uint32_t x; };
template <int COMPS>
ICAMD_DEV void metric_gather_channel(const uint8_t *img, uint32_t h, uint32_t wd, uint32_t stride, uint32_t row, uint32_t col,
                                     uint32_t ch, uint32_t r[4]) {
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    const uint8_t *line = img + (size_t)umin(row + (uint32_t)y, h - 1u) * stride + ch;
    uint32_t v = 0;
    ICAMD_UNROLL
    for (int x = 0; x < 4; ++x) v |= (uint32_t)line[(size_t)umin(col + (uint32_t)x, wd - 1u) * COMPS] << (8 * x);
    r[y] = v;
  }
}

// BC4 (w[0..1]) / BC5 (w[0..3]) block against channel R (and G) of the COMPS-byte source: R = byte 0, or byte 2 with swap
// (3 or 4 components); G = byte 1.  EAC: the words are EAC R11 / RG11 words (decode_eac11) instead, same channels and rules.
// PRECONDITION row < h, col < wd.
template <int COMPS, bool BC5, bool EAC = false>
ICAMD_DEV void metric_bc45_block(const uint32_t *w, bool swap, const uint8_t *img, uint32_t h, uint32_t wd, uint32_t stride,
                                 uint32_t row, uint32_t col, bool wide_ok, MetricAcc &a) {
  uint32_t sr[4], sg[4] = { 0, 0, 0, 0 }, dr[4], dg[4] = { 0, 0, 0, 0 };
  const bool whole = wide_ok && row + 4 <= h && col + 4 <= wd;
  const uint32_t rch = (swap && COMPS >= 3) ? 2u : 0u;
  if (whole && COMPS == 1) {
    const uint8_t *p = img + (size_t)row * stride + col;
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) sr[y] = reinterpret_cast<const MetricU1 *>(p + (uint32_t)y * stride)->x;
  } else if (whole && COMPS == 2) {
    const uint8_t *p = img + (size_t)row * stride + (size_t)col * 2u;
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      const U2 v = load_stream(reinterpret_cast<const U2 *>(p + (uint32_t)y * stride));
      sr[y] = rg_row_r(v.x, v.y);
      sg[y] = rg_row_g(v.x, v.y);
    }
  } else if (whole && COMPS >= 3) {
    uint32_t px[16];
    load_block_interior<(COMPS >= 3 ? COMPS : 4)>(img + (size_t)row * stride + (size_t)col * COMPS, 0u, stride, px);
    const uint32_t lo = rch ? 0x0c0c0602u : 0x0c0c0400u, hi = rch ? 0x06020c0cu : 0x04000c0cu;
    ICAMD_UNROLL
    for (int y = 0; y < 4; ++y) {
      sr[y] = perm(px[4 * y + 1], px[4 * y], lo) | perm(px[4 * y + 3], px[4 * y + 2], hi);
      if (BC5) sg[y] = perm(px[4 * y + 1], px[4 * y], 0x0c0c0501u) | perm(px[4 * y + 3], px[4 * y + 2], 0x05010c0cu);
    }
  } else {
    metric_gather_channel<COMPS>(img, h, wd, stride, row, col, rch, sr);
    if (BC5) metric_gather_channel<COMPS>(img, h, wd, stride, row, col, 1u, sg);
  }
  if (EAC) {
    decode_eac11(w[0], w[1], dr);
    if (BC5) decode_eac11(w[2], w[3], dg);
  } else {
    decode_bc4_rows(w[0], w[1], dr);
    if (BC5) decode_bc4_rows(w[2], w[3], dg);
  }
  const uint32_t cols = umin(wd - col, 4u), rows = umin(h - row, 4u);
  const uint32_t m = cols >= 4u ? 0xffffffffu : (1u << (8u * cols)) - 1u;
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    const uint32_t keep = (uint32_t)y < rows ? m : 0u;
    metric_plane_row<0>(sr[y] & keep, dr[y] & keep, a);
    if (BC5) metric_plane_row<1>(sg[y] & keep, dg[y] & keep, a);
  }
}

}  // namespace icamd
#endif  // ICAMD_METRIC_BLOCK_H_
