// TEST INFRASTRUCTURE ONLY.  The BC4 / BC5 block math of image-compression_amd/csrc/bc45_block.h compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION, like emul.cc) so that the CPU tier checks it against the oracle's definition
// (tests/test_bc45_host.py).  Never linked into libic_amd.so; the product has no CPU path.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <algorithm>
#include <cstring>

#include "bc45_block.h"
#include "emul_violations.h"

using namespace icamd;

namespace {
// byte `ch` of the COMPS-byte pixels of the block at pixel (row, col), clamped to the image: r[y] byte x = pixel (x, y)
void gather_rows(const uint8_t *src, uint32_t comps, uint32_t h, uint32_t w, uint32_t stride, uint32_t row, uint32_t col,
                 uint32_t ch, uint32_t r[4]) {
  for (uint32_t y = 0; y < 4; ++y) {
    r[y] = 0;
    for (uint32_t x = 0; x < 4; ++x)
      r[y] |= (uint32_t)src[(size_t)std::min(row + y, h - 1) * stride + (size_t)std::min(col + x, w - 1) * comps + ch] << (8 * x);
  }
}
}  // namespace

// The encoders as the kernels run them (bc45_kernels.hip): 1- and 2-byte sources through the packed-row form, 3- and 4-byte
// sources through the DXT5 alpha search on byte 0 / 2 (R) and 1 (G).  packed_only = 1: the packed-row form for every source.
// codec 5 = BC4, 6 = BC5.  Returns 0 for an argument the C ABI refuses.
extern "C" int bc45_emul_encode(int codec, int comps, int swap, int packed_only, uint32_t h, uint32_t w, uint32_t gh,
                                uint32_t gw, uint32_t stride, const uint8_t *src, uint8_t *out) {
  const bool bc5 = codec == 6;
  if (comps < (bc5 ? 2 : 1) || comps > 4 || (swap && comps < 3)) return 0;
  const uint32_t rows = (std::max(h, gh) + 3) / 4, cols = (std::max(w, gw) + 3) / 4, bytes = bc5 ? 16 : 8;
  const uint32_t rch = swap ? 2 : 0;
  for (uint32_t br = 0; br < rows; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      const bool one_pixel = bc * 4 >= w && br * 4 >= h;
      Out8 a, b = { 0, 0 };
      if (comps <= 2 || packed_only) {
        uint32_t r[4], g[4];
        if (comps == 1 && !packed_only) {
          gather_rows(src, 1, h, w, stride, br * 4, bc * 4, 0, r);
        } else if (comps == 2 && !packed_only) {
          // the kernel's RG8 interior path: two dwords per row, split by v_perm
          uint32_t d[4][2];
          gather_rows(src, 2, h, w, stride, br * 4, bc * 4, 0, r);
          gather_rows(src, 2, h, w, stride, br * 4, bc * 4, 1, g);
          for (int y = 0; y < 4; ++y) {
            interleave_rg_row(r[y], g[y], d[y]);  // the RG8 source bytes of the row
            r[y] = rg_row_r(d[y][0], d[y][1]);
            g[y] = rg_row_g(d[y][0], d[y][1]);
          }
        } else {
          gather_rows(src, comps, h, w, stride, br * 4, bc * 4, rch, r);
          if (bc5) gather_rows(src, comps, h, w, stride, br * 4, bc * 4, 1, g);
        }
        a = encode_bc4_rows(r, one_pixel);
        if (bc5) b = encode_bc4_rows(g, one_pixel);
      } else {
        uint32_t px[16];
        if (comps == 4) load_block<4>(src, h, w, stride, br * 4, bc * 4, px);
        else load_block<3>(src, h, w, stride, br * 4, bc * 4, px);
        a = swap ? encode_dxt5_alpha_block<2>(px, one_pixel) : encode_dxt5_alpha_block<0>(px, one_pixel);
        if (bc5) b = encode_dxt5_alpha_block<1>(px, one_pixel);
      }
      uint8_t *o = out + ((size_t)br * cols + bc) * bytes;
      memcpy(o, &a, 8);
      if (bc5) memcpy(o + 8, &b, 8);
    }
  return 1;
}

// The decoders' row math (decode_bc4_rows, interleave_rg_row): h rows of w * (1 | 2) + pad bytes; the pad bytes are left alone.
extern "C" int bc45_emul_decode(int codec, uint32_t h, uint32_t w, uint32_t pad, const uint8_t *blocks, uint8_t *out) {
  const bool bc5 = codec == 6;
  const uint32_t c = bc5 ? 2 : 1, bytes = bc5 ? 16 : 8, cols = (w + 3) / 4, stride = w * c + pad;
  for (uint32_t br = 0; br < (h + 3) / 4; ++br)
    for (uint32_t bc = 0; bc < cols; ++bc) {
      const uint8_t *b = blocks + ((size_t)br * cols + bc) * bytes;
      uint32_t wd[4];
      memcpy(wd, b, bytes);
      uint32_t r[4], g[4], row[4][2];
      decode_bc4_rows(wd[0], wd[1], r);
      if (bc5) decode_bc4_rows(wd[2], wd[3], g);
      for (int y = 0; y < 4; ++y) {
        if (bc5) interleave_rg_row(r[y], g[y], row[y]);
        else row[y][0] = r[y];
      }
      for (uint32_t y = 0; y < 4 && br * 4 + y < h; ++y)
        for (uint32_t i = 0; i < 4 * c && bc * 4 * c + i < w * c; ++i)
          out[(size_t)(br * 4 + y) * stride + bc * 4 * c + i] = (uint8_t)(row[y][i >> 2] >> (8 * (i & 3)));
    }
  return 1;
}

// One block of 16 values (raster order) through both forms: the packed-row encoder and the DXT5 alpha block it restates.
extern "C" void bc45_emul_block_both(const uint8_t v[16], int one_pixel, uint8_t rows_out[8], uint8_t dxt5_out[8]) {
  uint32_t r[4], px[16];
  for (int y = 0; y < 4; ++y) r[y] = (uint32_t)v[4 * y] | (uint32_t)v[4 * y + 1] << 8 | (uint32_t)v[4 * y + 2] << 16 | (uint32_t)v[4 * y + 3] << 24;
  for (int p = 0; p < 16; ++p) px[p] = 0x00a5c3e1u | (uint32_t)v[p] << 24;
  const Out8 a = encode_bc4_rows(r, one_pixel != 0), b = encode_dxt5_alpha_block(px, one_pixel != 0);
  memcpy(rows_out, &a, 8);
  memcpy(dxt5_out, &b, 8);
}
