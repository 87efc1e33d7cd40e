// bc45_block.h -- BC4 (RGTC1) and BC5 (RGTC2) block math on packed one-channel rows (extension, include/ic_amd.h ICAMD_BC4).
//
// A BC4 block is the alpha half of a DXT5 block, and BC4 of channel c is DEFINED as the reference's DXT5 alpha half of the
// image whose alpha is channel c (ComputeBaseAlphas + ComputeAlphaBits, dxtc.cc:374-479; decode DecodeAlphaValues,
// dxtc.cc:195-217).  The search is therefore the DXT5 one (encode_alpha_pairs, dxt_block.h) -- what differs is where the
// values come from: a one-channel source row of a block is ONE dword (pixel x = byte x), so a block is four dwords instead
// of sixteen pixel dwords, and each pixel pair {v(q), v(q + 8)} the search runs on is one v_perm_b32 of two rows.
//
// Rows: r[y] byte x = value of pixel (x, y) of the block (y = 0..3).
#ifndef ICAMD_BC45_BLOCK_H_
#define ICAMD_BC45_BLOCK_H_

#include "blockops_block.h"  // dxt5_alpha_planes, dxt5_row_alpha_selector (the palette-plane row decode)
#include "dxt_block.h"
#include "ic_device.h"

namespace icamd {

// BC4 block of four packed rows (8 bytes: alpha0, alpha1, 16 three-bit codes).  one_pixel: the block lies wholly right of
// AND below the image (has_one_pixel, pixel4x4.cc:58); its gathered pixels are all the image's corner pixel.
ICAMD_DEV Out8 encode_bc4_rows(const uint32_t r[4], bool one_pixel) {
  uint32_t w[8];
  ICAMD_UNROLL
  for (int q = 0; q < 8; ++q)  // pixel q = (q & 3, q >> 2) and pixel q + 8 = (q & 3, (q >> 2) + 2): {v(q), 0, v(q + 8), 0}
    w[q] = perm(r[(q >> 2) + 2], r[q >> 2], 0x0c040c00u + 0x00010001u * (uint32_t)(q & 3));
  return encode_alpha_pairs(w, r[0] & 0xffu, one_pixel);
}

// Two channels from the rows of a two-byte (RG) source: d0, d1 = the 8 bytes of one block row (R0 G0 R1 G1 | R2 G2 R3 G3).
ICAMD_DEV uint32_t rg_row_r(uint32_t d0, uint32_t d1) { return perm(d1, d0, 0x06040200u); }
ICAMD_DEV uint32_t rg_row_g(uint32_t d0, uint32_t d1) { return perm(d1, d0, 0x07050301u); }

// BC4 block (w0, w1 = its 8 bytes as little-endian dwords) -> its four pixel rows, byte x of rows[y] = pixel (x, y): the
// eight palette values as two dwords of bytes (dxt5_alpha_planes) and one v_perm_b32 per row whose selector bytes are the
// row's 3-bit codes.
ICAMD_DEV void decode_bc4_rows(uint32_t w0, uint32_t w1, uint32_t rows[4]) {
  uint32_t tlo, thi;
  dxt5_alpha_planes(w0, tlo, thi);
  const uint32_t lo24 = w0 >> 16 | (w1 & 0xffu) << 16, hi24 = w1 >> 8;  // codes of pixels 0-7 / 8-15
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) rows[y] = perm(thi, tlo, dxt5_row_alpha_selector(lo24, hi24, y));
}

// Interleave an R row and a G row (4 values each) into the 8 bytes R0 G0 R1 G1 | R2 G2 R3 G3 of an RG8 row.
ICAMD_DEV void interleave_rg_row(uint32_t r, uint32_t g, uint32_t out[2]) {
  out[0] = perm(g, r, 0x05010400u);
  out[1] = perm(g, r, 0x07030602u);
}

}  // namespace icamd
#endif  // ICAMD_BC45_BLOCK_H_
