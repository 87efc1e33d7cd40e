// pvrtc_pair.h -- PVRTC1 2 bpp, the pair path (morph kernel + encode kernel): a block's modulation word and mode from its rows,
// block by block and in the strip form the encode kernel runs.  Part of pvrtc_block.h.
#ifndef ICAMD_PVRTC_PAIR_H_
#define ICAMD_PVRTC_PAIR_H_

#include "pvrtc_pixel.h"

namespace icamd {

template <bool WITH_RIGHT>
ICAMD_DEV void pvrtc_row_mods(uint32_t yw, const PvrtcAB top[3], const PvrtcAB bot[3], const uint32_t *pixels,
                              uint32_t right_pixel, uint32_t row[2], uint32_t *right_mod) {
  uint32_t V[3][4];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    V[c][0] = vblend_pair(yw, top[c].a_rb, bot[c].a_rb);
    V[c][1] = vblend_pair(yw, top[c].a_ga, bot[c].a_ga);
    V[c][2] = vblend_pair(yw, top[c].b_rb, bot[c].b_rb);
    V[c][3] = vblend_pair(yw, top[c].b_ga, bot[c].b_ga);
  }
  pvrtc_row_mods_v<WITH_RIGHT>(V, pixels, right_pixel, row, right_mod);
}

ICAMD_DEV PvrtcAB pvrtc_expand(const PvrtcColors &c) {
  PvrtcAB e = { pair_rb(c.a), pair_ga(c.a), pair_rb(c.b), pair_ga(c.b) };
  return e;
}
// the same from packed RGBA colours
template <bool WITH_RIGHT>
ICAMD_DEV void pvrtc_row_mods(uint32_t yw, const PvrtcColors top[3], const PvrtcColors bot[3], const uint32_t *pixels,
                              uint32_t right_pixel, uint32_t row[2], uint32_t *right_mod) {
  PvrtcAB t[3], b[3];
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    t[c] = pvrtc_expand(top[c]);
    b[c] = pvrtc_expand(bot[c]);
  }
  pvrtc_row_mods<WITH_RIGHT>(yw, t, b, pixels, right_pixel, row, right_mod);
}

// All modulation values a block's encoding depends on, from its 3x3 block neighbourhood nb (toroidal wrap
// applied by the caller): its own 32 (rows[y][h]: byte x&3 of rows[y][x>>2] = pixel (x, y)), the pixel column
// right of it (right_col: byte y; right_px[y] = first pixel of row y of the right-hand block) and the pixel row
// below it (below[0..1]; below_px[0..7] = first pixel row of the block below).  CalculateBlockModulationMode
// looks one pixel right and one pixel down (pvrtc.cc:416-429), so these 12 extra values make the block
// self-contained: no exchange with other lanes is needed.
ICAMD_DEV void pvrtc_block_mods(const uint32_t px[32], const uint32_t right_px[4], const uint32_t below_px[8],
                                const PvrtcColors nb[3][3], uint32_t rows[4][2], uint32_t *right_col, uint32_t below[2]) {
  uint32_t rc = 0;
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    const int y0 = y < 2 ? 0 : 1;
    uint32_t m;
    pvrtc_row_mods<true>((uint32_t)((y + 2) & 3), nb[y0], nb[y0 + 1], &px[8 * y], right_px[y], rows[y], &m);
    rc |= m << (8 * y);
  }
  *right_col = rc;
  // first pixel row of the block below: y_in = 0 there -> block rows (centre, below), weight 2
  pvrtc_row_mods<false>(2u, nb[1], nb[2], below_px, 0u, below, nullptr);
}

// EncodeColors (pvrtc.cc:356-388); colours are the channel-reduced RGBA dwords.
ICAMD_DEV uint32_t pvrtc_pack_colors(uint32_t ca, uint32_t cb, bool mode_1bpp) {
  const uint32_t ar = bfe(ca, 0, 8), ag = bfe(ca, 8, 8), ab = bfe(ca, 16, 8), aa = ca >> 24;
  const uint32_t br = bfe(cb, 0, 8), bg = bfe(cb, 8, 8), bb = bfe(cb, 16, 8), ba = cb >> 24;
  const uint32_t va = aa == 255u ? (1u << 15 | (ab >> 4) << 1 | (ag >> 3) << 5 | (ar >> 3) << 10)
                                 : ((ab >> 5) << 1 | (ag >> 4) << 4 | (ar >> 4) << 8 | (aa >> 5) << 12);
  const uint32_t vb = ba == 255u ? (1u << 31 | (bb >> 3) << 16 | (bg >> 3) << 21 | (br >> 3) << 26)
                                 : ((bb >> 4) << 16 | (bg >> 4) << 20 | (br >> 4) << 24 | (ba >> 5) << 28);
  return va | vb | (mode_1bpp ? 0u : 1u);
}

// CalculateBlockModulationMode + CalculateBlockModulationData (pvrtc.cc:395-496) for one block.
// rows[y][0..1]: the block's modulation values as bytes (pixel x of row y = byte x&3 of rows[y][x>>2]);
// right_col: byte y = modulation of the pixel right of (7, y); below[0..1]: row below (bytes, x order).
// Returns the 32-bit modulation word; *mode_1bpp tells EncodeColors which flag to store.
ICAMD_DEV uint32_t pvrtc_block_modulation(const uint32_t rows[4][2], uint32_t right_col, const uint32_t below[2],
                                          bool *mode_1bpp) {
  uint32_t inter = 0, hc = 0, vc = 0, d1 = 0, d2 = 0;
  ICAMD_UNROLL
  for (int y = 0; y < 4; ++y) {
    ICAMD_UNROLL
    for (int h = 0; h < 2; ++h) {
      const uint32_t r = rows[y][h];
      // pixels best served by an intermediate value (1 or 2): low bit xor high bit of each byte
      inter += popcount_u32((r ^ (r >> 1)) & 0x01010101u);
      // "horizontal_count" in the source sums |m - m(x, y+1)|, "vertical_count" |m - m(x+1, y)|
      // (the names are swapped there, pvrtc.cc:426-429; kept as the reference computes them).
      const uint32_t down = y < 3 ? rows[y + 1][h] : below[h];
      hc = sad_u8(r, down, hc);
      // neighbour to the right: bytes shifted by one pixel; the last byte comes from the next dword of the
      // row or from the right-hand block's first column
      const uint32_t next = h == 0 ? rows[y][1] : (bfe(right_col, 8 * y, 8));
      vc = sad_u8(r, alignbit(next, r, 8), vc);
      // 1BPP word: bit 8y+x = m >> 1.  The four high bits of a dword's bytes are gathered into a nibble by
      // one multiply (bit 8j+1 -> bit 24+j; no two partial products collide below bit 28).
      const int pos = 8 * y + 4 * h;
      d1 |= ((((r >> 1) & 0x01010101u) * 0x01020408u) >> 24) << pos;
      // 2BPP word: checkerboard samples ((x^y)&1 == 0), 2 bits each, in raster order: bytes 0,2 of the dword on
      // even rows, bytes 1,3 on odd rows -> one nibble at the same position as the 1BPP nibble.
      const uint32_t v = ((y & 1) ? r >> 8 : r) & 0x00030003u;
      d2 |= ((v | v >> 14) & 0xfu) << pos;
    }
  }
  // modes: 0 = 1BPP, 1 = average-4, 2 = vertical, 3 = horizontal (pvrtc.cc:433-446)
  uint32_t mode = 1u;
  if (inter <= 4u) mode = 0u;
  else if (vc > 10u && vc > hc * 2u) mode = 2u;
  else if (hc > 10u && hc > vc * 2u) mode = 3u;
  // The samples at bit 0 (0,0) and bit 20 (4,2) keep only their high bit; the low bit selects the sub-mode
  // (pvrtc.cc:474-487): bit 0 = "not average-4", bit 20 = "vertical".
  d2 = mode == 1u ? (d2 & ~1u) : (d2 | 1u);
  d2 = mode == 2u ? (d2 | 1u << 20) : (d2 & ~(1u << 20));
  *mode_1bpp = mode == 0u;
  return mode == 0u ? d1 : d2;
}

// Row-streaming form of pvrtc_block_mods + pvrtc_block_modulation: the block is consumed one pixel row at a
// time (rows 0..3 of the block, then the first row of the block below), so only one row of pixels, its 9
// modulation values and a handful of counters are live at any moment -- this is what keeps the encode kernel
// at <= 64 VGPRs (8 waves per SIMD), where the full-rate add/and/shift instructions actually pay off.
// load(r, pixels[8], &right): r = 0..3 -> pixel row r of the block and the pixel right of it;
//                             r = 4    -> first pixel row of the block below (right unused).

template <typename RowLoader>
ICAMD_DEV void pvrtc_encode_block_rows(RowLoader &load, const PvrtcColors nb[3][3], uint32_t *data_out,
                                       bool *mode_1bpp) {
  uint32_t inter = 0, hc = 0, vc = 0, d1 = 0, d2 = 0, prev[2] = { 0, 0 };
  uint32_t cur[8], cur_right = 0, nxt[8], nxt_right = 0;
  load(0, cur, &cur_right);
  ICAMD_UNROLL
  for (int r = 0; r < 5; ++r) {
    if (r < 4) load(r + 1, nxt, &nxt_right);  // prefetch the next row while this one is processed
    ICAMD_SCHED_FENCE();
    uint32_t row[2], right_mod = 0;
    if (r < 4) {
      const int y0 = r < 2 ? 0 : 1;
      pvrtc_row_mods<true>((uint32_t)((r + 2) & 3), nb[y0], nb[y0 + 1], cur, cur_right, row, &right_mod);
    } else {
      pvrtc_row_mods<false>(2u, nb[1], nb[2], cur, 0u, row, nullptr);  // y_in = 0 of the block below
    }
    if (r > 0) {  // "horizontal_count" = sum |m - m(x, y+1)| (names swapped in the source, pvrtc.cc:426-429)
      hc = sad_u8(prev[0], row[0], hc);
      hc = sad_u8(prev[1], row[1], hc);
    }
    if (r < 4) {
      // "vertical_count" = sum |m - m(x+1, y)|: bytes shifted by one pixel, last one from the right-hand block
      vc = sad_u8(row[0], alignbit(row[1], row[0], 8), vc);
      vc = sad_u8(row[1], alignbit(right_mod, row[1], 8), vc);
      ICAMD_UNROLL
      for (int h = 0; h < 2; ++h) {
        const uint32_t m = row[h];
        inter += popcount_u32((m ^ (m >> 1)) & 0x01010101u);  // values 1 or 2: low bit xor high bit
        const int pos = 8 * r + 4 * h;
        d1 |= ((((m >> 1) & 0x01010101u) * 0x01020408u) >> 24) << pos;  // 1BPP: bit 8y+x = m >> 1
        const uint32_t v = ((r & 1) ? m >> 8 : m) & 0x00030003u;         // 2BPP: checkerboard samples
        d2 |= ((v | v >> 14) & 0xfu) << pos;
      }
      prev[0] = row[0];
      prev[1] = row[1];
      ICAMD_UNROLL
      for (int i = 0; i < 8; ++i) cur[i] = nxt[i];
      cur_right = nxt_right;
    }
    ICAMD_SCHED_FENCE();
  }
  uint32_t mode = 1u;  // 0 = 1BPP, 1 = average-4, 2 = vertical, 3 = horizontal (pvrtc.cc:433-446)
  if (inter <= 4u) mode = 0u;
  else if (vc > 10u && vc > hc * 2u) mode = 2u;
  else if (hc > 10u && hc > vc * 2u) mode = 3u;
  d2 = mode == 1u ? (d2 & ~1u) : (d2 | 1u);                 // pvrtc.cc:474-487
  d2 = mode == 2u ? (d2 | 1u << 20) : (d2 & ~(1u << 20));
  *mode_1bpp = mode == 0u;
  *data_out = mode == 0u ? d1 : d2;
}

// ---- strip form: one lane encodes K vertically adjacent blocks of one block column ---------------------------------
// Walking down a column, the pixel row below a block IS row 0 of the next block, so the "below" halo row of
// pvrtc_encode_block_rows (8 of its 12 redundant modulation values plus one row set-up) is computed once instead of
// twice; only the last block of a strip still pays for it.  A block is finished (its mode decided, its words stored)
// right after row 0 of the block under it.  44 -> 36 + 8/K modulation values per block.
struct PvrtcBlockAcc {
  uint32_t hc, vc, d1, d2;
  uint32_t u01, u23;    // rows (0, 1) / (2, 3): byte x = m(x, y) | m(x, y + 1) << 2 | m(x + 4, y) << 4 | m(x + 4, y + 1) << 6
  uint32_t col0, col7;  // EXCHANGE only: byte y = modulation of pixel (0, y) / (7, y) of the block
};
// one pixel row (y = 0..3, compile-time after unrolling) of a block: everything except the vertical differences.
// The bit gathers of CalculateBlockModulationData (pvrtc.cc:456-496) are v_dot4_u32_u8 with power-of-two weights: the
// modulation values sit one per byte, so  sum_x (m_x & 2) * 2^x  is twice the row's eight 1BPP bits, and
// sum_j m_(2j + odd row) * 4^j  its four checkerboard samples (2 bits each) -- one dot per half row instead of a
// shift-mask-multiply-shift chain (r03).
// EXCHANGE: the value right of the row is not computed here -- the term |m(7, y) - m(8, y)| is added when the block is
// finished, from the right-hand neighbour's own column-0 values (pvrtc_encode_strip); the row only records its two
// outer values.
template <bool EXCHANGE>
ICAMD_DEV void pvrtc_acc_row(PvrtcBlockAcc &A, int y, const uint32_t row[2], uint32_t right_mod) {
  A.vc = sad_u8(row[0], alignbit(row[1], row[0], 8), A.vc);   // "vertical_count" = sum |m - m(x+1, y)| (pvrtc.cc:426-429)
  if (EXCHANGE) {
    A.vc = sad_u8(row[1], perm(row[1], row[1], 0x03030201u), A.vc);  // bytes (5, 6, 7, 7): the last term is 0 here
    // byte y of col0 / col7 <- byte 0 of row[0] / byte 3 of row[1]; selector 4 + i keeps byte i of the old value
    const uint32_t keep = 0x07060504u & ~(0xffu << (8 * y));
    A.col0 = perm(A.col0, row[0], keep);
    A.col7 = perm(A.col7, row[1], keep | 0x03u << (8 * y));
  } else {
    A.vc = sad_u8(row[1], alignbit(right_mod, row[1], 8), A.vc);
  }
  // both half rows in one word (r06): byte x = m(x) | m(x + 4) << 4 (at most 51), so that ONE dot product per gather sees
  // all eight values -- a weight w on byte x is w on m(x) and 16 w on m(x + 4), which is what both gathers want
  const uint32_t u = row[0] | row[1] << 4;
  // 1BPP word: bit 8y + x = m >> 1;  sum_x (2 hi(x) + 32 hi(x + 4)) 2^x = twice the row's eight bits
  const uint32_t twice = udot4(u & 0x22222222u, 0x08040201u, 0u);
  A.d1 |= y == 0 ? twice >> 1 : twice << (8 * y - 1);
  // 2BPP word: the samples with (x ^ y) & 1 == 0, 2 bits each, raster order -> byte y
  A.d2 |= udot4(u, (y & 1) ? 0x04000100u : 0x00040001u, 0u) << (8 * y);
  // values 1 or 2 are counted at the end, two rows per dword (fields at bits (0, 1), (4, 5) of a byte | the next row's << 2)
  if (y == 0) A.u01 = u;
  else if (y == 1) A.u01 |= u << 2;
  else if (y == 2) A.u23 = u;
  else A.u23 |= u << 2;
}
ICAMD_DEV uint32_t pvrtc_acc_finish(const PvrtcBlockAcc &A, bool *mode_1bpp) {
  // pixels best served by an intermediate value (1 or 2): low bit xor high bit of each 2-bit field
  const uint32_t inter = popcount_u32((A.u01 ^ (A.u01 >> 1)) & 0x55555555u) + popcount_u32((A.u23 ^ (A.u23 >> 1)) & 0x55555555u);
  uint32_t mode = 1u;  // 0 = 1BPP, 1 = average-4, 2 = vertical, 3 = horizontal (pvrtc.cc:433-446)
  if (inter <= 4u) mode = 0u;
  else if (A.vc > 10u && A.vc > A.hc * 2u) mode = 2u;
  else if (A.hc > 10u && A.hc > A.vc * 2u) mode = 3u;
  uint32_t d2 = mode == 1u ? (A.d2 & ~1u) : (A.d2 | 1u);  // pvrtc.cc:474-487
  d2 = mode == 2u ? (d2 | 1u << 20) : (d2 & ~(1u << 20));
  *mode_1bpp = mode == 0u;
  return mode == 0u ? A.d1 : d2;
}

// Modulation value of the pixel at x_in = 0, row y_in (0..3, a RUN-TIME value) of a block, from the reduced colours of
// the four blocks its interpolation uses: columns (left neighbour, own) x block rows (upper, lower), where (upper,
// lower) = (by - 1, by) for y_in < 2 and (by, by + 1) otherwise (pvrtc.cc:216-227).  With xw = 4 the four bilinear
// weights are 4 (4 - yw), 4 (4 - yw), 4 yw, 4 yw, so the /32 of Interpolate4_2BPP is an exact >> 3 of
// (4 - yw)(c00 + c01) + yw (c10 + c11) (<= 2040 per 16-bit lane).  Used once per strip by the encode kernel for the
// column right of each wave (the lanes in between get these values from their right-hand neighbour lane).
ICAMD_DEV uint32_t pvrtc_left_edge_mod(uint32_t pixel, uint32_t y_in, const PvrtcColors &ul, const PvrtcColors &uc,
                                       const PvrtcColors &ll, const PvrtcColors &lc) {
  const uint32_t yw = (y_in + 2u) & 3u, uw = 4u - yw;
  const uint32_t a_rb = ((uw * (pair_rb(ul.a) + pair_rb(uc.a)) + yw * (pair_rb(ll.a) + pair_rb(lc.a))) >> 3) & 0x00ff00ffu;
  const uint32_t a_ga = ((uw * (pair_ga(ul.a) + pair_ga(uc.a)) + yw * (pair_ga(ll.a) + pair_ga(lc.a))) >> 3) & 0x00ff00ffu;
  const uint32_t b_rb = ((uw * (pair_rb(ul.b) + pair_rb(uc.b)) + yw * (pair_rb(ll.b) + pair_rb(lc.b))) >> 3) & 0x00ff00ffu;
  const uint32_t b_ga = ((uw * (pair_ga(ul.b) + pair_ga(uc.b)) + yw * (pair_ga(ll.b) + pair_ga(lc.b))) >> 3) & 0x00ff00ffu;
  return best_modulation(pixel, a_rb, a_ga, b_rb, b_ga);
}

// load_px(r, pixels[8], &right): pixel row r of the strip, r = 0 .. 4 K (row 4 K = first row of the block below the
//                                strip), and the pixel right of it; toroidal wrap is the loader's business.
// load_colours(j, c[3]):         reduced colours of block row j of the strip (j = -1 .. K), columns left/centre/right.
// store(j, data, mode_1bpp, own): block j of the strip is finished; own = its reduced colours.
// EXCHANGE: the modulation values right of a block (pvrtc.cc:426-429 looks one pixel right) are not computed by the
//   lane -- 4 of the 37 values a block costs -- but fetched when block j is finished:
// right_of(j, col0):             given this lane's column-0 values of block j (byte y = row y), returns those of the
//                                block to its right.  On the device consecutive lanes are consecutive block columns
//                                walking the same rows in lock-step, so this is a one-lane shuffle (the last lane of a
//                                wave reads values its workgroup computed up front with pvrtc_left_edge_mod).
//
// The walk is organised by COLOUR-ROW PAIRS, not by blocks: rows 2, 3 of block s-1 and rows 0, 1 of block s all
// interpolate between the colours of block rows s-1 (A) and s (B), with vertical weights 0, 1, 2, 3
// (pvrtc.cc:216-227).  So the twelve vertical blends 8 ((4 - yw) A + yw B) of a pixel row are set up once per four
// rows (32 A, and the step 8 (B - A)) and then just stepped -- twelve full-rate adds per row instead of re-expanding
// six colours and re-blending them; two pixel-row buffers alternate, so no row is ever copied.
template <bool EXCHANGE, typename PixelRowLoader, typename ColourRowLoader, typename BlockStore, typename RightOf>
ICAMD_DEV void pvrtc_encode_strip(uint32_t k_blocks, PixelRowLoader &load_px, ColourRowLoader &load_colours,
                                  BlockStore &store, RightOf &right_of) {
  PvrtcColors cc[3];
  uint32_t A[3][4];  // colour row s-1 as channel pairs
  load_colours(-1, cc);
  ICAMD_UNROLL
  for (int c = 0; c < 3; ++c) {
    A[c][0] = pair_rb(cc[c].a); A[c][1] = pair_ga(cc[c].a); A[c][2] = pair_rb(cc[c].b); A[c][3] = pair_ga(cc[c].b);
  }
  load_colours(0, cc);
  uint32_t buf0[8], buf1[8], right0 = 0, right1 = 0, prev[2] = { 0, 0 };
  ICAMD_UNROLL
  for (int i = 0; i < 8; ++i) buf1[i] = 0;
  load_px(0u, buf0, &right0);
  PvrtcBlockAcc acc = { 0, 0, 0, 0, 0, 0, 0, 0 };
  PvrtcColors own = cc[1];
  ICAMD_NOUNROLL
  for (uint32_t s = 0;; ++s) {
    // colour rows (s-1, s): V = 32 A, dV = 8 (B - A).  Plain 32-bit arithmetic on the 16-bit channel pairs: every
    // intermediate V is a true blend with both lanes in [0, 8160], so borrows between the lanes cancel exactly.
    uint32_t V[3][4], dV[3][4];
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c) {
      const uint32_t b[4] = { pair_rb(cc[c].a), pair_ga(cc[c].a), pair_rb(cc[c].b), pair_ga(cc[c].b) };
      ICAMD_UNROLL
      for (int v = 0; v < 4; ++v) {
        V[c][v] = A[c][v] << 5;
        dV[c][v] = (b[v] - A[c][v]) << 3;
        A[c][v] = b[v];
      }
    }
    const PvrtcColors own_next = cc[1];
    if (s < k_blocks) load_colours((int)s + 1, cc);  // next segment's colours, in flight during these rows
    uint32_t row[2], right_mod = 0;
    if (s > 0) {
      // rows 2 and 3 of block s-1: weights 0 and 1
      load_px(4u * s - 1u, buf1, &right1);
      ICAMD_SCHED_FENCE();
      pvrtc_row_mods_v<!EXCHANGE>(V, buf0, right0, row, &right_mod);
      acc.hc = sad_u8(prev[0], row[0], acc.hc);  // "horizontal_count" = sum |m - m(x, y+1)| (pvrtc.cc:426-429)
      acc.hc = sad_u8(prev[1], row[1], acc.hc);
      pvrtc_acc_row<EXCHANGE>(acc, 2, row, right_mod);
      prev[0] = row[0]; prev[1] = row[1];
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c)
        ICAMD_UNROLL
        for (int v = 0; v < 4; ++v) V[c][v] += dV[c][v];
      ICAMD_SCHED_FENCE();
      load_px(4u * s, buf0, &right0);
      ICAMD_SCHED_FENCE();
      pvrtc_row_mods_v<!EXCHANGE>(V, buf1, right1, row, &right_mod);
      acc.hc = sad_u8(prev[0], row[0], acc.hc);
      acc.hc = sad_u8(prev[1], row[1], acc.hc);
      pvrtc_acc_row<EXCHANGE>(acc, 3, row, right_mod);
      prev[0] = row[0]; prev[1] = row[1];
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c)
        ICAMD_UNROLL
        for (int v = 0; v < 4; ++v) V[c][v] += dV[c][v];
      ICAMD_SCHED_FENCE();
    } else {
      ICAMD_UNROLL
      for (int c = 0; c < 3; ++c)
        ICAMD_UNROLL
        for (int v = 0; v < 4; ++v) V[c][v] += 2u * dV[c][v];  // the strip starts at weight 2
    }
    // row 0 of block s, weight 2 -- for s == k_blocks the row below the strip, which only completes block K-1
    if (s < k_blocks) load_px(4u * s + 1u, buf1, &right1);
    ICAMD_SCHED_FENCE();
    pvrtc_row_mods_v<!EXCHANGE>(V, buf0, right0, row, &right_mod);
    if (s > 0) {  // the vertical differences across the block boundary, then block s-1 is complete
      acc.hc = sad_u8(prev[0], row[0], acc.hc);
      acc.hc = sad_u8(prev[1], row[1], acc.hc);
      if (EXCHANGE) acc.vc = sad_u8(acc.col7, right_of(s - 1u, acc.col0), acc.vc);  // sum_y |m(7, y) - m(8, y)|
      bool one_bpp;
      const uint32_t data = pvrtc_acc_finish(acc, &one_bpp);
      store(s - 1u, data, one_bpp, own);
    }
    if (s == k_blocks) break;
    own = own_next;
    acc.hc = acc.vc = acc.d1 = acc.d2 = 0;  // (u01 / u23 / col0 / col7 are overwritten piece by piece)
    pvrtc_acc_row<EXCHANGE>(acc, 0, row, right_mod);
    prev[0] = row[0]; prev[1] = row[1];
    ICAMD_UNROLL
    for (int c = 0; c < 3; ++c)
      ICAMD_UNROLL
      for (int v = 0; v < 4; ++v) V[c][v] += dV[c][v];
    ICAMD_SCHED_FENCE();
    // row 1 of block s, weight 3
    load_px(4u * s + 2u, buf0, &right0);
    ICAMD_SCHED_FENCE();
    pvrtc_row_mods_v<!EXCHANGE>(V, buf1, right1, row, &right_mod);
    acc.hc = sad_u8(prev[0], row[0], acc.hc);
    acc.hc = sad_u8(prev[1], row[1], acc.hc);
    pvrtc_acc_row<EXCHANGE>(acc, 1, row, right_mod);
    prev[0] = row[0]; prev[1] = row[1];
    ICAMD_SCHED_FENCE();
  }
}

}  // namespace icamd
#endif  // ICAMD_PVRTC_PAIR_H_
