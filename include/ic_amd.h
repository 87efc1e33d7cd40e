/* ic_amd.h -- C ABI of the MI355X (gfx950) texture block-encode backend.
 *
 * Drop-in boundary for the per-4x4-block encode path of google/image-compression:
 * these entry points are what a C FFI for `image_codec_compression::Compressor`
 * (reference image_compression/public/compressor.h:48-138) binds for the hot path,
 * and what our own C++ `DxtcCompressor / EtcCompressor / PvrtcCompressor` classes
 * (image-compression_amd/cxx/) call.  Plain pointers and sizes only; no C++ or
 * torch types cross this boundary.  INTEGRATION.md shows the reference-side binding.
 *
 * There is NO CPU fallback behind this ABI: every encode entry point runs the
 * hand-written HIP kernels on the current HIP device, and returns a negative
 * ICAMD_ERR_* (never silently a host result) when no device / kernel is available.
 */
#ifndef IC_AMD_H_
#define IC_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- enumerations (values match the reference's enums so they can be passed through) ---- */

/* Which reference Compressor subclass is being replaced. */
enum { ICAMD_COMPRESSOR_DXTC = 0,   /* public/dxtc_compressor.h:52-83  */
       ICAMD_COMPRESSOR_ETC = 1,    /* public/etc_compressor.h:53-109  */
       ICAMD_COMPRESSOR_PVRTC = 2 };/* public/pvrtc_compressor.h:71-104 */

/* CompressedImage::Format, public/compressed_image.h:35-40. */
enum { ICAMD_RGB = 0, ICAMD_BGR = 1, ICAMD_RGBA = 2, ICAMD_BGRA = 3 };

/* EtcCompressor::CompressionStrategy, public/etc_compressor.h:57-62. */
enum { ICAMD_ETC_SPLIT_HORIZONTALLY = 0, ICAMD_ETC_SPLIT_VERTICALLY = 1,
       ICAMD_ETC_SMALLER_ERROR = 2, ICAMD_ETC_HEURISTIC = 3 };

/* Block codec actually written (the reference derives it from compressor + format,
 * internal/dxtc_compressor.cc:741-749). */
enum { ICAMD_DXT1 = 0, ICAMD_DXT5 = 1, ICAMD_ETC1 = 2, ICAMD_PVRTC2 = 3,
       /* EXTENSION, PARITY UNPINNED: PVRTC1 4 bpp (4 x 4-pixel blocks, 64 bits each).  BASELINE.json's config 5 names it, the
        * reference only implements 2 bpp (public/pvrtc_compressor.h:15-18), so it is written from the reference's 2 bpp rules
        * (pvrtc_compressor.cc:111-349) with the block shape changed, and checked against oracle/ic_oracle.c's restatement of the
        * same rules and by decoding.  Accepted by icamd_encode_device (RGBA8, square power of two >= 8, no row padding:
        * size * size / 2 bytes per image, blocks in the 2 bpp Z order) and icamd_encoded_size only; under stream capture it needs a
        * caller workspace of icamd_pvrtc4_workspace_size bytes (icamd_pvrtc2_set_workspace). */
       ICAMD_PVRTC4 = 4,
       /* EXTENSION, PARITY PINNED through the reference's DXT5 alpha path: BC4 (RGTC1, one channel, 8 bytes per 4 x 4 block)
        * and BC5 (RGTC2, two channels, 16 bytes per block).  The reference has no BC4 / BC5 compressor; these are defined
        * through it:
        *   BC4 of channel c of an image = bytes 0..7 of every 16-byte block that the reference's DXT5 encoder
        *       (EncodeDxt5Block, dxtc.cc:516-528) writes for the RGBA image whose alpha is channel c -- same raster block
        *       order, same edge replication, same has_one_pixel rule (a block wholly right of AND below the image, i.e. only
        *       on a padded grid, gets alpha0 = alpha1 = its corner pixel and all codes 0);
        *   BC5 = BC4(R) followed by BC4(G) in each 16-byte block (the standard RGTC2 layout).
        * Decoding follows DecodeAlphaValues (dxtc.cc:195-217, truncating CombineUint8Fast interpolation) and the 3-bit code
        * order of DecodeDxt5Block (dxtc.cc:240-267).  Unsigned (UNORM) only; the channels are R and G.
        * Source channels read by icamd_encode_device: R = byte 0 (byte 2 when swap_rb and src_components >= 3), G = byte 1;
        * BC4 accepts src_components 1..4, BC5 2..4, swap_rb only with 3 or 4 (otherwise ICAMD_ERR_ARG).
        * icamd_decode_device writes R8 (BC4) or RG8 (BC5) rows and needs swap_rb = 0.  Reachable through icamd_encode_device,
        * icamd_encode_batch_sharded_device, icamd_decode_device, icamd_encoded_size, icamd_kernel_name and the container
        * functions only: no Compressor + format pair selects them. */
       ICAMD_BC4 = 5, ICAMD_BC5 = 6,
       /* Values 7..15 are unassigned and rejected by every entry point. */
       /* EXTENSION: ETC2 RGBA8 (COMPRESSED_RGBA8_ETC2_EAC), 16 bytes per 4 x 4 block in the raster block order of ETC1: the
        * 8-byte EAC alpha word, then the 8-byte colour word.
        *   Colour half, PARITY PINNED: bytes 8..15 of a block are exactly the 8 bytes icamd_encode_device(ICAMD_ETC1,
        *       etc_strategy, 4, swap_rb, ...) writes for it -- all four strategies, padded grids and image edges included (like
        *       ETC1 the encoder stores bytes 0..2 of a pixel as they lie in memory, whatever swap_rb).  Every such block is a valid
        *       ETC2 colour word: the ETC1 encoder only selects differential mode when both 5-bit bases lie in 0..31, so the
        *       overflow patterns of ETC2's T, H and planar modes never occur.
        *   Alpha half, PARITY UNPINNED (the reference has no EAC): byte 0 = base, byte 1 = multiplier << 4 | table, bytes 2..7 =
        *       sixteen 3-bit indices, big-endian, texel i = 4 x + y in bits 47 - 3 i .. 45 - 3 i.  The alpha of texel (x, y) is
        *       byte 3 of the RGBA texel the colour half is given for that position (same edge replication, same padded-grid
        *       fetch).  Decode (Khronos ETC2 / EAC): alpha = clamp(base + M[table][index] * multiplier, 0, 255) with the 16 x 8
        *       modifier table of the specification (csrc/etc2_block.h); multiplier 0 is legal on decode and gives base.
        *       Encode is a definition, not a heuristic: with lo / hi the smallest / largest of the 16 alphas,
        *       R = hi - lo and span[t] = M[t][7] - M[t][3], the candidates are, for every table t, the multipliers
        *       m in {m0 - 1, m0, m0 + 1} clamped to 1..15 with m0 = clamp((2 R + span[t]) / (2 span[t]), 1, 15), and for each m
        *       the bases b in {b0 - 1, b0, b0 + 1} clamped to 0..255 with b0 = (lo + hi + m + 1) >> 1; every texel takes the
        *       smallest index that minimises |clamp(b + M[t][k] m, 0, 255) - alpha|, sse is the sum of the squared minima, and
        *       the block is the candidate with the lexicographically smallest (sse, t, m, b).  Multiplier 0 is never written.
        * icamd_encode_device needs src_components == 4 (else ICAMD_ERR_ARG) and honours etc_strategy, grids, strides and batches
        * as for ETC1.  icamd_decode_device writes RGBA8 rows (swap_rb: stored R goes to the third byte, as for DXT5) and decodes
        * colour words in all five modes (individual, differential, T, H, planar: see ICAMD_ETC2_RGB8 below); the encoder
        * itself writes the two ETC1-compatible ones only.
        *   Colour half with planar, T and H words, opt-in: icamd_encode_etc2_colour_device(ICAMD_ETC2_RGBA8, ...,
        *       ICAMD_ETC2_COLOUR_PLANAR / _PLANAR_TH, ...) keeps bytes 0..7 and writes into bytes 8..15 what ICAMD_ETC2_RGB8 writes
        *       for the block of the same RGBA8 source (icamd_encode_device, or icamd_encode_etc2_device with ICAMD_ETC2_MODES_TH);
        *       stated in full at that function.  icamd_encode_device itself writes what is stated above.
        * icamd_measure_error_device compares all four channels.  Reachable through icamd_encode_device,
        * icamd_encode_batch_sharded_device, icamd_decode_device, icamd_measure_error_device, icamd_encoded_size,
        * icamd_kernel_name, icamd_metric_kernel_name and the container functions only: no Compressor + format pair selects it
        * (icamd_supports_format and the host-buffer entry points keep the reference's semantics, so icamd_measure_error does
        * not reach it), and the mip entry points answer ICAMD_ERR_ARG as they do for PVRTC.  Mip chains: reachable through
        * icamd_encode_etc2_mips_device, icamd_etc2_mip_chain_size, icamd_etc2_mip_workspace_size and icamd_etc2_mip_kernel_name. */
       ICAMD_ETC2_RGBA8 = 16,
       /* Value 17 is unassigned and rejected by every entry point. */
       /* EXTENSION: ETC2 RGB8 (COMPRESSED_RGB8_ETC2), 8 bytes per 4 x 4 block in the raster block order of ETC1: one ETC2
        * colour word.  Big-endian, bit 63 = top bit of byte 0; diff = bit 33.
        *   Decode, all five modes (Khronos ETC2).  diff = 0: individual, as ETC1.  Otherwise s_c = 5-bit base + sign-extended
        *       3-bit delta of byte c (R, G, B = bytes 0, 1, 2): s_R outside 0..31 selects T, else s_G outside H, else s_B outside
        *       planar, else differential as ETC1.  The two ETC1 modes decode exactly as ICAMD_ETC1 does (pinned to the reference).
        *       T: two 4-bit colours C1, C2 (expanded v * 17) and a distance d[di], d = 3, 6, 11, 16, 23, 32, 41, 64; paint colours
        *       C1, clamp(C2 + d), C2, clamp(C2 - d).  H: paint colours clamp(C1 + d), clamp(C1 - d), clamp(C2 + d), clamp(C2 - d),
        *       the lowest bit of di being (C1 >= C2 as R << 16 | G << 8 | B).  In both, texel (x, y) takes the paint colour
        *       bit(p) | bit(p + 16) << 1 of the low 32 bits, p = 4 x + y.  Planar: three colours O, H, V of 6 / 7 / 6 bits
        *       (expanded v << 2 | v >> 4 and v << 1 | v >> 6), texel (x, y) = clamp((x (H - O) + y (V - O) + 4 O + 2) >> 2, 0,
        *       255) per channel.  Field positions: csrc/etc2_colour_block.h.
        *   Encode, a definition and not a heuristic.  With px the sixteen texels the ETC1 block routine is handed
        *       for the block (same edge replication and padded-grid fetch; bytes 0..2 of a pixel as they lie in memory, whatever
        *       swap_rb):
        *       E = the 8 bytes icamd_encode_device(ICAMD_ETC1, etc_strategy, ...) writes for the block (PARITY PINNED through ETC1);
        *       P = the planar word of the least-squares plane: per channel S = Sum v, Sx = Sum (2 x - 3) v, Sy = Sum (2 y - 3) v,
        *       N_O = 5 S - 3 Sx - 3 Sy, N_H = 5 S + 5 Sx - 3 Sy, N_V = 5 S - 3 Sx + 5 Sy (80 times the plane at (0, 0), (4, 0),
        *       (0, 4)), and the n-bit code (6 for R and B, 7 for G) q = (2 clamp(N, 0, 20400) (2^n - 1) + 20400) / 40800,
        *       truncating; no refinement.  The ignored bits 63, 55, 47..45, 42 are set so that bytes 0 and 1 do not overflow and
        *       byte 2 does (bit 63 / 55 = the top bit of the byte's delta field; with b = BO bits 4..3 and t = BO bits 2..1, bits
        *       47..45 = 111 and bit 42 = 0 where b + t >= 4, else 000 and 1).
        *       The block is P if its squared error summed over the 16 texels and 3 channels is STRICTLY smaller than E's, else E
        *       byte for byte.  So the summed error never exceeds ETC1's, block by block.  T and H are decoded, never written.
        *   Encode with T and H, opt-in: icamd_encode_etc2_device(..., ICAMD_ETC2_MODES_TH, ...), a definition and not a heuristic
        *       (DESIGN.md 3.17).  icamd_encode_device itself writes what is stated above, for every etc_strategy.  With v_p the
        *       sixteen texels above (index p = 4 x + y), W the 8 bytes icamd_encode_device(ICAMD_ETC2_RGB8, etc_strategy, ...)
        *       writes for the block and err(W) its squared error summed over the 16 texels and 3 channels:
        *       Partitions of the texels into clusters A and B, two, tried in this order; one with A or B empty is dropped.
        *           L (luminance): Y_p = R + 2 G + B; p is in B iff 16 Y_p > Sum Y.
        *           C (widest channel): c* = the channel with the largest max - min over the block, ties to R before G before
        *           B; p is in B iff 2 v_p[c*] > max + min of that channel.
        *       Cluster colours: per cluster (n texels, channel sum S) and channel the 4-bit code q = (30 S + 255 n) / (510 n),
        *           truncating; the colour is 17 q.  a is A's colour, b is B's.  A partition whose two 12-bit codes are equal is
        *           dropped.
        *       Candidates of a partition, in this order, each with the distance index di = 0..7 ascending: T(C1 = a, C2 = b),
        *           T(C1 = b, C2 = a), H(a, b).  The paint colours are the decoder's (T: C1, clamp(C2 + d), C2, clamp(C2 - d); H:
        *           clamp(a +- d), clamp(b +- d)); the colours are not refined.  Every texel takes the paint with the smallest
        *           squared RGB distance, ties to the smallest paint index; the candidate's error is the sum over the texels.
        *       Choice: the best candidate has the smallest error, ties to the earliest in the order (partition L before C, then
        *           the candidate order, then di).  The block is the best candidate's word if its error is STRICTLY smaller than
        *           err(W), else W byte for byte; a block with no surviving partition is W.  So the summed error never exceeds
        *           icamd_encode_device's, block by block.
        *       Packing (fields: csrc/etc2_colour_block.h; bit 33 set).  T: di = bits 35-34 : 32; with a = R1 >> 2 and b = R1 & 3,
        *           bits 63-61 = 111 and bit 58 = 0 where a + b >= 4, else 000 and 1, so byte 0 overflows.  H: bit 34 = di >> 2,
        *           bit 32 = (di >> 1) & 1, and where (C1 >= C2 as R << 16 | G << 8 | B) != (di & 1) for (C1, C2) = (a, b) the
        *           colours are stored swapped and every texel's index flipped by k ^= 2; bit 63 = G1 bit 3, so byte 0 does not
        *           overflow; with a' = (G1 & 1) << 1 | B1 >> 3 and b' = (B1 >> 1) & 3, bits 55-53 = 111 and bit 50 = 0 where
        *           a' + b' >= 4, else 000 and 1, so byte 1 overflows.
        * icamd_encode_device takes src_components 3 or 4 and honours etc_strategy, grids, strides and batches as for ETC1.
        * icamd_decode_device writes RGB888 rows and, like ICAMD_ETC1, stores the word's channels in their stored order whatever
        * swap_rb.  icamd_measure_error_device compares three channels, sources of 3 or 4 components.  Reachable through
        * icamd_encode_device, icamd_encode_batch_sharded_device, icamd_decode_device, icamd_measure_error_device,
        * icamd_encoded_size, icamd_kernel_name, icamd_metric_kernel_name and the container functions (KTX 0x9274, PKM 2.0 type 1,
        * PVR 22; no DDS) only: no Compressor + format pair selects it, and the mip entry points answer ICAMD_ERR_ARG.  Mip chains
        * (with T and H too): reachable through icamd_encode_etc2_mips_device, icamd_etc2_mip_chain_size,
        * icamd_etc2_mip_workspace_size and icamd_etc2_mip_kernel_name. */
       ICAMD_ETC2_RGB8 = 18,
       /* EXTENSION: EAC R11 (COMPRESSED_R11_EAC, one channel, 8 bytes per 4 x 4 block) and EAC RG11 (COMPRESSED_RG11_EAC, two
        * channels, 16 bytes per block: the word of R, then the word of G), in the raster block order of ETC1.  Unsigned,
        * bytes in and out here; 16-bit samples and the signed formats: icamd_encode_eac11_16_device below.
        * They are to the ETC2 family what BC4 / BC5 are to DXT.  A word has the layout of the ETC2 RGBA8 alpha word: byte 0 =
        * base, byte 1 = multiplier << 4 | table, then sixteen 3-bit indices, big-endian, texel i = 4 x + y in bits
        * 47 - 3 i .. 45 - 3 i.
        *   Decode (Khronos EAC, 11-bit): v11 = clamp(8 base + 4 + M[table][index] * (multiplier == 0 ? 1 : 8 multiplier), 0,
        *       2047) with the modifier table of ICAMD_ETC2_RGBA8.  icamd_decode_device writes R8 (R11) or RG8 (RG11) rows of
        *       width * 1 / width * 2 + padding bytes, as the BC4 / BC5 decoders do, and needs swap_rb = 0 (else ICAMD_ERR_ARG).
        *       The byte written is v11 >> 3, the top byte of the specification's 16-bit expansion v11 << 5 | v11 >> 6.  For a
        *       multiplier of 1 or more that is clamp(base + M multiplier, 0, 255), exactly the alpha decoder's byte (8 x + 4
        *       clamped to 0..2047 and shifted is x clamped to 0..255).  For multiplier 0 it is not: the word
        *       80 0d 7e 49 24 92 49 24 (base 128, multiplier 0, table 13, indices 3, 7, 4, 4, ...) gives v11 = 1018, 1037, 1028,
        *       ... and the bytes 127, 129, 128, ..., where the alpha decoder gives 128 everywhere.  Base 255, multiplier 0,
        *       table 0, index 7 clamps to 2047 -> 255; base 0, multiplier 0, table 0, index 3 clamps to 0.
        *   Encode, a definition, PARITY PINNED through ICAMD_ETC2_RGBA8's alpha half: R11 of channel c of an image is bytes 0..7
        *       of every block that icamd_encode_device(ICAMD_ETC2_RGBA8, ...) writes for the RGBA image whose alpha is channel c
        *       -- the 144-candidate search stated there, the same clamp-to-edge replication and padded-grid fetch (no BC4-style
        *       one-pixel rule), smallest (sse, table, multiplier, base), smallest index at each texel's minimum; multiplier 0 is
        *       never written.  RG11 = R11(R) followed by R11(G).
        * Source channels read by icamd_encode_device follow the ICAMD_BC4 rules: R = byte 0 (byte 2 when swap_rb and
        * src_components >= 3), G = byte 1; R11 accepts src_components 1..4, RG11 2..4, swap_rb only with 3 or 4 (otherwise
        * ICAMD_ERR_ARG); etc_strategy is ignored.  icamd_measure_error_device compares k = 0 (R11) or k = 0, 1 (RG11) against the
        * decoder's byte.  Reachable through icamd_encode_device, icamd_encode_batch_sharded_device, icamd_decode_device,
        * icamd_measure_error_device, icamd_encoded_size, icamd_kernel_name, icamd_metric_kernel_name and the container functions
        * (KTX 0x9270 / 0x9272, PKM 2.0 types 5 / 6, PVR 25 / 26; no DDS) only: no Compressor + format pair selects them, the mip
        * entry points answer ICAMD_ERR_ARG and icamd_mip_chain_size 0.  Mip chains: reachable through
        * icamd_encode_etc2_mips_device, icamd_etc2_mip_chain_size, icamd_etc2_mip_workspace_size and icamd_etc2_mip_kernel_name. */
       ICAMD_EAC_R11 = 19, ICAMD_EAC_RG11 = 20,
       /* EXTENSION: ETC2 RGB8 with punch-through alpha (COMPRESSED_RGB8_PUNCHTHROUGH_ALPHA1_ETC2), 8 bytes per 4 x 4 block in the
        * raster block order of ETC1.  PARITY UNPINNED (the reference has no such format) except where stated.
        *   The word is big-endian; hi = bits 63..32, lo = bits 31..0.  The field positions are those of ICAMD_ETC2_RGB8
        *       (csrc/etc2_colour_block.h), with bit 33 the OPAQUE bit Op instead of the diff bit.
        *   Mode.  There is no individual mode.  For byte c (R, G, B = bytes 0, 1, 2) s_c = 5-bit base + sign-extended 3-bit
        *       delta, whatever Op: s_R outside 0..31 selects T, else s_G outside H, else s_B outside planar, else differential.
        *   Differential.  Bases, flip (bit 32), the two 3-bit table fields and the texel index k = bit(p) | bit(p + 16) << 1 of
        *       lo, p = 4 x + y, as in ETC1.  Op = 1: texel = clamp(base + {+a, +b, -a, -b}[k]), alpha 255 -- exactly an ETC1
        *       differential word.  Op = 0: the modifiers are {0, +b, -, -b}; k = 2 is a transparent texel, R = G = B = A = 0; every
        *       other texel has alpha 255.  a, b = 2, 5, 9, 13, 18, 24, 33, 47 and 8, 17, 29, 42, 60, 80, 106, 183 by table.
        *   T and H.  The paint colours of ICAMD_ETC2_RGB8; with Op = 0, k = 2 gives (0, 0, 0, 0) instead of paint 2.  The last bit
        *       of the H distance index is derived as there.
        *   Planar.  As ICAMD_ETC2_RGB8; alpha is 255 for every texel, whatever Op.
        *   Known answers: 00 00 00 00 ff ff 00 00 decodes to sixteen (0, 0, 0, 0).  1c 00 00 f4 ff 00 f0 f0 is T with Op = 0,
        *       C1 = (204, 0, 0), C2 = (0, 0, 255), d = 11: column x = 0 is (204, 0, 0, 255), x = 1 (11, 11, 255, 255), x = 2
        *       (0, 0, 0, 0), x = 3 (0, 0, 244, 255); with byte 3 = f6 (Op = 1) column 2 is (0, 0, 255, 255).
        *       60 90 c8 00 ff 00 00 00 gives (99, 148, 206, 255) in columns 0 and 1 and (0, 0, 0, 0) in columns 2 and 3.
        *   Encode, a definition and not a heuristic.  src_components == 4 only (else ICAMD_ERR_ARG).  The sixteen
        *       texels are the ones ICAMD_ETC2_RGBA8 is handed for the block (same edge replication and padded-grid fetch, bytes
        *       0..2 as they lie in memory whatever swap_rb).  A texel is TRANSPARENT iff its byte 3 is < 128.
        *       1. All 16 transparent: the word is 00 00 00 00 ff ff 00 00.
        *       2. None transparent: E = the 8 bytes icamd_encode_device(ICAMD_ETC1, etc_strategy, ...) writes for the block
        *          (PARITY PINNED through ETC1); C = E if E is differential (bit 33 set), else C = D(texels, no mask, Op = 1,
        *          partition = E's flip bit); the block is the least-squares planar word of ICAMD_ETC2_RGB8 where its summed squared
        *          error is STRICTLY smaller than C's, else C.  So wherever E is differential the block is byte for byte what
        *          ICAMD_ETC2_RGB8 writes.
        *       3. 1..15 transparent: the word is D(texels, mask, Op = 0, partitions by strategy): ICAMD_ETC_SPLIT_HORIZONTALLY flip
        *          1 only, ICAMD_ETC_SPLIT_VERTICALLY flip 0 only, the other two both, the smaller error wins and a tie keeps
        *          flip 0.  No planar candidate.
        *       D, the masked differential search, on the ETC1 sub-blocks (flip 0: S0 = columns 0..1, S1 = columns 2..3; flip 1:
        *       rows).  Per partition -- bases: n = the sub-block's opaque texels, per channel q5 = floor(sum over them / (8 n))
        *       (n = 8: ETC1's sum >> 6); a sub-block with n = 0 takes the other's q5.  Delta, per channel: d = q5(S1) - q5(S0),
        *       c = clamp(d, -4, 3), e = d - c, a' = q5(S0) + e / 2 (truncating toward zero), b' = a' + c; the word stores a' and c,
        *       the decoded bases are v << 3 | v >> 2 (both lie between the two q5, so no channel overflows).  Tables and indices:
        *       per sub-block and table t = 0..7 every opaque texel takes the allowed index (Op = 1: 0..3; Op = 0: 0, 1, 3) with
        *       the smallest squared RGB distance to clamp(base + modifier), ties to the smallest index; transparent texels take
        *       index 2 and add no error; the table is the t with the smallest error, ties to the smallest t (so n = 0: table 0).
        *       The partition's error is the sum of its two sub-blocks'.
        *       Example: every texel (100, 150, 200), alpha 255 for x < 2 and 0 for x >= 2: 60 90 c8 00 ff 00 00 00 for strategies
        *       1, 2, 3 (q5 = 12, 18, 25, every opaque texel index 0 at error 41, the partitions tie at 328), 60 90 c8 01 ff 00 00 00
        *       for strategy 0.  T and H are decoded, never written; a fully opaque block never gets Op = 0, and no block gets a
        *       transparent texel it did not have.
        *   Encode with T and H, opt-in: icamd_encode_etc2_colour_device(ICAMD_ETC2_RGB8A1, ..., ICAMD_ETC2_COLOUR_PLANAR_TH, ...)
        *       replaces the word W above where a T or H word is STRICTLY closer over the block's opaque texels: the search of
        *       ICAMD_ETC2_RGB8 on fully opaque blocks, a masked search with paints {0, 1, 3} on blocks with 1..15 transparent
        *       texels (a definition, stated in full at that function; csrc/etc2_a1_th_block.h); all-transparent blocks stay.
        * icamd_decode_device writes RGBA8 rows (swap_rb as for ICAMD_ETC2_RGBA8) and reads all four modes under both values of Op.
        * icamd_measure_error_device takes src_components == 4 and compares all four decoded channels against the source, as
        * ICAMD_ETC2_RGBA8 does -- so colour stored under a transparent texel counts against decoded 0, and a source alpha that is
        * not 0 / 255 counts against 0 / 255.  Reachable through icamd_encode_device, icamd_encode_batch_sharded_device,
        * icamd_decode_device, icamd_measure_error_device, icamd_encoded_size, icamd_kernel_name, icamd_metric_kernel_name and the
        * container functions (KTX 0x9276 with GL_RGBA, PKM 2.0 type 4, PVR 24; no DDS) only: no Compressor + format pair selects
        * it, the mip entry points answer ICAMD_ERR_ARG and icamd_mip_chain_size 0.  Mip chains: reachable through
        * icamd_encode_etc2_mips_device, icamd_etc2_mip_chain_size, icamd_etc2_mip_workspace_size and icamd_etc2_mip_kernel_name. */
       ICAMD_ETC2_RGB8A1 = 21,
       /* EXTENSION: signed EAC R11 (COMPRESSED_SIGNED_R11_EAC, 8 bytes per 4 x 4 block) and signed EAC RG11
        * (COMPRESSED_SIGNED_RG11_EAC, 16 bytes per block: the word of R, then the word of G).  The word layout is that of
        * ICAMD_EAC_R11, with byte 0 a two's-complement base.  PARITY UNPINNED (the reference has no EAC).  Signed data is 16-bit in
        * and out only: the codecs are reachable through icamd_encode_eac11_16_device, icamd_decode_eac11_16_device,
        * icamd_measure_error_eac11_16_device (where decoding and the encoder's search are stated in full),
        * icamd_eac11_16_kernel_name, icamd_eac11_16_metric_kernel_name, icamd_encoded_size and the container functions (KTX
        * 0x9271 with GL_RED / 0x9273 with GL_RG, PKM 2.0 types 7 / 8, PVR formats 25 / 26 with the header's channel-type field
        * = 1, signed byte normalised; no DDS).  Every other entry point refuses them as it refuses an unknown codec.
        * Values 22 and 23 are unassigned. */
       ICAMD_EAC_SIGNED_R11 = 24, ICAMD_EAC_SIGNED_RG11 = 25,
       /* EXTENSION: BC7 (BPTC, COMPRESSED_RGBA_BPTC_UNORM, DXGI_FORMAT_BC7_UNORM = 98): 16 bytes per 4 x 4 block, blocks in raster
        * order as DXT.  PARITY UNPINNED (the reference has no BC7).  Values 26..31 are unassigned.
        *   Decode (icamd_decode_device, RGBA8 rows, padding / batches / strides / swap_rb as ICAMD_DXT5): all eight modes of the
        *       BPTC specification -- both partition tables, the anchor tables, unique and shared p-bits, endpoint expansion
        *       (v << (8 - bits) | v >> (2 bits - 8)), the 2 / 3 / 4-bit weights {0,21,43,64}, {0,9,18,27,37,46,55,64},
        *       {0,4,9,13,17,21,26,30,34,38,43,47,51,55,60,64} with ((64 - w) e0 + w e1 + 32) >> 6, rotation and index selection of
        *       modes 4 / 5, alpha 255 in modes 0-3.  Texel i = 4 y + x.  A block whose byte 0 is 0 (reserved) decodes to sixteen
        *       (0, 0, 0, 0) texels.
        *   Metric (icamd_measure_error_device, src_components 3 or 4): the decoder's texels against the source, four channels
        *       for RGBA8 sources, R, G, B for RGB888 sources; records, padded grids and batches as ICAMD_DXT5.
        *   Encode (icamd_encode_device; src_components 3 or 4, else ICAMD_ERR_ARG; etc_strategy is not read): a DEFINITION that
        *       writes MODE 6 only (one subset, 7-bit endpoints + one p-bit each, 4-bit indices).  The sixteen texels
        *       v_p = (R, G, B, A), p = 4 y + x, are those ICAMD_DXT5's block routine is handed (clamp-to-edge replication, the
        *       same fetch for blocks of a padded grid; swap_rb exchanges bytes 0 and 2); A = 255 for 3-component sources.
        *       w_k, k = 0..15, are the 4-bit weights above.
        *       1. Targets.  Per channel lo_c = min_p v_p[c], hi_c = max_p v_p[c]; c* = the channel with the largest hi - lo
        *          (ties: R before G before B before A); T0 = lo, T1 = hi; for every c != c*, with
        *          cov_c = 16 sum_p v_p[c*] v_p[c] - (sum_p v_p[c*]) (sum_p v_p[c]): T0_c and T1_c are exchanged if cov_c < 0.
        *       2. Quantising an endpoint T -> E.  For p in {0, 1}: q_c(p) = clamp((T_c - p + 1) >> 1, 0, 127),
        *          err(p) = sum_c (2 q_c(p) + p - T_c)^2; p = the one with the smaller err (ties: 0), shared by the four channels;
        *          E_c = 2 q_c(p) + p.  E0 = Q(T0), E1 = Q(T1).
        *       3. Indices.  pal_k[c] = ((64 - w_k) E0[c] + w_k E1[c] + 32) >> 6; texel p takes the smallest k that minimises
        *          sum_c (pal_k[c] - v_p[c])^2; sse = the sum of the sixteen minima.
        *       4. One least-squares refit.  With w = w_{k_p} of step 3: a = sum (64 - w)^2, b = sum (64 - w) w, c = sum w^2,
        *          per channel X = sum (64 - w) v_p, Y = sum w v_p, det = a c - b^2.  If det = 0 there is no refit.  Otherwise
        *          T0'_c = clamp(rdiv(64 (c X - b Y), det), 0, 255), T1'_c = clamp(rdiv(64 (a Y - b X), det), 0, 255) with
        *          rdiv(n, d) = floor((2 n + d) / (2 d)) (exact integers: the products need 64 bits); steps 2 and 3 run on T', and
        *          their (E0, E1, k, sse) replace the first pass's only if the new sse is STRICTLY smaller -- so no block's error
        *          exceeds its first pass's.
        *       5. Anchor.  If k_0 >= 8: E0 and E1 are exchanged (their p-bits with them) and every k becomes 15 - k (the weights
        *          are symmetric, w_{15-k} = 64 - w_k: the decoded texels do not change).
        *       6. Pack, least significant bit first: bits 0..5 = 0, bit 6 = 1; R0, R1, G0, G1, B0, B1, A0, A1 (q, 7 bits each);
        *          P0, P1; k_0 in 3 bits; k_1..k_15 in 4 bits each.
        *       Example: sixteen texels (10, 20, 30, 255) give c0 42 41 a1 78 3c fe 7f 00 .. 00 (T0 = T1 = v; p = 0 at err 1
        *       against p = 1 at err 3; every k = 0; a = 65536, b = c = 0: det = 0).
        * Reachable through icamd_encode_device, icamd_encode_batch_sharded_device, icamd_decode_device,
        * icamd_measure_error_device, icamd_encoded_size, icamd_kernel_name, icamd_metric_kernel_name and the container functions
        * (DDS with the DX10 extension header, dxgiFormat 98; KTX 0x8E8C with GL_RGBA; PVR 15; no PKM) only: no Compressor + format
        * pair selects it; the mip, ETC2-specific and 16-bit EAC entry points answer as for an unknown codec. */
       ICAMD_BC7 = 32,
       /* EXTENSION: BC6H (BPTC float; DXGI_FORMAT_BC6H_UF16 = 95 / _SF16 = 96, COMPRESSED_RGB_BPTC_UNSIGNED_FLOAT 0x8E8F /
        * _SIGNED_FLOAT 0x8E8E): 16 bytes per 4 x 4 block of RGB halves, blocks in raster order as DXT.  PARITY UNPINNED (the
        * reference has no BC6H).  Value 33 is unassigned.  Half floats in and out only: the codecs are reachable through
        * icamd_encode_bc6h_device, icamd_decode_bc6h_device, icamd_measure_error_bc6h_device (where the format, the encoder's
        * definition and the metric are stated in full), icamd_bc6h_kernel_name, icamd_bc6h_metric_kernel_name, icamd_encoded_size
        * and the container functions (DDS with the DX10 extension header, dxgiFormat 95 / 96; KTX 0x8E8F / 0x8E8E with GL_RGB; no
        * PKM, no PVR).  Every other entry point refuses them as it refuses an unknown codec. */
       ICAMD_BC6H_UF16 = 34, ICAMD_BC6H_SF16 = 35,
       /* EXTENSIONS: BC1 with punch-through alpha ("DXT1A", COMPRESSED_RGBA_S3TC_DXT1_EXT; ICAMD_BC1A, 8 bytes per 4 x 4 block) and
        * BC2 ("DXT3", COMPRESSED_RGBA_S3TC_DXT3_EXT; ICAMD_BC2, 16 bytes per block: the alpha word, then the colour word).  Blocks in
        * raster order.  Values 38 and up are unassigned.  ICAMD_DXT1 and ICAMD_DXT5 are unchanged: they write and decode the bytes
        * they always did.
        *   Common rules.  src_components == 4 only (anything else: ICAMD_ERR_ARG); etc_strategy is ignored, as for DXT.  Grids, row
        *       strides, image strides, batches, padded grids and edge replication as for ICAMD_DXT5: a block's sixteen texels are
        *       the ones ICAMD_DXT5 is handed for it.  Texel p = 4 y + x; its 2-bit colour index is at bits 2p..2p+1 of the
        *       little-endian index dword.  Canonical colour: R = byte 0 (byte 2 when swap_rb), G = byte 1, B the remaining byte.
        *   Decode (icamd_decode_device, RGBA8 rows; with swap_rb the stored R goes to the third byte, as for ICAMD_DXT5): the
        *       formats' own rules.  E0, E1 = the 565 colours c0, c1 widened by bit replication; blends per channel, truncating.
        *       BC1A: c0 > c1: palette E0, E1, (2 E0 + E1) / 3, (E0 + 2 E1) / 3, alpha 255.  Otherwise -- c0 == c1 included --
        *       E0, E1, (E0 + E1) / 2 with alpha 255, and index 3 is (0, 0, 0, 0).  (ICAMD_DXT1's decoder keeps the reference's
        *       c0 == c1 rule and opaque black for index 3; it has no alpha channel.)
        *       BC2: the colour word ALWAYS decodes in four-colour mode, whatever the order of c0 and c1; the alpha of texel p is
        *       nibble p of the little-endian 64-bit alpha word (bits 4p..4p+3) times 17.
        *   Encode, BC1A: a DEFINITION, not a heuristic.  A texel is TRANSPARENT iff its byte 3 is < 128, the rule
        *       of ICAMD_ETC2_RGB8A1.
        *       1. All 16 transparent: the block is 00 00 00 00 ff ff ff ff.
        *       2. None transparent: the 8 bytes icamd_encode_device(ICAMD_DXT1, ..., 4, swap_rb, ...) writes for the block (PARITY
        *          PINNED through ICAMD_DXT1).  Under the BC1A decoder every such block is fully opaque and decodes to the RGB it
        *          has under the DXT1 decoder: the general path stores c0 > c1, the constant-colour path stores equal endpoints
        *          only with index 0 and index 3 only with c0 > c1 (checked over all 2^24 colours against the constant table).
        *       3. 1..15 transparent: three-colour mode.  Over the OPAQUE texels only, L = 4 R + 8 G + B on the canonical channels;
        *          lo = the first opaque texel in raster order with the smallest L, hi = the first with the largest L (the DXT1
        *          encoder's tie rules with the transparent texels left out); a = Quantize565(lo), b = Quantize565(hi) on canonical
        *          R, G, B (Quantize8: i = v (2^n - 1) + 128, (i + (i >> 8)) >> 8); stored c0 = min(a, b), c1 = max(a, b) as
        *          16-bit values -- they may be equal.  Palette: the decoder's, P0 = E(c0), P1 = E(c1), P2 = (P0 + P1) >> 1 per
        *          channel.  An opaque texel takes the k in {0, 1, 2} with the smallest squared RGB distance to its canonical
        *          colour, ties to the smallest k; a transparent texel takes 3, and the colour stored under it plays no part
        *          anywhere.  No constant-colour table refinement and no refit in this path.
        *       Examples.  Every texel (100, 150, 200), alpha 255 for x < 2 and 0 for x >= 2: b8 64 b8 64 f0 f0 f0 f0; columns 0 and
        *       1 decode to (99, 150, 198, 255), columns 2 and 3 to (0, 0, 0, 0).  Every texel (200, 100, 50, 255) except texel 0 =
        *       (10, 20, 30, 255), texel 5 = (105, 60, 40, 200) and texel 15 with alpha 127: a4 08 26 c3 54 59 55 d5; texel 0
        *       decodes to (8, 20, 33, 255), texel 1 to (198, 101, 49, 255), texel 5 to (103, 60, 41, 255), texel 15 to (0, 0, 0, 0).
        *       So no texel gains or loses transparency, and a fully opaque image encodes to exactly the ICAMD_DXT1 stream.
        *   Encode, BC2: bytes 8..15 are bytes 8..15 of the block icamd_encode_device(ICAMD_DXT5, ...) writes (the always-four-colour
        *       colour block, PARITY PINNED through ICAMD_DXT5).  Bytes 0..7 are the alpha word: nibble p = Quantize8(alpha_p, 15),
        *       i = 15 a + 128, (i + (i >> 8)) >> 8 -- so 0 -> 0, 127 -> 7, 128 -> 8, 200 -> 12, 255 -> 15.  No has_one_pixel
        *       special case: the gathered texels of such a block are all the corner pixel.
        *   Metric (icamd_measure_error_device, src_components == 4): all four decoded channels against the source with the
        *       decoders' own math, as ICAMD_ETC2_RGB8A1 and ICAMD_DXT5 -- so colour under a transparent texel counts against 0, and
        *       a source alpha that is not 0 / 255 counts against 0 / 255 for BC1A and against nibble x 17 for BC2.
        * Reachable through icamd_encode_device, icamd_encode_batch_sharded_device, icamd_decode_device,
        * icamd_measure_error_device, icamd_encoded_size, icamd_kernel_name, icamd_metric_kernel_name and the container functions
        * (BC1A: DDS FourCC DXT1 with ddspf.dwFlags = DDPF_FOURCC | DDPF_ALPHAPIXELS = 0x5, the only difference from ICAMD_DXT1's
        * header; KTX 0x83F1 with GL_RGBA; PVR 7 -- PVR has one DXT1 code.  BC2: DDS FourCC DXT3; KTX 0x83F2 with GL_RGBA; PVR 9.
        * No PKM) only: no Compressor + format pair selects them; every other family's entry points refuse them as they refuse an
        * unknown codec, and icamd_mip_chain_size answers 0. */
       ICAMD_BC1A = 36, ICAMD_BC2 = 37 };

/* Status codes.  0 = the reference's `true`; 1 = the reference's `false` (argument
 * validation, unsupported format, external-storage size mismatch); < 0 = the device
 * path could not run -- callers must treat that as a hard error. */
enum { ICAMD_OK = 0, ICAMD_FALSE = 1,
       ICAMD_ERR_NO_DEVICE = -1, ICAMD_ERR_HIP = -2, ICAMD_ERR_ALLOC = -3, ICAMD_ERR_ARG = -4 };

/* ---- size / capability queries (host only, no device needed) ---- */

/* Compressor::ComputeCompressedDataSize -- compressor.h:68-69; semantics of
 * dxtc_compressor.cc:725-733, etc_compressor.cc:734-745, pvrtc_compressor.cc:631-634. */
size_t icamd_compute_compressed_data_size(int compressor, int format, uint32_t height, uint32_t width);

/* Compressor::SupportsFormat -- compressor.h:54; dxtc.cc:700-703 (all four),
 * etc.cc:713-717 (kRGB only), pvrtc.cc:607-609 (kRGBA only). */
int icamd_supports_format(int compressor, int format);

/* Bytes written by icamd_encode_device for one image of that block grid. */
size_t icamd_encoded_size(int codec, uint32_t grid_height, uint32_t grid_width);

/* ---- the hot path, host buffers: exact drop-in for Compressor::Compress ----
 * compressor.h:77-80 (note (height, width) order).  `buffer` is `height` rows of
 * width*components + padding_bytes_per_row bytes of host memory; `out` is caller storage
 * of exactly out_size == icamd_compute_compressed_data_size(...) bytes (the reference's
 * external-storage contract, internal/compressor4x4_helper.cc:34-41).
 * Returns when `out` is filled.  Inside: DXT / ETC images are cut into bands of whole block rows whose H2D copy,
 * kernel and D2H copy are pipelined over two internal per-thread streams (bands are independent images: blocks are
 * row-major, compressor4x4_helper.h:202-214); PVRTC is staged whole.  Pageable caller buffers work as they are;
 * buffers page-locked with icamd_host_register (or hipHostMalloc) are DMA-ed at the PCIe rate. */
int icamd_compress(int compressor, int etc_strategy, int format,
                   uint32_t height, uint32_t width, uint32_t padding_bytes_per_row,
                   const uint8_t *buffer, uint8_t *out, size_t out_size);

/* Optional: page-lock a caller buffer that will be passed to icamd_compress / icamd_compress_and_pad repeatedly
 * (input images, output storage), so that the copies are true asynchronous DMA.  Thin wrappers over hipHostRegister /
 * hipHostUnregister; the caller unregisters before freeing the memory. */
int icamd_host_register(void *host_ptr, size_t bytes);
int icamd_host_unregister(void *host_ptr);

/* Compressor::CompressAndPad -- compressor.h:114-119; helper.h:479-520.
 * PVRTC returns ICAMD_FALSE like pvrtc_compressor.cc:684-691. */
int icamd_compress_and_pad(int compressor, int etc_strategy, int format,
                           uint32_t height, uint32_t width,
                           uint32_t padded_height, uint32_t padded_width,
                           uint32_t padding_bytes_per_row,
                           const uint8_t *buffer, uint8_t *out, size_t out_size);

/* Multi-GPU sharding of ONE PVRTC texture: encodes only the blocks whose Z-order index
 * (pvrtc_compressor.cc:80-86, :551-580) lies in [first_block, first_block + n_blocks) -- n_blocks a power of two,
 * first_block a multiple of it, i.e. a rectangle of the block grid and ONE contiguous 8*n_blocks-byte range of the
 * texture's output.  d_src is the whole size x size RGBA8 image (device); only the region's pixels and a one-block
 * toroidal ring around it are read (the neighbours' colours are recomputed locally: no exchange between ranks).
 * d_dst_region receives 8*n_blocks bytes.  ICAMD_FALSE where PvrtcCompressor::Compress would refuse the size. */
int icamd_pvrtc2_encode_region_device(uint32_t size, uint32_t first_block, uint32_t n_blocks, const void *d_src,
                                      void *d_dst_region, void *hip_stream);

/* PVRTC scratch memory.  The PVRTC encoder keeps 8 bytes per block (the reference's two low-resolution colour images,
 * pvrtc_compressor.cc:586-597) between its two kernels.  By default that lives in a per-thread, grow-only buffer the
 * library allocates, which cannot be used while the stream is being CAPTURED into a HIP graph (the graph would keep a
 * pointer that a later, larger call frees; a PVRTC call under capture then returns ICAMD_ERR_HIP).  To capture -- or to
 * control the memory -- hand the library a buffer of at least icamd_pvrtc2_workspace_size(size, n_images) bytes for the
 * calls that follow on THIS thread; the caller keeps it alive and exclusive for as long as work (or a graph) using it
 * can run, one per graph.  NULL returns to the internal buffer. */
size_t icamd_pvrtc2_workspace_size(uint32_t size, uint32_t n_images);
size_t icamd_pvrtc4_workspace_size(uint32_t size, uint32_t n_images); /* the same for ICAMD_PVRTC4 (extension) */
int icamd_pvrtc2_set_workspace(void *d_workspace, size_t bytes);

/* PVRTC kernel selection (EXTENSION, tuning / test hook; results are identical either way).  Whole textures of 512^2 ...
 * 4096^2 in launches large enough to fill the chip take the one-pass kernel (Morph, Modulate and Encode of
 * pvrtc_compressor.cc:586-597 in ONE read of the pixels, no scratch memory -- such launches can be captured into a HIP graph
 * without a caller-owned workspace).  Textures of 8192^2 and more, and regions (icamd_pvrtc2_encode_region_device) at least 64
 * block columns wide, take the same kernel in its HALO form where the time model prefers it (r06: a block row split over several
 * workgroups, each reducing the block columns beyond its edges itself -- still one launch and no scratch memory).  Everything
 * else takes the morph + encode pair.  mode 0 = automatic (default; also the
 * value of the environment variable ICAMD_PVRTC2_PATH=auto|two|one read at the first launch), 1 = always the pair, 2 = one pass
 * wherever eligible; log2_strip < 0 = automatic strip height (blocks per lane) of the one-pass kernel (2 ... 6), else that height, clamped to
 * 2 ... log2(size / 4) (the tallest strip is the whole texture: one workgroup per texture).
 * Process-wide.  Returns ICAMD_OK, or ICAMD_ERR_ARG for a mode outside 0 ... 2. */
int icamd_pvrtc2_tune(int mode, int log2_strip);

/* ---- the hot path, device-resident (the roofline entry points) ----
 * Same contracts, but `d_buffer` / `d_out` are device pointers on the current HIP
 * device and the work is enqueued on `hip_stream` (a hipStream_t, NULL = default
 * stream) without synchronising. */
int icamd_compress_device(int compressor, int etc_strategy, int format,
                          uint32_t height, uint32_t width, uint32_t padding_bytes_per_row,
                          const void *d_buffer, void *d_out, size_t out_size, void *hip_stream);

int icamd_compress_and_pad_device(int compressor, int etc_strategy, int format,
                                  uint32_t height, uint32_t width,
                                  uint32_t padded_height, uint32_t padded_width,
                                  uint32_t padding_bytes_per_row,
                                  const void *d_buffer, void *d_out, size_t out_size, void *hip_stream);

/* Generic block-grid encoder over a batch of equally-shaped images (one launch).
 *   codec            ICAMD_DXT1 / DXT5 / ETC1 / PVRTC2
 *   src_components   3 or 4 bytes per source pixel (BC4: 1..4, BC5: 2..4).  4 with DXT1/ETC1 is the
 *                    "RGBA8, alpha ignored" extension named by BASELINE.json; its result
 *                    is defined as the reference's output for the alpha-stripped image.
 *   swap_rb          source is B,G,R(,A) (NeedsRedAndBlueSwapped, compressed_image.h:202-204)
 *   grid_height/width  >= height/width: block grid to emit (CompressAndPad); pass the
 *                    image dims for plain Compress.
 *   row_stride_bytes distance between source rows; *_image_stride_bytes between images.
 * Image i is read at d_src + i*src_image_stride_bytes and its blocks written at
 * d_dst + i*dst_image_stride_bytes (row-major blocks; PVRTC: Z-order, pvrtc.cc:551-580).
 * Any uint32 geometry runs (grids, batches and strides beyond one launch's limits are chunked internally).
 * Alignment: DXT / ETC accept any pointers and strides; PVRTC reads 16 bytes at a time and requires d_src (and
 * src_image_stride_bytes) 16-byte aligned, d_dst (and dst_image_stride_bytes) 8-byte aligned, else ICAMD_ERR_ARG.
 * BC4 / BC5 (extension, see ICAMD_BC4): channels and argument rules at the codec enumeration; otherwise as DXT.
 * ETC2 RGBA8 (extension, see ICAMD_ETC2_RGBA8): src_components must be 4; otherwise as ETC1.
 * ETC2 RGB8 (extension, see ICAMD_ETC2_RGB8): src_components 3 or 4; as ETC1.
 * EAC R11 / RG11 (extension, see ICAMD_EAC_R11): channels and argument rules as BC4 / BC5; grids, strides and batches as ETC1.
 * ETC2 RGB8A1 (extension, see ICAMD_ETC2_RGB8A1): src_components must be 4; otherwise as ETC1. */
int icamd_encode_device(int codec, int etc_strategy, int src_components, int swap_rb,
                        uint32_t height, uint32_t width, uint32_t grid_height, uint32_t grid_width,
                        uint32_t row_stride_bytes, uint32_t n_images,
                        size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                        const void *d_src, void *d_dst, void *hip_stream);

/* EXTENSION: the ETC2 family's encoder with a choice of colour modes.  codec must be ICAMD_ETC2_RGB8 (ETC2 RGBA8's colour half and
 * ETC2 RGB8A1 are covered by icamd_encode_etc2_colour_device below; here they are ICAMD_ERR_ARG, like every other codec) and etc2_modes one of the two values below, else
 * ICAMD_ERR_ARG.  Every other argument means what it means to icamd_encode_device and is checked before any device work: a
 * null pointer or a zero height / width returns ICAMD_FALSE; then a codec, etc2_modes or src_components outside the above
 * ICAMD_ERR_ARG; then n_images == 0 ICAMD_OK; then a row stride shorter than a row ICAMD_ERR_ARG -- the order of
 * icamd_encode_device, so an empty batch with a short stride is ICAMD_OK in both.
 *   ICAMD_ETC2_MODES_DEFAULT  the call IS icamd_encode_device: the same kernels, byte for byte.
 *   ICAMD_ETC2_MODES_TH       after those kernels, a second launch on the same stream replaces every block for which the T / H
 *                             search defined at ICAMD_ETC2_RGB8 finds a strictly closer word; all other bytes stay as they are.
 * icamd_etc2_kernel_name names the kernel of that second launch ("" for combinations that have none); with
 * ICAMD_ETC2_MODES_DEFAULT it answers what icamd_kernel_name answers. */
enum { ICAMD_ETC2_MODES_DEFAULT = 0,   /* what icamd_encode_device writes */
       ICAMD_ETC2_MODES_TH = 1 };      /* + the T and H candidates */
int icamd_encode_etc2_device(int codec, int etc_strategy, int etc2_modes, int src_components, int swap_rb,
                             uint32_t height, uint32_t width, uint32_t grid_height, uint32_t grid_width,
                             uint32_t row_stride_bytes, uint32_t n_images,
                             size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                             const void *d_src, void *d_dst, void *hip_stream);
const char *icamd_etc2_kernel_name(int codec, int src_components, int etc2_modes);

/* EXTENSION: planar, T and H colour words for all three ETC2 colour codecs.  codec is ICAMD_ETC2_RGBA8,
 * ICAMD_ETC2_RGB8 or ICAMD_ETC2_RGB8A1; src_components 4 for ICAMD_ETC2_RGBA8 and ICAMD_ETC2_RGB8A1, 3 or 4 for ICAMD_ETC2_RGB8;
 * colour_modes one of the three values below.  Every other argument means what it means to icamd_encode_device.  Every argument
 * is checked before any device work, in the order of icamd_encode_etc2_device: a null pointer or a zero height / width returns
 * ICAMD_FALSE; then a codec, colour_modes or src_components outside the above ICAMD_ERR_ARG; then n_images == 0 ICAMD_OK; then a
 * row stride shorter than a row ICAMD_ERR_ARG.  icamd_encode_device, icamd_encode_etc2_device and icamd_encode_etc2_mips_device
 * write and refuse what they did before.  The output is defined through those entry points:
 *   ICAMD_ETC2_COLOUR_DEFAULT, any codec: the call IS icamd_encode_device -- the same kernels, the same bytes.
 *   ICAMD_ETC2_RGB8: PLANAR is icamd_encode_device; PLANAR_TH is icamd_encode_etc2_device(..., ICAMD_ETC2_MODES_TH, ...).
 *   ICAMD_ETC2_RGBA8: bytes 0..7 of every block (the EAC alpha word) are what icamd_encode_device(ICAMD_ETC2_RGBA8,
 *       etc_strategy, ...) writes.  PLANAR: bytes 8..15 are the 8 bytes icamd_encode_device(ICAMD_ETC2_RGB8, etc_strategy, 4,
 *       swap_rb, the same geometry) writes for that block of the same source; PLANAR_TH: the 8 bytes
 *       icamd_encode_etc2_device(ICAMD_ETC2_RGB8, etc_strategy, ICAMD_ETC2_MODES_TH, 4, ...) writes.  Alpha never enters the colour
 *       choice.
 *   ICAMD_ETC2_RGB8A1: PLANAR is icamd_encode_device (that encoder already takes the planar word on opaque blocks).  PLANAR_TH,
 *       with W the word icamd_encode_device(ICAMD_ETC2_RGB8A1, etc_strategy, ...) writes, by the block's class at
 *       ICAMD_ETC2_RGB8A1:
 *       1. All 16 texels transparent: W.
 *       2. None transparent: the T / H search of ICAMD_ETC2_RGB8 verbatim with this W in place of its W -- the winner's word
 *          (bit 33 set, so Op = 1) if its error is STRICTLY smaller than err(W), else W.
 *       3. 1..15 transparent: the masked T / H search, a definition and not a heuristic.  O = the opaque texels (byte 3 >= 128),
 *          n = |O|.
 *          Partitions of O into clusters A and B, tried in this order; one with A or B empty is dropped.
 *              L: Y_p = R + 2 G + B; p is in B iff n Y_p > Sum over O of Y.
 *              C: c* = the channel with the largest max - min over O, ties to R before G before B; p is in B iff
 *              2 v_p[c*] > max + min over O.
 *          Cluster colours: the rule of ICAMD_ETC2_RGB8 over the cluster's m texels, q = (30 S + 255 m) / (510 m) truncating,
 *              colour 17 q.  A partition whose two 12-bit codes are equal is dropped.
 *          Candidates of a partition, in this order, each with di = 0..7 ascending; the paints are the decoder's under Op = 0,
 *              where index 2 is the transparent texel.  T(C1 = a, C2 = b): {0: C1, 1: clamp(C2 + d), 3: clamp(C2 - d)};
 *              T(C1 = b, C2 = a): the same with the roles exchanged; H(a, b): the stored order is forced by di's lowest bit --
 *              (C1, C2) = (a, b) where (a >= b as R << 16 | G << 8 | B) == (di & 1), else (b, a) -- and the paints are
 *              {0: clamp(C1 + d), 1: clamp(C1 - d), 3: clamp(C2 - d)}; no index is flipped.
 *          Every opaque texel takes the allowed index (0, 1 or 3) with the smallest squared RGB distance, ties to the smallest
 *              index; transparent texels take index 2 and add no error.  The best candidate has the smallest error, ties to the
 *              earliest (L before C, then the candidate order, then di).  err(W) is W's squared RGB error over O only, W read
 *              by the ICAMD_ETC2_RGB8A1 decoder.  The block is the best candidate's word if its error is STRICTLY smaller than
 *              err(W), else W byte for byte -- also where no partition survives (always so for n = 1).
 *          Packing: that of the T / H words of ICAMD_ETC2_RGB8 with bit 33 clear.
 *       So no block gains or loses a transparent texel, and the summed error over the opaque texels never exceeds
 *       icamd_encode_device's, block by block.
 * Where new words are written (ICAMD_ETC2_RGBA8 PLANAR / PLANAR_TH, ICAMD_ETC2_RGB8A1 PLANAR_TH) a second launch on the same
 * stream follows the codec's own kernels and stores 8 bytes only where a block's colour word changes; all other bytes stay as the
 * first launch left them.  icamd_etc2_colour_kernel_name names the kernel of that launch; for the forwarding pairs it answers
 * what the entry point forwarded to answers (ICAMD_ETC2_COLOUR_DEFAULT: icamd_kernel_name), and "" for a refused combination.
 * Mip chains, the sharded batch entry, the transcodes and the C++ classes do not reach these modes. */
enum { ICAMD_ETC2_COLOUR_DEFAULT = 0,      /* what icamd_encode_device writes */
       ICAMD_ETC2_COLOUR_PLANAR = 1,       /* + the planar word */
       ICAMD_ETC2_COLOUR_PLANAR_TH = 2 };  /* + the T and H words */
int icamd_encode_etc2_colour_device(int codec, int etc_strategy, int colour_modes, int src_components, int swap_rb,
                                    uint32_t height, uint32_t width, uint32_t grid_height, uint32_t grid_width,
                                    uint32_t row_stride_bytes, uint32_t n_images,
                                    size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                                    const void *d_src, void *d_dst, void *hip_stream);
const char *icamd_etc2_colour_kernel_name(int codec, int src_components, int colour_modes);

/* EXTENSION: BC7 with a choice of modes.  The codec is ICAMD_BC7; bc7_modes is one of the two values below and
 * src_components 3 or 4; every other argument means what it means to icamd_encode_device(ICAMD_BC7, ...) (etc_strategy does not
 * exist here).  Every argument is checked before any device work, in the order of icamd_encode_etc2_device: a null pointer or a
 * zero height / width returns ICAMD_FALSE; then a bc7_modes or src_components outside the above ICAMD_ERR_ARG; then
 * n_images == 0 ICAMD_OK; then a row stride shorter than a row ICAMD_ERR_ARG.
 *   ICAMD_BC7_MODES_DEFAULT   the call IS icamd_encode_device(ICAMD_BC7, ...): the same kernels, the same launches, byte for byte.
 *   ICAMD_BC7_MODES_EXTENDED  ONE fused kernel in place of those: per block it computes the mode-6 block of ICAMD_BC7 and ONE
 *                             candidate, and writes the candidate iff it is STRICTLY closer.  A DEFINITION, not a heuristic:
 * Texels v_p, p = 4 y + x, are exactly those the mode-6 definition at ICAMD_BC7 is handed (edge replication, padded grids, swap_rb,
 * A = 255 for 3-component sources).  First the mode-6 block and its final sse (sse6), steps 1-5 at ICAMD_BC7, unchanged.
 *   Block class.  Opaque = all sixteen A = 255 (always so for 3-component sources): the mode-1 candidate.  Every other block: the
 *       mode-5 candidate.
 *   Endpoint grids.  A 7-bit value x decodes to e7(x) = (x << 1) | (x >> 6).  "Nearest to T" = the x of the allowed set that
 *       minimises |e7(x) - T|, ties to the smaller x.
 *   Sub-fit F(S, C, weights, Q) over a texel set S (not empty) and a channel set C = steps 1-4 at ICAMD_BC7 restricted to S and C:
 *       targets = the per-channel min / max over S; c* = the channel of C with the largest max - min, ties to the earlier
 *       channel; for every other channel c of C the targets are exchanged where
 *       |S| sum_S v[c*] v[c] - (sum_S v[c*]) (sum_S v[c]) < 0; the endpoint bytes E0, E1 come from the quantiser Q, which is
 *       handed the targets of BOTH endpoints; pal_k[c] = ((64 - w_k) E0[c] + w_k E1[c] + 32) >> 6 over the 2- or 3-bit weights
 *       at ICAMD_BC7, every texel of S takes the smallest k that minimises sum over C of (pal_k[c] - v_p[c])^2, and the sub-fit's
 *       sse is the sum of those minima over S; one least-squares refit with the formulas of step 4, every sum taken over S
 *       (a = sum_S (64 - w)^2, b = sum_S (64 - w) w, c = sum_S w^2, X = sum_S (64 - w) v, Y = sum_S w v); det = 0 means no refit;
 *       rdiv's result is clamped to 0..255; the refit is quantised by Q and searched again, and replaces the first pass only if
 *       the sub-fit's sse gets STRICTLY smaller.
 *   Mode 1 (opaque blocks).
 *       1. Partition.  For each of the 64 two-subset partitions s of the BPTC specification: n0, n1 = the subsets' texel
 *          counts, S0, S1 = the (R, G, B) vector sums over the subsets, N_s = n1 |S0|^2 + n0 |S1|^2, d_s = n0 n1.  s beats t
 *          iff N_s d_t > N_t d_s (exact integers; the products need 64 bits).  The best partition is taken, ties to the smaller
 *          s: the one with the smallest within-subset scatter.  ONE partition is fitted, not 64.
 *       2. Subset j = 0, 1 is fitted with F(subset j, {R, G, B}, the 3-bit weights, Q1).  Q1: for p in {0, 1}, every channel of
 *          both endpoints takes the nearest x with x & 1 = p; err(p) = the sum of the six (e7(x) - T)^2; the p with the smaller
 *          err wins, ties to 0.  Stored: q = x >> 1 per channel and endpoint, and the subset's one p.
 *       3. sse1 = the sum of the two sub-fits' sse (alpha decodes to 255 exactly and adds nothing).
 *       4. Anchors.  Subset 0's anchor is texel 0, subset 1's the specification's anchor of the partition.  Where an anchor's
 *          index is >= 4, that subset's endpoints are exchanged and its indices become 7 - k.
 *       5. Pack, least significant bit first: bit 0 = 0, bit 1 = 1; the partition (6 bits); R of (subset 0 E0, subset 0 E1,
 *          subset 1 E0, subset 1 E1), 6 bits each; G likewise; B likewise; p of subset 0, p of subset 1; the sixteen indices in
 *          texel order, 3 bits each, the two anchors' in 2 bits.
 *   Mode 5 (the other blocks), rotation 0 only (rotations 1-3 are decoded, never written).
 *       1. Colour: F(all sixteen texels, {R, G, B}, the 2-bit weights, Q5).  Q5: per channel and endpoint the nearest x of
 *          0..127; no p-bit.
 *       2. Alpha: F(all sixteen texels, {A}, the 2-bit weights, identity): the endpoints are the 8-bit targets themselves.  (One
 *          channel: c* = A and nothing is exchanged.)
 *       3. sse5 = the sum of the two.
 *       4. Anchor flips, applied to the colour indices and to the alpha indices separately: an index of texel 0 that is >= 2
 *          exchanges that plane's endpoints and turns its indices into 3 - k.
 *       5. Pack: bits 0..4 = 0, bit 5 = 1; rotation 00; R0 R1 G0 G1 B0 B1 (x, 7 bits each); A0 A1 (8 bits each); the colour
 *          indices (31 bits: texel 0 in 1 bit, the others 2 bits each); the alpha indices (31 bits likewise).
 *   Choice.  The candidate replaces the mode-6 block iff its sse is STRICTLY smaller than sse6; every sse is over the four
 *       channels.  So no block's error exceeds ICAMD_BC7_MODES_DEFAULT's.
 * icamd_bc7_kernel_name names the kernel that writes the final bytes under ICAMD_BC7_MODES_EXTENDED; under
 * ICAMD_BC7_MODES_DEFAULT it answers what icamd_kernel_name(ICAMD_BC7, ...) answers; "" outside the domain.
 * icamd_encode_device, the sharded batch entry, the mip entry points and every other export behave as before; they do not reach
 * ICAMD_BC7_MODES_EXTENDED. */
enum { ICAMD_BC7_MODES_DEFAULT = 0,    /* what icamd_encode_device writes: mode 6 */
       ICAMD_BC7_MODES_EXTENDED = 1 }; /* + a mode-1 candidate on opaque blocks, a mode-5 candidate on the others */
int icamd_encode_bc7_device(int bc7_modes, int src_components, int swap_rb, uint32_t height, uint32_t width,
                            uint32_t grid_height, uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                            size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                            const void *d_src, void *d_dst, void *hip_stream);
const char *icamd_bc7_kernel_name(int src_components, int bc7_modes);

/* ---- "next" row 8f.1: block decoders on device (Compressor::Decompress, compressor.h:85-86;
 * helper.h:218-262, dxtc.cc:167-267, etc.cc:198-289).  Writes height rows of
 * width*comps + padding_bytes_per_row bytes (comps = 4 for DXT5, PVRTC2 and PVRTC4, else 3).
 * codec ICAMD_PVRTC2 is an EXTENSION with PARITY UNPINNED: the reference has no PVRTC decoder
 * (PvrtcCompressor::Decompress returns false, pvrtc_compressor.cc:669-672, and so does icamd_decompress); this one is
 * written from the encoder's own rules (up-sampling pvrtc.cc:173-237, modulation :111-135, block layout :356-496,
 * Z order :80-86) and needs square power-of-two sizes and padding_bytes_per_row == 0.  codec ICAMD_PVRTC4 (r05) is the
 * decoder of the 4 bpp extension encoder, under the same conditions and as unpinned as that: 4 x 4 blocks, every pixel its
 * own 2-bit value (weights 0, 3, 5, 8; a block with colour-word bit 0 set -- the encoder never writes one -- takes PVRTC1's
 * punch-through weights 0, 4, 4, 8 with alpha 0 for value 2).  ICAMD_BC4 / ICAMD_BC5 (extension, see ICAMD_BC4) write
 * width*1 / width*2 bytes per row (R8 / RG8) plus the padding; swap_rb must be 0, else ICAMD_ERR_ARG.  ICAMD_ETC2_RGBA8 (extension)
 * writes width*4 bytes per row plus the padding, ICAMD_ETC2_RGB8 (extension) width*3 like ICAMD_ETC1 (and like it stores the
 * channels in their stored order whatever swap_rb); both decode all five ETC2 colour modes.  ICAMD_EAC_R11 / ICAMD_EAC_RG11
 * (extension) write R8 / RG8 rows under the BC4 / BC5 rules.  ICAMD_ETC2_RGB8A1 (extension) writes width*4 bytes per row plus the
 * padding, alpha 0 or 255, swap_rb as for ICAMD_ETC2_RGBA8. */
int icamd_decode_device(int codec, int swap_rb, uint32_t height, uint32_t width,
                        uint32_t padding_bytes_per_row, uint32_t n_images,
                        size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                        const void *d_blocks, void *d_pixels, void *hip_stream);

/* Host-buffer drop-in for Compressor::Decompress (compressor.h:85-86) on DXTC / ETC images: `blocks` holds
 * the block grid of an image whose metadata says (uncompressed_height, uncompressed_width,
 * padding_bytes_per_row); `out` receives height rows of width*comps + padding bytes (out_size must be
 * exactly that).  PVRTC returns ICAMD_FALSE (pvrtc_compressor.cc:669-672). */
int icamd_decompress(int compressor, int format, uint32_t height, uint32_t width, uint32_t padding_bytes_per_row,
                     const uint8_t *blocks, size_t blocks_size, uint8_t *out, size_t out_size);

/* EXTENSION (parity unpinned like icamd_decode_device(ICAMD_PVRTC2)): host-buffer PVRTC 2bpp decode of a size x size
 * texture into size*size*4 RGBA bytes.  icamd_decompress itself keeps answering ICAMD_FALSE for PVRTC, like
 * PvrtcCompressor::Decompress (pvrtc_compressor.cc:669-672); the C++ class of this repo only routes here when the
 * environment variable ICAMD_PVRTC_DECOMPRESS_EXTENSION=1 is set. */
int icamd_pvrtc2_decompress(uint32_t size, const uint8_t *blocks, size_t blocks_size, uint8_t *out, size_t out_size);

/* ---- "next" rows 8f.2-4: compressed-domain operations on one image's block grid ----
 * Compressor::Pad (compressor.h:104-106; helper.h:393-477; pad functors dxtc.cc:594-696, etc.cc:645-698) for the
 * case that really pads: the source grid covers (compressed_height, compressed_width) pixels, the result
 * (padded_height, padded_width); out_size must be the result's data size.  Device pointers of the block-domain
 * operations (pad, downsample: 4-byte; DXT1 -> ETC1 transcode: 8-byte; DXT5 -> ETC2 RGBA8 transcode: 16-byte; the ETC2-family
 * transcodes: their block size) must be aligned,
 * else ICAMD_ERR_ARG; the decoders accept
 * any pointer.  Returns ICAMD_FALSE for PVRTC and when a
 * padded dimension has fewer blocks than the source (the reference either just duplicates the image, which the caller
 * does itself, or overruns its buffer). */
int icamd_pad_device(int compressor, int etc_strategy, int format, uint32_t compressed_height, uint32_t compressed_width,
                     const void *d_blocks, uint32_t padded_height, uint32_t padded_width, void *d_out, size_t out_size,
                     void *hip_stream);
/* Extension (r05), like icamd_downsample_batch_device: n_images equally shaped grids padded in ONE launch (ETC1 with
 * kSplit* / kHeuristic: two -- the copy, then every image's border blocks together; kSmallerError: one, its pad blocks take
 * four lanes each in the first workgroups of the launch).  Image i at d_blocks + i * src_image_stride_bytes -> d_out + i * dst_image_stride_bytes (multiples of 4). */
int icamd_pad_batch_device(int compressor, int etc_strategy, int format, uint32_t compressed_height, uint32_t compressed_width,
                           uint32_t n_images, const void *d_blocks, size_t src_image_stride_bytes, uint32_t padded_height,
                           uint32_t padded_width, void *d_out, size_t dst_image_stride_bytes, size_t out_size_per_image,
                           void *hip_stream);
int icamd_pad(int compressor, int etc_strategy, int format, uint32_t compressed_height, uint32_t compressed_width,
              const uint8_t *blocks, uint32_t padded_height, uint32_t padded_width, uint8_t *out, size_t out_size);

/* Compressor::Downsample (compressor.h:95-96; helper.h:264-391,594-636): (uncompressed_height, uncompressed_width)
 * -> ((h+1)/2, (w+1)/2); decode, 2x2 average, re-encode per output block.  ICAMD_FALSE where the reference refuses
 * (odd block counts > 1, single block with a 3-pixel side, PVRTC). */
int icamd_downsample_device(int compressor, int etc_strategy, int format, uint32_t uncompressed_height,
                            uint32_t uncompressed_width, const void *d_blocks, void *d_out, size_t out_size,
                            void *hip_stream);
/* Extension: the same on n_images equally shaped block grids in ONE launch (image i at d_blocks + i * src_image_stride_bytes ->
 * d_out + i * dst_image_stride_bytes; strides multiples of 4).  One 4096^2 DXT1 level is 10 MB of traffic -- less than the
 * fixed cost of a launch is worth -- so a mip generator that halves many textures feeds them as a batch. */
int icamd_downsample_batch_device(int compressor, int etc_strategy, int format, uint32_t uncompressed_height,
                                  uint32_t uncompressed_width, uint32_t n_images, const void *d_blocks,
                                  size_t src_image_stride_bytes, void *d_out, size_t dst_image_stride_bytes,
                                  size_t out_size_per_image, void *hip_stream);
int icamd_downsample(int compressor, int etc_strategy, int format, uint32_t uncompressed_height,
                     uint32_t uncompressed_width, const uint8_t *blocks, uint8_t *out, size_t out_size);

/* Compressor::CreateSolidImage (compressor.h:124-127; helper.h:522-543; solid blocks dxtc_compressor.cc:42-49,77-82,
 * 820-839, etc_compressor.cc:595-617,802-812): the block grid of a height x width image of one colour.  `color` is a
 * HOST pointer to 3 (kRGB/kBGR) or 4 (kRGBA/kBGRA) bytes; out_size must be blocks * block size.  ICAMD_FALSE for PVRTC
 * (pvrtc_compressor.cc:693-698), for ETC formats other than kRGB, and on a size mismatch.  The _device form fills a
 * device-resident grid (one kernel, streaming stores); the host form replicates the block on the host like the reference
 * (byte shuffling: nothing to offload). */
int icamd_create_solid_device(int compressor, int format, uint32_t height, uint32_t width, const uint8_t *color,
                              void *d_out, size_t out_size, void *hip_stream);
/* Extension (r05): n_images grids in ONE launch, image i of colour colors[i * components .. ] (HOST pointer, n_images x 3 or 4
 * bytes) at d_out + i * dst_image_stride_bytes.  A 4096^2 DXT1 grid is 8 MiB: one fill per call is launch-bound. */
int icamd_create_solid_batch_device(int compressor, int format, uint32_t height, uint32_t width, uint32_t n_images,
                                    const uint8_t *colors, void *d_out, size_t dst_image_stride_bytes, size_t out_size_per_image,
                                    void *hip_stream);
int icamd_create_solid(int compressor, int format, uint32_t height, uint32_t width, const uint8_t *color, uint8_t *out,
                       size_t out_size);

/* Compressor::CopySubimage (compressor.h:133-136; helper.h:545-592): the blocks of the height x width window at
 * (start_row, start_column) of an image whose grid covers (compressed_height, compressed_width) pixels.  ICAMD_FALSE
 * unless all four are multiples of 4 and the window lies inside the compressed image (helper.h:555-563), for PVRTC, and
 * on a size mismatch. */
int icamd_copy_subimage_device(int compressor, int format, uint32_t compressed_height, uint32_t compressed_width,
                               const void *d_blocks, uint32_t start_row, uint32_t start_column, uint32_t height,
                               uint32_t width, void *d_out, size_t out_size, void *hip_stream);
/* Extension (r05): the same window of n_images equally shaped grids in ONE launch (strides multiples of 4). */
int icamd_copy_subimage_batch_device(int compressor, int format, uint32_t compressed_height, uint32_t compressed_width,
                                     uint32_t n_images, const void *d_blocks, size_t src_image_stride_bytes, uint32_t start_row,
                                     uint32_t start_column, uint32_t height, uint32_t width, void *d_out,
                                     size_t dst_image_stride_bytes, size_t out_size_per_image, void *hip_stream);
int icamd_copy_subimage(int compressor, int format, uint32_t compressed_height, uint32_t compressed_width,
                        const uint8_t *blocks, uint32_t start_row, uint32_t start_column, uint32_t height,
                        uint32_t width, uint8_t *out, size_t out_size);

/* TranscodeDxt1ToEtc1 (public/dxtc_to_etc_transcoder.h:24; dxtc_to_etc_transcoder.cc:29-40): in place. */
int icamd_transcode_dxt1_to_etc1_device(void *d_blocks, size_t n_bytes, void *hip_stream);
int icamd_transcode_dxt1_to_etc1(uint8_t *blocks, size_t n_bytes);

/* EXTENSION (the reference's only transcoder is DXT1 -> ETC1): DXT5 -> ETC2 RGBA8 (ICAMD_ETC2_RGBA8) in place, in the compressed
 * domain.  Both formats keep a block in 16 bytes, alpha word first, colour word second.  DEFINITION: every whole
 * 16-byte block B of the buffer is replaced by exactly the 16 bytes that
 *   icamd_encode_device(ICAMD_ETC2_RGBA8, ICAMD_ETC_HEURISTIC, 4 components, swap_rb = 0, ...)
 * writes for the 4 x 4 RGBA8 image that icamd_decode_device(ICAMD_DXT5, swap_rb = 0) produces from B:
 *   bytes 8..15  EncodeEtc1Block(kHeuristic) of the decoded colours (a DXT5 colour word always has four colours, so for c0 <= c1
 *                this differs from icamd_transcode_dxt1_to_etc1 of the same eight bytes; for c0 > c1 it is the same);
 *   bytes 0..7   the EAC search of ICAMD_ETC2_RGBA8 on the sixteen decoded alphas (the reference's truncating DecodeAlphaValues,
 *                0 and 255 in the six-value mode): lo and hi are the extremes of the alphas the texels use, the smallest
 *                (sse, table, multiplier, base) wins, every texel takes the smallest index at its minimum, multiplier 0 is never
 *                written.
 * No pixel is materialised: the search runs on the alpha word's eight palette values weighted by their use.
 * NULL -> ICAMD_FALSE; a device pointer that is not 16-byte aligned -> ICAMD_ERR_ARG; n_bytes < 16 -> ICAMD_OK, nothing touched;
 * otherwise n_bytes / 16 blocks are transcoded and the trailing n_bytes % 16 bytes are left as they were.  The device form is
 * stream-ordered, does not synchronise and can be captured into a graph. */
int icamd_transcode_dxt5_to_etc2_rgba8_device(void *d_blocks, size_t n_bytes, void *hip_stream);
int icamd_transcode_dxt5_to_etc2_rgba8(uint8_t *blocks, size_t n_bytes);

/* EXTENSIONS: the rest of a DXT / BC asset set to the ETC2 family in place, in the compressed domain.  Block
 * sizes do not change: DXT1 and ETC2 RGB8 keep a block in 8 bytes, BC4 and EAC R11 in 8, BC5 and EAC RG11 in 16.
 * DXT1 -> ETC2 RGB8 (ICAMD_ETC2_RGB8).  DEFINITION: every whole 8-byte block B of the buffer is replaced by exactly the 8 bytes that
 *   icamd_encode_device(ICAMD_ETC2_RGB8, ICAMD_ETC_HEURISTIC, 3 components, swap_rb = 0, ...)
 * writes for the 4 x 4 RGB888 image that icamd_decode_device(ICAMD_DXT1, swap_rb = 0) produces from B: with E the eight bytes
 * icamd_transcode_dxt1_to_etc1 writes for B and P the least-squares planar word of the sixteen decoded texels (the fit, the
 * quantisation and the ignored bits of ICAMD_ETC2_RGB8), the result is P where its squared error over 16 texels x 3 channels is
 * strictly smaller than E's, else E byte for byte.  The three-colour mode (c0 <= c1, index 3 black) decodes as the DXT1 decoder
 * decodes it.
 * BC4 -> EAC R11 (ICAMD_EAC_R11).  DEFINITION: every whole 8-byte block becomes the 8 bytes
 *   icamd_encode_device(ICAMD_EAC_R11, 1 component, ...)
 * writes for the 4 x 4 R8 image icamd_decode_device(ICAMD_BC4) produces from it -- the palette search of the DXT5 transcoder
 * above: lo and hi are the extremes of the palette entries some texel uses, the smallest (sse, table, multiplier, base) wins,
 * every texel takes the smallest index at its minimum, multiplier 0 is never written.
 * BC5 -> EAC RG11 (ICAMD_EAC_RG11).  DEFINITION: every whole 16-byte block becomes the BC4 -> EAC R11 result of its bytes 0..7
 * followed by that of its bytes 8..15.
 * No pixel is materialised.  With `block` = 8, 8, 16: NULL -> ICAMD_FALSE; a device pointer that is not block-aligned ->
 * ICAMD_ERR_ARG; n_bytes < block -> ICAMD_OK, nothing touched; otherwise n_bytes / block blocks are transcoded and the trailing
 * n_bytes % block bytes are left as they were.  The device forms are stream-ordered, do not synchronise, allocate nothing and can
 * be captured on a single stream; the host forms stage through the device (no CPU fall-back: ICAMD_ERR_NO_DEVICE without one). */
int icamd_transcode_dxt1_to_etc2_rgb8_device(void *d_blocks, size_t n_bytes, void *hip_stream);
int icamd_transcode_dxt1_to_etc2_rgb8(uint8_t *blocks, size_t n_bytes);
int icamd_transcode_bc4_to_eac_r11_device(void *d_blocks, size_t n_bytes, void *hip_stream);
int icamd_transcode_bc4_to_eac_r11(uint8_t *blocks, size_t n_bytes);
int icamd_transcode_bc5_to_eac_rg11_device(void *d_blocks, size_t n_bytes, void *hip_stream);
int icamd_transcode_bc5_to_eac_rg11(uint8_t *blocks, size_t n_bytes);

/* ---- multi-GPU from one process: a batch of independent images, host buffers ----
 * Image i is compressed exactly like icamd_compress(compressor, ..., buffers[i], outs[i], out_size) on device
 * devices[i % n_devices] (HIP device ordinals; a device may be listed more than once to get several in-flight
 * streams on it).  One host worker thread per list entry drives its own stream and staging buffers, so copies and
 * kernels of different devices overlap; images are independent, so there is no inter-device exchange and the
 * results land directly in the caller's host buffers.  statuses[i] (optional) receives each image's status; the
 * return value is ICAMD_OK if all are ICAMD_OK, otherwise the first non-OK status in image order. */
int icamd_compress_batch(int compressor, int etc_strategy, int format, uint32_t height, uint32_t width,
                         uint32_t padding_bytes_per_row, uint32_t n_images, const uint8_t *const *buffers,
                         uint8_t *const *outs, size_t out_size, const int *devices, int n_devices, int *statuses);

/* The same for images that are ALREADY RESIDENT IN HBM: image i lives on device
 * devices[i % n_devices] (d_srcs[i] is a pointer on that device) and is encoded there exactly like
 * icamd_encode_device(codec, ..., height, width, height, width, row_stride_bytes, 1 image) -- Compressor::Compress
 * (compressor.h:77-80) per image, no pixel ever crosses PCIe.  One host worker thread per list entry drives two HIP
 * streams on its device.  Output:
 *   d_dsts[i] != NULL      the image's blocks are written there (a pointer on the image's own device);
 *   gather_device >= 0     every image's blocks additionally land at d_gathered + i * gathered_image_stride_bytes, a
 *                          buffer on gather_device ("rank 0"): device-to-device copies (hipMemcpyPeerAsync, xGMI between
 *                          GPUs) that overlap the next image's encode; images on gather_device itself are encoded
 *                          straight into their slot when they have no d_dsts entry.  d_dsts may be NULL altogether.
 * Returns after all streams have drained.  statuses / return value as icamd_compress_batch. */
int icamd_encode_batch_sharded_device(int codec, int etc_strategy, int src_components, int swap_rb, uint32_t height,
                                      uint32_t width, uint32_t row_stride_bytes, uint32_t n_images,
                                      const void *const *d_srcs, void *const *d_dsts, const int *devices, int n_devices,
                                      int gather_device, void *d_gathered, size_t gathered_image_stride_bytes,
                                      int *statuses);

/* ---- multi-GPU, ONE PROCESS PER GPU: the gather of the compressed output over RCCL ("Collective" column) ----
 * BASELINE.json's north star: "large texture batches shard across the 8 GPUs of one node as independent image slabs ...
 * RCCL over xGMI only to gather the compressed output".  Encoding needs no exchange (icamd_encode_device on every rank's own
 * textures, or its block-row slab / PVRTC region of one image: helper.h:202-214 makes a slab's blocks ONE contiguous byte
 * range of the final buffer); what a C / C++ caller of the drop-in classes that runs one process per GPU still needs is the
 * collective that brings the ranks' byte ranges together on one rank -- this entry point.  The reference has nothing of the
 * kind (it is a single-threaded CPU library, public/compressor.h:48-138): there is no interface to cite, only the layout rule.
 *
 * RCCL is bound at run time (dlopen of librccl.so.1 -- the copy already loaded into the process if there is one, e.g.
 * PyTorch's), so libic_amd.so itself does not depend on it and every other entry point works without it.
 *
 * icamd_rccl_available       1 if librccl could be bound, else 0 (and icamd_last_error() says why).
 * icamd_rccl_get_unique_id   ncclGetUniqueId into id[ICAMD_RCCL_UNIQUE_ID_BYTES]; call on ONE rank and hand the bytes to the
 *                            others by any means (MPI_Bcast, a file, a socket, torch.distributed's store).
 * icamd_rccl_comm_init       ncclCommInitRank on the CURRENT HIP device; *comm is an ncclComm_t.  Collective: every rank
 *                            calls it with the same id and world.  A communicator the caller made with its own RCCL calls
 *                            (same librccl) is equally accepted by icamd_gather_blocks_rccl.
 * icamd_rccl_comm_destroy    ncclCommDestroy.
 * icamd_gather_blocks_rccl   rank r contributes counts_bytes[r] bytes at d_local (device memory of its own GPU); on rank
 *                            `root` they land at d_root_buffer + root_offsets_bytes[r] (NULL = the prefix sums of
 *                            counts_bytes: the ranks' ranges back to back, which is the final block stream when the ranks
 *                            hold consecutive slabs / texture ranges).  Unequal and zero counts are fine.  ONE grouped
 *                            ncclSend / ncclRecv exchange (ncclGroupStart ... ncclGroupEnd, ncclUint8): every peer writes
 *                            its own range of root's HBM over its own xGMI link; root's own range is a device-to-device
 *                            copy on the same stream (skipped when d_local already is its slot).  Enqueued on hip_stream,
 *                            not synchronised: run it on a second stream underneath the next batch's encode.  d_root_buffer
 *                            and root_offsets_bytes are only read on root.  Every rank passes the same counts.
 * Status: ICAMD_OK; ICAMD_ERR_ARG (bad rank / world / root, null pointers where bytes are due); ICAMD_ERR_NO_DEVICE when
 * librccl cannot be bound; ICAMD_ERR_HIP with RCCL's own error text for a failing RCCL or HIP call. */
#define ICAMD_RCCL_UNIQUE_ID_BYTES 128
int icamd_rccl_available(void);
int icamd_rccl_get_unique_id(void *id);
int icamd_rccl_comm_init(void **comm, int world, int rank, const void *id);
int icamd_rccl_comm_destroy(void *comm);
int icamd_gather_blocks_rccl(void *comm, int rank, int world, int root, const size_t *counts_bytes, const void *d_local,
                             void *d_root_buffer, const size_t *root_offsets_bytes, void *hip_stream);

/* ---- container framing (EXTENSION: SURVEY.md 8(f) row 4, tail) ----
 * The reference ends at the raw block stream (compressed_image.h:52-66); it has no file-container code, so there is
 * nothing to pin these against.  Host-side byte framing only (no device work), layouts from the public format
 * descriptions (csrc/containers.h): DDS (DXT1 / DXT5, BC4 as ATI1, BC5 as ATI2), KTX 1.1 and PVR v3 (DXT1, DXT5, ETC1,
 * PVRTC2, BC4, BC5, ETC2 RGBA8, ETC2 RGB8, ETC2 RGB8A1), PKM (ETC1 as "PKM 10" type 0, ETC2 RGB8 / RGBA8 / RGB8A1 as "PKM 20" type 1 / 3 / 4;
 * one level).  ICAMD_BC6H_UF16 / _SF16: DDS (DX10 header, dxgiFormat 95 / 96) and KTX (0x8E8F / 0x8E8E, GL_RGB) only.
 * ICAMD_BC7: DDS with the DX10 extension header (FourCC "DX10" + DDS_HEADER_DXT10, dxgiFormat 98; 148 header bytes
 * where the other codecs have 128), KTX 0x8E8C with GL_RGBA, PVR 15, no PKM.  The signed EAC codecs: see their values.
 * PVRTC4 is not framed (ICAMD_ERR_ARG from icamd_container_write).
 * Level l of a height x width texture is max(1, height >> l) x max(1, width >> l) pixels, its bytes exactly what
 * icamd_compress / icamd_downsample return for that size (PVRTC: square power-of-two levels of 8 x 8 and up only). */
enum { ICAMD_CONTAINER_DDS = 0, ICAMD_CONTAINER_KTX = 1, ICAMD_CONTAINER_PKM = 2, ICAMD_CONTAINER_PVR = 3 };
/* File size for `levels` mip levels (>= 1); 0 if the container cannot hold that codec / size / level count. */
size_t icamd_container_size(int container, int codec, uint32_t height, uint32_t width, uint32_t levels);
/* Writes header + levels (largest first) into out[out_size]; out_size must equal icamd_container_size(...) and
 * level_sizes[l] the level's block-stream size, else ICAMD_FALSE.  ICAMD_ERR_ARG for an unknown container / codec. */
int icamd_container_write(int container, int codec, uint32_t height, uint32_t width, uint32_t levels,
                          const uint8_t *const *level_data, const size_t *level_sizes, uint8_t *out, size_t out_size);

/* ---- mip chains (EXTENSION: one source image -> every level of its mip chain, each level encoded from pixels) ----
 * Level l of a height x width source P_0 is h_l x w_l = max(1, height >> l) x max(1, width >> l) pixels (the container
 * dimensions above); a full chain has L_max = floor(log2(max(height, width))) + 1 levels (icamd_mip_max_levels).
 * P_{l+1}[y][x], per channel, is the truncating average (a + b + c + d) / 4 of P_l at (y0, x0), (y0, x1), (y1, x0),
 * (y1, x1) -- the reference's Average4Uint8Fast, color_util.h:335-343 -- with y0 = 2y, y1 = min(2y + 1, h_l - 1) and
 * x0, x1 alike.  The pyramid is cascaded (each level from the one above); the last row / column of an odd-sized level is
 * dropped, not averaged with a replicated copy (clamping happens only where a side is already 1).
 * The bytes of level l are exactly icamd_encode_device(codec, etc_strategy, src_components, swap_rb, h_l, w_l, h_l, w_l,
 * w_l * src_components, 1, ...) of P_l -- for DXT1 / DXT5 / ETC1 the reference's Compress of those pixels -- and levels
 * are packed back to back, largest first: level l starts at offset[l] = sum over k < l of icamd_encoded_size(codec, h_k,
 * w_k), so that the level views go straight into icamd_container_write.  Averaging is per channel: swap_rb commutes. */
uint32_t icamd_mip_max_levels(uint32_t height, uint32_t width);  /* 0 for an empty image */
/* Bytes of one image's chain of `levels` levels; fills level_offsets[0 .. levels] (levels + 1 entries) when non-NULL.
 * 0 for PVRTC / unknown codecs, an empty image or levels outside 1 .. L_max. */
size_t icamd_mip_chain_size(int codec, uint32_t height, uint32_t width, uint32_t levels, size_t *level_offsets);
/* Device workspace icamd_encode_mips_device needs for that call (0: none; also 0 for arguments it refuses): the pixels of
 * level 6 (and 12, 18, ...) of every image, src_components bytes each, for chains longer than one pass reaches; for ETC1
 * the whole pixel pyramid (levels 1 .. levels-1 of every image, about a third of the source). */
size_t icamd_mip_workspace_size(int codec, int src_components, uint32_t height, uint32_t width, uint32_t levels,
                                uint32_t n_images);
/* Encodes levels 0 .. levels-1 of n_images sources (src_image_stride_bytes apart, rows of row_stride_bytes) into d_dst
 * (dst_image_stride_bytes apart, each image one chain laid out as above).  DXT1 / DXT5 / BC4 / BC5 read the source once:
 * one fused kernel per pass builds the 2 x 2 pyramid on chip and writes every level's blocks (2 launches for 4096^2, 3 for
 * 16384^2).  ETC1 has no fused kernel yet: it runs the ETC1 kernels on level 0 and on every level of the pixel pyramid,
 * which it builds in the workspace (the source is read twice).
 * Source rules as icamd_encode_device: DXT1 / ETC1 (any strategy) 3 or 4 bytes per pixel, DXT5 4, BC4 1..4, BC5 2..4,
 * swap_rb only with 3 or 4; any alignment and row padding.  ICAMD_FALSE for null pointers or an empty image;
 * ICAMD_ERR_ARG for PVRTC2 / PVRTC4 (whole-image encoders: use icamd_mip_pyramid_device, then icamd_encode_device per
 * level), levels of 0 or more than L_max, a workspace smaller than icamd_mip_workspace_size, or (n_images > 1) image
 * strides smaller than an image.  No allocation, no synchronisation: it can be captured into a graph. */
int icamd_encode_mips_device(int codec, int etc_strategy, int src_components, int swap_rb, uint32_t height,
                             uint32_t width, uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images,
                             size_t src_image_stride_bytes, size_t dst_image_stride_bytes, const void *d_src,
                             void *d_dst, void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* The pixel pyramid alone: levels 1 .. levels-1 of each image as tight rows of w_l * src_components bytes (1..4), back
 * to back (level 1 first) -- for PVRTC or uncompressed use.  Same argument rules; levels == 1 writes nothing. */
int icamd_mip_pyramid_device(int src_components, uint32_t height, uint32_t width, uint32_t row_stride_bytes,
                             uint32_t levels, uint32_t n_images, size_t src_image_stride_bytes,
                             size_t dst_image_stride_bytes, const void *d_src, void *d_dst, void *hip_stream);
/* Host buffers, Compressor + format as icamd_compress (its ICAMD_FALSE conventions: a format the compressor refuses, or
 * out_size != icamd_mip_chain_size); out receives the whole chain.  PVRTC: ICAMD_ERR_ARG. */
int icamd_compress_mips(int compressor, int etc_strategy, int format, uint32_t height, uint32_t width,
                        uint32_t padding_bytes_per_row, uint32_t levels, const uint8_t *buffer, uint8_t *out,
                        size_t out_size);

/* ---- mip filters (EXTENSION: opt-in; filter 0 is byte for byte the chain above) ----
 * The geometry, the cascade (level l+1 from the 8-bit level l), the four source pixels p_0..p_3 (rows 2y and
 * min(2y + 1, h_l - 1), columns alike), the per-level encode and the packing stay as above; only how P_{l+1} is made from
 * P_l changes.  `filter` is a combination of the bits below.  Integer arithmetic only; the result is exact.
 *   T[s] = floor(65535 * f(s / 255) + 0.5), f the sRGB transfer function (c / 12.92 for c <= 0.04045, else
 *          ((c + 0.055) / 1.055)^2.4): csrc/srgb_table.inc, generated by scripts/gen_srgb_table.py; strictly increasing.
 *   M[k] = (T[k-1] + T[k] + 1) >> 1 for k = 1..255;  inv(v) = the number of k with M[k] <= v (the nearest code; inv(T[s]) = s).
 * For each colour byte k in {0, 1, 2} (all three alike, so swap_rb still commutes):
 *   x_i = p_i[k] without ICAMD_MIP_FILTER_SRGB, T[p_i[k]] with it;   a_i = byte 3 of p_i;   A = a_0 + a_1 + a_2 + a_3
 *   unweighted   v = (x_0 + x_1 + x_2 + x_3) >> 2 without SRGB (the rule above), (x_0 + x_1 + x_2 + x_3 + 2) >> 2 with it
 *   weighted     (ICAMD_MIP_FILTER_ALPHA_WEIGHTED and A > 0)  v = (a_0 x_0 + a_1 x_1 + a_2 x_2 + a_3 x_3 + (A >> 1)) / A,
 *                integer division (the numerator is below 2^27); with A == 0 the unweighted value of the same filter
 *   output byte  v without SRGB, inv(v) with it.
 * Byte 3 is the truncating (a_0 + a_1 + a_2 + a_3) >> 2 under every filter: the alpha half of a DXT5 chain does not depend
 * on the filter.  A flat image stays flat under every filter, and a 0 / 255 checkerboard becomes 188 under SRGB (127 under
 * BOX).  Codecs: DXT1, DXT5, ETC1 (any strategy) and the pixel pyramid; a filter other than 0 needs src_components 3 or 4,
 * ALPHA_WEIGHTED 4.  ICAMD_ERR_ARG -- before a device is needed -- for BC4 / BC5 (data channels) with a filter other than 0,
 * a filter outside 0..3 (but see ICAMD_MIP_FILTER_NORMAL below) and those component counts; every other rule, status and the
 * workspace size (which does not depend on the filter) as for the entry point without `_filtered`, which is the same call
 * with filter 0.
 *
 * ---- normal-map mip filter (EXTENSION: ICAMD_MIP_FILTER_NORMAL = 4, on its own only: 5, 6 and 7 are ICAMD_ERR_ARG) ----
 * For tangent-space normal maps in BC5: R and G hold x and y of a unit vector.  The box filter shortens the averaged vector
 * and tilts it towards +z, so every lower mip is flatter than the surface it stands for; this filter sums the four vectors
 * (z rebuilt from x and y) and brings the sum back to unit length.  Geometry, cascade, the four source pixels, the per-level
 * encode and the packing are the mip-chain section's.  Integer arithmetic only; the result is exact.
 * r_i, g_i: the R and G bytes of p_i by the ICAMD_BC5 rules (R is byte 0, or byte 2 with swap_rb; G is byte 1).
 *   x_i = 2 r_i - 255,  y_i = 2 g_i - 255                      (unit length is 255)
 *   rem_i = max(0, 65025 - x_i^2 - y_i^2)
 *   z_i = (isqrt(4 rem_i) + 1) >> 1                            (the nearest integer to the root; isqrt is the floor root)
 *   X = sum x_i,  Y = sum y_i,  Z = sum z_i,  N2 = X^2 + Y^2 + Z^2          (N2 <= 3 * 1020^2 < 2^22)
 *   N2 == 0:  R' = (sum r_i) >> 2,  G' = (sum g_i) >> 2        (the box value, like A == 0 of the alpha-weighted filter)
 *   else      Ls = isqrt(N2 << 8)                              (the length with 4 fraction bits; N2 << 8 < 2^30)
 *             for V in (X, Y):  m = min(255, (4080 |V| + (Ls >> 1)) / Ls), integer division (the numerator is below 2^23);
 *                               v = m with the sign of V;  the output code is (v + 256) >> 1.
 * Every other byte of the pixel (B, A, or R's unused twin under swap_rb) is the truncating mean of filter 0, which keeps the
 * hand-off image of chains longer than one pass, and 3- and 4-byte sources, defined.
 * A flat image whose (x, y) is no longer than a unit vector stays flat; flat (255, 255), an over-long vector, becomes
 * (218, 218); the quad (218,128) (218,128) (128,218) (128,218) -- two normals tilted 45 degrees towards +x, two towards +y --
 * becomes (180, 180), the unit vector in that direction, where the box filter gives (173, 173).
 * icamd_encode_mips_filtered_device: ICAMD_BC5 only, src_components 2..4, swap_rb only with 3 or 4; the workspace size is
 * unchanged.  icamd_mip_pyramid_filtered_device: src_components == 2 only.  Every other codec or component count is
 * ICAMD_ERR_ARG before a device is needed.  icamd_compress_mips_filtered and the C++ CompressMipChainFiltered refuse it
 * (ICAMD_ERR_ARG): no Compressor + format pair selects BC5. */
enum { ICAMD_MIP_FILTER_BOX = 0, ICAMD_MIP_FILTER_SRGB = 1, ICAMD_MIP_FILTER_ALPHA_WEIGHTED = 2 };  /* bits; 3 = both */
enum { ICAMD_MIP_FILTER_NORMAL = 4 };  /* not a bit: valid alone */
int icamd_encode_mips_filtered_device(int codec, int etc_strategy, int src_components, int swap_rb, int filter,
                                      uint32_t height, uint32_t width, uint32_t row_stride_bytes, uint32_t levels,
                                      uint32_t n_images, size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                                      const void *d_src, void *d_dst, void *d_workspace, size_t workspace_bytes,
                                      void *hip_stream);
int icamd_mip_pyramid_filtered_device(int src_components, int filter, uint32_t height, uint32_t width,
                                      uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images,
                                      size_t src_image_stride_bytes, size_t dst_image_stride_bytes, const void *d_src,
                                      void *d_dst, void *hip_stream);
int icamd_compress_mips_filtered(int compressor, int etc_strategy, int format, int filter, uint32_t height, uint32_t width,
                                 uint32_t padding_bytes_per_row, uint32_t levels, const uint8_t *buffer, uint8_t *out,
                                 size_t out_size);
/* Name of the __global__ mip kernel a configuration launches ("" if it is refused); codec ICAMD_MIP_PYRAMID asks for the
 * pixel pyramid's, which is also what ETC1 chains launch before the ETC1 kernels. */
enum { ICAMD_MIP_PYRAMID = -1 };
const char *icamd_mip_kernel_name(int codec, int src_components, int filter);

/* ---- mip chains of the ETC2 family (EXTENSION: ICAMD_ETC2_RGBA8, ICAMD_ETC2_RGB8, ICAMD_ETC2_RGB8A1, ICAMD_EAC_R11, ICAMD_EAC_RG11) ----
 * The mip entry points above keep refusing these codecs (ICAMD_ERR_ARG, sizes 0); these are their chains.  Geometry, cascade,
 * level sizes and packing are those of icamd_encode_mips_device (the mip-chain section).  P_l is what icamd_mip_pyramid_device
 * writes for the source -- for filter != 0 icamd_mip_pyramid_filtered_device.  Averaging is per channel, so swap_rb commutes: the
 * pyramid is built unswapped and each level is encoded with swap_rb, as the ETC1 chain does.  Level l of an image is exactly the
 * bytes icamd_encode_etc2_device(codec, etc_strategy, etc2_modes, src_components, swap_rb, h_l, w_l, h_l, w_l,
 * w_l * src_components, 1, ...) writes for P_l; where etc2_modes is ICAMD_ETC2_MODES_DEFAULT that is icamd_encode_device (which is
 * what encodes the four codecs icamd_encode_etc2_device does not take).  ICAMD_ETC2_MODES_TH is accepted only with
 * ICAMD_ETC2_RGB8, as in that entry point.  Levels sit back to back at the icamd_etc2_mip_chain_size offsets, largest first: the
 * level views go straight into icamd_container_write.
 * What runs: the pixel-pyramid kernels into the workspace, then ONE encode launch over every level of every
 * image (per 65 535 images) -- its workgroups find their level in a table in the kernel argument and run the per-level kernels'
 * code on it -- then, with ICAMD_ETC2_MODES_TH, one launch of the T / H pass over the same grid.  1 + L launches become 2 (3 for
 * chains of more than 7 levels of an image larger than 128 x 128, whose pyramid takes two passes), 1 + 2 L become 3 (4).
 * Source rules are each codec's icamd_encode_device rules: src_components 4 for RGBA8 and RGB8A1, 3 or 4 for RGB8, 1..4 for R11,
 * 2..4 for RG11; swap_rb only with 3 or 4.  Filters (ICAMD_MIP_FILTER_*): 0 for all five; SRGB for RGB8, RGBA8 and RGB8A1;
 * ALPHA_WEIGHTED and SRGB | ALPHA_WEIGHTED for those three with src_components == 4; NORMAL for ICAMD_EAC_RG11 with
 * src_components == 2 only; everything else (R11 / RG11 with 1..3, NORMAL elsewhere, 5..7) is ICAMD_ERR_ARG.
 * Workspace: the whole pixel pyramid of every image (levels 1 .. levels-1, src_components bytes per pixel, about a third of the
 * source), 0 for levels == 1; it does not depend on the filter.
 * Statuses, in this order, all before a device is touched: ICAMD_FALSE for null pointers or an empty image; ICAMD_ERR_ARG for a
 * codec outside the five (ETC1 included), modes, components, swap_rb or a filter outside the rules; ICAMD_ERR_ARG for levels of 0
 * or more than L_max, a row stride smaller than a row, (n_images > 1) image strides smaller than an image / a chain, or a
 * workspace smaller than icamd_etc2_mip_workspace_size; ICAMD_OK for n_images == 0.  Then ICAMD_ERR_NO_DEVICE without a GPU.  No
 * allocation, no synchronisation: it can be captured on one stream. */
/* Bytes of one image's chain; fills level_offsets[0 .. levels] when non-NULL.  0 for every other codec, an empty image or
 * levels outside 1 .. L_max. */
size_t icamd_etc2_mip_chain_size(int codec, uint32_t height, uint32_t width, uint32_t levels, size_t *level_offsets);
/* 0 also for arguments the encode refuses (codec, components, levels). */
size_t icamd_etc2_mip_workspace_size(int codec, int src_components, uint32_t height, uint32_t width, uint32_t levels,
                                     uint32_t n_images);
int icamd_encode_etc2_mips_device(int codec, int etc_strategy, int etc2_modes, int src_components, int swap_rb, int filter,
                                  uint32_t height, uint32_t width, uint32_t row_stride_bytes, uint32_t levels,
                                  uint32_t n_images, size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                                  const void *d_src, void *d_dst, void *d_workspace, size_t workspace_bytes,
                                  void *hip_stream);
/* Name of the __global__ kernel of the encode launch; with ICAMD_ETC2_MODES_TH (ICAMD_ETC2_RGB8 only) of the T / H launch,
 * whatever the strategy.  An etc_strategy outside 0..3 is ICAMD_ETC_SMALLER_ERROR, as in the encoders; R11 / RG11 ignore it.
 * "" for combinations the encode refuses. */
const char *icamd_etc2_mip_kernel_name(int codec, int src_components, int etc_strategy, int etc2_modes);
/* Measurement knob (scripts/bench_etc2_mips.py): the order of the levels inside the encode launch's grid.x, 1 = largest level
 * first (the default), 0 = smallest first (the poorly filled workgroups of the small levels are dispatched first and run under
 * level 0's; measured within 2.3 % of the default, slower on large textures and faster on some batches of small ones, DESIGN.md
 * 3.18).  Process-wide; time only, never bytes.  ICAMD_ERR_ARG for any other value. */
int icamd_etc2_mip_tune(int level_order);

/* ---- quality metric (EXTENSION: the reference has no such function): the error of compressed blocks against source pixels ----
 * For image i, let D be the pixels that icamd_decode_device(codec, swap_rb, ...) yields for the blocks at
 * d_blocks + i * blocks_image_stride_bytes, laid out as icamd_encode_device writes them for that grid_height x grid_width
 * (block codecs: row-major; PVRTC: Z order, grid equal to the image), and S the source pixels, addressed as
 * icamd_encode_device addresses them (rows of row_stride_bytes, image i at d_src + i * src_image_stride_bytes).  Then, for
 * every compared channel k,
 *     stats[i].sse[k]     = sum over y < height, x < width of (S[y][x][k] - D[y][x][k])^2
 *     stats[i].max_abs[k] = the largest |S[y][x][k] - D[y][x][k]| over the same pixels.
 * Pixels of edge blocks outside the image do not count, nor do blocks of a padded grid wholly outside it (they are not read).
 * The compared channels are the decoder's output channels; the others are 0 in both arrays:
 *     DXT1, ETC1, ETC2 RGB8 bytes 0..2 of the source pixel   src_components 3 or 4 (alpha ignored, sse[3] = 0)
 *     DXT5, PVRTC2, PVRTC4  bytes 0..3                        src_components 4
 *     ETC2 RGBA8            bytes 0..3                        src_components 4
 *     ETC2 RGB8A1           bytes 0..3 (see ICAMD_ETC2_RGB8A1)  src_components 4
 *     BC4                   k = 0 is R                        src_components 1..4  (R, G located by the rules at ICAMD_BC4:
 *     BC5                   k = 0, 1 are R, G                 src_components 2..4   R = byte 0, or byte 2 with swap_rb)
 *     EAC R11 / RG11        as BC4 / BC5                      src_components 1..4 / 2..4
 * Everything is integer arithmetic: the result is exact and the same from run to run.  PSNR over N pixels and C channels is
 * 10 log10(255^2 N C / sum of sse).
 * Arguments: source rules as icamd_encode_device, codec by codec (swap_rb only with 3 or 4 components; PVRTC ignores it, as
 * its encoder and decoder do); PVRTC needs what its decoders need -- a square power of two of at least 8, grid equal to the
 * image, row_stride_bytes == width * 4 -- and answers ICAMD_FALSE otherwise.  Any pointers and strides are accepted for
 * d_src and d_blocks; d_stats (n_images records) must be 8-byte aligned and is overwritten.  ICAMD_FALSE for null pointers or
 * an empty image.  ICAMD_ERR_ARG for an unknown codec, a codec / component / swap combination the encoder refuses, a row
 * stride smaller than a row, a grid smaller than the image, a misaligned d_stats, or (uint64)height * width > 2^47 (a
 * squared byte difference is below 2^16, so every sum stays below 2^63).  All of these are answered before a device is
 * needed; ICAMD_ERR_NO_DEVICE without a GPU (there is no CPU path).  No allocation and no synchronisation: the zeroing of
 * d_stats is stream-ordered work of the call itself, so a captured graph can be replayed.  Geometries beyond one launch are
 * chunked like the decoders'. */
typedef struct { uint64_t sse[4]; uint32_t max_abs[4]; } icamd_error_stats;   /* 48 bytes */
int icamd_measure_error_device(int codec, int src_components, int swap_rb,
                               uint32_t height, uint32_t width, uint32_t grid_height, uint32_t grid_width,
                               uint32_t row_stride_bytes, uint32_t n_images,
                               size_t src_image_stride_bytes, size_t blocks_image_stride_bytes,
                               const void *d_src, const void *d_blocks, void *d_stats, void *hip_stream);
/* Host buffers, Compressor + format as icamd_decompress and its ICAMD_FALSE conventions (null pointers, an empty image, a
 * format the compressor refuses, blocks_size != the image's compressed size): `buffer` is the image as icamd_compress reads
 * it, `blocks` what icamd_compress wrote for it, *out one record.  ICAMD_COMPRESSOR_PVRTC (kRGBA, sizes as icamd_compress)
 * is measured through the PVRTC 2 bpp decoder extension. */
int icamd_measure_error(int compressor, int format, uint32_t height, uint32_t width, uint32_t padding_bytes_per_row,
                        const uint8_t *buffer, const uint8_t *blocks, size_t blocks_size, icamd_error_stats *out);
/* Name of the __global__ kernel icamd_measure_error_device launches for a configuration ("" if it refuses it). */
const char *icamd_metric_kernel_name(int codec, int src_components);

/* ---- 16-bit and signed EAC R11 / RG11 (EXTENSION, PARITY UNPINNED: the reference has no EAC) ----
 * codec: ICAMD_EAC_R11, ICAMD_EAC_RG11 (unsigned, uint16 samples) or ICAMD_EAC_SIGNED_R11, ICAMD_EAC_SIGNED_RG11 (int16 samples).
 * The words are EAC words (see ICAMD_EAC_R11); blocks in the raster order of ETC1, 8 (R11) / 16 (RG11: R's word, then G's) bytes.
 * M is the modifier table of ICAMD_ETC2_RGBA8; s = (multiplier == 0 ? 1 : 8 multiplier).
 *
 * Decode to 16 bits (Khronos EAC).
 *   Unsigned: v = clamp(8 base + 4 + M[table][index] * s, 0, 2047); out16 = v << 5 | v >> 6.
 *   Signed: b = byte 0 as int8, with -128 read as -127; v = clamp(8 b + M[table][index] * s, -1023, 1023);
 *           out16 = sign(v) * ((|v| << 5) + (|v| >> 5)), an int16 in -32767 .. 32767.
 *   Known answers, the word 80 0d 7e 49 24 92 49 24.  Read unsigned (base 128, multiplier 0, table 13, indices 3, 7, 4, 4, ...):
 *   v = 1018, 1037, 1028, ... and out16 = 32591, 33200, 32912, ...  Read signed (base -128 -> -127): v = -1023 (clamped), -1007,
 *   -1016, ... and out16 = -32767, -32255, -32543, ...  Signed base 127, multiplier 15, table 0, index 7 clamps to 1023 -> 32767.
 *
 * Encode from 16-bit samples, a DEFINITION, in the 11-bit domain (restated in numpy in tests/eac11_16_oracle.py; the kernels are
 * bit-exact against it).  The source has src_channels (1..4) little-endian 16-bit samples per pixel, R = sample 0, G = sample 1
 * (RG needs at least 2; there is no swap).  Grids, clamp-to-edge replication, the padded-grid fetch, strides and batches as for
 * ICAMD_EAC_R11 through icamd_encode_device.  Per channel and block:
 *   target per texel: a = u16 >> 5 (unsigned); with x = max(s16, -32767), a = sign(x) * (|x| >> 5) (signed);
 *   lo, hi = the smallest and largest a, R = hi - lo; span[t] = M[t][7] - M[t][3]; (Vmin, Vmax) = (0, 2047) unsigned,
 *   (-1023, 1023) signed;
 *   candidates, in this order, replacing the best on a STRICTLY smaller sse only:
 *     for table t = 0..15, with m0 = (2 R + 8 span[t]) / (16 span[t]) (truncating):
 *       for m in (0, clamp(m0 - 1, 1, 15), clamp(m0, 1, 15), clamp(m0 + 1, 1, 15)):
 *           s = (m == 0 ? 1 : 8 m), c2 = lo + hi + s, b0 = c2 >> 4 (unsigned) or (c2 + 8) >> 4 (signed; arithmetic shift: floor);
 *         for b in b0 - 1, b0, b0 + 1, each clamped to 0..255 (unsigned) or -127..127 (signed):
 *           v_k = clamp(B + M[t][k] s, Vmin, Vmax) with B = 8 b + 4 (unsigned) or 8 b (signed); every texel takes the smallest
 *           k minimising |a - v_k|; sse = the sum of the squared minima (at most 16 * 2047^2 < 2^27).
 *   That is 192 candidates (duplicates after clamping are harmless).  The word is (b, m, t) of the best candidate and its
 *   texels' indices.  Multiplier 0 IS written (its modifier steps are 1/8 of multiplier 1's: smooth content).  The signed encoder
 *   never writes base -128. */
/* icamd_encode_eac11_16_device: arguments as icamd_encode_device without etc_strategy and swap_rb.  Status, in this order:
 * ICAMD_FALSE for a null pointer or height or width 0; ICAMD_ERR_ARG for a codec other than the four, src_channels outside
 * 1..4 (R11) / 2..4 (RG11), or an odd d_src, row_stride_bytes or src_image_stride_bytes (samples are 2-byte aligned);
 * ICAMD_OK for n_images == 0; ICAMD_ERR_ARG for row_stride_bytes < width * src_channels * 2.  All answered before a device is
 * needed.  d_dst: any alignment, icamd_encoded_size(codec, grid) bytes per image.  No allocation, no synchronisation. */
int icamd_encode_eac11_16_device(int codec, int src_channels, uint32_t height, uint32_t width, uint32_t grid_height,
                                 uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                                 size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                                 const void *d_src, void *d_dst, void *hip_stream);
/* icamd_decode_eac11_16_device: arguments as icamd_decode_device without swap_rb.  Writes `height` rows of width * 2 (R11) /
 * width * 4 (RG11: R then G per pixel) + padding_bytes_per_row bytes, samples uint16 (unsigned codecs) or int16 (signed),
 * little-endian; padding bytes are left alone.  ICAMD_FALSE for a null pointer or an empty image; ICAMD_ERR_ARG for a codec
 * other than the four, an odd padding_bytes_per_row, d_pixels or dst_image_stride_bytes, or a row of 2^32 bytes or more;
 * ICAMD_OK for n_images == 0.  d_blocks: any alignment.  No allocation, no synchronisation. */
int icamd_decode_eac11_16_device(int codec, uint32_t height, uint32_t width, uint32_t padding_bytes_per_row, uint32_t n_images,
                                 size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                                 const void *d_blocks, void *d_pixels, void *hip_stream);
/* icamd_measure_error_eac11_16_device: arguments as icamd_measure_error_device with src_channels for src_components and no
 * swap_rb; fills n_images icamd_error_stats records.  sse[k] and max_abs[k], k = 0 (R) and 1 (G, RG11 only), compare the
 * decoder's 16-bit value with the 16-bit source sample AS STORED (not with its 11-bit target), over the pixels inside the
 * image; the other entries are 0.  ICAMD_FALSE for a null pointer or an empty image; ICAMD_ERR_ARG for a codec other than the
 * four, src_channels the encoder refuses, an odd d_src, row_stride_bytes or src_image_stride_bytes, a row stride smaller than
 * a row, a grid smaller than the image, a d_stats that is not 8-byte aligned, or (uint64)height * width > 2^31 (a squared
 * difference is below 2^32, so every sum stays below 2^63); ICAMD_OK for n_images == 0.  All answered before a device is
 * needed.  No allocation and no synchronisation (the zeroing of d_stats is stream-ordered work of the call). */
int icamd_measure_error_eac11_16_device(int codec, int src_channels, uint32_t height, uint32_t width,
                                        uint32_t grid_height, uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                                        size_t src_image_stride_bytes, size_t blocks_image_stride_bytes,
                                        const void *d_src, const void *d_blocks, void *d_stats, void *hip_stream);
/* Names of the __global__ kernels the two launch for a configuration ("" where they refuse it). */
const char *icamd_eac11_16_kernel_name(int codec, int src_channels);
const char *icamd_eac11_16_metric_kernel_name(int codec, int src_channels);

/* ---- BC6H: BPTC float (EXTENSION, PARITY UNPINNED: the reference has no BC6H) ----
 * codec: ICAMD_BC6H_UF16 (unsigned) or ICAMD_BC6H_SF16 (signed).  A sample is an IEEE binary16 BIT PATTERN, little-endian; all
 * arithmetic below is on integers.  Texel i = 4 y + x.  Blocks are 16 bytes, read as a 128-bit little-endian number, bit 0 first.
 *
 * Decode: the whole format.  The independent decoder the tests hold this to is Pillow's (DDS, dxgiFormat 95 / 96); where the
 * public descriptions and that decoder differ, THIS TEXT STATES WHAT THE DECODER DOES (marked [*]).
 *   Modes.  Bits 0..1 = 00 or 01: a 2-bit mode field; otherwise bits 0..4 are the mode field.  Fourteen modes; the fields 10011,
 *     10111, 11011, 11111 are reserved and decode to R = G = B = 0 (A as below).  Per mode (csrc/bc6h_mode_tables.inc holds the
 *     placement of every header bit; tests/bc6h_oracle.py states it a second time):
 *       field  endpoint bits  delta bits R G B  transformed  subsets      field  endpoint bits  delta bits  transformed  subsets
 *       00     10             5 5 5             yes          2            11010  8              5 5 6       yes          2
 *       01     7              6 6 6             yes          2            11110  6              (6 6 6)     no           2
 *       00010  11             5 4 4             yes          2            00011  10             (10 each)   no           1
 *       00110  11             4 5 4             yes          2            00111  11             9 9 9       yes          1
 *       01010  11             4 4 5             yes          2            01011  12             8 8 8       yes          1
 *       01110  9              5 5 5             yes          2            01111  16             4 4 4       yes          1
 *       10010  8              6 5 5             yes          2
 *       10110  8              5 6 5             yes          2
 *     Two-subset modes: the header is 82 bits, the 5-bit partition its last field; partitions and anchors are the first 32
 *     entries of BC7's two-subset tables; indices are 3 bits (2 bits for texel 0 and for the second subset's anchor), weights
 *     {0,9,18,27,37,46,55,64}.  One-subset modes: the header is 65 bits; indices are 4 bits (3 for texel 0), weights BC7's 4-bit
 *     set.  Subset 0 interpolates endpoints 0 and 1, subset 1 endpoints 2 and 3.
 *   Endpoints, per colour, bits = the mode's endpoint bits.  Endpoint 0 is the stored field; in the signed format it is
 *     sign-extended from `bits`.  Transformed modes: e_k = (e_0 + sext(delta_k)) & (2^bits - 1), the delta sign-extended from
 *     its own width; in the signed format e_k is then read as a 16-bit two's-complement number -- it is NOT sign-extended from
 *     `bits`, so only the 16-bit mode sees negative transformed endpoints [*].  Untransformed modes: the stored fields, in the
 *     signed format each sign-extended from `bits`.
 *   Un-quantise c.  Unsigned: bits >= 15: c; c == 0: 0; c == 2^bits - 1: 0xFFFF; else ((c << 16) + 0x8000) >> bits.
 *     Signed: bits >= 16: c; otherwise on |c|: 0 -> 0; >= 2^(bits-1) - 1 -> 0x7FFF; else ((|c| << 15) + 0x4000) >> (bits - 1);
 *     the sign is put back.
 *   Interpolate: x = (a (64 - w) + b w) >> 6, an arithmetic shift, WITHOUT a rounding term [*].
 *   Finish: unsigned (x * 31) >> 6; signed x < 0 ? (((-x) * 31) >> 5) | 0x8000 : (x * 31) >> 5.  The result is the half's bits.
 *   Known answers: the unsigned block 03 | e << 5 | e << 15 | ... (mode field 00011, all six endpoints e, indices 0) decodes
 *     e = 100 to 3115, 300 to 9315, 400 to 12415, 480 to 14895, 495 to 15360 (1.0), 1023 to 31743 (0x7BFF).
 *
 * Encode, a DEFINITION (restated in numpy in tests/bc6h_oracle.py; the kernels are bit-exact against it).  It writes mode field
 * 00011 only: one subset, 10-bit endpoints stored directly, 4-bit indices.  The source has src_channels (3 or 4) halves per
 * pixel, R, G, B = samples 0, 1, 2 (the fourth is not read).  Grids, clamp-to-edge replication, the padded-grid fetch, strides
 * and batches as for ICAMD_BC7.
 *   The t domain.  A half h with magnitude m = h & 0x7FFF has the target t: unsigned format: 0 for a NaN (m > 0x7C00) and for
 *     any h with the sign bit set, else min(m, 0x7BFF); signed format: 0 for a NaN, else +-min(m, 0x7BFF) (-0 gives 0).  t is
 *     monotone in the float's value.  D(q) = t(finish(un-quantise(q))) at 10 bits for q in 0..1023 (unsigned) or -511..511
 *     (signed; -512 is never written): 0, 31 q + 15, ..., D(1023) = 31743; signed +-(62 |q| + 31), D(+-511) = +-31743.
 *   1. Targets, as step 1 of ICAMD_BC7 over the three channels of t_p: lo_c, hi_c; c* = the channel with the largest hi - lo
 *      (ties: R before G before B); T0 = lo, T1 = hi; for c != c*, T0_c and T1_c are exchanged if
 *      16 sum_p t_p[c*] t_p[c] - (sum_p t_p[c*]) (sum_p t_p[c]) < 0 (64-bit sums).
 *   2. Quantise, per channel: E_c = the smallest q that minimises |D(q) - T_c|.  (The kernels try T / 31 resp. T / 62, truncating,
 *      and its two neighbours; tests/test_bc6h_host.py proves that equal for every T.)
 *   3. Indices.  pal_k[c] = t(finish(((64 - w_k) U0_c + w_k U1_c) >> 6)) with U = un-quantise(E): exactly what the decoder
 *      makes of index k (no rounding term, see Decode).  Texel p takes the smallest k that minimises sum_c (pal_k[c] - t_p[c])^2.
 *      Widths: one channel's square is below 2^32 in both formats; a texel's sum is below 2^32 in the unsigned format
 *      (3 * 31743^2) and needs 64 bits in the signed one (3 * 63486^2); sse, the sum of the sixteen minima, is 64-bit.
 *   4. One refit: step 4 of ICAMD_BC7 on t_p (three channels), T0', T1' clamped to 0..31743 (unsigned) or -31743..31743 (signed;
 *      rdiv is a floor division); steps 2 and 3 run on T' and replace the first pass only on a STRICTLY smaller sse.
 *   5. Anchor.  If k_0 >= 8: E0 and E1 are exchanged and every k becomes 15 - k (the interpolation is symmetric: the decoded
 *      texels do not change).
 *   6. Pack: bits 0..4 = 00011 (the byte 0x03 | ...); E0 of R, G, B at bits 5, 15, 25 and E1 of R, G, B at bits 35, 45, 55
 *      (10 bits each, two's complement in the signed format); k_0 in 3 bits at bit 65; k_1..k_15 in 4 bits each.
 *   Example: sixteen texels (1.0, 0.5, 0.25) = halves (0x3C00, 0x3800, 0x3400), unsigned, give
 *     e3 3d e7 5a 7b cf b9 d6 00 .. 00: t = (15360, 14336, 13312), E0 = E1 = (495, 462, 429) with D = 15360, 14337, 13314 (sse 80),
 *     every k = 0, a = 65536 and b = c = 0: det = 0, no refit.  The signed format gives e3 9e 73 ac b9 e7 1c 6b 00 .. 00:
 *     E = (247, 231, 214) with D = 15345, 14353, 13299 (sse 10928).
 *
 * Metric: per image and channel k = 0, 1, 2 (R, G, B; entry 3 is 0), sse[k] and max_abs[k] of d = t(decoded half) - t(source
 * half) with the encoder's map t of the codec's format applied to both, over the pixels inside the image. */
/* icamd_encode_bc6h_device: arguments as icamd_encode_eac11_16_device.  Status, in this order: ICAMD_FALSE for a null pointer or
 * height or width 0; ICAMD_ERR_ARG for a codec other than the two, src_channels other than 3 or 4, or an odd d_src,
 * row_stride_bytes or src_image_stride_bytes (samples are 2-byte aligned); ICAMD_OK for n_images == 0; ICAMD_ERR_ARG for
 * row_stride_bytes < width * src_channels * 2.  All answered before a device is needed.  d_dst: any alignment,
 * icamd_encoded_size(codec, grid) bytes per image.  No allocation, no synchronisation. */
int icamd_encode_bc6h_device(int codec, int src_channels, uint32_t height, uint32_t width, uint32_t grid_height,
                             uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                             size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                             const void *d_src, void *d_dst, void *hip_stream);
/* icamd_decode_bc6h_device: arguments as icamd_decode_eac11_16_device.  Writes `height` rows of width RGBA16F pixels (8 bytes:
 * R, G, B as decoded, A = 0x3C00 = 1.0) + padding_bytes_per_row bytes; padding bytes are left alone.  ICAMD_FALSE for a null
 * pointer or an empty image; ICAMD_ERR_ARG for a codec other than the two, an odd padding_bytes_per_row, d_pixels or
 * dst_image_stride_bytes, or a row of 2^32 bytes or more; ICAMD_OK for n_images == 0.  d_blocks: any alignment.  No allocation,
 * no synchronisation. */
int icamd_decode_bc6h_device(int codec, uint32_t height, uint32_t width, uint32_t padding_bytes_per_row, uint32_t n_images,
                             size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                             const void *d_blocks, void *d_pixels, void *hip_stream);
/* icamd_measure_error_bc6h_device: arguments as icamd_measure_error_eac11_16_device; fills n_images icamd_error_stats records
 * (Metric, above).  ICAMD_FALSE for a null pointer or an empty image; ICAMD_ERR_ARG for a codec other than the two, src_channels
 * the encoder refuses, an odd d_src, row_stride_bytes or src_image_stride_bytes, a row stride smaller than a row, a grid smaller
 * than the image, a d_stats that is not 8-byte aligned, or (uint64)height * width > 2^31 (a squared difference is below 2^32,
 * so every sum stays below 2^63); ICAMD_OK for n_images == 0.  All answered before a device is needed.  No allocation and no
 * synchronisation (the zeroing of d_stats is stream-ordered work of the call). */
int icamd_measure_error_bc6h_device(int codec, int src_channels, uint32_t height, uint32_t width,
                                    uint32_t grid_height, uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                                    size_t src_image_stride_bytes, size_t blocks_image_stride_bytes,
                                    const void *d_src, const void *d_blocks, void *d_stats, void *hip_stream);
/* Names of the __global__ kernels the two launch for a configuration ("" where they refuse it). */
const char *icamd_bc6h_kernel_name(int codec, int src_channels);
const char *icamd_bc6h_metric_kernel_name(int codec, int src_channels);

/* ---- BC6H with a two-subset candidate (EXTENSION, opt-in, PARITY UNPINNED) ----
 * icamd_encode_bc6h_modes_device is icamd_encode_bc6h_device with one more argument, bc6h_modes:
 *   ICAMD_BC6H_MODES_DEFAULT   the call IS icamd_encode_bc6h_device: the same kernels, the same launches, byte for byte.
 *   ICAMD_BC6H_MODES_EXTENDED  ONE fused kernel in place of those: per block it computes the one-subset block of
 *                              icamd_encode_bc6h_device and ONE two-subset candidate, and writes the candidate iff it is
 *                              STRICTLY closer in the t domain.
 * Statuses, in this order, all before a device is needed: ICAMD_FALSE for a null pointer or height or width 0; ICAMD_ERR_ARG for
 * a codec other than the two, a bc6h_modes other than the two, src_channels other than 3 or 4, or an odd d_src,
 * row_stride_bytes or src_image_stride_bytes; ICAMD_OK for n_images == 0; ICAMD_ERR_ARG for row_stride_bytes < width *
 * src_channels * 2; ICAMD_ERR_NO_DEVICE without a GPU.  No allocation, no synchronisation, capturable on one stream.  The
 * decoder, the metric and the containers read and frame every mode already.
 *
 * The candidate, a DEFINITION (restated in numpy in tests/bc6h_modes_oracle.py; the kernels are bit-exact against it).  The
 * texels t_p are exactly those of the one-subset definition above (the t domain of the codec's format, edge replication, padded
 * grids, channels); that definition's steps 1-6 give the one-subset block and its final sse, sse1.
 *   Grids.  An endpoint of b bits is q in 0 .. 2^b - 1 (unsigned) or -(2^(b-1) - 1) .. 2^(b-1) - 1 (signed).
 *     D_b(q) = t(finish(un-quantise_b(q))); Q_b(T) = the smallest q that minimises |D_b(q) - T|.  (The kernels try
 *     T / (31 * 2^(10-b)) resp. T / (62 * 2^(10-b)), truncating, and its two neighbours; tests/test_bc6h_modes_host.py proves that
 *     equal for every T and b = 6..10.)
 *   1. Partition.  For s = 0..31 (the two-subset partitions of Decode): n0, n1 = the subsets' texel counts, S0, S1 = their
 *      (R, G, B) sums of t; N_s = n1 |S0|^2 + n0 |S1|^2, d_s = n0 n1; s beats s' iff N_s d_s' > N_s' d_s (exact integers below
 *      2^50).  The best partition, ties to the smaller s.  ONE partition is fitted.
 *   2. Targets.  Subset j: step 1 of the one-subset definition over the subset's texels (the factor 16 of the exchange test
 *      becomes the subset's texel count): T0_j, T1_j.
 *   3. Mode ladder, tried in this order; the first feasible mode is the candidate's:
 *        field  endpoint bits b  delta bits R G B
 *        00     10               5 5 5
 *        01110  9                5 5 5
 *        10010  8                6 5 5
 *        10110  8                5 6 5
 *        11010  8                5 5 6
 *        01     7                6 6 6
 *        11110  6                none: four endpoints stored directly; always feasible
 *      E = Q_b of the twelve targets: E[0], E[1] = subset 0's, E[2], E[3] = subset 1's.  A transformed mode is feasible iff for
 *      every channel c of delta width w, both x in {E[0][c], E[1][c]} and every endpoint y: -2^(w-1) <= y[c] - x <= 2^(w-1) - 1
 *      (both of subset 0's endpoints can be the base, so step 5 cannot push a delta out of range; no wrap-around is used), and,
 *      in the signed format, all twelve E >= 0 (Decode does not sign-extend transformed endpoints from b bits [*], a
 *      specification decoder does; with non-negative endpoints they agree, and a block with a negative endpoint goes to 11110,
 *      which sign-extends in both).  The three 11-bit two-subset modes are decoded, never written.
 *   4. Sub-fits at the mode's b, subset 0 then subset 1.  pal_k[c] = t(finish(((64 - w_k) U0_c + w_k U1_c) >> 6)) over the
 *      3-bit weights, U = un-quantise_b(E).  Every texel of the subset takes the smallest k of the least squared distance over
 *      three channels; the sub-sse is the sum of the minima.  One refit: step 4 of the one-subset definition with the sums over
 *      the subset and the 3-bit weights (det = 0: none), T' clamped as there, E' = Q_b(T'), searched again; it replaces the first
 *      pass iff its sub-sse is STRICTLY smaller AND E' with the other subset's current endpoints is still feasible for the mode
 *      (subset 1 is checked against subset 0's final endpoints).  sse2 = the two sub-sses.  Widths as in the one-subset definition.
 *   5. Anchors: texel 0 for subset 0, the partition's anchor for subset 1.  Where the anchor's k >= 4 the subset's endpoints are
 *      exchanged and its k become 7 - k (the weights are symmetric: the decoded texels do not change).
 *   6. Pack: the mode field; E[0] in b bits per channel; in the transformed modes E[1..3] as (E[k] - E[0]) & (2^w - 1), in 11110
 *      as they are in 6 bits, two's complement; the 5-bit partition; every header bit where csrc/bc6h_mode_tables.inc puts it; the
 *      sixteen k from bit 82 in texel order, 3 bits each, the two anchors' in 2.
 *   Choice: the candidate is written iff sse2 < sse1.  So no block's t-domain error exceeds ICAMD_BC6H_MODES_DEFAULT's.
 *   Example: ICAMD_BC6H_UF16, a block whose rows 0..3 hold the halves (0x3C00, 0x3800, 0x3400), (0x3C40, 0x3800, 0x3400),
 *     (0x3D00, 0x3700, 0x3480), (0x3D00, 0x3740, 0x3480) gives e4 3d e7 5a 13 15 40 80 50 a4 01 e0 ff ff 3f 49: sse1 = 16024;
 *     partition 13 (rows 0-1 | rows 2-3), mode field 00 at the first rung, first pass E = (495, 462, 429), (497, 462, 429) |
 *     (503, 454, 433), (503, 456, 433) with sub-sses 56 and 884, neither refit strictly better, subset 1's anchor (texel 15) at
 *     k = 7: its endpoints exchanged; sse2 = 940 < sse1, so the candidate is written.  ICAMD_BC6H_SF16 gives
 *     e4 9e 73 ac 09 1b 60 50 08 a2 29 e9 ff ff 7f db (sse1 = 23840, sse2 = 13944).
 * icamd_bc6h_modes_kernel_name names the kernel that writes the final bytes under ICAMD_BC6H_MODES_EXTENDED; under
 * ICAMD_BC6H_MODES_DEFAULT it answers what icamd_bc6h_kernel_name answers; "" outside the domain. */
enum { ICAMD_BC6H_MODES_DEFAULT = 0,    /* what icamd_encode_bc6h_device writes: field 00011 */
       ICAMD_BC6H_MODES_EXTENDED = 1 }; /* + one two-subset candidate per block, written where strictly closer */
int icamd_encode_bc6h_modes_device(int codec, int bc6h_modes, int src_channels, uint32_t height, uint32_t width,
                                   uint32_t grid_height, uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                                   size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                                   const void *d_src, void *d_dst, void *hip_stream);
const char *icamd_bc6h_modes_kernel_name(int codec, int src_channels, int bc6h_modes);

/* ---- half-float pixel pyramid (EXTENSION: levels 1 .. levels-1 of RGB16F / RGBA16F images) ----
 * What icamd_mip_pyramid_device is for 8-bit pixels, for pixels of src_channels (3 or 4) binary16 samples, given and written as
 * bit patterns: rows of level l are tight (w_l * src_channels * 2 bytes), levels 1 .. levels-1 sit back to back, image i at
 * d_dst + i * dst_image_stride_bytes.  Geometry, cascade and odd-size rule are that entry point's: h_l = max(1, h >> l), pixel
 * (x, y) of level l + 1 from rows 2 y and min(2 y + 1, h_l - 1) and columns 2 x and min(2 x + 1, w_l - 1) of level l, each level
 * made from the ROUNDED level above.  It filters linear light: there is no filter argument, and all src_channels samples of a
 * pixel (alpha too) are treated alike.
 * The filter, per sample, from the four samples p0 .. p3 above it -- exact integer arithmetic on the 16-bit patterns:
 *   Clean.  Let m = h & 0x7FFF.  If m > 0x7C00 (NaN), h := 0.  If m == 0x7C00 (+-Inf), h := (h & 0x8000) | 0x7BFF.
 *   Fixed point.  Let e = (h >> 10) & 31 and f = h & 1023.  F(h) = +-(e == 0 ? f : (1024 + f) << (e - 1)): the value in units
 *     of 2^-24, below 2^40 in magnitude.
 *   Sum and shift.  S = F(p0) + F(p1) + F(p2) + F(p3) in 64 bits (|S| < 2^42), A = |S|, n = the bit length of A,
 *     s = max(2, n - 11).
 *   Round.  q = A >> s, rem = A & (2^s - 1); add 1 to q if rem > 2^(s-1), or if rem == 2^(s-1) and q is odd (nearest even).
 *   Output.  M = ((s - 2) << 10) + q; a carry of q into 2048 runs into the exponent, and M never exceeds 0x7BFF.  M == 0
 *     (S == 0, or an |S| of at most 2 units that rounds to nothing) gives 0x0000: -0 is never written.  Otherwise M, with
 *     | 0x8000 if S < 0.
 * That is the half nearest to the mean of the four cleaned values, ties to even.
 *   Example: (0x3C00, 0x3C00, 0x3C01, 0x3C01) gives 0x3C00 and (0x3C01, 0x3C01, 0x3C02, 0x3C02) gives 0x3C02 (ties);
 *     (0x7C00, 0x7C00, 0x7C00, 0x7C00) gives 0x7BFF; (0x3C00, 0xBC00, 0x0001, 0x8001) gives 0x0000.
 * Statuses: ICAMD_ERR_ARG for src_channels other than 3 or 4; ICAMD_FALSE for null pointers or an empty image; ICAMD_ERR_ARG
 * for levels of 0 or more than L_max, a row stride smaller than a row, (n_images > 1) image strides smaller than an image / a
 * pyramid, or an odd d_src, d_dst, row_stride_bytes or image stride (samples are 2-byte aligned; no wider alignment is assumed);
 * ICAMD_OK for n_images == 0.  Then ICAMD_ERR_NO_DEVICE without a GPU.  levels == 1 writes nothing.  No allocation, no
 * synchronisation.  One launch per six levels (seven where the pass's input level is at most 128 x 128). */
int icamd_mip_pyramid_f16_device(int src_channels, uint32_t height, uint32_t width, uint32_t row_stride_bytes,
                                 uint32_t levels, uint32_t n_images, size_t src_image_stride_bytes,
                                 size_t dst_image_stride_bytes, const void *d_src, void *d_dst, void *hip_stream);
/* Name of the __global__ kernel; "" unless src_channels is 3 or 4. */
const char *icamd_mip_f16_kernel_name(int src_channels);

/* ---- mip chains of BC7 and BC6H (EXTENSION: ICAMD_BC7, ICAMD_BC6H_UF16, ICAMD_BC6H_SF16) ----
 * The mip entry points of the mip-chain section keep refusing these codecs (ICAMD_ERR_ARG, sizes 0); these are their chains.
 * Geometry, cascade, level sizes and packing are those of icamd_encode_mips_device.  P_l is what the pixel-pyramid entry point
 * writes for the source: icamd_mip_pyramid_filtered_device(src_components, filter, ...) for BC7 (built unswapped: averaging is
 * per channel, so swap_rb commutes), icamd_mip_pyramid_f16_device(src_channels, ...) for BC6H.  Level l of image i is exactly
 * the bytes icamd_encode_bc7_device(bc7_modes, src_components, swap_rb, h_l, w_l, h_l, w_l, w_l * src_components, 1, ...), or
 * icamd_encode_bc6h_modes_device(codec, bc6h_modes, src_channels, h_l, w_l, h_l, w_l, w_l * src_channels * 2, 1, ...), writes
 * for P_l (P_0: the source with its own strides).  Levels sit back to back at the icamd_bptc_mip_chain_size offsets, largest
 * first: the level views go straight into icamd_container_write.
 * What runs: the pixel-pyramid kernels into the workspace, then ONE encode launch over every level of every image (per 65 535
 * images), whose workgroups find their level in a table in the kernel argument and run the per-level kernels' code on it: the
 * 1 + L launches of pyramid + one encode call per level become 2 (3 where the pyramid takes two passes).
 * BC7: src_components 3 or 4, any swap_rb; filter ICAMD_MIP_FILTER_BOX or ICAMD_MIP_FILTER_SRGB with either, ALPHA_WEIGHTED and
 * SRGB | ALPHA_WEIGHTED with 4 components; ICAMD_MIP_FILTER_NORMAL and 5..7 are ICAMD_ERR_ARG.  BC6H: src_channels 3 or 4;
 * no filter argument (the data is linear light).
 * Workspace: the whole pixel pyramid of every image (levels 1 .. levels-1, tight rows), 0 for levels == 1, where d_workspace
 * may be NULL.  For BC6H d_workspace must be 2-byte aligned, as d_src, row_stride_bytes and src_image_stride_bytes.
 * Statuses, in this order, all before a device is touched: ICAMD_FALSE for null pointers or an empty image; ICAMD_ERR_ARG for
 * a codec, modes, components / channels or a filter outside the rules; ICAMD_ERR_ARG for levels of 0 or more than L_max, a
 * row stride smaller than a row, (n_images > 1) image strides smaller than an image / a chain, a workspace smaller than
 * icamd_bptc_mip_workspace_size, or BC6H's odd pointers and strides; ICAMD_OK for n_images == 0.  Then ICAMD_ERR_NO_DEVICE
 * without a GPU.  No allocation, no synchronisation: it can be captured on one stream. */
/* Bytes of one image's chain; fills level_offsets[0 .. levels] when non-NULL.  0 for every other codec, an empty image or
 * levels outside 1 .. L_max. */
size_t icamd_bptc_mip_chain_size(int codec, uint32_t height, uint32_t width, uint32_t levels, size_t *level_offsets);
/* src_channels: bytes (BC7) or halves (BC6H) per source pixel.  0 also for arguments the encode refuses. */
size_t icamd_bptc_mip_workspace_size(int codec, int src_channels, uint32_t height, uint32_t width, uint32_t levels,
                                     uint32_t n_images);
int icamd_encode_bc7_mips_device(int bc7_modes, int src_components, int swap_rb, int filter, uint32_t height, uint32_t width,
                                 uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images,
                                 size_t src_image_stride_bytes, size_t dst_image_stride_bytes, const void *d_src, void *d_dst,
                                 void *d_workspace, size_t workspace_bytes, void *hip_stream);
int icamd_encode_bc6h_mips_device(int codec, int bc6h_modes, int src_channels, uint32_t height, uint32_t width,
                                  uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images,
                                  size_t src_image_stride_bytes, size_t dst_image_stride_bytes, const void *d_src, void *d_dst,
                                  void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* Name of the __global__ kernel of the encode launch: modes is ICAMD_BC7_MODES_* / ICAMD_BC6H_MODES_*; "" for combinations
 * the encode refuses. */
const char *icamd_bptc_mip_kernel_name(int codec, int src_channels, int modes);

/* ---- runtime ---- */
int icamd_device_count(void);             /* HIP devices visible; 0 if none */
const char *icamd_last_error(void);       /* thread-local message for the last negative status */
const char *icamd_version(void);
/* Name of the __global__ kernel a given configuration launches (for matching rocprofv3 rows). */
const char *icamd_kernel_name(int codec, int src_components);

/* ---- diagnostics (measurement aid; not part of the encode path) ----
 * Effective shader clock under load: enqueues ONE wave on hip_stream that sleeps for duration_us and then writes
 * {shader cycles elapsed (s_memtime), constant-rate ticks elapsed (s_memrealtime)} as two uint64 to d_out16.  Run it
 * on a stream of its own next to the kernels being timed; mean clock = cycles / ticks * icamd_wall_clock_rate_khz().
 * duration_us above ICAMD_CLOCK_PROBE_MAX_US is refused with ICAMD_ERR_ARG. */
#define ICAMD_CLOCK_PROBE_MAX_US 10000000u
int icamd_clock_probe_device(void *d_out16, uint32_t duration_us, void *hip_stream);
uint32_t icamd_wall_clock_rate_khz(void);  /* hipDeviceAttributeWallClockRate of the current device; 0 if unknown */

#ifdef __cplusplus
}
#endif
#endif /* IC_AMD_H_ */
