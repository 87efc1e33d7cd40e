// TEST INFRASTRUCTURE ONLY.  The one list of the instruction wrappers of image-compression_amd/csrc: every wrapper that has a
// device form (a gfx950 instruction or builtin) and a host twin (-DICAMD_HOST_EMULATION) has one line here, and the line is
// compiled twice -- by hipcc into tests/device_probe/wrapper_probe.hip, where it applies the DEVICE form on an MI355X, and by
// g++ into tests/host_emul/wrapper_emul.cc, where it applies the TWIN.  tests/test_gpu_wrappers.py holds the two results
// together; tests/test_wrappers_host.py checks that no wrapper of csrc/*.h is missing from the list (it parses the X(...) lines
// below: keep one per line).  The wrappers themselves come from the csrc headers; nothing is copied here.
//
// X(id, "wrapper", arity, "header that defines it", expression over the uint32_t operands a, b, c)
//   The id is the op's name in tests/wrapper_cases.py, and its position in the list is its number in the probe's files.
#ifndef ICAMD_TESTS_WRAPPER_OPS_H_
#define ICAMD_TESTS_WRAPPER_OPS_H_

#include "dxt_block.h"
#include "etc1_block.h"
#include "decode_block.h"
#include "pvrtc_walk.h"
#include "transcode5_block.h"
#include "mip_normal.h"

namespace icamd_probe {
using namespace icamd;

// fastdiv takes a host-made FastDiv: the operands (n, d, -) of a case are rewritten to (n, mul, shift) on the host of both
// builds before the op runs.  d = 0 has no FastDiv; it runs as mul 0, shift 32, which the instruction reads as a shift of 0.
inline void prepare_fastdiv(uint32_t *triples, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t *t = triples + 3 * (size_t)i;
    FastDiv f = { 0u, 32u, 0u };
    if (t[1] != 0u) f = make_fastdiv(t[1]);
    t[1] = f.mul;
    t[2] = f.shift;
  }
}
ICAMD_DEV uint32_t apply_fastdiv(uint32_t n, uint32_t mul, uint32_t shift) {
  FastDiv f;
  f.mul = mul;
  f.shift = shift;
  f.d = 0u;
  return fastdiv(n, f);
}
// the six operands of scan_into_byte from three: d0 | d1 << 16, d2 | d3 << 16, acc; the unit is the op's own
ICAMD_DEV uint32_t apply_scan(uint32_t a, uint32_t b, uint32_t unit, uint32_t acc) {
  return scan_into_byte(a & 0xffffu, a >> 16, b & 0xffffu, b >> 16, unit, acc);
}

// scan_into_byte has two device builds (pvrtc_pixel.h): the probe compiles this part a second time with
// -DICAMD_PVRTC_NO_SCAN_SDWA and runs those four under the ids scan_plain_b0 .. scan_plain_b3 (numbers after the list's).
#define ICAMD_WRAPPER_SCAN_OPS(X)                                                  \
  X(scan_b0, "scan_into_byte", 3, "pvrtc_pixel.h", apply_scan(a, b, 1u, c))        \
  X(scan_b1, "scan_into_byte", 3, "pvrtc_pixel.h", apply_scan(a, b, 1u << 8, c))   \
  X(scan_b2, "scan_into_byte", 3, "pvrtc_pixel.h", apply_scan(a, b, 1u << 16, c))  \
  X(scan_b3, "scan_into_byte", 3, "pvrtc_pixel.h", apply_scan(a, b, 1u << 24, c))

#define ICAMD_WRAPPER_OPS(X)                                                                      \
  X(umulhi32, "umulhi32", 2, "ic_device.h", umulhi32(a, b))                                      \
  X(udot4, "udot4", 3, "ic_device.h", udot4(a, b, c))                                            \
  X(sad_u32, "sad_u32", 3, "ic_device.h", sad_u32(a, b, c))                                      \
  X(sad_u16x2, "sad_u16x2", 3, "ic_device.h", sad_u16x2(a, b, c))                                \
  X(sad_u8, "sad_u8", 3, "ic_device.h", sad_u8(a, b, c))                                         \
  X(sad_hi_u8, "sad_hi_u8", 3, "ic_device.h", sad_hi_u8(a, b, c))                                \
  X(alignbit, "alignbit", 3, "ic_device.h", alignbit(a, b, c))                                   \
  X(avg_u8, "avg_u8", 2, "ic_device.h", avg_u8(a, b))                                            \
  X(perm, "perm", 3, "ic_device.h", perm(a, b, c))                                               \
  X(bfe, "bfe", 3, "ic_device.h", bfe(a, b, c))                                                  \
  X(bit_mask, "bit_mask", 2, "ic_device.h", bit_mask(a, b))                                      \
  X(imad24, "imad24", 3, "ic_device.h", (uint32_t)imad24((int32_t)a, (int32_t)b, (int32_t)c))    \
  X(umad24, "umad24", 3, "ic_device.h", umad24(a, b, c))                                         \
  X(umin, "umin", 2, "ic_device.h", umin(a, b))                                                  \
  X(umax, "umax", 2, "ic_device.h", umax(a, b))                                                  \
  X(imin, "imin", 2, "ic_device.h", (uint32_t)imin((int32_t)a, (int32_t)b))                      \
  X(imax, "imax", 2, "ic_device.h", (uint32_t)imax((int32_t)a, (int32_t)b))                      \
  X(fastdiv, "fastdiv", 2, "ic_device.h", apply_fastdiv(a, b, c))                                \
  X(pk_addsat_u16, "pk_addsat_u16", 2, "etc1_block.h", pk_addsat_u16(a, b))                      \
  X(pk_subsat_u16, "pk_subsat_u16", 2, "etc1_block.h", pk_subsat_u16(a, b))                      \
  X(udot2_u16, "udot2_u16", 3, "etc1_block.h", udot2_u16(a, b, c))                               \
  X(pk_sub_u16, "pk_sub_u16", 2, "dxt_block.h", pk_sub_u16(a, b))                                \
  X(pk_min_u16, "pk_min_u16", 2, "dxt_block.h", pk_min_u16(a, b))                                \
  X(pk_max_u16, "pk_max_u16", 2, "dxt_block.h", pk_max_u16(a, b))                                \
  X(pk_lshr16, "pk_lshr16", 2, "dxt_block.h", pk_lshr16(a, b))                                   \
  X(pk_mad_u16, "pk_mad_u16", 3, "dxt_block.h", pk_mad_u16(a, b, c))                             \
  X(pk_mad_u16_lane0, "pk_mad_u16_lane", 3, "decode_block.h", pk_mad_u16_lane<0>(a, b, c))       \
  X(pk_mad_u16_lane1, "pk_mad_u16_lane", 3, "decode_block.h", pk_mad_u16_lane<1>(a, b, c))       \
  X(popcount_u32, "popcount_u32", 1, "pvrtc_pixel.h", popcount_u32(a))                           \
  X(pack64, "pack64", 3, "pvrtc_walk.h", (uint32_t)(pack64(a, b) >> (c & 63u)))                  \
  X(lo32, "lo32", 3, "pvrtc_walk.h", lo32(((icamd_u64)b << 32 | a) + c))                         \
  X(hi32, "hi32", 3, "pvrtc_walk.h", hi32(((icamd_u64)b << 32 | a) + c))                         \
  X(popc32, "popc32", 1, "transcode5_block.h", popc32(a))                                        \
  ICAMD_WRAPPER_SCAN_OPS(X)

// The wrappers that are no function of three operands: they have sections of their own in the probe's files.
// Y(id, "wrapper", arity, "header", what the probe runs)
#define ICAMD_WRAPPER_FLOAT_OPS(Y)                                                                                   \
  Y(normal_isqrt_guess, "normal_isqrt_guess", 1, "mip_normal.h", "the truncated v_sqrt_f32 guess")                  \
  Y(normal_div_guess, "normal_div_guess", 2, "mip_normal.h", "the truncated v_rcp_f32 guess")                       \
  Y(normal_isqrt, "normal_isqrt", 1, "mip_normal.h", "normal_isqrt<0>(n), settled from that guess")                  \
  Y(normal_div, "normal_div", 2, "mip_normal.h", "normal_div<0>(n, d), settled from that guess")
#define ICAMD_WRAPPER_LANE_OPS(Y)                                                                 \
  Y(wave_all, "wave_all", 1, "ic_device.h", "one wave of 64, some lanes returned early")         \
  Y(wave_count, "wave_count", 1, "ic_device.h", "one wave of 64, some lanes returned early")     \
  Y(quad_xor1, "quad_xor1", 1, "etc1_block.h", "one wave of 64 in full quads")                    \
  Y(quad_xor2, "quad_xor2", 1, "etc1_block.h", "one wave of 64 in full quads")

enum WrapperOp {
#define ICAMD_X(id, name, arity, header, expr) kOp_##id,
  ICAMD_WRAPPER_OPS(ICAMD_X)
#undef ICAMD_X
  kOpCount,
  // the second build of the scan
  kOp_scan_plain_b0 = kOpCount, kOp_scan_plain_b1, kOp_scan_plain_b2, kOp_scan_plain_b3, kOpCountBoth
};

// The op's wrapper on one case, in whichever form this build selects.
ICAMD_DEV uint32_t wrapper_apply(int op, uint32_t a, uint32_t b, uint32_t c) {
  switch (op) {
#define ICAMD_X(id, name, arity, header, expr) case kOp_##id: return (expr);
    ICAMD_WRAPPER_OPS(ICAMD_X)
#undef ICAMD_X
  }
  return 0xdeadbeefu;
}

}  // namespace icamd_probe
#endif  // ICAMD_TESTS_WRAPPER_OPS_H_
