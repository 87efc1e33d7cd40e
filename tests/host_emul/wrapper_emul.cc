// TEST INFRASTRUCTURE ONLY.  The wrapper list of tests/device_probe/wrapper_ops.h compiled for the HOST
// (g++ -DICAMD_HOST_EMULATION): every op applies the wrapper's TWIN form.  tests/test_wrappers_host.py checks the twins against
// the plain definitions of tests/wrapper_cases.py and against the device's recorded hashes; tests/test_gpu_wrappers.py holds
// them against the device form case by case.  Never linked into libic_amd.so.
#ifndef ICAMD_HOST_EMULATION
#error "build with -DICAMD_HOST_EMULATION"
#endif
#include <vector>

#include "../device_probe/wrapper_ops.h"
#include "emul_violations.h"

using namespace icamd_probe;

extern "C" int wrapper_emul_op_count(void) { return kOpCount; }
extern "C" const char *wrapper_emul_op_id(int op) {
  switch (op) {
#define ICAMD_X(id, name, arity, header, expr) case kOp_##id: return #id;
    ICAMD_WRAPPER_OPS(ICAMD_X)
#undef ICAMD_X
  }
  return "";
}

// out[i] = the op's twin on operands[3 i .. 3 i + 2]; returns 0 for an op the list does not have
extern "C" int wrapper_emul_apply(int op, uint32_t n, const uint32_t *operands, uint32_t *out) {
  if (op < 0 || op >= kOpCount) return 0;
  std::vector<uint32_t> t(operands, operands + 3 * (size_t)n);
  if (op == kOp_fastdiv) prepare_fastdiv(t.data(), n);
  for (uint32_t i = 0; i < n; ++i) out[i] = wrapper_apply(op, t[3 * (size_t)i], t[3 * (size_t)i + 1], t[3 * (size_t)i + 2]);
  return 1;
}

// flag[i] = 1 iff the twin counted case i as outside the wrapper's domain (the counter is left where it was)
extern "C" int wrapper_emul_flags(int op, uint32_t n, const uint32_t *operands, uint8_t *flag) {
  if (op < 0 || op >= kOpCount) return 0;
  std::vector<uint32_t> t(operands, operands + 3 * (size_t)n);
  if (op == kOp_fastdiv) prepare_fastdiv(t.data(), n);
  const icamd::emul::Violations &v = icamd::emul::violations();
  char first[sizeof v.first];
  memcpy(first, v.first, sizeof first);
  first[sizeof first - 1] = 0;
  const unsigned long long before = v.count.load();
  for (uint32_t i = 0; i < n; ++i) {
    const unsigned long long c0 = v.count.load();
    (void)wrapper_apply(op, t[3 * (size_t)i], t[3 * (size_t)i + 1], t[3 * (size_t)i + 2]);
    flag[i] = v.count.load() != c0;
  }
  icamd::emul::restore_violations(before, first);
  return 1;
}

// The float guesses of mip_normal.h as the host forms them, and the settled results: n[i] (and d[i]) -> guess[i], settled[i].
extern "C" void wrapper_emul_isqrt(uint32_t count, const uint32_t *n, uint32_t *guess, uint32_t *settled) {
  for (uint32_t i = 0; i < count; ++i) {
    guess[i] = normal_isqrt_guess(n[i]);
    settled[i] = normal_isqrt<0>(n[i]);
  }
}
extern "C" void wrapper_emul_div(uint32_t count, const uint32_t *n, const uint32_t *d, uint32_t *guess, uint32_t *settled) {
  for (uint32_t i = 0; i < count; ++i) {
    guess[i] = normal_div_guess(n[i], d[i]);
    settled[i] = normal_div<0>(n[i], d[i]);
  }
}
