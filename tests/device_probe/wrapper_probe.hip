// TEST INFRASTRUCTURE ONLY.  wrapper_probe IN OUT: applies the DEVICE form of every instruction wrapper of
// image-compression_amd/csrc (the list of wrapper_ops.h) to operands read from IN and writes the results to OUT; one kernel per
// op, the operands loaded from memory so that nothing folds at compile time.  tests/test_gpu_wrappers.py compares the results
// with the host twins (tests/host_emul/wrapper_emul.cc) and the plain definitions (tests/wrapper_cases.py).  Every HIP call is
// checked and every kernel is followed by a synchronise; any error ends the program with a non-zero status.
//
// Both files are sequences of little-endian uint32 sections, ended by a 0:
//   IN   1 op n  a b c ...                      OUT  1 op n  r ...              r[i] = the op on case i
//        2 n  (exit_lo exit_hi pred_lo pred_hi) ...  2 n  (all[64] count[64]) ...   wave_all / wave_count; exited lanes: 0xffffffff
//        3  v[64]                                    3  xor1[64] xor2[64]           quad_xor1 / quad_xor2
//        4                                           4  (count guess[count] settled[count]) x 3
//                                                       normal_isqrt<0>(4 rem), rem 0 .. 65025; normal_isqrt<0>(n2 << 8),
//                                                       n2 0 .. 3 * 1020^2; normal_div<0>(4080 a + (Ls >> 1), Ls),
//                                                       a 0 .. 1020 (slow) x Ls 16 .. 28267 (fast)
// This file is compiled twice: as it is, and with -DICAMD_PVRTC_NO_SCAN_SDWA -DWRAPPER_PROBE_PLAIN_SCAN for the second build of
// scan_into_byte (ops kOp_scan_plain_b0 ..), which leaves only run_plain_scan().
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "wrapper_ops.h"

using namespace icamd_probe;

#define HIP_OK(call)                                                                             \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      fprintf(stderr, "wrapper_probe: %s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(2);                                                                                   \
    }                                                                                            \
  } while (0)

// the scan of list position `which` (0 .. 3) in this build's form
__device__ __forceinline__ uint32_t scan_apply(int which, uint32_t a, uint32_t b, uint32_t c) {
  switch (which) {
#define ICAMD_X(id, name, arity, header, expr) case kOp_##id - kOp_scan_b0: return (expr);
    ICAMD_WRAPPER_SCAN_OPS(ICAMD_X)
#undef ICAMD_X
  }
  return 0xdeadbeefu;
}

#if defined(WRAPPER_PROBE_PLAIN_SCAN)

template <int WHICH>
__global__ void plain_scan_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = scan_apply(WHICH, in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]);
}
void run_plain_scan(int which, const uint32_t *d_in, uint32_t *d_out, uint32_t n) {
  const dim3 grid((n + 255u) / 256u), block(256);
  switch (which) {
    case 0: plain_scan_kernel<0><<<grid, block>>>(d_in, d_out, n); break;
    case 1: plain_scan_kernel<1><<<grid, block>>>(d_in, d_out, n); break;
    case 2: plain_scan_kernel<2><<<grid, block>>>(d_in, d_out, n); break;
    default: plain_scan_kernel<3><<<grid, block>>>(d_in, d_out, n); break;
  }
}

#else

void run_plain_scan(int which, const uint32_t *d_in, uint32_t *d_out, uint32_t n);

template <int OP>
__global__ void op_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = wrapper_apply(OP, in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]);
}
typedef void (*OpKernel)(const uint32_t *, uint32_t *, uint32_t);
static const OpKernel kOpKernels[kOpCount] = {
#define ICAMD_X(id, name, arity, header, expr) op_kernel<kOp_##id>,
  ICAMD_WRAPPER_OPS(ICAMD_X)
#undef ICAMD_X
};

// One wave.  masks[4 c ..]: exit mask and predicate mask of case c, 64 bits each.  A lane whose exit bit is set returns before
// the votes; out[128 c + lane] = wave_all, out[128 c + 64 + lane] = wave_count as the lane saw them.
__global__ void vote_kernel(const uint32_t *__restrict__ masks, uint32_t *__restrict__ out, uint32_t c) {
  const uint32_t lane = threadIdx.x;
  const uint32_t ex = masks[4 * c + (lane >> 5)], pr = masks[4 * c + 2 + (lane >> 5)];
  if ((ex >> (lane & 31u)) & 1u) return;
  const bool p = ((pr >> (lane & 31u)) & 1u) != 0u;
  out[128 * c + lane] = wave_all(p) ? 1u : 0u;
  out[128 * c + 64 + lane] = wave_count(p);
}
__global__ void quad_kernel(const uint32_t *__restrict__ v, uint32_t *__restrict__ out) {
  const uint32_t lane = threadIdx.x;
  out[lane] = quad_xor1(v[lane]);
  out[64 + lane] = quad_xor2(v[lane]);
}

// The float first guesses of normal_isqrt<0> / normal_div<0> (mip_normal.h: the functions they call), next to the settled results.
// MODE 0: n = 4 i; 1: n = i << 8; 2: i = a * n_ls + (Ls - 16), n = 4080 a + (Ls >> 1), d = Ls.
template <int MODE>
__global__ void guess_kernel(uint32_t *__restrict__ guess, uint32_t *__restrict__ settled, uint32_t count, uint32_t n_ls) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if (MODE == 2) {
    const uint32_t a = i / n_ls, Ls = 16u + i % n_ls;
    const uint32_t n = 4080u * a + (Ls >> 1);
    guess[i] = normal_div_guess(n, Ls);
    settled[i] = normal_div<0>(n, Ls);
  } else {
    const uint32_t n = MODE == 0 ? 4u * i : i << 8;
    guess[i] = normal_isqrt_guess(n);
    settled[i] = normal_isqrt<0>(n);
  }
}

static FILE *g_in, *g_out;
static uint32_t read_u32() {
  uint32_t v;
  if (fread(&v, 4, 1, g_in) != 1) { fprintf(stderr, "wrapper_probe: the input ends inside a section\n"); exit(3); }
  return v;
}
static void read_words(uint32_t *p, size_t n) {
  if (n && fread(p, 4, n, g_in) != n) { fprintf(stderr, "wrapper_probe: the input ends inside a section\n"); exit(3); }
}
static void write_words(const uint32_t *p, size_t n) {
  if (n && fwrite(p, 4, n, g_out) != n) { fprintf(stderr, "wrapper_probe: cannot write the output\n"); exit(4); }
}
static void write_u32(uint32_t v) { write_words(&v, 1); }

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: wrapper_probe IN OUT\n"); return 1; }
  g_in = fopen(argv[1], "rb");
  g_out = fopen(argv[2], "wb");
  if (!g_in || !g_out) { fprintf(stderr, "wrapper_probe: cannot open %s\n", !g_in ? argv[1] : argv[2]); return 1; }
  const uint32_t kMaxCases = 1u << 22;
  std::vector<uint32_t> host;
  for (;;) {
    const uint32_t tag = read_u32();
    if (tag == 0u) break;
    write_u32(tag);
    if (tag == 1u) {
      const uint32_t op = read_u32(), n = read_u32();
      if (op >= (uint32_t)kOpCountBoth || n == 0u || n > kMaxCases) { fprintf(stderr, "wrapper_probe: op %u with %u cases\n", op, n); return 3; }
      host.resize(3 * (size_t)n);
      read_words(host.data(), host.size());
      if (op == (uint32_t)kOp_fastdiv) prepare_fastdiv(host.data(), n);
      uint32_t *d_in, *d_out;
      HIP_OK(hipMalloc(&d_in, 12 * (size_t)n));
      HIP_OK(hipMalloc(&d_out, 4 * (size_t)n));
      HIP_OK(hipMemcpy(d_in, host.data(), 12 * (size_t)n, hipMemcpyHostToDevice));
      HIP_OK(hipMemset(d_out, 0xEE, 4 * (size_t)n));
      if (op >= (uint32_t)kOpCount) run_plain_scan((int)op - kOpCount, d_in, d_out, n);
      else kOpKernels[op]<<<dim3((n + 255u) / 256u), dim3(256)>>>(d_in, d_out, n);
      HIP_OK(hipGetLastError());
      HIP_OK(hipDeviceSynchronize());
      host.resize(n);
      HIP_OK(hipMemcpy(host.data(), d_out, 4 * (size_t)n, hipMemcpyDeviceToHost));
      HIP_OK(hipFree(d_in));
      HIP_OK(hipFree(d_out));
      write_u32(op);
      write_u32(n);
      write_words(host.data(), n);
    } else if (tag == 2u) {
      const uint32_t n = read_u32();
      if (n == 0u || n > 4096u) { fprintf(stderr, "wrapper_probe: %u vote cases\n", n); return 3; }
      host.resize(4 * (size_t)n);
      read_words(host.data(), host.size());
      uint32_t *d_in, *d_out;
      HIP_OK(hipMalloc(&d_in, 16 * (size_t)n));
      HIP_OK(hipMalloc(&d_out, 512 * (size_t)n));
      HIP_OK(hipMemcpy(d_in, host.data(), 16 * (size_t)n, hipMemcpyHostToDevice));
      HIP_OK(hipMemset(d_out, 0xFF, 512 * (size_t)n));
      for (uint32_t c = 0; c < n; ++c) {
        vote_kernel<<<dim3(1), dim3(64)>>>(d_in, d_out, c);
        HIP_OK(hipGetLastError());
      }
      HIP_OK(hipDeviceSynchronize());
      host.resize(128 * (size_t)n);
      HIP_OK(hipMemcpy(host.data(), d_out, 512 * (size_t)n, hipMemcpyDeviceToHost));
      HIP_OK(hipFree(d_in));
      HIP_OK(hipFree(d_out));
      write_u32(n);
      write_words(host.data(), host.size());
    } else if (tag == 3u) {
      host.resize(64);
      read_words(host.data(), 64);
      uint32_t *d_in, *d_out;
      HIP_OK(hipMalloc(&d_in, 256));
      HIP_OK(hipMalloc(&d_out, 512));
      HIP_OK(hipMemcpy(d_in, host.data(), 256, hipMemcpyHostToDevice));
      HIP_OK(hipMemset(d_out, 0xEE, 512));
      quad_kernel<<<dim3(1), dim3(64)>>>(d_in, d_out);
      HIP_OK(hipGetLastError());
      HIP_OK(hipDeviceSynchronize());
      host.resize(128);
      HIP_OK(hipMemcpy(host.data(), d_out, 512, hipMemcpyDeviceToHost));
      HIP_OK(hipFree(d_in));
      HIP_OK(hipFree(d_out));
      write_words(host.data(), 128);
    } else if (tag == 4u) {
      const uint32_t n_ls = 28267u - 16u + 1u;
      const uint32_t counts[3] = { 65025u + 1u, 3u * 1020u * 1020u + 1u, 1021u * n_ls };
      for (int mode = 0; mode < 3; ++mode) {
        const uint32_t count = counts[mode];
        uint32_t *d_guess, *d_settled;
        HIP_OK(hipMalloc(&d_guess, 4 * (size_t)count));
        HIP_OK(hipMalloc(&d_settled, 4 * (size_t)count));
        HIP_OK(hipMemset(d_guess, 0xEE, 4 * (size_t)count));
        HIP_OK(hipMemset(d_settled, 0xEE, 4 * (size_t)count));
        const dim3 grid((count + 255u) / 256u), block(256);
        if (mode == 0) guess_kernel<0><<<grid, block>>>(d_guess, d_settled, count, n_ls);
        else if (mode == 1) guess_kernel<1><<<grid, block>>>(d_guess, d_settled, count, n_ls);
        else guess_kernel<2><<<grid, block>>>(d_guess, d_settled, count, n_ls);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        write_u32(count);
        host.resize(count);
        HIP_OK(hipMemcpy(host.data(), d_guess, 4 * (size_t)count, hipMemcpyDeviceToHost));
        write_words(host.data(), count);
        HIP_OK(hipMemcpy(host.data(), d_settled, 4 * (size_t)count, hipMemcpyDeviceToHost));
        write_words(host.data(), count);
        HIP_OK(hipFree(d_guess));
        HIP_OK(hipFree(d_settled));
      }
    } else {
      fprintf(stderr, "wrapper_probe: unknown section %u\n", tag);
      return 3;
    }
  }
  write_u32(0u);
  if (fclose(g_out) != 0) { fprintf(stderr, "wrapper_probe: cannot write the output\n"); return 4; }
  fclose(g_in);
  printf("wrapper_probe: done\n");
  return 0;
}

#endif  // WRAPPER_PROBE_PLAIN_SCAN
