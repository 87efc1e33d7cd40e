// r05 micro-benchmark (gfx950): what the HBM delivers to the plainest streaming kernels over 1 GiB -- read only (non-temporal and
// plain dwordx4 loads, 16 B per lane and instruction, 1 / 4 loads in flight per lane), write only (non-temporal / plain), copy
// (float4, the figure MI355X_MICROARCH.md quotes), and a read : write mix of 8 : 1 like DXT1 from RGBA8 -- the ceiling the
// roofline fractions of the memory-bound encoders should be read against.  r07 adds the parts of that mix (no stores, a linear read,
// 16-byte stores, XCD-consecutive tiles, one workgroup per block-row span) and store cache policies, each also timed with an event
// in front of every launch as bench.py does (profiles/r07_ab_dxt1_store_policy.log).
// Build: hipcc --offload-arch=gfx950 -O3 scripts/ubench_hbm.hip -o scripts/scratch/ubench_hbm
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));
template <bool NT> __device__ inline u4 ld(const u4 *p) { return NT ? __builtin_nontemporal_load(p) : *p; }
template <bool NT> __device__ inline void st(u4 *p, u4 v) { if (NT) __builtin_nontemporal_store(v, p); else *p = v; }
// each workgroup streams UNROLL x 256 x 16 bytes
template <bool NT, int UNROLL> __global__ void __launch_bounds__(256) k_read(const u4 *src, u4 *sink, uint32_t n16) {
  const uint32_t base = blockIdx.x * (256u * UNROLL) + threadIdx.x;
  u4 acc = { 0, 0, 0, 0 };
#pragma unroll
  for (int i = 0; i < UNROLL; ++i) { const uint32_t k = base + i * 256u; if (k < n16) acc ^= ld<NT>(src + k); }
  if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) sink[threadIdx.x] = acc;  // (never: keeps the loads)
}
template <bool NT, int UNROLL> __global__ void __launch_bounds__(256) k_write(u4 *dst, uint32_t n16, uint32_t seed) {
  const uint32_t base = blockIdx.x * (256u * UNROLL) + threadIdx.x;
#pragma unroll
  for (int i = 0; i < UNROLL; ++i) { const uint32_t k = base + i * 256u; if (k < n16) st<NT>(dst + k, (u4){ k, seed, k ^ seed, 7u }); }
}
template <bool NT, int UNROLL> __global__ void __launch_bounds__(256) k_copy(const u4 *src, u4 *dst, uint32_t n16) {
  const uint32_t base = blockIdx.x * (256u * UNROLL) + threadIdx.x;
  u4 v[UNROLL];
#pragma unroll
  for (int i = 0; i < UNROLL; ++i) { const uint32_t k = base + i * 256u; v[i] = k < n16 ? ld<NT>(src + k) : (u4){ 0, 0, 0, 0 }; }
#pragma unroll
  for (int i = 0; i < UNROLL; ++i) { const uint32_t k = base + i * 256u; if (k < n16) st<NT>(dst + k, v[i]); }
}
// 8 : 1 like DXT1 <- RGBA8: a lane reads 64 bytes (4 x 16, rows of a 4 x 4-pixel block 16 KiB apart) and writes 8
// stride16: distance between pixel rows in 16-byte units (= row16 for a dense image; larger = padded rows)
__global__ void __launch_bounds__(256) k_mix(const u4 *src, u2 *dst, uint32_t n_blocks, uint32_t row16, uint32_t stride16) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n_blocks) return;
  const uint32_t brow = k / row16, bcol = k - brow * row16;  // row16 = blocks per row
  const u4 *p = src + (size_t)brow * 4u * stride16 + bcol;
  u4 a = __builtin_nontemporal_load(p), b = __builtin_nontemporal_load(p + stride16), c = __builtin_nontemporal_load(p + 2 * stride16),
     d = __builtin_nontemporal_load(p + 3 * stride16);
  a ^= b; c ^= d; a ^= c;
  __builtin_nontemporal_store((u2){ a.x ^ a.y, a.z ^ a.w }, dst + k);
}
// the same bytes with ONE load per lane: lane t of a quad reads pixel row t of its block, lane 0 of the quad writes the 8 bytes
// (quad-xor'ed so that the loads are kept).  MODE 0: the quad = 4 adjacent lanes; MODE 1: row t of a wave's 16 blocks in lanes 16 t .. 16 t + 15
template <int MODE> __global__ void __launch_bounds__(256) k_mix_quad(const u4 *src, u2 *dst, uint32_t n_blocks, uint32_t row16) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  uint32_t k, t;
  if (MODE == 0) { k = g >> 2; t = g & 3u; }
  else { const uint32_t wave = g >> 6, lane = g & 63u; k = wave * 16u + (lane & 15u); t = lane >> 4; }
  if (k >= n_blocks) return;
  const uint32_t brow = k / row16, bcol = k - brow * row16;
  u4 a = __builtin_nontemporal_load(src + ((size_t)brow * 4u + t) * row16 + bcol);
  uint32_t x = a.x ^ a.y, y = a.z ^ a.w;
  if (MODE == 0) {
    x ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xb1, 0xf, 0xf, true); y ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)y, 0xb1, 0xf, 0xf, true);
    x ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4e, 0xf, 0xf, true); y ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)y, 0x4e, 0xf, 0xf, true);
  } else {
    x ^= (uint32_t)__shfl_xor((int)x, 16); y ^= (uint32_t)__shfl_xor((int)y, 16);
    x ^= (uint32_t)__shfl_xor((int)x, 32); y ^= (uint32_t)__shfl_xor((int)y, 32);
  }
  if (t == 0u) __builtin_nontemporal_store((u2){ x, y }, dst + k);
}

// ---- r07: splitting the "mix 8 : 1" shape into its parts (16 x 4096^2 RGBA8 = 1 GiB in, 8 B per 4 x 4 block out) ----
// XCD: workgroup b runs on XCD b % 8; XCD_SWZ hands XCD x the x-th eighth of the tiles in order, so the workgroups resident on one
// XCD at the same time read consecutive tiles (n_wg % 8 == 0)
template <bool XCD_SWZ> __device__ inline uint32_t wg_id(uint32_t n_wg) {
  const uint32_t b = blockIdx.x;
  return XCD_SWZ ? (b & 7u) * (n_wg >> 3) + (b >> 3) : b;
}
// WT: the store's cache policy.  0: non-temporal (nt, store_stream8); 1: written through to memory (sc0 sc1, a system-scope relaxed
// store); 2: sc1 (an agent-scope relaxed store); 3 / 4: buffer stores with sc0 sc1 nt / sc0 set through the builtin's policy operand
template <int WT> __device__ inline void st8(u2 *p, u2 v) {
  if (WT == 1) __hip_atomic_store(reinterpret_cast<uint64_t *>(p), (uint64_t)v.x | (uint64_t)v.y << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else if (WT == 2) __hip_atomic_store(reinterpret_cast<uint64_t *>(p), (uint64_t)v.x | (uint64_t)v.y << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else if (WT >= 3) {
    // workgroup-uniform base (the workgroup's 2 KiB of output), lane offset in bytes
    u2 *base = p - threadIdx.x;
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7fffffff, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b64(v, r, (int)(threadIdx.x * 8u), 0, WT == 3 ? 19 : 1);
  } else __builtin_nontemporal_store(v, p);
}
// the mix shape (k_mix, 4096-pixel rows); STORE = 0: no stores (kept loads), 1: 8 B per lane, 2: 16 B from every even lane (its block
// and its neighbour's), WT / XCD_SWZ as above
// LANES: the workgroup's size (r08: the same waves launched as 128- or 64-lane workgroups, grid = n_blocks / LANES)
template <int STORE, int WT, bool XCD_SWZ, int LANES = 256> __global__ void __launch_bounds__(LANES) k_mix2(const u4 *src, u2 *dst, uint32_t n_blocks) {
  const uint32_t k = wg_id<XCD_SWZ>(gridDim.x) * (uint32_t)LANES + threadIdx.x, row16 = 1024u;
  const uint32_t brow = k >> 10, bcol = k & 1023u;
  const u4 *p = src + (size_t)brow * 4u * row16 + bcol;
  u4 a = __builtin_nontemporal_load(p), b = __builtin_nontemporal_load(p + row16), c = __builtin_nontemporal_load(p + 2 * row16),
     d = __builtin_nontemporal_load(p + 3 * row16);
  a ^= b; c ^= d; a ^= c;
  const u2 v = { a.x ^ a.y, a.z ^ a.w };
  if (STORE == 0) { if ((v.x ^ v.y) == 0x12345678u) dst[k] = v; }
  else if (STORE == 1) st8<WT>(dst + k, v);
  else {
    const uint32_t nx = (uint32_t)__shfl_xor((int)v.x, 1), ny = (uint32_t)__shfl_xor((int)v.y, 1);
    if ((threadIdx.x & 1u) == 0u) __builtin_nontemporal_store((u4){ v.x, v.y, nx, ny }, reinterpret_cast<u4 *>(dst + k));
  }
}
// linear read (a workgroup streams 16 KiB: 4 x 4 KiB, k_read<true, 4>) + an 8-byte store per lane
__global__ void __launch_bounds__(256) k_lin_st8(const u4 *src, u2 *dst, uint32_t n_blocks) {
  const uint32_t base = blockIdx.x * 1024u + threadIdx.x;
  u4 a = __builtin_nontemporal_load(src + base), b = __builtin_nontemporal_load(src + base + 256u),
     c = __builtin_nontemporal_load(src + base + 512u), d = __builtin_nontemporal_load(src + base + 768u);
  a ^= b; c ^= d; a ^= c;
  __builtin_nontemporal_store((u2){ a.x ^ a.y, a.z ^ a.w }, dst + blockIdx.x * 256u + threadIdx.x);
}
// one workgroup per 64 KiB block row of a 4096-pixel texture (1 024 blocks): load 4 r + q (q = 0..3) of lane l is pixel row r of
// block q * 256 + l, so the workgroup reads its span linearly (16 x 4 KiB) with no transpose, and writes 4 x 2 KiB = 8 KiB
// contiguously.  PIPE: the blocks are taken one at a time (4 loads, then the store) instead of all 16 loads first.
template <bool XCD_SWZ, bool PIPE> __global__ void __launch_bounds__(256) k_span(const u4 *src, u2 *dst, uint32_t n_blocks) {
  const uint32_t brow = wg_id<XCD_SWZ>(gridDim.x), l = threadIdx.x;
  const u4 *p = src + (size_t)brow * 4096u + l;
  u2 *q = dst + (size_t)brow * 1024u + l;
  if (PIPE) {
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      u4 a = __builtin_nontemporal_load(p + 256 * j), b = __builtin_nontemporal_load(p + 1024 + 256 * j),
         c = __builtin_nontemporal_load(p + 2048 + 256 * j), d = __builtin_nontemporal_load(p + 3072 + 256 * j);
      a ^= b; c ^= d; a ^= c;
      __builtin_nontemporal_store((u2){ a.x ^ a.y, a.z ^ a.w }, q + 256 * j);
    }
  } else {
    u4 v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = __builtin_nontemporal_load(p + 256 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      u4 a = v[j] ^ v[4 + j] ^ v[8 + j] ^ v[12 + j];
      __builtin_nontemporal_store((u2){ a.x ^ a.y, a.z ^ a.w }, q + 256 * j);
    }
  }
}
template <typename F> double timeit(F f, int reps = 30) {
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  for (int i = 0; i < 10; ++i) f();
  hipEventRecord(e0);
  for (int i = 0; i < reps; ++i) f();
  hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  return ms / reps;
}
// bench.py's way: an event recorded in front of every launch (the step time includes the gap between launches)
template <typename F> double timeit_ev(F f, int reps = 30) {
  hipEvent_t ev[31];
  for (int i = 0; i <= reps; ++i) hipEventCreate(&ev[i]);
  for (int i = 0; i < 10; ++i) f();
  for (int i = 0; i < reps; ++i) { hipEventRecord(ev[i]); f(); }
  hipEventRecord(ev[reps]); hipEventSynchronize(ev[reps]);
  float ms; hipEventElapsedTime(&ms, ev[0], ev[reps]);
  for (int i = 0; i <= reps; ++i) hipEventDestroy(ev[i]);
  return ms / reps;
}
int main() {
  const size_t bytes = 1ull << 30; const uint32_t n16 = (uint32_t)(bytes / 16);
  u4 *a, *b, *sink; hipMalloc(&a, bytes); hipMalloc(&b, bytes); hipMalloc(&sink, 4096);
  hipMemset(a, 1, bytes); hipMemset(b, 2, bytes);
#define RUN(label, bytes_moved, ...) { double ms = timeit([&] { __VA_ARGS__; }); printf("%-34s %.4f ms  %7.1f GB/s\n", label, ms, (bytes_moved) / ms / 1e6); }
  RUN("read  nt, 1 load / lane", (double)bytes, hipLaunchKernelGGL((k_read<true, 1>), dim3(n16 / 256), dim3(256), 0, 0, a, sink, n16))
  RUN("read  nt, 4 loads / lane", (double)bytes, hipLaunchKernelGGL((k_read<true, 4>), dim3(n16 / 1024), dim3(256), 0, 0, a, sink, n16))
  RUN("read  plain, 4 loads / lane", (double)bytes, hipLaunchKernelGGL((k_read<false, 4>), dim3(n16 / 1024), dim3(256), 0, 0, a, sink, n16))
  RUN("write nt, 1 store / lane", (double)bytes, hipLaunchKernelGGL((k_write<true, 1>), dim3(n16 / 256), dim3(256), 0, 0, b, n16, 3u))
  RUN("write nt, 4 stores / lane", (double)bytes, hipLaunchKernelGGL((k_write<true, 4>), dim3(n16 / 1024), dim3(256), 0, 0, b, n16, 3u))
  RUN("write plain, 4 stores / lane", (double)bytes, hipLaunchKernelGGL((k_write<false, 4>), dim3(n16 / 1024), dim3(256), 0, 0, b, n16, 3u))
  RUN("copy  nt, 1 / lane (read + write)", 2.0 * bytes, hipLaunchKernelGGL((k_copy<true, 1>), dim3(n16 / 256), dim3(256), 0, 0, a, b, n16))
  RUN("copy  nt, 4 / lane (read + write)", 2.0 * bytes, hipLaunchKernelGGL((k_copy<true, 4>), dim3(n16 / 1024), dim3(256), 0, 0, a, b, n16))
  RUN("copy  plain, 4 / lane", 2.0 * bytes, hipLaunchKernelGGL((k_copy<false, 4>), dim3(n16 / 1024), dim3(256), 0, 0, a, b, n16))
  { const uint32_t row16 = 1024, nb = n16 / 4;  // 4096-pixel rows of RGBA8 = 1024 x 16 B
    RUN("mix 8 : 1 (DXT1 <- RGBA8, 4096 px rows)", 1.125 * bytes, hipLaunchKernelGGL(k_mix, dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb, row16, row16))
    RUN("mix 8 : 1, one load per lane (quads)", 1.125 * bytes, hipLaunchKernelGGL(k_mix_quad<0>, dim3(nb / 64), dim3(256), 0, 0, a, (u2 *)b, nb, row16))
    RUN("mix 8 : 1, one load per lane (16 x 4)", 1.125 * bytes, hipLaunchKernelGGL(k_mix_quad<1>, dim3(nb / 64), dim3(256), 0, 0, a, (u2 *)b, nb, row16))
    const uint32_t pad = 1024 + 16, nbp = (uint32_t)((bytes / 16 / pad / 4) * 1024);  // rows padded by 256 bytes
    RUN("mix 8 : 1, rows padded by 256 B", 72.0 * nbp, hipLaunchKernelGGL(k_mix, dim3(nbp / 256), dim3(256), 0, 0, a, (u2 *)b, nbp, row16, pad))
    const uint32_t pad2 = 1024 + 2, nbq = (uint32_t)((bytes / 16 / pad2 / 4) * 1024);  // rows padded by 32 bytes
    RUN("mix 8 : 1, rows padded by 32 B", 72.0 * nbq, hipLaunchKernelGGL(k_mix, dim3(nbq / 256), dim3(256), 0, 0, a, (u2 *)b, nbq, row16, pad2))
    RUN("mix 8 : 1, 8192 px rows", 1.125 * bytes, hipLaunchKernelGGL(k_mix, dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb, 2048u, 2048u))
    RUN("mix 8 : 1, 1024 px rows", 1.125 * bytes, hipLaunchKernelGGL(k_mix, dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb, 256u, 256u)) }
  // r07: the parts of the mix shape, and the shapes and store policies the issue asked about (all on 4096-pixel rows)
  { const uint32_t nb = n16 / 4;
#define RUN2(label, bytes_moved, ...) { double ms = timeit([&] { __VA_ARGS__; }), me = timeit_ev([&] { __VA_ARGS__; }); \
      printf("%-40s %.4f ms  %7.1f GB/s   event per launch %.4f ms\n", label, ms, (bytes_moved) / ms / 1e6, me); }
    for (int rep = 0; rep < 2; ++rep) {
      RUN2("r07 mix 8 : 1 (k_mix2, 8 B stores)", 1.125 * bytes, hipLaunchKernelGGL((k_mix2<1, 0, false>), dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 mix shape, no stores", 1.0 * bytes, hipLaunchKernelGGL((k_mix2<0, 0, false>), dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 linear read + 8 B stores", 1.125 * bytes, hipLaunchKernelGGL(k_lin_st8, dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 mix shape, 16 B stores / 2 lanes", 1.125 * bytes, hipLaunchKernelGGL((k_mix2<2, 0, false>), dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 mix shape, XCD-consecutive tiles", 1.125 * bytes, hipLaunchKernelGGL((k_mix2<1, 0, true>), dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 mix shape, write-through stores", 1.125 * bytes, hipLaunchKernelGGL((k_mix2<1, 1, false>), dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r08 write-through, 128-lane workgroups", 1.125 * bytes, hipLaunchKernelGGL((k_mix2<1, 1, false, 128>), dim3(nb / 128), dim3(128), 0, 0, a, (u2 *)b, nb))
      RUN2("r08 write-through, 64-lane workgroups", 1.125 * bytes, hipLaunchKernelGGL((k_mix2<1, 1, false, 64>), dim3(nb / 64), dim3(64), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 mix shape, sc1 stores (agent)", 1.125 * bytes, hipLaunchKernelGGL((k_mix2<1, 2, false>), dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 mix shape, sc0 sc1 nt buffer stores", 1.125 * bytes, hipLaunchKernelGGL((k_mix2<1, 3, false>), dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 mix shape, sc0 buffer stores", 1.125 * bytes, hipLaunchKernelGGL((k_mix2<1, 4, false>), dim3(nb / 256), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 block-row span, 16 loads first", 1.125 * bytes, hipLaunchKernelGGL((k_span<false, false>), dim3(nb / 1024), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 block-row span, block by block", 1.125 * bytes, hipLaunchKernelGGL((k_span<false, true>), dim3(nb / 1024), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 block-row span + XCD-consecutive", 1.125 * bytes, hipLaunchKernelGGL((k_span<true, false>), dim3(nb / 1024), dim3(256), 0, 0, a, (u2 *)b, nb))
      RUN2("r07 span + XCD-consecutive, by block", 1.125 * bytes, hipLaunchKernelGGL((k_span<true, true>), dim3(nb / 1024), dim3(256), 0, 0, a, (u2 *)b, nb))
    } }
  return 0;
}
