// metric_walk.inc -- the block walk of every raster metric kernel (metric_kernels.hip, eac11_16_kernels.hip, bc6h_kernels.hip),
// once: which blocks a lane takes, when a workgroup, a wave or a lane commits to an image's record, and the launch whose grid
// that walk assumes.  Kernel code; include it inside namespace icamd after ic_launch.h and ic_amd.h.
//
// A family brings its accumulator as an Ops: the type Acc, clear(acc), wave_reduce(acc) (every lane ends with the wave's
// figures) and commit(P, img, acc) (adds one contribution to image img's record).

// Blocks per lane: a workgroup covers 256 * kMetricBlocksPerLane consecutive blocks (lane t takes blocks t, t + 256, ...: a
// wave still reads 64 consecutive blocks at a time), a quarter of the atomics of one block per lane.  The range budget of
// metric_block.h holds for 4 blocks of 32 pixels.
constexpr uint32_t kMetricBlocksPerLane = 4;

// The lanes of a wave may hold blocks of different images (small images in a batch): one commit per wave where they agree,
// one per lane where they do not.  Every lane of the wave calls this (lanes without a block bring zeros).
template <typename Ops>
__device__ __forceinline__ void metric_flush_wave(const MetricParams &P, uint32_t img, typename Ops::Acc &a) {
  const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)img);
  if (wave_all(img == first)) {
    Ops::wave_reduce(a);
    if ((threadIdx.x & 63u) == 0u) Ops::commit(P, first, a);
  } else {
    Ops::commit(P, img, a);
  }
}

// Blocks in raster order of the images' own block grids, kMetricBlocksPerLane per lane.  one(img, brow, bcol, acc) adds
// block (brow, bcol) of image img to acc; whole(img, acc) commits for a workgroup whose blocks all lie in image img
// (workgroup-uniform: it may contain a barrier).
template <typename Ops, typename One, typename Whole>
__device__ __forceinline__ void metric_walk(const MetricParams &P, One one, Whole whole) {
  const uint32_t chunk0 = blockIdx.x * (kThreadsPerWorkgroup * kMetricBlocksPerLane);
  const uint32_t last = umin(chunk0 + kThreadsPerWorkgroup * kMetricBlocksPerLane, P.total_blocks) - 1u;
  const uint32_t img_first = fastdiv(chunk0, P.div_bpi), img_last = fastdiv(last, P.div_bpi);
  const bool one_image = img_first == img_last;  // workgroup-uniform
  typename Ops::Acc acc;
  Ops::clear(acc);
#pragma nounroll
  for (uint32_t j = 0; j < kMetricBlocksPerLane; ++j) {
    const uint32_t k = chunk0 + j * kThreadsPerWorkgroup + threadIdx.x;
    uint32_t img = img_last;
    if (k < P.total_blocks) {
      img = one_image ? img_first : fastdiv(k, P.div_bpi);
      const uint32_t rem = k - img * P.blocks_per_image;
      const uint32_t brow = fastdiv(rem, P.div_cols), bcol = rem - brow * P.block_cols;
      one(img, brow, bcol, acc);
    }
    if (!one_image) {
      metric_flush_wave<Ops>(P, img, acc);
      Ops::clear(acc);
    }
  }
  if (one_image) whole(img_first, acc);
}
// Every wave commits for itself.
template <typename Ops, typename One>
__device__ __forceinline__ void metric_walk(const MetricParams &P, One one) {
  metric_walk<Ops>(P, one, [&](uint32_t img, typename Ops::Acc &acc) { metric_flush_wave<Ops>(P, img, acc); });
}

// Accumulators with N channels of a 64-bit sum sse[k] and a 32-bit maximum mx[k] (Eac16Acc, Bc6hAcc); vector atomics, zero
// contributions are skipped.
template <typename A, int N>
struct MetricWideOps {
  using Acc = A;
  static __device__ __forceinline__ void clear(A &a) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      a.sse[k] = 0u;
      a.mx[k] = 0u;
    }
  }
  static __device__ __forceinline__ void wave_reduce(A &a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        a.sse[k] += (uint64_t)__shfl_xor((unsigned long long)a.sse[k], off);
        a.mx[k] = umax(a.mx[k], (uint32_t)__shfl_xor((int)a.mx[k], off));
      }
    }
  }
  static __device__ __forceinline__ void commit(const MetricParams &P, uint32_t img, const A &a) {
    icamd_error_stats *rec = reinterpret_cast<icamd_error_stats *>(P.stats) + img;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (a.sse[k]) atomicAdd(reinterpret_cast<unsigned long long *>(&rec->sse[k]), (unsigned long long)a.sse[k]);
      if (a.mx[k]) atomicMax(&rec->max_abs[k], a.mx[k]);
    }
  }
};

// The launch metric_walk assumes: 256 * kMetricBlocksPerLane blocks a workgroup.
template <typename Kernel>
hipError_t launch_metric_walk(Kernel kernel, const MetricParams &P, hipStream_t stream) {
  if (P.total_blocks == 0) return hipSuccess;
  (void)hipGetLastError();  // a stale error of another library on this thread is not this launch's
  const uint32_t per = kThreadsPerWorkgroup * kMetricBlocksPerLane;
  hipLaunchKernelGGL(kernel, dim3((P.total_blocks + per - 1u) / per), dim3(kThreadsPerWorkgroup), 0, stream, P);
  return hipGetLastError();
}
