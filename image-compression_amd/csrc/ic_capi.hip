// ic_capi.hip -- implementation of the C ABI declared in include/ic_amd.h.
//
// Argument validation mirrors the reference's public wrappers (the bool they return
// becomes ICAMD_OK / ICAMD_FALSE); everything else is geometry set-up and kernel
// launches.  There is no CPU encode path in this library.
#include "ic_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "codec_info.h"
#include "containers.h"
#include "decode_plan.h"
#include "ic_abi.h"
#include "ic_launch.h"

// Error text and the exception barrier of the C ABI: declared in ic_abi.h (shared with rccl_gather.hip), defined here.
namespace icamd {
thread_local char g_last_error[kErrorChars] = "";

void set_last_error(const char *text) noexcept {
  std::snprintf(g_last_error, kErrorChars, "%s", text ? text : "");
}

int fail(int code, const char *what, hipError_t e) noexcept {
  if (e != hipSuccess)
    std::snprintf(g_last_error, kErrorChars, "%s: %s (%s)", what, hipGetErrorName(e), hipGetErrorString(e));
  else
    std::snprintf(g_last_error, kErrorChars, "%s", what);
  return code;
}

int abi_exception() noexcept {
  try {
    throw;
  } catch (const std::bad_alloc &) {
    return fail(ICAMD_ERR_ALLOC, "out of host memory (std::bad_alloc)");
  } catch (const std::system_error &e) {
    char buf[kErrorChars];
    std::snprintf(buf, sizeof buf, "system resource unavailable (std::system_error: %s)", e.what());
    return fail(ICAMD_ERR_ALLOC, buf);
  } catch (const std::exception &e) {
    char buf[kErrorChars];
    std::snprintf(buf, sizeof buf, "unexpected C++ exception: %s", e.what());
    return fail(ICAMD_ERR_HIP, buf);
  } catch (...) {
    return fail(ICAMD_ERR_HIP, "unexpected C++ exception");
  }
}
}  // namespace icamd

namespace {
using icamd::abi_exception;
using icamd::fail;
using icamd::g_last_error;
using icamd::kErrorChars;
using icamd::set_last_error;

// Worker threads of the two batch entry points.  A worker's body never lets an exception out (that would be std::terminate);
// the guard joins whatever was started before the vectors the workers write to go out of scope, on every path out.
struct JoinAll {
  std::vector<std::thread> &threads;
  ~JoinAll() {
    for (std::thread &t : threads)
      if (t.joinable()) t.join();
  }
};
// A device list is a handful of GPUs, possibly each named a few times (two workers per GPU overlap their copies): a longer
// list is a caller's mistake, and one worker thread per entry must not be something a caller can ask 10 000 of.
constexpr int kMaxDeviceListEntries = 256;
// Text of a worker's first failure (fixed size: written from inside the worker without allocating).
struct WorkerError {
  char text[kErrorChars] = "";
  bool empty() const { return text[0] == 0; }
  void set(const char *t) noexcept { std::snprintf(text, sizeof text, "%s", t ? t : ""); }
};

#define ICAMD_HIP(call, what)                                   \
  do {                                                          \
    hipError_t e_ = (call);                                     \
    if (e_ != hipSuccess) return fail(ICAMD_ERR_HIP, what, e_); \
  } while (0)

uint32_t num_blocks4(uint32_t n) { return (n + 3) / 4; }  // helper.h:86-88
bool is_pow2(uint32_t x) { return x != 0 && !(x & (x - 1)); }
int format_components(int format) {  // compressed_image.h:188-199
  return (format == ICAMD_RGB || format == ICAMD_BGR) ? 3 : (format == ICAMD_RGBA || format == ICAMD_BGRA) ? 4 : 0;
}
bool format_swaps(int format) { return format == ICAMD_BGR || format == ICAMD_BGRA; }  // compressed_image.h:202-204

uint32_t ilog2(uint32_t x) {
  uint32_t l = 0;
  while ((1u << l) < x) ++l;
  return l;
}

// Per-thread device staging for the host-buffer entry points (grow-only).
struct Staging {
  int device = -1;
  hipStream_t stream = nullptr, stream2 = nullptr;  // two streams: bands of one image alternate between them
  void *d_in = nullptr, *d_out = nullptr;
  size_t cap_in = 0, cap_out = 0;
  // No destructor: a Staging is never destroyed (see TlsStaging below) -- no HIP call may run from a thread_local or
  // static destructor, where the HIP runtime can already be gone.
  void drop() {
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (stream) (void)hipStreamDestroy(stream);
    if (stream2) (void)hipStreamDestroy(stream2);
    d_in = d_out = nullptr;
    cap_in = cap_out = 0;
    stream = stream2 = nullptr;
  }
  int ensure(size_t in_bytes, size_t out_bytes) {
    int dev = 0;
    ICAMD_HIP(hipGetDevice(&dev), "hipGetDevice");
    if (dev != device) {  // thread moved to another device: drop the old buffers
      drop();
      device = dev;
    }
    if (!stream) ICAMD_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
    if (!stream2) ICAMD_HIP(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking), "hipStreamCreate");
    if (in_bytes > cap_in) {
      if (d_in) (void)hipFree(d_in);
      d_in = nullptr; cap_in = 0;
      if (hipMalloc(&d_in, in_bytes) != hipSuccess) return fail(ICAMD_ERR_ALLOC, "hipMalloc(input staging)");
      cap_in = in_bytes;
    }
    if (out_bytes > cap_out) {
      if (d_out) (void)hipFree(d_out);
      d_out = nullptr; cap_out = 0;
      if (hipMalloc(&d_out, out_bytes) != hipSuccess) return fail(ICAMD_ERR_ALLOC, "hipMalloc(output staging)");
      cap_out = out_bytes;
    }
    return ICAMD_OK;
  }
};

// Every Staging lives in (or is on loan from) this process-wide pool: icamd_compress_batch's short-lived worker
// threads take one and give it back, so repeated batches allocate nothing, and a thread's own staging (tls_staging())
// returns to the pool when the thread ends instead of being destroyed.  The pool itself is heap-allocated and never
// destroyed: at process exit the HIP runtime may already be gone, so nothing here calls into it from a destructor --
// the driver reclaims device memory and streams with the process.
std::mutex &g_pool_mutex = *new std::mutex();
std::vector<std::unique_ptr<Staging>> &g_pool = *new std::vector<std::unique_ptr<Staging>>();

std::unique_ptr<Staging> pool_take(int device) {
  std::lock_guard<std::mutex> lock(g_pool_mutex);
  for (size_t i = 0; i < g_pool.size(); ++i)
    if (g_pool[i]->device == device) {
      std::unique_ptr<Staging> s = std::move(g_pool[i]);
      g_pool.erase(g_pool.begin() + (long)i);
      return s;
    }
  return std::unique_ptr<Staging>(new Staging());
}
void pool_give(std::unique_ptr<Staging> s) {
  std::lock_guard<std::mutex> lock(g_pool_mutex);
  g_pool.push_back(std::move(s));
}

// The calling thread's staging for the host-buffer entry points: borrowed from the pool on first use (any device --
// Staging::ensure re-targets it), handed back -- not freed -- by the thread_local destructor.
struct TlsStaging {
  Staging *p = nullptr;
  Staging &get() {
    if (!p) {
      int dev = 0;
      (void)hipGetDevice(&dev);
      p = pool_take(dev).release();
    }
    return *p;
  }
  ~TlsStaging() {
    if (!p) return;
    try {
      pool_give(std::unique_ptr<Staging>(p));  // no HIP call here
    } catch (...) {
      // (the pool could not grow: the staging's device buffers stay allocated until the process ends)
    }
  }
};
thread_local TlsStaging g_tls_staging;
Staging &tls_staging() { return g_tls_staging.get(); }

int require_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(ICAMD_ERR_NO_DEVICE, "no HIP device available; this library has no CPU path", e);
  return ICAMD_OK;
}

// What (compressor, format) encodes to; returns false when the reference's Compress would.
bool resolve_codec(int compressor, int format, int *codec, int *comps = nullptr, bool *swap = nullptr) {
  const int c = format_components(format);
  if (c == 0) return false;
  if (comps) *comps = c;
  if (swap) *swap = format_swaps(format);
  if (compressor == ICAMD_COMPRESSOR_DXTC) {  // dxtc.cc:741-749: 3 components -> DXT1, else DXT5
    *codec = c == 3 ? ICAMD_DXT1 : ICAMD_DXT5;
    return true;
  }
  if (compressor == ICAMD_COMPRESSOR_ETC) {  // etc.cc:751-754: kRGB only
    if (format != ICAMD_RGB) return false;
    *codec = ICAMD_ETC1;
    return true;
  }
  return false;
}

// Which source component counts a codec encodes from (icamd_encode_device): DXT1 / ETC1 / ETC2 RGB8 3 or 4, DXT5 / ETC2 RGBA8 /
// ETC2 RGB8A1 / BC1A / BC2 4,
// BC4 and EAC R11 1..4, BC5 and EAC RG11 2..4, BC7 3 or 4.
bool codec_accepts_components(int codec, int comps) {
  switch (codec) {
    case ICAMD_DXT1: case ICAMD_ETC1: case ICAMD_ETC2_RGB8: case ICAMD_BC7: return comps == 3 || comps == 4;
    case ICAMD_DXT5: case ICAMD_ETC2_RGBA8: case ICAMD_ETC2_RGB8A1: case ICAMD_BC1A: case ICAMD_BC2: return comps == 4;
    case ICAMD_BC4: case ICAMD_EAC_R11: return comps >= 1 && comps <= 4;
    case ICAMD_BC5: case ICAMD_EAC_RG11: return comps >= 2 && comps <= 4;
  }
  return false;
}
// The one- and two-channel codecs (R, or R and G, of 1..4-byte pixels; R8 / RG8 rows out): BC4 / BC5 and EAC R11 / RG11.
bool plane_codec(int codec) { return codec == ICAMD_BC4 || codec == ICAMD_BC5 || codec == ICAMD_EAC_R11 || codec == ICAMD_EAC_RG11; }
bool eac11_codec(int codec) { return codec == ICAMD_EAC_R11 || codec == ICAMD_EAC_RG11; }
// BC1 with punch-through alpha and BC2 (EXTENSIONS, include/ic_amd.h ICAMD_BC1A): RGBA8 in, RGBA8 rows out
bool bc1a_bc2_codec(int codec) { return codec == ICAMD_BC1A || codec == ICAMD_BC2; }

// The sizes PvrtcCompressor::Compress accepts (pvrtc.cc:636-650): a square power of two of at least 8 x 8 (for a square
// power of two, width % 8 == 0 && height % 4 == 0 is width >= 8).  The reference sizes its output with the uint32 product
// width * height / 4 (pvrtc.cc:631-634), which wraps to 0 at 65536^2 -- it would then write 2^30 bytes into a zero-byte
// buffer; refused here (the kernels also index pixels with 32 bits).
bool pvrtc_size_ok(uint32_t height, uint32_t width) { return is_pow2(width) && width == height && width >= 8u && width < 65536u; }

// Compressor::Compress of PVRTC, device or host buffers (pvrtc.cc:636-667): no row padding, the reference's output size.
// `format` is deliberately not validated (neither does the reference): the buffer is read as RGBA8888, pvrtc.cc:664.
bool pvrtc_compress_ok(uint32_t height, uint32_t width, uint32_t padding_bytes_per_row, size_t out_size) {
  return pvrtc_size_ok(height, width) && padding_bytes_per_row == 0 && out_size == (size_t)(width * height / 4);
}

// host-buffer wrappers: stage in, run, stage out.  The device output holds dev_out_bytes (>= out_size, of which the first
// out_size come back); in_place: the result is read back from the input buffer.
template <typename F>
int staged_blockop(Staging &st, const void *in, size_t in_size, void *out, size_t out_size, size_t dev_out_bytes,
                   bool in_place, F &&run) {
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  rc = st.ensure(std::max<size_t>(in_size, 1), std::max<size_t>(dev_out_bytes, 1));
  if (rc != ICAMD_OK) return rc;
  hipStream_t s = st.stream;
  ICAMD_HIP(hipMemcpyAsync(st.d_in, in, in_size, hipMemcpyHostToDevice, s), "H2D copy");
  rc = run(st.d_in, st.d_out, s);
  if (rc != ICAMD_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  ICAMD_HIP(hipMemcpyAsync(out, in_place ? st.d_in : st.d_out, out_size, hipMemcpyDeviceToHost, s), "D2H copy");
  ICAMD_HIP(hipStreamSynchronize(s), "stream synchronize");
  return ICAMD_OK;
}

icamd::PvrtcParams pvrtc_params(const void *d_src, void *d_dst, uint32_t size, uint32_t n_images, size_t src_image_stride_bytes,
                                size_t dst_image_stride_bytes) {
  icamd::PvrtcParams P;
  P.src = static_cast<const uint8_t *>(d_src);
  P.dst = static_cast<uint8_t *>(d_dst);
  P.src_image_stride = src_image_stride_bytes;
  P.dst_image_stride = dst_image_stride_bytes;
  P.size = size;
  P.log2_size = ilog2(size);
  P.n_images = n_images;
  return P;
}

// PVRTC branch of icamd_encode_device.  internal_workspace: the call comes from the library's own host-buffer path
// (its staging stream), which must not borrow the workspace a caller registered for its own streams / graphs.
// PVRTC4 is an EXTENSION (parity unpinned, include/ic_amd.h): PVRTC1 4 bpp under the same preconditions.
int pvrtc_encode_device_impl(int codec, int src_components, uint32_t height, uint32_t width, uint32_t row_stride_bytes,
                             uint32_t n_images, size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                             const void *d_src, void *d_dst, hipStream_t stream, bool internal_workspace) {
  // preconditions of PvrtcCompressor::Compress (source always read as RGBA8888, no row padding)
  if (!pvrtc_size_ok(height, width)) return ICAMD_FALSE;
  if (src_components != 4 || row_stride_bytes != width * 4u) return ICAMD_FALSE;
  if (reinterpret_cast<uintptr_t>(d_src) % 16u || reinterpret_cast<uintptr_t>(d_dst) % 8u ||
      (n_images > 1 && (src_image_stride_bytes % 16u || dst_image_stride_bytes % 8u)))
    return fail(ICAMD_ERR_ARG, "PVRTC: source must be 16-byte aligned, output 8-byte aligned");
  icamd::PvrtcParams P = pvrtc_params(d_src, d_dst, width, n_images, src_image_stride_bytes, dst_image_stride_bytes);
  P.internal_workspace = internal_workspace;
  if (codec == ICAMD_PVRTC4)
    ICAMD_HIP(icamd::launch_pvrtc4(P, stream), "launch pvrtc4");
  else
    ICAMD_HIP(icamd::launch_pvrtc2(P, stream), "launch pvrtc2");
  return ICAMD_OK;
}

icamd::GridParams grid_params(const void *d_src, void *d_dst, uint32_t height, uint32_t width, uint32_t grid_height,
                              uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images, size_t src_image_stride_bytes,
                              size_t dst_image_stride_bytes, int swap_rb, uint32_t etc_strategy) {
  icamd::GridParams P;
  P.src = static_cast<const uint8_t *>(d_src);
  P.dst = static_cast<uint8_t *>(d_dst);
  P.src_image_stride = src_image_stride_bytes;
  P.dst_image_stride = dst_image_stride_bytes;
  P.height = height;
  P.width = width;
  P.block_rows = num_blocks4(std::max(height, grid_height));  // helper.h:487-488,501-502
  P.block_cols = num_blocks4(std::max(width, grid_width));
  P.row_stride = row_stride_bytes;
  P.n_images = n_images;
  P.swap_rb = swap_rb ? 1u : 0u;
  P.etc_strategy = etc_strategy;
  P.log2_tile_cols = P.tile_row0 = P.force_gather = 0;
  return P;
}

// EXTENSION (include/ic_amd.h ICAMD_BC4, ICAMD_EAC_R11): BC4 / EAC R11 from 1..4-byte sources, BC5 / EAC RG11 from 2..4-byte ones;
// R = byte 0 (byte 2 when swap_rb and the source has 3 or 4 bytes), G = byte 1.  The argument checks come before any device work.
int plane_encode_device_impl(int codec, int src_components, int swap_rb, uint32_t height, uint32_t width, uint32_t grid_height,
                            uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images, size_t src_image_stride_bytes,
                            size_t dst_image_stride_bytes, const void *d_src, void *d_dst, hipStream_t stream) {
  if (!codec_accepts_components(codec, src_components))
    return fail(ICAMD_ERR_ARG, codec == ICAMD_BC5 ? "BC5 needs 2, 3 or 4 source components"
                               : codec == ICAMD_BC4 ? "BC4 needs 1 to 4 source components"
                               : codec == ICAMD_EAC_RG11 ? "EAC RG11 needs 2, 3 or 4 source components"
                                                         : "EAC R11 needs 1 to 4 source components");
  if (swap_rb && src_components < 3) return fail(ICAMD_ERR_ARG, "swap_rb needs a 3- or 4-component source");
  if ((uint64_t)row_stride_bytes < (uint64_t)width * (uint32_t)src_components)
    return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  if (n_images == 0) return ICAMD_OK;
  const int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  const icamd::GridParams P = grid_params(d_src, d_dst, height, width, grid_height, grid_width, row_stride_bytes, n_images,
                                          src_image_stride_bytes, dst_image_stride_bytes, swap_rb, 0);
  if (eac11_codec(codec))
    ICAMD_HIP(icamd::launch_eac11_encode(codec, src_components, P, stream), "launch eac r11 / rg11");
  else
    ICAMD_HIP(icamd::launch_bc45_encode(codec, src_components, P, stream), codec == ICAMD_BC5 ? "launch bc5" : "launch bc4");
  return ICAMD_OK;
}

// The geometry checks of Pad and Downsample, for device and host buffers alike: false where the reference refuses.  Pad
// (helper.h:393-404): the padded grid holds the image's, and the output is the padded image's size.
bool pad_geometry_ok(int codec, uint32_t ch, uint32_t cw, uint32_t ph, uint32_t pw, size_t out_size) {
  return num_blocks4(ph) >= num_blocks4(ch) && num_blocks4(pw) >= num_blocks4(cw) && out_size == icamd_encoded_size(codec, ph, pw);
}
// Downsample (helper.h:281-284, :340-341): grids of more than one block have an even number of them per side, a single block
// is 1, 2 or 4 pixels per side (none of zero: the entry points' first check); the output is the halved image's size.
bool downsample_geometry_ok(int codec, uint32_t uh, uint32_t uw, size_t out_size) {
  const uint32_t r = num_blocks4(uh), c = num_blocks4(uw);
  if ((r > 1 && r % 2) || (c > 1 && c % 2) || (r == 1 && c == 1 && (uh == 3 || uw == 3))) return false;
  return out_size == icamd_encoded_size(codec, (uh + 1) / 2, (uw + 1) / 2);
}

// The compressed-domain batches (pad, downsample) once their arguments are checked: `in` holds the geometry; the launcher
// plans the launches (blockops_plan.h) and groups the images.
int blockop_batch(hipError_t (*launch)(icamd::BlockOpCall, hipStream_t), const char *what, const icamd::BlockOpIn &in,
                  const void *d_blocks, size_t src_image_stride_bytes, void *d_out, size_t dst_image_stride_bytes, void *hip_stream) {
  if (in.n_images == 0) return ICAMD_OK;  // (after the checks: a call the reference would refuse is refused for any count)
  const int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  if (!icamd::blockop_image_fits(in.out_rows, in.out_cols)) return fail(ICAMD_ERR_ARG, "more than 2^31 blocks in one image");
  ICAMD_HIP(launch({ in, static_cast<const uint8_t *>(d_blocks), static_cast<uint8_t *>(d_out), src_image_stride_bytes,
                     dst_image_stride_bytes }, static_cast<hipStream_t>(hip_stream)), what);
  return ICAMD_OK;
}

// The device list of a batch entry point: every ordinal must name a visible device (*visible: how many there are).
int check_device_list(const char *entry, const int *devices, int n_devices, int *visible) {
  ICAMD_HIP(hipGetDeviceCount(visible), "hipGetDeviceCount");
  for (int d = 0; d < n_devices; ++d)
    if (devices[d] < 0 || devices[d] >= *visible) {
      char text[kErrorChars];
      std::snprintf(text, sizeof text, "%s: bad device ordinal", entry);
      return fail(ICAMD_ERR_ARG, text);
    }
  return ICAMD_OK;
}

// One worker thread per device-list entry, but no more than there are images: work(d, local, error) does images d,
// d + n_devices, ... -- it writes each one's status to local[i] and a failure's text to `error`, and lets no exception out.
// statuses[] (optional) receives every image's status; the result is the first non-OK one in image order, and the
// error text that of the first worker that has one.
template <typename Work>
int run_workers(const char *entry, int n_devices, uint32_t n_images, int *statuses, Work &&work) {
  std::vector<int> local(n_images, ICAMD_OK);
  std::vector<WorkerError> errors((size_t)n_devices);
  std::vector<std::thread> workers;
  workers.reserve((size_t)n_devices);
  int not_started_from = n_devices;  // list entries from here on have no worker (thread creation failed)
  {
    JoinAll join_on_every_path_out{workers};
    for (int d = 0; d < n_devices && (uint32_t)d < n_images; ++d) {
      try {
        workers.emplace_back([&, d]() noexcept { work(d, local, errors[(size_t)d]); });
      } catch (...) {  // std::system_error from the thread's creation (or bad_alloc): the workers started so far finish
        (void)abi_exception();
        not_started_from = d;
        break;
      }
    }
  }  // all started workers joined
  for (int d = not_started_from; d < n_devices; ++d) {
    for (uint64_t i = (uint64_t)d; i < n_images; i += (uint64_t)n_devices) local[i] = ICAMD_ERR_ALLOC;
    std::snprintf(errors[(size_t)d].text, kErrorChars, "%s: could not start a worker thread", entry);
  }
  int first = ICAMD_OK;
  for (uint32_t i = 0; i < n_images; ++i) {
    if (statuses) statuses[i] = local[i];
    if (first == ICAMD_OK && local[i] != ICAMD_OK) first = local[i];
  }
  if (first < 0)
    for (const WorkerError &e : errors)
      if (!e.empty()) { set_last_error(e.text); break; }
  return first;
}


// ---- mip chains (EXTENSION, include/ic_amd.h): what a call launches is mip_plan.h's; here are the argument checks ----
using icamd::mip_codec;
using icamd::mip_max_levels;
int mip_check_components(int codec, int comps, int swap_rb) {
  if (!codec_accepts_components(codec, comps))
    return fail(ICAMD_ERR_ARG, "mip chain: source components not accepted by this codec (as icamd_encode_device)");
  if (swap_rb && comps < 3) return fail(ICAMD_ERR_ARG, "swap_rb needs a 3- or 4-component source");
  return ICAMD_OK;
}
// The filter rules of the filtered mip entry points (ICAMD_MIP_FILTER_*; codec may be icamd::kMipPyramidMode): the colour
// filters for colour only, the normal-map filter for BC5 and the two-byte pyramid only.
int mip_check_filter(int codec, int comps, int filter) {
  if (filter == ICAMD_MIP_FILTER_NORMAL) {
    if (codec == icamd::kMipPyramidMode)
      return comps == 2 ? ICAMD_OK : fail(ICAMD_ERR_ARG, "ICAMD_MIP_FILTER_NORMAL: the pixel pyramid needs a 2-component (RG) source");
    return codec == ICAMD_BC5 ? ICAMD_OK : fail(ICAMD_ERR_ARG, "ICAMD_MIP_FILTER_NORMAL applies to ICAMD_BC5 chains only");
  }
  if (filter < 0 || filter > (ICAMD_MIP_FILTER_SRGB | ICAMD_MIP_FILTER_ALPHA_WEIGHTED))
    return fail(ICAMD_ERR_ARG, "mip filter must be a combination of ICAMD_MIP_FILTER_SRGB and ICAMD_MIP_FILTER_ALPHA_WEIGHTED, "
                               "or ICAMD_MIP_FILTER_NORMAL alone");
  if (filter == ICAMD_MIP_FILTER_BOX) return ICAMD_OK;
  if (codec == ICAMD_BC4 || codec == ICAMD_BC5)
    return fail(ICAMD_ERR_ARG, "BC4 / BC5 hold data channels: only ICAMD_MIP_FILTER_BOX applies");
  if (comps != 3 && comps != 4) return fail(ICAMD_ERR_ARG, "mip filters other than the box need a 3- or 4-component source");
  if ((filter & ICAMD_MIP_FILTER_ALPHA_WEIGHTED) && comps != 4)
    return fail(ICAMD_ERR_ARG, "ICAMD_MIP_FILTER_ALPHA_WEIGHTED needs a 4-component source");
  return ICAMD_OK;
}
// The geometry checks of the mip entry points: the level count, the row stride, and (n_images > 1) the image strides
// against one image's source and output -- its encoded chain, or its pixel pyramid when codec is icamd::kMipPyramidMode.
int mip_check_geometry(int codec, int comps, uint32_t height, uint32_t width, uint32_t row_stride_bytes, uint32_t levels,
                       uint32_t n_images, size_t src_image_stride_bytes, size_t dst_image_stride_bytes) {
  if (levels == 0 || levels > mip_max_levels(height, width))
    return fail(ICAMD_ERR_ARG, "levels must be 1 .. floor(log2(max(height, width))) + 1");
  if ((uint64_t)row_stride_bytes < (uint64_t)width * (uint32_t)comps) return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  const size_t src_bytes = (size_t)(height - 1u) * row_stride_bytes + (size_t)width * (uint32_t)comps;
  const size_t dst_bytes = codec == icamd::kMipPyramidMode ? icamd::mip_pyramid_bytes(height, width, levels, comps)
                                                           : icamd::mip_chain_bytes(codec, height, width, levels, nullptr);
  if (n_images > 1 && (src_image_stride_bytes < src_bytes || dst_image_stride_bytes < dst_bytes))
    return fail(ICAMD_ERR_ARG, "image stride smaller than an image");
  return ICAMD_OK;
}
}  // namespace

extern "C" {
#pragma GCC visibility push(default)

const char *icamd_version(void) { return "image-compression_amd 0.6 (gfx950)"; }
const char *icamd_last_error(void) { return g_last_error; }

int icamd_device_count(void) try {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
} ICAMD_ABI_CATCH

const char *icamd_kernel_name(int codec, int src_components) {
  switch (codec) {
    case ICAMD_DXT1: case ICAMD_DXT5: return icamd::dxt_kernel_name(codec, src_components);
    case ICAMD_ETC1: return icamd::etc1_kernel_name(src_components);
    case ICAMD_ETC2_RGBA8: return icamd::etc2_kernel_name(src_components);
    case ICAMD_ETC2_RGB8: return icamd::etc2_rgb8_kernel_name(src_components);
    case ICAMD_ETC2_RGB8A1: return icamd::etc2_a1_kernel_name(src_components);
    case ICAMD_PVRTC2: return icamd::pvrtc2_kernel_name();
    case ICAMD_PVRTC4: return icamd::pvrtc4_kernel_name();
    case ICAMD_BC4: case ICAMD_BC5: return icamd::bc45_kernel_name(codec, src_components);
    case ICAMD_EAC_R11: case ICAMD_EAC_RG11: return icamd::eac11_kernel_name(codec, src_components);
    case ICAMD_BC7: return icamd::bc7_kernel_name(src_components);
    case ICAMD_BC1A: case ICAMD_BC2: return icamd::bc1a_bc2_kernel_name(codec, src_components);
  }
  return "";
}

int icamd_supports_format(int compressor, int format) try {
  if (format_components(format) == 0) return 0;
  if (compressor == ICAMD_COMPRESSOR_DXTC) return 1;                      // dxtc.cc:707-710
  if (compressor == ICAMD_COMPRESSOR_ETC) return format == ICAMD_RGB;     // etc.cc:713-717
  if (compressor == ICAMD_COMPRESSOR_PVRTC) return format == ICAMD_RGBA;  // pvrtc.cc:607-609
  return 0;
} ICAMD_ABI_CATCH

size_t icamd_compute_compressed_data_size(int compressor, int format, uint32_t height, uint32_t width) {
  if (compressor == ICAMD_COMPRESSOR_PVRTC) return (size_t)(width * height / 4);  // pvrtc.cc:631-634 (uint32 product)
  if (height == 0 || width == 0) return 0;
  const size_t blocks = (size_t)std::max(1u, num_blocks4(height)) * std::max(1u, num_blocks4(width));
  if (compressor == ICAMD_COMPRESSOR_DXTC) return blocks * (format_components(format) == 3 ? 8u : 16u);  // dxtc.cc:276-280,725-733
  if (compressor == ICAMD_COMPRESSOR_ETC) return format == ICAMD_RGB ? blocks * 8u : 0;                  // etc.cc:734-745
  return 0;
}

size_t icamd_encoded_size(int codec, uint32_t grid_height, uint32_t grid_width) {
  if (codec == ICAMD_PVRTC2) return (size_t)grid_width * grid_height / 4;
  if (codec == ICAMD_PVRTC4) return (size_t)grid_width * grid_height / 2;
  return (size_t)num_blocks4(grid_height) * num_blocks4(grid_width) * icamd::codec_block_bytes(codec);
}

int icamd_encode_device(int codec, int etc_strategy, int src_components, int swap_rb,
                        uint32_t height, uint32_t width, uint32_t grid_height, uint32_t grid_width,
                        uint32_t row_stride_bytes, uint32_t n_images,
                        size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                        const void *d_src, void *d_dst, void *hip_stream) try {
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (plane_codec(codec))
    return plane_encode_device_impl(codec, src_components, swap_rb, height, width, grid_height, grid_width, row_stride_bytes,
                                    n_images, src_image_stride_bytes, dst_image_stride_bytes, d_src, d_dst, stream);
  // EXTENSIONS (include/ic_amd.h ICAMD_BC1A, ICAMD_BC2): the transparency rule and the alpha word need the fourth byte
  if (codec == ICAMD_BC1A && src_components != 4) return fail(ICAMD_ERR_ARG, "BC1A needs a 4-component source");
  if (codec == ICAMD_BC2 && src_components != 4) return fail(ICAMD_ERR_ARG, "BC2 needs a 4-component source");
  if (src_components != 3 && src_components != 4) return fail(ICAMD_ERR_ARG, "src_components must be 3 or 4");
  // EXTENSION (include/ic_amd.h ICAMD_ETC2_RGBA8): the alpha half needs the fourth byte; checked before any device work
  if (codec == ICAMD_ETC2_RGBA8 && src_components != 4) return fail(ICAMD_ERR_ARG, "ETC2 RGBA8 needs a 4-component source");
  if (codec == ICAMD_ETC2_RGB8A1 && src_components != 4) return fail(ICAMD_ERR_ARG, "ETC2 RGB8A1 needs a 4-component source");
  if (n_images == 0) return ICAMD_OK;
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;

  if (codec == ICAMD_PVRTC2 || codec == ICAMD_PVRTC4)
    return pvrtc_encode_device_impl(codec, src_components, height, width, row_stride_bytes, n_images, src_image_stride_bytes,
                                    dst_image_stride_bytes, d_src, d_dst, stream, false);
  if (codec != ICAMD_DXT1 && codec != ICAMD_DXT5 && codec != ICAMD_ETC1 && codec != ICAMD_ETC2_RGBA8 && codec != ICAMD_ETC2_RGB8 &&
      codec != ICAMD_ETC2_RGB8A1 && codec != ICAMD_BC7 && !bc1a_bc2_codec(codec))
    return fail(ICAMD_ERR_ARG, "unknown codec");
  if (!codec_accepts_components(codec, src_components)) return fail(ICAMD_ERR_ARG, "DXT5 needs a 4-component source");
  if (row_stride_bytes < width * (uint32_t)src_components) return fail(ICAMD_ERR_ARG, "row stride smaller than a row");

  const icamd::GridParams P = grid_params(d_src, d_dst, height, width, grid_height, grid_width, row_stride_bytes, n_images,
                                          src_image_stride_bytes, dst_image_stride_bytes, swap_rb, (uint32_t)etc_strategy);
  if (codec == ICAMD_ETC1)
    ICAMD_HIP(icamd::launch_etc1(src_components, P, stream), "launch etc1");
  else if (codec == ICAMD_ETC2_RGBA8)
    ICAMD_HIP(icamd::launch_etc2(P, stream), "launch etc2");
  else if (codec == ICAMD_ETC2_RGB8)
    ICAMD_HIP(icamd::launch_etc2_rgb8(src_components, P, stream), "launch etc2 rgb8");
  else if (codec == ICAMD_ETC2_RGB8A1)
    ICAMD_HIP(icamd::launch_etc2_a1(P, stream), "launch etc2 rgb8a1");
  else if (codec == ICAMD_BC7)  // EXTENSION (include/ic_amd.h ICAMD_BC7): mode 6 from 3- or 4-component sources
    ICAMD_HIP(icamd::launch_bc7_encode(src_components, P, stream), "launch bc7");
  else if (bc1a_bc2_codec(codec))
    ICAMD_HIP(icamd::launch_bc1a_bc2_encode(codec, P, stream), codec == ICAMD_BC2 ? "launch bc2" : "launch bc1a");
  else
    ICAMD_HIP(icamd::launch_dxt(codec, src_components, P, stream), "launch dxt");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

// EXTENSION (include/ic_amd.h ICAMD_ETC2_MODES_TH): every argument is checked before any device work; modes 0 IS
// icamd_encode_device, modes 1 its launch followed on the same stream by the T / H pass over the same grid
int icamd_encode_etc2_device(int codec, int etc_strategy, int etc2_modes, int src_components, int swap_rb,
                             uint32_t height, uint32_t width, uint32_t grid_height, uint32_t grid_width,
                             uint32_t row_stride_bytes, uint32_t n_images,
                             size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                             const void *d_src, void *d_dst, void *hip_stream) try {
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  if (codec != ICAMD_ETC2_RGB8) return fail(ICAMD_ERR_ARG, "icamd_encode_etc2_device encodes ICAMD_ETC2_RGB8 only");
  if (etc2_modes != ICAMD_ETC2_MODES_DEFAULT && etc2_modes != ICAMD_ETC2_MODES_TH)
    return fail(ICAMD_ERR_ARG, "etc2_modes must be ICAMD_ETC2_MODES_DEFAULT or ICAMD_ETC2_MODES_TH");
  if (src_components != 3 && src_components != 4) return fail(ICAMD_ERR_ARG, "src_components must be 3 or 4");
  if (n_images == 0) return ICAMD_OK;  // (before the stride, as in icamd_encode_device)
  if (row_stride_bytes < width * (uint32_t)src_components) return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  const int rc = icamd_encode_device(codec, etc_strategy, src_components, swap_rb, height, width, grid_height, grid_width,
                                     row_stride_bytes, n_images, src_image_stride_bytes, dst_image_stride_bytes, d_src, d_dst,
                                     hip_stream);
  if (rc != ICAMD_OK || etc2_modes == ICAMD_ETC2_MODES_DEFAULT) return rc;
  const icamd::GridParams P = grid_params(d_src, d_dst, height, width, grid_height, grid_width, row_stride_bytes, n_images,
                                          src_image_stride_bytes, dst_image_stride_bytes, swap_rb, (uint32_t)etc_strategy);
  ICAMD_HIP(icamd::launch_etc2_th(src_components, P, static_cast<hipStream_t>(hip_stream)), "launch etc2 t/h");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

const char *icamd_etc2_kernel_name(int codec, int src_components, int etc2_modes) {
  if (codec == ICAMD_BC7 || bc1a_bc2_codec(codec)) return "";  // (as for an unknown codec: not ETC2-family codecs, include/ic_amd.h ICAMD_BC7)
  if (etc2_modes == ICAMD_ETC2_MODES_DEFAULT) return icamd_kernel_name(codec, src_components);
  if (etc2_modes == ICAMD_ETC2_MODES_TH && codec == ICAMD_ETC2_RGB8) return icamd::etc2_th_kernel_name(src_components);
  return "";
}

// EXTENSION (include/ic_amd.h ICAMD_BC7_MODES_EXTENDED): every argument is checked before any device work; modes 0 IS
// icamd_encode_device(ICAMD_BC7), modes 1 the fused kernel of bc7_modes_kernels.hip in its place
int icamd_encode_bc7_device(int bc7_modes, int src_components, int swap_rb, uint32_t height, uint32_t width,
                            uint32_t grid_height, uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                            size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                            const void *d_src, void *d_dst, void *hip_stream) try {
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  if (bc7_modes != ICAMD_BC7_MODES_DEFAULT && bc7_modes != ICAMD_BC7_MODES_EXTENDED)
    return fail(ICAMD_ERR_ARG, "bc7_modes must be ICAMD_BC7_MODES_DEFAULT or ICAMD_BC7_MODES_EXTENDED");
  if (src_components != 3 && src_components != 4) return fail(ICAMD_ERR_ARG, "src_components must be 3 or 4");
  if (n_images == 0) return ICAMD_OK;  // (before the stride, as in icamd_encode_device)
  if (row_stride_bytes < width * (uint32_t)src_components) return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  if (bc7_modes == ICAMD_BC7_MODES_DEFAULT)
    return icamd_encode_device(ICAMD_BC7, 0, src_components, swap_rb, height, width, grid_height, grid_width, row_stride_bytes,
                               n_images, src_image_stride_bytes, dst_image_stride_bytes, d_src, d_dst, hip_stream);
  const int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  const icamd::GridParams P = grid_params(d_src, d_dst, height, width, grid_height, grid_width, row_stride_bytes, n_images,
                                          src_image_stride_bytes, dst_image_stride_bytes, swap_rb, 0u);
  ICAMD_HIP(icamd::launch_bc7_modes_encode(src_components, P, static_cast<hipStream_t>(hip_stream)), "launch bc7 modes");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

const char *icamd_bc7_kernel_name(int src_components, int bc7_modes) {
  if (bc7_modes == ICAMD_BC7_MODES_DEFAULT) return icamd::bc7_kernel_name(src_components);
  if (bc7_modes == ICAMD_BC7_MODES_EXTENDED) return icamd::bc7_modes_kernel_name(src_components);
  return "";
}

// EXTENSION (include/ic_amd.h ICAMD_ETC2_COLOUR_PLANAR_TH): planar, T and H colour words for all three ETC2 colour codecs.
// true for the three codecs with a component count they take
static bool etc2_colour_accepts(int codec, int src_components) {
  if (codec == ICAMD_ETC2_RGB8) return src_components == 3 || src_components == 4;
  return (codec == ICAMD_ETC2_RGBA8 || codec == ICAMD_ETC2_RGB8A1) && src_components == 4;
}
// true where the pair has a pass of etc2_colour_modes_kernels.hip (the others forward to an existing entry point)
static bool etc2_colour_has_pass(int codec, int colour_modes) {
  return (codec == ICAMD_ETC2_RGBA8 && colour_modes != ICAMD_ETC2_COLOUR_DEFAULT) ||
         (codec == ICAMD_ETC2_RGB8A1 && colour_modes == ICAMD_ETC2_COLOUR_PLANAR_TH);
}

// Every argument is checked before any device work, in the order of icamd_encode_etc2_device; then the codec's own encode
// and, where the pair has one, the colour-mode pass on the same stream over the same grid
int icamd_encode_etc2_colour_device(int codec, int etc_strategy, int colour_modes, int src_components, int swap_rb,
                                    uint32_t height, uint32_t width, uint32_t grid_height, uint32_t grid_width,
                                    uint32_t row_stride_bytes, uint32_t n_images,
                                    size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                                    const void *d_src, void *d_dst, void *hip_stream) try {
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  if (codec != ICAMD_ETC2_RGBA8 && codec != ICAMD_ETC2_RGB8 && codec != ICAMD_ETC2_RGB8A1)
    return fail(ICAMD_ERR_ARG, "icamd_encode_etc2_colour_device encodes ICAMD_ETC2_RGBA8, ICAMD_ETC2_RGB8 and ICAMD_ETC2_RGB8A1 only");
  if (colour_modes != ICAMD_ETC2_COLOUR_DEFAULT && colour_modes != ICAMD_ETC2_COLOUR_PLANAR &&
      colour_modes != ICAMD_ETC2_COLOUR_PLANAR_TH)
    return fail(ICAMD_ERR_ARG, "colour_modes must be ICAMD_ETC2_COLOUR_DEFAULT, _PLANAR or _PLANAR_TH");
  if (!etc2_colour_accepts(codec, src_components))
    return fail(ICAMD_ERR_ARG, "src_components must be 4 (ICAMD_ETC2_RGB8: 3 or 4)");
  if (n_images == 0) return ICAMD_OK;  // (before the stride, as in icamd_encode_device)
  if (row_stride_bytes < width * (uint32_t)src_components) return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  if (codec == ICAMD_ETC2_RGB8 && colour_modes == ICAMD_ETC2_COLOUR_PLANAR_TH)
    return icamd_encode_etc2_device(codec, etc_strategy, ICAMD_ETC2_MODES_TH, src_components, swap_rb, height, width, grid_height,
                                    grid_width, row_stride_bytes, n_images, src_image_stride_bytes, dst_image_stride_bytes, d_src,
                                    d_dst, hip_stream);
  const int rc = icamd_encode_device(codec, etc_strategy, src_components, swap_rb, height, width, grid_height, grid_width,
                                     row_stride_bytes, n_images, src_image_stride_bytes, dst_image_stride_bytes, d_src, d_dst,
                                     hip_stream);
  if (rc != ICAMD_OK || !etc2_colour_has_pass(codec, colour_modes)) return rc;
  const icamd::GridParams P = grid_params(d_src, d_dst, height, width, grid_height, grid_width, row_stride_bytes, n_images,
                                          src_image_stride_bytes, dst_image_stride_bytes, swap_rb, (uint32_t)etc_strategy);
  ICAMD_HIP(icamd::launch_etc2_colour_modes(codec, colour_modes, P, static_cast<hipStream_t>(hip_stream)),
            "launch etc2 colour modes");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

const char *icamd_etc2_colour_kernel_name(int codec, int src_components, int colour_modes) {
  if (codec == ICAMD_BC7 || bc1a_bc2_codec(codec)) return "";  // (as for an unknown codec)
  if (colour_modes == ICAMD_ETC2_COLOUR_DEFAULT) return icamd_kernel_name(codec, src_components);
  if ((colour_modes != ICAMD_ETC2_COLOUR_PLANAR && colour_modes != ICAMD_ETC2_COLOUR_PLANAR_TH) ||
      !etc2_colour_accepts(codec, src_components))
    return "";
  if (etc2_colour_has_pass(codec, colour_modes)) return icamd::etc2_colour_modes_kernel_name(codec, colour_modes);
  if (codec == ICAMD_ETC2_RGB8 && colour_modes == ICAMD_ETC2_COLOUR_PLANAR_TH)
    return icamd_etc2_kernel_name(codec, src_components, ICAMD_ETC2_MODES_TH);
  return icamd_kernel_name(codec, src_components);  // PLANAR of ICAMD_ETC2_RGB8 and ICAMD_ETC2_RGB8A1 is icamd_encode_device
}

int icamd_pvrtc2_encode_region_device(uint32_t size, uint32_t first_block, uint32_t n_blocks, const void *d_src,
                                      void *d_dst_region, void *hip_stream) try {
  if (!d_src || !d_dst_region || n_blocks == 0) return ICAMD_FALSE;
  if (!pvrtc_size_ok(size, size)) return ICAMD_FALSE;  // as icamd_encode_device
  const uint64_t blocks = (uint64_t)(size / 8) * (size / 4);
  if (!is_pow2(n_blocks) || (first_block & (n_blocks - 1u)) != 0 || (uint64_t)first_block + n_blocks > blocks)
    return fail(ICAMD_ERR_ARG, "PVRTC region must be a power-of-two, aligned range of the image's blocks");
  if (reinterpret_cast<uintptr_t>(d_src) % 16u || reinterpret_cast<uintptr_t>(d_dst_region) % 8u)
    return fail(ICAMD_ERR_ARG, "PVRTC: source must be 16-byte aligned, output 8-byte aligned");
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  icamd::PvrtcParams P = pvrtc_params(d_src, d_dst_region, size, 1, 0, 0);
  P.region_first = first_block;
  P.region_blocks = n_blocks;
  ICAMD_HIP(icamd::launch_pvrtc2(P, static_cast<hipStream_t>(hip_stream)), "launch pvrtc2 region");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

int icamd_host_register(void *host_ptr, size_t bytes) try {
  if (!host_ptr || bytes == 0) return fail(ICAMD_ERR_ARG, "icamd_host_register: null buffer");
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  ICAMD_HIP(hipHostRegister(host_ptr, bytes, hipHostRegisterDefault), "hipHostRegister");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

int icamd_host_unregister(void *host_ptr) try {
  if (!host_ptr) return fail(ICAMD_ERR_ARG, "icamd_host_unregister: null buffer");
  ICAMD_HIP(hipHostUnregister(host_ptr), "hipHostUnregister");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

size_t icamd_pvrtc2_workspace_size(uint32_t size, uint32_t n_images) {
  if (!is_pow2(size) || size < 8) return 0;
  return icamd::pvrtc2_workspace_bytes(size, n_images);
}

size_t icamd_pvrtc4_workspace_size(uint32_t size, uint32_t n_images) {
  if (!is_pow2(size) || size < 8) return 0;
  return icamd::pvrtc4_workspace_bytes(size, n_images);
}

int icamd_pvrtc2_set_workspace(void *d_workspace, size_t bytes) try {
  if (d_workspace && reinterpret_cast<uintptr_t>(d_workspace) % 8u) return fail(ICAMD_ERR_ARG, "workspace must be 8-byte aligned");
  if (d_workspace) {
    // the kernels of this thread's later calls write through this pointer: it must be device memory of the current device
    hipPointerAttribute_t attr;
    int dev = -1;
    if (hipPointerGetAttributes(&attr, d_workspace) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        attr.type != hipMemoryTypeDevice || attr.device != dev) {
      (void)hipGetLastError();
      return fail(ICAMD_ERR_ARG, "workspace must be device memory of the current HIP device");
    }
  }
  icamd::pvrtc2_set_workspace(d_workspace, bytes);
  return ICAMD_OK;
} ICAMD_ABI_CATCH

int icamd_pvrtc2_tune(int mode, int log2_strip) try {
  if (mode < 0 || mode > 2) return fail(ICAMD_ERR_ARG, "icamd_pvrtc2_tune: mode must be 0 (auto), 1 (two kernels) or 2 (one pass)");
  icamd::pvrtc2_tune(mode, log2_strip);
  return ICAMD_OK;
} ICAMD_ABI_CATCH

int icamd_compress_and_pad_device(int compressor, int etc_strategy, int format,
                                  uint32_t height, uint32_t width,
                                  uint32_t padded_height, uint32_t padded_width,
                                  uint32_t padding_bytes_per_row,
                                  const void *d_buffer, void *d_out, size_t out_size, void *hip_stream) try {
  if (compressor == ICAMD_COMPRESSOR_PVRTC) return ICAMD_FALSE;  // pvrtc.cc:684-691
  // dxtc.cc:799-818 / etc.cc:787-800
  if (!d_buffer || !d_out || height == 0 || width == 0) return ICAMD_FALSE;
  int codec, comps;
  bool swap;
  if (!resolve_codec(compressor, format, &codec, &comps, &swap)) return ICAMD_FALSE;
  const uint32_t gh = std::max(height, padded_height), gw = std::max(width, padded_width);
  const size_t need = icamd_encoded_size(codec, gh, gw);
  if (out_size != need) return ICAMD_FALSE;  // compressor4x4_helper.cc:34-41
  return icamd_encode_device(codec, etc_strategy, comps, swap, height, width, gh, gw,
                             width * (uint32_t)comps + padding_bytes_per_row, 1, 0, 0, d_buffer, d_out, hip_stream);
} ICAMD_ABI_CATCH

int icamd_compress_device(int compressor, int etc_strategy, int format,
                          uint32_t height, uint32_t width, uint32_t padding_bytes_per_row,
                          const void *d_buffer, void *d_out, size_t out_size, void *hip_stream) try {
  if (compressor == ICAMD_COMPRESSOR_PVRTC) {
    if (!d_buffer || !d_out || !pvrtc_compress_ok(height, width, padding_bytes_per_row, out_size)) return ICAMD_FALSE;
    return icamd_encode_device(ICAMD_PVRTC2, 0, 4, 0, height, width, height, width, width * 4u, 1, 0, 0,
                               d_buffer, d_out, hip_stream);
  }
  return icamd_compress_and_pad_device(compressor, etc_strategy, format, height, width, height, width,
                                       padding_bytes_per_row, d_buffer, d_out, out_size, hip_stream);
} ICAMD_ABI_CATCH

// Source bytes per band of the host-buffer pipeline (whole block rows): the kernel and the D2H copy of band i run
// underneath the H2D copy of band i+1.  Measured on the MI355X box (r02, one 4096^2 kRGB image = 48 MiB, pageable
// buffers, ms per call): bands of 2 / 4 / 8 / 16 / 24 / 32 MiB -> 2.33 / 1.91 / 1.38 / 1.32 / 1.21 / 1.09 (one band):
// a PCIe copy needs tens of MiB to reach its ~50 GB/s, and there is little to hide (D2H + kernel = 15 % of the H2D
// time), so bands are large and images below 64 MiB go in one piece.
constexpr size_t kHostBandBytes = (size_t)32 << 20;

// The host-buffer drop-in (Compressor::Compress / CompressAndPad, compressor.h:77-80,114-119): argument validation
// first (nothing is staged or copied for a call the reference would refuse), then DXT / ETC images are cut into bands
// of whole block rows -- blocks are independent and stored row-major (helper.h:202-214), so a band is an image of its
// own and its blocks are one contiguous byte range of the output -- and band i's H2D copy, kernel and D2H copy are
// enqueued on stream i % 2: the copy engines and the kernel of consecutive bands overlap.  Caller buffers that are
// page-locked (icamd_host_register, or allocated pinned) are DMA-ed directly at the PCIe rate; pageable ones go through the
// runtime's own staging.  PVRTC (toroidal neighbourhood, Z-order output) is staged whole.  Batch workers copy from
// pageable memory too: page-locked mirrors measured 10 / 14 / 20 / 22 GB/s with 1 / 2 / 4 / 8 workers against 21 GB/s
// for one pageable worker (r01, 32 x 2048^2 kRGB -> DXT1) -- the extra CPU memcpy costs more than the DMA gains.
static int compress_host_common(Staging &st, bool and_pad, int compressor, int etc_strategy, int format,
                                uint32_t height, uint32_t width, uint32_t padded_height, uint32_t padded_width,
                                uint32_t padding_bytes_per_row, const uint8_t *buffer, uint8_t *out,
                                size_t out_size) {
  if (!buffer || !out || height == 0 || width == 0) return ICAMD_FALSE;
  const bool pvrtc = compressor == ICAMD_COMPRESSOR_PVRTC;
  int codec = ICAMD_PVRTC2, comps = 4;  // PVRTC: the buffer is reinterpreted as RGBA8888 whatever `format`, pvrtc.cc:664
  bool swap = false;
  uint32_t gh = height, gw = width;
  if (pvrtc) {
    if (and_pad) return ICAMD_FALSE;  // pvrtc.cc:684-691
    if (!pvrtc_compress_ok(height, width, padding_bytes_per_row, out_size)) return ICAMD_FALSE;
  } else {
    if (!resolve_codec(compressor, format, &codec, &comps, &swap)) return ICAMD_FALSE;  // dxtc.cc:735-750, etc.cc:747-758
    gh = std::max(height, padded_height);
    gw = std::max(width, padded_width);
    if (out_size != icamd_encoded_size(codec, gh, gw)) return ICAMD_FALSE;  // compressor4x4_helper.cc:34-41
  }
  const size_t stride = (size_t)width * comps + padding_bytes_per_row;
  // the reference never touches the padding after the LAST row (pixel4x4.h:47-48 addresses row * stride + col)
  const size_t in_bytes = (size_t)(height - 1) * stride + (size_t)width * comps;
  if (pvrtc)  // (no row padding: the stride fits 32 bits)
    return staged_blockop(st, buffer, in_bytes, out, out_size, out_size, false, [&](void *din, void *dout, hipStream_t s) {
      return pvrtc_encode_device_impl(ICAMD_PVRTC2, 4, height, width, width * 4u, 1, 0, 0, din, dout, s, true);
    });
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  if (stride > 0xffffffffull) return fail(ICAMD_ERR_ARG, "row stride does not fit 32 bits");
  rc = st.ensure(in_bytes, std::max<size_t>(out_size, 1));
  if (rc != ICAMD_OK) return rc;
  uint8_t *d_in = static_cast<uint8_t *>(st.d_in), *d_out = static_cast<uint8_t *>(st.d_out);
  const uint32_t block_bytes = icamd::codec_block_bytes(codec);
  const uint32_t img_block_rows = num_blocks4(height), grid_block_rows = num_blocks4(gh), block_cols = num_blocks4(gw);
  uint64_t band_rows = std::max<uint64_t>(1, kHostBandBytes / (4u * stride));  // block rows per band
  if (band_rows * 2 > img_block_rows) band_rows = img_block_rows;               // small images: one band
  int status = ICAMD_OK;
  uint32_t band = 0;
  for (uint64_t r0 = 0; r0 < img_block_rows && status == ICAMD_OK; r0 += band_rows, ++band) {
    const bool last = r0 + band_rows >= img_block_rows;
    const uint32_t rows_b = (uint32_t)(last ? img_block_rows - r0 : band_rows);        // block rows with pixels
    const uint32_t h_b = (uint32_t)std::min<uint64_t>((uint64_t)rows_b * 4u, height - r0 * 4u);
    const uint32_t grid_rows_b = last ? (uint32_t)(grid_block_rows - r0) : rows_b;     // + the pad rows below the image
    const size_t src_off = (size_t)r0 * 4u * stride;
    const size_t src_len = (size_t)(h_b - 1) * stride + (size_t)width * comps;
    const size_t dst_off = (size_t)r0 * block_cols * block_bytes, dst_len = (size_t)grid_rows_b * block_cols * block_bytes;
    hipStream_t s = (band & 1u) ? st.stream2 : st.stream;
    hipError_t e = hipMemcpyAsync(d_in + src_off, buffer + src_off, src_len, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { status = fail(ICAMD_ERR_HIP, "H2D copy", e); break; }
    status = icamd_encode_device(codec, etc_strategy, comps, swap, h_b, width, grid_rows_b * 4u, gw, (uint32_t)stride, 1, 0,
                                 0, d_in + src_off, d_out + dst_off, s);
    if (status != ICAMD_OK) break;
    e = hipMemcpyAsync(out + dst_off, d_out + dst_off, dst_len, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) status = fail(ICAMD_ERR_HIP, "D2H copy", e);
  }
  const hipError_t e1 = hipStreamSynchronize(st.stream), e2 = hipStreamSynchronize(st.stream2);
  if (status != ICAMD_OK) return status;
  if (e1 != hipSuccess || e2 != hipSuccess) return fail(ICAMD_ERR_HIP, "stream synchronize", e1 != hipSuccess ? e1 : e2);
  return ICAMD_OK;
}

int icamd_compress(int compressor, int etc_strategy, int format, uint32_t height, uint32_t width,
                   uint32_t padding_bytes_per_row, const uint8_t *buffer, uint8_t *out, size_t out_size) try {
  return compress_host_common(tls_staging(), false, compressor, etc_strategy, format, height, width, height, width,
                              padding_bytes_per_row, buffer, out, out_size);
} ICAMD_ABI_CATCH

int icamd_compress_and_pad(int compressor, int etc_strategy, int format, uint32_t height, uint32_t width,
                           uint32_t padded_height, uint32_t padded_width, uint32_t padding_bytes_per_row,
                           const uint8_t *buffer, uint8_t *out, size_t out_size) try {
  return compress_host_common(tls_staging(), true, compressor, etc_strategy, format, height, width, padded_height,
                              padded_width, padding_bytes_per_row, buffer, out, out_size);
} ICAMD_ABI_CATCH

// Blocks per block row of a stored image.  PVRTC 2 bpp: 8x4-pixel blocks
static uint32_t codec_block_cols(int codec, uint32_t width) { return codec == ICAMD_PVRTC2 ? width / 8u : num_blocks4(width); }

// The launches of a checked decode call, one per piece of decode_plan.h (the decode kernels index blocks with 32 bits): whole
// images, or bands of block rows of a single image of 2^31 blocks or more.
static int decode_pieces(int codec, int swap_rb, uint32_t height, uint32_t width, uint32_t row_stride, uint32_t n_images,
                         size_t src_image_stride, size_t dst_image_stride, const void *d_blocks, void *d_pixels, void *hip_stream) {
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const uint8_t *blocks = static_cast<const uint8_t *>(d_blocks);
  uint8_t *pixels = static_cast<uint8_t *>(d_pixels);
  const uint32_t block_cols = codec_block_cols(codec, width);
  const uint64_t block_row_bytes = (uint64_t)block_cols * icamd::codec_block_bytes(codec);
  return icamd::for_each_launch_piece(height, block_cols, n_images, [&](const icamd::LaunchPiece &piece) -> int {
    const icamd::DecodeParams P = icamd::decode_params(
        blocks + piece.first_image * src_image_stride + piece.first_block_row * block_row_bytes,
        pixels + piece.first_image * dst_image_stride + (uint64_t)piece.first_block_row * 4u * row_stride, src_image_stride,
        dst_image_stride, piece.pixel_rows, width, block_cols, row_stride, piece.image_count, swap_rb != 0);
    if (codec == ICAMD_ETC2_RGBA8)
      ICAMD_HIP(icamd::launch_etc2_decode(P, stream), "launch etc2 decode");
    else if (codec == ICAMD_ETC2_RGB8)
      ICAMD_HIP(icamd::launch_etc2_rgb8_decode(P, stream), "launch etc2 rgb8 decode");
    else if (codec == ICAMD_ETC2_RGB8A1)
      ICAMD_HIP(icamd::launch_etc2_a1_decode(P, stream), "launch etc2 rgb8a1 decode");
    else if (codec == ICAMD_BC7)
      ICAMD_HIP(icamd::launch_bc7_decode(P, stream), "launch bc7 decode");
    else if (codec == ICAMD_BC6H_UF16 || codec == ICAMD_BC6H_SF16)  // (icamd_decode_bc6h_device only: RGBA16F rows)
      ICAMD_HIP(icamd::launch_bc6h_decode(codec, P, stream), "launch bc6h decode");
    else
      ICAMD_HIP(icamd::launch_decode(codec, P, stream), "launch decode");
    return ICAMD_OK;
  });
}

int icamd_decode_device(int codec, int swap_rb, uint32_t height, uint32_t width, uint32_t padding_bytes_per_row,
                        uint32_t n_images, size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                        const void *d_blocks, void *d_pixels, void *hip_stream) try {
  if (!d_blocks || !d_pixels || height == 0 || width == 0) return ICAMD_FALSE;
  const bool plane = plane_codec(codec);  // (BC4 / BC5 and EAC R11 / RG11: R8 / RG8 rows)
  if (codec != ICAMD_DXT1 && codec != ICAMD_DXT5 && codec != ICAMD_ETC1 && codec != ICAMD_PVRTC2 && codec != ICAMD_PVRTC4 &&
      codec != ICAMD_ETC2_RGBA8 && codec != ICAMD_ETC2_RGB8 && codec != ICAMD_ETC2_RGB8A1 && codec != ICAMD_BC7 &&
      !bc1a_bc2_codec(codec) && !plane)
    return ICAMD_FALSE;
  if (plane && swap_rb) return fail(ICAMD_ERR_ARG, eac11_codec(codec) ? "EAC R11 / RG11 decode: swap_rb must be 0" : "BC4 / BC5 decode: swap_rb must be 0");
  if (n_images == 0) return ICAMD_OK;
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  const uint32_t row_stride = width * icamd::codec_decoded_pixel_bytes(codec) + padding_bytes_per_row;
  if (plane) {
    // EXTENSION (include/ic_amd.h ICAMD_BC4, ICAMD_EAC_R11): R8 / RG8 rows; 64-bit addressing and chunked grids, so no banding is needed
    const icamd::Bc45DecodeParams P =
        icamd::bc45_decode_params(static_cast<const uint8_t *>(d_blocks), static_cast<uint8_t *>(d_pixels), src_image_stride_bytes,
                                  dst_image_stride_bytes, height, width, row_stride);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (eac11_codec(codec))
      ICAMD_HIP(icamd::launch_eac11_decode(codec, n_images, P, stream), "launch eac r11 / rg11 decode");
    else
      ICAMD_HIP(icamd::launch_bc45_decode(codec, n_images, P, stream), "launch bc4 / bc5 decode");
    return ICAMD_OK;
  }
  const bool pvrtc = codec == ICAMD_PVRTC2 || codec == ICAMD_PVRTC4;
  if (pvrtc) {
    // EXTENSION (the reference's PvrtcCompressor::Decompress returns false, pvrtc.cc:669-672; 4 bpp: no such format there at
    // all): the sizes PvrtcCompressor::Compress accepts (pvrtc.cc:636-650), RGBA8 out, no row padding, one launch per <= 2^30 blocks
    if (!is_pow2(width) || width != height || width < 8 || padding_bytes_per_row != 0) return ICAMD_FALSE;
    swap_rb = 0;
    if ((uint64_t)num_blocks4(height) * codec_block_cols(codec, width) > icamd::kMaxLaunchBlocks)
      return fail(ICAMD_ERR_ARG, "PVRTC texture too large to decode");
  }
  return decode_pieces(codec, swap_rb, height, width, row_stride, n_images, src_image_stride_bytes, dst_image_stride_bytes, d_blocks,
                       d_pixels, hip_stream);
} ICAMD_ABI_CATCH

int icamd_decompress(int compressor, int format, uint32_t height, uint32_t width, uint32_t padding_bytes_per_row,
                     const uint8_t *blocks, size_t blocks_size, uint8_t *out, size_t out_size) try {
  if (!blocks || !out || height == 0 || width == 0) return ICAMD_FALSE;
  int codec, comps;
  bool swap;
  if (!resolve_codec(compressor, format, &codec, &comps, &swap)) return ICAMD_FALSE;
  if (blocks_size != icamd_encoded_size(codec, height, width)) return ICAMD_FALSE;
  const size_t need = (size_t)height * ((size_t)width * comps + padding_bytes_per_row);
  if (out_size != need) return ICAMD_FALSE;
  return staged_blockop(tls_staging(), blocks, blocks_size, out, need, need, false, [&](void *din, void *dout, hipStream_t s) {
    if (padding_bytes_per_row) ICAMD_HIP(hipMemsetAsync(dout, 0, need, s), "memset");
    return icamd_decode_device(codec, swap, height, width, padding_bytes_per_row, 1, 0, 0, din, dout, s);
  });
} ICAMD_ABI_CATCH

// EXTENSION (parity unpinned, see icamd_decode_device): host-buffer PVRTC 2bpp decode.  Kept apart from
// icamd_decompress, which answers ICAMD_FALSE for PVRTC like the reference (pvrtc_compressor.cc:669-672).
int icamd_pvrtc2_decompress(uint32_t size, const uint8_t *blocks, size_t blocks_size, uint8_t *out, size_t out_size) try {
  if (!blocks || !out || !is_pow2(size) || size < 8) return ICAMD_FALSE;
  if (blocks_size != (size_t)size * size / 4 || out_size != (size_t)size * size * 4) return ICAMD_FALSE;
  return staged_blockop(tls_staging(), blocks, blocks_size, out, out_size, out_size, false,
                        [&](void *din, void *dout, hipStream_t s) {
                          return icamd_decode_device(ICAMD_PVRTC2, 0, size, size, 0, 1, 0, 0, din, dout, s);
                        });
} ICAMD_ABI_CATCH

// ---- quality metric (extension, include/ic_amd.h): blocks against source pixels

// The launches of a checked metric call: the records are zeroed, then one launch per piece of decode_plan.h over the images' own
// block grids (grid_width gives the pitch of a block row of the stored grid).  The bands of a single image of 2^31 blocks or more
// all add to the image's one record.
using MetricLauncher = hipError_t (*)(int codec, int comps, const icamd::MetricParams &P, hipStream_t stream);
static int metric_pieces(MetricLauncher launch, const char *what, int codec, int comps, int swap_rb, uint32_t height, uint32_t width,
                         uint32_t grid_width, uint32_t row_stride, uint32_t n_images, size_t src_image_stride,
                         size_t blocks_image_stride, const void *d_src, const void *d_blocks, void *d_stats, void *hip_stream) {
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const uint8_t *src = static_cast<const uint8_t *>(d_src), *blocks = static_cast<const uint8_t *>(d_blocks);
  uint8_t *stats = static_cast<uint8_t *>(d_stats);
  ICAMD_HIP(icamd::launch_metric_clear(stats, n_images, stream), "launch metric clear");
  const uint32_t block_cols = codec_block_cols(codec, width), grid_cols = num_blocks4(grid_width);
  const uint64_t grid_row_bytes = (uint64_t)grid_cols * icamd::codec_block_bytes(codec);
  return icamd::for_each_launch_piece(height, block_cols, n_images, [&](const icamd::LaunchPiece &piece) -> int {
    const icamd::MetricParams P = icamd::metric_params(
        src + piece.first_image * src_image_stride + (uint64_t)piece.first_block_row * 4u * row_stride,
        blocks + piece.first_image * blocks_image_stride + piece.first_block_row * grid_row_bytes,
        stats + piece.first_image * sizeof(icamd_error_stats), src_image_stride, blocks_image_stride, piece.pixel_rows, width,
        block_cols, grid_cols, row_stride, piece.image_count, swap_rb != 0);
    ICAMD_HIP(launch(codec, comps, P, stream), what);
    return ICAMD_OK;
  });
}

int icamd_measure_error_device(int codec, int src_components, int swap_rb, uint32_t height, uint32_t width,
                               uint32_t grid_height, uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                               size_t src_image_stride_bytes, size_t blocks_image_stride_bytes, const void *d_src,
                               const void *d_blocks, void *d_stats, void *hip_stream) try {
  if (!d_src || !d_blocks || !d_stats || height == 0 || width == 0) return ICAMD_FALSE;
  const bool pvrtc = codec == ICAMD_PVRTC2 || codec == ICAMD_PVRTC4;
  if (!pvrtc && !codec_accepts_components(codec, 4)) return fail(ICAMD_ERR_ARG, "unknown codec");  // (every codec takes 4)
  if (pvrtc ? src_components != 4 : !codec_accepts_components(codec, src_components))
    return fail(ICAMD_ERR_ARG, "the codec does not encode from that many source components");
  if (swap_rb && src_components < 3) return fail(ICAMD_ERR_ARG, "swap_rb needs a 3- or 4-component source");
  if ((uint64_t)row_stride_bytes < (uint64_t)width * (uint32_t)src_components)
    return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  if (grid_height < height || grid_width < width) return fail(ICAMD_ERR_ARG, "block grid smaller than the image");
  if (reinterpret_cast<uintptr_t>(d_stats) % 8u) return fail(ICAMD_ERR_ARG, "d_stats must be 8-byte aligned");
  if ((uint64_t)height * width > (1ull << 47)) return fail(ICAMD_ERR_ARG, "more than 2^47 pixels in one image");
  if (pvrtc) {  // what the PVRTC decoders need (icamd_decode_device), and the encoder's row rule
    if (!is_pow2(width) || width != height || width < 8 || grid_height != height || grid_width != width ||
        row_stride_bytes != width * 4u)
      return ICAMD_FALSE;
    if ((uint64_t)num_blocks4(height) * codec_block_cols(codec, width) > icamd::kMaxLaunchBlocks)
      return fail(ICAMD_ERR_ARG, "PVRTC texture too large to decode");
    swap_rb = 0;
  }
  if (n_images == 0) return ICAMD_OK;
  const int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  return metric_pieces(icamd::launch_metric, "launch metric", codec, src_components, swap_rb, height, width, grid_width,
                       row_stride_bytes, n_images, src_image_stride_bytes, blocks_image_stride_bytes, d_src, d_blocks, d_stats, hip_stream);
} ICAMD_ABI_CATCH

int icamd_measure_error(int compressor, int format, uint32_t height, uint32_t width, uint32_t padding_bytes_per_row,
                        const uint8_t *buffer, const uint8_t *blocks, size_t blocks_size, icamd_error_stats *out) try {
  if (!buffer || !blocks || !out || height == 0 || width == 0) return ICAMD_FALSE;
  int codec = ICAMD_PVRTC2, comps = 4;
  bool swap = false;
  if (compressor == ICAMD_COMPRESSOR_PVRTC) {  // pvrtc.cc:607-609, 636-667: kRGBA, no row padding
    if (format != ICAMD_RGBA || !pvrtc_compress_ok(height, width, padding_bytes_per_row, blocks_size)) return ICAMD_FALSE;
  } else {
    if (!resolve_codec(compressor, format, &codec, &comps, &swap)) return ICAMD_FALSE;
    if (blocks_size != icamd_encoded_size(codec, height, width)) return ICAMD_FALSE;
  }
  const size_t stride = (size_t)width * comps + padding_bytes_per_row;
  if (stride > 0xffffffffull) return fail(ICAMD_ERR_ARG, "row stride does not fit 32 bits");
  const size_t in_bytes = (size_t)(height - 1) * stride + (size_t)width * comps;  // as icamd_compress: no padding after the last row
  const size_t blocks_at = (in_bytes + 15u) & ~(size_t)15u;
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  Staging &st = tls_staging();
  rc = st.ensure(blocks_at + blocks_size, sizeof(icamd_error_stats));
  if (rc != ICAMD_OK) return rc;
  hipStream_t s = st.stream;
  uint8_t *d_in = static_cast<uint8_t *>(st.d_in);
  ICAMD_HIP(hipMemcpyAsync(d_in, buffer, in_bytes, hipMemcpyHostToDevice, s), "H2D copy");
  ICAMD_HIP(hipMemcpyAsync(d_in + blocks_at, blocks, blocks_size, hipMemcpyHostToDevice, s), "H2D copy");
  rc = icamd_measure_error_device(codec, comps, swap, height, width, height, width, (uint32_t)stride, 1, 0, 0, d_in,
                                  d_in + blocks_at, st.d_out, s);
  if (rc != ICAMD_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  ICAMD_HIP(hipMemcpyAsync(out, st.d_out, sizeof(icamd_error_stats), hipMemcpyDeviceToHost, s), "D2H copy");
  ICAMD_HIP(hipStreamSynchronize(s), "stream synchronize");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

const char *icamd_metric_kernel_name(int codec, int src_components) { return icamd::metric_kernel_name(codec, src_components); }

// ---- 16-bit and signed EAC R11 / RG11 (EXTENSION, include/ic_amd.h icamd_encode_eac11_16_device; csrc/eac11_16_kernels.hip) ----
// Every argument check comes before any device work.
static bool eac11_16_codec(int codec) {
  return codec == ICAMD_EAC_R11 || codec == ICAMD_EAC_RG11 || codec == ICAMD_EAC_SIGNED_R11 || codec == ICAMD_EAC_SIGNED_RG11;
}
static bool eac11_16_two(int codec) { return codec == ICAMD_EAC_RG11 || codec == ICAMD_EAC_SIGNED_RG11; }
// The source rules the encoder and the metric share: the codec, the channel count, 2-byte alignment of the samples.
static int eac11_16_check_source(int codec, int src_channels, uint32_t row_stride_bytes, size_t src_image_stride_bytes,
                                 const void *d_src) {
  if (!eac11_16_codec(codec)) return fail(ICAMD_ERR_ARG, "16-bit EAC: the codec must be EAC R11 / RG11 or signed EAC R11 / RG11");
  if (src_channels < (eac11_16_two(codec) ? 2 : 1) || src_channels > 4)
    return fail(ICAMD_ERR_ARG, eac11_16_two(codec) ? "16-bit EAC RG11 needs 2, 3 or 4 source channels"
                                                   : "16-bit EAC R11 needs 1 to 4 source channels");
  if (reinterpret_cast<uintptr_t>(d_src) % 2u || row_stride_bytes % 2u || src_image_stride_bytes % 2u)
    return fail(ICAMD_ERR_ARG, "16-bit EAC: d_src, row_stride_bytes and src_image_stride_bytes must be even");
  return ICAMD_OK;
}

int icamd_encode_eac11_16_device(int codec, int src_channels, uint32_t height, uint32_t width, uint32_t grid_height,
                                 uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                                 size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                                 const void *d_src, void *d_dst, void *hip_stream) try {
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  int rc = eac11_16_check_source(codec, src_channels, row_stride_bytes, src_image_stride_bytes, d_src);
  if (rc != ICAMD_OK) return rc;
  if (n_images == 0) return ICAMD_OK;
  if ((uint64_t)row_stride_bytes < (uint64_t)width * (uint32_t)src_channels * 2u)
    return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  rc = require_device();
  if (rc != ICAMD_OK) return rc;
  const icamd::GridParams P = grid_params(d_src, d_dst, height, width, grid_height, grid_width, row_stride_bytes, n_images,
                                          src_image_stride_bytes, dst_image_stride_bytes, 0, 0);
  ICAMD_HIP(icamd::launch_eac11_16_encode(codec, src_channels, P, static_cast<hipStream_t>(hip_stream)), "launch 16-bit eac r11 / rg11");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

int icamd_decode_eac11_16_device(int codec, uint32_t height, uint32_t width, uint32_t padding_bytes_per_row, uint32_t n_images,
                                 size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                                 const void *d_blocks, void *d_pixels, void *hip_stream) try {
  if (!d_blocks || !d_pixels || height == 0 || width == 0) return ICAMD_FALSE;
  if (!eac11_16_codec(codec)) return fail(ICAMD_ERR_ARG, "16-bit EAC: the codec must be EAC R11 / RG11 or signed EAC R11 / RG11");
  if (padding_bytes_per_row % 2u || reinterpret_cast<uintptr_t>(d_pixels) % 2u || dst_image_stride_bytes % 2u)
    return fail(ICAMD_ERR_ARG, "16-bit EAC decode: padding_bytes_per_row, d_pixels and dst_image_stride_bytes must be even");
  const uint64_t row_bytes = (uint64_t)width * (eac11_16_two(codec) ? 4u : 2u) + padding_bytes_per_row;
  if (row_bytes > 0xffffffffull) return fail(ICAMD_ERR_ARG, "16-bit EAC decode: a row of 2^32 bytes or more");
  if (n_images == 0) return ICAMD_OK;
  const int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  const icamd::Bc45DecodeParams P =
      icamd::bc45_decode_params(static_cast<const uint8_t *>(d_blocks), static_cast<uint8_t *>(d_pixels), src_image_stride_bytes,
                                dst_image_stride_bytes, height, width, (uint32_t)row_bytes);
  ICAMD_HIP(icamd::launch_eac11_16_decode(codec, n_images, P, static_cast<hipStream_t>(hip_stream)), "launch 16-bit eac r11 / rg11 decode");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

int icamd_measure_error_eac11_16_device(int codec, int src_channels, uint32_t height, uint32_t width,
                                        uint32_t grid_height, uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                                        size_t src_image_stride_bytes, size_t blocks_image_stride_bytes,
                                        const void *d_src, const void *d_blocks, void *d_stats, void *hip_stream) try {
  if (!d_src || !d_blocks || !d_stats || height == 0 || width == 0) return ICAMD_FALSE;
  int rc = eac11_16_check_source(codec, src_channels, row_stride_bytes, src_image_stride_bytes, d_src);
  if (rc != ICAMD_OK) return rc;
  if ((uint64_t)row_stride_bytes < (uint64_t)width * (uint32_t)src_channels * 2u)
    return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  if (grid_height < height || grid_width < width) return fail(ICAMD_ERR_ARG, "block grid smaller than the image");
  if (reinterpret_cast<uintptr_t>(d_stats) % 8u) return fail(ICAMD_ERR_ARG, "d_stats must be 8-byte aligned");
  if ((uint64_t)height * width > (1ull << 31)) return fail(ICAMD_ERR_ARG, "more than 2^31 pixels in one image");
  if (n_images == 0) return ICAMD_OK;
  rc = require_device();
  if (rc != ICAMD_OK) return rc;
  // an image of at most 2^31 pixels has fewer than 2^31 blocks: whole images only
  return metric_pieces(icamd::launch_eac11_16_metric, "launch 16-bit eac metric", codec, src_channels, 0, height, width, grid_width, row_stride_bytes,
                       n_images, src_image_stride_bytes, blocks_image_stride_bytes, d_src, d_blocks, d_stats, hip_stream);
} ICAMD_ABI_CATCH

const char *icamd_eac11_16_kernel_name(int codec, int src_channels) { return icamd::eac11_16_kernel_name(codec, src_channels); }
const char *icamd_eac11_16_metric_kernel_name(int codec, int src_channels) {
  return icamd::eac11_16_metric_kernel_name(codec, src_channels);
}

// ---- BC6H (EXTENSION, include/ic_amd.h icamd_encode_bc6h_device; csrc/bc6h_kernels.hip) ----
// Every argument check comes before any device work; the order of the checks is that of the 16-bit EAC entry points.
static bool bc6h_codec(int codec) { return codec == ICAMD_BC6H_UF16 || codec == ICAMD_BC6H_SF16; }
// The source rules the encoder and the metric share: the codec, the channel count, 2-byte alignment of the samples.
static int bc6h_check_source(int codec, int src_channels, uint32_t row_stride_bytes, size_t src_image_stride_bytes, const void *d_src) {
  if (!bc6h_codec(codec)) return fail(ICAMD_ERR_ARG, "BC6H: the codec must be ICAMD_BC6H_UF16 or ICAMD_BC6H_SF16");
  if (src_channels != 3 && src_channels != 4) return fail(ICAMD_ERR_ARG, "BC6H needs 3 or 4 source channels");
  if (reinterpret_cast<uintptr_t>(d_src) % 2u || row_stride_bytes % 2u || src_image_stride_bytes % 2u)
    return fail(ICAMD_ERR_ARG, "BC6H: d_src, row_stride_bytes and src_image_stride_bytes must be even");
  return ICAMD_OK;
}

int icamd_encode_bc6h_device(int codec, int src_channels, uint32_t height, uint32_t width, uint32_t grid_height,
                             uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images, size_t src_image_stride_bytes,
                             size_t dst_image_stride_bytes, const void *d_src, void *d_dst, void *hip_stream) try {
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  int rc = bc6h_check_source(codec, src_channels, row_stride_bytes, src_image_stride_bytes, d_src);
  if (rc != ICAMD_OK) return rc;
  if (n_images == 0) return ICAMD_OK;
  if ((uint64_t)row_stride_bytes < (uint64_t)width * (uint32_t)src_channels * 2u)
    return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  rc = require_device();
  if (rc != ICAMD_OK) return rc;
  const icamd::GridParams P = grid_params(d_src, d_dst, height, width, grid_height, grid_width, row_stride_bytes, n_images,
                                          src_image_stride_bytes, dst_image_stride_bytes, 0, 0);
  ICAMD_HIP(icamd::launch_bc6h_encode(codec, src_channels, P, static_cast<hipStream_t>(hip_stream)), "launch bc6h");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

int icamd_decode_bc6h_device(int codec, uint32_t height, uint32_t width, uint32_t padding_bytes_per_row, uint32_t n_images,
                             size_t src_image_stride_bytes, size_t dst_image_stride_bytes, const void *d_blocks, void *d_pixels,
                             void *hip_stream) try {
  if (!d_blocks || !d_pixels || height == 0 || width == 0) return ICAMD_FALSE;
  if (!bc6h_codec(codec)) return fail(ICAMD_ERR_ARG, "BC6H: the codec must be ICAMD_BC6H_UF16 or ICAMD_BC6H_SF16");
  if (padding_bytes_per_row % 2u || reinterpret_cast<uintptr_t>(d_pixels) % 2u || dst_image_stride_bytes % 2u)
    return fail(ICAMD_ERR_ARG, "BC6H decode: padding_bytes_per_row, d_pixels and dst_image_stride_bytes must be even");
  const uint64_t row_bytes = (uint64_t)width * icamd::codec_decoded_pixel_bytes(codec) + padding_bytes_per_row;
  if (row_bytes > 0xffffffffull) return fail(ICAMD_ERR_ARG, "BC6H decode: a row of 2^32 bytes or more");
  if (n_images == 0) return ICAMD_OK;
  const int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  return decode_pieces(codec, 0, height, width, (uint32_t)row_bytes, n_images, src_image_stride_bytes, dst_image_stride_bytes, d_blocks,
                       d_pixels, hip_stream);
} ICAMD_ABI_CATCH

int icamd_measure_error_bc6h_device(int codec, int src_channels, uint32_t height, uint32_t width, uint32_t grid_height,
                                    uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                                    size_t src_image_stride_bytes, size_t blocks_image_stride_bytes, const void *d_src,
                                    const void *d_blocks, void *d_stats, void *hip_stream) try {
  if (!d_src || !d_blocks || !d_stats || height == 0 || width == 0) return ICAMD_FALSE;
  int rc = bc6h_check_source(codec, src_channels, row_stride_bytes, src_image_stride_bytes, d_src);
  if (rc != ICAMD_OK) return rc;
  if ((uint64_t)row_stride_bytes < (uint64_t)width * (uint32_t)src_channels * 2u)
    return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  if (grid_height < height || grid_width < width) return fail(ICAMD_ERR_ARG, "block grid smaller than the image");
  if (reinterpret_cast<uintptr_t>(d_stats) % 8u) return fail(ICAMD_ERR_ARG, "d_stats must be 8-byte aligned");
  if ((uint64_t)height * width > (1ull << 31)) return fail(ICAMD_ERR_ARG, "more than 2^31 pixels in one image");
  if (n_images == 0) return ICAMD_OK;
  rc = require_device();
  if (rc != ICAMD_OK) return rc;
  // an image of at most 2^31 pixels has fewer than 2^31 blocks: whole images only
  return metric_pieces(icamd::launch_bc6h_metric, "launch bc6h metric", codec, src_channels, 0, height, width, grid_width, row_stride_bytes,
                       n_images, src_image_stride_bytes, blocks_image_stride_bytes, d_src, d_blocks, d_stats, hip_stream);
} ICAMD_ABI_CATCH

const char *icamd_bc6h_kernel_name(int codec, int src_channels) { return icamd::bc6h_kernel_name(codec, src_channels); }
const char *icamd_bc6h_metric_kernel_name(int codec, int src_channels) { return icamd::bc6h_metric_kernel_name(codec, src_channels); }

// EXTENSION (include/ic_amd.h ICAMD_BC6H_MODES_EXTENDED): every argument is checked before any device work, in the order of
// icamd_encode_bc6h_device; modes 0 IS icamd_encode_bc6h_device, modes 1 the fused kernel of bc6h_modes_kernels.hip in its place
int icamd_encode_bc6h_modes_device(int codec, int bc6h_modes, int src_channels, uint32_t height, uint32_t width,
                                   uint32_t grid_height, uint32_t grid_width, uint32_t row_stride_bytes, uint32_t n_images,
                                   size_t src_image_stride_bytes, size_t dst_image_stride_bytes, const void *d_src, void *d_dst,
                                   void *hip_stream) try {
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  if (!bc6h_codec(codec)) return fail(ICAMD_ERR_ARG, "BC6H: the codec must be ICAMD_BC6H_UF16 or ICAMD_BC6H_SF16");
  if (bc6h_modes != ICAMD_BC6H_MODES_DEFAULT && bc6h_modes != ICAMD_BC6H_MODES_EXTENDED)
    return fail(ICAMD_ERR_ARG, "bc6h_modes must be ICAMD_BC6H_MODES_DEFAULT or ICAMD_BC6H_MODES_EXTENDED");
  if (bc6h_modes == ICAMD_BC6H_MODES_DEFAULT)
    return icamd_encode_bc6h_device(codec, src_channels, height, width, grid_height, grid_width, row_stride_bytes, n_images,
                                    src_image_stride_bytes, dst_image_stride_bytes, d_src, d_dst, hip_stream);
  int rc = bc6h_check_source(codec, src_channels, row_stride_bytes, src_image_stride_bytes, d_src);
  if (rc != ICAMD_OK) return rc;
  if (n_images == 0) return ICAMD_OK;
  if ((uint64_t)row_stride_bytes < (uint64_t)width * (uint32_t)src_channels * 2u)
    return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  rc = require_device();
  if (rc != ICAMD_OK) return rc;
  const icamd::GridParams P = grid_params(d_src, d_dst, height, width, grid_height, grid_width, row_stride_bytes, n_images,
                                          src_image_stride_bytes, dst_image_stride_bytes, 0, 0);
  ICAMD_HIP(icamd::launch_bc6h_modes_encode(codec, src_channels, P, static_cast<hipStream_t>(hip_stream)), "launch bc6h modes");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

const char *icamd_bc6h_modes_kernel_name(int codec, int src_channels, int bc6h_modes) {
  if (bc6h_modes == ICAMD_BC6H_MODES_DEFAULT) return icamd::bc6h_kernel_name(codec, src_channels);
  if (bc6h_modes == ICAMD_BC6H_MODES_EXTENDED) return icamd::bc6h_modes_kernel_name(codec, src_channels);
  return "";
}

// ---- compressed-domain operations

int icamd_pad_batch_device(int compressor, int etc_strategy, int format, uint32_t ch, uint32_t cw, uint32_t n_images,
                           const void *d_blocks, size_t src_image_stride_bytes, uint32_t ph, uint32_t pw, void *d_out,
                           size_t dst_image_stride_bytes, size_t out_size_per_image, void *hip_stream) try {
  int codec;
  if (!d_blocks || !d_out || !resolve_codec(compressor, format, &codec)) return ICAMD_FALSE;
  if ((reinterpret_cast<uintptr_t>(d_blocks) | reinterpret_cast<uintptr_t>(d_out) | src_image_stride_bytes | dst_image_stride_bytes) % 4u)
    return fail(ICAMD_ERR_ARG, "block pointers and image strides must be 4-byte aligned");
  if (ch == 0 || cw == 0 || !pad_geometry_ok(codec, ch, cw, ph, pw, out_size_per_image)) return ICAMD_FALSE;
  // (a non-zero stride is checked for one image too: a caller that passes one states how far its buffer reaches)
  if (((n_images > 1 || src_image_stride_bytes != 0) && src_image_stride_bytes < icamd_encoded_size(codec, ch, cw)) ||
      ((n_images > 1 || dst_image_stride_bytes != 0) && dst_image_stride_bytes < out_size_per_image))
    return fail(ICAMD_ERR_ARG, "image stride smaller than an image");
  const icamd::BlockOpIn in = { codec, (uint32_t)etc_strategy, num_blocks4(ch), num_blocks4(cw), num_blocks4(ph), num_blocks4(pw),
                                ch, cw, n_images, false };
  return blockop_batch(icamd::launch_pad, "launch pad", in, d_blocks, src_image_stride_bytes, d_out, dst_image_stride_bytes, hip_stream);
} ICAMD_ABI_CATCH

int icamd_pad_device(int compressor, int etc_strategy, int format, uint32_t ch, uint32_t cw, const void *d_blocks,
                     uint32_t ph, uint32_t pw, void *d_out, size_t out_size, void *hip_stream) try {
  return icamd_pad_batch_device(compressor, etc_strategy, format, ch, cw, 1, d_blocks, 0, ph, pw, d_out, 0, out_size, hip_stream);
} ICAMD_ABI_CATCH

int icamd_downsample_batch_device(int compressor, int etc_strategy, int format, uint32_t uh, uint32_t uw, uint32_t n_images,
                                  const void *d_blocks, size_t src_image_stride_bytes, void *d_out,
                                  size_t dst_image_stride_bytes, size_t out_size_per_image, void *hip_stream) try {
  int codec;
  if (!d_blocks || !d_out || uh == 0 || uw == 0 || !resolve_codec(compressor, format, &codec)) return ICAMD_FALSE;
  if ((reinterpret_cast<uintptr_t>(d_blocks) | reinterpret_cast<uintptr_t>(d_out) | src_image_stride_bytes | dst_image_stride_bytes) % 4u)
    return fail(ICAMD_ERR_ARG, "block pointers and image strides must be 4-byte aligned");
  if (!downsample_geometry_ok(codec, uh, uw, out_size_per_image)) return ICAMD_FALSE;
  // (a non-zero stride is checked for one image too: a caller that passes one states how far its buffer reaches)
  if ((n_images > 1 || src_image_stride_bytes != 0) && src_image_stride_bytes < icamd_encoded_size(codec, uh, uw))
    return fail(ICAMD_ERR_ARG, "source image stride smaller than an image");
  if ((n_images > 1 || dst_image_stride_bytes != 0) && dst_image_stride_bytes < out_size_per_image)
    return fail(ICAMD_ERR_ARG, "destination image stride smaller than an image");
  const icamd::BlockOpIn in = { codec, (uint32_t)etc_strategy, num_blocks4(uh), num_blocks4(uw), num_blocks4((uh + 1) / 2),
                                num_blocks4((uw + 1) / 2), uh, uw, n_images, false };
  return blockop_batch(icamd::launch_downsample, "launch downsample", in, d_blocks, src_image_stride_bytes, d_out,
                       dst_image_stride_bytes, hip_stream);
} ICAMD_ABI_CATCH

int icamd_downsample_device(int compressor, int etc_strategy, int format, uint32_t uh, uint32_t uw,
                            const void *d_blocks, void *d_out, size_t out_size, void *hip_stream) try {
  return icamd_downsample_batch_device(compressor, etc_strategy, format, uh, uw, 1, d_blocks, 0, d_out, 0, out_size, hip_stream);
} ICAMD_ABI_CATCH

int icamd_transcode_dxt1_to_etc1_device(void *d_blocks, size_t n_bytes, void *hip_stream) try {
  if (!d_blocks) return ICAMD_FALSE;
  if (reinterpret_cast<uintptr_t>(d_blocks) % 8u) return fail(ICAMD_ERR_ARG, "block pointer must be 8-byte aligned");
  if (n_bytes < 8) return ICAMD_OK;
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  ICAMD_HIP(icamd::launch_transcode_dxt1_to_etc1(d_blocks, n_bytes / 8, static_cast<hipStream_t>(hip_stream)), "launch transcode");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

// EXTENSION (include/ic_amd.h): DXT5 -> ETC2 RGBA8, 16-byte blocks in place
int icamd_transcode_dxt5_to_etc2_rgba8_device(void *d_blocks, size_t n_bytes, void *hip_stream) try {
  if (!d_blocks) return ICAMD_FALSE;
  if (reinterpret_cast<uintptr_t>(d_blocks) % 16u) return fail(ICAMD_ERR_ARG, "block pointer must be 16-byte aligned");
  if (n_bytes < 16) return ICAMD_OK;
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  ICAMD_HIP(icamd::launch_transcode_dxt5_to_etc2_rgba8(d_blocks, n_bytes / 16, static_cast<hipStream_t>(hip_stream)),
            "launch transcode dxt5 -> etc2 rgba8");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

// EXTENSIONS (include/ic_amd.h): DXT1 -> ETC2 RGB8, BC4 -> EAC R11 (8-byte blocks), BC5 -> EAC RG11 (16-byte blocks) in place
using TranscodeLauncher = hipError_t (*)(void *, uint64_t, hipStream_t);
static int transcode_family_device(TranscodeLauncher launch, const char *what, size_t block, void *d_blocks, size_t n_bytes,
                                   void *hip_stream) {
  if (!d_blocks) return ICAMD_FALSE;
  if (reinterpret_cast<uintptr_t>(d_blocks) % block)
    return fail(ICAMD_ERR_ARG, block == 16 ? "block pointer must be 16-byte aligned" : "block pointer must be 8-byte aligned");
  if (n_bytes < block) return ICAMD_OK;
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  ICAMD_HIP(launch(d_blocks, n_bytes / block, static_cast<hipStream_t>(hip_stream)), what);
  return ICAMD_OK;
}
int icamd_transcode_dxt1_to_etc2_rgb8_device(void *d_blocks, size_t n_bytes, void *hip_stream) try {
  return transcode_family_device(icamd::launch_transcode_dxt1_to_etc2_rgb8, "launch transcode dxt1 -> etc2 rgb8", 8, d_blocks,
                                 n_bytes, hip_stream);
} ICAMD_ABI_CATCH
int icamd_transcode_bc4_to_eac_r11_device(void *d_blocks, size_t n_bytes, void *hip_stream) try {
  return transcode_family_device(icamd::launch_transcode_bc4_to_eac_r11, "launch transcode bc4 -> eac r11", 8, d_blocks, n_bytes,
                                 hip_stream);
} ICAMD_ABI_CATCH
int icamd_transcode_bc5_to_eac_rg11_device(void *d_blocks, size_t n_bytes, void *hip_stream) try {
  return transcode_family_device(icamd::launch_transcode_bc5_to_eac_rg11, "launch transcode bc5 -> eac rg11", 16, d_blocks,
                                 n_bytes, hip_stream);
} ICAMD_ABI_CATCH

int icamd_pad(int compressor, int etc_strategy, int format, uint32_t ch, uint32_t cw, const uint8_t *blocks,
              uint32_t ph, uint32_t pw, uint8_t *out, size_t out_size) try {
  int codec;
  if (!blocks || !out || !resolve_codec(compressor, format, &codec)) return ICAMD_FALSE;
  if (!pad_geometry_ok(codec, ch, cw, ph, pw, out_size)) return ICAMD_FALSE;  // (an empty image is refused by the device entry)
  return staged_blockop(tls_staging(), blocks, icamd_encoded_size(codec, ch, cw), out, out_size, out_size, false,
                        [&](void *din, void *dout, hipStream_t s) {
                          return icamd_pad_device(compressor, etc_strategy, format, ch, cw, din, ph, pw, dout, out_size, s);
                        });
} ICAMD_ABI_CATCH

int icamd_downsample(int compressor, int etc_strategy, int format, uint32_t uh, uint32_t uw, const uint8_t *blocks,
                     uint8_t *out, size_t out_size) try {
  int codec;
  if (!blocks || !out || uh == 0 || uw == 0 || !resolve_codec(compressor, format, &codec)) return ICAMD_FALSE;
  if (!downsample_geometry_ok(codec, uh, uw, out_size)) return ICAMD_FALSE;
  return staged_blockop(tls_staging(), blocks, icamd_encoded_size(codec, uh, uw), out, out_size, out_size, false,
                        [&](void *din, void *dout, hipStream_t s) {
                          return icamd_downsample_device(compressor, etc_strategy, format, uh, uw, din, dout, out_size, s);
                        });
} ICAMD_ABI_CATCH

int icamd_transcode_dxt1_to_etc1(uint8_t *blocks, size_t n_bytes) try {
  if (!blocks) return ICAMD_FALSE;
  if (n_bytes < 8) return ICAMD_OK;
  const size_t whole = n_bytes - n_bytes % 8;
  return staged_blockop(tls_staging(), blocks, n_bytes, blocks, whole, whole, true, [&](void *din, void *, hipStream_t s) {
    return icamd_transcode_dxt1_to_etc1_device(din, n_bytes, s);
  });
} ICAMD_ABI_CATCH

int icamd_transcode_dxt5_to_etc2_rgba8(uint8_t *blocks, size_t n_bytes) try {
  if (!blocks) return ICAMD_FALSE;
  if (n_bytes < 16) return ICAMD_OK;
  const size_t whole = n_bytes - n_bytes % 16;
  return staged_blockop(tls_staging(), blocks, n_bytes, blocks, whole, whole, true, [&](void *din, void *, hipStream_t s) {
    return icamd_transcode_dxt5_to_etc2_rgba8_device(din, n_bytes, s);
  });
} ICAMD_ABI_CATCH

// the host forms of the ETC2-family transcodes: staged through the device like the two above
using TranscodeDeviceFn = int (*)(void *, size_t, void *);
static int transcode_family_host(TranscodeDeviceFn device_form, size_t block, uint8_t *blocks, size_t n_bytes) {
  if (!blocks) return ICAMD_FALSE;
  if (n_bytes < block) return ICAMD_OK;
  const size_t whole = n_bytes - n_bytes % block;
  return staged_blockop(tls_staging(), blocks, n_bytes, blocks, whole, whole, true,
                        [&](void *din, void *, hipStream_t s) { return device_form(din, n_bytes, s); });
}
int icamd_transcode_dxt1_to_etc2_rgb8(uint8_t *blocks, size_t n_bytes) try {
  return transcode_family_host(icamd_transcode_dxt1_to_etc2_rgb8_device, 8, blocks, n_bytes);
} ICAMD_ABI_CATCH
int icamd_transcode_bc4_to_eac_r11(uint8_t *blocks, size_t n_bytes) try {
  return transcode_family_host(icamd_transcode_bc4_to_eac_r11_device, 8, blocks, n_bytes);
} ICAMD_ABI_CATCH
int icamd_transcode_bc5_to_eac_rg11(uint8_t *blocks, size_t n_bytes) try {
  return transcode_family_host(icamd_transcode_bc5_to_eac_rg11_device, 16, blocks, n_bytes);
} ICAMD_ABI_CATCH

int icamd_compress_batch(int compressor, int etc_strategy, int format, uint32_t height, uint32_t width,
                         uint32_t padding_bytes_per_row, uint32_t n_images, const uint8_t *const *buffers,
                         uint8_t *const *outs, size_t out_size, const int *devices, int n_devices, int *statuses) try {
  if (n_images == 0) return ICAMD_OK;
  if (!buffers || !outs || !devices || n_devices <= 0) return fail(ICAMD_ERR_ARG, "icamd_compress_batch: null list");
  if (n_devices > kMaxDeviceListEntries) return fail(ICAMD_ERR_ARG, "icamd_compress_batch: device list longer than 256 entries");
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  int visible = 0;
  rc = check_device_list("icamd_compress_batch", devices, n_devices, &visible);
  if (rc != ICAMD_OK) return rc;
  return run_workers("icamd_compress_batch", n_devices, n_images, statuses,
                     [&](int d, std::vector<int> &local, WorkerError &error) {
    auto fail_all = [&](int code, const char *what) {
      for (uint64_t i = (uint64_t)d; i < n_images; i += (uint64_t)n_devices) local[i] = code;
      if (error.empty()) error.set(what);
    };
    uint64_t reached = (uint64_t)d;  // the image being worked on: what an exception leaves undone starts here
    try {
      // each worker owns its device context and a pooled Staging (streams, device buffers)
      if (hipSetDevice(devices[d]) != hipSuccess) return fail_all(ICAMD_ERR_HIP, "hipSetDevice failed");
      std::unique_ptr<Staging> st = pool_take(devices[d]);
      for (; reached < n_images; reached += (uint64_t)n_devices) {
        const uint32_t i = (uint32_t)reached;
        local[i] = compress_host_common(*st, false, compressor, etc_strategy, format, height, width, height, width,
                                        padding_bytes_per_row, buffers[i], outs[i], out_size);
        if (local[i] < 0 && error.empty()) error.set(g_last_error);
      }
      pool_give(std::move(st));
    } catch (...) {
      const int code = abi_exception();
      for (uint64_t i = reached; i < n_images; i += (uint64_t)n_devices) local[i] = code;
      if (error.empty()) error.set(g_last_error);
    }
  });
} ICAMD_ABI_CATCH

// ---- CreateSolidImage / CopySubimage

namespace {
// Quantize8<n> (color_util.h:156-164)
uint32_t quantize8(uint32_t v, uint32_t bits) {
  const uint32_t i = v * ((1u << bits) - 1u) + 128u;
  return (i + (i >> 8)) >> 8;
}
// The one block CreateSolidImage replicates, as little-endian dwords; returns its size in bytes, 0 where the reference
// returns false.  DXT (dxtc_compressor.cc:42-49,77-82,820-839): c0 = c1 = RGB565(color) -- no red/blue swap --, index
// bits zero; DXT5 puts alpha0 = alpha1 = color[3] and zero codes in front.  ETC (etc_compressor.cc:595-617,802-812):
// differential mode, 5-bit base = color >> 3 (the "adjusted" colour computed there is never used), zero difference,
// codeword 0 twice, all indices 0; big-endian high word, then the zero low word.
uint32_t solid_block(int compressor, int format, const uint8_t *color, uint32_t w[4]) {
  w[0] = w[1] = w[2] = w[3] = 0;
  const int comps = format_components(format);
  if (comps == 0 || !color) return 0;
  if (compressor == ICAMD_COMPRESSOR_ETC) {
    if (format != ICAMD_RGB) return 0;
    const uint32_t hi = 2u | (uint32_t)(color[0] >> 3) << 27 | (uint32_t)(color[1] >> 3) << 19 | (uint32_t)(color[2] >> 3) << 11;
    w[0] = __builtin_bswap32(hi);
    return 8;
  }
  if (compressor != ICAMD_COMPRESSOR_DXTC) return 0;  // pvrtc_compressor.cc:693-698
  const uint32_t c565 = quantize8(color[0], 5) << 11 | quantize8(color[1], 6) << 5 | quantize8(color[2], 5);
  if (comps == 3) {
    w[0] = c565 | c565 << 16;
    return 8;
  }
  w[0] = (uint32_t)color[3] | (uint32_t)color[3] << 8;
  w[2] = c565 | c565 << 16;
  return 16;
}
// CopySubimage's argument check (helper.h:555-563) and geometry
bool subimage_geometry(int compressor, int format, uint32_t ch, uint32_t cw, uint32_t row, uint32_t col, uint32_t h,
                       uint32_t w, int *block_bytes) {
  int codec;
  if (!resolve_codec(compressor, format, &codec)) return false;
  *block_bytes = (int)icamd::codec_block_bytes(codec);
  if (row % 4 || col % 4 || h % 4 || w % 4) return false;
  // 64-bit sums: the reference's uint32 start + extent can wrap and then accept a window outside the image
  return !(row > ch || col > cw || (uint64_t)row + h > ch || (uint64_t)col + w > cw);
}
}  // namespace

int icamd_create_solid_batch_device(int compressor, int format, uint32_t height, uint32_t width, uint32_t n_images,
                                    const uint8_t *colors, void *d_out, size_t dst_image_stride_bytes, size_t out_size_per_image,
                                    void *hip_stream) try {
  const int comps = format_components(format);
  uint32_t probe[4];
  if (!colors || !d_out || comps == 0) return ICAMD_FALSE;
  const uint32_t bb = solid_block(compressor, format, colors, probe);
  if (bb == 0) return ICAMD_FALSE;
  const uint64_t n = (uint64_t)num_blocks4(height) * num_blocks4(width);
  if (out_size_per_image != n * bb) return ICAMD_FALSE;  // compressor4x4_helper.cc:34-41
  if ((reinterpret_cast<uintptr_t>(d_out) | dst_image_stride_bytes) % 4u) return fail(ICAMD_ERR_ARG, "block pointers and image strides must be 4-byte aligned");
  if ((n_images > 1 || dst_image_stride_bytes != 0) && dst_image_stride_bytes < out_size_per_image)
    return fail(ICAMD_ERR_ARG, "image stride smaller than an image");
  if (n >= (1ull << 32)) return fail(ICAMD_ERR_ARG, "more than 2^32 blocks in one image");
  if (n_images == 0) return ICAMD_OK;
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  std::vector<uint32_t> words((size_t)n_images * 4u);
  for (uint32_t i = 0; i < n_images; ++i) (void)solid_block(compressor, format, colors + (size_t)i * (size_t)comps, &words[(size_t)i * 4u]);
  ICAMD_HIP(icamd::launch_fill_blocks_batch(d_out, dst_image_stride_bytes, (uint32_t)n, (int)bb,
                                            reinterpret_cast<const uint32_t (*)[4]>(words.data()), n_images,
                                            static_cast<hipStream_t>(hip_stream)), "launch fill");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

int icamd_create_solid_device(int compressor, int format, uint32_t height, uint32_t width, const uint8_t *color,
                              void *d_out, size_t out_size, void *hip_stream) try {
  uint32_t w[4];
  const uint32_t bb = solid_block(compressor, format, color, w);
  if (bb == 0 || !d_out) return ICAMD_FALSE;
  const uint64_t n = (uint64_t)num_blocks4(height) * num_blocks4(width);
  if (out_size != n * bb) return ICAMD_FALSE;  // compressor4x4_helper.cc:34-41
  if (reinterpret_cast<uintptr_t>(d_out) % 4u) return fail(ICAMD_ERR_ARG, "block pointers must be 4-byte aligned");
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  ICAMD_HIP(icamd::launch_fill_blocks(d_out, n, (int)bb, w, static_cast<hipStream_t>(hip_stream)), "launch fill");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

// Host buffers in, host buffers out: replicating one block is byte shuffling with nothing to offload (a PCIe round
// trip would be pure overhead), exactly what the reference does (helper.h:536-540).
int icamd_create_solid(int compressor, int format, uint32_t height, uint32_t width, const uint8_t *color, uint8_t *out,
                       size_t out_size) try {
  uint32_t w[4];
  const uint32_t bb = solid_block(compressor, format, color, w);
  if (bb == 0 || !out) return ICAMD_FALSE;
  const uint64_t n = (uint64_t)num_blocks4(height) * num_blocks4(width);
  if (out_size != n * bb) return ICAMD_FALSE;
  for (uint64_t i = 0; i < n; ++i) std::memcpy(out + i * bb, w, bb);
  return ICAMD_OK;
} ICAMD_ABI_CATCH

int icamd_copy_subimage_batch_device(int compressor, int format, uint32_t compressed_height, uint32_t compressed_width,
                                     uint32_t n_images, const void *d_blocks, size_t src_image_stride_bytes, uint32_t start_row,
                                     uint32_t start_column, uint32_t height, uint32_t width, void *d_out,
                                     size_t dst_image_stride_bytes, size_t out_size_per_image, void *hip_stream) try {
  int bb;
  if (!d_blocks || !d_out ||
      !subimage_geometry(compressor, format, compressed_height, compressed_width, start_row, start_column, height, width, &bb))
    return ICAMD_FALSE;
  const uint32_t rows = num_blocks4(height), cols = num_blocks4(width);
  if (out_size_per_image != (size_t)rows * cols * (size_t)bb) return ICAMD_FALSE;
  if ((reinterpret_cast<uintptr_t>(d_blocks) | reinterpret_cast<uintptr_t>(d_out) | src_image_stride_bytes | dst_image_stride_bytes) % 4u)
    return fail(ICAMD_ERR_ARG, "block pointers and image strides must be 4-byte aligned");
  if (((n_images > 1 || src_image_stride_bytes != 0) &&
       src_image_stride_bytes < (size_t)num_blocks4(compressed_height) * num_blocks4(compressed_width) * (size_t)bb) ||
      ((n_images > 1 || dst_image_stride_bytes != 0) && dst_image_stride_bytes < out_size_per_image))
    return fail(ICAMD_ERR_ARG, "image stride smaller than an image");
  if (n_images == 0) return ICAMD_OK;
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  ICAMD_HIP(icamd::launch_copy_subimage(bb, d_blocks, num_blocks4(compressed_width), start_row / 4u, start_column / 4u,
                                        rows, cols, d_out, static_cast<hipStream_t>(hip_stream), n_images,
                                        src_image_stride_bytes, dst_image_stride_bytes), "launch copy_subimage");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

int icamd_copy_subimage_device(int compressor, int format, uint32_t compressed_height, uint32_t compressed_width,
                               const void *d_blocks, uint32_t start_row, uint32_t start_column, uint32_t height,
                               uint32_t width, void *d_out, size_t out_size, void *hip_stream) try {
  return icamd_copy_subimage_batch_device(compressor, format, compressed_height, compressed_width, 1, d_blocks, 0, start_row,
                                          start_column, height, width, d_out, 0, out_size, hip_stream);
} ICAMD_ABI_CATCH

// Host form: block-row memcpys like the reference (helper.h:583-589); nothing to offload.
int icamd_copy_subimage(int compressor, int format, uint32_t compressed_height, uint32_t compressed_width,
                        const uint8_t *blocks, uint32_t start_row, uint32_t start_column, uint32_t height,
                        uint32_t width, uint8_t *out, size_t out_size) try {
  int bb;
  if (!blocks || !out ||
      !subimage_geometry(compressor, format, compressed_height, compressed_width, start_row, start_column, height, width, &bb))
    return ICAMD_FALSE;
  const uint32_t rows = num_blocks4(height), cols = num_blocks4(width), src_cols = num_blocks4(compressed_width);
  if (out_size != (size_t)rows * cols * (size_t)bb) return ICAMD_FALSE;
  const uint8_t *src = blocks + ((size_t)(start_row / 4u) * src_cols + start_column / 4u) * (size_t)bb;
  for (uint32_t r = 0; r < rows; ++r)
    std::memcpy(out + (size_t)r * cols * bb, src + (size_t)r * src_cols * bb, (size_t)cols * bb);
  return ICAMD_OK;
} ICAMD_ABI_CATCH

// ---- diagnostics

uint32_t icamd_wall_clock_rate_khz(void) {
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) return 0;
  return (uint32_t)khz;
}

int icamd_clock_probe_device(void *d_out16, uint32_t duration_us, void *hip_stream) try {
  if (!d_out16 || reinterpret_cast<uintptr_t>(d_out16) % 8u) return fail(ICAMD_ERR_ARG, "clock probe: 8-byte aligned 16-byte buffer needed");
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  const uint32_t khz = icamd_wall_clock_rate_khz();
  if (khz == 0) return fail(ICAMD_ERR_HIP, "hipDeviceAttributeWallClockRate unavailable");
  // an exported entry point must not be able to park a wave on the device for an hour (uint32 microseconds = 71 minutes)
  if (duration_us > ICAMD_CLOCK_PROBE_MAX_US) return fail(ICAMD_ERR_ARG, "clock probe: duration above ICAMD_CLOCK_PROBE_MAX_US (10 s)");
  const uint64_t ticks = (uint64_t)duration_us * khz / 1000u;
  ICAMD_HIP(icamd::launch_clock_probe(static_cast<uint64_t *>(d_out16), ticks, static_cast<hipStream_t>(hip_stream)), "launch clock probe");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

// ---- multi-GPU from one process, device-resident

int icamd_encode_batch_sharded_device(int codec, int etc_strategy, int src_components, int swap_rb, uint32_t height,
                                      uint32_t width, uint32_t row_stride_bytes, uint32_t n_images,
                                      const void *const *d_srcs, void *const *d_dsts, const int *devices, int n_devices,
                                      int gather_device, void *d_gathered, size_t gathered_image_stride_bytes,
                                      int *statuses) try {
  if (n_images == 0) return ICAMD_OK;
  if (!d_srcs || !devices || n_devices <= 0) return fail(ICAMD_ERR_ARG, "icamd_encode_batch_sharded_device: null list");
  if (n_devices > kMaxDeviceListEntries) return fail(ICAMD_ERR_ARG, "icamd_encode_batch_sharded_device: device list longer than 256 entries");
  const bool gather = gather_device >= 0;
  if (!gather && !d_dsts) return fail(ICAMD_ERR_ARG, "icamd_encode_batch_sharded_device: no output (d_dsts and no gather)");
  if (gather && !d_gathered) return fail(ICAMD_ERR_ARG, "icamd_encode_batch_sharded_device: gather without a buffer");
  if (height == 0 || width == 0) return ICAMD_FALSE;
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  int visible = 0;
  rc = check_device_list("icamd_encode_batch_sharded_device", devices, n_devices, &visible);
  if (rc != ICAMD_OK) return rc;
  if (gather && gather_device >= visible) return fail(ICAMD_ERR_ARG, "icamd_encode_batch_sharded_device: bad gather device");
  const size_t out_size = icamd_encoded_size(codec, height, width);
  if (gather && gathered_image_stride_bytes < out_size) return fail(ICAMD_ERR_ARG, "gathered image stride smaller than an image");
  int prev_device = 0;
  (void)hipGetDevice(&prev_device);
  rc = run_workers("icamd_encode_batch_sharded_device", n_devices, n_images, statuses,
                   [&](int d, std::vector<int> &local, WorkerError &error) {
    const int dev = devices[d];
    auto fail_all = [&](int code, const char *what) {
      for (uint64_t i = (uint64_t)d; i < n_images; i += (uint64_t)n_devices) local[i] = code;
      error.set(what);
    };
    try {
    if (hipSetDevice(dev) != hipSuccess) return fail_all(ICAMD_ERR_HIP, "hipSetDevice failed");
    if (gather && dev != gather_device) {
      // direct xGMI copies into the gather buffer: without peer access hipMemcpyPeerAsync bounces through host memory.
      // Best effort -- "already enabled" and "not supported" both leave a working (if slower) copy path.
      // (ICAMD_DISABLE_PEER_ACCESS=1: test knob -- take the host-bounced copy path on a box that has peer access)
      int can = 0;
      const char *no_peer = getenv("ICAMD_DISABLE_PEER_ACCESS");
      if (!(no_peer && no_peer[0] == '1') && hipDeviceCanAccessPeer(&can, dev, gather_device) == hipSuccess && can)
        (void)hipDeviceEnablePeerAccess(gather_device, 0);
      (void)hipGetLastError();
    }
    std::unique_ptr<Staging> st = pool_take(dev);
    // this worker's images, in order
    std::vector<uint32_t> mine;
    for (uint64_t i = (uint64_t)d; i < n_images; i += (uint64_t)n_devices) mine.push_back((uint32_t)i);
    auto slot_of = [&](uint32_t i) { return static_cast<uint8_t *>(d_gathered) + (size_t)i * gathered_image_stride_bytes; };
    // where image i is encoded to: its own buffer, its gather slot (images of the gather device), or scratch (nullptr here)
    auto target_of = [&](uint32_t i) -> uint8_t * {
      if (d_dsts && d_dsts[i]) return static_cast<uint8_t *>(d_dsts[i]);
      return (gather && dev == gather_device) ? slot_of(i) : nullptr;
    };
    // Consecutive images of a worker whose sources AND targets are evenly spaced (a batch laid out as one array, the
    // usual case) go out as ONE launch of up to kRun images: a 1024^2 texture alone fills a quarter of the chip's wave
    // slots, so one launch per texture leaves an MI355X mostly idle (bench.py single_image: 97 vs 252 Gpix/s for ETC1).
    const size_t kRun = 64;
    auto run_length = [&](size_t j, size_t *src_stride, size_t *dst_stride) -> size_t {
      const uint32_t i0 = mine[j];
      if (!d_srcs[i0] || j + 1 >= mine.size() || !d_srcs[mine[j + 1]]) return 1;
      const uint8_t *s0 = static_cast<const uint8_t *>(d_srcs[i0]), *s1 = static_cast<const uint8_t *>(d_srcs[mine[j + 1]]);
      uint8_t *t0 = target_of(i0), *t1 = target_of(mine[j + 1]);
      if (s1 <= s0 || (t0 == nullptr) != (t1 == nullptr) || (t0 && t1 <= t0)) return 1;
      const size_t ss = (size_t)(s1 - s0), ds = t0 ? (size_t)(t1 - t0) : out_size;
      if (ds < out_size || ss % 16u || ds % 16u) return 1;  // (PVRTC wants 16-byte strides; harmless for the others)
      size_t len = 2;
      while (len < kRun && j + len < mine.size()) {
        const uint32_t in = mine[j + len];
        const uint8_t *sn = static_cast<const uint8_t *>(d_srcs[in]);
        uint8_t *tn = target_of(in);
        if (!sn || sn != s0 + len * ss || (tn == nullptr) != (t0 == nullptr) || (t0 && tn != t0 + len * ds)) break;
        ++len;
      }
      *src_stride = ss;
      *dst_stride = ds;
      return len;
    };
    // scratch for the images that have no buffer on this device (gather only): two halves, so that the peer copies of
    // one run overlap the encode of the next (two streams, alternating)
    size_t scratch_images = 0;
    for (size_t j = 0; j < mine.size(); ++j)
      if (gather && target_of(mine[j]) == nullptr) scratch_images = std::min(kRun, std::max<size_t>(scratch_images + 1, 1));
    const size_t scratch_bytes = scratch_images ? scratch_images * out_size : 1;
    if (st->ensure(scratch_bytes, scratch_bytes) != ICAMD_OK) {
      pool_give(std::move(st));
      return fail_all(ICAMD_ERR_ALLOC, "staging allocation failed");
    }
    size_t run_no = 0;
    for (size_t j = 0; j < mine.size(); ++run_no) {
      size_t src_stride = 0, dst_stride = 0;
      size_t len = run_length(j, &src_stride, &dst_stride);
      const uint32_t i0 = mine[j];
      hipStream_t s = (run_no & 1u) ? st->stream2 : st->stream;
      uint8_t *scratch = static_cast<uint8_t *>((run_no & 1u) ? st->d_in : st->d_out);
      uint8_t *own = target_of(i0);
      if (!own && gather) len = std::min(len, scratch_images);
      auto set_all = [&](int code) { for (size_t k = 0; k < len; ++k) local[mine[j + k]] = code; };
      if (!d_srcs[i0]) { local[i0] = ICAMD_FALSE; j += 1; continue; }
      if (!own && !gather) {  // nowhere to put this image's blocks
        local[i0] = ICAMD_ERR_ARG;
        if (error.empty()) error.set("icamd_encode_batch_sharded_device: image without an output buffer");
        j += 1;
        continue;
      }
      uint8_t *target = own ? own : scratch;
      if (codec == ICAMD_PVRTC2) icamd::pvrtc2_select_workspace((int)(run_no & 1u));  // one scratch buffer per stream
      const int rc_run = icamd_encode_device(codec, etc_strategy, src_components, swap_rb, height, width, height, width,
                                             row_stride_bytes, (uint32_t)len, len > 1 ? src_stride : 0,
                                             len > 1 ? (own ? dst_stride : out_size) : 0, d_srcs[i0], target, s);
      set_all(rc_run);
      if (rc_run == ICAMD_OK && gather) {
        for (size_t k = 0; k < len; ++k) {
          const uint32_t i = mine[j + k];
          uint8_t *from = own ? own + k * dst_stride : scratch + k * out_size;
          if (from == slot_of(i)) continue;  // encoded straight into its slot
          // the encoded image travels device -> device (xGMI between GPUs); no host staging
          const hipError_t e = dev == gather_device ? hipMemcpyAsync(slot_of(i), from, out_size, hipMemcpyDeviceToDevice, s)
                                                    : hipMemcpyPeerAsync(slot_of(i), gather_device, from, dev, out_size, s);
          if (e != hipSuccess) local[i] = fail(ICAMD_ERR_HIP, "gather copy", e);
        }
      }
      for (size_t k = 0; k < len; ++k)
        if (local[mine[j + k]] < 0 && error.empty()) error.set(g_last_error);
      j += len;
    }
    icamd::pvrtc2_select_workspace(0);
    const hipError_t e1 = hipStreamSynchronize(st->stream), e2 = hipStreamSynchronize(st->stream2);
    if (e1 != hipSuccess || e2 != hipSuccess) fail_all(ICAMD_ERR_HIP, "stream synchronize failed");
    pool_give(std::move(st));
    } catch (...) {
      // what was enqueued may still be running on the worker's streams: this device's images all count as failed
      const int code = abi_exception();
      fail_all(code, g_last_error);
      (void)hipDeviceSynchronize();
    }
  });
  (void)hipSetDevice(prev_device);
  return rc;
} ICAMD_ABI_CATCH

// ---- container framing (extension; csrc/containers.h) ----
size_t icamd_container_size(int container, int codec, uint32_t height, uint32_t width, uint32_t levels) {
  using namespace icamd;
  if (!container_supports(container, codec) || height == 0 || width == 0 || levels == 0 || levels > 32) return 0;
  if (container == ICAMD_CONTAINER_PKM && (levels != 1 || height > 65532u || width > 65532u)) return 0;
  if (codec == ICAMD_PVRTC2 && (height != width || !is_pow2(width))) return 0;
  size_t total = container_header_size(container, codec);
  for (uint32_t l = 0; l < levels; ++l) {
    if (l > 0 && (height >> l) == 0 && (width >> l) == 0) return 0;  // past the 1 x 1 level
    const size_t b = container_level_bytes(codec, height, width, l);
    if (b == 0 || b > 0xffffffffull) return 0;
    total += container_level_prefix(container) + b;
  }
  return total;
}

int icamd_container_write(int container, int codec, uint32_t height, uint32_t width, uint32_t levels,
                          const uint8_t *const *level_data, const size_t *level_sizes, uint8_t *out, size_t out_size) try {
  using namespace icamd;
  if (container < ICAMD_CONTAINER_DDS || container > ICAMD_CONTAINER_PVR) return fail(ICAMD_ERR_ARG, "unknown container");
  if (codec < ICAMD_DXT1 || (codec > ICAMD_PVRTC2 && !plane_codec(codec) && codec != ICAMD_ETC2_RGBA8 && codec != ICAMD_ETC2_RGB8 &&
                             codec != ICAMD_ETC2_RGB8A1 && codec != ICAMD_EAC_SIGNED_R11 && codec != ICAMD_EAC_SIGNED_RG11 &&
                             codec != ICAMD_BC7 && codec != ICAMD_BC6H_UF16 && codec != ICAMD_BC6H_SF16 && !bc1a_bc2_codec(codec)))
    return fail(ICAMD_ERR_ARG, "unknown codec");  // (PVRTC4 has no container code)
  if (!level_data || !level_sizes || !out) return ICAMD_FALSE;
  const size_t need = icamd_container_size(container, codec, height, width, levels);
  if (need == 0 || out_size != need) return ICAMD_FALSE;
  for (uint32_t l = 0; l < levels; ++l)
    if (!level_data[l] || level_sizes[l] != container_level_bytes(codec, height, width, l)) return ICAMD_FALSE;
  container_write_header(container, codec, height, width, levels, level_sizes[0], out);
  uint8_t *p = out + container_header_size(container, codec);
  for (uint32_t l = 0; l < levels; ++l) {
    if (container_level_prefix(container)) {
      put_le32(p, (uint32_t)level_sizes[l]);  // KTX imageSize; block streams are multiples of 8 bytes: no mip padding
      p += 4;
    }
    std::memcpy(p, level_data[l], level_sizes[l]);
    p += level_sizes[l];
  }
  return ICAMD_OK;
} ICAMD_ABI_CATCH


// ---- mip chains (EXTENSION) ----
uint32_t icamd_mip_max_levels(uint32_t height, uint32_t width) { return mip_max_levels(height, width); }

size_t icamd_mip_chain_size(int codec, uint32_t height, uint32_t width, uint32_t levels, size_t *level_offsets) {
  return icamd::mip_chain_bytes(codec, height, width, levels, level_offsets);
}

size_t icamd_mip_workspace_size(int codec, int src_components, uint32_t height, uint32_t width, uint32_t levels,
                                uint32_t n_images) {
  if (!mip_codec(codec)) return 0;
  return icamd::mip_chain_plan({ codec, src_components, ICAMD_MIP_FILTER_BOX, height, width, levels, n_images, 0, 0, 0 }).workspace_bytes;
}

// icamd_encode_mips_device / icamd_encode_mips_filtered_device (the former is filter 0)
static int encode_mips(int codec, int etc_strategy, int src_components, int swap_rb, int filter, uint32_t height, uint32_t width,
                       uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images, size_t src_image_stride_bytes,
                       size_t dst_image_stride_bytes, const void *d_src, void *d_dst, void *d_workspace,
                       size_t workspace_bytes, void *hip_stream) {
  if (filter == ICAMD_MIP_FILTER_NORMAL && codec != ICAMD_BC5) return mip_check_filter(codec, src_components, filter);
  if (codec == ICAMD_PVRTC2 || codec == ICAMD_PVRTC4)
    return fail(ICAMD_ERR_ARG, "PVRTC has no fused mip chain: icamd_mip_pyramid_device, then icamd_encode_device per level");
  if (codec == ICAMD_ETC2_RGBA8 || codec == ICAMD_ETC2_RGB8 || codec == ICAMD_ETC2_RGB8A1 || eac11_codec(codec))  // (EAC R11 / RG11: of the ETC2 family)
    return fail(ICAMD_ERR_ARG, "ETC2 has no fused mip chain: icamd_mip_pyramid_device, then icamd_encode_device per level");
  if (!mip_codec(codec)) return fail(ICAMD_ERR_ARG, "unknown codec");
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  int rc = mip_check_components(codec, src_components, swap_rb);
  if (rc != ICAMD_OK) return rc;
  rc = mip_check_filter(codec, src_components, filter);
  if (rc != ICAMD_OK) return rc;
  rc = mip_check_geometry(codec, src_components, height, width, row_stride_bytes, levels, n_images, src_image_stride_bytes,
                          dst_image_stride_bytes);
  if (rc != ICAMD_OK) return rc;
  const icamd::MipChainPlan plan = icamd::mip_chain_plan({ codec, src_components, filter, height, width, levels, n_images,
                                                           row_stride_bytes, src_image_stride_bytes, dst_image_stride_bytes });
  if (plan.workspace_bytes && (!d_workspace || workspace_bytes < plan.workspace_bytes))
    return fail(ICAMD_ERR_ARG, "workspace smaller than icamd_mip_workspace_size");
  if (n_images == 0) return ICAMD_OK;
  rc = require_device();
  if (rc != ICAMD_OK) return rc;
  if (plan.form != icamd::kMipLaunch) return fail(ICAMD_ERR_ARG, "mip chain: no kernel for this codec, source layout and filter");
  const icamd::MipBuffers buffers = { static_cast<const uint8_t *>(d_src), static_cast<uint8_t *>(d_workspace), static_cast<uint8_t *>(d_dst) };
  // ETC1 (the plan has encode calls): level 0 from the source, the pixel pyramid into the workspace, then every other level from
  // it, each through the ETC1 kernels of icamd_encode_device (a fused ETC1 kernel is deferred)
  const bool etc1 = plan.n_encodes != 0;
  const auto encode_level = [&](const icamd::MipEncodeCall &e) {
    const uint8_t *in = (e.in.base == icamd::kMipSource ? buffers.src : buffers.workspace) + e.in.offset;
    return icamd_encode_device(codec, etc_strategy, src_components, swap_rb, e.height, e.width, e.height, e.width, e.in_row_stride,
                               n_images, e.in_image_stride, dst_image_stride_bytes, in, buffers.out + e.out_offset, hip_stream);
  };
  if (etc1 && (rc = encode_level(plan.encode[0])) != ICAMD_OK) return rc;
  for (uint32_t k = 0; k < plan.n_passes; ++k)
    ICAMD_HIP(icamd::launch_mip_pass(etc1 ? icamd::kMipPyramidMode : codec, src_components, filter, plan.pass[k], buffers,
                                     !etc1 && swap_rb, static_cast<hipStream_t>(hip_stream)), "launch mip chain");
  for (uint32_t l = 1; l < plan.n_encodes; ++l)
    if ((rc = encode_level(plan.encode[l])) != ICAMD_OK) return rc;
  return ICAMD_OK;
}

int icamd_encode_mips_device(int codec, int etc_strategy, int src_components, int swap_rb, uint32_t height, uint32_t width,
                             uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images, size_t src_image_stride_bytes,
                             size_t dst_image_stride_bytes, const void *d_src, void *d_dst, void *d_workspace,
                             size_t workspace_bytes, void *hip_stream) try {
  return encode_mips(codec, etc_strategy, src_components, swap_rb, ICAMD_MIP_FILTER_BOX, height, width, row_stride_bytes, levels,
                     n_images, src_image_stride_bytes, dst_image_stride_bytes, d_src, d_dst, d_workspace, workspace_bytes, hip_stream);
} ICAMD_ABI_CATCH

int icamd_encode_mips_filtered_device(int codec, int etc_strategy, int src_components, int swap_rb, int filter, uint32_t height,
                                      uint32_t width, uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images,
                                      size_t src_image_stride_bytes, size_t dst_image_stride_bytes, const void *d_src,
                                      void *d_dst, void *d_workspace, size_t workspace_bytes, void *hip_stream) try {
  return encode_mips(codec, etc_strategy, src_components, swap_rb, filter, height, width, row_stride_bytes, levels, n_images,
                     src_image_stride_bytes, dst_image_stride_bytes, d_src, d_dst, d_workspace, workspace_bytes, hip_stream);
} ICAMD_ABI_CATCH

// ---- mip chains of the ETC2 family (EXTENSION): the plan is etc2_mip_plan.h's; here are the argument checks ----
// the order of the levels inside the encode launch's grid.x (icamd_etc2_mip_tune: time, never bytes)
static std::atomic<int> g_etc2_mip_order{icamd::kEtc2MipLargestFirst};  // (measured: DESIGN.md 3.18)
int icamd_etc2_mip_tune(int level_order) try {
  if (level_order != icamd::kEtc2MipSmallestFirst && level_order != icamd::kEtc2MipLargestFirst)
    return fail(ICAMD_ERR_ARG, "icamd_etc2_mip_tune: level_order must be 0 (smallest level first) or 1 (largest first, the default)");
  g_etc2_mip_order.store(level_order);
  return ICAMD_OK;
} ICAMD_ABI_CATCH

size_t icamd_etc2_mip_chain_size(int codec, uint32_t height, uint32_t width, uint32_t levels, size_t *level_offsets) {
  return icamd::etc2_mip_chain_bytes(codec, height, width, levels, level_offsets);
}

size_t icamd_etc2_mip_workspace_size(int codec, int src_components, uint32_t height, uint32_t width, uint32_t levels,
                                     uint32_t n_images) {
  if (!icamd::etc2_mip_codec(codec) || !codec_accepts_components(codec, src_components)) return 0;
  return icamd::etc2_mip_plan({ codec, src_components, ICAMD_MIP_FILTER_BOX, ICAMD_ETC2_MODES_DEFAULT, height, width, levels, n_images,
                                0, 0, 0, icamd::kEtc2MipSmallestFirst }).workspace_bytes;
}

// The filter rules of icamd_encode_etc2_mips_device: the colour filters for the three colour codecs, the normal-map filter for
// EAC RG11 from RG8 (the one layout the filtered pixel pyramid covers), the box for everything.
static int etc2_mip_check_filter(int codec, int comps, int filter) {
  if (filter == ICAMD_MIP_FILTER_BOX) return ICAMD_OK;
  if (filter == ICAMD_MIP_FILTER_NORMAL)
    return codec == ICAMD_EAC_RG11 && comps == 2
               ? ICAMD_OK
               : fail(ICAMD_ERR_ARG, "ICAMD_MIP_FILTER_NORMAL applies to ICAMD_EAC_RG11 chains from a 2-component (RG) source only");
  if (filter < 0 || filter > (ICAMD_MIP_FILTER_SRGB | ICAMD_MIP_FILTER_ALPHA_WEIGHTED))
    return fail(ICAMD_ERR_ARG, "mip filter must be a combination of ICAMD_MIP_FILTER_SRGB and ICAMD_MIP_FILTER_ALPHA_WEIGHTED, "
                               "or ICAMD_MIP_FILTER_NORMAL alone");
  if (eac11_codec(codec)) return fail(ICAMD_ERR_ARG, "EAC R11 / RG11 hold data channels: ICAMD_MIP_FILTER_BOX, or NORMAL for RG11 from RG8");
  if ((filter & ICAMD_MIP_FILTER_ALPHA_WEIGHTED) && comps != 4)
    return fail(ICAMD_ERR_ARG, "ICAMD_MIP_FILTER_ALPHA_WEIGHTED needs a 4-component source");
  return ICAMD_OK;
}

int icamd_encode_etc2_mips_device(int codec, int etc_strategy, int etc2_modes, int src_components, int swap_rb, int filter,
                                  uint32_t height, uint32_t width, uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images,
                                  size_t src_image_stride_bytes, size_t dst_image_stride_bytes, const void *d_src, void *d_dst,
                                  void *d_workspace, size_t workspace_bytes, void *hip_stream) try {
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  if (!icamd::etc2_mip_codec(codec))
    return fail(ICAMD_ERR_ARG, "icamd_encode_etc2_mips_device encodes ETC2 RGBA8 / RGB8 / RGB8A1 and EAC R11 / RG11 only");
  if (etc2_modes != ICAMD_ETC2_MODES_DEFAULT && !(etc2_modes == ICAMD_ETC2_MODES_TH && codec == ICAMD_ETC2_RGB8))
    return fail(ICAMD_ERR_ARG, "etc2_modes must be ICAMD_ETC2_MODES_DEFAULT, or ICAMD_ETC2_MODES_TH with ICAMD_ETC2_RGB8");
  int rc = mip_check_components(codec, src_components, swap_rb);
  if (rc != ICAMD_OK) return rc;
  rc = etc2_mip_check_filter(codec, src_components, filter);
  if (rc != ICAMD_OK) return rc;
  if (levels == 0 || levels > mip_max_levels(height, width))
    return fail(ICAMD_ERR_ARG, "levels must be 1 .. floor(log2(max(height, width))) + 1");
  if ((uint64_t)row_stride_bytes < (uint64_t)width * (uint32_t)src_components) return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  const icamd::Etc2MipPlan plan = icamd::etc2_mip_plan({ codec, src_components, filter, etc2_modes, height, width, levels, n_images,
                                                         row_stride_bytes, src_image_stride_bytes, dst_image_stride_bytes,
                                                         g_etc2_mip_order.load() });
  const size_t src_bytes = (size_t)(height - 1u) * row_stride_bytes + (size_t)width * (uint32_t)src_components;
  if (n_images > 1 && (src_image_stride_bytes < src_bytes || dst_image_stride_bytes < plan.chain_bytes))
    return fail(ICAMD_ERR_ARG, "image stride smaller than an image");
  if (plan.workspace_bytes && (!d_workspace || workspace_bytes < plan.workspace_bytes))
    return fail(ICAMD_ERR_ARG, "workspace smaller than icamd_etc2_mip_workspace_size");
  if (n_images == 0) return ICAMD_OK;
  rc = require_device();
  if (rc != ICAMD_OK) return rc;
  if (plan.form != icamd::kMipLaunch) return fail(ICAMD_ERR_ARG, "ETC2 mip chain: more workgroups than one launch holds");
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const icamd::MipBuffers buffers = { static_cast<const uint8_t *>(d_src), static_cast<uint8_t *>(d_workspace), static_cast<uint8_t *>(d_dst) };
  // the pixel pyramid into the workspace (built unswapped: averaging is per channel), then every level of every image in one
  // launch (per piece of 65 535 images), then -- ICAMD_ETC2_MODES_TH -- the T / H pass over the same grid
  for (uint32_t k = 0; k < plan.pyramid.n_passes; ++k)
    ICAMD_HIP(icamd::launch_mip_pass(icamd::kMipPyramidMode, src_components, filter, plan.pyramid.pass[k], buffers, false, stream),
              "launch mip pyramid");
  ICAMD_HIP(icamd::launch_etc2_mip(codec, src_components, (uint32_t)etc_strategy, false, swap_rb != 0, plan, buffers,
                                   src_image_stride_bytes, dst_image_stride_bytes, stream), "launch etc2 mip chain");
  if (plan.th)
    ICAMD_HIP(icamd::launch_etc2_mip(codec, src_components, (uint32_t)etc_strategy, true, swap_rb != 0, plan, buffers,
                                     src_image_stride_bytes, dst_image_stride_bytes, stream), "launch etc2 mip chain t/h");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

const char *icamd_etc2_mip_kernel_name(int codec, int src_components, int etc_strategy, int etc2_modes) {
  if (etc2_modes != ICAMD_ETC2_MODES_DEFAULT && !(etc2_modes == ICAMD_ETC2_MODES_TH && codec == ICAMD_ETC2_RGB8)) return "";
  return icamd::etc2_mip_kernel_form(codec, src_components, etc_strategy, etc2_modes == ICAMD_ETC2_MODES_TH);
}

// ---- mip chains of BC7 and BC6H (EXTENSION): the plan is bptc_mip_plan.h's; here are the argument checks ----
size_t icamd_bptc_mip_chain_size(int codec, uint32_t height, uint32_t width, uint32_t levels, size_t *level_offsets) {
  return icamd::bptc_mip_chain_bytes(codec, height, width, levels, level_offsets);
}

size_t icamd_bptc_mip_workspace_size(int codec, int src_channels, uint32_t height, uint32_t width, uint32_t levels,
                                     uint32_t n_images) {
  return icamd::bptc_mip_plan({ codec, src_channels, ICAMD_MIP_FILTER_BOX, 0, height, width, levels, n_images, 0, 0, 0 }).workspace_bytes;
}

// What the two entry points share once codec, modes, channels, swap_rb and filter are accepted: the geometry checks in the order
// of icamd_encode_etc2_mips_device, then the pyramid passes and the one encode launch.
static int encode_bptc_mips(int codec, int modes, int chans, int swap_rb, int filter, uint32_t height, uint32_t width,
                            uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images, size_t src_image_stride_bytes,
                            size_t dst_image_stride_bytes, const void *d_src, void *d_dst, void *d_workspace, size_t workspace_bytes,
                            void *hip_stream) {
  const bool halves = codec != ICAMD_BC7;
  const uint32_t pixel_bytes = icamd::bptc_mip_pixel_bytes(codec, chans);
  if (levels == 0 || levels > mip_max_levels(height, width))
    return fail(ICAMD_ERR_ARG, "levels must be 1 .. floor(log2(max(height, width))) + 1");
  if ((uint64_t)row_stride_bytes < (uint64_t)width * pixel_bytes) return fail(ICAMD_ERR_ARG, "row stride smaller than a row");
  const icamd::BptcMipPlan plan = icamd::bptc_mip_plan({ codec, chans, filter, modes, height, width, levels, n_images, row_stride_bytes,
                                                         src_image_stride_bytes, dst_image_stride_bytes });
  const size_t src_bytes = (size_t)(height - 1u) * row_stride_bytes + (size_t)width * pixel_bytes;
  if (n_images > 1 && (src_image_stride_bytes < src_bytes || dst_image_stride_bytes < plan.chain_bytes))
    return fail(ICAMD_ERR_ARG, "image stride smaller than an image");
  if (plan.workspace_bytes && (!d_workspace || workspace_bytes < plan.workspace_bytes))
    return fail(ICAMD_ERR_ARG, "workspace smaller than icamd_bptc_mip_workspace_size");
  if (halves && (reinterpret_cast<uintptr_t>(d_src) % 2u || reinterpret_cast<uintptr_t>(d_workspace) % 2u || row_stride_bytes % 2u ||
                 src_image_stride_bytes % 2u))
    return fail(ICAMD_ERR_ARG, "BC6H: d_src, d_workspace, row_stride_bytes and src_image_stride_bytes must be even");
  if (n_images == 0) return ICAMD_OK;
  int rc = require_device();
  if (rc != ICAMD_OK) return rc;
  if (plan.form != icamd::kMipLaunch) return fail(ICAMD_ERR_ARG, "BC7 / BC6H mip chain: more workgroups than one launch holds");
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const icamd::MipBuffers buffers = { static_cast<const uint8_t *>(d_src), static_cast<uint8_t *>(d_workspace), static_cast<uint8_t *>(d_dst) };
  // the pixel pyramid into the workspace (BC7: built unswapped, averaging is per channel), then every level of every image in
  // one launch (per piece of 65 535 images)
  for (uint32_t k = 0; k < plan.pyramid.n_passes; ++k)
    ICAMD_HIP(halves ? icamd::launch_mip_f16_pass(chans, plan.pyramid.pass[k], buffers, stream)
                     : icamd::launch_mip_pass(icamd::kMipPyramidMode, chans, filter, plan.pyramid.pass[k], buffers, false, stream),
              "launch mip pyramid");
  ICAMD_HIP(icamd::launch_bptc_mip(codec, chans, modes, swap_rb != 0, plan, buffers, src_image_stride_bytes, dst_image_stride_bytes,
                                   stream), "launch bptc mip chain");
  return ICAMD_OK;
}

int icamd_encode_bc7_mips_device(int bc7_modes, int src_components, int swap_rb, int filter, uint32_t height, uint32_t width,
                                 uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images, size_t src_image_stride_bytes,
                                 size_t dst_image_stride_bytes, const void *d_src, void *d_dst, void *d_workspace,
                                 size_t workspace_bytes, void *hip_stream) try {
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  if (bc7_modes != ICAMD_BC7_MODES_DEFAULT && bc7_modes != ICAMD_BC7_MODES_EXTENDED)
    return fail(ICAMD_ERR_ARG, "bc7_modes must be ICAMD_BC7_MODES_DEFAULT or ICAMD_BC7_MODES_EXTENDED");
  if (src_components != 3 && src_components != 4) return fail(ICAMD_ERR_ARG, "src_components must be 3 or 4");
  if (filter < 0 || filter > (ICAMD_MIP_FILTER_SRGB | ICAMD_MIP_FILTER_ALPHA_WEIGHTED))
    return fail(ICAMD_ERR_ARG, "BC7 chains take ICAMD_MIP_FILTER_BOX or a combination of ICAMD_MIP_FILTER_SRGB and "
                               "ICAMD_MIP_FILTER_ALPHA_WEIGHTED");
  if ((filter & ICAMD_MIP_FILTER_ALPHA_WEIGHTED) && src_components != 4)
    return fail(ICAMD_ERR_ARG, "ICAMD_MIP_FILTER_ALPHA_WEIGHTED needs a 4-component source");
  return encode_bptc_mips(ICAMD_BC7, bc7_modes, src_components, swap_rb, filter, height, width,
                          row_stride_bytes, levels, n_images, src_image_stride_bytes, dst_image_stride_bytes, d_src, d_dst, d_workspace,
                          workspace_bytes, hip_stream);
} ICAMD_ABI_CATCH

int icamd_encode_bc6h_mips_device(int codec, int bc6h_modes, int src_channels, uint32_t height, uint32_t width,
                                  uint32_t row_stride_bytes, uint32_t levels, uint32_t n_images, size_t src_image_stride_bytes,
                                  size_t dst_image_stride_bytes, const void *d_src, void *d_dst, void *d_workspace,
                                  size_t workspace_bytes, void *hip_stream) try {
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  if (!bc6h_codec(codec)) return fail(ICAMD_ERR_ARG, "BC6H: the codec must be ICAMD_BC6H_UF16 or ICAMD_BC6H_SF16");
  if (bc6h_modes != ICAMD_BC6H_MODES_DEFAULT && bc6h_modes != ICAMD_BC6H_MODES_EXTENDED)
    return fail(ICAMD_ERR_ARG, "bc6h_modes must be ICAMD_BC6H_MODES_DEFAULT or ICAMD_BC6H_MODES_EXTENDED");
  if (src_channels != 3 && src_channels != 4) return fail(ICAMD_ERR_ARG, "BC6H needs 3 or 4 source channels");
  return encode_bptc_mips(codec, bc6h_modes, src_channels, 0, ICAMD_MIP_FILTER_BOX, height, width,
                          row_stride_bytes, levels, n_images, src_image_stride_bytes, dst_image_stride_bytes, d_src, d_dst, d_workspace,
                          workspace_bytes, hip_stream);
} ICAMD_ABI_CATCH

const char *icamd_bptc_mip_kernel_name(int codec, int src_channels, int modes) {
  return icamd::bptc_mip_kernel_form(codec, src_channels, modes);
}

// The half-float pixel pyramid: the checks of icamd_mip_pyramid_device with 2 * src_channels bytes per pixel, and even addresses.
int icamd_mip_pyramid_f16_device(int src_channels, uint32_t height, uint32_t width, uint32_t row_stride_bytes, uint32_t levels,
                                 uint32_t n_images, size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                                 const void *d_src, void *d_dst, void *hip_stream) try {
  if (src_channels != 3 && src_channels != 4) return fail(ICAMD_ERR_ARG, "src_channels must be 3 or 4");
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  const int pixel_bytes = 2 * src_channels;
  int rc = mip_check_geometry(icamd::kMipPyramidMode, pixel_bytes, height, width, row_stride_bytes, levels, n_images,
                              src_image_stride_bytes, dst_image_stride_bytes);
  if (rc != ICAMD_OK) return rc;
  if (reinterpret_cast<uintptr_t>(d_src) % 2u || reinterpret_cast<uintptr_t>(d_dst) % 2u || row_stride_bytes % 2u ||
      src_image_stride_bytes % 2u || dst_image_stride_bytes % 2u)
    return fail(ICAMD_ERR_ARG, "half-float pyramid: pointers, row_stride_bytes and the image strides must be even");
  if (n_images == 0) return ICAMD_OK;
  rc = require_device();
  if (rc != ICAMD_OK) return rc;
  if (levels == 1) return ICAMD_OK;
  size_t pixel_off[icamd::kMipMaxLevels + 1];
  (void)icamd::mip_pyramid_bytes(height, width, levels, pixel_bytes, pixel_off);
  icamd::MipChainPlan plan = {};
  const icamd::MipChainIn in = { icamd::kMipPyramidMode, pixel_bytes, ICAMD_MIP_FILTER_BOX, height, width, levels, n_images,
                                 row_stride_bytes, src_image_stride_bytes, dst_image_stride_bytes };
  (void)icamd::mip_plan_passes(in, false, icamd::kMipOutput, dst_image_stride_bytes, nullptr, pixel_off, plan);
  const icamd::MipBuffers buffers = { static_cast<const uint8_t *>(d_src), nullptr, static_cast<uint8_t *>(d_dst) };
  for (uint32_t k = 0; k < plan.n_passes; ++k)
    ICAMD_HIP(icamd::launch_mip_f16_pass(src_channels, plan.pass[k], buffers, static_cast<hipStream_t>(hip_stream)),
              "launch half-float mip pyramid");
  return ICAMD_OK;
} ICAMD_ABI_CATCH

const char *icamd_mip_f16_kernel_name(int src_channels) { return icamd::mip_f16_kernel_name(src_channels); }

// icamd_mip_pyramid_device / icamd_mip_pyramid_filtered_device (the former is filter 0)
static int mip_pyramid(int src_components, int filter, uint32_t height, uint32_t width, uint32_t row_stride_bytes, uint32_t levels,
                       uint32_t n_images, size_t src_image_stride_bytes, size_t dst_image_stride_bytes, const void *d_src,
                       void *d_dst, void *hip_stream) {
  if (src_components < 1 || src_components > 4) return fail(ICAMD_ERR_ARG, "src_components must be 1 .. 4");
  if (!d_src || !d_dst || height == 0 || width == 0) return ICAMD_FALSE;
  int rc = mip_check_filter(icamd::kMipPyramidMode, src_components, filter);
  if (rc != ICAMD_OK) return rc;
  rc = mip_check_geometry(icamd::kMipPyramidMode, src_components, height, width, row_stride_bytes, levels, n_images,
                              src_image_stride_bytes, dst_image_stride_bytes);
  if (rc != ICAMD_OK) return rc;
  if (n_images == 0) return ICAMD_OK;
  rc = require_device();
  if (rc != ICAMD_OK) return rc;
  const icamd::MipChainPlan plan = icamd::mip_chain_plan({ icamd::kMipPyramidMode, src_components, filter, height, width, levels, n_images,
                                                           row_stride_bytes, src_image_stride_bytes, dst_image_stride_bytes });
  if (plan.form == icamd::kMipRefused) return fail(ICAMD_ERR_ARG, "mip pyramid: no kernel for this source layout and filter");
  const icamd::MipBuffers buffers = { static_cast<const uint8_t *>(d_src), nullptr, static_cast<uint8_t *>(d_dst) };
  for (uint32_t k = 0; k < plan.n_passes; ++k)
    ICAMD_HIP(icamd::launch_mip_pass(icamd::kMipPyramidMode, src_components, filter, plan.pass[k], buffers, false,
                                     static_cast<hipStream_t>(hip_stream)), "launch mip pyramid");
  return ICAMD_OK;
}

int icamd_mip_pyramid_device(int src_components, uint32_t height, uint32_t width, uint32_t row_stride_bytes, uint32_t levels,
                             uint32_t n_images, size_t src_image_stride_bytes, size_t dst_image_stride_bytes,
                             const void *d_src, void *d_dst, void *hip_stream) try {
  return mip_pyramid(src_components, ICAMD_MIP_FILTER_BOX, height, width, row_stride_bytes, levels, n_images, src_image_stride_bytes,
                     dst_image_stride_bytes, d_src, d_dst, hip_stream);
} ICAMD_ABI_CATCH

int icamd_mip_pyramid_filtered_device(int src_components, int filter, uint32_t height, uint32_t width, uint32_t row_stride_bytes,
                                      uint32_t levels, uint32_t n_images, size_t src_image_stride_bytes,
                                      size_t dst_image_stride_bytes, const void *d_src, void *d_dst, void *hip_stream) try {
  return mip_pyramid(src_components, filter, height, width, row_stride_bytes, levels, n_images, src_image_stride_bytes,
                     dst_image_stride_bytes, d_src, d_dst, hip_stream);
} ICAMD_ABI_CATCH

const char *icamd_mip_kernel_name(int codec, int src_components, int filter) {
  if (filter < 0 || filter > ICAMD_MIP_FILTER_NORMAL) return "";
  const bool pyramid = codec == ICAMD_MIP_PYRAMID || codec == ICAMD_ETC1;  // ETC1 chains: the pyramid kernel, then the ETC1 kernels
  if (!pyramid && !mip_codec(codec)) return "";
  if (codec == ICAMD_ETC1 && src_components != 3 && src_components != 4) return "";
  return icamd::mip_kernel_name(pyramid ? icamd::kMipPyramidMode : codec, src_components, filter);
}

// icamd_compress_mips / icamd_compress_mips_filtered (the former is filter 0)
static int compress_mips(int compressor, int etc_strategy, int format, int filter, uint32_t height, uint32_t width,
                         uint32_t padding_bytes_per_row, uint32_t levels, const uint8_t *buffer, uint8_t *out, size_t out_size) {
  if (compressor == ICAMD_COMPRESSOR_PVRTC)
    return fail(ICAMD_ERR_ARG, "PVRTC has no fused mip chain: icamd_mip_pyramid_device, then icamd_encode_device per level");
  if (!buffer || !out || height == 0 || width == 0) return ICAMD_FALSE;
  int codec = 0, comps = 0;
  bool swap = false;
  if (!resolve_codec(compressor, format, &codec, &comps, &swap)) return ICAMD_FALSE;  // dxtc.cc:735-750, etc.cc:747-758
  const int frc = mip_check_filter(codec, comps, filter);
  if (frc != ICAMD_OK) return frc;
  if (levels == 0 || levels > mip_max_levels(height, width))
    return fail(ICAMD_ERR_ARG, "levels must be 1 .. floor(log2(max(height, width))) + 1");
  if (out_size != icamd_mip_chain_size(codec, height, width, levels, nullptr)) return ICAMD_FALSE;
  const size_t stride = (size_t)width * comps + padding_bytes_per_row;
  if (stride > 0xffffffffull) return fail(ICAMD_ERR_ARG, "row stride does not fit 32 bits");
  const size_t in_bytes = (size_t)(height - 1) * stride + (size_t)width * comps;
  const size_t ws_off = (out_size + 255u) & ~(size_t)255u;
  const size_t ws = icamd_mip_workspace_size(codec, comps, height, width, levels, 1);
  return staged_blockop(tls_staging(), buffer, in_bytes, out, out_size, ws_off + ws, false, [&](void *din, void *dout, hipStream_t s) {
    uint8_t *d_out = static_cast<uint8_t *>(dout);
    return encode_mips(codec, etc_strategy, comps, swap, filter, height, width, (uint32_t)stride, levels, 1, 0, 0, din, d_out,
                       ws ? d_out + ws_off : nullptr, ws, s);
  });
}

int icamd_compress_mips(int compressor, int etc_strategy, int format, uint32_t height, uint32_t width,
                        uint32_t padding_bytes_per_row, uint32_t levels, const uint8_t *buffer, uint8_t *out,
                        size_t out_size) try {
  return compress_mips(compressor, etc_strategy, format, ICAMD_MIP_FILTER_BOX, height, width, padding_bytes_per_row, levels, buffer,
                       out, out_size);
} ICAMD_ABI_CATCH

int icamd_compress_mips_filtered(int compressor, int etc_strategy, int format, int filter, uint32_t height, uint32_t width,
                                 uint32_t padding_bytes_per_row, uint32_t levels, const uint8_t *buffer, uint8_t *out,
                                 size_t out_size) try {
  return compress_mips(compressor, etc_strategy, format, filter, height, width, padding_bytes_per_row, levels, buffer, out, out_size);
} ICAMD_ABI_CATCH

#pragma GCC visibility pop
}  // extern "C"
