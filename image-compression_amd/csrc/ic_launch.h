// ic_launch.h -- host-side launch entry points of the kernel translation units
// (dxt_kernels.hip, etc1_kernels.hip, pvrtc_kernels.hip, decode_kernels.hip, blockops_kernels.hip); called by ic_capi.hip.
// Which kernels a call gets is decided in the host-only plans: pvrtc_plan.h (PVRTC), blockops_plan.h (Pad, Downsample and
// the chunks of CopySubimage, CreateSolid and the transcode), mip_plan.h (the passes, grids and kernels of the mip chains) and
// etc2_mip_plan.h (the level table and grid of the ETC2-family chains' one encode launch, and the encoders' tile shape),
// bptc_mip_plan.h (the same for the BC7 and BC6H chains, with the half-float pyramid's passes),
// dxt_plan.h (the workgroup size of the DXT encoders) and decode_plan.h (the pieces of a decode or metric call, fewer than 2^31
// blocks each); the launchers here run what a plan says.  The raster decoders' cut of a block index (raster_block) and their
// launch (launch_raster_decode) are here, next to DecodeParams; the metric kernels' walk and launch are in metric_walk.inc.
#ifndef ICAMD_IC_LAUNCH_H_
#define ICAMD_IC_LAUNCH_H_

#include <hip/hip_runtime.h>

#include <atomic>

#include "blockops_plan.h"
#include "bptc_mip_plan.h"
#include "etc2_mip_plan.h"
#include "ic_device.h"
#include "mip_plan.h"

namespace icamd {

constexpr int kThreadsPerWorkgroup = 256;  // 4 waves; one 4x4 block per lane

// Compute units of a device (cached per ordinal): launch shapes and time models count the workgroup slots of THIS device -- a
// partitioned MI355X (CPX: 32 CUs per partition) or another part must not be taken for 256 CUs.  A wrong figure
// costs time, never bytes.
inline uint32_t device_compute_units(int dev) {
  static std::atomic<uint32_t> cached[64];
  if (dev >= 0 && dev < 64) {
    const uint32_t c = cached[dev].load();
    if (c) return c;
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    cus = 256;
  }
  if (dev >= 0 && dev < 64) cached[dev].store((uint32_t)cus);
  return (uint32_t)cus;
}

// (the tile shape for a block grid, GridParams::log2_tile_cols and force_gather: tile_log2_cols and encode_tile_shape of
// etc2_mip_plan.h, where the chain plan applies the same rule to every level)
// Launches `kernel` over every tile of every image; images go into grid.z in chunks of at most 65 535, tile rows into
// grid.y in chunks of at most 65 535 (GridParams::tile_row0), so any uint32 geometry the reference accepts runs.
// max_log2_cols < 8 asks for squarer tiles (e.g. 4: 16 x 16 blocks, a wave = 16 x 4 blocks = 64 x 16 pixels):
// worse coalescing, but the lanes of a wave see more homogeneous content, which is what wave-uniform shortcuts need.
template <typename Kernel>
// wave_workgroups: every wave of a tile is launched as its own 64-lane workgroup (grid.x = 4 x column tiles; the kernel
// undoes it: etc1_locate_tile; the wide DXT1 <- RGBA8 kernels, which dxt_plan.h gives this form: locate_tile<true, 1, 64>)
hipError_t launch_tiled(Kernel wide_kernel, Kernel narrow_kernel, GridParams P, hipStream_t stream,
                        uint32_t max_log2_cols = 8, uint32_t wide_rows = 1, bool wave_workgroups = false, uint32_t lanes_per_block = 1) {
  if (P.n_images == 0 || P.block_rows == 0 || P.block_cols == 0) return hipSuccess;
  const TileShape shape = encode_tile_shape(P.block_cols, P.row_stride, max_log2_cols);
  P.log2_tile_cols = shape.log2_tile_cols;
  P.force_gather = shape.force_gather;
  const uint32_t cols = 1u << P.log2_tile_cols, rows = P.log2_tile_cols == 8 ? wide_rows : 256u >> P.log2_tile_cols;
  const uint32_t gx = (uint32_t)(((uint64_t)P.block_cols + cols - 1) / cols);
  const uint32_t gy = (uint32_t)(((uint64_t)P.block_rows + rows - 1) / rows);
  (void)hipGetLastError();  // do not attribute a stale error of another library on this thread to these launches
  for (uint32_t first = 0; first < P.n_images; first += 65535u) {
    const uint32_t count = P.n_images - first < 65535u ? P.n_images - first : 65535u;
    for (uint32_t row0 = 0; row0 < gy; row0 += 65535u) {
      GridParams Q = P;
      Q.src = P.src + (uint64_t)first * P.src_image_stride;
      Q.dst = P.dst + (uint64_t)first * P.dst_image_stride;
      Q.tile_row0 = row0;
      const uint32_t gyc = gy - row0 < 65535u ? gy - row0 : 65535u;
      // (lanes_per_block = 4: the tile's 256 blocks are 16 one-wave workgroups of 16 blocks x 4 lanes, etc1_locate_tile_quad)
      hipLaunchKernelGGL(P.log2_tile_cols == 8 ? wide_kernel : narrow_kernel,
                         dim3(wave_workgroups ? gx * 4u * lanes_per_block : gx, gyc, count),
                         dim3(wave_workgroups ? 64 : kThreadsPerWorkgroup), 0, stream, Q);
    }
  }
  return hipGetLastError();
}

// codec: ICAMD_DXT1 / ICAMD_DXT5; comps: source bytes per pixel (3 or 4; DXT5 requires 4).
hipError_t launch_dxt(int codec, int comps, const GridParams &P, hipStream_t stream);
hipError_t launch_etc1(int comps, const GridParams &P, hipStream_t stream);
// ETC2 RGBA8 (extension, etc2_kernels.hip): RGBA8 sources only; P.etc_strategy picks the colour half's kernel as for ETC1
hipError_t launch_etc2(const GridParams &P, hipStream_t stream);
const char *etc2_kernel_name(int comps);  // "" unless comps == 4
// ETC2 RGB8 (extension, etc2_rgb8_kernels.hip): comps 3 or 4; P.etc_strategy picks the ETC1 candidate's kernel as for ETC1
hipError_t launch_etc2_rgb8(int comps, const GridParams &P, hipStream_t stream);
const char *etc2_rgb8_kernel_name(int comps);  // "" unless comps is 3 or 4
// The T / H pass of ETC2 RGB8 (extension, etc2_th_kernels.hip; icamd_encode_etc2_device with ICAMD_ETC2_MODES_TH): runs on the
// stream AFTER launch_etc2_rgb8 with the same P and replaces the blocks a T or H word renders strictly closer
hipError_t launch_etc2_th(int comps, const GridParams &P, hipStream_t stream);
const char *etc2_th_kernel_name(int comps);  // "" unless comps is 3 or 4
// ETC2 RGB8A1 (extension, etc2_a1_kernels.hip): RGBA8 sources only; P.etc_strategy as for ETC1
hipError_t launch_etc2_a1(const GridParams &P, hipStream_t stream);
const char *etc2_a1_kernel_name(int comps);  // "" unless comps == 4
// The colour-mode passes of ETC2 RGBA8 and ETC2 RGB8A1 (extension, etc2_colour_modes_kernels.hip; icamd_encode_etc2_colour_device):
// run on the stream AFTER launch_etc2 / launch_etc2_a1 with the same P.  codec ICAMD_ETC2_RGBA8 with colour_modes
// ICAMD_ETC2_COLOUR_PLANAR or _PLANAR_TH, or ICAMD_ETC2_RGB8A1 with _PLANAR_TH; the name is "" for every other pair
hipError_t launch_etc2_colour_modes(int codec, int colour_modes, const GridParams &P, hipStream_t stream);
const char *etc2_colour_modes_kernel_name(int codec, int colour_modes);

// PVRTC1 2bpp: square power-of-two RGBA8 images, n_images of them.
struct PvrtcParams {
  const uint8_t *src;
  uint8_t *dst;
  uint64_t src_image_stride, dst_image_stride;
  uint32_t size;      // width == height
  uint32_t log2_size;
  uint32_t n_images;
  // region_blocks != 0: encode only the blocks [region_first, region_first + region_blocks) of ONE image's Z-order
  // output (a power-of-two, aligned range = a rectangle of blocks); dst receives just those 8 * region_blocks bytes
  uint32_t region_first = 0, region_blocks = 0;
  // the library's own host-buffer path: never borrow the caller-owned workspace (icamd_pvrtc2_set_workspace)
  bool internal_workspace = false;
};
hipError_t launch_pvrtc2(const PvrtcParams &P, hipStream_t stream);
// PVRTC1 4 bpp (extension, parity unpinned): same parameters (no regions), 4 x 4-pixel blocks, size * size / 2 bytes per image
hipError_t launch_pvrtc4(const PvrtcParams &P, hipStream_t stream);
size_t pvrtc4_workspace_bytes(uint32_t size, uint32_t n_images);
const char *pvrtc4_kernel_name();
// Scratch the PVRTC encoder needs between its two kernels for n_images size x size textures (8 bytes per block of one
// launch group), and the thread-local caller-owned override of the library's internal scratch buffer.
size_t pvrtc2_workspace_bytes(uint32_t size, uint32_t n_images);
void pvrtc2_set_workspace(void *d_workspace, size_t bytes);
// this thread's library-owned workspace slot (0 / 1) for the PVRTC launches that follow: one per alternating stream
void pvrtc2_select_workspace(int slot);
// which kernels whole-texture PVRTC launches take: mode 0 = automatic, 1 = always morph + encode, 2 = the one-pass kernel
// wherever it is eligible (512^2 ... 4096^2); log2_strip < 0 = automatic strip height of the one-pass kernel
void pvrtc2_tune(int mode, int log2_strip);

struct DecodeParams {
  const uint8_t *blocks;
  uint8_t *pixels;
  uint64_t src_image_stride, dst_image_stride;
  uint32_t height, width, block_rows, block_cols, row_stride;
  uint32_t blocks_per_image, total_blocks, swap_rb;
  FastDiv div_bpi, div_cols;
};
// One launch (a piece of decode_plan.h): n_images images of height x width pixels, block_cols blocks per block row.
inline DecodeParams decode_params(const uint8_t *blocks, uint8_t *pixels, uint64_t src_image_stride, uint64_t dst_image_stride,
                                  uint32_t height, uint32_t width, uint32_t block_cols, uint32_t row_stride, uint32_t n_images,
                                  bool swap_rb) {
  DecodeParams P;
  P.blocks = blocks;
  P.pixels = pixels;
  P.src_image_stride = src_image_stride;
  P.dst_image_stride = dst_image_stride;
  P.height = height;
  P.width = width;
  P.block_rows = (height + 3u) / 4u;
  P.block_cols = block_cols;
  P.row_stride = row_stride;
  P.blocks_per_image = P.block_rows * block_cols;
  P.total_blocks = P.blocks_per_image * n_images;
  P.swap_rb = swap_rb ? 1u : 0u;
  P.div_bpi = make_fastdiv(P.blocks_per_image);
  P.div_cols = make_fastdiv(block_cols);
  return P;
}
// Block k of a launch, in raster order of the images' block grids: image img, block rem of it = (brow, bcol).
struct RasterBlock {
  uint32_t img, rem, brow, bcol;
};
__device__ __forceinline__ RasterBlock raster_block(const DecodeParams &P, uint32_t k) {
  const uint32_t img = fastdiv(k, P.div_bpi);
  const uint32_t rem = k - img * P.blocks_per_image;
  const uint32_t brow = fastdiv(rem, P.div_cols), bcol = rem - brow * P.block_cols;
  return { img, rem, brow, bcol };
}
// One block per lane, 256 a workgroup: the launch of every raster decoder.
template <typename Kernel>
hipError_t launch_raster_decode(Kernel kernel, const DecodeParams &P, hipStream_t stream) {
  if (P.total_blocks == 0) return hipSuccess;
  (void)hipGetLastError();  // a stale error of another library on this thread is not this launch's
  hipLaunchKernelGGL(kernel, dim3((P.total_blocks + kThreadsPerWorkgroup - 1) / kThreadsPerWorkgroup), dim3(kThreadsPerWorkgroup), 0,
                     stream, P);
  return hipGetLastError();
}
hipError_t launch_decode(int codec, const DecodeParams &P, hipStream_t stream);
hipError_t launch_etc2_decode(const DecodeParams &P, hipStream_t stream);  // ETC2 RGBA8 -> RGBA8 rows (etc2_kernels.hip)
hipError_t launch_etc2_rgb8_decode(const DecodeParams &P, hipStream_t stream);  // ETC2 RGB8 -> RGB888 rows (etc2_rgb8_kernels.hip)
hipError_t launch_etc2_a1_decode(const DecodeParams &P, hipStream_t stream);  // ETC2 RGB8A1 -> RGBA8 rows (etc2_a1_kernels.hip)

// Quality metric (metric_kernels.hip): n_images block grids against their source pixels, one launch of fewer than 2^31
// blocks.  block_rows x block_cols are the blocks that cover the IMAGE (blocks of a padded grid beyond it are never visited);
// grid_cols is the pitch of a block row in blocks (block codecs; PVRTC blocks sit in Z order and the grid is the image).
// stats: n_images records of icamd_error_stats (include/ic_amd.h), zeroed before the launch; the kernels add to them.
struct MetricParams {
  const uint8_t *src, *blocks;
  uint8_t *stats;
  uint64_t src_image_stride, blocks_image_stride;
  uint32_t height, width, block_rows, block_cols, grid_cols, row_stride;
  uint32_t blocks_per_image, total_blocks, swap_rb;
  uint32_t force_gather;  // rows too long for 32-bit row offsets: every block gathers with 64-bit addresses
  FastDiv div_bpi, div_cols;
};
// One launch (a piece of decode_plan.h), as decode_params; force_gather is the encoders' rule (encode_tile_shape).
inline MetricParams metric_params(const uint8_t *src, const uint8_t *blocks, uint8_t *stats, uint64_t src_image_stride,
                                  uint64_t blocks_image_stride, uint32_t height, uint32_t width, uint32_t block_cols,
                                  uint32_t grid_cols, uint32_t row_stride, uint32_t n_images, bool swap_rb) {
  MetricParams P;
  P.src = src;
  P.blocks = blocks;
  P.stats = stats;
  P.src_image_stride = src_image_stride;
  P.blocks_image_stride = blocks_image_stride;
  P.height = height;
  P.width = width;
  P.block_rows = (height + 3u) / 4u;
  P.block_cols = block_cols;
  P.grid_cols = grid_cols;
  P.row_stride = row_stride;
  P.blocks_per_image = P.block_rows * block_cols;
  P.total_blocks = P.blocks_per_image * n_images;
  P.swap_rb = swap_rb ? 1u : 0u;
  P.force_gather = encode_tile_shape(block_cols, row_stride, 8u).force_gather;
  P.div_bpi = make_fastdiv(P.blocks_per_image);
  P.div_cols = make_fastdiv(block_cols);
  return P;
}
hipError_t launch_metric(int codec, int comps, const MetricParams &P, hipStream_t stream);
hipError_t launch_metric_clear(void *stats, uint64_t n_images, hipStream_t stream);  // zeroes n_images records (8-byte aligned)
const char *metric_kernel_name(int codec, int comps);

// BC4 / BC5 (extension, bc45_kernels.hip).  Encode: GridParams as for DXT, comps = 1..4 (BC4) / 2..4 (BC5).  Decode: n_images
// block grids of block_rows x block_cols, R8 / RG8 rows of row_stride bytes; log2_tile_cols / tile_row0 are the launcher's.
struct Bc45DecodeParams {
  const uint8_t *blocks;
  uint8_t *pixels;
  uint64_t src_image_stride, dst_image_stride;
  uint32_t height, width, block_rows, block_cols, row_stride;
  uint32_t log2_tile_cols, tile_row0;
};
inline Bc45DecodeParams bc45_decode_params(const uint8_t *blocks, uint8_t *pixels, uint64_t src_image_stride,
                                           uint64_t dst_image_stride, uint32_t height, uint32_t width, uint32_t row_stride) {
  return { blocks, pixels, src_image_stride, dst_image_stride, height, width, (height + 3u) / 4u, (width + 3u) / 4u, row_stride, 0u, 0u };
}
hipError_t launch_bc45_encode(int codec, int comps, const GridParams &P, hipStream_t stream);
hipError_t launch_bc45_decode(int codec, uint32_t n_images, const Bc45DecodeParams &P, hipStream_t stream);
const char *bc45_kernel_name(int codec, int comps);
// EAC R11 / RG11 (extension, eac11_kernels.hip).  Encode: GridParams as for ETC1 (etc_strategy is not read), comps = 1..4 (R11) /
// 2..4 (RG11).  Decode: Bc45DecodeParams and the lane groups of the BC4 / BC5 decoders, R8 / RG8 rows.
hipError_t launch_eac11_encode(int codec, int comps, const GridParams &P, hipStream_t stream);
hipError_t launch_eac11_decode(int codec, uint32_t n_images, const Bc45DecodeParams &P, hipStream_t stream);
const char *eac11_kernel_name(int codec, int comps);  // "" where launch_eac11_encode has no kernel
// 16-bit and signed EAC R11 / RG11 (extension, eac11_16_kernels.hip): codec ICAMD_EAC_R11 / RG11 / SIGNED_R11 / SIGNED_RG11,
// chans = 16-bit samples per source pixel, 1..4 (R11) / 2..4 (RG11).  Encode: GridParams (swap_rb and etc_strategy are not
// read; addresses are 64-bit per lane, so force_gather is not either).  Decode: Bc45DecodeParams, uint16 / int16 rows of
// row_stride bytes.  Metric: MetricParams as launch_metric (swap_rb and force_gather are not read); the records get sse[k] and
// max_abs[k] of the 16-bit values, k = 0 (R) and 1 (G).
hipError_t launch_eac11_16_encode(int codec, int chans, const GridParams &P, hipStream_t stream);
hipError_t launch_eac11_16_decode(int codec, uint32_t n_images, const Bc45DecodeParams &P, hipStream_t stream);
hipError_t launch_eac11_16_metric(int codec, int chans, const MetricParams &P, hipStream_t stream);
const char *eac11_16_kernel_name(int codec, int chans);         // "" where launch_eac11_16_encode has no kernel
const char *eac11_16_metric_kernel_name(int codec, int chans);  // "" where launch_eac11_16_metric has no kernel
// BC7 (extension, bc7_kernels.hip).  Encode (mode 6): GridParams as for DXT5 (etc_strategy is not read), comps 3 or 4.  Decode
// (all eight modes): DecodeParams as launch_decode, RGBA8 rows.  The metric kernels are launch_metric's.
hipError_t launch_bc7_encode(int comps, const GridParams &P, hipStream_t stream);
hipError_t launch_bc7_decode(const DecodeParams &P, hipStream_t stream);
const char *bc7_kernel_name(int comps);  // "" unless comps is 3 or 4
// BC7 with the mode-1 / mode-5 candidates (extension, bc7_modes_kernels.hip; icamd_encode_bc7_device with
// ICAMD_BC7_MODES_EXTENDED): one fused kernel in place of launch_bc7_encode's, the same GridParams.
hipError_t launch_bc7_modes_encode(int comps, const GridParams &P, hipStream_t stream);
const char *bc7_modes_kernel_name(int comps);  // "" unless comps is 3 or 4
// BC1A / BC2 (extensions, bc1a_bc2_kernels.hip): codec ICAMD_BC1A / ICAMD_BC2.  Encode: GridParams as for DXT5 (etc_strategy is
// not read), RGBA8 sources only.  The decode kernels (RGBA8 rows) are launch_decode's, the metric kernels launch_metric's.
hipError_t launch_bc1a_bc2_encode(int codec, const GridParams &P, hipStream_t stream);
const char *bc1a_bc2_kernel_name(int codec, int comps);  // "" unless comps == 4
// BC6H (extension, bc6h_kernels.hip; icamd_encode_bc6h_device): codec ICAMD_BC6H_UF16 / ICAMD_BC6H_SF16, chans = halves per source
// pixel, 3 or 4.  Encode (mode field 00011): GridParams (swap_rb, etc_strategy and force_gather are not read: addresses are 64-bit
// per lane).  Decode (all fourteen modes): DecodeParams as launch_decode (swap_rb is not read), RGBA16F rows.  Metric: MetricParams
// as launch_eac11_16_metric; the records get sse[k] and max_abs[k] of the t-domain values, k = 0, 1, 2 (R, G, B).
hipError_t launch_bc6h_encode(int codec, int chans, const GridParams &P, hipStream_t stream);
hipError_t launch_bc6h_decode(int codec, const DecodeParams &P, hipStream_t stream);
hipError_t launch_bc6h_metric(int codec, int chans, const MetricParams &P, hipStream_t stream);
const char *bc6h_kernel_name(int codec, int chans);         // "" where launch_bc6h_encode has no kernel
const char *bc6h_metric_kernel_name(int codec, int chans);  // "" where launch_bc6h_metric has no kernel
// BC6H with the two-subset candidate (extension, bc6h_modes_kernels.hip; icamd_encode_bc6h_modes_device with
// ICAMD_BC6H_MODES_EXTENDED): one fused kernel in place of launch_bc6h_encode's, the same GridParams.
hipError_t launch_bc6h_modes_encode(int codec, int chans, const GridParams &P, hipStream_t stream);
const char *bc6h_modes_kernel_name(int codec, int chans);  // "" where launch_bc6h_modes_encode has no kernel

// Mip chains (mip_kernels.hip).  One pass: the input level (src, COMPS bytes per pixel, height x width, row_stride) of each of
// n_images images and up to eight local levels j = 0..7 of it (level j = max(1, height >> j) x max(1, width >> j)).  Bit j of
// enc_mask: encode level j's blocks to dst + level_off[j]; bit j of pix_mask (j >= 1): write level j's pixels as tight
// COMPS-byte rows to pix + pix_off[j].  A pass over more than one 128 x 128 tile builds at most local level 6.
struct MipParams {
  const uint8_t *src;
  uint8_t *dst, *pix;
  uint64_t src_image_stride, dst_image_stride, pix_image_stride;
  uint64_t level_off[8], pix_off[8];
  uint32_t height, width, row_stride;
  uint32_t enc_mask, pix_mask;
  uint32_t swap_rb;
  uint32_t tile_row0;  // first tile row of this launch (launch_mip_pass: a piece of the plan's tile rows)
};
// A planned pass (mip_plan.h: which passes a call runs, where each reads and writes and how it is cut into launches is decided
// there) with the kernel of (mode, comps, filter): mode is ICAMD_DXT1 / DXT5 / BC4 / BC5 or kMipPyramidMode (ETC1 chains are the
// pyramid + the ETC1 kernels, mip_plan.h).  hipErrorInvalidValue where the kernel list has no such row.
struct MipBuffers {  // what MipBase names: the caller's source, workspace and output
  const uint8_t *src;
  uint8_t *workspace, *out;
};
hipError_t launch_mip_pass(int mode, int comps, int filter, const MipPassPlan &pass, const MipBuffers &buffers, bool swap_rb,
                           hipStream_t stream);
const char *mip_kernel_name(int mode, int comps, int filter);  // "" where launch_mip_pass has no kernel
// The launches of a planned pass with the kernel given (mip_kernels.hip): what launch_mip_pass and launch_mip_f16_pass share.
hipError_t launch_mip_kernel(void (*kernel)(MipParams), const MipPassPlan &pass, const MipBuffers &buffers, bool swap_rb,
                             hipStream_t stream);
// The half-float pixel pyramid (extension, mip_f16_kernels.hip; icamd_mip_pyramid_f16_device): a pass planned by mip_plan_passes
// with 2 * chans bytes per pixel for the component count, chans = halves per pixel, 3 or 4.  Pixels only: enc_mask is not read.
hipError_t launch_mip_f16_pass(int chans, const MipPassPlan &pass, const MipBuffers &buffers, hipStream_t stream);
const char *mip_f16_kernel_name(int chans);  // "" unless chans is 3 or 4
// Mip chains of the ETC2 family (extension, etc2_mip_kernels.hip): the encode launch of a plan of etc2_mip_plan.h -- every level
// of every image in one launch per piece of grid.y -- or (th) the T / H pass over the same grid, after it on the stream.  The
// pixel pyramid is in the workspace by then (launch_mip_pass on the same stream).  hipErrorInvalidValue where the list has no
// kernel.
hipError_t launch_etc2_mip(int codec, int comps, uint32_t etc_strategy, bool th, bool swap_rb, const Etc2MipPlan &plan,
                           const MipBuffers &buffers, uint64_t src_image_stride, uint64_t dst_image_stride, hipStream_t stream);
// Mip chains of BC7 and BC6H (extension, bptc_mip_kernels.hip): the encode launch of a plan of bptc_mip_plan.h, as
// launch_etc2_mip.  chans: bytes (BC7) or halves (BC6H) per source pixel; modes: ICAMD_BC7_MODES_* / ICAMD_BC6H_MODES_*; swap_rb
// is BC7's.  The pixel pyramid is in the workspace by then (launch_mip_pass / launch_mip_f16_pass on the same stream).
hipError_t launch_bptc_mip(int codec, int chans, int modes, bool swap_rb, const BptcMipPlan &plan, const MipBuffers &buffers,
                           uint64_t src_image_stride, uint64_t dst_image_stride, hipStream_t stream);

// Compressed-domain operations on block grids.  BlockOpParams is what a kernel receives: launch_blockop
// (blockops_kernels.hip) fills it, per launch, from the caller's BlockOpCall and the plan of blockops_plan.h.
struct BlockOpParams {
  const uint8_t *src;
  uint8_t *dst;
  uint32_t in_rows, in_cols;    // source block grid
  uint32_t out_rows, out_cols;  // result block grid
  uint32_t total_out;
  uint32_t etc_strategy;
  uint32_t src_height, src_width;  // uncompressed pixels of the source (Downsample's single-block case)
  FastDiv div_out_cols;
  // Downsample / Pad: n_images equally shaped block grids per launch (total_out = out_rows * out_cols * n_images)
  uint32_t n_images = 1, out_per_image = 0;
  uint64_t src_image_stride = 0, dst_image_stride = 0;  // bytes
  FastDiv div_out_per_image = { 0, 0, 1 };
  // ETC1 Pad, kSmallerError, ONE launch (r05): the first border_wgs workgroups are the pad blocks' quad lanes
  // (border_lanes = 4 * pad blocks over all images, border_lanes_per_image of them per image), the rest copy the grid
  uint32_t border_wgs = 0, border_lanes = 0, border_lanes_per_image = 0;
  FastDiv div_border_lanes_per_image = { 0, 0, 1 };
};
// A Pad / Downsample call: the geometry the plan is made from (in.quad is the launcher's), the first image's blocks and the
// strides to the next ones in bytes.  Any number of images: the launcher groups them as the plan says.
struct BlockOpCall {
  BlockOpIn in;
  const uint8_t *src;
  uint8_t *dst;
  uint64_t src_image_stride, dst_image_stride;
};
hipError_t launch_pad(BlockOpCall call, hipStream_t stream);
hipError_t launch_downsample(BlockOpCall call, hipStream_t stream);
hipError_t launch_transcode_dxt1_to_etc1(void *blocks, uint64_t n_blocks, hipStream_t stream);  // 8-byte blocks, in place
hipError_t launch_transcode_dxt5_to_etc2_rgba8(void *blocks, uint64_t n_blocks, hipStream_t stream);  // 16-byte blocks, in place
hipError_t launch_transcode_dxt1_to_etc2_rgb8(void *blocks, uint64_t n_blocks, hipStream_t stream);   // 8-byte blocks, in place
hipError_t launch_transcode_bc4_to_eac_r11(void *blocks, uint64_t n_blocks, hipStream_t stream);      // 8-byte blocks, in place
hipError_t launch_transcode_bc5_to_eac_rg11(void *blocks, uint64_t n_blocks, hipStream_t stream);     // 16-byte blocks, in place
// CreateSolidImage: `words` (block_bytes / 4 of them) replicated n_blocks times.  CopySubimage: rows x cols blocks
// starting at block (r0, c0) of a grid src_cols blocks wide.
hipError_t launch_fill_blocks(void *dst, uint64_t n_blocks, int block_bytes, const uint32_t words[4], hipStream_t stream);
hipError_t launch_copy_subimage(int block_bytes, const void *src, uint32_t src_cols, uint32_t r0, uint32_t c0,
                                uint32_t rows, uint32_t cols, void *dst, hipStream_t stream, uint32_t n_images = 1,
                                uint64_t src_image_stride = 0, uint64_t dst_image_stride = 0);
// n_images grids of blocks_per_image blocks, dst_image_stride bytes apart, image i filled with words[i]
hipError_t launch_fill_blocks_batch(void *dst, uint64_t dst_image_stride, uint32_t blocks_per_image, int block_bytes,
                                    const uint32_t (*words)[4], uint32_t n_images, hipStream_t stream);
// Diagnostics: one wave spins for `ticks` periods of the constant-rate clock (s_memrealtime) and records how many shader
// cycles (s_memtime) passed meanwhile: d_out[0] = shader cycles, d_out[1] = constant-rate ticks.
hipError_t launch_clock_probe(uint64_t *d_out, uint64_t ticks, hipStream_t stream);

const char *dxt_kernel_name(int codec, int comps);
const char *etc1_kernel_name(int comps);
const char *pvrtc2_kernel_name();

}  // namespace icamd
#endif  // ICAMD_IC_LAUNCH_H_
