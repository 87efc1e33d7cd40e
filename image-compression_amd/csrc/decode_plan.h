// decode_plan.h -- how a decode or metric call is cut into launches (ic_capi.hip).
//
// Host-only arithmetic on a handful of integers: no HIP header, no runtime call.  The decode and metric kernels index blocks
// with 32 bits, so one launch covers fewer than 2^31 blocks; tests/host_emul/decode_plan_driver.cc runs the same cut with g++,
// at the sizes no test can allocate and at small limits.
#ifndef ICAMD_DECODE_PLAN_H_
#define ICAMD_DECODE_PLAN_H_

#include <cstdint>

namespace icamd {

constexpr uint64_t kMaxLaunchBlocks = (1ull << 31) - 1;

// One launch: image_count whole images from first_image on, or (image_count == 1) the pixel_rows rows of first_image that
// begin at block row first_block_row.
struct LaunchPiece {
  uint32_t first_image, image_count, first_block_row, pixel_rows;
};

// Calls launch(piece) for every piece of n_images images of `height` pixel rows and block_cols blocks per block row, in order;
// a result other than 0 ends the walk and is returned.  Images of at most `limit` blocks go whole, as many per piece as the
// limit allows; a larger image goes in bands of limit / block_cols block rows (blocks are row-major, helper.h:218-262), the last
// band taking the rows that are left.  1 <= block_cols <= limit, height >= 1.  The limit is a parameter for the host driver
// alone: every entry point takes the default.
template <typename Launch>
int for_each_launch_piece(uint32_t height, uint32_t block_cols, uint32_t n_images, Launch &&launch,
                          uint64_t limit = kMaxLaunchBlocks) {
  const uint64_t block_rows = ((uint64_t)height + 3u) / 4u, per_image = block_rows * block_cols;
  if (per_image <= limit) {
    const uint64_t group = limit / per_image;  // >= 1
    for (uint64_t first = 0; first < n_images; first += group) {
      const uint64_t count = n_images - first < group ? n_images - first : group;
      if (const int rc = launch(LaunchPiece{ (uint32_t)first, (uint32_t)count, 0u, height })) return rc;
    }
    return 0;
  }
  const uint64_t band = limit / block_cols;
  for (uint32_t image = 0; image < n_images; ++image)
    for (uint64_t row0 = 0; row0 < block_rows; row0 += band) {
      const uint64_t left = height - row0 * 4u, rows = left < band * 4u ? left : band * 4u;
      if (const int rc = launch(LaunchPiece{ image, 1u, (uint32_t)row0, (uint32_t)rows })) return rc;
    }
  return 0;
}

}  // namespace icamd
#endif  // ICAMD_DECODE_PLAN_H_
