// decode_plan_driver.cc -- prints the pieces of for_each_launch_piece (image-compression_amd/csrc/decode_plan.h) for the arguments
// on its command line:
//   decode_plan_driver height block_cols n_images [limit [stop_after]]
// one line per piece: first_image image_count first_block_row pixel_rows.  limit 0 or absent: the header's default; stop_after
// k > 0: the callback answers 7 at piece k, which must end the walk and come back as the result (printed last, as "rc 7").
// Answers 2 for arguments outside the cut's precondition.  Built with g++ against the header alone
// (tests/test_decode_plan_host.py).
#include <cstdio>
#include <cstdlib>

#include "decode_plan.h"

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const uint32_t height = (uint32_t)strtoull(argv[1], nullptr, 10), block_cols = (uint32_t)strtoull(argv[2], nullptr, 10);
  const uint32_t n_images = (uint32_t)strtoull(argv[3], nullptr, 10);
  const uint64_t limit = argc > 4 ? strtoull(argv[4], nullptr, 10) : 0;
  const long stop_after = argc > 5 ? atol(argv[5]) : 0;
  if (height == 0 || block_cols == 0 || (limit != 0 && block_cols > limit)) return 2;
  long seen = 0;
  const auto print = [&](const icamd::LaunchPiece &p) {
    printf("%u %u %u %u\n", p.first_image, p.image_count, p.first_block_row, p.pixel_rows);
    return ++seen == stop_after ? 7 : 0;
  };
  const int rc = limit ? icamd::for_each_launch_piece(height, block_cols, n_images, print, limit)
                       : icamd::for_each_launch_piece(height, block_cols, n_images, print);
  printf("rc %d\n", rc);
  return 0;
}
