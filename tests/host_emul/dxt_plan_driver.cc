// dxt_plan_driver.cc -- prints dxt_launch_form (image-compression_amd/csrc/dxt_plan.h) for the arguments on its command line:
//   dxt_plan_driver codec comps block_cols row_stride [codec comps block_cols row_stride ...]
// one line per quadruple: log2_tile_cols wide_rows wave_workgroups lanes grid_x.  Built with g++ against the header alone
// (tests/test_dxt_plan_host.py).
#include <cstdio>
#include <cstdlib>

#include "dxt_plan.h"

int main(int argc, char **argv) {
  for (int i = 1; i + 3 < argc; i += 4) {
    const icamd::DxtLaunchForm f = icamd::dxt_launch_form(atoi(argv[i]), atoi(argv[i + 1]), (uint32_t)strtoul(argv[i + 2], nullptr, 10),
                                                          (uint32_t)strtoul(argv[i + 3], nullptr, 10));
    printf("%u %u %d %u %u\n", f.log2_tile_cols, f.wide_rows, f.wave_workgroups ? 1 : 0, f.lanes, f.grid_x);
  }
  return 0;
}
