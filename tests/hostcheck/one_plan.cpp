// ftk_amd/csrc/one_plan.hpp without a GPU, for tests/one_launch_cases.py: the first line of the output names the limits of the one-launch
// pass as ftk_amd/csrc/sweep_params.hpp has them; then, for every line "nd n k cells n_vertices last_hits" of the input, a line
// "eligible nblocks nwg" -- what series.hip's series_one_eligible and series_plan_one compute from the same functions.  A program of its
// own: no Python in the process.
#include <cstdio>

#ifndef __HIPCC__      // (sweep_params.hpp marks two helpers for both sides: nothing to g++)
#define __host__
#define __device__
#endif
#include "../../ftk_amd/csrc/one_plan.hpp"

using namespace ftkx;

int main()
{
  printf("kOneMaxSteps=%d kOneMaxSlices=%d kOneParts=%d kOneKeys=%u kOneMaxBlocks=%u kOneOwnBlocks=%u block2=%llu block3=%llu SERIES_AMBIGUOUS=%d SERIES_INF=%d SERIES_OVERFLOW=%d SERIES_ONE=%d\n",
         kOneMaxSteps, kOneMaxSlices, kOneParts, kOneKeys, kOneMaxBlocks, kOneOwnBlocks, one_block_corners(2), one_block_corners(3),
         (int)SERIES_AMBIGUOUS, (int)SERIES_INF, (int)SERIES_OVERFLOW, (int)SERIES_ONE);
  int nd, n;
  unsigned long long k, cells, nv, hits;
  while (scanf("%d %d %llu %llu %llu %llu", &nd, &n, &k, &cells, &nv, &hits) == 6) {
    const u64 nblocks = one_blocks(nd, cells, n);
    printf("%d %llu %d\n", one_eligible_by_size(nd, n, (size_t)k, cells, nv, hits) ? 1 : 0, nblocks, one_workgroups(nblocks));
  }
  return 0;
}
