// TEST INFRASTRUCTURE.  Compiles the mask kernels' launch plan and the decode of blockIdx.z that mask_march6_kernel runs
// (ftk_amd/csrc/mask_plan.hpp: plan_masks, zplan_decode) for the HOST with g++, so that tests/test_mask_order.py can walk every
// workgroup of a launch without a GPU.  Nothing in the product loads this library.
#include "../../ftk_amd/csrc/mask_plan.hpp"

using namespace ftkx;

extern "C" {

// shape = {nd, scalar_mode, DW, DH, DD, mask_pitch}; hooks as FTKX_MASK_PLAN would hold them (NULL: not set) ->
// head[6] = family, grid[2], njobs, npieces, sgroup, 1 if the decode was written; where = (job, piece) of bz = 0 .. grid[2] - 1 (3D scalar
// marching kernel only, and only if `cap` pairs hold them)
void hc_mask_order(const int *shape, const char *mask_plan, int njobs, long long *head, unsigned *where, unsigned cap)
{
  const MaskShape s{shape[0], shape[1], {shape[2], shape[3], shape[4]}, shape[5]};
  const MaskPlan p = plan_masks(s, parse_mask_hooks(mask_plan, nullptr), njobs, false);
  head[0] = p.family; head[1] = p.grid[2]; head[2] = p.njobs; head[3] = p.z.npieces; head[4] = p.z.sgroup; head[5] = 0;
  if (p.family != MASK_MARCH6 || p.grid[2] > cap) return;
  for (unsigned bz = 0; bz < p.grid[2]; bz ++) { const ZWhere w = zplan_decode(p.z, p.njobs, bz); where[2 * bz] = w.job; where[2 * bz + 1] = w.piece; }
  head[5] = 1;
}
}
