// The one-launch pass for small series (one_kernel.hip): which series it takes and the grid it is launched with, as functions of the
// series' sizes alone.  series.hip (series_one_eligible, series_plan_one) asks here; the context's switches -- the hook, a slab pass, the
// passes left to sit out after a decline -- stay there.  No HIP in this file: tests/hostcheck/one_plan.cpp gives the same functions to
// tests/test_one_launch_cases.py, which places series on every limit below without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include "sweep_params.hpp"

namespace ftkx {

// corners of (step, corner) a staging batch of the kernel holds: SUB x G = 4 x (kThreads >> (nd + 1))
inline u64 one_block_corners(int nd) { return nd == 2 ? 128 : 64; }

inline u64 one_blocks(int nd, u64 cells, int n)
{
  const u64 bs = one_block_corners(nd);
  return (cells * (u64)n + bs - 1) / bs;
}

// workgroups of the launch: four or more blocks per workgroup, kOneOwnBlocks at most
inline int one_workgroups(u64 nblocks) { return (int)std::max<u64>(8, std::min<u64>(256, (nblocks + 3) / 4)); }

// n steps over k slices of n_vertices vertices each, `cells` corners in core; last_hits: the records of the context's last pass
inline bool one_eligible_by_size(int nd, int n, size_t k, u64 cells, u64 n_vertices, u64 last_hits)
{
  if (n > kOneMaxSteps || k > (size_t)kOneMaxSlices) return false;
  // small: at most kOneMaxBlocks staging batches of (step, corner) -- 128 corners a batch in 2D, 64 in 3D --, and slices whose reduction is a few
  // chunks' worth of reading
  if (one_blocks(nd, cells, n) > (u64)kOneMaxBlocks || n_vertices * (u64)k > (1ull << 22)) return false;
  // ... and where it wins.  Measured (tools: in-kernel stamps, NOTES.md round 5): a device-wide barrier costs ~10 us on this part, two of them plus
  // launch and hand-over ~35 us before any work; moving_extremum_3d 32^3 x 8 (sparse): 138 against 192 us for the kernel chain; woven 128^2 x 10
  // (7 357 records, BASELINE config 1): 92-105 against 91 -- hit-dense series of that size stay with the chain, whose kernels overlap nothing
  // either but whose ten launches cost no more than this kernel's barriers and its one wavefront per SIMD.  The last pass's record count decides.
  if (cells * (u64)n > (1ull << 17) && last_hits > 2048) return false;
  return true;
}

}  // namespace ftkx
