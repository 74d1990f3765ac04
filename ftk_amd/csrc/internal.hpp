// Shared between the translation units of libftkx.so; not part of the ABI.
#ifndef FTKX_INTERNAL_HPP
#define FTKX_INTERNAL_HPP
namespace ftkx {
// message returned by ftkx_last_error(NULL, ...) on this thread (entry points that have no context)
void set_global_error(const char *msg);
}
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/ftkx.h"
namespace ftkx {
// The library's test hooks come in two families, one environment variable each, "name=value,name=value" (DESIGN.md section 8):
// FTKX_SERIES_HOOKS (small, short, fold, split, one: which forms of the device-driven pass are taken; rank_max=N: buckets of the ordering
// step fuller than N are left to the host; bins=K: 2^K buckets, 0 .. 16, in place of the 2^14 -- 2^10 in a sparse split pass -- that
// series_bucket_geometry spreads the keys over, so that a small series fills its buckets like a large one) and FTKX_MASK_PLAN (swizzle,
// yg, zchunk, lmin, lcap, order, rows, lean: launch geometry of the mask kernels; parsed by read_mask_hooks, mask_plan.hpp).  Read at every use: tests switch them
// inside one process.  env_hook reads one knob of the first family.
inline long env_hook(const char *var, const char *name, long dflt)
{
  const char *e = getenv(var);
  if (!e) return dflt;
  const size_t n = strlen(name);
  for (const char *p = e; *p;) {
    while (*p == ',' || *p == ' ') p ++;
    if (!strncmp(p, name, n) && p[n] == '=') return atol(p + n + 1);
    while (*p && *p != ',') p ++;
  }
  return dflt;
}
inline bool env_hook_set(const char *var, const char *name) { return env_hook(var, name, -0x7fffffffL) != -0x7fffffffL; }
}
namespace ftkx {
// pass 2 with the neighbour search and the component labelling done on the device (trace.cpp <-> trace_device.hip)
int trace_candidates(int nd, std::vector<int> &cand_off, std::vector<int> &cand_flat);
int trace_curves_with(int nd, const long long *dst, const long long *dsz, const unsigned long long *tags, size_t n, ftkx_curves *out,
                      const int *nbr, const unsigned char *deg, const int *root, int maxnb);
int trace_curves_tags(int nd, const long long *dst, const long long *dsz, const unsigned long long *tags, size_t n, ftkx_curves *out);   // host only
// Result arrays as ftkx_free_curves / ftkx_free_trajectories release them (trace.cpp): the struct zeroed, every array malloc'ed for
// max(count, 1) elements (offsets: n_curves + 1, offsets[0] = 0), the counts set.  FTKX_E_NOMEM: nothing is left allocated.
int alloc_curves(ftkx_curves *out, size_t n_curves, size_t n_points);
int alloc_trajectories(ftkx_trajectories *out, size_t n_curves, size_t n_points);
}
#endif
