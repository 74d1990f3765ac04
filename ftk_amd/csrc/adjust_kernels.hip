// Perturbation and clamp of a snapshot on the device: dst[e] = clamp(double(src[e]) + sigma * z(seed, t, e), lo, hi) -- the two steps that
// ndarray_stream::modified_callback (include/ftk/ndarray/stream.hh:1570-1604) runs on one host thread between the spatial smoothing and the
// temporal filter (ndarray::perturb, ndarray.hh:1331-1341; ndarray::clamp, ndarray.hh:1344-1350), with the float32 widening in front where
// the source is float.  What an element becomes, the noise and the plan of a launch are adjust_steps.hpp's, which
// tests/hostcheck/adjust_host.cpp runs on the CPU: the host build of that header is the kernel's oracle, bit for bit.
//
// An element-wise map.  A lane takes the pair of elements that shares one Philox4x32-10 call (16 bytes in and out on the FP64 side where the
// pointers allow it); a capped grid walks the array in a grid-stride loop; every index is size_t.  sigma, seed, t, lo and hi arrive as
// kernel arguments (SGPRs).  No LDS, no scratch.  The clamp-only instantiation is a streaming kernel (8 or 4 bytes in, 8 out, two compares
// and two selects); the perturbing ones execute, per element, half a Philox call (forty 32-bit multiplies for two elements), some thirty
// FP64 operations and a division, and in the tail branch of the quantile (15 % of the elements, so nearly every wavefront) a second
// division, a square root and the logarithm.  Measured at 512^3 (NOTES, "Perturbation and clamp"): clamp only 1.09 x a bare read of the same
// bytes, bound by HBM; the perturbing ones 2.4 x, bound by the VALU.
// Source == destination is allowed (T = double), so neither pointer is __restrict__.
#include <hip/hip_runtime.h>

#include "adjust_steps.hpp"

namespace ftkx {

template <class T, bool PERTURB, bool CLAMP>
__global__ __launch_bounds__(kAdjustThreads) void adjust_kernel(const T *src, AdjustPlan p, AdjustArgs a, double *dst)
{
  adjust_lane<T, PERTURB, CLAMP>(src, p, a, dst, (size_t)blockIdx.x, (size_t)gridDim.x, (int)threadIdx.x);
}

// src: `count` elements at a multiple of sizeof(T) bytes, dst: `count` doubles at a multiple of 8, equal to src or not overlapping it,
// count >= 1, perturb || clamp: checked by the callers (ingest.hip)
template <class T> void launch_adjust(const T *src, size_t count, bool perturb, bool clamp, const AdjustArgs &a, double *dst, hipStream_t st)
{
  const AdjustPlan p = adjust_plan<T>(src, count, dst);
  const dim3 grid(adjust_blocks(p)), block(kAdjustThreads);
  if (perturb && clamp) hipLaunchKernelGGL((adjust_kernel<T, true, true>), grid, block, 0, st, src, p, a, dst);
  else if (perturb) hipLaunchKernelGGL((adjust_kernel<T, true, false>), grid, block, 0, st, src, p, a, dst);
  else if (clamp) hipLaunchKernelGGL((adjust_kernel<T, false, true>), grid, block, 0, st, src, p, a, dst);
}

template void launch_adjust<double>(const double *, size_t, bool, bool, const AdjustArgs &, double *, hipStream_t);
template void launch_adjust<float>(const float *, size_t, bool, bool, const AdjustArgs &, double *, hipStream_t);

}  // namespace ftkx
