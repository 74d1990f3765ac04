// Float32 -> FP64 on the device: dst[e] = static_cast<double>(src[e]), what the reference's stream does on one host thread when it reads a
// "float32" file (include/ftk/ndarray/stream.hh:986-987, 1066-1069; ndarray::from_array, include/ftk/ndarray.hh:403-410).  It is what
// stands between a float32 snapshot, which crosses PCIe at 4 bytes per value, and the FP64 slice every kernel behind it reads.
//
// A pure streaming kernel: 4 bytes in and 8 out per element, one conversion.  A lane takes 16 bytes (one global_load_dwordx4) and stores
// 32 (two global_store_dwordx4); a capped grid walks the array in a grid-stride loop; every index is size_t (a 1024^3 snapshot has 2^30
// elements).  The plan -- the head peeled for alignment, the element-wise variant for pointers that cannot be aligned together, the tail --
// and the lane's loop live in widen_steps.hpp, which tests/hostcheck/widen_host.cpp runs on the CPU.  No LDS, no scratch.
// v_cvt_f64_f32 under the mode this library is compiled with keeps subnormal inputs (tests/test_gpu_f32.py holds every class of value to
// numpy's astype as 64-bit integers).
#include <hip/hip_runtime.h>

#include "widen_steps.hpp"

namespace ftkx {

template <bool VEC>
__global__ __launch_bounds__(kWidenThreads) void widen_kernel(const float *__restrict__ src, WidenPlan p, double *__restrict__ dst)
{
  widen_lane<VEC>(src, p, dst, (size_t)blockIdx.x, (size_t)gridDim.x, (int)threadIdx.x);
}

// src: `count` floats at a multiple of 4 bytes, dst: `count` doubles at a multiple of 8, not overlapping, count >= 1: checked by the callers (ingest.hip)
void launch_widen(const float *src, size_t count, double *dst, hipStream_t st)
{
  const WidenPlan p = widen_plan(src, count, dst);
  if (p.vec) hipLaunchKernelGGL((widen_kernel<true>), dim3(widen_blocks(p)), dim3(kWidenThreads), 0, st, src, p, dst);
  else hipLaunchKernelGGL((widen_kernel<false>), dim3(widen_blocks(p)), dim3(kWidenThreads), 0, st, src, p, dst);
}

}  // namespace ftkx
