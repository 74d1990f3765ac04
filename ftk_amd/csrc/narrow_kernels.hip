// Half, bfloat16 and 8- / 16- / 32-bit integers -> FP64 on the device: dst[e] = static_cast<double>(src[e]), what the reference does on one host
// thread for every array that is not stored as doubles (ndarray<T>::from_array<T1>, include/ftk/ndarray.hh:401-410).  It is what stands
// between a snapshot that crosses PCIe at 1, 2 or 4 bytes per value and the FP64 slice every kernel behind it reads.
//
// A pure streaming kernel, like widen_kernels.hip: a lane takes 4 elements with one load (global_load_dword / dwordx2 / dwordx4 by the
// element's size), unpacks the sub-word types with shifts and sign extension, converts (v_cvt_f64_i32 / v_cvt_f64_u32; v_cvt_f32_f16 and
// v_cvt_f64_f32 for a half, a shift and v_cvt_f64_f32 for a bfloat16) and stores 32 bytes (two global_store_dwordx4); a capped grid walks
// the array in a grid-stride loop, two such groups a turn; every index is size_t.  The plan -- the head peeled for alignment, the element-wise variant for pointers
// that cannot be aligned together, the tail -- and the lane's loop live in narrow_steps.hpp, which tests/hostcheck/narrow_host.cpp runs on
// the CPU.  No LDS, no scratch.  The conversions keep subnormal halves under the mode this library is compiled with
// (tests/test_gpu_narrow.py holds all 65 536 patterns to numpy's astype as 64-bit integers).
#include <hip/hip_runtime.h>

#include "narrow_steps.hpp"

namespace ftkx {

template <class T, bool VEC>
__global__ __launch_bounds__(kWidenThreads) void narrow_kernel(const T *__restrict__ src, NarrowPlan p, double *__restrict__ dst)
{
  narrow_lane<T, VEC>(src, p, dst, (size_t)blockIdx.x, (size_t)gridDim.x, (int)threadIdx.x);
}

template <class T> static void launch_narrow_of(const void *src, size_t count, double *dst, hipStream_t st)
{
  const NarrowPlan p = narrow_plan(src, sizeof(T), count, dst);
  const T *s = static_cast<const T *>(src);
  if (p.vec) hipLaunchKernelGGL((narrow_kernel<T, true>), dim3(narrow_blocks(p)), dim3(kWidenThreads), 0, st, s, p, dst);
  else hipLaunchKernelGGL((narrow_kernel<T, false>), dim3(narrow_blocks(p)), dim3(kWidenThreads), 0, st, s, p, dst);
}

// src: `count` elements of type `dtype` (narrow_dtype_ok) at a multiple of their size, dst: `count` doubles at a multiple of 8, not
// overlapping, count >= 1: checked by the callers (ingest.hip).  Any other dtype: nothing is launched.
void launch_narrow(int dtype, const void *src, size_t count, double *dst, hipStream_t st)
{
  switch (dtype) {
  case NARROW_F16: launch_narrow_of<NarrowHalf>(src, count, dst, st); break;
  case NARROW_BF16: launch_narrow_of<NarrowBf16>(src, count, dst, st); break;
  case NARROW_U8: launch_narrow_of<uint8_t>(src, count, dst, st); break;
  case NARROW_I8: launch_narrow_of<int8_t>(src, count, dst, st); break;
  case NARROW_U16: launch_narrow_of<uint16_t>(src, count, dst, st); break;
  case NARROW_I16: launch_narrow_of<int16_t>(src, count, dst, st); break;
  case NARROW_U32: launch_narrow_of<uint32_t>(src, count, dst, st); break;
  case NARROW_I32: launch_narrow_of<int32_t>(src, count, dst, st); break;
  default: break;
  }
}

}  // namespace ftkx
