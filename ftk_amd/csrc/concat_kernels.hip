// Component planes -> the interleaved FP64 vector array on the device: dst[v * NC + k] = (double)plane_k[v], what the reference's stream does
// on one host thread with ndarray<T>::concat when a file keeps u, v, w in separate variables (include/ftk/ndarray/stream.hh:1347-1354,
// 1371-1378, 1423-1433; include/ftk/ndarray.hh:1157-1172), with the float32 widening (ndarray::from_array) in the same pass where the planes
// are float.  It is what stands between a reader of per-variable files and the resident V every kernel behind it reads.
//
// A pure streaming kernel: sizeof(T) bytes in and 8 out per element, at most one conversion.  A lane takes 16 bytes of every plane (NC
// global_load_dwordx4), which make NC * G doubles of one run of the output; a capped grid walks the vertices; every index is size_t.  The
// plan -- the common head peeled for alignment, the vertex-wise variant for pointers that cannot be aligned together, the tail -- and what
// the lanes do live in concat_steps.hpp, which tests/hostcheck/concat_host.cpp runs on the CPU.  No scratch.  FP64 values are moved as bits
// (tests/test_gpu_planar.py holds NaN payloads to numpy as 64-bit integers).
// Store shape, measured at 512^3 vertices against a streaming kernel of the parent commit that moves the same bytes (NOTES, "Planar vector
// snapshots"): double planes store their run from the lane that loaded it (NC 3 / 2: 1.04 x / 0.96 x the yardstick's slowest repetition;
// staged through LDS they took 1.03 x / 1.09 x the direct form's time); float planes stage a workgroup's tile through LDS, 24 or 16 KiB, so
// that every store instruction writes consecutive 16-byte pieces (NC 3 / 2: 0.89 x / 0.79 x the direct form's time, which was 1.06 x /
// 1.09 x the yardstick's slowest repetition).
#include <hip/hip_runtime.h>

#include "concat_steps.hpp"

namespace ftkx {

// the direct form: the 16-byte body of double planes (VEC), and every vertex on its own for both types
template <class T, int NC, bool VEC>
__global__ __launch_bounds__(kConcatThreads) void concat_kernel(ConcatPlanes<T, NC> pl, ConcatPlan p, double *__restrict__ dst)
{
  concat_lane<T, NC, VEC>(pl, p, dst, (size_t)blockIdx.x, (size_t)gridDim.x, (int)threadIdx.x);
}

// the staged form: the 16-byte body of float planes
template <class T, int NC>
__global__ __launch_bounds__(kConcatThreads) void concat_kernel_staged(ConcatPlanes<T, NC> pl, ConcatPlan p, double *__restrict__ dst)
{
  __shared__ __attribute__((aligned(16))) unsigned long long lds[concat_tile_words<T, NC>()];
  const size_t ntiles = concat_tiles(p);
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    concat_tile_fill<T, NC>(pl, p, tile, (int)threadIdx.x, lds);
    __syncthreads();
    concat_tile_drain<T, NC>(lds, p, tile, (int)threadIdx.x, dst);
    __syncthreads();
  }
  if (blockIdx.x == 0) concat_edges<T, NC>(pl, p, dst, (int)threadIdx.x);
}

template <class T, int NC> static bool launch_concat_nc(const T *const *planes, size_t count, double *dst, hipStream_t st)
{
  ConcatPlanes<T, NC> pl;
  for (int k = 0; k < NC; k ++) pl.p[k] = planes[k];
  const ConcatPlan p = concat_plan<T, NC>(pl, count, dst);
  const dim3 grid(concat_blocks(p)), block(kConcatThreads);
  if (!p.vec) hipLaunchKernelGGL((concat_kernel<T, NC, false>), grid, block, 0, st, pl, p, dst);
  else if constexpr (concat_staged<T>()) hipLaunchKernelGGL((concat_kernel_staged<T, NC>), grid, block, 0, st, pl, p, dst);
  else hipLaunchKernelGGL((concat_kernel<T, NC, true>), grid, block, 0, st, pl, p, dst);
  return p.vec;
}

// planes: nc (2 or 3) arrays of `count` elements each at a multiple of sizeof(T) bytes, dst: count * nc doubles at a multiple of 8 that
// overlap no plane, count >= 1: checked by the callers (ingest.hip).  Returns whether the 16-byte body was launched.
template <class T> bool launch_concat(const T *const *planes, int nc, size_t count, double *dst, hipStream_t st)
{
  return nc == 2 ? launch_concat_nc<T, 2>(planes, count, dst, st) : launch_concat_nc<T, 3>(planes, count, dst, st);
}

template bool launch_concat<double>(const double *const *, int, size_t, double *, hipStream_t);
template bool launch_concat<float>(const float *const *, int, size_t, double *, hipStream_t);

}  // namespace ftkx
