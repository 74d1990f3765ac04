// Temporal Gaussian smoothing on the device: out[e] = sum over K taps of w[i] * x_i[e], the x_i being up to K raw snapshots resident in HBM.
//
// Reference (host, K passes of ndarray operators over a snapshot): include/ftk/filters/streaming_filter.hh, get().  Which snapshots an
// emission reads and the arithmetic of one element live in temporal_steps.hpp, which tests/hostcheck/temporal_steps.cpp runs on the CPU:
// the accumulator starts as the rounded product w[0] * x0, every later tap is a rounded multiply and a rounded add in order
// (-ffp-contract=off), taps on the same snapshot are not merged.
//
// A pure streaming kernel: per element 8 bytes from every DISTINCT array and 8 bytes out, against 2 K - 1 FP64 operations and a few
// selects.  A lane takes 16 bytes of every array at a time (one global_load_dwordx4 each, all issued before the first is needed) and
// stores 16; a capped grid walks the arrays in a grid-stride loop; every index is size_t (a 1024^3 slice is 8.6 GB).  An array that
// several taps read (the edge phases of a series) is loaded once: the kernel is instantiated per (K, number of distinct arrays), the
// values stay in registers and a tap picks its own by selects on a uniform index.  Weights, pointers and taps are kernel arguments.
// Pointers that are not multiples of 16 (ftkx_temporal_combine takes any) go through the same code at 8 bytes per lane.
#include <hip/hip_runtime.h>

#include "temporal_steps.hpp"

namespace ftkx {

template <int K, int NSRC, int W>
__global__ __launch_bounds__(kTemporalThreads) void temporal_kernel(TemporalArgs a, size_t count, double *__restrict__ out)
{
  temporal_lane<K, NSRC, W>(a, count, out, (size_t)blockIdx.x, (size_t)gridDim.x, (int)threadIdx.x);
}

template <int K, int NSRC> static void launch_temporal_kn(const TemporalArgs &a, size_t count, double *out, hipStream_t st)
{
  if (temporal_aligned16(a, NSRC, out)) hipLaunchKernelGGL((temporal_kernel<K, NSRC, 2>), dim3(temporal_blocks(count, 2)), dim3(kTemporalThreads), 0, st, a, count, out);
  else hipLaunchKernelGGL((temporal_kernel<K, NSRC, 1>), dim3(temporal_blocks(count, 1)), dim3(kTemporalThreads), 0, st, a, count, out);
}

template <int K, int NSRC> struct TemporalDispatch {
  static void go(int nsrc, const TemporalArgs &a, size_t count, double *out, hipStream_t st)
  {
    if (nsrc == NSRC) launch_temporal_kn<K, NSRC>(a, count, out, st);
    else TemporalDispatch<K, NSRC - 1>::go(nsrc, a, count, out, st);
  }
};
template <int K> struct TemporalDispatch<K, 0> { static void go(int, const TemporalArgs &, size_t, double *, hipStream_t) {} };

// arrays: ksize device pointers of `count` doubles, repeats allowed; weights: ksize doubles on the host; ksize odd in [1, 9] and count >= 1:
// checked by the callers (ingest.hip)
void launch_temporal(const double *const *arrays, int ksize, const double *weights, size_t count, double *out, hipStream_t st)
{
  TemporalArgs a;
  const int nsrc = temporal_plan(arrays, ksize, weights, &a);
#define TEMPORAL_CASE(k) case k: TemporalDispatch<k, k>::go(nsrc, a, count, out, st); break
  switch (ksize) { TEMPORAL_CASE(1); TEMPORAL_CASE(3); TEMPORAL_CASE(5); TEMPORAL_CASE(7); TEMPORAL_CASE(9); default: break; }
#undef TEMPORAL_CASE
}

}  // namespace ftkx
