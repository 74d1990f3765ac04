// Auxiliary scalar fields sampled at critical points (ftkx_sample_aux): one lane per record.  16 bytes in -- tag and aux word --, one or
// two doubles out; the arithmetic is sample_steps.hpp, which tests/hostcheck/sample_host.cpp runs on the CPU.
//
// A record is a chain of dependent gathers like the record kernels' (sweep_device.hpp, make_record_impl): tag -> corner -> the slice
// pointers of its timestep (a small table indexed by timestep - t_min) -> the nd + 1 vertices' field values (scalar input: the 4 or 6
// neighbours of each vertex) and aux values -> solve -> lerp.  Nothing here hides a memory latency but other wavefronts, so all loads of
// a record are issued before the solve and the kernel keeps its registers low enough for full occupancy.  Records arrive in tag order:
// neighbouring lanes mostly read neighbouring rows of the same slices.  No LDS, no scratch, no atomics.
#include <hip/hip_runtime.h>

#include "sample_steps.hpp"
#include "sweep_params.hpp"   // CNT_PASS

namespace ftkx {

static __constant__ fan_table<3> c_sample_fan3 = make_fan<3>();
static __constant__ fan_table<4> c_sample_fan4 = make_fan<4>();

template <int ND> __device__ inline const fan_table<ND + 1> &sample_fan();
template <> __device__ inline const fan_table<3> &sample_fan<2>() { return c_sample_fan3; }
template <> __device__ inline const fan_table<4> &sample_fan<3>() { return c_sample_fan4; }

// out: n doubles per slot asked for, slot 1's (where asked for) in front of slot 2's
template <int ND>
__global__ __launch_bounds__(kSampleThreads) void sample_kernel(SampleMesh m, const SampleIn *__restrict__ in, size_t n, const SampleSlice *__restrict__ tab, int t_min,
                                                                 unsigned slots, double *__restrict__ out)
{
  const size_t i = (size_t)blockIdx.x * (size_t)kSampleThreads + (size_t)threadIdx.x;
  if (i >= n) return;
  double r[2];
  sample_record<ND>(m, sample_fan<ND>(), in[i], tab, t_min, slots, r);
  size_t at = i;
  if (slots & 1u) { out[at] = r[0]; at += n; }
  if (slots & 2u) out[at] = r[1];
}

// every record has been decoded on the host (ftkx_api.hip, ftkx_sample_aux): its vertices lie inside the arrays of `tab`
void launch_sample(int nd, const SampleMesh &m, const SampleIn *in, size_t n, const SampleSlice *tab, int t_min, unsigned slots, double *out, hipStream_t st)
{
  if (n == 0) return;
  const dim3 grid((unsigned)((n + (size_t)kSampleThreads - 1) / (size_t)kSampleThreads));
  if (nd == 2) hipLaunchKernelGGL((sample_kernel<2>), grid, dim3(kSampleThreads), 0, st, m, in, n, tab, t_min, slots, out);
  else hipLaunchKernelGGL((sample_kernel<3>), grid, dim3(kSampleThreads), 0, st, m, in, n, tab, t_min, slots, out);
}

// ---- the series pass samples its own records (ftkx_set_series_sampling) ------------------------------------------------------------------
// In place over the records a pass left in device memory (series.hip queues it between the record kernel and the finish kernel): how many
// there are is read on the device, the grid is whatever the host chose without knowing -- a stride loop, one lane per record.  The loop
// body is series_sample_lane (sample_steps.hpp), which the CPU build runs as this kernel's oracle.  The two doubles of a record are stored
// the way the record kernel stores the record (series_kernels.hip): relaxed, system scope -- they go through to memory, where the copy
// kernel, which may be resident on another XCD and polling already, finds them once its acquire has let it past.  No LDS, no scratch, no
// atomic read-modify-write.
template <int ND>
__global__ __launch_bounds__(kSampleThreads) void series_sample_kernel(SampleMesh m, ftkx_cp_t *recs, const u64 *__restrict__ counters, u64 capacity,
                                                                        const SampleSlice *__restrict__ tab, int t_min, int ntab, unsigned slots)
{
  u64 n = counters[CNT_PASS];
  if (n > capacity) n = capacity;
  const size_t first = (size_t)blockIdx.x * (size_t)kSampleThreads + (size_t)threadIdx.x, stride = (size_t)gridDim.x * (size_t)kSampleThreads;
  series_sample_lane<ND>(m, sample_fan<ND>(), recs, (size_t)n, tab, t_min, ntab, slots, first, stride,
                         [](double *at, double v) { __hip_atomic_store(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); });
}

void launch_series_sample(int nd, const SampleMesh &m, ftkx_cp_t *recs, const u64 *counters, u64 capacity, const SampleSlice *tab, int t_min, int ntab, unsigned slots,
                          unsigned workgroups, hipStream_t st)
{
  const dim3 grid(workgroups < 1u ? 1u : workgroups);
  if (nd == 2) hipLaunchKernelGGL((series_sample_kernel<2>), grid, dim3(kSampleThreads), 0, st, m, recs, counters, capacity, tab, t_min, ntab, slots);
  else hipLaunchKernelGGL((series_sample_kernel<3>), grid, dim3(kSampleThreads), 0, st, m, recs, counters, capacity, tab, t_min, ntab, slots);
}

}  // namespace ftkx
