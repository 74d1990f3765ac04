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

}  // namespace ftkx
