// Trajectory post-processing on the device: the maps and scans of post_process_steps.hpp as kernels.
//
// One scan building block serves every step.  A workgroup of 256 threads takes a tile of 2048 consecutive elements, eight per thread:
// every thread folds its eight in order, the threads' totals are scanned across the wave by shuffles (wave64: six steps) and across the
// four waves through LDS, and the thread runs through its eight again with what lies before them.  Operand order is kept everywhere
// (op(left, right)): the operators of adjust_time are not commutative in the bits they return.  Few points (<= kSingle): ONE workgroup
// walks the tiles with a carry -- one launch per scan.  Otherwise reduce-then-scan, three launches: every tile's total, an exclusive scan
// of the totals by one workgroup, the tiles again with their prefix.  Segments (curves, gaps between ordinal points, pieces) are part of
// the operators, not of the building block: a flag in the element (ScanTime*), or "the last flagged point so far" compared with the
// segment's head (ScanLast) -- the scans run over the flat point array whatever the curves' lengths.
#include "ctx.hpp"
#include "post_process_steps.hpp"

namespace ftkx {
namespace {

constexpr int kItems = 8, kTile = 256 * kItems, kSingle = 4 * kTile;

template <class T> __device__ inline T shfl_up_any(const T &v, unsigned d)
{
  static_assert(sizeof(T) % 4 == 0, "scanned in 32-bit words");
  int w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
  for (unsigned k = 0; k < sizeof(T) / 4; k ++) w[k] = __shfl_up(w[k], d);
  T r;
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}

// exclusive scan of one value per thread in thread order over the workgroup; `total` = all 256
template <class S> __device__ inline typename S::T block_scan_exclusive(typename S::T v, typename S::T &total)
{
  typedef typename S::T T;
  __shared__ T wave_total[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T inc = v;
  for (unsigned d = 1; d < 64; d <<= 1) {
    const T o = shfl_up_any(inc, d);
    if (lane >= (int)d) inc = S::op(o, inc);
  }
  if (lane == 63) wave_total[w] = inc;
  const T before = shfl_up_any(inc, 1);
  __syncthreads();
  T prefix = S::identity();
  total = S::identity();
  for (int k = 0; k < 4; k ++) { if (k == w) prefix = total; total = S::op(total, wave_total[k]); }
  __syncthreads();                                         // (wave_total is written again by the next call)
  return lane ? S::op(prefix, before) : prefix;
}

template <class S> __device__ inline typename S::T tile_total(const S &s, int tile, int n)
{
  typedef typename S::T T;
  const long long base = (long long)tile * kTile + (long long)threadIdx.x * kItems;
  T acc = S::identity();
  for (int k = 0; k < kItems; k ++) if (base + k < n) acc = S::op(acc, s.load((int)(base + k)));
  T total;
  (void)block_scan_exclusive<S>(acc, total);
  return total;
}

// the tile's elements with `carry` in front of them; returns the tile's total
template <class S> __device__ inline typename S::T tile_scan(const S &s, int tile, int n, typename S::T carry)
{
  typedef typename S::T T;
  const long long base = (long long)tile * kTile + (long long)threadIdx.x * kItems;
  T item[kItems];
  T acc = S::identity();
  for (int k = 0; k < kItems; k ++) {
    item[k] = base + k < n ? s.load((int)(base + k)) : S::identity();
    acc = S::op(acc, item[k]);
  }
  T total;
  T run = S::op(carry, block_scan_exclusive<S>(acc, total));
  for (int k = 0; k < kItems; k ++) {
    const T incl = S::op(run, item[k]);
    if (base + k < n) s.store((int)(base + k), incl, run);
    run = incl;
  }
  return total;
}

template <class S> __global__ __launch_bounds__(256) void pp_scan_single_kernel(const S s)
{
  const int n = s.n();
  typename S::T carry = S::identity();
  for (int tile = 0; (long long)tile * kTile < n; tile ++) carry = S::op(carry, tile_scan(s, tile, n, carry));
}

template <class S> __global__ __launch_bounds__(256) void pp_scan_reduce_kernel(const S s, typename S::T *agg)
{
  const typename S::T total = tile_total(s, (int)blockIdx.x, s.n());
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// the tiles' totals -> what lies before every tile
template <class S> __global__ __launch_bounds__(256) void pp_scan_spine_kernel(typename S::T *agg, int ntiles)
{
  typedef typename S::T T;
  T carry = S::identity();
  for (int b = 0; b < ntiles; b += 256) {
    const int k = b + (int)threadIdx.x;
    T total;
    const T before = block_scan_exclusive<S>(k < ntiles ? agg[k] : S::identity(), total);
    if (k < ntiles) agg[k] = S::op(carry, before);
    carry = S::op(carry, total);
  }
}

template <class S> __global__ __launch_bounds__(256) void pp_scan_tiles_kernel(const S s, const typename S::T *agg)
{
  const int n = s.n();
  if ((long long)blockIdx.x * kTile < n) (void)tile_scan(s, (int)blockIdx.x, n, agg[blockIdx.x]);
}

template <class F> __global__ __launch_bounds__(256) void pp_map_kernel(const F f)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < f.n()) f(i);
}

// post_process_steps' Run on a stream; grids are sized by the points that came in (what a step works on may be fewer: n() says)
struct DeviceRun {
  int np;
  void *agg;
  hipStream_t st;
  ftkx_phase_clock &clock;
  hipError_t err = hipSuccess;
  template <class F> void map(const F &f) { hipLaunchKernelGGL(pp_map_kernel<F>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, f); }
  template <class S> void scan(const S &s)
  {
    static_assert(sizeof(typename S::T) <= kPostProcAggBytes, "aggregates: kPostProcAggBytes per tile");
    typename S::T *a = (typename S::T *)agg;
    if (np <= kSingle) { hipLaunchKernelGGL(pp_scan_single_kernel<S>, dim3(1), dim3(256), 0, st, s); return; }
    const int ntiles = (np + kTile - 1) / kTile;
    hipLaunchKernelGGL(pp_scan_reduce_kernel<S>, dim3((unsigned)ntiles), dim3(256), 0, st, s, a);
    hipLaunchKernelGGL(pp_scan_spine_kernel<S>, dim3(1), dim3(256), 0, st, a, ntiles);
    hipLaunchKernelGGL(pp_scan_tiles_kernel<S>, dim3((unsigned)ntiles), dim3(256), 0, st, s, (const typename S::T *)a);
  }
  void phase(const char *what) { if (err == hipSuccess) err = clock.lap(what, (size_t)np); }
};

}  // namespace

size_t post_process_tiles(size_t np) { return (np + kTile - 1) / kTile + 1; }

hipError_t launch_post_process(const PostProc &p, void *agg, ftkx_phase_clock &clock)
{
  DeviceRun run{p.np, agg, clock.stream, clock};
  post_process_steps(p, run);
  return run.err != hipSuccess ? run.err : hipGetLastError();
}

}  // namespace ftkx
