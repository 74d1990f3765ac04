// Pass 2 on the device, the half that used to be serial per curve: from every record's neighbours, degree and component root
// (trace_device.hip: trace_neighbours_kernel, trace_unite_kernel, trace_roots_kernel) to the curves in the reference's order
// (geometry/cc2curves.hh:10-122, as trace.cpp's trace_impl reproduces it) without a walk.
//
//   ordinary        a record with at most two neighbours in the set; the others ("special") are on no curve
//   curve           a connected component of the ordinary records over the edges between them: a simple path, a cycle or one record
//   seed            the member with the smallest order key (corner with x most significant, then time, then type): a 64-bit atomic
//                   minimum per root.  Curves come in ascending order of their seed's key (the host sorts the seeds: see NOTES)
//   order in curve  reverse(front), seed, back: back = the chain from the seed's first ordinary neighbour (in the order of the neighbour
//                   list) to its end, front = the chain from its last one, unless the curve is closed -- then back holds everything
//
// The walk is replaced by list ranking.  Every edge between ordinary records is two arcs u -> v; arc 2u + s leaves u for its first
// (s = 0) or last (s = 1, only if it has two) ordinary neighbour.  The arc before u -> v is w -> u, w being u's other ordinary
// neighbour; arcs that leave a seed, or an end of a path, have none.  Pointer jumping over these links gives every arc the arc its
// chain starts with and its distance from it: an arc whose chain starts at a seed on side s, d links on, enters the record d + 1 hops
// from the seed on that side.  The links of a record and its distance are one 64-bit word, read and written whole, so a launch may
// update them in place: whatever state of another arc a thread reads is a true (link, distance) pair of that arc.
#include "ctx.hpp"

namespace ftkx {
namespace {

constexpr int kJumps = 4;      // jumps per arc and launch

__device__ inline u64 ld64(const u64 *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ inline void st64(u64 *p, u64 v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

// device-resident tags: strictly ascending?  a timestep the order key has no room for?  (the largest tag holds the largest timestep)
__global__ __launch_bounds__(256) void trace_check_kernel(const u64 *__restrict__ tags, int n, u64 per_step, unsigned *counters)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned bad = 0;
  if (i > 0 && !(tags[i - 1] < tags[i])) bad |= 1u;
  if (tags[i] / per_step >= (1ull << 24)) bad |= 2u;
  if (bad) atomicOr(&counters[TRO_CHECK], bad);
}

__global__ __launch_bounds__(256) void trace_order_init_kernel(const TraceOrder o)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < o.n) { o.best[i] = ~0ull; o.cyc[i] = 0; o.cnt[2 * i] = 0; o.cnt[2 * i + 1] = 0; o.indices[i] = -1; }
  if (i < TRO_WORDS && i != TRO_CHECK) o.counters[i] = 0;
}

// order key, ordinary neighbours, and the smallest key of every component
__global__ __launch_bounds__(256) void trace_order_keys_kernel(const TraceOrder o)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= o.n) return;
  const int d = o.deg[i];
  if (d > 2) { o.on[2 * i] = -1; o.on[2 * i + 1] = -1; atomicAdd(&o.counters[TRO_SPECIAL], 1u); return; }
  int first = -1, last = -1, cnt = 0;
  for (int q = 0; q < d; q ++) {
    const int j = o.nbr[(size_t)i * o.maxnb + q];
    if (j < 0 || j >= o.n || o.deg[j] > 2) continue;
    if (cnt == 0) first = j;
    last = j; cnt ++;
  }
  o.on[2 * i] = first;
  o.on[2 * i + 1] = cnt == 2 ? last : -1;
  const u64 tag = o.tags[i];
  const u64 type = tag % (u64)o.ntypes;
  u64 ci = tag / (u64)o.ntypes, rel[3] = {0, 0, 0};
  for (int a = 0; a < o.nd; a ++) { rel[a] = ci % (u64)o.sz[a]; ci /= (u64)o.sz[a]; }
  u64 key = 0;
  for (int a = 0; a < o.nd; a ++) key = key * (u64)o.sz[a] + rel[a];
  key = ((key << 24) | ci) * (u64)o.ntypes + type;
  o.key[i] = key;
  u64 *slot = &o.best[o.root[i]];
  if (key < ld64(slot)) atomicMin(slot, key);               // (the minimum only falls: a key that is not below it now never will be -- two long curves are two addresses)
}

__device__ inline bool is_seed(const TraceOrder &o, int u) { return o.deg[u] <= 2 && o.key[u] == o.best[o.root[u]]; }

// the arcs and the arc before each; the seeds, in no order
__global__ __launch_bounds__(256) void trace_order_arcs_kernel(const TraceOrder o)
{
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= o.n) return;
  const bool seed = is_seed(o, u);
  if (seed) o.seedlist[atomicAdd(&o.counters[TRO_SEEDS], 1u)] = u;
  for (int s = 0; s < 2; s ++) {
    const int a = 2 * u + s;
    int link = a; unsigned dist = 0;
    const int v = o.on[a], w = o.on[a ^ 1];
    if (v >= 0 && !seed && w >= 0) {
      const int p = o.on[2 * w] == u ? 2 * w : o.on[2 * w + 1] == u ? 2 * w + 1 : -1;
      if (p >= 0) { link = p; dist = 1; }
    }
    o.link[a] = ((u64)(unsigned)link << 32) | dist;
  }
}

__global__ __launch_bounds__(256) void trace_order_jump_kernel(const TraceOrder o, int round)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= 2 * o.n) return;
  u64 p = ld64(&o.link[a]);
  for (int it = 0; it <= kJumps; it ++) {
    const unsigned l = (unsigned)(p >> 32);
    if (l == (unsigned)a) return;                                  // starts its chain
    const u64 q = ld64(&o.link[l]);
    if ((unsigned)(q >> 32) == l) return;                          // points at the start of its chain: done
    if (it == kJumps) { o.counters[TRO_FLAGS + round] = 1; return; }
    p = (q & 0xffffffff00000000ull) | (u64)((unsigned)p + (unsigned)q);
    st64(&o.link[a], p);
  }
}

// the arc that ends a chain from a seed tells how long that side is (one writer per side), or that the curve is closed
__global__ __launch_bounds__(256) void trace_order_ends_kernel(const TraceOrder o)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= 2 * o.n) return;
  const int v = o.on[a];
  if (v < 0) return;
  const u64 p = o.link[a];
  const int h = (int)(p >> 32), sd = h >> 1, s = h & 1;
  const unsigned d = (unsigned)p;
  if (!is_seed(o, sd)) return;
  const int r = o.root[sd];
  if (v == sd) { o.cyc[r] = 1; if (s == 0) o.cnt[2 * r] = (int)d; }
  else if (o.on[2 * v + 1] < 0) o.cnt[2 * r + s] = (int)d + 1;
}

__global__ __launch_bounds__(256) void trace_order_info_kernel(const TraceOrder o, unsigned nseeds)
{
  const unsigned k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nseeds) return;
  const int u = o.seedlist[k], r = o.root[u];
  const int len = 1 + o.cnt[2 * r] + (o.cyc[r] ? 0 : o.cnt[2 * r + 1]);
  o.info[2 * (size_t)k] = o.key[u];
  o.info[2 * (size_t)k + 1] = (u64)(unsigned)u | ((u64)(unsigned)len << 32);
}

// curve c begins at off[c]: its seed goes behind its front
__global__ __launch_bounds__(256) void trace_order_place_kernel(const TraceOrder o, int ncurves, int npoints)
{
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncurves) return;
  const int u = o.sorted[c], r = o.root[u];
  const int pos = o.off[c] + (o.cyc[r] ? 0 : o.cnt[2 * r + 1]);
  o.seedpos[r] = pos;
  if (pos >= 0 && pos < npoints) o.indices[pos] = u; else o.counters[TRO_ERROR] = 1;
}

__global__ __launch_bounds__(256) void trace_order_scatter_kernel(const TraceOrder o, int npoints)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= 2 * o.n) return;
  const int v = o.on[a];
  if (v < 0) return;
  const u64 p = o.link[a];
  const int h = (int)(p >> 32), sd = h >> 1, s = h & 1;
  const long long hops = (long long)(unsigned)p + 1;
  if (!is_seed(o, sd) || v == sd) return;
  const int r = o.root[sd];
  if (s == 1 && o.cyc[r]) return;                                  // a closed curve is all `back`
  const long long pos = (long long)o.seedpos[r] + (s == 0 ? hops : -hops);
  if (pos >= 0 && pos < npoints) o.indices[pos] = v; else o.counters[TRO_ERROR] = 1;
}

// loop: at least two points, and the last one is a neighbour of the first (cc2curves.hh:113-122) -- every cycle, and every path of two
__global__ __launch_bounds__(256) void trace_order_loop_kernel(const TraceOrder o, int ncurves)
{
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncurves) return;
  const int b = o.off[c], e = o.off[c + 1];
  int loop = 0;
  if (e - b >= 2) {
    const int f = o.indices[b], l = o.indices[e - 1];
    if (f >= 0 && f < o.n && l >= 0) for (int q = 0; q < o.deg[f]; q ++) if (o.nbr[(size_t)f * o.maxnb + q] == l) loop = 1;
  }
  o.loop[c] = loop;
}

inline unsigned grid_of(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void launch_trace_check(const u64 *tags, int n, u64 per_step, unsigned *counters, hipStream_t st)
{
  hipLaunchKernelGGL(trace_check_kernel, dim3(grid_of((size_t)n)), dim3(256), 0, st, tags, n, per_step, counters);
}

void launch_trace_order_begin(const TraceOrder &o, hipStream_t st)
{
  const size_t n = (size_t)o.n;
  hipLaunchKernelGGL(trace_order_init_kernel, dim3(grid_of(n > TRO_WORDS ? n : (size_t)TRO_WORDS)), dim3(256), 0, st, o);
  hipLaunchKernelGGL(trace_order_keys_kernel, dim3(grid_of(n)), dim3(256), 0, st, o);
  hipLaunchKernelGGL(trace_order_arcs_kernel, dim3(grid_of(n)), dim3(256), 0, st, o);
}

void launch_trace_order_jump(const TraceOrder &o, int round, hipStream_t st)
{
  hipLaunchKernelGGL(trace_order_jump_kernel, dim3(grid_of(2 * (size_t)o.n)), dim3(256), 0, st, o, round);
}

void launch_trace_order_ends(const TraceOrder &o, unsigned nseeds, hipStream_t st)
{
  hipLaunchKernelGGL(trace_order_ends_kernel, dim3(grid_of(2 * (size_t)o.n)), dim3(256), 0, st, o);
  if (nseeds) hipLaunchKernelGGL(trace_order_info_kernel, dim3(grid_of(nseeds)), dim3(256), 0, st, o, nseeds);
}

void launch_trace_order_scatter(const TraceOrder &o, int ncurves, int npoints, hipStream_t st)
{
  if (!ncurves) return;
  hipLaunchKernelGGL(trace_order_place_kernel, dim3(grid_of((size_t)ncurves)), dim3(256), 0, st, o, ncurves, npoints);
  hipLaunchKernelGGL(trace_order_scatter_kernel, dim3(grid_of(2 * (size_t)o.n)), dim3(256), 0, st, o, npoints);
  hipLaunchKernelGGL(trace_order_loop_kernel, dim3(grid_of((size_t)ncurves)), dim3(256), 0, st, o, ncurves);
}

}  // namespace ftkx
