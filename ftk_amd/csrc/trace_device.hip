// Pass 2 on the hit set, its data-parallel half on the device: ftkx_trace_curves_ctx.
//
// The reference traces on the host (critical_point_tracker::trace_critical_points_offline, include/ftk/filters/critical_point_tracker.hh:
// 668-817: a std::set of elements, union-find over the neighbours that share a (d+1)-cell, geometry/cc2curves.hh:10-111 for the order
// of the points).  ftkx_trace_curves (trace.cpp) does that on host threads in 1.5 ms for the 62 181 records of woven 1024^2 x 64 -- four
// times the sweep that produced them.  Two of its phases are independent per record: the neighbour search (a handful of tag look-ups per
// record) and the component labelling (a union-find over the neighbour edges).  Those run here, on the GPU the records came from: the
// tags go up (8 bytes per record), a kernel finds every record's neighbours by binary search in the sorted tags, a lock-free union-find
// labels the components, and neighbours, degrees and roots come back (29-37 bytes per record).  What stays on the host is what is
// serial per curve -- seeds in the reference's element order, the walk along each curve -- in trace.cpp, unchanged.
//
// ftkx_trace_curves_device goes on from there without the host walk: the same three kernels, then the kernels of
// trace_order_kernels.hip -- order keys and an atomic minimum per component for the seeds, list ranking by pointer jumping over the arcs
// for every record's side of its seed and hop count, the chain ends for the lengths -- with two small exchanges in between (the jump
// rounds' "done" flag; 16 bytes per curve down, sorted by key on the host, 8 bytes per curve up) and one download of the finished
// curves: 4 bytes per point and per curve.  No size floor; tags may already be on the device.
#include <chrono>
#include "ctx.hpp"

using namespace ftkxh;
using namespace ftkx;

namespace {

struct TraceGeom { long long lb[3], sz[3]; unsigned long long prod[4]; int nd, ntypes, maxnb; };

// neighbours of record i inside the set, in the order of the candidate table (= the reference's element order)
__global__ __launch_bounds__(256) void trace_neighbours_kernel(const TraceGeom g, const u64 *__restrict__ tags, int n, const int *__restrict__ cand_off, const int *__restrict__ cand,
                                                               int *__restrict__ nbr, unsigned char *__restrict__ deg, int *__restrict__ parent)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 tag = tags[i];
  const int type = (int)(tag % (u64)g.ntypes);
  u64 ci = tag / (u64)g.ntypes;
  long long cc[4] = {0, 0, 0, 0};
  for (int d = 0; d < g.nd; d ++) { cc[d] = g.lb[d] + (long long)(ci % (u64)g.sz[d]); ci /= (u64)g.sz[d]; }
  cc[g.nd] = (long long)ci;
  int cnt = 0;
  for (int q = cand_off[type]; q < cand_off[type + 1]; q ++) {
    const int *c = cand + 5 * q;
    u64 idx = 0;
    bool ok = true;
    for (int d = 0; d < g.nd; d ++) {
      const long long rel = cc[d] + c[1 + d] - g.lb[d];
      ok = ok && rel >= 0 && rel < g.sz[d];
      idx += (u64)rel * g.prod[d];
    }
    const long long tt = cc[g.nd] + c[1 + g.nd];
    if (!ok || tt < 0) continue;
    idx += (u64)tt * g.prod[g.nd];
    const u64 want = idx * (u64)g.ntypes + (u64)c[0];
    int lo = 0, hi = n;                                   // first position with tags[pos] >= want
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (tags[mid] < want) lo = mid + 1; else hi = mid; }
    if (lo < n && tags[lo] == want && cnt < g.maxnb) nbr[(size_t)i * g.maxnb + cnt ++] = lo;
  }
  for (int q = cnt; q < g.maxnb; q ++) nbr[(size_t)i * g.maxnb + q] = -1;
  deg[i] = (unsigned char)cnt;
  parent[i] = i;
}

__device__ inline int uf_find(int *parent, int x)
{
  for (;;) {
    const int p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
    if (p == x) return x;
    const int pp = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
    if (pp != p) __atomic_store_n(&parent[x], pp, __ATOMIC_RELAXED);     // path halving (a benign race: any ancestor will do)
    x = p;
  }
}

// curves = connected components of the ordinary records (at most two neighbours): larger roots are linked under smaller ones only
__global__ __launch_bounds__(256) void trace_unite_kernel(int n, int maxnb, const int *__restrict__ nbr, const unsigned char *__restrict__ deg, int *parent)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || deg[i] > 2) return;
  for (int q = 0; q < deg[i]; q ++) {
    const int j = nbr[(size_t)i * maxnb + q];
    if (j < 0 || j >= i || deg[j] > 2) continue;           // (every edge is seen from both ends: once is enough)
    int a = i, b = j;
    for (;;) {
      a = uf_find(parent, a); b = uf_find(parent, b);
      if (a == b) break;
      if (a < b) { const int t = a; a = b; b = t; }
      if (atomicCAS(&parent[a], a, b) == a) break;
    }
  }
}

__global__ __launch_bounds__(256) void trace_roots_kernel(int n, int *parent, int *__restrict__ root)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) root[i] = uf_find(parent, i);
}

}  // namespace

// device / pinned buffers, kept with the context: tags | nbr | root | deg on both sides, parent and the candidate tables on the device
static int ensure_trace_buffers(ftkx_ctx *c, int nd, size_t n, int maxnb, const std::vector<int> &cand_off, const std::vector<int> &cand_flat)
{
  const size_t per = 8 + (size_t)maxnb * 4 + 4 + 1;
  const size_t bytes = n * per + 64, tbytes = (cand_off.size() + cand_flat.size()) * sizeof(int);
  if (c->tr_cap < bytes) {
    if (c->tr_dev) (void)hipFree(c->tr_dev);
    if (c->tr_host) (void)hipHostFree(c->tr_host);
    if (c->tr_parent) (void)hipFree(c->tr_parent);
    c->tr_dev = nullptr; c->tr_host = nullptr; c->tr_parent = nullptr; c->tr_cap = 0;
    const size_t cap = bytes + bytes / 4;
    HIP_TRY(c, hipMalloc(&c->tr_dev, cap));
    HIP_TRY(c, hipHostMalloc(&c->tr_host, cap, hipHostMallocNonCoherent));
    HIP_TRY(c, hipMalloc(&c->tr_parent, (cap / per + 1) * sizeof(int)));
    c->tr_cap = cap;
  }
  if (c->tr_tables_nd != nd) {
    if (c->tr_tables) (void)hipFree(c->tr_tables);
    c->tr_tables = nullptr; c->tr_tables_nd = 0;
    HIP_TRY(c, hipMalloc(&c->tr_tables, tbytes));
    HIP_TRY(c, hipMemcpy(c->tr_tables, cand_off.data(), cand_off.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy((int *)c->tr_tables + cand_off.size(), cand_flat.data(), cand_flat.size() * sizeof(int), hipMemcpyHostToDevice));
    c->tr_tables_nd = nd;
  }
  return FTKX_OK;
}

// the candidate tables of the neighbour search (trace.cpp), built once per thread and dimension; returns the slots per record
static int trace_tables(int nd, const std::vector<int> **off, const std::vector<int> **flat)
{
  static thread_local std::vector<int> cand_off[2], cand_flat[2];
  static thread_local int maxnb_of[2] = {0, 0};
  const int w = nd - 2;
  if (cand_off[w].empty()) maxnb_of[w] = ftkx::trace_candidates(nd, cand_off[w], cand_flat[w]);
  *off = &cand_off[w]; *flat = &cand_flat[w];
  return maxnb_of[w];
}

static TraceGeom trace_geom(int nd, const long long domain_st[3], const long long domain_sz[3], int maxnb)
{
  TraceGeom g;
  memset(&g, 0, sizeof(g));
  g.nd = nd; g.ntypes = nd == 2 ? 12 : 60; g.maxnb = maxnb;
  g.prod[0] = 1;
  for (int a = 0; a < nd; a ++) { g.lb[a] = domain_st[a]; g.sz[a] = domain_sz[a]; g.prod[a + 1] = g.prod[a] * (unsigned long long)domain_sz[a]; }
  return g;
}

// the ordering's arrays inside the context's block
static void order_arrays(const ftkx_ctx *c, ftkx::TraceOrder &o)
{
  const size_t cap = c->tr_ord_cap;
  u64 *q = (u64 *)c->tr_ord;
  o.key = q; q += cap; o.best = q; q += cap; o.info = q; q += 2 * cap; o.link = q; q += 2 * cap;
  int *r = (int *)q;
  o.on = r; r += 2 * cap; o.cnt = r; r += 2 * cap; o.cyc = r; r += cap; o.seedpos = r; r += cap; o.seedlist = r; r += cap;
  o.indices = r; r += cap; o.loop = r; r += cap; o.off = r; r += cap; o.sorted = r; r += cap;
  o.counters = (unsigned *)r;
}

void ftkxh::trace_device_curves(const ftkx_ctx *c, const int **indices, const int **off, const int **loop)
{
  ftkx::TraceOrder o;
  order_arrays(c, o);
  *indices = o.indices; *off = o.off; *loop = o.loop;
}

extern "C" {

static int trace_curves_ctx_impl(ftkx_ctx *c, int nd, const long long domain_st[3], const long long domain_sz[3], const ftkx_cp_t *recs, const unsigned long long *tags, size_t n, ftkx_curves *out)
{
  auto tag_of = [&](size_t i) { return tags ? tags[i] : recs[i].tag; };
  auto on_host = [&]() { return tags ? ftkx::trace_curves_tags(nd, domain_st, domain_sz, tags, n, out) : ftkx_trace_curves(nd, domain_st, domain_sz, recs, n, out); };
  if (!c) return on_host();
  c->tr_last_path = 0;
  constexpr bool timing = false;      // (phase timing to stderr: a debugging aid, compiled out)
  const auto tp0 = std::chrono::steady_clock::now();
  if ((nd != 2 && nd != 3) || !domain_st || !domain_sz || (!recs && !tags && n) || !out) return fail(c, FTKX_E_INVALID, "ftkx_trace_curves_ctx: bad arguments");
  // few records, or tags that do not come strictly ascending (the sweep delivers them so): the host does it all
  bool ascending = n < (1u << 30);
  for (size_t i = 1; i < n && ascending; i ++) ascending = tag_of(i - 1) < tag_of(i);
  if (n < 4096 || !ascending) return on_host();
  HIP_TRY(c, hipSetDevice(c->device));
  c->tr_last_path = 1;
  const std::vector<int> *p_off, *p_flat;
  const int maxnb = trace_tables(nd, &p_off, &p_flat);
  const std::vector<int> &cand_off = *p_off, &cand_flat = *p_flat;
  if (const int rc = ensure_trace_buffers(c, nd, n, maxnb, cand_off, cand_flat)) return rc;
  // layout (8-byte aligned pieces): tags u64[n] | nbr int[n * maxnb] | root int[n] | deg u8[n]
  const size_t off_nbr = n * 8, off_root = off_nbr + n * (size_t)maxnb * 4, off_deg = off_root + n * 4;
  u64 *h_tags = (u64 *)c->tr_host;
  if (tags) memcpy(h_tags, tags, n * sizeof(u64)); else for (size_t i = 0; i < n; i ++) h_tags[i] = recs[i].tag;
  char *d = (char *)c->tr_dev;
  const auto tp1 = std::chrono::steady_clock::now();
  HIP_TRY(c, hipMemcpyAsync(d, c->tr_host, n * 8, hipMemcpyHostToDevice, c->stream));
  const TraceGeom g = trace_geom(nd, domain_st, domain_sz, maxnb);
  const unsigned grid = (unsigned)((n + 255) / 256);
  const int *d_off = (const int *)c->tr_tables, *d_cand = d_off + cand_off.size();
  hipLaunchKernelGGL(trace_neighbours_kernel, dim3(grid), dim3(256), 0, c->stream, g, (const u64 *)d, (int)n, d_off, d_cand, (int *)(d + off_nbr), (unsigned char *)(d + off_deg), (int *)c->tr_parent);
  hipLaunchKernelGGL(trace_unite_kernel, dim3(grid), dim3(256), 0, c->stream, (int)n, maxnb, (const int *)(d + off_nbr), (const unsigned char *)(d + off_deg), (int *)c->tr_parent);
  hipLaunchKernelGGL(trace_roots_kernel, dim3(grid), dim3(256), 0, c->stream, (int)n, (int *)c->tr_parent, (int *)(d + off_root));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync((char *)c->tr_host + off_nbr, d + off_nbr, off_deg + n - off_nbr, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const auto tp2 = std::chrono::steady_clock::now();
  const char *h = (const char *)c->tr_host;
  const int rc = ftkx::trace_curves_with(nd, domain_st, domain_sz, h_tags, n, out, (const int *)(h + off_nbr), (const unsigned char *)(h + off_deg), (const int *)(h + off_root), maxnb);
  if (timing) {
    const auto tp3 = std::chrono::steady_clock::now();
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    fprintf(stderr, "ftkx_trace_curves_ctx: %zu records, maxnb %d: checks + tags %.0f us, device (up, 3 kernels, down %zu bytes) %.0f us, host (seeds, walks, curves) %.0f us\n",
            n, maxnb, us(tp0, tp1), off_deg + n - off_nbr, us(tp1, tp2), us(tp2, tp3));
  }
  if (rc != FTKX_OK) return fail(c, rc, "ftkx_trace_curves_ctx: tracing failed (%d)", rc);
  return FTKX_OK;
}


int ftkx_trace_curves_ctx(ftkx_ctx *c, int nd, const long long domain_st[3], const long long domain_sz[3], const ftkx_cp_t *recs, size_t n, ftkx_curves *out)
{ return trace_curves_ctx_impl(c, nd, domain_st, domain_sz, recs, nullptr, n, out); }

int ftkx_trace_curves_tags_ctx(ftkx_ctx *c, int nd, const long long domain_st[3], const long long domain_sz[3], const unsigned long long *tags, size_t n, ftkx_curves *out)
{ return trace_curves_ctx_impl(c, nd, domain_st, domain_sz, nullptr, tags, n, out); }

// the ordering's device arrays (TraceOrder) and pinned staging for `cap` records
static constexpr size_t kOrdDevPer = 6 * 8 + 11 * 4;                     // key, best, info[2], link[2] | on[2], cnt[2], cyc, seedpos, seedlist, indices, loop, off, sorted
static constexpr size_t kOrdHostPer = 16 + 8 + 8;                        // info | off, sorted | indices, loop
static int ensure_order_buffers(ftkx_ctx *c, size_t n)
{
  if (c->tr_ord_cap >= n + 2) return FTKX_OK;
  if (c->tr_ord) (void)hipFree(c->tr_ord);
  if (c->tr_ord_host) (void)hipHostFree(c->tr_ord_host);
  c->tr_ord = nullptr; c->tr_ord_host = nullptr; c->tr_ord_cap = 0;
  const size_t cap = n + n / 4 + 64;
  HIP_TRY(c, hipMalloc(&c->tr_ord, cap * kOrdDevPer + TRO_WORDS * sizeof(unsigned)));
  HIP_TRY(c, hipHostMalloc(&c->tr_ord_host, cap * kOrdHostPer + TRO_WORDS * sizeof(unsigned), hipHostMallocNonCoherent));
  c->tr_ord_cap = cap;
  return FTKX_OK;
}

static int empty_curves(ftkx_curves *out)
{
  memset(out, 0, sizeof(*out));
  out->offsets = (long long *)malloc(sizeof(long long));
  out->indices = (long long *)malloc(sizeof(long long));
  out->loop = (int *)malloc(sizeof(int));
  if (!out->offsets || !out->indices || !out->loop) return FTKX_E_NOMEM;
  out->offsets[0] = 0;
  return FTKX_OK;
}

int ftkx_trace_curves_device(ftkx_ctx *c, int nd, const long long domain_st[3], const long long domain_sz[3], const unsigned long long *tags, size_t n, int tags_on_device, ftkx_curves *out)
{
  if (!c) return FTKX_E_INVALID;
  if ((nd != 2 && nd != 3) || !domain_st || !domain_sz || (!tags && n) || !out) return fail(c, FTKX_E_INVALID, "ftkx_trace_curves_device: bad arguments");
  for (int a = 0; a < nd; a ++) if (domain_sz[a] < 1) return fail(c, FTKX_E_INVALID, "ftkx_trace_curves_device: empty domain");
  // FTKX_TRACE_PHASES=1: the host waits after every phase and prints its time (a measuring aid: the waits cost time of their own)
  static const bool phases = [] { const char *e = getenv("FTKX_TRACE_PHASES"); return e && atoi(e) > 0; }();
  if (n == 0) {
    c->tr_last_path = 2;
    const int rc = empty_curves(out);
    return rc == FTKX_OK ? rc : fail(c, rc, "ftkx_trace_curves_device: out of memory");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const int ntypes = nd == 2 ? 12 : 60;
  // what the device form does not cover goes the way of ftkx_trace_curves_tags_ctx, tags fetched first where they are on the device
  std::vector<unsigned long long> fetched;
  auto other_way = [&]() -> int {
    const unsigned long long *h = tags;
    if (tags_on_device) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      fetched.resize(n);
      HIP_TRY(c, hipMemcpy(fetched.data(), tags, n * sizeof(u64), hipMemcpyDeviceToHost));
      h = fetched.data();
    }
    return trace_curves_ctx_impl(c, nd, domain_st, domain_sz, nullptr, h, n, out);
  };
  u64 per_step = (u64)ntypes;
  bool covered = n < (1u << 30);
  {
    long double span = 16777216.0L * (long double)ntypes;      // the order key: corner, 24 bits of time, type (trace.cpp)
    for (int a = 0; a < nd; a ++) { span *= (long double)domain_sz[a]; per_step *= (u64)domain_sz[a]; }
    covered = covered && span < 18446744073709551615.0L;
  }
  if (covered && !tags_on_device) {
    for (size_t i = 1; i < n && covered; i ++) covered = tags[i - 1] < tags[i];
    covered = covered && tags[n - 1] / per_step < (1ull << 24);
  }
  if (!covered) return other_way();

  const auto tp0 = std::chrono::steady_clock::now();
  auto lap = [&](const char *what, size_t count) -> int {
    static thread_local std::chrono::steady_clock::time_point last;
    if (!phases) return FTKX_OK;
    if (!what) { last = std::chrono::steady_clock::now(); return FTKX_OK; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "ftkx_trace_curves_device: %-28s %8.1f us  (%zu)\n", what, std::chrono::duration<double, std::micro>(now - last).count(), count);
    last = now;
    return FTKX_OK;
  };
  const std::vector<int> *p_off, *p_flat;
  const int maxnb = trace_tables(nd, &p_off, &p_flat);
  if (const int rc = ensure_trace_buffers(c, nd, n, maxnb, *p_off, *p_flat)) return rc;
  if (const int rc = ensure_order_buffers(c, n)) return rc;
  const size_t off_nbr = n * 8, off_root = off_nbr + n * (size_t)maxnb * 4, off_deg = off_root + n * 4;
  char *d = (char *)c->tr_dev;
  const size_t cap = c->tr_ord_cap;
  ftkx::TraceOrder o;
  memset(&o, 0, sizeof(o));
  o.n = (int)n; o.nd = nd; o.ntypes = ntypes; o.maxnb = maxnb;
  o.prod[0] = 1;
  for (int a = 0; a < nd; a ++) { o.sz[a] = domain_sz[a]; o.prod[a + 1] = o.prod[a] * (u64)domain_sz[a]; }
  order_arrays(c, o);
  // pinned: info u64[2 cap] | off int[cap] | sorted int[cap] | indices int[cap] | loop int[cap] | counters
  u64 *h_info = (u64 *)c->tr_ord_host;
  int *h_off = (int *)(h_info + 2 * cap), *h_sorted = h_off + cap, *h_indices = h_sorted + cap, *h_loop = h_indices + cap;
  unsigned *h_counters = (unsigned *)(h_loop + cap);

  lap(nullptr, 0);
  const u64 *d_tags = (const u64 *)d;
  if (tags_on_device) {
    // one check kernel and its flag: strictly ascending, no timestep beyond the key's 24 bits
    d_tags = (const u64 *)tags;
    HIP_TRY(c, hipMemsetAsync(o.counters, 0, TRO_WORDS * sizeof(unsigned), c->stream));
    ftkx::launch_trace_check(d_tags, (int)n, per_step, o.counters, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(h_counters, o.counters, TRO_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_counters[TRO_CHECK]) return other_way();
  } else {
    memcpy(c->tr_host, tags, n * sizeof(u64));
    HIP_TRY(c, hipMemcpyAsync(d, c->tr_host, n * 8, hipMemcpyHostToDevice, c->stream));
  }
  if (const int rc = lap(tags_on_device ? "check" : "upload", n)) return rc;
  o.tags = d_tags; o.nbr = (const int *)(d + off_nbr); o.deg = (const unsigned char *)(d + off_deg); o.root = (const int *)(d + off_root);
  const TraceGeom g = trace_geom(nd, domain_st, domain_sz, maxnb);
  const unsigned grid = (unsigned)((n + 255) / 256);
  const int *d_off = (const int *)c->tr_tables, *d_cand = d_off + p_off->size();
  hipLaunchKernelGGL(trace_neighbours_kernel, dim3(grid), dim3(256), 0, c->stream, g, d_tags, (int)n, d_off, d_cand, (int *)(d + off_nbr), (unsigned char *)(d + off_deg), (int *)c->tr_parent);
  hipLaunchKernelGGL(trace_unite_kernel, dim3(grid), dim3(256), 0, c->stream, (int)n, maxnb, o.nbr, o.deg, (int *)c->tr_parent);
  hipLaunchKernelGGL(trace_roots_kernel, dim3(grid), dim3(256), 0, c->stream, (int)n, (int *)c->tr_parent, (int *)(d + off_root));
  HIP_TRY(c, hipGetLastError());
  if (const int rc = lap("neighbours, unite, roots", n)) return rc;
  ftkx::launch_trace_order_begin(o, c->stream);
  HIP_TRY(c, hipGetLastError());
  if (const int rc = lap("keys, seeds, arcs", n)) return rc;
  // pointer jumping: a launch doubles what every arc knows at least; the flag of the last launch is read every third one
  int max_rounds = 2;
  while (max_rounds < 40 && (1ull << (max_rounds - 1)) < 2 * (u64)n) max_rounds ++;
  int rounds = 0;
  bool done = false;
  while (!done && rounds < max_rounds) {
    const int upto = std::min(max_rounds, rounds + 3);
    for (; rounds < upto; rounds ++) ftkx::launch_trace_order_jump(o, rounds, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(h_counters, o.counters, TRO_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    done = h_counters[TRO_FLAGS + rounds - 1] == 0;
  }
  if (const int rc = lap("ordering rounds", (size_t)rounds)) return rc;
  const size_t nseeds = h_counters[TRO_SEEDS], nspecial = h_counters[TRO_SPECIAL];
  if (!done || nseeds > n || nspecial > n) return other_way();        // (links that do not end: not a set of paths and cycles)
  ftkx::launch_trace_order_ends(o, (unsigned)nseeds, c->stream);
  HIP_TRY(c, hipGetLastError());
  if (nseeds) HIP_TRY(c, hipMemcpyAsync(h_info, o.info, nseeds * 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (const int rc = lap("ends, seeds down", nseeds)) return rc;
  // the curves in the order of their seeds' keys (the host path sorts the same pairs)
  struct SeedInfo { u64 key, rec_len; };
  SeedInfo *si = (SeedInfo *)h_info;
  std::sort(si, si + nseeds, [](const SeedInfo &a, const SeedInfo &b) { return a.key < b.key; });
  size_t npoints = 0;
  bool sane = true;
  for (size_t k = 0; k < nseeds && sane; k ++) {
    const size_t rec = (size_t)(si[k].rec_len & 0xffffffffull), len = (size_t)(si[k].rec_len >> 32);
    sane = rec < n && len >= 1 && npoints + len <= n;
    h_off[k] = (int)npoints; h_sorted[k] = (int)rec;
    npoints += len;
  }
  h_off[nseeds] = (int)npoints;
  if (!sane || npoints + nspecial != n) return other_way();
  if (const int rc = lap("seed sort (host)", nseeds)) return rc;
  if (nseeds) {
    HIP_TRY(c, hipMemcpyAsync(o.off, h_off, (nseeds + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(o.sorted, h_sorted, nseeds * sizeof(int), hipMemcpyHostToDevice, c->stream));
    ftkx::launch_trace_order_scatter(o, (int)nseeds, (int)npoints, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(h_indices, o.indices, npoints * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_loop, o.loop, nseeds * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_counters, o.counters, TRO_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_counters[TRO_ERROR]) return other_way();
  }
  if (const int rc = lap("scatter, curves down", npoints)) return rc;
  memset(out, 0, sizeof(*out));
  out->n_curves = nseeds; out->n_points = npoints; out->n_special = nspecial;
  out->offsets = (long long *)malloc((nseeds + 1) * sizeof(long long));
  out->indices = (long long *)malloc((npoints ? npoints : 1) * sizeof(long long));
  out->loop = (int *)malloc((nseeds ? nseeds : 1) * sizeof(int));
  if (!out->offsets || !out->indices || !out->loop) { ftkx_free_curves(out); return fail(c, FTKX_E_NOMEM, "ftkx_trace_curves_device: out of memory"); }
  for (size_t k = 0; k <= nseeds; k ++) out->offsets[k] = h_off[k];
  bool filled = true;
  for (size_t k = 0; k < npoints; k ++) { out->indices[k] = h_indices[k]; filled = filled && h_indices[k] >= 0; }
  if (nseeds) memcpy(out->loop, h_loop, nseeds * sizeof(int));
  if (!filled) { ftkx_free_curves(out); return other_way(); }
  c->tr_last_path = 2;
  if (phases) fprintf(stderr, "ftkx_trace_curves_device: %zu records, %zu curves, %zu special, %d rounds: %.1f us in all (with the waits of the phase timing)\n", n, nseeds, nspecial, rounds,
                      std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tp0).count());
  return FTKX_OK;
}

int ftkx_trace_last_path(const ftkx_ctx *c) { return c ? c->tr_last_path : 0; }

}  // extern "C"
