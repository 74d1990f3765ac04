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

// the blocks of one call's layout, and the candidate tables of its dimension on the device
static int reserve_trace(ftkx_ctx *c, int nd, const TraceLayout &L, const std::vector<int> &cand_off, const std::vector<int> &cand_flat)
{
  ftkx_pass2_state &s = c->p2;
  if (const int rc = s.trace_dev.reserve(c, L.dev_bytes, pass2_room(L.dev_bytes))) return rc;
  if (const int rc = s.trace_host.reserve(c, L.host_bytes, pass2_room(L.host_bytes))) return rc;
  if (s.tables_nd != nd) {
    s.tables_nd = 0;
    if (const int rc = s.tables.reserve(c, (cand_off.size() + cand_flat.size()) * sizeof(int), pass2_room((cand_off.size() + cand_flat.size()) * sizeof(int)))) return rc;
    HIP_TRY(c, hipMemcpy(s.tables.p, cand_off.data(), cand_off.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy((int *)s.tables.p + cand_off.size(), cand_flat.data(), cand_flat.size() * sizeof(int), hipMemcpyHostToDevice));
    s.tables_nd = nd;
  }
  return FTKX_OK;
}

// the geometry of the neighbour search and (o given) the ordering's copy of it
static TraceGeom trace_geom(int nd, const long long domain_st[3], const long long domain_sz[3], int maxnb, ftkx::TraceOrder *o = nullptr)
{
  TraceGeom g;
  memset(&g, 0, sizeof(g));
  g.nd = nd; g.ntypes = nd == 2 ? 12 : 60; g.maxnb = maxnb;
  g.prod[0] = 1;
  for (int a = 0; a < nd; a ++) { g.lb[a] = domain_st[a]; g.sz[a] = domain_sz[a]; g.prod[a + 1] = g.prod[a] * (unsigned long long)domain_sz[a]; }
  if (o) {
    o->nd = nd; o->ntypes = g.ntypes; o->maxnb = maxnb;
    for (int a = 0; a < 3; a ++) o->sz[a] = g.sz[a];
    for (int a = 0; a < 4; a ++) o->prod[a] = g.prod[a];
  }
  return g;
}

// neighbours, unite, roots: queued on the layout's arrays in the context's device block
static void launch_trace_front(ftkx_ctx *c, const TraceGeom &g, const TraceLayout &L, const u64 *d_tags, size_t n, size_t n_cand_off)
{
  void *d = c->p2.trace_dev.p;
  int *nbr = L.nbr.in<int>(d), *root = L.root.in<int>(d), *parent = L.parent.in<int>(d);
  unsigned char *deg = L.deg.in<unsigned char>(d);
  const int *d_off = (const int *)c->p2.tables.p, *d_cand = d_off + n_cand_off;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(trace_neighbours_kernel, dim3(grid), dim3(256), 0, c->stream, g, d_tags, (int)n, d_off, d_cand, nbr, deg, parent);
  hipLaunchKernelGGL(trace_unite_kernel, dim3(grid), dim3(256), 0, c->stream, (int)n, g.maxnb, (const int *)nbr, (const unsigned char *)deg, parent);
  hipLaunchKernelGGL(trace_roots_kernel, dim3(grid), dim3(256), 0, c->stream, (int)n, parent, root);
}

void ftkxh::trace_device_curves(const ftkx_ctx *c, const int **indices, const int **off, const int **loop)
{
  const OrderLayout &L = c->p2.order;
  void *d = c->p2.order_dev.p;
  *indices = L.indices.in<int>(d); *off = L.off.in<int>(d); *loop = L.loop.in<int>(d);
}

extern "C" {

static int trace_curves_ctx_impl(ftkx_ctx *c, int nd, const long long domain_st[3], const long long domain_sz[3], const ftkx_cp_t *recs, const unsigned long long *tags, size_t n, ftkx_curves *out)
{
  auto tag_of = [&](size_t i) { return tags ? tags[i] : recs[i].tag; };
  auto on_host = [&]() { return tags ? ftkx::trace_curves_tags(nd, domain_st, domain_sz, tags, n, out) : ftkx_trace_curves(nd, domain_st, domain_sz, recs, n, out); };
  if (!c) return on_host();
  c->p2.trace_last_path = 0;
  if ((nd != 2 && nd != 3) || !domain_st || !domain_sz || (!recs && !tags && n) || !out) return fail(c, FTKX_E_INVALID, "ftkx_trace_curves_ctx: bad arguments");
  // few records, or tags that do not come strictly ascending (the sweep delivers them so): the host does it all
  bool ascending = n < (1u << 30);
  for (size_t i = 1; i < n && ascending; i ++) ascending = tag_of(i - 1) < tag_of(i);
  if (n < 4096 || !ascending) return on_host();
  HIP_TRY(c, hipSetDevice(c->device));
  c->p2.trace_last_path = 1;
  const std::vector<int> *p_off, *p_flat;
  const int maxnb = trace_tables(nd, &p_off, &p_flat);
  const TraceLayout L(maxnb, n);
  if (const int rc = reserve_trace(c, nd, L, *p_off, *p_flat)) return rc;
  char *h = (char *)c->p2.trace_host.p, *d = (char *)c->p2.trace_dev.p;
  u64 *h_tags = L.tags.in<u64>(h);
  if (tags) memcpy(h_tags, tags, n * sizeof(u64)); else for (size_t i = 0; i < n; i ++) h_tags[i] = recs[i].tag;
  HIP_TRY(c, hipMemcpyAsync(d + L.tags.at, h_tags, n * 8, hipMemcpyHostToDevice, c->stream));
  launch_trace_front(c, trace_geom(nd, domain_st, domain_sz, maxnb), L, L.tags.in<const u64>(d), n, p_off->size());
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(h + L.nbr.at, d + L.nbr.at, L.down_bytes(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int rc = ftkx::trace_curves_with(nd, domain_st, domain_sz, h_tags, n, out, L.nbr.in<const int>(h), L.deg.in<const unsigned char>(h), L.root.in<const int>(h), maxnb);
  if (rc != FTKX_OK) return fail(c, rc, "ftkx_trace_curves_ctx: tracing failed (%d)", rc);
  return FTKX_OK;
}


int ftkx_trace_curves_ctx(ftkx_ctx *c, int nd, const long long domain_st[3], const long long domain_sz[3], const ftkx_cp_t *recs, size_t n, ftkx_curves *out)
{ return trace_curves_ctx_impl(c, nd, domain_st, domain_sz, recs, nullptr, n, out); }

int ftkx_trace_curves_tags_ctx(ftkx_ctx *c, int nd, const long long domain_st[3], const long long domain_sz[3], const unsigned long long *tags, size_t n, ftkx_curves *out)
{ return trace_curves_ctx_impl(c, nd, domain_st, domain_sz, nullptr, tags, n, out); }

int ftkx_trace_curves_device(ftkx_ctx *c, int nd, const long long domain_st[3], const long long domain_sz[3], const unsigned long long *tags, size_t n, int tags_on_device, ftkx_curves *out)
{
  if (!c) return FTKX_E_INVALID;
  if ((nd != 2 && nd != 3) || !domain_st || !domain_sz || (!tags && n) || !out) return fail(c, FTKX_E_INVALID, "ftkx_trace_curves_device: bad arguments");
  for (int a = 0; a < nd; a ++) if (domain_sz[a] < 1) return fail(c, FTKX_E_INVALID, "ftkx_trace_curves_device: empty domain");
  // FTKX_TRACE_PHASES=1: the host waits after every phase and prints its time (a measuring aid: the waits cost time of their own)
  static const bool phases = [] { const char *e = getenv("FTKX_TRACE_PHASES"); return e && atoi(e) > 0; }();
  if (n == 0) {
    c->p2.trace_last_path = 2;
    const int rc = ftkx::alloc_curves(out, 0, 0);
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

  ftkx_phase_clock clock{phases, c->stream, "ftkx_trace_curves_device"};
  const std::vector<int> *p_off, *p_flat;
  const int maxnb = trace_tables(nd, &p_off, &p_flat);
  const TraceLayout L(maxnb, n);
  const OrderLayout O(n);
  if (const int rc = reserve_trace(c, nd, L, *p_off, *p_flat)) return rc;
  if (const int rc = c->p2.order_dev.reserve(c, O.dev_bytes, pass2_room(O.dev_bytes))) return rc;
  if (const int rc = c->p2.order_host.reserve(c, O.host_bytes, pass2_room(O.host_bytes))) return rc;
  void *d = c->p2.trace_dev.p, *od = c->p2.order_dev.p, *oh = c->p2.order_host.p;
  ftkx::TraceOrder o;
  memset(&o, 0, sizeof(o));
  o.n = (int)n;
  const TraceGeom g = trace_geom(nd, domain_st, domain_sz, maxnb, &o);
  o.key = O.key.in<u64>(od); o.best = O.best.in<u64>(od); o.info = O.info.in<u64>(od); o.link = O.link.in<u64>(od);
  o.on = O.on.in<int>(od); o.cnt = O.cnt.in<int>(od); o.cyc = O.cyc.in<int>(od); o.seedpos = O.seedpos.in<int>(od); o.seedlist = O.seedlist.in<int>(od);
  o.indices = O.indices.in<int>(od); o.loop = O.loop.in<int>(od); o.off = O.off.in<int>(od); o.sorted = O.sorted.in<int>(od);
  o.counters = O.counters.in<unsigned>(od);
  u64 *h_info = O.h_info.in<u64>(oh);
  int *h_off = O.h_off.in<int>(oh), *h_sorted = O.h_sorted.in<int>(oh), *h_indices = O.h_indices.in<int>(oh), *h_loop = O.h_loop.in<int>(oh);
  unsigned *h_counters = O.h_counters.in<unsigned>(oh);

  clock.start();
  const u64 *d_tags = L.tags.in<const u64>(d);
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
    memcpy(c->p2.trace_host.p, tags, n * sizeof(u64));
    HIP_TRY(c, hipMemcpyAsync(L.tags.in<u64>(d), c->p2.trace_host.p, n * 8, hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, clock.lap(tags_on_device ? "check" : "upload", n));
  o.tags = d_tags; o.nbr = L.nbr.in<const int>(d); o.deg = L.deg.in<const unsigned char>(d); o.root = L.root.in<const int>(d);
  launch_trace_front(c, g, L, d_tags, n, p_off->size());
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, clock.lap("neighbours, unite, roots", n));
  ftkx::launch_trace_order_begin(o, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, clock.lap("keys, seeds, arcs", n));
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
  HIP_TRY(c, clock.lap("ordering rounds", (size_t)rounds));
  const size_t nseeds = h_counters[TRO_SEEDS], nspecial = h_counters[TRO_SPECIAL];
  if (!done || nseeds > n || nspecial > n) return other_way();        // (links that do not end: not a set of paths and cycles)
  ftkx::launch_trace_order_ends(o, (unsigned)nseeds, c->stream);
  HIP_TRY(c, hipGetLastError());
  if (nseeds) HIP_TRY(c, hipMemcpyAsync(h_info, o.info, nseeds * 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, clock.lap("ends, seeds down", nseeds));
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
  HIP_TRY(c, clock.lap("seed sort (host)", nseeds));
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
  HIP_TRY(c, clock.lap("scatter, curves down", npoints));
  if (const int rc = ftkx::alloc_curves(out, nseeds, npoints)) return fail(c, rc, "ftkx_trace_curves_device: out of memory");
  out->n_special = nspecial;
  for (size_t k = 0; k <= nseeds; k ++) out->offsets[k] = h_off[k];
  bool filled = true;
  for (size_t k = 0; k < npoints; k ++) { out->indices[k] = h_indices[k]; filled = filled && h_indices[k] >= 0; }
  if (nseeds) memcpy(out->loop, h_loop, nseeds * sizeof(int));
  if (!filled) { ftkx_free_curves(out); return other_way(); }
  c->p2.trace_last_path = 2;
  c->p2.order = O;
  if (phases) fprintf(stderr, "ftkx_trace_curves_device: %zu records, %zu curves, %zu special, %d rounds: %.1f us in all (with the waits of the phase timing)\n", n, nseeds, nspecial, rounds,
                      clock.us_in_all());
  return FTKX_OK;
}

int ftkx_trace_last_path(const ftkx_ctx *c) { return c ? c->p2.trace_last_path : 0; }

}  // extern "C"
