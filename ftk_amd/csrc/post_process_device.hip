// Pass 2, its second half on the device: ftkx_post_process_curves_device and, with the trace in front of it, ftkx_pass2_device.
//
// ftkx_post_process_curves (trace.cpp) hands the traced curves to host threads one by one.  Every step of it -- smoothing the types along
// the ordinal points and across the gaps between them, rotating loops, split_all, re-ordering in time, adjust_time -- is a map or a scan
// over the flat array of points with the curves' heads as borders (post_process_steps.hpp), and the only floating-point operations are
// max and min: the kernels of post_process_kernels.hip give the same trajectories bit for bit.  Up go 16 bytes per record (type, aux
// word, t) and, where the curves are not on the device already, 4 bytes per point and 8 per curve; the host waits once for the counts of
// pieces and points, then once for the trajectories: 16 bytes per point, 12 per piece.  After ftkx_trace_curves_device the curves lie in
// the context's ordering buffers (indices, offsets, loop flags): ftkx_pass2_device reads them there.
#include <chrono>
#include "ctx.hpp"
#include "post_process_steps.hpp"

using namespace ftkxh;
using namespace ftkx;

namespace {

struct PpBuffers {                    // offsets into the context's device block / pinned block for one call
  size_t total = 0;
  size_t take(size_t bytes) { const size_t at = total; total += (bytes + 15) & ~(size_t)15; return at; }
};

int ensure_pp_buffers(ftkx_ctx *c, size_t dev_bytes, size_t host_bytes)
{
  if (c->pp_dev_cap < dev_bytes) {
    if (c->pp_dev) (void)hipFree(c->pp_dev);
    c->pp_dev = nullptr; c->pp_dev_cap = 0;
    const size_t cap = dev_bytes + dev_bytes / 4;
    HIP_TRY(c, hipMalloc(&c->pp_dev, cap));
    c->pp_dev_cap = cap;
  }
  if (c->pp_host_cap < host_bytes) {
    if (c->pp_host) (void)hipHostFree(c->pp_host);
    c->pp_host = nullptr; c->pp_host_cap = 0;
    const size_t cap = host_bytes + host_bytes / 4;
    HIP_TRY(c, hipHostMalloc(&c->pp_host, cap, hipHostMallocNonCoherent));
    c->pp_host_cap = cap;
  }
  return FTKX_OK;
}

// One call's place in the context's blocks.  The input block has the same shape on both sides -- records | indices | offsets | loop flags
// -- so that it goes up in one copy; the curves' part is left out where they are on the device already.
struct PpPlan {
  size_t n_rec, np, nc;
  size_t in_rec, in_indices, in_off, in_loop, in_end;       // both sides
  size_t dev_bytes, host_bytes;
  size_t h_counters, h_t, h_idx, h_type, h_poff, h_ploop, h_pcurve;
  PostProc p;                                                // device pointers, filled by bind()
  void *agg;
};

void plan_sizes(PpPlan &pl, size_t n_rec, size_t np, size_t nc)
{
  pl.n_rec = n_rec; pl.np = np; pl.nc = nc;
  PpBuffers in;
  pl.in_rec = in.take(n_rec * sizeof(PpRecord)); pl.in_indices = in.take(np * 4); pl.in_off = in.take((nc + 1) * 4); pl.in_loop = in.take(nc * 4);
  pl.in_end = in.total;
  PpBuffers h = in;
  pl.h_counters = h.take(PPC_WORDS * 4); pl.h_t = h.take(np * 8); pl.h_idx = h.take(np * 4); pl.h_type = h.take(np * 4);
  pl.h_poff = h.take((np + 1) * 4); pl.h_ploop = h.take(np * 4); pl.h_pcurve = h.take(np * 4);
  pl.host_bytes = h.total;
  // device: the input block, 9 arrays of doubles-or-less per point ... counted by bind() on a null base
  pl.dev_bytes = 0;
}

// the work arrays behind the input block; base == nullptr: only counts the bytes
void bind(PpPlan &pl, char *base)
{
  PpBuffers d;
  d.total = pl.in_end;
  const size_t np = pl.np, nc = pl.nc;
  PostProc &p = pl.p;
  auto at = [&](size_t bytes) { return base + d.take(bytes); };
  p.n_rec = (int)pl.n_rec; p.nc = (int)nc; p.np = (int)np;
  p.rec = (const PpRecord *)(base + pl.in_rec); p.indices = (const int *)(base + pl.in_indices); p.off = (const int *)(base + pl.in_off); p.loop = (const int *)(base + pl.in_loop);
  p.cid = (int *)at(np * 4); p.first = (int *)at((nc + 1) * 4);
  p.type_a = (unsigned *)at(np * 4); p.type_b = (unsigned *)at(np * 4); p.aux = (unsigned *)at(np * 4); p.t = (double *)at(np * 8);
  p.rank = (int *)at((np + 1) * 4); p.olist = (int *)at((np + 1) * 4); p.last = (int *)at((np + 1) * 4);
  p.type_r = (unsigned *)at(np * 4); p.aux_r = (unsigned *)at(np * 4); p.t_r = (double *)at(np * 8); p.idx_r = (int *)at(np * 4);
  p.type_c = (unsigned *)at(np * 4); p.aux_c = (unsigned *)at(np * 4); p.t_c = (double *)at(np * 8); p.idx_c = (int *)at(np * 4); p.pid_c = (int *)at(np * 4);
  p.poff = (int *)at((np + 1) * 4); p.ploop = (int *)at(np * 4); p.pcurve = (int *)at(np * 4);
  p.idx_o = (int *)at(np * 4); p.type_o = (unsigned *)at(np * 4); p.flag_o = (unsigned *)at(np * 4);
  p.t_o = (double *)at(np * 8); p.t_f = (double *)at(np * 8); p.t_out = (double *)at(np * 8);
  p.counters = (unsigned *)at(PPC_WORDS * 4);
  pl.agg = at(post_process_tiles(np) * kPostProcAggBytes);
  pl.dev_bytes = d.total;
}

int prepare(ftkx_ctx *c, PpPlan &pl, size_t n_rec, size_t np, size_t nc)
{
  plan_sizes(pl, n_rec, np, nc);
  bind(pl, nullptr);
  if (const int rc = ensure_pp_buffers(c, pl.dev_bytes, pl.host_bytes)) return rc;
  bind(pl, (char *)c->pp_dev);
  return FTKX_OK;
}

void pack_records(const ftkx_cp_t *recs, size_t n, PpRecord *dst)
{
  for (size_t i = 0; i < n; i ++) dst[i] = PpRecord{recs[i].type, ftkx_cp_aux(&recs[i]), recs[i].t};
}

bool phases_wanted()
{
  static const bool phases = [] { const char *e = getenv("FTKX_POST_PROCESS_PHASES"); return e && atoi(e) > 0; }();
  return phases;
}

// The kernels on what the plan holds on the device, and the trajectories down.  *declined: the gather kernel met a t that is not finite.
// orig (nullable): the device's curve k is the caller's curve orig[k] of n_orig, the others being empty (an empty curve is one empty trajectory)
int run_and_fetch(ftkx_ctx *c, PpPlan &pl, const std::vector<int> *orig, size_t n_orig, const int *orig_loop, ftkx_trajectories *out, bool *declined)
{
  const bool phases = phases_wanted();
  const auto tp0 = std::chrono::steady_clock::now();
  char *h = (char *)c->pp_host;
  unsigned *h_counters = (unsigned *)(h + pl.h_counters);
  *declined = false;
  HIP_TRY(c, hipMemsetAsync(pl.p.counters, 0, PPC_WORDS * 4, c->stream));
  HIP_TRY(c, launch_post_process(pl.p, pl.agg, c->stream, phases));
  HIP_TRY(c, hipMemcpyAsync(h_counters, pl.p.counters, PPC_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (h_counters[PPC_BAD_INDEX]) return fail(c, FTKX_E_INVALID, "ftkx_post_process_curves_device: an index outside the records");
  if (h_counters[PPC_NONFINITE]) { *declined = true; return FTKX_OK; }
  const size_t M = h_counters[PPC_POINTS], P = h_counters[PPC_PIECES];
  if (M > pl.np || P > M || P < pl.nc) return fail(c, FTKX_E_DEVICE, "ftkx_post_process_curves_device: %zu points in %zu pieces from %zu points in %zu curves", M, P, pl.np, pl.nc);
  const auto tp1 = std::chrono::steady_clock::now();
  HIP_TRY(c, hipMemcpyAsync(h + pl.h_t, pl.p.t_out, M * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + pl.h_idx, pl.p.idx_o, M * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + pl.h_type, pl.p.type_o, M * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + pl.h_poff, pl.p.poff, (P + 1) * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + pl.h_ploop, pl.p.ploop, P * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + pl.h_pcurve, pl.p.pcurve, P * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const auto tp2 = std::chrono::steady_clock::now();
  const double *h_t = (const double *)(h + pl.h_t);
  const int *h_idx = (const int *)(h + pl.h_idx), *h_poff = (const int *)(h + pl.h_poff), *h_ploop = (const int *)(h + pl.h_ploop), *h_pcurve = (const int *)(h + pl.h_pcurve);
  const unsigned *h_type = (const unsigned *)(h + pl.h_type);
  const size_t nres = orig ? P + (n_orig - orig->size()) : P;
  memset(out, 0, sizeof(*out));
  out->n_curves = nres; out->n_points = M;
  out->offsets = (long long *)malloc((nres + 1) * sizeof(long long));
  out->indices = (long long *)malloc((M ? M : 1) * sizeof(long long));
  out->loop = (int *)malloc((nres ? nres : 1) * sizeof(int));
  out->type = (unsigned *)malloc((M ? M : 1) * sizeof(unsigned));
  out->t = (double *)malloc((M ? M : 1) * sizeof(double));
  out->id = (int *)malloc((nres ? nres : 1) * sizeof(int));
  if (!out->offsets || !out->indices || !out->loop || !out->type || !out->t || !out->id) { ftkx_free_trajectories(out); return fail(c, FTKX_E_NOMEM, "ftkx_post_process_curves_device: out of memory"); }
  for (size_t k = 0; k < M; k ++) out->indices[k] = h_idx[k];
  memcpy(out->type, h_type, M * sizeof(unsigned));
  memcpy(out->t, h_t, M * sizeof(double));
  if (!orig) {
    for (size_t k = 0; k <= P; k ++) out->offsets[k] = h_poff[k];
    memcpy(out->loop, h_ploop, P * sizeof(int));
    memcpy(out->id, h_pcurve, P * sizeof(int));
  } else {
    size_t r = 0, k = 0, next = 0;                          // trajectory, piece, position in *orig
    for (size_t cu = 0; cu < n_orig; cu ++) {
      if (next < orig->size() && (size_t)(*orig)[next] == cu) {
        for (; k < P && (size_t)h_pcurve[k] == next; k ++, r ++) { out->offsets[r] = h_poff[k]; out->loop[r] = h_ploop[k]; out->id[r] = (int)cu; }
        next ++;
      } else { out->offsets[r] = k < P ? h_poff[k] : (long long)M; out->loop[r] = orig_loop[cu]; out->id[r] = (int)cu; r ++; }
    }
    out->offsets[nres] = (long long)M;
  }
  if (phases) {
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    fprintf(stderr, "ftkx_post_process_curves_device: %zu points in %zu curves -> %zu in %zu: kernels + counts %.1f us, trajectories down %.1f us, host copy %.1f us (with the waits of the phase timing)\n",
            pl.np, pl.nc, M, P, us(tp0, tp1), us(tp1, tp2), us(tp2, std::chrono::steady_clock::now()));
  }
  return FTKX_OK;
}

}  // namespace

extern "C" {

int ftkx_post_process_curves_device(ftkx_ctx *c, const ftkx_cp_t *recs, size_t n, const ftkx_curves *in, ftkx_trajectories *out)
{
  if (!c) return FTKX_E_INVALID;
  c->pp_last_path = 0;
  if (!out || !in || (n && !recs)) return fail(c, FTKX_E_INVALID, "ftkx_post_process_curves_device: bad arguments");
  memset(out, 0, sizeof(*out));
  const size_t nc = in->n_curves;
  size_t empty = 0;
  for (size_t k = 0; k < nc; k ++) {
    if (in->offsets[k] < 0 || in->offsets[k + 1] < in->offsets[k] || (size_t)in->offsets[k + 1] > in->n_points)
      return fail(c, FTKX_E_INVALID, "ftkx_post_process_curves_device: offsets that do not ascend, or run past n_points");
    empty += in->offsets[k + 1] == in->offsets[k];
  }
  auto on_host = [&](int path) {
    const int rc = ftkx_post_process_curves(recs, n, in, out);
    if (rc != FTKX_OK) return fail(c, rc, "ftkx_post_process_curves failed (%d)", rc);
    c->pp_last_path = path;
    return rc;
  };
  const size_t first = nc ? (size_t)in->offsets[0] : 0, np = nc ? (size_t)in->offsets[nc] - first : 0;
  if (np == 0) return on_host(2);                           // (nothing to do for a GPU: as many empty trajectories as there are curves)
  if (np >= (1u << 30) || n >= (1ull << 31)) return on_host(0);
  const auto tp0 = std::chrono::steady_clock::now();
  HIP_TRY(c, hipSetDevice(c->device));
  PpPlan pl;
  if (const int rc = prepare(c, pl, n, np, nc - empty)) return rc;
  char *h = (char *)c->pp_host;
  int *h_indices = (int *)(h + pl.in_indices), *h_off = (int *)(h + pl.in_off), *h_loop = (int *)(h + pl.in_loop);
  for (size_t k = 0; k < np; k ++) {
    const long long i = in->indices[first + k];
    if (i < 0 || (size_t)i >= n) return fail(c, FTKX_E_INVALID, "ftkx_post_process_curves_device: an index outside the records");
    h_indices[k] = (int)i;
  }
  std::vector<int> orig;                                    // only where some curve is empty
  if (empty) orig.reserve(nc - empty);
  size_t m = 0;
  for (size_t k = 0; k < nc; k ++) {
    if (in->offsets[k + 1] == in->offsets[k]) continue;
    h_off[m] = (int)((size_t)in->offsets[k] - first); h_loop[m] = in->loop[k];
    if (empty) orig.push_back((int)k);
    m ++;
  }
  h_off[m] = (int)np;
  pack_records(recs, n, (PpRecord *)(h + pl.in_rec));
  HIP_TRY(c, hipMemcpyAsync(c->pp_dev, c->pp_host, pl.in_end, hipMemcpyHostToDevice, c->stream));
  if (phases_wanted()) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    fprintf(stderr, "ftkx_post_process_curves_device: %-32s %8.1f us\n", "checks, staging, upload", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tp0).count());
  }
  bool declined = false;
  if (const int rc = run_and_fetch(c, pl, empty ? &orig : nullptr, nc, in->loop, out, &declined)) return rc;
  if (declined) return on_host(0);
  c->pp_last_path = 2;
  return FTKX_OK;
}

int ftkx_pass2_device(ftkx_ctx *c, int nd, const long long domain_st[3], const long long domain_sz[3], const ftkx_cp_t *recs, size_t n, ftkx_curves *curves, ftkx_trajectories *out)
{
  if (!c) return FTKX_E_INVALID;
  c->pp_last_path = 0;
  if (!out || (n && !recs)) return fail(c, FTKX_E_INVALID, "ftkx_pass2_device: bad arguments");
  memset(out, 0, sizeof(*out));
  if (curves) memset(curves, 0, sizeof(*curves));
  // the records' 16 bytes go up first: the copy runs while the host prepares the trace
  const bool fits = n > 0 && n < (1u << 30);
  PpPlan pl;
  if (fits) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = prepare(c, pl, n, n, n)) return rc;   // (points and curves: at most one per record)
    pack_records(recs, n, (PpRecord *)((char *)c->pp_host + pl.in_rec));
    HIP_TRY(c, hipMemcpyAsync((char *)c->pp_dev + pl.in_rec, (char *)c->pp_host + pl.in_rec, n * sizeof(PpRecord), hipMemcpyHostToDevice, c->stream));
  }
  std::vector<unsigned long long> tags(n);
  for (size_t i = 0; i < n; i ++) tags[i] = recs[i].tag;
  ftkx_curves cur;
  memset(&cur, 0, sizeof(cur));
  int rc = ftkx_trace_curves_device(c, nd, domain_st, domain_sz, tags.data(), n, 0, &cur);
  if (rc != FTKX_OK) { ftkx_free_curves(&cur); return rc; }
  bool declined = true;
  if (fits && c->tr_last_path == 2 && cur.n_points > 0) {
    // the curves where the trace's scatter kernel left them
    const size_t np = cur.n_points, nc = cur.n_curves;
    plan_sizes(pl, n, np, nc);
    bind(pl, (char *)c->pp_dev);                             // (no larger than what was prepared)
    trace_device_curves(c, &pl.p.indices, &pl.p.off, &pl.p.loop);
    rc = run_and_fetch(c, pl, nullptr, nc, nullptr, out, &declined);
    if (rc == FTKX_OK && !declined) c->pp_last_path = 2;
  }
  if (rc == FTKX_OK && declined) {
    rc = ftkx_post_process_curves(recs, n, &cur, out);
    if (rc != FTKX_OK) rc = fail(c, rc, "ftkx_post_process_curves failed (%d)", rc);
    else if (cur.n_points == 0 && c->tr_last_path == 2) c->pp_last_path = 2;
  }
  if (curves && rc == FTKX_OK) *curves = cur; else ftkx_free_curves(&cur);
  return rc;
}

int ftkx_post_process_last_path(const ftkx_ctx *c) { return c ? c->pp_last_path : 0; }

}  // extern "C"
