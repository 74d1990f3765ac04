// Pass 2, its second half on the device: ftkx_post_process_curves_device and, with the trace in front of it, ftkx_pass2_device.
//
// ftkx_post_process_curves (trace.cpp) hands the traced curves to host threads one by one.  Every step of it -- smoothing the types along
// the ordinal points and across the gaps between them, rotating loops, split_all, re-ordering in time, adjust_time -- is a map or a scan
// over the flat array of points with the curves' heads as borders (post_process_steps.hpp), and the only floating-point operations are
// max and min: the kernels of post_process_kernels.hip give the same trajectories bit for bit.  Up go 16 bytes per record (type, aux
// word, t) and, where the curves are not on the device already, 4 bytes per point and 8 per curve; the host waits once for the counts of
// pieces and points, then once for the trajectories: 16 bytes per point, 12 per piece.  After ftkx_trace_curves_device the curves lie in
// the context's ordering buffers (indices, offsets, loop flags): ftkx_pass2_device reads them there.
#include "ctx.hpp"

using namespace ftkxh;
using namespace ftkx;

namespace {

const char *const kName = "ftkx_post_process_curves_device";

PpPlan plan_of(size_t n_rec, size_t np, size_t nc) { return PpPlan(n_rec, np, nc, post_process_tiles(np) * kPostProcAggBytes); }

// the context's blocks for the plan, and its work arrays bound to the device block
int prepare(ftkx_ctx *c, PpPlan &pl)
{
  if (const int rc = c->p2.pp_dev.reserve(c, pl.dev_bytes, pass2_room(pl.dev_bytes))) return rc;
  if (const int rc = c->p2.pp_host.reserve(c, pl.host_bytes, pass2_room(pl.host_bytes))) return rc;
  pl.bind(c->p2.pp_dev.p);
  return FTKX_OK;
}

void pack_records(const ftkx_cp_t *recs, size_t n, PpRecord *dst)
{
  for (size_t i = 0; i < n; i ++) dst[i] = PpRecord{recs[i].type, ftkx_cp_aux(&recs[i]), recs[i].t};
}

// FTKX_POST_PROCESS_PHASES=1: the host waits after every phase and prints its time
ftkx_phase_clock phase_clock(const ftkx_ctx *c)
{
  static const bool phases = [] { const char *e = getenv("FTKX_POST_PROCESS_PHASES"); return e && atoi(e) > 0; }();
  return ftkx_phase_clock{phases, c->stream, kName};
}

// The kernels on what the plan holds on the device, and the trajectories down.  *declined: the gather kernel met a t that is not finite.
// orig (nullable): the device's curve k is the caller's curve orig[k] of n_orig, the others being empty (an empty curve is one empty trajectory)
int run_and_fetch(ftkx_ctx *c, PpPlan &pl, ftkx_phase_clock &clock, const std::vector<int> *orig, size_t n_orig, const int *orig_loop, ftkx_trajectories *out, bool *declined)
{
  void *h = c->p2.pp_host.p;
  unsigned *h_counters = pl.h_counters.in<unsigned>(h);
  *declined = false;
  HIP_TRY(c, hipMemsetAsync(pl.p.counters, 0, PPC_WORDS * 4, c->stream));
  HIP_TRY(c, launch_post_process(pl.p, pl.agg, clock));
  HIP_TRY(c, hipMemcpyAsync(h_counters, pl.p.counters, PPC_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (h_counters[PPC_BAD_INDEX]) return fail(c, FTKX_E_INVALID, "ftkx_post_process_curves_device: an index outside the records");
  if (h_counters[PPC_NONFINITE]) { *declined = true; return FTKX_OK; }
  const size_t M = h_counters[PPC_POINTS], P = h_counters[PPC_PIECES];
  if (M > pl.np || P > M || P < pl.nc) return fail(c, FTKX_E_DEVICE, "ftkx_post_process_curves_device: %zu points in %zu pieces from %zu points in %zu curves", M, P, pl.np, pl.nc);
  HIP_TRY(c, clock.lap("counts down", P));
  double *h_t = pl.h_t.in<double>(h);
  int *h_idx = pl.h_idx.in<int>(h), *h_poff = pl.h_poff.in<int>(h), *h_ploop = pl.h_ploop.in<int>(h), *h_pcurve = pl.h_pcurve.in<int>(h);
  unsigned *h_type = pl.h_type.in<unsigned>(h);
  HIP_TRY(c, hipMemcpyAsync(h_t, pl.p.t_out, M * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h_idx, pl.p.idx_o, M * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h_type, pl.p.type_o, M * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h_poff, pl.p.poff, (P + 1) * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h_ploop, pl.p.ploop, P * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h_pcurve, pl.p.pcurve, P * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, clock.lap("trajectories down", M));
  const size_t nres = orig ? P + (n_orig - orig->size()) : P;
  if (const int rc = alloc_trajectories(out, nres, M)) return fail(c, rc, "ftkx_post_process_curves_device: out of memory");
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
  if (const hipError_t waited = clock.lap("host copy", M)) { ftkx_free_trajectories(out); HIP_TRY(c, waited); }
  if (clock.on) fprintf(stderr, "%s: %zu points in %zu curves -> %zu in %zu: %.1f us in all (with the waits of the phase timing)\n", kName, pl.np, pl.nc, M, P, clock.us_in_all());
  return FTKX_OK;
}

}  // namespace

extern "C" {

int ftkx_post_process_curves_device(ftkx_ctx *c, const ftkx_cp_t *recs, size_t n, const ftkx_curves *in, ftkx_trajectories *out)
{
  if (!c) return FTKX_E_INVALID;
  c->p2.pp_last_path = 0;
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
    c->p2.pp_last_path = path;
    return rc;
  };
  const size_t first = nc ? (size_t)in->offsets[0] : 0, np = nc ? (size_t)in->offsets[nc] - first : 0;
  if (np == 0) return on_host(2);                           // (nothing to do for a GPU: as many empty trajectories as there are curves)
  if (np >= (1u << 30) || n >= (1ull << 31)) return on_host(0);
  ftkx_phase_clock clock = phase_clock(c);
  clock.start();
  HIP_TRY(c, hipSetDevice(c->device));
  PpPlan pl = plan_of(n, np, nc - empty);
  if (const int rc = prepare(c, pl)) return rc;
  void *h = c->p2.pp_host.p;
  int *h_indices = pl.in_indices.in<int>(h), *h_off = pl.in_off.in<int>(h), *h_loop = pl.in_loop.in<int>(h);
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
  pack_records(recs, n, pl.in_rec.in<PpRecord>(h));
  HIP_TRY(c, hipMemcpyAsync(c->p2.pp_dev.p, h, pl.in_end, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, clock.lap("checks, staging, upload", np));
  bool declined = false;
  if (const int rc = run_and_fetch(c, pl, clock, empty ? &orig : nullptr, nc, in->loop, out, &declined)) return rc;
  if (declined) return on_host(0);
  c->p2.pp_last_path = 2;
  return FTKX_OK;
}

int ftkx_pass2_device(ftkx_ctx *c, int nd, const long long domain_st[3], const long long domain_sz[3], const ftkx_cp_t *recs, size_t n, ftkx_curves *curves, ftkx_trajectories *out)
{
  if (!c) return FTKX_E_INVALID;
  c->p2.pp_last_path = 0;
  if (!out || (n && !recs)) return fail(c, FTKX_E_INVALID, "ftkx_pass2_device: bad arguments");
  memset(out, 0, sizeof(*out));
  if (curves) memset(curves, 0, sizeof(*curves));
  // the records' 16 bytes go up first: the copy runs while the host prepares the trace
  const bool fits = n > 0 && n < (1u << 30);
  ftkx_phase_clock clock = phase_clock(c);
  clock.start();
  if (fits) {
    HIP_TRY(c, hipSetDevice(c->device));
    PpPlan pl = plan_of(n, n, n);                            // (points and curves: at most one per record)
    if (const int rc = prepare(c, pl)) return rc;
    PpRecord *h_rec = pl.in_rec.in<PpRecord>(c->p2.pp_host.p);
    pack_records(recs, n, h_rec);
    HIP_TRY(c, hipMemcpyAsync(pl.in_rec.in<PpRecord>(c->p2.pp_dev.p), h_rec, n * sizeof(PpRecord), hipMemcpyHostToDevice, c->stream));
  }
  std::vector<unsigned long long> tags(n);
  for (size_t i = 0; i < n; i ++) tags[i] = recs[i].tag;
  ftkx_curves cur;
  memset(&cur, 0, sizeof(cur));
  int rc = ftkx_trace_curves_device(c, nd, domain_st, domain_sz, tags.data(), n, 0, &cur);
  if (rc != FTKX_OK) { ftkx_free_curves(&cur); return rc; }
  bool declined = true;
  if (fits && c->p2.trace_last_path == 2 && cur.n_points > 0) {
    // the curves where the trace's scatter kernel left them
    const size_t np = cur.n_points, nc = cur.n_curves;
    PpPlan pl = plan_of(n, np, nc);
    pl.bind(c->p2.pp_dev.p);                                 // (no larger than what was prepared: the records lie where they went up)
    trace_device_curves(c, &pl.p.indices, &pl.p.off, &pl.p.loop);
    const hipError_t waited = clock.lap("records up, trace", n);
    rc = waited == hipSuccess ? run_and_fetch(c, pl, clock, nullptr, nc, nullptr, out, &declined) : fail(c, FTKX_E_DEVICE, "ftkx_pass2_device: %s", hipGetErrorString(waited));
    if (rc == FTKX_OK && !declined) c->p2.pp_last_path = 2;
  }
  if (rc == FTKX_OK && declined) {
    rc = ftkx_post_process_curves(recs, n, &cur, out);
    if (rc != FTKX_OK) rc = fail(c, rc, "ftkx_post_process_curves failed (%d)", rc);
    else if (cur.n_points == 0 && c->p2.trace_last_path == 2) c->p2.pp_last_path = 2;
  }
  if (curves && rc == FTKX_OK) *curves = cur; else ftkx_free_curves(&cur);
  return rc;
}

int ftkx_post_process_last_path(const ftkx_ctx *c) { return c ? c->p2.pp_last_path : 0; }

}  // extern "C"
