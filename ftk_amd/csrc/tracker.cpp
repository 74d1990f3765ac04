// Host-side tracker with the reference's operator interface (include/ftkx_tracker.hh).  Pure host logic over the C ABI:
// snapshot window, sticky quantisation factor, ordinal + interval sweep per step, record bookkeeping.
// Reference counterparts are cited per method.
#include "../../include/ftkx_tracker.hh"
#include "host_sort.hpp"

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <set>
#include <thread>

namespace ftkx {

namespace {
// the writer of what ftkx_cp_ordinal / ftkx_cp_timestep (include/ftkx.h) read: bit 0 = ordinal, bits 1..31 = the timestep
void set_cp_aux(ftkx_cp_t &r, int timestep, bool ordinal) { reinterpret_cast<unsigned int *>(&r)[15] = ((unsigned)timestep << 1) | (ordinal ? 1u : 0u); }
ftkx_cp_t record_of(const feature_point_t &cp)
{
  ftkx_cp_t r;
  std::memset(&r, 0, sizeof(r));
  for (int k = 0; k < 3; k ++) { r.x[k] = cp.x[k]; r.scalar[k] = cp.scalar[k]; }
  r.t = cp.t; r.type = cp.type; r.tag = cp.tag;
  set_cp_aux(r, cp.timestep, cp.ordinal);
  return r;
}
feature_point_t point_of(const ftkx_cp_t &r)
{
  feature_point_t cp;
  for (int k = 0; k < 3; k ++) { cp.x[k] = r.x[k]; cp.scalar[k] = r.scalar[k]; }
  cp.t = r.t; cp.type = r.type; cp.tag = r.tag;
  cp.ordinal = ftkx_cp_ordinal(&r) != 0; cp.timestep = ftkx_cp_timestep(&r);
  return cp;
}

// a failed call of the C ABI -> ftkx_error with the context's message (c == nullptr: the calling thread's last error)
ftkx_error last_error_of(const ftkx_ctx *c, int rc) { char buf[512] = ""; ftkx_last_error(c, buf, sizeof(buf)); return ftkx_error(rc, buf); }
[[noreturn]] void throw_last(const ftkx_ctx *c, int rc) { throw last_error_of(c, rc); }
void check_on(const ftkx_ctx *c, int rc) { if (rc != FTKX_OK) throw_last(c, rc); }
void check_slab(const ftkx_slab *s, int rc) { if (rc != FTKX_OK) throw ftkx_error(rc, ftkx_slab_last_error(s)); }

ftkx_ctx *create_context(int nd, int device_id)
{
  ftkx_ctx *c = nullptr;
  check_on(nullptr, ftkx_create(&c, nd, device_id));   // no device, no tracker: there is no CPU path behind this class
  return c;
}

// critical_point_tracker.hh:857-863: the quantisation factor that belongs to a running minimum of ndarray::resolution()
unsigned long long factor_of(double resolution, int minbits, int maxbits)
{
  const int nbits = (int)std::ceil(std::log2(1.0 / resolution));
  return 1ull << std::max(minbits, std::min(nbits, maxbits));
}

// one snapshot -> one context.  kind: 0 scalar (V derived), 1 vector, 2 all three given; dtype: the arrays' element type, FTKX_DTYPE_*
// (everything but FP64 is widened on the device; the typed entries hand FP64 and float32 to the entries they always took);
// planes (kind 1; FP64 or float32): v is an array of that many pointers, one per component (interleaved on the device)
int push_to(ftkx_ctx *c, int kind, int t, const void *s, const void *v, const void *j, int on_device, int dtype = FTKX_DTYPE_F64, int planes = 0)
{
  if (planes) {
    if (dtype == FTKX_DTYPE_F32) return ftkx_push_slice_planar_f32(c, t, static_cast<const float *const *>(v), planes, nullptr, nullptr, on_device);
    return ftkx_push_slice_planar(c, t, static_cast<const double *const *>(v), planes, nullptr, nullptr, on_device);
  }
  if (kind == 0) return ftkx_push_scalar_slice_typed(c, t, s, dtype, on_device);
  if (kind == 1) return ftkx_push_slice_typed(c, t, v, nullptr, nullptr, dtype, on_device);
  return ftkx_push_slice_typed(c, t, v, j, s, dtype, on_device);
}
}  // namespace

// ---- several devices behind one tracker ---------------------------------------------------------------------------------------
struct critical_point_tracker_regular::multi_engine {
  struct worker {
    ftkx_ctx *ctx = nullptr;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::function<void()>> q;
    bool stop = false, busy = false;
    unsigned long long posted = 0, done = 0;     // jobs handed in / finished (FIFO: `done >= ticket` says a particular job is through)
    ~worker() { ftkx_destroy(ctx); }
  };
  // what one step hands back to the tracker (the records are the context's: valid while `deliver` runs)
  struct step_result {
    int t = 0;
    double resolution = 0;                     // the running minimum at this step, and the factor it gives
    unsigned long long factor = 0;
    const ftkx_cp_t *recs = nullptr; size_t n = 0;
    ftkx_stats stats;
  };
  std::vector<std::unique_ptr<worker>> w;
  int block = 2, t_first = -1;
  std::map<int, std::set<int>> resident;       // timestep -> workers that hold the slice
  // the reduction board: what each slice contributes to the sticky running minimum, published by whichever step reduces it first
  std::mutex bmu;
  std::condition_variable bcv;
  std::map<int, double> res_below;
  double base_resolution = std::numeric_limits<double>::max();   // the running minimum before this series (never reset, like the reference's)
  // errors raised inside jobs surface at the next sync()
  std::mutex emu;
  int error_code = 0;
  std::string error;
  std::mutex rmu;                              // held while a step's result is delivered: the jobs of several devices finish at the same time

  multi_engine(int nd, const std::vector<int> &device_ids, int block_) : block(block_)
  {
    for (int dev : device_ids) { w.emplace_back(new worker()); w.back()->ctx = create_context(nd, dev); }
    for (auto &W : w) { worker *wp = W.get(); W->th = std::thread([this, wp] { run(wp); }); }
  }

  int dev_of(int t) const { return ((t - t_first) / block) % (int)w.size(); }

  void run(worker *W)
  {
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> lk(W->mu);
        W->cv.wait(lk, [&] { return W->stop || !W->q.empty(); });
        if (W->q.empty()) return;
        f = std::move(W->q.front()); W->q.pop_front(); W->busy = true;
      }
      try { f(); }
      catch (const ftkx_error &e) { raise(e.code, e.what()); }
      catch (const std::exception &e) { raise(FTKX_E_INVALID, e.what()); }
      { std::lock_guard<std::mutex> lk(W->mu); W->busy = false; W->done ++; }
      W->cv.notify_all();
    }
  }
  // A failing job wakes every step that waits on the board.  The error is set under emu, the notify goes out under bmu: a waiter that
  // has evaluated its predicate (failed() == false) and not yet blocked holds bmu, so the notify cannot fall into that gap.
  void raise(int code, const char *what)
  {
    { std::lock_guard<std::mutex> g(emu); if (!error_code) { error_code = code; error = what; } }
    { std::lock_guard<std::mutex> g(bmu); }
    bcv.notify_all();
  }
  unsigned long long post(int d, std::function<void()> f)
  {
    unsigned long long ticket;
    { std::lock_guard<std::mutex> lk(w[d]->mu); w[d]->q.push_back(std::move(f)); ticket = ++ w[d]->posted; }
    w[d]->cv.notify_all();
    return ticket;
  }
  // waits for ONE job (its ticket), not for the device's queue to drain: a push only has to know that its own copy is through, while the
  // sweeps queued behind it on that device run on
  void wait_job(int d, unsigned long long ticket)
  {
    std::unique_lock<std::mutex> lk(w[d]->mu);
    w[d]->cv.wait(lk, [&] { return w[d]->done >= ticket; });
  }
  void wait_all()
  {
    for (auto &W : w) { std::unique_lock<std::mutex> lk(W->mu); W->cv.wait(lk, [&] { return W->q.empty() && !W->busy; }); }
  }
  bool failed() { std::lock_guard<std::mutex> g(emu); return error_code != 0; }
  void rethrow()
  {
    std::lock_guard<std::mutex> g(emu);
    if (error_code) { const int c = error_code; const std::string m = error; error_code = 0; error.clear(); throw ftkx_error(c, m); }
  }
  // running minimum over what has been published of the slices BEFORE t (any subset of them bounds the factor from below)
  double known_before(int t)
  {
    std::lock_guard<std::mutex> g(bmu);
    double r = base_resolution;
    for (const auto &kv : res_below) if (kv.first < t) r = std::min(r, kv.second);
    return r;
  }
  void publish(const std::vector<int> &ts, const std::vector<double> &below)
  {
    {
      std::lock_guard<std::mutex> g(bmu);
      for (size_t i = 0; i < ts.size(); i ++) {
        auto it = res_below.find(ts[i]);
        if (it == res_below.end()) res_below[ts[i]] = below[i]; else it->second = std::min(it->second, below[i]);
      }
    }
    bcv.notify_all();
  }
  // the reference's vector_field_resolution at the step whose last snapshot is t_last: needs every slice up to it
  double wait_running_min(int t_last)
  {
    std::unique_lock<std::mutex> lk(bmu);
    bcv.wait(lk, [&] {
      if (failed()) return true;
      for (int s = t_first; s <= t_last; s ++) if (!res_below.count(s)) return false;
      return true;
    });
    double r = base_resolution;
    for (int s = t_first; s <= t_last; s ++) { auto it = res_below.find(s); if (it != res_below.end()) r = std::min(r, it->second); }
    return r;
  }

  // one snapshot -> the devices whose steps read it; returns when the caller's buffer is free again
  void push(int kind, int t, const double *s, const double *v, const double *j, bool device)
  {
    if (t_first < 0) t_first = t;
    std::set<int> targets;
    targets.insert(dev_of(t));
    if (t > t_first) targets.insert(dev_of(t - 1));        // the interval sweep [t-1, t] of the previous block reads it too
    // Device memory is COPIED into each context (a peer copy where the devices differ; the contexts recycle their slice buffers, so
    // no allocation per step): the steps run later than the calls that queue them, and the caller's buffer is free again on return
    // -- adopting the pointer would tie its lifetime to a queue the caller cannot see.
    std::vector<std::pair<int, unsigned long long>> tickets;
    for (int d : targets) {
      ftkx_ctx *c = w[d]->ctx;
      tickets.push_back({d, post(d, [=] { check_on(c, push_to(c, kind, t, s, v, j, device ? 2 : 0)); })});
    }
    for (const auto &tk : tickets) wait_job(tk.first, tk.second);     // (the caller's buffer is free again once these copies are through)
    rethrow();
    resident[t] = targets;
  }
  // the slice of timestep t leaves every device that holds it: queued behind the steps that still read it
  void drop(int t)
  {
    for (int d : resident[t]) {
      ftkx_ctx *c = w[d]->ctx;
      post(d, [=] { check_on(c, ftkx_drop_slice(c, t)); });
    }
    resident.erase(t);
  }
  // The step of timestep t over the slices `ts` is queued on the device that owns t, and this call returns.  Inside the job: reduce
  // (and mask) the step's slices under the factor known so far, publish their contribution, wait for the contributions of ALL
  // earlier slices -- other devices publish theirs before they sweep, so this is a wait for reductions only -- and sweep under
  // the factor the reference would have at this step.  `deliver(const step_result &)` runs on the device's thread, under rmu.
  template <class Deliver>
  void step(int t, int scope, const std::vector<int> &ts, int minbits, int maxbits, Deliver deliver)
  {
    rethrow();
    ftkx_ctx *c = w[dev_of(t)]->ctx;
    post(dev_of(t), [this, c, t, scope, ts, minbits, maxbits, deliver] {
      std::vector<double> below(ts.size());
      check_on(c, ftkx_sweep_announce(c, &t, &scope, 1));
      check_on(c, ftkx_slices_prepare(c, ts.data(), (int)ts.size(), factor_of(known_before(t), minbits, maxbits), below.data(), nullptr));
      publish(ts, below);
      step_result r;
      r.t = t;
      r.resolution = wait_running_min(ts.back());
      if (failed()) return;                     // another step failed: do not sweep with a partial minimum
      r.factor = factor_of(r.resolution, minbits, maxbits);
      check_on(c, ftkx_sweep(c, t, scope, r.factor, &r.recs, &r.n));
      check_on(c, ftkx_get_stats(c, &r.stats));
      std::lock_guard<std::mutex> g(rmu);
      deliver(r);
    });
  }
  void settle() { wait_all(); rethrow(); }
  // a new series: the board is empty again, and what the last series reduced stays in force (the running minimum is sticky)
  void restart(double resolution) { base_resolution = resolution; res_below.clear(); t_first = -1; }

  ~multi_engine()      // (the workers' destructors then destroy the contexts)
  {
    for (auto &W : w) { { std::lock_guard<std::mutex> lk(W->mu); W->stop = true; } W->cv.notify_all(); }
    for (auto &W : w) if (W->th.joinable()) W->th.join();
  }
};

critical_point_tracker_regular::critical_point_tracker_regular(int nd_, int device_id) : critical_point_tracker_regular(nd_, std::vector<int>(1, device_id)) {}

critical_point_tracker_regular::critical_point_tracker_regular(int nd_, const std::vector<int> &device_ids, int block) : nd(nd_)
{
  std::memset(&last_stats, 0, sizeof(last_stats));
  if (device_ids.empty() || block < 1) throw ftkx_error(FTKX_E_INVALID, "critical_point_tracker_regular: need at least one device and block >= 1");
  if (device_ids.size() == 1) { ctx = create_context(nd, device_ids[0]); return; }
  multi.reset(new multi_engine(nd, device_ids, block));
  ctx = multi->w[0]->ctx;     // (context() of a multi-device tracker: its first device's)
}

critical_point_tracker_regular::~critical_point_tracker_regular()
{
  ftkx_online_tracer_destroy(online);
  if (slab) ftkx_slab_destroy(slab);
  if (multi) multi.reset();   // joins the workers, destroys their contexts (ctx is one of them)
  else ftkx_destroy(ctx);
}

// ---- several ranks behind the tracker: slab mode -----------------------------------------------------------------------------------------
void critical_point_tracker_regular::enter_slab_mode(int rank, int nranks, int nt)
{
  if (multi) throw ftkx_error(FTKX_E_UNSUPPORTED, "slab mode: a tracker with one device (several devices of one process: one tracker per device over a ftkx_slab_hub)");
  if (slab || !field_data_snapshots.empty()) throw ftkx_error(FTKX_E_INVALID, "slab mode: set it once, before the first snapshot is pushed");
  if (enable_streaming_trajectories) throw ftkx_error(FTKX_E_UNSUPPORTED, "slab mode: not with streaming trajectories");
  if (temporal_smoothing_ksize) throw ftkx_error(FTKX_E_UNSUPPORTED, "slab mode: not with temporal smoothing (a slab needs raw halo snapshots of its neighbours)");
  if (nt <= 0 || nranks <= 0 || rank < 0 || rank >= nranks) throw ftkx_error(FTKX_E_INVALID, "slab mode: bad rank / nranks / nt");
  slab_rank = rank;
  ftkx_slab_range(nt, nranks, rank, &slab_t0, &slab_t1);
  restart_slab();
}

// the first snapshot this rank pushes is its slab's first timestep; nothing recorded, nothing swept
void critical_point_tracker_regular::restart_slab() { current_timestep = next_push_timestep = slab_t0; slab_steps.clear(); slab_swept = false; }

void critical_point_tracker_regular::set_communicator(void *comm, int rank, int nranks, int nt)
{
  enter_slab_mode(rank, nranks, nt);
  check(ftkx_slab_create_rccl(ctx, nt, rank, nranks, comm, nullptr, &slab));
}

void critical_point_tracker_regular::set_slab_transport(const ftkx_slab_transport &tr, int rank, int nranks, int nt)
{
  enter_slab_mode(rank, nranks, nt);
  check(ftkx_slab_create(ctx, nt, rank, nranks, &tr, &slab));
}

void critical_point_tracker_regular::set_slab_hub(ftkx_slab_hub *hub, int rank, int nt)
{
  if (!hub) throw ftkx_error(FTKX_E_INVALID, "set_slab_hub: null hub");
  ftkx_slab *probe = nullptr;
  // (the hub knows how many ranks it has: the slab says so)
  check(ftkx_slab_create_local(ctx, nt, rank, hub, &probe));
  ftkx_slab_info info;
  ftkx_slab_get_info(probe, &info);
  try { enter_slab_mode(rank, info.nranks, nt); } catch (...) { ftkx_slab_destroy(probe); throw; }
  slab = probe;
}

// slab mode: the step is recorded; the slab is swept as one pass (run_slab)
void critical_point_tracker_regular::step_slab()
{
  if (slab_swept) throw ftkx_error(FTKX_E_INVALID, "slab mode: the slab has been swept (reset() starts a new series)");
  if (slab_steps.empty() || slab_steps.back() != current_timestep) slab_steps.push_back(current_timestep);
}

// the slab's pass: every step recorded so far must be the slab's -- t0 .. t1 - 1 in order -- and every snapshot still resident
void critical_point_tracker_regular::run_slab()
{
  const int nown = slab_t1 - slab_t0;
  if ((int)slab_steps.size() != nown || (int)field_data_snapshots.size() != nown)
    throw ftkx_error(FTKX_E_INVALID, "slab mode: " + std::to_string(slab_steps.size()) + " steps recorded and " + std::to_string(field_data_snapshots.size()) +
                     " snapshots pushed of this rank's " + std::to_string(nown) + " (push the slab's snapshots, advance_timestep() between them, update_timestep() after the last)");
  for (int i = 0; i < nown; i ++) if (slab_steps[(size_t)i] != slab_t0 + i) throw ftkx_error(FTKX_E_INVALID, "slab mode: the steps must be the slab's timesteps in order");
  check_slab(slab, ftkx_slab_submit(slab, &vector_field_resolution));
  std::vector<unsigned long long> f((size_t)std::max(nown, 1), 0ull);
  const ftkx_cp_t *recs = nullptr;
  size_t n = 0;
  double run = vector_field_resolution;
  check_slab(slab, ftkx_slab_complete(slab, &run, f.data(), &recs, &n));
  slab_swept = true;
  if (nown > 0) {
    vector_field_resolution = std::min(vector_field_resolution, run);
    vector_field_scaling_factor = f[(size_t)nown - 1];
    take_records_by_step(recs, n);
    check(ftkx_get_stats(ctx, &last_stats));
  }
}

// what is still out comes in: the slab's pass, the queues of several devices, the deferred sweeps
void critical_point_tracker_regular::wait_devices()
{
  if (slab) { if (!slab_swept) run_slab(); return; }
  if (multi) multi->settle();
  collect_deferred();
}

void critical_point_tracker_regular::collect_deferred()
{
  if (!batch_ts.empty()) submit_batch();                       // deferred collection in batches: the steps recorded since the last full batch
  while (!open_steps.empty()) collect_open_step();             // deferred collection: what is still out
}

// deferred collection: the oldest queued sweep -> its records, factor, running minimum and statistics, as update_timestep leaves them
void critical_point_tracker_regular::collect_open_step()
{
  const int t = open_steps.front();
  open_steps.erase(open_steps.begin());
  const ftkx_cp_t *recs = nullptr;
  size_t n = 0;
  unsigned long long f = 0;
  double res = vector_field_resolution;
  const int rc = ftkx_sweep_series_complete(ctx, &res, &f, &recs, &n);
  if (rc != FTKX_OK) {
    // the other open pass (if any) is discarded with it: the context is left as if nothing had been queued, so that the tracker's later
    // calls do not fail with "passes open" or chain from a stale running minimum
    const ftkx_error why = last_error_of(ctx, rc);
    open_steps.clear();
    (void)ftkx_sweep_series_abort(ctx);
    batch_ts.clear(); batch_scopes.clear();
    for (int d : batch_drops) (void)ftkx_drop_slice(ctx, d);
    batch_drops.clear();
    throw why;
  }
  vector_field_resolution = res;
  vector_field_scaling_factor = f;
  if (t >= 0) take_records(recs, n, t);
  else take_records_by_step(recs, n);                            // a batch: its steps' records, ordered by tag, not by step
  check(ftkx_get_stats(ctx, &last_stats));
}

// deferred collection in batches: the recorded steps as one pass (continuing, on the device, from the pass queued before it if that one is
// still out); the snapshots popped since the batch began are dropped behind it -- their buffers are reused in stream order
void critical_point_tracker_regular::submit_batch()
{
  const bool chained = !open_steps.empty();
  std::vector<int> ts, scopes, drops;
  ts.swap(batch_ts); scopes.swap(batch_scopes); drops.swap(batch_drops);
  int rc = ftkx_sweep_series_submit(ctx, ts.data(), scopes.data(), (int)ts.size(), chained ? nullptr : &vector_field_resolution);
  if (rc == FTKX_OK) open_steps.push_back(-1);
  for (int t : drops) { const int rc2 = ftkx_drop_slice(ctx, t); if (rc == FTKX_OK) rc = rc2; }
  check(rc);
  if (open_steps.size() >= 3) collect_open_step();      // (three in flight: the host runs one pass ahead of a split pass's tail)
}

void critical_point_tracker_regular::sync() const
{
  const_cast<critical_point_tracker_regular *>(this)->wait_devices();   // (a getter is const; bringing in what is still out is not)
  flush_points();
}

// the parked records into the flat store: ordered by the element order's integer key, merged with what is there (a later point with
// the same tag replaces the earlier one, like operator[] of the reference's map)
void critical_point_tracker_regular::flush_points() const
{
  if (pending_points.empty()) return;
  typedef std::pair<std::pair<unsigned long long, unsigned long long>, size_t> keyed;
  std::vector<keyed> order(pending_points.size());
  for (size_t i = 0; i < pending_points.size(); i ++) order[i] = {order_.key(pending_points[i].tag), i};
  ftkx::sort_on_threads(order);                                  // (equal keys = equal tags: their insertion order, the index, breaks the tie)
  std::vector<feature_point_t> merged;
  std::vector<std::pair<unsigned long long, unsigned long long>> keys;
  merged.reserve(points.size() + order.size()); keys.reserve(points.size() + order.size());
  size_t a = 0, b = 0;
  while (a < points.size() || b < order.size()) {
    if (b < order.size() && b + 1 < order.size() && order[b + 1].first == order[b].first) { b ++; continue; }   // the later of two pending points with one tag
    if (b == order.size() || (a < points.size() && point_keys[a] < order[b].first)) { merged.push_back(points[a]); keys.push_back(point_keys[a]); a ++; }
    else {
      if (a < points.size() && point_keys[a] == order[b].first) a ++;                                            // replaced
      merged.push_back(pending_points[order[b].second]); keys.push_back(order[b].first); b ++;
    }
  }
  points.swap(merged); point_keys.swap(keys);
  pending_points.clear();
  pending_ascending = true;
  map_valid = false;
}

const discrete_map_t &critical_point_tracker_regular::get_discrete_critical_points() const
{
  sync();
  if (!map_valid) {
    discrete_map_t fresh(order_);
    for (const feature_point_t &cp : points) fresh.emplace_hint(fresh.end(), cp.tag, cp);     // (already in the map's order: linear)
    discrete_critical_points.swap(fresh);
    map_valid = true;
  }
  return discrete_critical_points;
}

int critical_point_tracker_regular::num_devices() const { return multi ? (int)multi->w.size() : 1; }

void critical_point_tracker_regular::check(int rc) const { check_on(ctx, rc); }

void critical_point_tracker_regular::set_stream(void *s)
{
  if (multi) throw ftkx_error(FTKX_E_UNSUPPORTED, "set_stream: a multi-device tracker runs each device on its context's own stream");
  check(ftkx_set_stream(ctx, s));
}

void critical_point_tracker_regular::domain_arrays(long long dst[3], long long dsz[3]) const
{
  for (int d = 0; d < 3; d ++) { dst[d] = d < nd ? domain.start(d) : 0; dsz[d] = d < nd ? domain.size(d) : 1; }
}

// regular_tracker::initialize, regular_tracker.hh:105-149.  Single process per GPU: the partitioner returns the whole domain
// (local_domain == domain) and, with is_input_array_partial == false, local_array_domain == array_domain.
void critical_point_tracker_regular::apply_configuration(ftkx_ctx *c)
{
  long long dst[3], dsz[3], est[3] = {0, 0, 0}, esz[3] = {1, 1, 1};
  domain_arrays(dst, dsz);
  for (int d = 0; d < nd; d ++) { est[d] = array_domain.start(d); esz[d] = array_domain.size(d); }
  check_on(c, ftkx_set_mesh(c, dst, dsz, dst, dsz, est, esz));
  ftkx_options o;
  ftkx_default_options(&o);
  o.jacobian_symmetric = is_jacobian_field_symmetric;
  o.robust = enable_robust_detection;
  o.use_type_filter = use_type_filter;
  o.type_filter = type_filter;
  o.compute_degrees = enable_computing_degrees;
  o.tag_mode = tag_mode;
  o.exact_only = exact_only;
  o.derive_jacobian = jacobian_field_source == SOURCE_DERIVED;
  if (mode_phys_coords == 2) {
    if ((int)rectilinear_coords.size() < nd) throw ftkx_error(FTKX_E_INVALID, "initialize: set_coords_rectilinear needs one array per axis");
    const std::vector<double> none;
    const std::vector<double> &z = nd == 3 ? rectilinear_coords[2] : none;
    check_on(c, ftkx_set_coords_rectilinear(c, rectilinear_coords[0].data(), rectilinear_coords[0].size(), rectilinear_coords[1].data(), rectilinear_coords[1].size(),
                                            z.empty() ? nullptr : z.data(), z.size()));
  } else if (mode_phys_coords == 3)
    check_on(c, ftkx_set_coords_explicit(c, explicit_coords.data(), explicit_ncomp, explicit_n0, explicit_n1));
  o.coords_mode = mode_phys_coords;
  for (size_t i = 0; i < 6 && i < bounds_coords.size(); i ++) o.coords_bounds[i] = bounds_coords[i];
  check_on(c, ftkx_set_options(c, &o));
  check_on(c, ftkx_set_spatial_smoothing(c, spatial_smoothing_sigma, spatial_smoothing_ksize));
  check_on(c, ftkx_set_vector_smoothing(c, vector_smoothing_sigma, vector_smoothing_ksize));
  check_on(c, ftkx_set_perturbation(c, perturbation_sigma, perturbation_seed));
  check_on(c, ftkx_set_clamp(c, clamp_on ? 1 : 0, clamp_lo, clamp_hi));
  check_on(c, ftkx_set_temporal_smoothing(c, temporal_smoothing_sigma, temporal_smoothing_ksize, next_push_timestep));
  check_on(c, ftkx_set_series_sampling(c, samples_in_pass() ? 1 : 0));      // (set_sampling_in_pass with components: the passes fill slots 1, 2)
}

void critical_point_tracker_regular::initialize()
{
  if ((int)domain.nd() != nd || (int)array_domain.nd() != nd) throw ftkx_error(FTKX_E_INVALID, "initialize: set_domain / set_array_domain first");
  if (temporal_smoothing_ksize && (multi || slab))
    throw ftkx_error(FTKX_E_UNSUPPORTED, "initialize: temporal smoothing with one device and no slab mode only (a slab needs raw halo snapshots of its neighbours)");
  if (n_extra_expected() > 0 && (multi || slab || temporal_smoothing_ksize))
    throw ftkx_error(FTKX_E_UNSUPPORTED, "initialize: extra scalar components with one device, no slab mode and no temporal smoothing only (its emissions lag the pushes)");
  sync();
  if (multi) { for (auto &W : multi->w) apply_configuration(W->ctx); }
  else apply_configuration(ctx);
  // the discrete points are kept in the reference's element order, which needs the mesh sizes: what is there is ordered afresh
  order_.nd = nd;
  for (int d = 0; d < nd; d ++) order_.n[d] = domain.size(d);
  if (!points.empty()) {
    std::vector<feature_point_t> again;
    again.swap(points); point_keys.clear();
    again.insert(again.end(), pending_points.begin(), pending_points.end());
    pending_points.swap(again);
    pending_ascending = false;
  }
  discrete_critical_points = discrete_map_t(order_);
  map_valid = false;
  initialized = true;
}

// critical_point_tracker_2d_regular::reset, 2d:227-236 (+ critical_point_tracker::reset, critical_point_tracker.hh:31-34).
// Like the reference, the running resolution is NOT reset.
void critical_point_tracker_regular::reset()
{
  if (!slab) sync();                            // (slab mode: sync() is the slab's pass, a collective -- a reset does not sweep)
  ftkx_online_tracer_destroy(online); online = nullptr;
  if (multi) multi->restart(vector_field_resolution);
  current_timestep = 0;
  while (pop_field_data_snapshot()) {}
  next_push_timestep = 0;
  last_push_snapshots = 1;
  if (initialized && temporal_smoothing_ksize) check(ftkx_set_temporal_smoothing(ctx, temporal_smoothing_sigma, temporal_smoothing_ksize, 0));   // the ring is emptied
  if (slab) restart_slab();
  pending_points.clear(); pending_ascending = true;
  points.clear(); point_keys.clear();
  discrete_critical_points.clear(); map_valid = true;
}

// one snapshot -> the context(s) whose steps read it (kind: see push_to)
void critical_point_tracker_regular::push_snapshot(int kind, const void *s, const void *v, const void *j, bool device, int dtype, int planes)
{
  const bool f32 = dtype == FTKX_DTYPE_F32;
  if (ftkx_dtype_size(dtype) == 0) throw ftkx_error(FTKX_E_INVALID, "push: element type " + std::to_string(dtype) + " is not one of FTKX_DTYPE_*");
  if (planes && dtype != FTKX_DTYPE_F64 && !f32) throw ftkx_error(FTKX_E_UNSUPPORTED, "push: component planes are FP64 or float32");
  if (planes && multi) throw ftkx_error(FTKX_E_UNSUPPORTED, "push: component planes with one device only (a multi-device tracker takes the interleaved FP64 array)");
  if (f32 && multi) throw ftkx_error(FTKX_E_UNSUPPORTED, "push: float32 snapshots with one device only (a multi-device tracker takes FP64 arrays)");
  if (dtype != FTKX_DTYPE_F64 && multi) throw ftkx_error(FTKX_E_UNSUPPORTED, "push: half, bfloat16 and integer snapshots with one device only (a multi-device tracker takes FP64 arrays)");
  if (extras_in_push != n_extra_expected())
    throw ftkx_error(FTKX_E_INVALID, "push: " + std::to_string(scalar_components.size()) + " scalar components take " + std::to_string(n_extra_expected()) + " extra arrays with every snapshot, not " +
                                     std::to_string(extras_in_push));
  if (extras_in_push > 0 && (multi || slab || temporal_smoothing_ksize || (deferred_collection && !samples_in_pass())))
    throw ftkx_error(FTKX_E_UNSUPPORTED, "push: extra scalar components not with deferred collection, several devices, slab mode or temporal smoothing");
  if (temporal_smoothing_ksize) {
    // the raw snapshot feeds the filter; what the filter emits is the snapshot the tracker sees (a device source is read, not adopted)
    if (kind == 2) throw ftkx_error(FTKX_E_UNSUPPORTED, "push_field_data_snapshot: temporal smoothing takes a scalar or a vector snapshot alone");
    int t_emitted = -1;
    last_push_snapshots = 0;
    const void *a = kind == 0 ? s : v;
    if (planes) check(f32 ? ftkx_temporal_push_planar_f32(ctx, static_cast<const float *const *>(v), planes, device ? 1 : 0, &t_emitted)
                          : ftkx_temporal_push_planar(ctx, static_cast<const double *const *>(v), planes, device ? 1 : 0, &t_emitted));
    else check(ftkx_temporal_push_typed(ctx, a, dtype, kind, device ? 1 : 0, &t_emitted));
    take_emitted(t_emitted);
    return;
  }
  last_push_snapshots = 1;
  const int t = next_push_timestep;
  if (slab && (t < slab_t0 || t >= slab_t1)) throw ftkx_error(FTKX_E_INVALID, "slab mode: timestep " + std::to_string(t) + " is not in this rank's slab [" + std::to_string(slab_t0) + ", " + std::to_string(slab_t1) + ")");
  if (multi) multi->push(kind, t, static_cast<const double *>(s), static_cast<const double *>(v), static_cast<const double *>(j), device);
  else check(push_to(ctx, kind, t, s, v, j, device ? 1 : 0, dtype, planes));
  field_data_snapshots.push_back(t);
  next_push_timestep ++;
}

// the filter's emission `t` (-1: none) is the next snapshot of the series
void critical_point_tracker_regular::take_emitted(int t)
{
  if (t < 0) return;
  if (t != next_push_timestep) throw ftkx_error(FTKX_E_INVALID, "temporal smoothing: emission " + std::to_string(t) + " where timestep " + std::to_string(next_push_timestep) + " was due");
  field_data_snapshots.push_back(t);
  next_push_timestep ++;
  last_push_snapshots = 1;
}

bool critical_point_tracker_regular::flush_temporal_smoothing()
{
  if (!initialized || !temporal_smoothing_ksize) return false;
  int t_emitted = -1;
  check(ftkx_temporal_flush(ctx, &t_emitted));
  take_emitted(t_emitted);
  return t_emitted >= 0;
}

void critical_point_tracker_regular::push_scalar(const void *s, bool device, int dtype)
{
  if (!initialized) throw ftkx_error(FTKX_E_INVALID, "push: initialize() first");
  if (vector_field_source != SOURCE_DERIVED) throw ftkx_error(FTKX_E_INVALID, "push_scalar_field_snapshot: vector_field_source must be SOURCE_DERIVED");
  push_snapshot(0, s, nullptr, nullptr, device, dtype);       // V = gradientND(s) on the device
}

void critical_point_tracker_regular::push_vector(const void *v, bool device, int dtype, int planes)
{
  if (!initialized) throw ftkx_error(FTKX_E_INVALID, "push: initialize() first");
  if (spatial_smoothing_ksize && !vector_smoothing_ksize)
    throw ftkx_error(FTKX_E_UNSUPPORTED, "push_vector_field_snapshot: spatial smoothing takes scalar snapshots only (vectors: set_vector_spatial_smoothing)");
  push_snapshot(1, nullptr, v, nullptr, device, dtype, planes);       // J derived at hits when jacobian_field_source == SOURCE_DERIVED
}

void critical_point_tracker_regular::push_field_data(const void *s, const void *v, const void *j, bool device, int dtype)
{
  if (!initialized) throw ftkx_error(FTKX_E_INVALID, "push: initialize() first");
  if (spatial_smoothing_ksize) throw ftkx_error(FTKX_E_UNSUPPORTED, "push_field_data_snapshot: spatial smoothing takes scalar snapshots only");
  if (vector_smoothing_ksize) throw ftkx_error(FTKX_E_UNSUPPORTED, "push_field_data_snapshot: vector smoothing takes a vector snapshot alone (a given J or S does not belong to the smoothed field)");
  if (perturbation_sigma > 0 || clamp_on) throw ftkx_error(FTKX_E_UNSUPPORTED, "push_field_data_snapshot: perturbation and clamp take a scalar or a vector snapshot alone");
  push_snapshot(2, s, v, j, device, dtype);
}

void critical_point_tracker_regular::push_scalar_field_snapshot(const double *s, bool device) { push_scalar(s, device, FTKX_DTYPE_F64); }
void critical_point_tracker_regular::push_vector_field_snapshot(const double *v, bool device) { push_vector(v, device, FTKX_DTYPE_F64); }
void critical_point_tracker_regular::push_field_data_snapshot(const double *s, const double *v, const double *j, bool device) { push_field_data(s, v, j, device, FTKX_DTYPE_F64); }
void critical_point_tracker_regular::push_scalar_field_snapshot(const float *s, bool device) { push_scalar(s, device, FTKX_DTYPE_F32); }
void critical_point_tracker_regular::push_vector_field_snapshot(const float *v, bool device) { push_vector(v, device, FTKX_DTYPE_F32); }
void critical_point_tracker_regular::push_field_data_snapshot(const float *s, const float *v, const float *j, bool device) { push_field_data(s, v, j, device, FTKX_DTYPE_F32); }
void critical_point_tracker_regular::push_scalar_field_snapshot(const void *s, int dtype, bool device) { push_scalar(s, device, dtype); }
void critical_point_tracker_regular::push_vector_field_snapshot(const void *v, int dtype, bool device) { push_vector(v, device, dtype); }
void critical_point_tracker_regular::push_field_data_snapshot(const void *s, const void *v, const void *j, int dtype, bool device) { push_field_data(s, v, j, device, dtype); }

// ---- extra scalar components (set_scalar_components) ------------------------------------------------------------------------------------
void critical_point_tracker_regular::set_scalar_components(const std::vector<std::string> &names)
{
  if (names.empty() || names.size() > 3) throw ftkx_error(FTKX_E_INVALID, "set_scalar_components: one to three names (FTK_CP_MAX_NUM_VARS = 3)");
  scalar_components = names;
}

// a snapshot and its extras: the snapshot as ever, then extra[k] as the aux array of slot k + 1 at the snapshot's timestep.  The extras are
// checked first: a push that fails leaves no snapshot behind.
void critical_point_tracker_regular::push_with_extras(int kind, const void *s, const void *v, const void *j, const void *const *extra, int n_extra, bool device, bool f32)
{
  if (n_extra < 0 || n_extra > 2 || (n_extra > 0 && !extra)) throw ftkx_error(FTKX_E_INVALID, "push: zero to two extra arrays");
  for (int k = 0; k < n_extra; k ++) if (!extra[k]) throw ftkx_error(FTKX_E_INVALID, "push: extra array " + std::to_string(k) + " is null");
  const int t = next_push_timestep;
  extras_in_push = n_extra;
  try {
    const int dtype = f32 ? FTKX_DTYPE_F32 : FTKX_DTYPE_F64;
    if (kind == 0) push_scalar(s, device, dtype);
    else if (kind == 1) push_vector(v, device, dtype);
    else push_field_data(s, v, j, device, dtype);
  } catch (...) { extras_in_push = 0; throw; }
  extras_in_push = 0;
  for (int k = 0; k < n_extra; k ++)
    check(f32 ? ftkx_push_aux_slice_f32(ctx, t, k + 1, static_cast<const float *>(extra[k]), device ? 1 : 0)
              : ftkx_push_aux_slice(ctx, t, k + 1, static_cast<const double *>(extra[k]), device ? 1 : 0));
}

void critical_point_tracker_regular::push_scalar_field_snapshot(const double *s, const double *const *extra, int n_extra, bool device)
{ push_with_extras(0, s, nullptr, nullptr, reinterpret_cast<const void *const *>(extra), n_extra, device, false); }
void critical_point_tracker_regular::push_vector_field_snapshot(const double *v, const double *const *extra, int n_extra, bool device)
{ push_with_extras(1, nullptr, v, nullptr, reinterpret_cast<const void *const *>(extra), n_extra, device, false); }
void critical_point_tracker_regular::push_field_data_snapshot(const double *s, const double *v, const double *j, const double *const *extra, int n_extra, bool device)
{ push_with_extras(2, s, v, j, reinterpret_cast<const void *const *>(extra), n_extra, device, false); }
void critical_point_tracker_regular::push_scalar_field_snapshot(const float *s, const float *const *extra, int n_extra, bool device)
{ push_with_extras(0, s, nullptr, nullptr, reinterpret_cast<const void *const *>(extra), n_extra, device, true); }
void critical_point_tracker_regular::push_vector_field_snapshot(const float *v, const float *const *extra, int n_extra, bool device)
{ push_with_extras(1, nullptr, v, nullptr, reinterpret_cast<const void *const *>(extra), n_extra, device, true); }
void critical_point_tracker_regular::push_field_data_snapshot(const float *s, const float *v, const float *j, const float *const *extra, int n_extra, bool device)
{ push_with_extras(2, s, v, j, reinterpret_cast<const void *const *>(extra), n_extra, device, true); }

// The sampling point: behind the step's sweep, in front of the pop of its snapshots.  The context's record buffer stays as the sweep left it.
void critical_point_tracker_regular::sample_step_records(const ftkx_cp_t *&recs, size_t n, std::vector<ftkx_cp_t> &store)
{
  if (n_extra_expected() == 0 || n == 0) return;
  store.assign(recs, recs + n);
  check(ftkx_sample_aux(ctx, store.data(), n));
  recs = store.data();
}

// nc < 1 never reaches push_snapshot, where 0 means "no planes"; whether nc is the tracker's dimension is the context's check
void critical_point_tracker_regular::push_vector_field_components(const double *const *comps, int nc, bool device)
{
  if (!comps || nc < 1) throw ftkx_error(FTKX_E_INVALID, "push_vector_field_components: no components");
  push_vector(comps, device, FTKX_DTYPE_F64, nc);
}
void critical_point_tracker_regular::push_vector_field_components(const float *const *comps, int nc, bool device)
{
  if (!comps || nc < 1) throw ftkx_error(FTKX_E_INVALID, "push_vector_field_components: no components");
  push_vector(comps, device, FTKX_DTYPE_F32, nc);
}

bool critical_point_tracker_regular::pop_field_data_snapshot()
{
  if (field_data_snapshots.empty()) return false;
  const int t = field_data_snapshots.front();
  if (multi) multi->drop(t);
  else if (!batch_ts.empty() && t >= batch_ts.front()) batch_drops.push_back(t);      // (a recorded step still reads it: dropped behind its batch)
  else check(ftkx_drop_slice(ctx, t));
  field_data_snapshots.erase(field_data_snapshots.begin());
  return true;
}

// critical_point_tracker::update_vector_field_scaling_factor, critical_point_tracker.hh:850-864: sticky running minimum of
// ndarray::resolution() over every queued snapshot.  The per-slice reduction is fused into the pass that builds the slice's
// sign masks (ftkx_slices_prepare: each snapshot is read from HBM once, when it first takes part in a step), under the factor
// in force so far -- which the running minimum can only raise.  What comes back per slice is its smallest non-zero |v| BELOW
// 1 / that factor (or DBL_MAX): values at or above it cannot change nbits, so the factor sequence is the reference's, while
// vector_field_resolution itself (never observable in the reference either) is exact only once it is below 2^-8.
void critical_point_tracker_regular::update_vector_field_scaling_factor(int minbits, int maxbits)
{
  const unsigned long long hint = std::max(vector_field_scaling_factor, 1ull << minbits);   // never above the factor this step ends up with
  std::vector<double> below(field_data_snapshots.size());
  if (!field_data_snapshots.empty())
    check(ftkx_slices_prepare(ctx, field_data_snapshots.data(), (int)field_data_snapshots.size(), hint, below.data(), nullptr));
  for (double r : below) vector_field_resolution = std::min(vector_field_resolution, r);
  vector_field_scaling_factor = factor_of(vector_field_resolution, minbits, maxbits);
}

// the records of one sweep -> pending points of timestep `timestep`
void critical_point_tracker_regular::take_records(const ftkx_cp_t *recs, size_t n, int timestep)
{
  for (size_t i = 0; i < n; i ++) {
    feature_point_t cp = point_of(recs[i]);
    cp.timestep = timestep;
    if (scalar_field_source == SOURCE_NONE) cp.scalar[0] = 0.0;   // 2d:642-646: scalar only when a scalar field exists
    if (!pending_points.empty() && pending_points.back().tag >= cp.tag) pending_ascending = false;
    pending_points.push_back(cp);                                 // -> the flat store at the next sync()
  }
}

// records of several steps, each under the timestep it carries
void critical_point_tracker_regular::take_records_by_step(const ftkx_cp_t *recs, size_t n)
{
  for (size_t i = 0; i < n; i ++) take_records(recs + i, 1, ftkx_cp_timestep(recs + i));
}

// critical_point_tracker_{2d,3d}_regular::update_timestep (2d:263-433, 3d:150-308): ordinal sweep at current_timestep and,
// when two snapshots are queued, the interval sweep [current, current+1] -- here one launch, one download.
void critical_point_tracker_regular::update_timestep()
{
  if (field_data_snapshots.empty()) return;
  if (slab) return step_slab();
  const int scope = field_data_snapshots.size() >= 2 ? FTKX_SCOPE_BOTH : FTKX_SCOPE_ORDINAL;
  if (multi) return step_multi(scope);
  if (deferred_collection && !enable_streaming_trajectories && window_is_the_step()) return step_deferred(scope);
  step_now(scope);
}

// deferred collection: queue this step (continuing, on the device, from the running minimum of the step queued before it if that one is
// still out), then collect the step before it
void critical_point_tracker_regular::step_deferred(int scope)
{
  // (components: only where the pass samples its own records -- in stream order, in front of whatever reuses the popped snapshots' arrays)
  if (n_extra_expected() > 0 && !samples_in_pass())
    throw ftkx_error(FTKX_E_UNSUPPORTED, "update_timestep: extra scalar components not with deferred collection (a step's snapshots are popped before its records arrive; set_sampling_in_pass(true) lifts this)");
  if (deferred_depth > 1) {                 // batches: recorded; queued with the batch's last step (submit_batch)
    batch_ts.push_back(current_timestep); batch_scopes.push_back(scope);
    if ((int)batch_ts.size() >= deferred_depth) submit_batch();
    return;
  }
  const bool chained = !open_steps.empty();
  check(ftkx_sweep_series_submit(ctx, &current_timestep, &scope, 1, chained ? nullptr : &vector_field_resolution));
  open_steps.push_back(current_timestep);
  if (open_steps.size() >= 3) collect_open_step();      // (three in flight: the host runs one pass ahead of a split pass's tail)
}

// one device, the step swept and collected in this call
void critical_point_tracker_regular::step_now(int scope)
{
  // (the step that follows is known before its factor is: announced, its cull is queued right behind the mask kernel of the
  // newly arrived snapshot and runs while the host waits for the reduction)
  const ftkx_cp_t *recs = nullptr;
  size_t n = 0;
  collect_deferred();
  bool filled = false;      // the pass filled slots 1, 2 itself (set_sampling_in_pass)
  if (window_is_the_step()) {
    // The device-driven pass (ftkx_sweep_series): the newly arrived snapshot's masks and reduction, the sticky factor (formed on the
    // device from the running minimum handed in), cull, exact test and records are queued at once and waited for once.
    unsigned long long f = 0;
    check(ftkx_sweep_series(ctx, &current_timestep, &scope, 1, &vector_field_resolution, &f, &recs, &n));
    vector_field_scaling_factor = f;
    filled = samples_in_pass();
  } else {
    // (more than two snapshots queued: the reference's factor takes every queued snapshot into account, critical_point_tracker.hh:853)
    check(ftkx_sweep_announce(ctx, &current_timestep, &scope, 1));
    update_vector_field_scaling_factor();
    check(ftkx_sweep(ctx, current_timestep, scope, vector_field_scaling_factor, &recs, &n));
  }
  std::vector<ftkx_cp_t> sampled;
  if (!filled) sample_step_records(recs, n, sampled);
  take_records(recs, n, current_timestep);
  check(ftkx_get_stats(ctx, &last_stats));
  if (enable_streaming_trajectories && scope == FTKX_SCOPE_BOTH) grow();      // 2d:326-330, 3d:197-201: only after an interval sweep
}

// Several devices: the step is queued on the device that owns its timestep and this call returns (multi_engine::step).
void critical_point_tracker_regular::step_multi(int scope)
{
  if (enable_streaming_trajectories) throw ftkx_error(FTKX_E_UNSUPPORTED, "enable_streaming_trajectories: single-device trackers only");
  const std::vector<int> ts(field_data_snapshots.begin(), field_data_snapshots.begin() + (scope == FTKX_SCOPE_BOTH ? 2 : 1));
  multi->step(current_timestep, scope, ts, default_minbits, default_maxbits, [this](const multi_engine::step_result &r) {
    take_records(r.recs, r.n, r.t);
    // steps finish out of order: the members keep the values of the LATEST timestep, as a sequential run would leave them
    if (r.t >= result_timestep) { result_timestep = r.t; last_stats = r.stats; vector_field_scaling_factor = r.factor; vector_field_resolution = r.resolution; }
  });
}

// critical_point_tracker::advance_timestep, critical_point_tracker.hh:841-848
bool critical_point_tracker_regular::advance_timestep()
{
  update_timestep();
  if (slab) { current_timestep ++; return current_timestep < next_push_timestep; }      // (slab mode: the snapshots stay until the slab's pass has run)
  pop_field_data_snapshot();
  current_timestep ++;
  return field_data_snapshots.size() > 0;
}

// trace_critical_points_online (critical_point_tracker.hh:523-639) on everything in discrete_critical_points, which it consumes
void critical_point_tracker_regular::grow()
{
  flush_points();
  if (!online) {
    long long dst[3], dsz[3];
    domain_arrays(dst, dsz);
    const int rc = ftkx_online_tracer_create(&online, nd, dst, dsz);
    if (rc != FTKX_OK) throw ftkx_error(rc, "online tracer");
  }
  std::vector<ftkx_cp_t> recs;
  recs.reserve(points.size());
  for (const feature_point_t &cp : points) recs.push_back(record_of(cp));
  const int rc = ftkx_online_tracer_grow(online, recs.data(), recs.size());
  if (rc != FTKX_OK) throw ftkx_error(rc, "grow: ftkx_online_tracer_grow failed (element tags needed: FTKX_TAG_EXACT64, or REFERENCE where it does not wrap)");
  points.clear(); point_keys.clear();
  discrete_critical_points.clear(); map_valid = true;
}

void critical_point_tracker_regular::clear_traced() { traced_points.clear(); traced_offsets.assign(1, 0); traced_nested_valid = false; traced_loop.clear(); traced_id.clear(); }

// critical_point_tracker_{2d,3d}_regular::finalize (2d:143-225, 3d:86-117)
void critical_point_tracker_regular::finalize()
{
  wait_devices();
  if (slab && !gather_slab_points()) { clear_traced(); return; }
  if (enable_streaming_trajectories) finish_streaming();
  else trace_offline();
}

// critical_point_tracker.hh:689: the ranks' discrete points gathered on the root, which traces them -- curves cross slab boundaries like
// any other cell boundary.  The other ranks keep their own points and end without trajectories.  True on the rank that traces.
bool critical_point_tracker_regular::gather_slab_points()
{
  flush_points();
  std::vector<ftkx_cp_t> mine(points.size());
  for (size_t i = 0; i < points.size(); i ++) mine[i] = record_of(points[i]);
  ftkx_cp_t *merged = nullptr;
  size_t nm = 0;
  check_slab(slab, ftkx_slab_gather_records(slab, mine.data(), mine.size(), 0, &merged, &nm));
  if (slab_rank != 0) return false;
  points.clear(); point_keys.clear(); pending_points.clear(); pending_ascending = true;
  discrete_critical_points.clear(); map_valid = false;
  take_records_by_step(merged, nm);
  ftkx_free(merged);
  return true;
}

// 2d:150-151: "done" -- the trajectories are what grow() built
void critical_point_tracker_regular::finish_streaming()
{
  flush_points();
  clear_traced();
  if (!online) return;
  ftkx_cp_t *pts = nullptr;
  ftkx_curves c{};
  const int rc = ftkx_online_tracer_curves(online, &pts, &c);
  if (rc != FTKX_OK) { ftkx_free(pts); ftkx_free_curves(&c); throw ftkx_error(rc, "finalize: ftkx_online_tracer_curves failed"); }
  for (size_t i = 0; i < c.n_curves; i ++) {
    for (long long k = c.offsets[i]; k < c.offsets[i + 1]; k ++) traced_points.push_back(point_of(pts[k]));
    traced_offsets.push_back((long long)traced_points.size());
    traced_loop.push_back(c.loop[i]);
    traced_id.push_back((int)i);
  }
  ftkx_free(pts); ftkx_free_curves(&c);
}

// Without streaming trajectories:
// traced_critical_points = trace_critical_points_offline(discrete_critical_points, neighbours-sharing-a-cell)
void critical_point_tracker_regular::trace_offline()
{
  // Nothing has to be ordered for this: ftkx_trace_curves takes the points in any order (it indexes them by tag) and returns the curves
  // in the reference's order.  Sweeps in time order with 64-bit tags deliver ascending tags: the pending points are traced as they are.
  if (!(points.empty() && pending_ascending)) flush_points();
  const std::vector<feature_point_t> &src = points.empty() ? pending_points : points;
  // (the flat store is in the reference's element order; the trace's device phases want ascending tags: an index sorted on a few
  // threads, and the curves' indices mapped back through it)
  std::vector<std::pair<unsigned long long, size_t>> by_tag;
  if (!points.empty()) {
    by_tag.resize(src.size());
    for (size_t i = 0; i < src.size(); i ++) by_tag[i] = {src[i].tag, i};
    ftkx::sort_on_threads(by_tag);
  }
  std::vector<unsigned long long> tags(src.size());           // (the trace reads nothing but the tags)
  for (size_t i = 0; i < src.size(); i ++) tags[i] = by_tag.empty() ? src[i].tag : by_tag[i].first;
  long long dst[3], dsz[3];
  domain_arrays(dst, dsz);
  ftkx_curves c{};
  // (neighbour search and component labelling on the tracker's GPU where the record set is large enough to pay for the round trip)
  const int rc = trace_on_device && ctx ? ftkx_trace_curves_device(ctx, nd, dst, dsz, tags.data(), tags.size(), 0, &c)
                                 : ftkx_trace_curves_tags_ctx(ctx, nd, dst, dsz, tags.data(), tags.size(), &c);
  if (rc != FTKX_OK) { ftkx_free_curves(&c); throw ftkx_error(rc, "finalize: ftkx_trace_curves failed (tags must not have overflowed int32: use FTKX_TAG_EXACT64 on very large meshes)"); }
  // the curves stay flat -- the points of all curves one after the other; one vector per curve is built only if somebody asks for it
  traced_points.resize(c.n_points); traced_offsets.assign(c.offsets, c.offsets + c.n_curves + 1);
  traced_loop.assign(c.loop, c.loop + c.n_curves); traced_id.resize(c.n_curves);
  ftkx::for_ranges_on_threads(c.n_points, [&](size_t b, size_t e) {
    for (size_t k = b; k < e; k ++) traced_points[k] = src[by_tag.empty() ? (size_t)c.indices[k] : by_tag[(size_t)c.indices[k]].second];
  });
  for (size_t i = 0; i < c.n_curves; i ++) traced_id[i] = (int)i;
  traced_nested_valid = false;
  ftkx_free_curves(&c);
}

namespace {
struct flat_curves {   // traced curves as one record array (points in curve order) + the identity as index list
  std::vector<ftkx_cp_t> recs;
  std::vector<long long> indices;
  flat_curves(const std::vector<feature_point_t> &pts) : recs(pts.size()), indices(pts.size())
  {
    ftkx::for_ranges_on_threads(pts.size(), [&](size_t b, size_t e) { for (size_t i = b; i < e; i ++) { recs[i] = record_of(pts[i]); indices[i] = (long long)i; } });
  }
};
}  // namespace
// json_interface::post_process (filters/json_interface.hh:758-800) with the options it defaults to
void critical_point_tracker_regular::post_process()
{
  flat_curves f(traced_points);
  ftkx_curves in;
  std::memset(&in, 0, sizeof(in));
  in.n_curves = num_traced_curves(); in.n_points = f.recs.size();
  in.offsets = traced_offsets.data(); in.indices = f.indices.data(); in.loop = traced_loop.data();
  ftkx_trajectories out{};
  const int rc = post_process_on_device && trace_on_device && ctx ? ftkx_post_process_curves_device(ctx, f.recs.data(), f.recs.size(), &in, &out)
                                                                  : ftkx_post_process_curves(f.recs.data(), f.recs.size(), &in, &out);
  if (rc != FTKX_OK) { ftkx_free_trajectories(&out); throw ftkx_error(rc, "post_process failed"); }
  std::vector<feature_point_t> pts(out.n_points);
  std::vector<int> loop(out.n_curves), ids(out.n_curves);
  ftkx::for_ranges_on_threads(out.n_points, [&](size_t b, size_t e) {
    for (size_t k = b; k < e; k ++) {
      pts[k] = traced_points[(size_t)out.indices[k]];
      pts[k].type = out.type[k]; pts[k].t = out.t[k];
    }
  });
  // a split piece keeps its parent's label; labels of traced curves are their own (possibly already post-processed) ids
  for (size_t c = 0; c < out.n_curves; c ++) { loop[c] = out.loop[c]; ids[c] = traced_id[out.id[c]]; }
  traced_offsets.assign(out.offsets, out.offsets + out.n_curves + 1);
  ftkx_free_trajectories(&out);
  traced_points.swap(pts); traced_loop.swap(loop); traced_id.swap(ids);
  traced_nested_valid = false;
}

const std::vector<std::vector<feature_point_t>> &critical_point_tracker_regular::get_traced_critical_points() const
{
  if (!traced_nested_valid) {
    traced_critical_points.assign(num_traced_curves(), std::vector<feature_point_t>());
    for (size_t c = 0; c < num_traced_curves(); c ++)
      traced_critical_points[c].assign(traced_points.begin() + traced_offsets[c], traced_points.begin() + traced_offsets[c + 1]);
    traced_nested_valid = true;
  }
  return traced_critical_points;
}

void critical_point_tracker_regular::write_discrete(const std::string &filename, int format) const
{
  sync();
  std::vector<ftkx_cp_t> recs;
  recs.reserve(points.size());
  for (const feature_point_t &cp : points) recs.push_back(record_of(cp));
  // text labels: the reference's scalar_components default to {"scalar"} whether or not a scalar field exists
  std::vector<const char *> names;
  for (const std::string &s : scalar_components) names.push_back(s.c_str());
  check_on(nullptr, ftkx_write_critical_points(filename.c_str(), format, recs.data(), recs.size(), nullptr, nullptr, names.empty() ? nullptr : names.data(),
                                               names.empty() ? -1 : (int)names.size()));     // (the i/o calls leave their message with the calling thread)
}
void critical_point_tracker_regular::write_critical_points_json(const std::string &f) const { write_discrete(f, FTKX_FORMAT_JSON); }
void critical_point_tracker_regular::write_critical_points_binary(const std::string &f) const { write_discrete(f, FTKX_FORMAT_BINARY); }
void critical_point_tracker_regular::write_critical_points_text(const std::string &f) const { write_discrete(f, FTKX_FORMAT_TEXT); }

// critical_point_tracker_regular::put_critical_points (critical_point_tracker_regular.hh:40-46): tags are trusted as keys
void critical_point_tracker_regular::put_critical_points(const std::vector<feature_point_t> &cps)
{
  for (const auto &cp : cps) {
    if (!pending_points.empty() && pending_points.back().tag >= cp.tag) pending_ascending = false;
    pending_points.push_back(cp);
  }
}

void critical_point_tracker_regular::read_discrete(const std::string &filename, int format)
{
  ftkx_cp_t *recs = nullptr;
  size_t n = 0;
  check_on(nullptr, ftkx_read_critical_points(filename.c_str(), format, &recs, &n, nullptr, nullptr));     // (the i/o calls leave their message with the calling thread)
  std::vector<feature_point_t> cps;
  cps.reserve(n);
  for (size_t i = 0; i < n; i ++) cps.push_back(point_of(recs[i]));
  ftkx_free(recs);
  put_critical_points(cps);
}
void critical_point_tracker_regular::read_critical_points_json(const std::string &f) { read_discrete(f, FTKX_FORMAT_JSON); }
void critical_point_tracker_regular::read_critical_points_binary(const std::string &f) { read_discrete(f, FTKX_FORMAT_BINARY); }

void critical_point_tracker_regular::write_traced(const std::string &filename, int format) const
{
  flat_curves f(traced_points);
  std::vector<unsigned> type(f.recs.size() ? f.recs.size() : 1);
  std::vector<double> t(f.recs.size() ? f.recs.size() : 1);
  for (size_t i = 0; i < f.recs.size(); i ++) { type[i] = f.recs[i].type; t[i] = f.recs[i].t; }
  std::vector<int> loop(traced_loop), ids(traced_id);
  loop.resize(num_traced_curves() + 1); ids.resize(num_traced_curves() + 1);
  std::vector<long long> offsets(traced_offsets);
  ftkx_trajectories tr;
  std::memset(&tr, 0, sizeof(tr));
  tr.n_curves = num_traced_curves(); tr.n_points = f.recs.size();
  tr.offsets = offsets.data(); tr.indices = f.indices.data(); tr.loop = loop.data(); tr.type = type.data(); tr.t = t.data(); tr.id = ids.data();
  std::vector<const char *> names;
  for (const std::string &s : scalar_components) names.push_back(s.c_str());
  check_on(nullptr, ftkx_write_traced_critical_points(filename.c_str(), format, f.recs.data(), f.recs.size(), &tr, names.empty() ? nullptr : names.data(),
                                                      names.empty() ? -1 : (int)names.size()));     // (the i/o calls leave their message with the calling thread)
}
void critical_point_tracker_regular::write_traced_critical_points_json(const std::string &f) const { write_traced(f, FTKX_FORMAT_JSON); }
void critical_point_tracker_regular::write_traced_critical_points_binary(const std::string &f) const { write_traced(f, FTKX_FORMAT_BINARY); }
void critical_point_tracker_regular::write_traced_critical_points_text(const std::string &f) const { write_traced(f, FTKX_FORMAT_TEXT); }

std::vector<feature_point_t> critical_point_tracker_regular::get_critical_points() const
{
  sync();
  return points;
}

}  // namespace ftkx

// ---- C handles ---------------------------------------------------------------------------------------------------
struct ftkx_tracker {
  ftkx::critical_point_tracker_regular *t = nullptr;
  int nd = 0;
  mutable std::string err;     // (the last error is the handle's own note: a failing getter of a const handle leaves it too)
};

namespace {
thread_local std::string g_tracker_error;

template <class F>
int guarded(const ftkx_tracker *h, F f)
{
  if (!h || !h->t) { g_tracker_error = "null tracker"; return FTKX_E_INVALID; }
  try { f(); return FTKX_OK; }
  catch (const ftkx::ftkx_error &e) { h->err = e.what(); g_tracker_error = e.what(); return e.code; }
  catch (const std::exception &e) { h->err = e.what(); g_tracker_error = e.what(); return FTKX_E_INVALID; }
}

// a handle around the tracker that `make` constructs; a constructor's error is the calling thread's
template <class Make>
int create_handle(ftkx_tracker **out, int nd, Make make)
{
  std::unique_ptr<ftkx_tracker> h(new ftkx_tracker());
  try { h->nd = nd; h->t = make(); *out = h.release(); return FTKX_OK; }
  catch (const ftkx::ftkx_error &e) { g_tracker_error = e.what(); return e.code; }
  catch (const std::exception &e) { g_tracker_error = e.what(); return FTKX_E_INVALID; }
}
}  // namespace

extern "C" {

int ftkx_tracker_create(ftkx_tracker **out, int nd, int device_id)
{
  if (!out || (nd != 2 && nd != 3)) { g_tracker_error = "ftkx_tracker_create: nd must be 2 or 3"; return FTKX_E_INVALID; }
  return create_handle(out, nd, [&] { return new ftkx::critical_point_tracker_regular(nd, device_id); });
}

int ftkx_tracker_create_multi(ftkx_tracker **out, int nd, const int *device_ids, int ndev, int block)
{
  if (!out || (nd != 2 && nd != 3) || !device_ids || ndev < 1) { g_tracker_error = "ftkx_tracker_create_multi: bad arguments"; return FTKX_E_INVALID; }
  return create_handle(out, nd, [&] { return new ftkx::critical_point_tracker_regular(nd, std::vector<int>(device_ids, device_ids + ndev), block); });
}

int ftkx_tracker_sync(ftkx_tracker *h) { return guarded(h, [&] { h->t->sync(); }); }

void ftkx_tracker_destroy(ftkx_tracker *h) { if (h) { delete h->t; delete h; } }

int ftkx_tracker_last_error(const ftkx_tracker *h, char *buf, size_t n)
{
  const std::string &e = h ? h->err : g_tracker_error;
  if (buf && n) { strncpy(buf, e.c_str(), n - 1); buf[n - 1] = 0; }
  return (int)e.size();
}

int ftkx_tracker_set_domain(ftkx_tracker *h, const long long *st, const long long *sz)
{ return guarded(h, [&] { h->t->set_domain(ftkx::lattice(std::vector<long long>(st, st + h->nd), std::vector<long long>(sz, sz + h->nd))); }); }
int ftkx_tracker_set_array_domain(ftkx_tracker *h, const long long *st, const long long *sz)
{ return guarded(h, [&] { h->t->set_array_domain(ftkx::lattice(std::vector<long long>(st, st + h->nd), std::vector<long long>(sz, sz + h->nd))); }); }
int ftkx_tracker_set_sources(ftkx_tracker *h, int s, int v, int j, int sym)
{ return guarded(h, [&] { h->t->set_scalar_field_source(s); h->t->set_vector_field_source(v); h->t->set_jacobian_field_source(j); h->t->set_jacobian_symmetric(sym != 0); }); }
int ftkx_tracker_set_flags(ftkx_tracker *h, int robust, int use_tf, unsigned tf, int degrees, int exact_only, int tag_mode)
{
  return guarded(h, [&] {
    h->t->set_enable_robust_detection(robust != 0);
    if (use_tf) h->t->set_type_filter(tf);
    h->t->set_enable_computing_degrees(degrees != 0);
    h->t->set_exact_only(exact_only != 0);
    h->t->set_tag_mode(tag_mode);
  });
}
int ftkx_tracker_set_stream(ftkx_tracker *h, void *s) { return guarded(h, [&] { h->t->set_stream(s); }); }
int ftkx_tracker_set_spatial_smoothing(ftkx_tracker *h, double sigma, int ksize) { return guarded(h, [&] { h->t->set_spatial_smoothing(sigma, ksize); }); }
int ftkx_tracker_set_vector_spatial_smoothing(ftkx_tracker *h, double sigma, int ksize) { return guarded(h, [&] { h->t->set_vector_spatial_smoothing(sigma, ksize); }); }
int ftkx_tracker_set_perturbation(ftkx_tracker *h, double sigma, unsigned long long seed) { return guarded(h, [&] { h->t->set_perturbation(sigma, seed); }); }
int ftkx_tracker_set_clamp(ftkx_tracker *h, int on, double lo, double hi) { return guarded(h, [&] { if (on) h->t->set_clamp(lo, hi); else h->t->unset_clamp(); }); }
int ftkx_tracker_set_temporal_smoothing(ftkx_tracker *h, double sigma, int ksize) { return guarded(h, [&] { h->t->set_temporal_smoothing(sigma, ksize); }); }
int ftkx_tracker_snapshots_from_last_push(const ftkx_tracker *h, int *n)
{ return guarded(h, [&] { if (!n) throw ftkx::ftkx_error(FTKX_E_INVALID, "null argument"); *n = h->t->snapshots_from_last_push(); }); }
int ftkx_tracker_reset(ftkx_tracker *h) { return guarded(h, [&] { h->t->reset(); }); }
int ftkx_tracker_flush_temporal_smoothing(ftkx_tracker *h, int *appended)
{ return guarded(h, [&] { const bool b = h->t->flush_temporal_smoothing(); if (appended) *appended = b ? 1 : 0; }); }
int ftkx_tracker_set_trace_on_device(ftkx_tracker *h, int on) { return guarded(h, [&] { h->t->set_trace_on_device(on != 0); }); }
int ftkx_tracker_set_post_process_on_device(ftkx_tracker *h, int on) { return guarded(h, [&] { h->t->set_post_process_on_device(on != 0); }); }
int ftkx_tracker_set_sampling_in_pass(ftkx_tracker *h, int on) { return guarded(h, [&] { h->t->set_sampling_in_pass(on != 0); }); }
int ftkx_tracker_set_deferred_collection(ftkx_tracker *h, int on) { return guarded(h, [&] { h->t->set_deferred_collection(on != 0, on); }); }
int ftkx_tracker_set_communicator(ftkx_tracker *h, void *comm, int rank, int nranks, int nt) { return guarded(h, [&] { h->t->set_communicator(comm, rank, nranks, nt); }); }
int ftkx_tracker_set_slab_transport(ftkx_tracker *h, const ftkx_slab_transport *tr, int rank, int nranks, int nt)
{ return guarded(h, [&] { if (!tr) throw ftkx::ftkx_error(FTKX_E_INVALID, "null transport"); h->t->set_slab_transport(*tr, rank, nranks, nt); }); }
int ftkx_tracker_set_slab_hub(ftkx_tracker *h, ftkx_slab_hub *hub, int rank, int nt) { return guarded(h, [&] { h->t->set_slab_hub(hub, rank, nt); }); }
int ftkx_tracker_set_enable_streaming_trajectories(ftkx_tracker *h, int on) { return guarded(h, [&] { h->t->set_enable_streaming_trajectories(on != 0); }); }
int ftkx_tracker_set_current_timestep(ftkx_tracker *h, int t)
{ return guarded(h, [&] { if (t < 0) throw ftkx::ftkx_error(FTKX_E_INVALID, "set_current_timestep: negative timestep"); h->t->set_current_timestep(t); }); }
int ftkx_tracker_set_coords_bounds(ftkx_tracker *h, const double *b) { return guarded(h, [&] { h->t->set_coords_bounds(std::vector<double>(b, b + 2 * h->nd)); }); }
int ftkx_tracker_set_coords_rectilinear(ftkx_tracker *h, const double *x, size_t nx, const double *y, size_t ny, const double *z, size_t nz)
{
  return guarded(h, [&] {
    std::vector<std::vector<double>> c;
    c.emplace_back(x, x + nx); c.emplace_back(y, y + ny);
    if (h->nd == 3) c.emplace_back(z, z + nz);
    h->t->set_coords_rectilinear(c);
  });
}
int ftkx_tracker_set_coords_explicit(ftkx_tracker *h, const double *c, int ncomp, size_t n0, size_t n1)
{ return guarded(h, [&] { if (!c || ncomp < 2) throw ftkx::ftkx_error(FTKX_E_INVALID, "set_coords_explicit: bad arguments"); h->t->set_coords_explicit(c, ncomp, n0, n1); }); }
int ftkx_tracker_initialize(ftkx_tracker *h) { return guarded(h, [&] { h->t->initialize(); }); }
int ftkx_tracker_push_scalar_field_snapshot(ftkx_tracker *h, const double *s, int dev) { return guarded(h, [&] { h->t->push_scalar_field_snapshot(s, dev != 0); }); }
int ftkx_tracker_push_vector_field_snapshot(ftkx_tracker *h, const double *v, int dev) { return guarded(h, [&] { h->t->push_vector_field_snapshot(v, dev != 0); }); }
int ftkx_tracker_push_field_data_snapshot(ftkx_tracker *h, const double *s, const double *v, const double *j, int dev)
{ return guarded(h, [&] { h->t->push_field_data_snapshot(s, v, j, dev != 0); }); }
int ftkx_tracker_push_scalar_field_snapshot_f32(ftkx_tracker *h, const float *s, int dev) { return guarded(h, [&] { h->t->push_scalar_field_snapshot(s, dev != 0); }); }
int ftkx_tracker_push_vector_field_snapshot_f32(ftkx_tracker *h, const float *v, int dev) { return guarded(h, [&] { h->t->push_vector_field_snapshot(v, dev != 0); }); }
int ftkx_tracker_push_field_data_snapshot_f32(ftkx_tracker *h, const float *s, const float *v, const float *j, int dev)
{ return guarded(h, [&] { h->t->push_field_data_snapshot(s, v, j, dev != 0); }); }
int ftkx_tracker_push_scalar_field_snapshot_typed(ftkx_tracker *h, const void *s, int dtype, int dev) { return guarded(h, [&] { h->t->push_scalar_field_snapshot(s, dtype, dev != 0); }); }
int ftkx_tracker_push_vector_field_snapshot_typed(ftkx_tracker *h, const void *v, int dtype, int dev) { return guarded(h, [&] { h->t->push_vector_field_snapshot(v, dtype, dev != 0); }); }
int ftkx_tracker_push_field_data_snapshot_typed(ftkx_tracker *h, const void *s, const void *v, const void *j, int dtype, int dev)
{ return guarded(h, [&] { h->t->push_field_data_snapshot(s, v, j, dtype, dev != 0); }); }
int ftkx_tracker_push_vector_field_components(ftkx_tracker *h, const double *const *comps, int nc, int dev)
{ return guarded(h, [&] { h->t->push_vector_field_components(comps, nc, dev != 0); }); }
int ftkx_tracker_push_vector_field_components_f32(ftkx_tracker *h, const float *const *comps, int nc, int dev)
{ return guarded(h, [&] { h->t->push_vector_field_components(comps, nc, dev != 0); }); }
int ftkx_tracker_advance_timestep(ftkx_tracker *h) { return guarded(h, [&] { h->t->advance_timestep(); }); }
int ftkx_tracker_update_timestep(ftkx_tracker *h) { return guarded(h, [&] { h->t->update_timestep(); }); }

int ftkx_tracker_num_critical_points(const ftkx_tracker *h, size_t *n)
{
  if (!n) return FTKX_E_INVALID;
  return guarded(h, [&] { *n = h->t->num_discrete_critical_points(); });
}

int ftkx_tracker_get_critical_points(const ftkx_tracker *h, ftkx_cp_t *out, int *ordinal, int *timestep, size_t cap)
{
  if (!h || !h->t || !out) return FTKX_E_INVALID;
  size_t i = 0;
  std::vector<ftkx::feature_point_t> pts;
  const int rc = guarded(h, [&] { pts = h->t->get_critical_points(); });
  if (rc) return rc;
  for (const ftkx::feature_point_t &cp : pts) {
    if (i >= cap) break;
    std::memset(&out[i], 0, sizeof(ftkx_cp_t));
    for (int k = 0; k < 3; k ++) { out[i].x[k] = cp.x[k]; out[i].scalar[k] = cp.scalar[k]; }
    out[i].t = cp.t; out[i].type = cp.type; out[i].tag = cp.tag;
    if (ordinal) ordinal[i] = cp.ordinal;
    if (timestep) timestep[i] = cp.timestep;
    i ++;
  }
  return FTKX_OK;
}

int ftkx_tracker_get_scaling(const ftkx_tracker *h, unsigned long long *factor, double *resolution)
{
  // (a getter waits for what is still out -- a several-device tracker's queues, a slab's pass: whatever that raises is the call's error)
  return guarded(h, [&] {
    if (factor) *factor = h->t->get_vector_field_scaling_factor();
    if (resolution) *resolution = h->t->get_vector_field_resolution();
  });
}

int ftkx_tracker_finalize(ftkx_tracker *h) { return guarded(h, [&] { h->t->finalize(); }); }

int ftkx_tracker_num_curves(const ftkx_tracker *h, size_t *n_curves, size_t *n_points)
{
  if (!h || !h->t || !n_curves || !n_points) return FTKX_E_INVALID;
  *n_curves = h->t->num_traced_curves();
  *n_points = h->t->get_traced_points().size();
  return FTKX_OK;
}

int ftkx_tracker_get_curves(const ftkx_tracker *h, long long *offsets, unsigned long long *tags, int *loop)
{
  if (!h || !h->t || !offsets || !tags || !loop) return FTKX_E_INVALID;
  const auto &pts = h->t->get_traced_points();
  const auto &off = h->t->get_traced_offsets();
  for (size_t k = 0; k < pts.size(); k ++) tags[k] = pts[k].tag;
  for (size_t i = 0; i < off.size(); i ++) offsets[i] = off[i];
  for (size_t i = 0; i + 1 < off.size(); i ++) loop[i] = h->t->get_traced_loop_flags()[i];
  return FTKX_OK;
}

int ftkx_tracker_post_process(ftkx_tracker *h) { return guarded(h, [&] { h->t->post_process(); }); }

int ftkx_tracker_get_curve_points(const ftkx_tracker *h, unsigned int *type, double *t, int *ids)
{
  if (!h || !h->t) return FTKX_E_INVALID;
  const auto &pts = h->t->get_traced_points();
  for (size_t k = 0; k < pts.size(); k ++) { if (type) type[k] = pts[k].type; if (t) t[k] = pts[k].t; }
  if (ids) for (size_t i = 0; i < h->t->num_traced_curves(); i ++) ids[i] = h->t->get_traced_ids()[i];
  return FTKX_OK;
}

int ftkx_tracker_get_curve_scalars(const ftkx_tracker *h, double *scalars)
{
  if (!h || !h->t || !scalars) return FTKX_E_INVALID;
  const auto &pts = h->t->get_traced_points();
  for (size_t k = 0; k < pts.size(); k ++) for (int s = 0; s < 3; s ++) scalars[3 * k + s] = pts[k].scalar[s];
  return FTKX_OK;
}

int ftkx_tracker_set_scalar_components(ftkx_tracker *h, const char *const *names, int n)
{
  return guarded(h, [&] {
    if (!names || n < 1 || n > 3) throw ftkx::ftkx_error(FTKX_E_INVALID, "ftkx_tracker_set_scalar_components: one to three names");
    std::vector<std::string> v;
    for (int i = 0; i < n; i ++) { if (!names[i]) throw ftkx::ftkx_error(FTKX_E_INVALID, "ftkx_tracker_set_scalar_components: null name"); v.push_back(names[i]); }
    h->t->set_scalar_components(v);
  });
}

int ftkx_tracker_push_snapshot_extra(ftkx_tracker *h, int kind, const void *s, const void *v, const void *j, const void *const *extra, int n_extra, int dev, int f32)
{
  return guarded(h, [&] {
    ftkx::critical_point_tracker_regular &t = *h->t;
    if (kind < 0 || kind > 2) throw ftkx::ftkx_error(FTKX_E_INVALID, "ftkx_tracker_push_snapshot_extra: kind 0, 1 or 2");
    if (f32) {
      const float *const *e = reinterpret_cast<const float *const *>(extra);
      if (kind == 0) t.push_scalar_field_snapshot(static_cast<const float *>(s), e, n_extra, dev != 0);
      else if (kind == 1) t.push_vector_field_snapshot(static_cast<const float *>(v), e, n_extra, dev != 0);
      else t.push_field_data_snapshot(static_cast<const float *>(s), static_cast<const float *>(v), static_cast<const float *>(j), e, n_extra, dev != 0);
    } else {
      const double *const *e = reinterpret_cast<const double *const *>(extra);
      if (kind == 0) t.push_scalar_field_snapshot(static_cast<const double *>(s), e, n_extra, dev != 0);
      else if (kind == 1) t.push_vector_field_snapshot(static_cast<const double *>(v), e, n_extra, dev != 0);
      else t.push_field_data_snapshot(static_cast<const double *>(s), static_cast<const double *>(v), static_cast<const double *>(j), e, n_extra, dev != 0);
    }
  });
}

int ftkx_tracker_write(const ftkx_tracker *h, const char *path, int format, int traced)
{
  if (!path) return FTKX_E_INVALID;
  return guarded(h, [&] {
    const std::string f(path);
    const ftkx::critical_point_tracker_regular &t = *h->t;
    if (format == FTKX_FORMAT_JSON) { if (traced) t.write_traced_critical_points_json(f); else t.write_critical_points_json(f); }
    else if (format == FTKX_FORMAT_TEXT) { if (traced) t.write_traced_critical_points_text(f); else t.write_critical_points_text(f); }
    else if (format == FTKX_FORMAT_BINARY) { if (traced) t.write_traced_critical_points_binary(f); else t.write_critical_points_binary(f); }
    else throw ftkx::ftkx_error(FTKX_E_INVALID, "ftkx_tracker_write: unknown format");
  });
}

int ftkx_tracker_read_critical_points(ftkx_tracker *h, const char *path, int format)
{
  if (!path) return FTKX_E_INVALID;
  return guarded(h, [&] {
    if (format == FTKX_FORMAT_JSON) h->t->read_critical_points_json(path);
    else if (format == FTKX_FORMAT_BINARY) h->t->read_critical_points_binary(path);
    else throw ftkx::ftkx_error(FTKX_E_UNSUPPORTED, "ftkx_tracker_read_critical_points: json or binary");
  });
}

int ftkx_tracker_get_stats(const ftkx_tracker *h, ftkx_stats *st)
{
  if (!st) return FTKX_E_INVALID;
  return guarded(h, [&] { *st = h->t->get_last_stats(); });
}

int ftkx_tracker_trace_last_path(const ftkx_tracker *h) { return h && h->t ? ftkx_trace_last_path(h->t->context()) : 0; }
int ftkx_tracker_post_process_last_path(const ftkx_tracker *h) { return h && h->t ? ftkx_post_process_last_path(h->t->context()) : 0; }

}  // extern "C"
