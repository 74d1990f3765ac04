// The batched sweep: ftkx_sweep_enqueue / ftkx_sweep_collect (masks where missing -> cull -> exact test -> records -> device sort ->
// download) and the kernel timing that goes with it.  Reference counterpart: the per-call host wrapper extract_cp2dt<scope> /
// extract_cp3dt<scope> (src/filters/critical_point_tracer_2d_regular.cu:168-272, ..._3d_regular.cu:144-250).
#include "ctx.hpp"
#include "cp_device.hpp"   // classify3 on the HOST (fragile 3D records, see there)

using namespace ftkxh;

namespace ftkxh {

// types re-computed on the host written back into the hit buffer: pairs (slot, type)
__global__ void patch_types_kernel(ftkx_cp_t *hits, const u64 *__restrict__ pairs, size_t n)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) hits[pairs[2 * i]].type = (unsigned)pairs[2 * i + 1];
}

__global__ void sort_keys_kernel(const ftkx_cp_t *__restrict__ hits, size_t n, u64 *__restrict__ keys, unsigned *__restrict__ idx)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { keys[i] = hits[i].tag; idx[i] = (unsigned)i; }
}

__global__ void sort_gather_kernel(const ftkx_cp_t *__restrict__ hits, const unsigned *__restrict__ idx, size_t n, ftkx_cp_t *__restrict__ out)
{
  // 72-byte records moved as nine 8-byte words by nine consecutive lanes: coalesced stores
  const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < n * 9) {
    const size_t r = w / 9, k = w % 9;
    reinterpret_cast<u64 *>(out)[w] = reinterpret_cast<const u64 *>(hits)[(size_t)idx[r] * 9 + k];
  }
}

// ---- the records of a batch in tag order: a radix sort of (tag, index) pairs, least significant digit first ---------------------------
// 4-bit digits, three launches per digit: per-tile digit counts, ONE exclusive scan over (digit, tile), a stable scatter.  A tile is
// 256 threads x 8 consecutive keys each; inside it a key's place among its digit's keys = the keys of that digit in the threads before
// (a prefix over per-thread counts in LDS) + those before it in its own thread -- stable without a single atomic.  Only the digits a tag
// of this batch can have take part (key_bits).  This is the host-driven batch's ordering step (the device-driven pass orders by buckets,
// series_kernels.hip); rounds 1-3 called hipcub::DeviceRadixSort here.
constexpr int kRsThreads = 256, kRsPer = 8, kRsTile = kRsThreads * kRsPer;

__global__ __launch_bounds__(kRsThreads) void rs_count_kernel(const u64 *__restrict__ keys, size_t n, int shift, unsigned *__restrict__ counts, unsigned ntiles)
{
  __shared__ unsigned s_cnt[16];
  if (threadIdx.x < 16) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * kRsTile;
  for (int e = 0; e < kRsPer; e ++) {
    const size_t i = base + (size_t)e * kRsThreads + threadIdx.x;
    if (i < n) atomicAdd(&s_cnt[(unsigned)(keys[i] >> shift) & 15u], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 16) counts[(size_t)threadIdx.x * ntiles + blockIdx.x] = s_cnt[threadIdx.x];
}

// exclusive scan in place, one workgroup: a thread's contiguous share serially, the shares' totals by wavefront and through LDS
__global__ __launch_bounds__(1024) void rs_scan_kernel(unsigned *__restrict__ v, unsigned n)
{
  __shared__ unsigned s_wave[16];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const unsigned per = (n + 1023u) / 1024u, lo = tid * per, hi = lo + per < n ? lo + per : n;
  unsigned sum = 0;
  for (unsigned i = lo; i < hi; i ++) sum += v[i];
  unsigned incl = sum;
  for (int o = 1; o < 64; o <<= 1) { const unsigned up = __shfl_up(incl, o); if ((int)lane >= o) incl += up; }
  if (lane == 63u) s_wave[wv] = incl;
  __syncthreads();
  unsigned run = incl - sum;
  for (unsigned q = 0; q < wv; q ++) run += s_wave[q];
  for (unsigned i = lo; i < hi; i ++) { const unsigned c = v[i]; v[i] = run; run += c; }
}

__global__ __launch_bounds__(kRsThreads) void rs_scatter_kernel(const u64 *__restrict__ keys, const unsigned *__restrict__ idx, size_t n, int shift,
                                                                const unsigned *__restrict__ offs, unsigned ntiles, u64 *__restrict__ keys_out, unsigned *__restrict__ idx_out)
{
  __shared__ unsigned short s_cnt[16][kRsThreads];          // column t: thread t's keys per digit, then its first place per digit inside the tile
  __shared__ unsigned s_base[16];
  const unsigned tid = threadIdx.x;
  const size_t first = (size_t)blockIdx.x * kRsTile + (size_t)tid * kRsPer;      // this thread's eight consecutive keys
  u64 k[kRsPer];
  unsigned v[kRsPer];
  for (int d = 0; d < 16; d ++) s_cnt[d][tid] = 0;
  for (int e = 0; e < kRsPer; e ++) {
    const size_t i = first + (size_t)e;
    k[e] = 0ull; v[e] = 0u;
    if (i < n) { k[e] = keys[i]; v[e] = idx[i]; s_cnt[(unsigned)(k[e] >> shift) & 15u][tid] ++; }
  }
  if (tid < 16) s_base[tid] = offs[(size_t)tid * ntiles + blockIdx.x];
  __syncthreads();
  {
    // exclusive prefix over the 256 threads, per digit: thread (d, seg) = (tid / 16, tid % 16) walks sixteen columns, the sixteen
    // segments of a digit are sixteen consecutive lanes
    const unsigned d = tid >> 4, seg = tid & 15u;
    unsigned sum = 0;
    for (unsigned j = 0; j < 16; j ++) sum += s_cnt[d][seg * 16u + j];
    unsigned incl = sum;
    for (int o = 1; o < 16; o <<= 1) { const unsigned up = __shfl_up(incl, o, 16); if ((int)seg >= o) incl += up; }
    unsigned run = incl - sum;
    for (unsigned j = 0; j < 16; j ++) { const unsigned c = s_cnt[d][seg * 16u + j]; s_cnt[d][seg * 16u + j] = (unsigned short)run; run += c; }
  }
  __syncthreads();
  for (int e = 0; e < kRsPer; e ++) {
    if (first + (size_t)e < n) {
      const unsigned d = (unsigned)(k[e] >> shift) & 15u;
      const size_t at = (size_t)s_base[d] + (size_t)(s_cnt[d][tid] ++);
      keys_out[at] = k[e]; idx_out[at] = v[e];
    }
  }
}

// the reference keeps hits in a std::map ordered by element; device append order is arbitrary
int sort_hits_on_device(ftkx_ctx *c, size_t n, int key_bits)
{
  if (n == 0) return FTKX_OK;                                // (no tiles: nothing to launch)
  if (n >= (size_t)1 << 31) return fail(c, FTKX_E_UNSUPPORTED, "sort_hits_on_device: %zu records (indices are 32-bit)", n);
  const size_t room = n + n / 4 + 1024;
  auto tile_counts = [](size_t records) { return 16 * ((records + kRsTile - 1) / kRsTile) * sizeof(unsigned); };      // digit counts per tile
  int rc;
  if ((rc = c->d_sorted.reserve(c, n * sizeof(ftkx_cp_t), room * sizeof(ftkx_cp_t))) || (rc = c->d_keys.reserve(c, 2 * n * sizeof(u64), 2 * room * sizeof(u64))) ||
      (rc = c->d_idx.reserve(c, 2 * n * sizeof(unsigned), 2 * room * sizeof(unsigned))) || (rc = c->d_sort_tmp.reserve(c, tile_counts(n), tile_counts(room)))) return rc;
  const size_t cap = std::min(c->d_keys.count<u64>(), c->d_idx.count<unsigned>()) / 2;      // where the second half of the ping-pong buffers starts: n or more
  hipLaunchKernelGGL(sort_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_hits.as<ftkx_cp_t>(), n, c->d_keys.as<u64>(), c->d_idx.as<unsigned>());
  const unsigned ntiles = (unsigned)((n + kRsTile - 1) / kRsTile);
  unsigned *counts = (unsigned *)c->d_sort_tmp.p;
  int from = 0;                                              // which half of the ping-pong buffers holds the pairs
  for (int shift = 0; shift < key_bits; shift += 4) {
    const u64 *kin = c->d_keys.as<u64>() + (from ? cap : 0);
    const unsigned *iin = c->d_idx.as<unsigned>() + (from ? cap : 0);
    u64 *kout = c->d_keys.as<u64>() + (from ? 0 : cap);
    unsigned *iout = c->d_idx.as<unsigned>() + (from ? 0 : cap);
    hipLaunchKernelGGL(rs_count_kernel, dim3(ntiles), dim3(kRsThreads), 0, c->stream, kin, n, shift, counts, ntiles);
    hipLaunchKernelGGL(rs_scan_kernel, dim3(1), dim3(1024), 0, c->stream, counts, 16u * ntiles);
    hipLaunchKernelGGL(rs_scatter_kernel, dim3(ntiles), dim3(kRsThreads), 0, c->stream, kin, iin, n, shift, counts, ntiles, kout, iout);
    from ^= 1;
  }
  hipLaunchKernelGGL(sort_gather_kernel, dim3((unsigned)((n * 9 + 255) / 256)), dim3(256), 0, c->stream, c->d_hits.as<ftkx_cp_t>(), c->d_idx.as<unsigned>() + (from ? cap : 0), n, c->d_sorted.as<ftkx_cp_t>());
  HIP_TRY(c, hipGetLastError());
  return FTKX_OK;
}

// (events are recycled: creating and destroying a pair per kernel cost a hit-dense 2D pass several per cent)
hipEvent_t ev_take(ftkx_ctx *c)
{
  if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}
void ev_give(ftkx_ctx *c, hipEvent_t e) { if (e) c->event_pool.push_back(e); }
void ev_begin(ftkx_ctx *c, int kind)
{
  c->ev_open = false;
  if (!c->profiling || (c->profiling == 2 && kind != K_MASK)) return;     // level 2: the dominant kernel only (an event pair costs the stream ~10 us of idle time)
  hipEvent_t a = ev_take(c), b = ev_take(c);
  if (!a || !b) { ev_give(c, a); ev_give(c, b); return; }
  (void)hipEventRecord(a, c->stream);
  c->events.push_back({kind, {a, b}});
  c->ev_open = true;
}
void ev_end(ftkx_ctx *c)
{
  if (!c->profiling || !c->ev_open || c->events.empty()) return;
  c->ev_open = false;
  (void)hipEventRecord(c->events.back().second.second, c->stream);
}
void ev_harvest(ftkx_ctx *c, bool all)
{
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> later;
  for (auto &e : c->events) {
    if (!all && hipEventQuery(e.second.second) != hipSuccess) { later.push_back(e); continue; }
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.second.first, e.second.second) == hipSuccess) { c->k_ms[e.first] += ms; c->k_launches[e.first] ++; }
    ev_give(c, e.second.first); ev_give(c, e.second.second);
  }
  c->events.swap(later);
}

void ev_drop(ftkx_ctx *c) { for (auto &e : c->events) { ev_give(c, e.second.first); ev_give(c, e.second.second); } c->events.clear(); }

int read_counters(ftkx_ctx *c)
{
  HIP_TRY(c, hipMemcpyAsync(c->h_counters.p, c->sr_tail[0].counters.as<u64>(), ftkx::CNT_N * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FTKX_OK;
}

// ---- the host-driven batch: gather -> plan_batch (batch_plan.hpp) -> stage -> queue -> commit -------------------------------------------
namespace {
// the slices the pending requests read, each once, and the requests in terms of them
struct BatchInput { std::vector<Slice *> slice; std::vector<SliceFacts> facts; std::vector<BatchRequest> requests; };

void gather_batch(ftkx_ctx *c, BatchInput &in)
{
  std::map<int, int> index;
  auto at = [&](int t) {
    const auto ins = index.emplace(t, (int)in.slice.size());
    if (ins.second) { Slice &s = c->slices[t]; in.slice.push_back(&s); in.facts.push_back(slice_facts(s)); }
    return ins.first->second;
  };
  for (const Request &r : c->pending) {
    const int s0 = at(r.t);
    in.requests.push_back(BatchRequest{r.mode, s0, (r.scope & FTKX_SCOPE_INTERVAL) ? at(r.t + 1) : -1, r.factor});
  }
}

// everything the plan needs in memory: mask arrays of the slices it builds, the descriptor block, filled, the tile kernels' statistics
int stage_batch(ftkx_ctx *c, const Mesh &m, bool two_level, const BatchInput &in, const BatchPlan &P)
{
  for (const BatchSub &sb : P.subs)
    for (const BatchMaskJob &j : sb.jobs)
      if (const int rc = ensure_mask_arrays(c, *in.slice[j.slice], two_level)) return rc;
  if (!P.runs.empty()) {
    bool fresh = false;
    if (const int rc = c->d_tile_stats.reserve(c, 512 * sizeof(u64), 0, nullptr, &fresh)) return rc;
    if (fresh) HIP_TRY(c, hipMemsetAsync(c->d_tile_stats.p, 0, 512 * sizeof(u64), c->stream));
  }
  if (!P.bytes) return FTKX_OK;
  if (const int rc = ensure_desc(c, P.bytes)) return rc;
  auto fields_of = [&](int i, bool fast) {
    const Request &r = c->pending[i];
    const int of[2] = {in.requests[i].s0, in.requests[i].s1};
    Fields f;
    memset(&f, 0, sizeof(f));
    f.factor = (double)r.factor; f.t = r.t; f.scope_mask = r.scope;
    for (int k = 0; k < 2; k ++) {
      if (of[k] < 0) continue;
      const Slice &s = *in.slice[of[k]];
      f.S[k] = s.S.as<double>(); f.V[k] = s.V.as<double>(); f.J[k] = s.J.as<double>();
      if (fast) { f.M[k] = s.M.as<unsigned char>(); f.U[k] = two_level ? s.U.as<unsigned char>() : nullptr; }
    }
    return f;
  };
  char *h = (char *)c->h_desc.p;
  Fields *hf = (Fields *)(h + P.fields_off);
  for (size_t i = 0; i < P.subs.size(); i ++) {
    MaskJob *hj = (MaskJob *)(h + P.job_off[i]);
    for (const BatchMaskJob &j : P.subs[i].jobs) {
      const Slice &s = *in.slice[j.slice];
      *hj ++ = with_lean_thresholds(MaskJob{s.S.as<double>(), s.V.as<double>(), s.M.as<unsigned char>(), two_level ? s.U.as<unsigned char>() : nullptr, nullptr, 1.0 / (double)j.factor, j.big}, m);
    }
    Fields *hs = hf + P.step_base[i];
    for (int r : P.subs[i].steps) *hs ++ = fields_of(r, true);
  }
  for (size_t k = 0; k < P.tile_steps.size(); k ++) hf[P.tile_base + k] = fields_of(P.tile_steps[k], false);
  return FTKX_OK;
}

// the whole batch onto the context's stream, in one go; counters must have been zeroed
int queue_batch(ftkx_ctx *c, const Mesh &m, bool two_level, const BatchPlan &P, const double *sparse_field, bool cull_done)
{
  const bool cull_only = sparse_field != nullptr;
  ftkx_tail_set &T = c->sr_tail[0];
  if (P.bytes) HIP_TRY(c, hipMemcpyAsync(c->d_desc.p, c->h_desc.p, P.bytes, hipMemcpyHostToDevice, c->stream));
  const Fields *d_fields = (const Fields *)((char *)c->d_desc.p + P.fields_off);
  for (size_t i = 0; i < P.subs.size(); i ++) {
    const BatchSub &sb = P.subs[i];
    if (sb.steps.empty()) continue;
    const MaskJob *d_jobs = (const MaskJob *)((char *)c->d_desc.p + P.job_off[i]);
    const Fields *d_steps = d_fields + P.step_base[i];
    if (!sb.jobs.empty()) { ev_begin(c, K_MASK); ftkx::launch_masks(m, d_jobs, (int)sb.jobs.size(), c->stream); ev_end(c); }
    // the survivor list is shared by the sub-batches of one collect: the exact kernel of sub-batch i must not re-test the
    // survivors of sub-batch i-1, so each sub-batch gets its own list segment by resetting the list counter in between
    if (i > 0) {
      HIP_TRY(c, hipMemsetAsync(T.counters.as<u64>() + ftkx::CNT_SURVIVOR_LIST, 0, sizeof(u64), c->stream));
      HIP_TRY(c, hipMemsetAsync(T.counters.as<u64>() + ftkx::CNT_REFINE_LIST, 0, sizeof(u64), c->stream));
    }
    if (!cull_done) {    // (cull-ahead, see ftkx_ctx::ahead: the survivor list of exactly these steps is on the device already)
      ev_begin(c, K_CULL);
      if (two_level) ftkx::launch_cull_two_level(m, d_steps, (int)sb.steps.size(), T.refine.as<u64>(), T.refine_capacity, T.list.as<u64>(), T.list_capacity, c->stream);
      else ftkx::launch_cull(m, d_steps, (int)sb.steps.size(), T.list.as<u64>(), T.list_capacity, c->stream);
      ev_end(c);
    }
    if (cull_only) {
      // (the exact kernel is what publishes the list peak; without it the host reads the list counter itself)
      ftkx::launch_sparse_cells(m, d_steps, T.list.as<u64>(), T.list_capacity, sparse_field, c->d_cells.as<u64>(), c->d_cells.count<u64>(), c->stream);
      continue;
    }
    ev_begin(c, K_EXACT); ftkx::launch_exact(m, d_steps, (int)P.step_base[i], T.list.as<u64>(), T.list_capacity, c->stream); ev_end(c);
  }
  if (cull_only) { HIP_TRY(c, hipGetLastError()); return FTKX_OK; }
  if (!P.runs.empty()) {
    TileParams p;
    p.m = m; p.repeat = c->tile_repeat; p.stats = c->d_tile_stats.as<u64>();
    int tile[3];
    ftkx::tile_dims(c->nd, tile);
    for (int d = 0; d < 3; d ++) p.ntiles[d] = d < c->nd ? (int)((c->core_sz[d] + tile[d] - 1) / tile[d]) : 1;
    for (const BatchTileRun &run : P.runs) {
      p.step = (int)P.tile_base + run.first; p.steps = d_fields + p.step; p.nsteps = run.nsteps;
      p.cull = run.cull; p.fan = run.fan; p.form = run.form;
      ev_begin(c, K_TILE); ftkx::launch_tile(p, c->stream); ev_end(c);
    }
    ftkx::launch_tile_stats_fold(c->d_tile_stats.as<u64>(), m.counters, c->stream);
  }
  // the FP64 half, once for the whole batch: records of every simplex that passed (timed with the kernel family that fed it)
  // (K_EXACT also behind tile requests: K_TILE is the integer test of every simplex and nothing else -- bench.py's int-VALU figure)
  if (P.nfields) { ev_begin(c, K_EXACT); ftkx::launch_records(m, d_fields, c->stream); ev_end(c); }
  HIP_TRY(c, hipGetLastError());
  return FTKX_OK;
}
}  // namespace

// Launches everything the pending requests need.  What the slices say of their masks changes once the whole batch has been queued --
// one uninterrupted sequence on one stream, so "built" then holds for everything queued later -- and not before: a batch that is
// refused, or cannot get its memory, leaves every slice as it was; one that fails between launches leaves the masks it meant to
// build marked as not built.
int run_batch(ftkx_ctx *c, const double *sparse_field, bool cull_done)
{
  Mesh m;
  fill_mesh(c, m);
  const bool two_level = ftkx::masks_have_summary(m);
  BatchInput in;
  gather_batch(c, in);
  // (test hooks, read per batch: 0 = a tile launch per step; the tile kernel's fan)
  const char *walk = getenv("FTKX_TILE_WALK"), *fan = getenv("FTKX_TILE_FAN");
  const BatchPlan P = plan_batch(BatchMesh{c->nd, m.robust != 0, two_level, m.u_rows}, in.requests, in.facts, BatchKnobs{!(walk && atoi(walk) == 0), fan ? atoi(fan) : 2});
  if (P.status == BATCH_SPARSE_CANNOT_SERVE)
    return fail(c, FTKX_E_NOSLICE, "sweep: the masks of halo slice (masks only) do not serve factor %llu: send the slice itself", c->pending[P.refused].factor);
  if (P.status == BATCH_TOO_MANY) return fail(c, FTKX_E_INVALID, "sweep: too many requests in one batch (%zu)", P.nfields);
  if (sparse_field && (P.subs.size() > 1 || !P.runs.empty()))      // ftkx_sweep_cull: one cull, whose survivors that read `sparse_field` are listed
    return fail(c, FTKX_E_UNSUPPORTED, "ftkx_sweep_cull: the batch needs masks under two factors or the tile path (send the slice itself)");
  if (cull_done && (P.subs.size() != 1 || !P.subs[0].jobs.empty())) return fail(c, FTKX_E_DEVICE, "internal: cull-ahead taken over by a batch that rebuilds masks");
  if (const int rc = stage_batch(c, m, two_level, in, P)) return rc;
  const int rc = queue_batch(c, m, two_level, P, sparse_field, cull_done);
  for (const BatchSub &sb : P.subs)
    for (const BatchMaskJob &j : sb.jobs) {
      Slice &s = *in.slice[j.slice];
      const SliceFacts &f = P.facts[j.slice];
      if (rc) s.mask_factor = 0;
      else { s.mask_factor = f.mask_factor; s.mask_big = f.mask_big; s.u_rows = f.u_rows; }
    }
  return rc;
}

// ---- ftkx_sweep_collect's stages --------------------------------------------------------------------------------------------------------
namespace {
// the buffers a batch writes: at their first sizes, or as earlier batches left them
int collect_reserve(ftkx_ctx *c, bool any_fast)
{
  ftkx_tail_set &T = c->sr_tail[0];
  int rc;
  if ((rc = ensure_hit_buffer(c, std::max<u64>(c->capacity, 1u << 16)))) return rc;
  if (c->nd == 3 && (rc = ensure_fragile(c, T, std::max<u64>(T.fragile_capacity, 1u << 12)))) return rc;
  if (any_fast && (rc = ensure_list(c, T, std::max<u64>(T.list_capacity, 1u << 20)))) return rc;
  if (any_fast && (rc = ensure_refine(c, T, std::max<u64>(T.refine_capacity, 1u << 20)))) return rc;
  return FTKX_OK;
}

// the batch, and again while a buffer was too small (overflow_verdict, batch_plan.hpp); afterwards h_counters holds the counters of the run that fitted
int collect_attempts(ftkx_ctx *c, bool any_fast, u64 fast_cells, bool use_ahead)
{
  ftkx_tail_set &T = c->sr_tail[0];
  const u64 *hc = c->h_counters.as<u64>();
  for (int attempt = 0; ; attempt ++) {
    int rc;
    // (cull-ahead: the counters were zeroed before that cull and hold its list counts)
    if (!use_ahead) HIP_TRY(c, hipMemsetAsync(T.counters.as<u64>(), 0, ftkx::CNT_N * sizeof(u64), c->stream));
    if ((rc = run_batch(c, nullptr, use_ahead))) return rc;
    use_ahead = false;                                         // a replay culls afresh
    if ((rc = read_counters(c))) return rc;
    c->ahead_staged = false;
    // (records <= simplices that passed: the 2D type filter may drop some; the pass list shares the hit buffer's capacity)
    const BatchSizes n{std::max(hc[ftkx::CNT_HITS], hc[ftkx::CNT_PASS]), hc[ftkx::CNT_LIST_PEAK], hc[ftkx::CNT_REFINE_PEAK], hc[ftkx::CNT_FRAGILE]};
    const BatchSizes cap{c->capacity, T.list_capacity, T.refine_capacity, T.fragile_capacity};
    const BatchVerdict v = overflow_verdict(n, cap, any_fast, fast_cells, attempt);
    if (v.what == BATCH_DONE) { ev_harvest(c); return FTKX_OK; }
    ev_drop(c);
    if (v.what == BATCH_GIVE_UP) return fail(c, FTKX_E_DEVICE, "buffer overflow persisted after regrowing four times");
    if (v.what == BATCH_REPLAY_DENSE) {
      for (const Request &r : c->pending) {
        auto a = c->slices.find(r.t), b = c->slices.find(r.t + 1);
        if ((a != c->slices.end() && a->second.sparse) || ((r.scope & FTKX_SCOPE_INTERVAL) && b != c->slices.end() && b->second.sparse))
          return fail(c, FTKX_E_UNSUPPORTED, "sweep: most cells survive the cull and a masked halo slice is involved (send the slice itself)");
      }
      for (Request &r : c->pending) if (r.mode == MODE_FAST) r.mode = MODE_TILE_CULL;
      any_fast = false;
      c->dense_collects = 16;
    }
    if (v.want.fragile > cap.fragile && (rc = ensure_fragile(c, T, v.want.fragile))) return rc;
    if (v.want.refined > cap.refined && (rc = ensure_refine(c, T, v.want.refined))) return rc;
    if (v.want.listed > cap.listed && (rc = ensure_list(c, T, v.want.listed))) return rc;
    if (v.want.hits > cap.hits && (rc = ensure_hit_buffer(c, v.want.hits))) return rc;
  }
}

// 3D records whose class hangs on the last bits of pow / acos / cos (an eigenvalue of the Hessian that is zero up to rounding):
// classified again here, with the libm the reference itself runs on, and written back before the records are sorted.  Rare -- an
// exactly singular Hessian takes plateaus or lattice-aligned data -- and then one small round trip.
int reclassify_fragile(ftkx_ctx *c, u64 nf)
{
  std::vector<u64> frag((size_t)nf * 10), pairs((size_t)nf * 2);
  HIP_TRY(c, hipMemcpyAsync(frag.data(), c->sr_tail[0].fragile.as<u64>(), frag.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < (size_t)nf; i ++) {
    double A[3][3];
    memcpy(A, &frag[i * 10 + 1], sizeof(A));
    pairs[2 * i] = frag[i * 10];
    pairs[2 * i + 1] = (u64)ftkx::classify3(A, c->opt.jacobian_symmetric != 0);
  }
  if (const int rc = ensure_desc(c, pairs.size() * sizeof(u64))) return rc;
  memcpy(c->h_desc.p, pairs.data(), pairs.size() * sizeof(u64));
  HIP_TRY(c, hipMemcpyAsync(c->d_desc.p, c->h_desc.p, pairs.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(patch_types_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, c->stream, c->d_hits.as<ftkx_cp_t>(), (const u64 *)c->d_desc.p, (size_t)nf);
  HIP_TRY(c, hipGetLastError());
  c->stats.reclassified = nf;
  return FTKX_OK;
}

// the records into h_hits in tag order: sorted on the device where there are enough of them, by the host otherwise
int order_and_download(ftkx_ctx *c, size_t n, int key_bits)
{
  if (!n) return FTKX_OK;
  const bool on_device = n >= 4096 && n < (1ull << 31);
  if (on_device) { if (const int rc = sort_hits_on_device(c, n, key_bits)) return rc; }
  HIP_TRY(c, hipMemcpyAsync(c->h_hits.as<ftkx_cp_t>(), (on_device ? c->d_sorted : c->d_hits).as<ftkx_cp_t>(), n * sizeof(ftkx_cp_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (!on_device) std::sort(c->h_hits.as<ftkx_cp_t>(), c->h_hits.as<ftkx_cp_t>() + n, [](const ftkx_cp_t &a, const ftkx_cp_t &b) { return a.tag < b.tag; });
  return FTKX_OK;
}
}  // namespace

// may ftkx_sweep_collect take the cull-ahead's survivor list over?
bool ahead_serves_pending(const ftkx_ctx *c, const Mesh &m, bool two_level)
{
  if (c->ahead.empty() || c->ahead.size() != c->pending.size()) return false;
  for (size_t i = 0; i < c->pending.size(); i ++) {
    const Request &r = c->pending[i];
    const ftkx_ctx::AheadStep &a = c->ahead[i];
    if (r.t != a.t || r.scope != a.scope || r.mode != MODE_FAST) return false;
    auto s0 = c->slices.find(r.t);
    if (s0 == c->slices.end() || s0->second.M.p != a.M[0] || (two_level ? s0->second.U.p : nullptr) != a.U[0] || !masks_valid(c, s0->second, r.factor, two_level, m.u_rows)) return false;
    if (r.scope & FTKX_SCOPE_INTERVAL) {
      auto s1 = c->slices.find(r.t + 1);
      if (s1 == c->slices.end() || s1->second.M.p != a.M[1] || (two_level ? s1->second.U.p : nullptr) != a.U[1] || !masks_valid(c, s1->second, r.factor, two_level, m.u_rows)) return false;
    }
  }
  return true;
}

}  // namespace ftkxh

extern "C" {

int ftkx_sweep_enqueue(ftkx_ctx *c, int t, int scope, unsigned long long factor)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!c->mesh_set) return fail(c, FTKX_E_INVALID, "sweep: call ftkx_set_mesh first");
  if (c->sr_open && !c->sr_internal) return fail(c, FTKX_E_INVALID, "ftkx_sweep_enqueue: series passes open (ftkx_sweep_series_submit), complete them first");
  if (scope < FTKX_SCOPE_ORDINAL || scope > FTKX_SCOPE_BOTH) return fail(c, FTKX_E_INVALID, "sweep: bad scope %d", scope);
  if (scope == FTKX_SCOPE_BOTH && c->opt.tag_mode == FTKX_TAG_WORK_INDEX)
    return fail(c, FTKX_E_INVALID, "sweep: FTKX_SCOPE_BOTH needs an element tag (work indices of the two scopes collide)");
  if (factor == 0) return fail(c, FTKX_E_INVALID, "sweep: factor must be non-zero");
  auto it0 = c->slices.find(t);
  if (it0 == c->slices.end()) return fail(c, FTKX_E_NOSLICE, "sweep: slice %d not resident", t);
  Slice *s0 = &it0->second, *s1 = nullptr;
  if (scope & FTKX_SCOPE_INTERVAL) {
    auto it1 = c->slices.find(t + 1);
    if (it1 == c->slices.end()) return fail(c, FTKX_E_NOSLICE, "sweep: interval [%d, %d] needs slice %d", t, t + 1, t + 1);
    s1 = &it1->second;
  }
  if (s1 && ((s0->J.p == nullptr) != (s1->J.p == nullptr) || (s0->S.p == nullptr) != (s1->S.p == nullptr)))
    return fail(c, FTKX_E_INVALID, "sweep: slices %d and %d disagree on which of J / S are given", t, t + 1);
  // coordinate arrays are indexed by vertex coordinates: they must cover the vertex box
  if (c->opt.coords_mode == 2)
    for (int d = 0; d < c->nd; d ++)
      if (c->dom_st[d] < 0 || (size_t)(c->dom_st[d] + c->dom_sz[d]) > c->rect_n[d])
        return fail(c, FTKX_E_INVALID, "sweep: rectilinear coordinates of axis %d have %zu entries, vertices reach %lld", d, c->rect_n[d], c->dom_st[d] + c->dom_sz[d] - 1);
  if (c->opt.coords_mode == 3 && (c->dom_st[0] < 0 || c->dom_st[1] < 0 || (size_t)(c->dom_st[0] + c->dom_sz[0]) > c->expl_n0 || (size_t)(c->dom_st[1] + c->dom_sz[1]) > c->expl_n1))
    return fail(c, FTKX_E_INVALID, "sweep: explicit coordinates are %zu x %zu, the vertex box needs %lld x %lld", c->expl_n0, c->expl_n1, c->dom_st[0] + c->dom_sz[0], c->dom_st[1] + c->dom_sz[1]);
  for (int d = 0; d < c->nd; d ++)
    if (c->core_sz[d] == 0) return FTKX_OK;    // empty core: nothing to enumerate
  HIP_TRY(c, hipSetDevice(c->device));
  const int nd = c->nd;
  const int mode = request_mode(c->opt.exact_only != 0, factor, nd, c->opt.robust != 0, c->dense_collects);
  const bool fast = mode != MODE_TILE;          // the strict-sign cull is usable (as masks, or inside the tile kernel)
  if ((s0->sparse || (s1 && s1->sparse)) && sparse_slice_refuses(mode))
    return fail(c, FTKX_E_UNSUPPORTED, "sweep: a masked halo slice only serves sweeps that use the cull (send the slice itself)");
  if (c->pending.empty()) memset(&c->stats, 0, sizeof(c->stats));
  c->pending.push_back(Request{t, scope, factor, mode});

  u64 cells = 1;
  for (int d = 0; d < nd; d ++) cells *= (u64)c->core_sz[d];
  const u64 n_ord = nd == 2 ? 2 : 6, n_int = nd == 2 ? 10 : 54;
  c->stats.cells += cells;
  c->stats.work_items += cells * (((scope & 1) ? n_ord : 0) + ((scope & 2) ? n_int : 0));
  c->stats.cull_enabled = fast ? 1 : 0;
  return FTKX_OK;
}

int ftkx_sweep_collect(ftkx_ctx *c, const ftkx_cp_t **out, size_t *n_out)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  HIP_TRY(c, hipSetDevice(c->device));
  if (out) *out = nullptr;
  if (n_out) *n_out = 0;
  if (c->pending.empty()) return FTKX_OK;
  struct Forget { ftkx_ctx *c; ~Forget() { c->pending.clear(); } } forget{c};      // whichever way out: the batch is not pending afterwards
  bool any_fast = false;
  u64 fast_cells = 0;
  int t_max = 0;
  {
    u64 cells = 1;
    for (int d = 0; d < c->nd; d ++) cells *= (u64)c->core_sz[d];
    for (const Request &r : c->pending) {
      if (r.mode == MODE_FAST) { any_fast = true; fast_cells += cells; }
      t_max = std::max(t_max, r.t);
    }
  }
  int rc;
  if ((rc = collect_reserve(c, any_fast))) return rc;
  if (c->dense_collects > 0) c->dense_collects --;          // the fast path is probed again after a while
  const int sort_bits = key_bits(c->opt.tag_mode, c->nd, c->core_sz, c->dom_sz, t_max);
  bool use_ahead = false;
  if (!c->ahead.empty()) {
    Mesh m; fill_mesh(c, m);
    use_ahead = ahead_serves_pending(c, m, ftkx::masks_have_summary(m));
    c->ahead.clear();                                        // one use
  }
  if ((rc = collect_attempts(c, any_fast, fast_cells, use_ahead))) return rc;
  const u64 *hc = c->h_counters.as<u64>();
  const size_t n = (size_t)hc[ftkx::CNT_HITS];
  c->stats.hits = n;
  c->stats.cells_survived = hc[ftkx::CNT_CELLS_SURVIVED];
  c->stats.simplices_tested = hc[ftkx::CNT_SIMPLICES_TESTED];
  if ((rc = ensure_host_buffer(c, n))) return rc;
  if (hc[ftkx::CNT_FRAGILE] && (rc = reclassify_fragile(c, hc[ftkx::CNT_FRAGILE]))) return rc;
  if ((rc = order_and_download(c, n, sort_bits))) return rc;
  if (out) *out = c->h_hits.as<ftkx_cp_t>();
  if (n_out) *n_out = n;
  return FTKX_OK;
}

int ftkx_sweep_enqueue_many(ftkx_ctx *c, const int *ts, const int *scopes, const unsigned long long *factors, int n)
{
  if (!c || (n > 0 && (!ts || !scopes || !factors))) return fail(c, FTKX_E_INVALID, "null argument");
  for (int i = 0; i < n; i ++) { const int rc = ftkx_sweep_enqueue(c, ts[i], scopes[i], factors[i]); if (rc) { c->pending.clear(); return rc; } }
  return FTKX_OK;
}

int ftkx_sweep_cancel(ftkx_ctx *c)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  c->pending.clear();
  return FTKX_OK;
}

// test aid: the host-driven batch's ordering step on records of the caller's -- into the hit buffer, through sort_hits_on_device as
// ftkx_sweep_collect calls it, out of d_sorted
int ftkx_debug_sort_records(ftkx_ctx *c, const ftkx_cp_t *in, size_t n, int key_bits, ftkx_cp_t *out)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (key_bits < 1 || key_bits > 64) return fail(c, FTKX_E_INVALID, "ftkx_debug_sort_records: key_bits %d (1 .. 64)", key_bits);
  if (n == 0) return FTKX_OK;
  if (!in || !out) return fail(c, FTKX_E_INVALID, "ftkx_debug_sort_records: null argument");
  if (!c->pending.empty() || c->sr_open) return fail(c, FTKX_E_INVALID, "ftkx_debug_sort_records: sweeps pending or series passes open, collect them first");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  if (n > c->capacity && (rc = ensure_hit_buffer(c, n))) return rc;
  c->ahead.clear(); c->announced.clear();                    // (a cull queued ahead counted on the buffers as they were)
  HIP_TRY(c, hipMemcpyAsync(c->d_hits.as<ftkx_cp_t>(), in, n * sizeof(ftkx_cp_t), hipMemcpyHostToDevice, c->stream));
  if ((rc = sort_hits_on_device(c, n, key_bits))) return rc;
  HIP_TRY(c, hipMemcpyAsync(out, c->d_sorted.as<ftkx_cp_t>(), n * sizeof(ftkx_cp_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FTKX_OK;
}

int ftkx_sweep(ftkx_ctx *c, int t, int scope, unsigned long long factor, const ftkx_cp_t **out, size_t *n_out)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "ftkx_sweep: asynchronous sweeps pending, collect first");
  if (c->sr_open && !c->sr_internal) return fail(c, FTKX_E_INVALID, "ftkx_sweep: series passes open (ftkx_sweep_series_submit), complete them first");
  int rc = ftkx_sweep_enqueue(c, t, scope, factor);
  if (rc) return rc;
  return ftkx_sweep_collect(c, out, n_out);
}

}  // extern "C"
