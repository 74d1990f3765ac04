// Host side of the C ABI declared in include/ftkx.h: context, HBM-resident slices, launch bookkeeping, hit download.
// The reference's counterpart is the per-call host wrapper extract_cp2dt<scope> / extract_cp3dt<scope>
// (src/filters/critical_point_tracer_2d_regular.cu:168-272, ..._3d_regular.cu:144-250), which re-allocates, re-uploads and
// frees everything on every call and synchronises the whole device; here slices stay resident, launches go to a stream,
// and the hit buffer is persistent (grown and the batch replayed if a launch overflows it).
#include <atomic>
#include <map>
#include <mutex>
#include "ctx.hpp"
#include "cp_device.hpp"
#include "host_sort.hpp"
#include "relaunch.hpp"
#include <sched.h>

using namespace ftkxh;

namespace { thread_local std::string g_last_error; }

namespace ftkx { void set_global_error(const char *msg) { g_last_error = msg ? msg : ""; } }

namespace ftkx {
// Waits for a sequence number a kernel stores, with system scope, into coherent pinned memory.  A short spin (the common case: the
// value is microseconds away), then the core is given up between polls -- a multi-device tracker waits like this on one thread per
// device while the trace's worker pool may want the same cores -- and the stream is looked at once per millisecond, so that a queue
// that faulted or drained without the store is noticed promptly.  Returns nullptr, or what went wrong.
const char *wait_flag(const unsigned *flag, unsigned seq, hipStream_t stream)
{
  const auto t_start = std::chrono::steady_clock::now();
  auto t_poll = t_start;
  for (unsigned long long spins = 0; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq; spins ++) {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();                                  // (a spin-wait hint: the sibling hyperthread keeps its issue slots)
#endif
    if ((spins & 0x3ffull) != 0x3ffull) continue;
    const auto now = std::chrono::steady_clock::now();
    if (now - t_start > std::chrono::microseconds(200)) sched_yield();
    if (now - t_poll < std::chrono::milliseconds(1)) continue;
    t_poll = now;
    const hipError_t q = hipStreamQuery(stream);
    if (q != hipSuccess && q != hipErrorNotReady) return hipGetErrorString(q);
    if (q == hipSuccess && __atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) return "the stream drained without the result arriving";
    if (now - t_start > std::chrono::seconds(120)) return "timed out waiting for the device";
  }
  return nullptr;
}
}  // namespace ftkx

namespace ftkxh {

int fail(ftkx_ctx *c, int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  if (c) c->err = buf;
  return code;
}

const std::string &global_error() { return g_last_error; }

int settings_not_now(ftkx_ctx *c, const char *who)
{
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "%s: sweeps pending, collect first", who);
  if (c->sr_open && !c->sr_internal) return fail(c, FTKX_E_INVALID, "%s: series passes open (ftkx_sweep_series_submit), complete them first", who);
  return FTKX_OK;
}

size_t n_vertices(const ftkx_ctx *c)
{
  size_t n = 1;
  for (int d = 0; d < c->nd; d ++) n *= (size_t)c->ext_sz[d];
  return n;
}

int mask_pitch(const ftkx_ctx *c) { return (int)(((c->ext_sz[0] + 7) / 8) * 8 + 8); }
int u_pitch(const ftkx_ctx *c) { return (int)((((c->ext_sz[0] + 7) / 8 + 7) / 8) * 8 + 8); }
size_t u_bytes(const ftkx_ctx *c) { return (size_t)u_pitch(c) * (size_t)c->ext_sz[1] * (size_t)(c->nd == 3 ? c->ext_sz[2] : 1); }   // allocation (u_rows = 1)
// the part of a summary array that carries data: ceil(rows / u_rows) rows per plane, planes back to back
size_t u_bytes_used(const ftkx_ctx *c, const Mesh &m) { return (size_t)u_pitch(c) * (size_t)((c->ext_sz[1] + m.u_rows - 1) / m.u_rows) * (size_t)(c->nd == 3 ? c->ext_sz[2] : 1); }
size_t mask_bytes(const ftkx_ctx *c) { return (size_t)mask_pitch(c) * (size_t)c->ext_sz[1] * (size_t)(c->nd == 3 ? c->ext_sz[2] : 1); }

void release_slice(Slice &s, ftkx_ctx *c)
{
  // owned copies go back to the context's pool, each under its own bytes (ctx_block.hpp); lent arrays are let go
  for (ftkx_block *f : {&s.V, &s.J, &s.S}) c->arrays.give(FTKX_ARRAY_FIELD, std::move(*f), kPoolCap);
  c->arrays.give(FTKX_ARRAY_MASK, std::move(s.M), kPoolCap);
  c->arrays.give(FTKX_ARRAY_SUMMARY, std::move(s.U), kPoolCap);
  s = Slice();
}

void free_slice(Slice &s, ftkx_ctx *c)
{
  // The newest open pass is a SPLIT pass: its tail runs on a stream of its own and may still read this slice's arrays, while whatever takes
  // them out of the pools next -- a push, the mask kernel of the next pass -- runs on the context's stream, in no order with that tail.
  // The slice is parked with that pass and is released when it has been completed (series.hip, release_retired).
  if (c->sr_open > 0) {
    ftkx_series_pending &N = c->sr_pend[c->sr_place(c->sr_open - 1)];
    if (N.open && N.split) { N.parked.push_back(std::move(s)); s = Slice(); return; }
  }
  release_slice(s, c);
}

void release_retired(ftkx_ctx *c, ftkx_series_pending &P)
{
  // (no cap: a pass of 32 slices would free, and its successor allocate again, 40 arrays per pass)
  for (auto &mu : P.retired) { c->arrays.give(FTKX_ARRAY_MASK, std::move(mu.first)); c->arrays.give(FTKX_ARRAY_SUMMARY, std::move(mu.second)); }
  P.retired.clear();
  // (slices dropped while this pass was the newest one open: its tail is through, a pass queued behind it was planned after the drop)
  for (Slice &sl : P.parked) release_slice(sl, c);
  P.parked.clear();
  for (ftkx_block &b : P.parked_aux) c->arrays.give(FTKX_ARRAY_FIELD, std::move(b), kPoolCap);      // (the pass's sample kernel was on that tail)
  P.parked_aux.clear();
}

// ---- the tail sets (ctx.hpp) ---------------------------------------------------------------------------------------------------------
// An array of a set replaced by a larger one; contents are not kept.  Nothing of a set is freed while its stream may still read it: the stream is
// drained first.  (Set 0 grows only where everything has been waited for anyway; the synchronise costs the rare growth path a call.)
// The element counts the kernels are handed are read off the blocks here, on the line behind the reserve.
constexpr size_t kFragileBytes = 10 * sizeof(u64);      // (slot, J[9])
int ensure_pass(ftkx_ctx *c, ftkx_tail_set &S, u64 want) { const int rc = S.pass.reserve(c, want * sizeof(u64), 0, S.stream); S.capacity = S.pass.count<u64>(); return rc; }
int ensure_fragile(ftkx_ctx *c, ftkx_tail_set &S, u64 want) { const int rc = S.fragile.reserve(c, want * kFragileBytes, 0, S.stream); S.fragile_capacity = S.fragile.bytes / kFragileBytes; return rc; }
int ensure_list(ftkx_ctx *c, ftkx_tail_set &S, u64 want) { const int rc = S.list.reserve(c, want * sizeof(u64), 0, S.stream); S.list_capacity = S.list.count<u64>(); return rc; }
int ensure_refine(ftkx_ctx *c, ftkx_tail_set &S, u64 want) { const int rc = S.refine.reserve(c, want * sizeof(u64), 0, S.stream); S.refine_capacity = S.refine.count<u64>(); return rc; }
int ensure_bins(ftkx_ctx *c, ftkx_tail_set &S, u64 want)
{
  if (const int rc = S.hist.reserve(c, want * sizeof(unsigned), 0, S.stream)) return rc;
  return S.boff.reserve(c, want * sizeof(unsigned), 0, S.stream);
}
int ensure_order(ftkx_ctx *c, ftkx_tail_set &S, u64 want)
{
  if (const int rc = S.bucketed.reserve(c, want * sizeof(u64), 0, S.stream)) return rc;
  return S.sorted.reserve(c, want * sizeof(u64), 0, S.stream);
}

int ensure_hit_buffer(ftkx_ctx *c, u64 want)
{
  int rc = c->d_hits.reserve(c, want * sizeof(ftkx_cp_t));
  if (rc == FTKX_OK) rc = ensure_pass(c, c->sr_tail[0], want);
  c->capacity = rc == FTKX_OK ? c->d_hits.count<ftkx_cp_t>() : 0;
  return rc;
}

hipError_t sync_tails(ftkx_ctx *c)
{
  for (ftkx_tail_set &S : c->sr_tail)
    if (S.stream) { const hipError_t e = hipStreamSynchronize(S.stream); if (e != hipSuccess) return e; }
  return hipSuccess;
}

int ensure_desc(ftkx_ctx *c, size_t bytes)
{
  const size_t cap = std::max<size_t>(bytes, 1 << 16);
  if (const int rc = c->h_desc.reserve(c, bytes, cap)) return rc;
  return c->d_desc.reserve(c, bytes, cap);
}

int ensure_red(ftkx_ctx *c, size_t nslices) { return c->d_red.reserve(c, nslices * 128 * sizeof(u64)); }

// h_hits is non-coherent = ordinary cached host memory for the CPU (it only reads the records after a stream synchronise);
// the default coherent mapping is uncached on this platform and made every consumer crawl (5 GB/s)
int ensure_host_buffer(ftkx_ctx *c, size_t want) { return c->h_hits.reserve(c, want * sizeof(ftkx_cp_t), std::max<size_t>(want, 4096) * sizeof(ftkx_cp_t)); }

void fill_mesh(const ftkx_ctx *c, Mesh &m)
{
  memset(&m, 0, sizeof(m));
  const int nd = c->nd;
  m.nd = nd;
  for (int d = 0; d < 3; d ++) {
    m.dom_lb[d] = (int)c->dom_st[d]; m.dom_ub[d] = (int)(c->dom_st[d] + c->dom_sz[d] - 1);
    m.core_st[d] = (int)c->core_st[d]; m.core_sz[d] = (int)c->core_sz[d];
    m.ext_st[d] = (int)c->ext_st[d]; m.ext_sz[d] = (int)c->ext_sz[d];
  }
  // lattice::prod_ of the mesh lattice (lattice.hh:156-167) and simplicial_regular_mesh::dimprod_ (int; simplicial_regular_mesh.hh:930-947)
  m.mesh_prod[0] = 1; m.dimprod[0] = 1; m.exact_prod[0] = 1;
  for (int d = 1; d <= nd; d ++) {
    m.mesh_prod[d] = m.mesh_prod[d - 1] * (u64)c->dom_sz[d - 1];
    m.exact_prod[d] = m.exact_prod[d - 1] * (u64)c->dom_sz[d - 1];
    m.dimprod[d] = (int)((u64)c->dom_sz[d - 1] * (u64)(long long)m.dimprod[d - 1]);
  }
  m.mask_pitch = mask_pitch(c);
  m.u_pitch = u_pitch(c);
  m.u_rows = 1;
  m.jacobian_symmetric = c->opt.jacobian_symmetric; m.robust = c->opt.robust;
  m.use_type_filter = c->opt.use_type_filter; m.type_filter = c->opt.type_filter;
  m.compute_degrees = c->opt.compute_degrees; m.tag_mode = c->opt.tag_mode;
  m.scalar_mode = c->scalar_mode == 1;
  m.derive_jacobian = c->opt.derive_jacobian;
  { const char *e = getenv("FTKX_RECORD_GENERAL"); m.record_general = (e && atoi(e) != 0) ? 1 : 0; }
  m.coords_mode = c->opt.coords_mode;
  for (int i = 0; i < 6; i ++) m.coords_bounds[i] = c->opt.coords_bounds[i];
  for (int d = 0; d < 3; d ++) m.coords_rect[d] = c->d_rect[d].as<double>();
  m.coords_expl = c->d_expl.as<double>(); m.coords_expl_ncomp = c->expl_ncomp; m.coords_expl_n0 = (int)c->expl_n0;
  const ftkx_tail_set &S = c->sr_tail[0];                     // (a series pass on the other set: series.hip, series_mesh)
  m.hits = c->d_hits.as<ftkx_cp_t>(); m.pass = S.pass.as<u64>(); m.counters = S.counters.as<u64>(); m.capacity = c->capacity;
  m.fragile = S.fragile.as<u64>(); m.fragile_capacity = S.fragile_capacity;
  m.u_rows = ftkx::mask_summary_rows(m);
}

int slice_resolution(ftkx_ctx *c, Slice &s)
{
  if (s.have_res) return FTKX_OK;
  u64 *d = c->sr_tail[0].counters.as<u64>() + ftkx::CNT_N;
  u64 init[128];
  for (int i = 0; i < 64; i ++) { init[2 * i] = 0x7fefffffffffffffull; init[2 * i + 1] = 0ull; }
  HIP_TRY(c, hipMemcpyAsync(d, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
  if (c->scalar_mode == 1) {
    Mesh m; fill_mesh(c, m);
    if (ftkx::march2_supported(m)) {
      // the marching stencil kernel in reduce-only mode: same single pass over S as the mask kernel, nothing stored
      int rc = ensure_desc(c, sizeof(MaskJob));
      if (rc) return rc;
      const MaskJob job{s.S.as<double>(), nullptr, nullptr, nullptr, d, 1.0};
      HIP_TRY(c, hipMemcpyAsync(c->d_desc.p, &job, sizeof(job), hipMemcpyHostToDevice, c->stream));
      ftkx::launch_reduce_march(m, (const MaskJob *)c->d_desc.p, 1, c->stream);
    } else ftkx::launch_resolution_scalar(m, s.S.as<double>(), d, c->stream);
  }
  else ftkx::launch_resolution(s.V.as<double>(), n_vertices(c) * (size_t)c->nd, d, c->stream);
  HIP_TRY(c, hipGetLastError());
  u64 out[128];
  HIP_TRY(c, hipMemcpyAsync(out, d, sizeof(out), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  u64 mn = out[0], mx = out[1];
  for (int i = 1; i < 64; i ++) { mn = std::min(mn, out[2 * i]); mx = std::max(mx, out[2 * i + 1]); }
  memcpy(&s.res, &mn, 8);
  memcpy(&s.maxabs, &mx, 8);
  s.have_res = true;
  return FTKX_OK;
}

// (what masks serve and which jobs need the per-vertex rule: batch_plan.hpp)
bool masks_valid(const ftkx_ctx *c, const Slice &s, u64 factor, bool two_level, int u_rows) { return masks_valid(c->nd, slice_facts(s), factor, two_level, u_rows); }
double job_big(const ftkx_ctx *c, const Slice &s, u64 factor, bool *rule_on) { return job_big(c->nd, slice_facts(s), factor, rule_on); }

// (host memory -> HBM: upload.cpp)

// ---- the library's auxiliary streams ----------------------------------------------------------------------------------------------
// A pass's tail (series.hip) and the copy of its records run on streams of the library's own.  They are kept for the PROCESS, per device and
// priority, and handed from a context that is destroyed to the next one that asks: what a stream is mapped to -- the hardware queue, its
// priority -- is decided by the runtime when the stream is made, and a process that makes and destroys contexts (bench.py's configurations,
// a test session) otherwise gets a different mapping for every context (round 5: the split pass of hit-dense data ran at 0.78 ms in a
// fresh process and at 0.93-0.97 behind other contexts).  FTKX_STREAM_POOL=0: streams made and destroyed with the context, as before.
namespace {
std::mutex g_aux_mutex;
std::map<std::pair<int, int>, std::vector<hipStream_t>> g_aux_free;      // (device, high priority?) -> idle streams
bool aux_pool_on() { const char *e = getenv("FTKX_STREAM_POOL"); return !e || atoi(e) != 0; }
}
int aux_stream_get(ftkx_ctx *c, bool high, hipStream_t *out)
{
  if (aux_pool_on()) {
    std::lock_guard<std::mutex> g(g_aux_mutex);
    auto &v = g_aux_free[{c->device, high ? 1 : 0}];
    if (!v.empty()) { *out = v.back(); v.pop_back(); return FTKX_OK; }
  }
  if (high) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    HIP_TRY(c, hipStreamCreateWithPriority(out, hipStreamNonBlocking, hi));
  } else HIP_TRY(c, hipStreamCreateWithFlags(out, hipStreamNonBlocking));
  return FTKX_OK;
}
void aux_stream_put(ftkx_ctx *c, bool high, hipStream_t st)
{
  if (!st) return;
  (void)hipStreamSynchronize(st);
  if (!aux_pool_on()) { (void)hipStreamDestroy(st); return; }
  std::lock_guard<std::mutex> g(g_aux_mutex);
  g_aux_free[{c->device, high ? 1 : 0}].push_back(st);
}

int ensure_mask_arrays(ftkx_ctx *c, Slice &s, bool two_level)
{
  s.mask_gen = ++ c->mask_epoch;    // (every builder of masks comes through here: a series pass collected later leaves this slice's marks alone)
  // (a pooled array's padding is still neutral from its first life; a new one: row padding and whatever no kernel writes is made cull-neutral)
  auto take = [&](ftkx_array_class k, size_t bytes, ftkx_block &dst) -> int {
    bool fresh = false;
    if (const int rc = c->arrays.take(c, k, bytes, dst, &fresh)) return rc;
    if (fresh) HIP_TRY(c, hipMemsetAsync(dst.p, 0x3f, bytes, c->stream));
    s.mask_factor = 0;      // (summaries must be produced together with the masks)
    return FTKX_OK;
  };
  if (!s.M.p) { if (const int rc = take(FTKX_ARRAY_MASK, mask_bytes(c), s.M)) return rc; }
  return two_level && !s.U.p ? take(FTKX_ARRAY_SUMMARY, u_bytes(c), s.U) : FTKX_OK;
}

}  // namespace ftkxh

// ---- the three raw functions behind ftkx_block (ctx_block.hpp) -----------------------------------------------------------------------
int ftkx_block_alloc(ftkx_ctx *c, ftkx_block_kind kind, size_t bytes, void **p)
{
  *p = nullptr;
  switch (kind) {
    case FTKX_BLOCK_DEVICE: HIP_TRY(c, hipMalloc(p, bytes)); break;
    case FTKX_BLOCK_PINNED: HIP_TRY(c, hipHostMalloc(p, bytes, hipHostMallocDefault)); break;
    case FTKX_BLOCK_PINNED_COHERENT: HIP_TRY(c, hipHostMalloc(p, bytes, hipHostMallocCoherent)); break;
    case FTKX_BLOCK_PINNED_NONCOHERENT: HIP_TRY(c, hipHostMalloc(p, bytes, hipHostMallocNonCoherent)); break;
    case FTKX_BLOCK_LENT: return fail(c, FTKX_E_INVALID, "a block the caller lent cannot be reserved");
  }
  return FTKX_OK;
}
void ftkx_block_free(ftkx_block_kind kind, void *p) { (void)(kind == FTKX_BLOCK_DEVICE ? hipFree(p) : hipHostFree(p)); }
int ftkx_block_drain(ftkx_ctx *c, void *stream) { HIP_TRY(c, hipStreamSynchronize((hipStream_t)stream)); return FTKX_OK; }

// f(begin, end) over the records of a call: on a few host threads from 2^18 records (below that starting the threads costs more than the
// loops: 62 181 records of bench.py's C2 take 0.5 ms on one thread, 0.76 ms on eight)
template <class F> static void sample_ranges(size_t n, F f)
{
  if (n < ((size_t)1 << 18)) f((size_t)0, n);
  else ftkx::for_ranges_on_threads(n, f);
}

extern "C" {

const char *ftkx_last_mask_kernel(void) { return ftkx::last_mask_kernel(); }
int ftkx_debug_mask_kernel_launches(unsigned long long *launches, const char **names, int n)
{
  unsigned long long l[ftkx::kMaskKernels]; const char *nm[ftkx::kMaskKernels];
  ftkx::mask_kernel_launches(l, nm);
  for (int i = 0; i < n && i < ftkx::kMaskKernels; i ++) { if (launches) launches[i] = l[i]; if (names) names[i] = nm[i]; }
  return ftkx::kMaskKernels;
}

const char *ftkx_version(void) { return "ftkx 0.1 (gfx950)"; }

// which device a pointer lives on: its ordinal, or -1 for host memory / unknown pointers
int ftkx_pointer_device(const void *p)
{
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return a.type == hipMemoryTypeDevice ? a.device : -1;
}

int ftkx_context_device(const ftkx_ctx *c) { return c ? c->device : -1; }

int ftkx_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void ftkx_default_options(ftkx_options *o)
{
  memset(o, 0, sizeof(*o));
  o->jacobian_symmetric = 1;
  o->robust = 1;
  o->tag_mode = FTKX_TAG_EXACT64;
}

int ftkx_last_error(const ftkx_ctx *ctx, char *buf, size_t n)
{
  const std::string &e = ctx ? ctx->err : g_last_error;
  if (buf && n) { strncpy(buf, e.c_str(), n - 1); buf[n - 1] = 0; }
  return (int)e.size();
}

int ftkx_create(ftkx_ctx **out, int nd, int device_id)
{
  if (!out || (nd != 2 && nd != 3)) return fail(nullptr, FTKX_E_INVALID, "ftkx_create: nd must be 2 or 3");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) return fail(nullptr, FTKX_E_DEVICE, "ftkx_create: no HIP device (%s)", hipGetErrorString(e));
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, FTKX_E_INVALID, "ftkx_create: device %d of %d", device_id, ndev);
  ftkx_ctx *c = new ftkx_ctx();
  c->nd = nd;
  c->device = device_id;
  ftkx_default_options(&c->opt);
  memset(&c->stats, 0, sizeof(c->stats));
  // a blocking stream: it orders itself against the legacy default stream, which is where a caller that never heard of
  // streams (and torch's default stream) puts its copies and fills
  auto init = [&]() -> int {
    HIP_TRY(c, hipSetDevice(device_id));
    HIP_TRY(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamDefault));
    c->stream = c->own_stream;
    // CNT_N counters, 128 words of reduction slots, one word that says "a halo message did not fit this mesh" (halo.hip; survives the sweeps' resets)
    if (const int rc = c->sr_tail[0].counters.reserve(c, (ftkx::CNT_N + 128 + 8) * sizeof(u64))) return rc;
    HIP_TRY(c, hipMemset(c->sr_tail[0].counters.p, 0, (ftkx::CNT_N + 128 + 8) * sizeof(u64)));
    return c->h_counters.reserve(c, ftkx::CNT_N * sizeof(u64));
  };
  const int rc = init();
  if (rc != FTKX_OK) { ftkx_destroy(c); return rc; }     // nothing half-built is left behind
  *out = c;
  return FTKX_OK;
}

void ftkx_destroy(ftkx_ctx *c)
{
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  (void)sync_tails(c);                                        // (passes left open: their tails and copies read what is freed below)
  if (c->sr_copy_stream) (void)hipStreamSynchronize(c->sr_copy_stream);
  if (c->tm_read) (void)hipEventDestroy(c->tm_read);
  for (auto &e : c->events) { (void)hipEventDestroy(e.second.first); (void)hipEventDestroy(e.second.second); }
  for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
  for (ftkx_series_buffers &B : c->sr_buf)
    for (hipEvent_t e : {B.ev_copied, B.ev_export, B.ev_masks, B.ev_factors, B.ev_tail}) if (e) (void)hipEventDestroy(e);
  if (c->sr_ev_fetched) (void)hipEventDestroy(c->sr_ev_fetched);
  aux_stream_put(c, false, c->sr_copy_stream);
  for (ftkx_tail_set &S : c->sr_tail) aux_stream_put(c, true, S.stream);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;                                                   // every block (ctx_block.hpp) goes with it: the slices, parked and retired arrays, the ring and the pool too
}

int ftkx_set_stream(ftkx_ctx *c, void *s)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = settings_not_now(c, "ftkx_set_stream")) return rc;
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return FTKX_OK;
}

int ftkx_set_options(ftkx_ctx *c, const ftkx_options *o)
{
  if (c) c->ahead.clear();
  if (!c || !o) return fail(c, FTKX_E_INVALID, "null argument");
  if (int rc = settings_not_now(c, "ftkx_set_options")) return rc;
  if (o->tag_mode < FTKX_TAG_WORK_INDEX || o->tag_mode > FTKX_TAG_EXACT64) return fail(c, FTKX_E_INVALID, "bad tag_mode %d", o->tag_mode);
  if (o->coords_mode < 0 || o->coords_mode > 3) return fail(c, FTKX_E_INVALID, "bad coords_mode %d", o->coords_mode);
  if (o->coords_mode == 2 && !c->d_rect[0].as<double>()) return fail(c, FTKX_E_INVALID, "coords_mode RECTILINEAR: call ftkx_set_coords_rectilinear");
  if (o->coords_mode == 3 && !c->d_expl.as<double>()) return fail(c, FTKX_E_INVALID, "coords_mode EXPLICIT: call ftkx_set_coords_explicit");
  c->opt = *o;
  return FTKX_OK;
}

int ftkx_set_coords_rectilinear(ftkx_ctx *c, const double *x, size_t nx, const double *y, size_t ny, const double *z, size_t nz)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "ftkx_set_coords_rectilinear: sweeps pending, collect first");
  const double *src[3] = {x, y, z};
  const size_t n[3] = {nx, ny, nz};
  for (int d = 0; d < c->nd; d ++) if (!src[d] || !n[d]) return fail(c, FTKX_E_INVALID, "ftkx_set_coords_rectilinear: axis %d missing", d);
  HIP_TRY(c, hipSetDevice(c->device));
  for (int d = 0; d < c->nd; d ++) {
    c->d_rect[d] = ftkx_block();                             // (a new array every time, of exactly this size)
    if (const int rc = c->d_rect[d].reserve(c, n[d] * sizeof(double))) return rc;
    HIP_TRY(c, hipMemcpy(c->d_rect[d].p, src[d], n[d] * sizeof(double), hipMemcpyHostToDevice));
    c->rect_n[d] = n[d];
  }
  c->opt.coords_mode = 2;
  return FTKX_OK;
}

int ftkx_set_coords_explicit(ftkx_ctx *c, const double *coords, int ncomp, size_t n0, size_t n1)
{
  if (!c || !coords) return fail(c, FTKX_E_INVALID, "null argument");
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "ftkx_set_coords_explicit: sweeps pending, collect first");
  if (ncomp < 2 || (c->nd == 3 && ncomp < 3) || !n0 || !n1) return fail(c, FTKX_E_INVALID, "ftkx_set_coords_explicit: need %d components and a non-empty array", c->nd == 3 ? 3 : 2);
  HIP_TRY(c, hipSetDevice(c->device));
  c->d_expl = ftkx_block();                                  // (a new array every time, of exactly this size)
  const size_t count = (size_t)ncomp * n0 * n1;
  if (const int rc = c->d_expl.reserve(c, count * sizeof(double))) return rc;
  HIP_TRY(c, hipMemcpy(c->d_expl.p, coords, count * sizeof(double), hipMemcpyHostToDevice));
  c->expl_ncomp = ncomp; c->expl_n0 = n0; c->expl_n1 = n1;
  c->opt.coords_mode = 3;
  return FTKX_OK;
}

int ftkx_set_mesh(ftkx_ctx *c, const long long dst[3], const long long dsz[3], const long long cst[3], const long long csz[3],
                  const long long est[3], const long long esz[3])
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!c->slices.empty()) return fail(c, FTKX_E_INVALID, "ftkx_set_mesh: drop all slices first");
  HIP_TRY(c, hipSetDevice(c->device));
  // nothing of the old lattice stays: slices and aux arrays dropped under an open split pass are parked with it, not in `slices` / `aux` -- its tail is waited for
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, sync_tails(c));
  for (ftkx_series_pending &P : c->sr_pend) release_retired(c, P);
  temporal_release(c);                    // a temporal series that was open starts afresh: its raw snapshots have the old lattice's size
  c->aux.clear();                         // (aux arrays left behind by slices that were never dropped: the old lattice's, too)
  c->arrays.clear();
  for (int d = 0; d < c->nd; d ++) {
    if (dsz[d] < 0 || csz[d] < 0 || esz[d] <= 0) return fail(c, FTKX_E_INVALID, "ftkx_set_mesh: negative size on axis %d", d);
    if (dst[d] + dsz[d] > 2147483647LL || est[d] + esz[d] > 2147483647LL || cst[d] + csz[d] > 2147483647LL)
      return fail(c, FTKX_E_INVALID, "ftkx_set_mesh: axis %d exceeds int range", d);
    // every corner enumerated must be addressable: the kernel reads a vertex only when it is inside domain AND ext
    c->dom_st[d] = dst[d]; c->dom_sz[d] = dsz[d];
    c->core_st[d] = cst[d]; c->core_sz[d] = csz[d];
    c->ext_st[d] = est[d]; c->ext_sz[d] = esz[d];
  }
  for (int d = c->nd; d < 3; d ++) { c->dom_st[d] = 0; c->dom_sz[d] = 1; c->core_st[d] = 0; c->core_sz[d] = 1; c->ext_st[d] = 0; c->ext_sz[d] = 1; }
  c->mesh_set = true;
  c->scalar_mode = -1;
  c->dense_collects = 0;
  return FTKX_OK;
}

// ---- auxiliary scalar fields sampled at critical points (sample_steps.hpp, sample_kernels.hip; the arrays come in through ingest.hip) -----
// What a launch of the sample kernel needs, on the device when sample_prepare returns FTKX_OK with slots != 0: the records' (tag, aux word)
// pairs and behind them the table of slice pointers in sm_d_in, room for the results in sm_d_out and sm_h_out.  Every check of
// ftkx_sample_aux is made there, before anything is written anywhere.
struct SamplePlan {
  ftkx::SampleMesh m;
  int t_min = 0, ntab = 0;
  unsigned slots = 0;
  int nslots = 0;
  const ftkx::SampleIn *d_in = nullptr;
  const ftkx::SampleSlice *d_tab = nullptr;
};

static int sample_prepare(ftkx_ctx *c, const char *who, const ftkx_cp_t *recs, size_t n, SamplePlan &P)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!c->mesh_set) return fail(c, FTKX_E_INVALID, "%s: call ftkx_set_mesh first", who);
  if (n == 0) return FTKX_OK;
  if (!recs) return fail(c, FTKX_E_INVALID, "%s: null records", who);
  HIP_TRY(c, hipSetDevice(c->device));
  const int nd = c->nd;
  ftkx::SampleMesh &m = P.m;
  m = sample_mesh_of(c);
  // ONE pass over the records (72 bytes each: at 10^6 of them every pass is a walk through memory), on a few host threads where there are
  // many (sample_ranges): tag and aux word into the pinned block that goes up, the range of the timesteps beside it.  Everything behind reads the
  // 16-byte pairs.  The table of slice pointers travels behind the pairs; the block has room for 2 048 timesteps from the start.
  const size_t in_bytes = n * sizeof(ftkx::SampleIn);
  size_t tab_room = 2048 * sizeof(ftkx::SampleSlice);
  if (int rc = c->sm_h_in.reserve(c, in_bytes + tab_room, in_bytes + in_bytes / 4 + tab_room, c->stream)) return rc;
  ftkx::SampleIn *h_in = c->sm_h_in.as<ftkx::SampleIn>();
  std::atomic<int> lo(2147483647), hi(-1);
  auto pack = [&]() {
    sample_ranges(n, [&](size_t b, size_t e) {
      int mn = 2147483647, mx = -1;
      for (size_t i = b; i < e; i ++) {
        h_in[i] = ftkx::SampleIn{recs[i].tag, ftkx_cp_aux(&recs[i]), 0u};
        const int t = (int)(h_in[i].aux >> 1);
        mn = std::min(mn, t); mx = std::max(mx, t);
      }
      for (int seen = lo.load(); mn < seen && !lo.compare_exchange_weak(seen, mn); ) {}
      for (int seen = hi.load(); mx > seen && !hi.compare_exchange_weak(seen, mx); ) {}
    });
  };
  pack();
  const int t_min = lo.load(), t_max = hi.load();
  if (t_max >= 2147483646 || (long long)t_max - (long long)t_min > (1ll << 22)) return fail(c, FTKX_E_NOSLICE, "%s: the records' timesteps span %d .. %d, which cannot all be resident", who, t_min, t_max);
  if (m.tag_mode == FTKX_TAG_REFERENCE && !ftkx::sample_reference_tags_exact(nd, c->dom_sz, t_max))
    return fail(c, FTKX_E_UNSUPPORTED, "%s: FTKX_TAG_REFERENCE tags may have wrapped at timestep %d of this mesh and cannot be decoded (use FTKX_TAG_EXACT64)", who, t_max);
  const int ntab = t_max - t_min + 2;                                    // (an interval record of t_max reads t_max + 1)
  const size_t tab_bytes = (size_t)ntab * sizeof(ftkx::SampleSlice);
  if (tab_bytes > tab_room) {                                            // (more than 2 048 timesteps: the pairs are packed again into the larger block)
    if (int rc = c->sm_h_in.reserve(c, in_bytes + tab_bytes, in_bytes + in_bytes / 4 + tab_bytes, c->stream)) return rc;
    h_in = c->sm_h_in.as<ftkx::SampleIn>();
    pack();
  }
  // which timesteps are read, and that every record decodes to a simplex inside the arrays: nothing else reaches the kernel
  std::vector<unsigned char> need((size_t)ntab, 0);
  std::mutex need_lock;
  std::atomic<size_t> first_bad(n);
  sample_ranges(n, [&](size_t b, size_t e) {
    std::vector<unsigned char> mine((size_t)ntab, 0);
    for (size_t i = b; i < e; i ++) {
      const ftkx::SampleIn in = h_in[i];
      const size_t at = (size_t)((int)(in.aux >> 1) - t_min);
      mine[at] = 1;
      if (!(in.aux & 1u)) mine[at + 1] = 1;
      int corner[4], type = 0;
      const bool ok = nd == 2 ? ftkx::sample_element<2>(m, ftkx::k_fan3, in.tag, in.aux, corner, type) : ftkx::sample_element<3>(m, ftkx::k_fan4, in.tag, in.aux, corner, type);
      if (!ok) { size_t seen = first_bad.load(); while (i < seen && !first_bad.compare_exchange_weak(seen, i)) {} }
    }
    std::lock_guard<std::mutex> g(need_lock);
    for (int k = 0; k < ntab; k ++) need[(size_t)k] |= mine[(size_t)k];
  });
  std::vector<ftkx::SampleSlice> tab((size_t)ntab, ftkx::SampleSlice{nullptr, nullptr, {nullptr, nullptr}});
  int needed = 0, have[2] = {0, 0};
  for (int k = 0; k < ntab; k ++) {
    if (!need[(size_t)k]) continue;
    const int t = t_min + k;
    auto it = c->slices.find(t);
    if (it == c->slices.end()) return fail(c, FTKX_E_NOSLICE, "%s: slice %d not resident", who, t);
    const Slice &s = it->second;
    if (s.sparse) return fail(c, FTKX_E_UNSUPPORTED, "%s: slice %d exists as masks and patches only", who, t);
    if (m.scalar_mode ? !s.S.p : !s.V.p) return fail(c, FTKX_E_INVALID, "%s: slice %d has no field array", who, t);
    tab[(size_t)k].S = s.S.as<double>(); tab[(size_t)k].V = s.V.as<double>();
    needed ++;
    auto ia = c->aux.find(t);
    for (int a = 0; a < 2; a ++)
      if (ia != c->aux.end() && ia->second.A[a].p) { tab[(size_t)k].A[a] = ia->second.A[a].as<double>(); have[a] ++; }
  }
  for (int a = 0; a < 2; a ++) {
    if (have[a] != 0 && have[a] != needed) return fail(c, FTKX_E_NOSLICE, "%s: slot %d has an aux array at %d of the %d timesteps the records read", who, a + 1, have[a], needed);
    if (have[a]) { P.slots |= 1u << a; P.nslots ++; }
  }
  if (const size_t i = first_bad.load(); i < n)
    return fail(c, FTKX_E_INVALID, "%s: record %zu (tag %llu, timestep %d) is not an element of this context's mesh under its tag mode", who, i, recs[i].tag, ftkx_cp_timestep(&recs[i]));
  if (!P.slots) return FTKX_OK;
  memcpy(h_in + n, tab.data(), tab_bytes);
  if (int rc = c->sm_d_in.reserve(c, in_bytes + tab_bytes, in_bytes + in_bytes / 4 + tab_bytes + 4096, c->stream)) return rc;
  const size_t out_bytes = n * (size_t)P.nslots * sizeof(double);
  if (int rc = c->sm_d_out.reserve(c, out_bytes, out_bytes + out_bytes / 4, c->stream)) return rc;
  if (int rc = c->sm_h_out.reserve(c, out_bytes, out_bytes + out_bytes / 4, c->stream)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->sm_d_in.p, c->sm_h_in.p, in_bytes + tab_bytes, hipMemcpyHostToDevice, c->stream));
  P.t_min = t_min; P.ntab = ntab;
  P.d_in = c->sm_d_in.as<ftkx::SampleIn>();
  P.d_tab = reinterpret_cast<const ftkx::SampleSlice *>(P.d_in + n);
  return FTKX_OK;
}

int ftkx_sample_aux(ftkx_ctx *c, ftkx_cp_t *recs, size_t n)
{
  SamplePlan P;
  if (int rc = sample_prepare(c, "ftkx_sample_aux", recs, n, P)) return rc;
  if (n == 0 || !P.slots) return FTKX_OK;
  ftkx::launch_sample(c->nd, P.m, P.d_in, n, P.d_tab, P.t_min, P.slots, c->sm_d_out.as<double>(), c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(c->sm_h_out.p, c->sm_d_out.p, n * (size_t)P.nslots * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->sm_launches ++; c->sm_records += n;
  const double *o = c->sm_h_out.as<double>();
  const double *o1 = (P.slots & 1u) ? o : nullptr, *o2 = (P.slots & 2u) ? o + ((P.slots & 1u) ? n : 0) : nullptr;
  sample_ranges(n, [&](size_t b, size_t e) {      // (one walk through the records for both slots)
    for (size_t i = b; i < e; i ++) { if (o1) recs[i].scalar[1] = o1[i]; if (o2) recs[i].scalar[2] = o2[i]; }
  });
  return FTKX_OK;
}

// profiling aid (tools/sample_time.py): the sample kernel `reps` times back to back, a pair of events around every launch; the records are
// not written
int ftkx_debug_sample_relaunch(ftkx_ctx *c, const ftkx_cp_t *recs, size_t n, int reps, double *ms)
{
  if (c && (!ms || reps < 1 || n == 0)) return fail(c, FTKX_E_INVALID, "ftkx_debug_sample_relaunch: bad argument");
  SamplePlan P;
  if (int rc = sample_prepare(c, "ftkx_debug_sample_relaunch", recs, n, P)) return rc;
  if (!P.slots) return fail(c, FTKX_E_NOSLICE, "ftkx_debug_sample_relaunch: no aux array is resident");
  return timed_relaunch(c, reps, ms, [&] { ftkx::launch_sample(c->nd, P.m, P.d_in, n, P.d_tab, P.t_min, P.slots, c->sm_d_out.as<double>(), c->stream); });
}

int ftkx_debug_sample_counts(const ftkx_ctx *c, unsigned long long *launches, unsigned long long *records)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (launches) *launches = c->sm_launches;
  if (records) *records = c->sm_records;
  return FTKX_OK;
}

int ftkx_debug_array_counts(const ftkx_ctx *c, unsigned long long allocated[3], unsigned long long pooled[3])
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  for (int k = 0; k < FTKX_ARRAY_CLASSES; k ++) { if (allocated) allocated[k] = c->arrays.allocated[k]; if (pooled) pooled[k] = c->arrays.held[k].size(); }
  return FTKX_OK;
}

int ftkx_drop_slice(ftkx_ctx *c, int t)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  auto it = c->slices.find(t);
  if (it == c->slices.end()) return fail(c, FTKX_E_NOSLICE, "ftkx_drop_slice: timestep %d not resident", t);
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "ftkx_drop_slice: sweeps pending, collect first");
  (void)hipSetDevice(c->device);
  free_slice(it->second, c);
  c->slices.erase(it);
  drop_aux(c, t);
  return FTKX_OK;
}

int ftkx_slice_resolution(ftkx_ctx *c, int t, double *res, double *max_abs)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  auto it = c->slices.find(t);
  if (it == c->slices.end()) return fail(c, FTKX_E_NOSLICE, "ftkx_slice_resolution: timestep %d not resident", t);
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = slice_resolution(c, it->second);
  if (rc) return rc;
  if (res) *res = it->second.res;
  if (max_abs) *max_abs = it->second.maxabs;
  return FTKX_OK;
}

// the same reduction for several slices at once: one launch, one download, one synchronise (a time series that is already
// resident does not need a round trip per slice)
int ftkx_slices_resolution(ftkx_ctx *c, const int *ts, int n, double *res, double *max_abs)
{
  if (!c || (n > 0 && !ts)) return fail(c, FTKX_E_INVALID, "null argument");
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<Slice *> todo;
  for (int i = 0; i < n; i ++) {
    auto it = c->slices.find(ts[i]);
    if (it == c->slices.end()) return fail(c, FTKX_E_NOSLICE, "ftkx_slices_resolution: timestep %d not resident", ts[i]);
    if (!it->second.have_res) todo.push_back(&it->second);
  }
  Mesh m; fill_mesh(c, m);
  if (todo.size() > 1) {
    const size_t k = todo.size();
    int rc = ensure_red(c, k);
    // descriptors and results share the pinned staging buffer (stream order: upload, kernel, download)
    if (rc == FTKX_OK) rc = ensure_desc(c, std::max(k * sizeof(MaskJob), k * 128 * sizeof(u64)));
    if (rc) return rc;
    launch_init_red(c->d_red.as<u64>(), k * 64, nullptr, c->stream);
    if (c->scalar_mode == 1 && ftkx::march2_supported(m)) {
      // the marching stencil kernel in reduce-only mode over all slices at once
      MaskJob *jobs = (MaskJob *)c->h_desc.p;
      for (size_t i = 0; i < k; i ++) jobs[i] = MaskJob{todo[i]->S.as<double>(), nullptr, nullptr, nullptr, c->d_red.as<u64>() + i * 128, 1.0};
      HIP_TRY(c, hipMemcpyAsync(c->d_desc.p, c->h_desc.p, k * sizeof(MaskJob), hipMemcpyHostToDevice, c->stream));
      ftkx::launch_reduce_march(m, (const MaskJob *)c->d_desc.p, (int)k, c->stream);
    } else {
      // one launch per slice, back to back, each into its own slots
      for (size_t i = 0; i < k; i ++) {
        if (c->scalar_mode == 1) ftkx::launch_resolution_scalar(m, todo[i]->S.as<double>(), c->d_red.as<u64>() + i * 128, c->stream);
        else ftkx::launch_resolution(todo[i]->V.as<double>(), n_vertices(c) * (size_t)c->nd, c->d_red.as<u64>() + i * 128, c->stream);
      }
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_desc.p, c->d_red.as<u64>(), k * 128 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const u64 *host = (const u64 *)c->h_desc.p;
    for (size_t i = 0; i < k; i ++) {
      u64 mn = host[i * 128], mx = host[i * 128 + 1];
      for (int q = 1; q < 64; q ++) { mn = std::min(mn, host[i * 128 + 2 * q]); mx = std::max(mx, host[i * 128 + 2 * q + 1]); }
      memcpy(&todo[i]->res, &mn, 8);
      memcpy(&todo[i]->maxabs, &mx, 8);
      todo[i]->have_res = true;
    }
  } else {
    for (Slice *s : todo) { int rc = slice_resolution(c, *s); if (rc) return rc; }
  }
  for (int i = 0; i < n; i ++) {
    const Slice &s = c->slices.find(ts[i])->second;
    if (res) res[i] = s.res;
    if (max_abs) max_abs[i] = s.maxabs;
  }
  return FTKX_OK;
}

int ftkx_set_slice_resolution(ftkx_ctx *c, int t, double resolution, double max_abs)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  auto it = c->slices.find(t);
  if (it == c->slices.end()) return fail(c, FTKX_E_NOSLICE, "ftkx_set_slice_resolution: timestep %d not resident", t);
  if (!(resolution > 0) || !(max_abs >= 0)) return fail(c, FTKX_E_INVALID, "ftkx_set_slice_resolution: bad values");
  it->second.res = resolution; it->second.maxabs = max_abs; it->second.have_res = true;
  return FTKX_OK;
}

unsigned long long ftkx_scaling_factor(double resolution, int *nbits_out)
{
  // critical_point_tracker.hh:850-864
  int nbits = (int)std::ceil(std::log2(1.0 / resolution));
  nbits = std::max(8, std::min(nbits, 21));
  if (nbits_out) *nbits_out = nbits;
  return 1ull << nbits;
}

int ftkx_get_stats(const ftkx_ctx *c, ftkx_stats *st)
{
  if (!c || !st) return fail(nullptr, FTKX_E_INVALID, "null argument");
  *st = c->stats;
  return FTKX_OK;
}

int ftkx_invalidate_masks(ftkx_ctx *c)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "ftkx_invalidate_masks: sweeps pending, collect first");
  for (auto &kv : c->slices) { kv.second.mask_factor = 0; kv.second.have_fused = false; kv.second.mask_gen = ++ c->mask_epoch; }
  c->ahead.clear();
  c->dense_collects = 0;
  return FTKX_OK;
}


// profiling aid (bench.py's int-VALU yardstick): from the next sweep on, the tile kernel runs its fan phase -- the predicate arithmetic on
// the tile staged in LDS -- `repeat` times per tile and step; records and statistics are those of one.  1 = off.
int ftkx_debug_tile_repeat(ftkx_ctx *c, int repeat)
{
  if (!c || repeat < 1) return fail(c, FTKX_E_INVALID, "ftkx_debug_tile_repeat: repeat >= 1");
  c->tile_repeat = repeat;
  return FTKX_OK;
}
int ftkx_debug_stream_read(ftkx_ctx *c, const void *device_ptr, size_t bytes)
{
  if (!c || !device_ptr) return fail(c, FTKX_E_INVALID, "null argument");
  HIP_TRY(c, hipSetDevice(c->device));
  ftkx::launch_calib_read(device_ptr, bytes, (double *)(c->sr_tail[0].counters.as<u64>() + ftkx::CNT_N), c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FTKX_OK;
}

int ftkx_set_profiling(ftkx_ctx *c, int on)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  c->profiling = on < 0 ? 0 : (on > 2 ? 1 : on);
  for (int k = 0; k < K_N; k ++) { c->k_ms[k] = 0; c->k_launches[k] = 0; }
  return FTKX_OK;
}

int ftkx_get_kernel_times(const ftkx_ctx *c, double ms[4], unsigned long long launches[4])
{
  if (!c || !ms || !launches) return fail(nullptr, FTKX_E_INVALID, "null argument");
  ev_harvest(const_cast<ftkx_ctx *>(c), false);          // (pairs that have completed since the last call that waited)
  for (int k = 0; k < K_N; k ++) { ms[k] = c->k_ms[k]; launches[k] = c->k_launches[k]; }
  return FTKX_OK;
}

void ftkx_free(void *p) { free(p); }

static int extract_common(int nd, int scope, int t, const long long *dst, const long long *dsz, const long long *cst, const long long *csz,
                          const long long *est, const long long *esz, const double *Vc, const double *Vn, const double *Jc, const double *Jn,
                          const double *Sc, const double *Sn, unsigned long long factor, const ftkx_options *opt, int device_id,
                          ftkx_cp_t **out, size_t *n_out, const double *explicit_coords = nullptr)
{
  if (!out || !n_out) return fail(nullptr, FTKX_E_INVALID, "extract: null output");
  *out = nullptr; *n_out = 0;
  if (scope != FTKX_SCOPE_ORDINAL && scope != FTKX_SCOPE_INTERVAL) return fail(nullptr, FTKX_E_INVALID, "extract: scope must be 1 or 2");
  if (!Vc || (scope == FTKX_SCOPE_INTERVAL && !Vn)) return fail(nullptr, FTKX_E_INVALID, "extract: missing vector field");
  // the time axis of core must be the single step `t` (element_for builds it that way, regular_tracker.hh:196-211)
  if (cst[nd] != t || csz[nd] != 1) return fail(nullptr, FTKX_E_INVALID, "extract: core must cover exactly timestep %d", t);
  if (dst[nd] != 0) return fail(nullptr, FTKX_E_UNSUPPORTED, "extract: domain must start at time 0");
  ftkx_ctx *c = nullptr;
  int rc = ftkx_create(&c, nd, device_id);
  if (rc) return rc;
  ftkx_options o;
  if (opt) o = *opt; else { ftkx_default_options(&o); o.tag_mode = FTKX_TAG_WORK_INDEX; }
  long long e3[3] = {est[0], est[1], nd == 3 ? est[2] : 0}, s3[3] = {esz[0], esz[1], nd == 3 ? esz[2] : 1};
  if (explicit_coords) {   // the boundary's `coords`: (2, DW, DH) doubles over `ext` (critical_point_tracer_2d_regular.cu:194-198)
    if (est[0] != 0 || est[1] != 0) { ftkx_destroy(c); return fail(nullptr, FTKX_E_UNSUPPORTED, "extract: explicit coordinates need an array lattice starting at 0"); }
    if ((rc = ftkx_set_coords_explicit(c, explicit_coords, 2, (size_t)esz[0], (size_t)esz[1]))) { g_last_error = c->err; ftkx_destroy(c); return rc; }
    o.coords_mode = 3;
  }
  if ((rc = ftkx_set_options(c, &o)) || (rc = ftkx_set_mesh(c, dst, dsz, cst, csz, e3, s3)) ||
      (rc = ftkx_push_slice(c, t, Vc, Jc, Sc, 0)) ||
      (scope == FTKX_SCOPE_INTERVAL && (rc = ftkx_push_slice(c, t + 1, Vn, Jn, Sn, 0)))) {
    g_last_error = c->err; ftkx_destroy(c); return rc;
  }
  const ftkx_cp_t *recs = nullptr; size_t n = 0;
  rc = ftkx_sweep(c, t, scope, factor, &recs, &n);
  if (rc) { g_last_error = c->err; ftkx_destroy(c); return rc; }
  ftkx_cp_t *copy = (ftkx_cp_t *)malloc((n ? n : 1) * sizeof(ftkx_cp_t));
  if (!copy) { ftkx_destroy(c); return fail(nullptr, FTKX_E_NOMEM, "extract: out of host memory"); }
  if (n) memcpy(copy, recs, n * sizeof(ftkx_cp_t));
  ftkx_destroy(c);
  *out = copy; *n_out = n;
  return FTKX_OK;
}

int ftkx_extract_cp2dt(int scope, int current_timestep, const long long domain_st[3], const long long domain_sz[3],
                       const long long core_st[3], const long long core_sz[3], const long long ext_st[2], const long long ext_sz[2],
                       const double *Vc, const double *Vn, const double *Jc, const double *Jn, const double *Sc, const double *Sn,
                       int use_explicit_coords, const double *coords, unsigned long long factor, const ftkx_options *opt, int device_id,
                       ftkx_cp_t **out, size_t *n_out)
{
  if (use_explicit_coords && !coords) return fail(nullptr, FTKX_E_INVALID, "extract: use_explicit_coords without coords");
  return extract_common(2, scope, current_timestep, domain_st, domain_sz, core_st, core_sz, ext_st, ext_sz, Vc, Vn, Jc, Jn, Sc, Sn, factor, opt, device_id, out, n_out,
                        use_explicit_coords ? coords : nullptr);
}

int ftkx_extract_cp3dt(int scope, int current_timestep, const long long domain_st[4], const long long domain_sz[4],
                       const long long core_st[4], const long long core_sz[4], const long long ext_st[3], const long long ext_sz[3],
                       const double *Vc, const double *Vn, const double *Jc, const double *Jn, const double *Sc, const double *Sn,
                       unsigned long long factor, const ftkx_options *opt, int device_id, ftkx_cp_t **out, size_t *n_out)
{
  return extract_common(3, scope, current_timestep, domain_st, domain_sz, core_st, core_sz, ext_st, ext_sz, Vc, Vn, Jc, Jn, Sc, Sn, factor, opt, device_id, out, n_out);
}


int ftkx_gradient2D(ftkx_ctx *c, const double *S, int DW, int DH, double *V)
{ DERIVE_PROLOGUE(c); ftkx::launch_gradient2d(S, DW, DH, V, c->stream); HIP_TRY(c, hipGetLastError()); HIP_TRY(c, hipStreamSynchronize(c->stream)); return FTKX_OK; }
int ftkx_jacobian2D(ftkx_ctx *c, const double *V, int DW, int DH, int symmetric, double *J)
{ DERIVE_PROLOGUE(c); ftkx::launch_jacobian2d(V, DW, DH, symmetric, J, c->stream); HIP_TRY(c, hipGetLastError()); HIP_TRY(c, hipStreamSynchronize(c->stream)); return FTKX_OK; }
int ftkx_gradient3D(ftkx_ctx *c, const double *S, int DW, int DH, int DD, double *V)
{ DERIVE_PROLOGUE(c); ftkx::launch_gradient3d(S, DW, DH, DD, V, c->stream); HIP_TRY(c, hipGetLastError()); HIP_TRY(c, hipStreamSynchronize(c->stream)); return FTKX_OK; }
int ftkx_jacobian3D(ftkx_ctx *c, const double *V, int DW, int DH, int DD, double *J)
{ DERIVE_PROLOGUE(c); ftkx::launch_jacobian3d(V, DW, DH, DD, J, c->stream); HIP_TRY(c, hipGetLastError()); HIP_TRY(c, hipStreamSynchronize(c->stream)); return FTKX_OK; }
}  // extern "C"
