// Host side of the C ABI declared in include/ftkx.h: context, HBM-resident slices, launch bookkeeping, hit download.
// The reference's counterpart is the per-call host wrapper extract_cp2dt<scope> / extract_cp3dt<scope>
// (src/filters/critical_point_tracer_2d_regular.cu:168-272, ..._3d_regular.cu:144-250), which re-allocates, re-uploads and
// frees everything on every call and synchronises the whole device; here slices stay resident, launches go to a stream,
// and the hit buffer is persistent (grown and the batch replayed if a launch overflows it).
#include <atomic>
#include <map>
#include <mutex>
#include <type_traits>
#include "ctx.hpp"
#include "cp_device.hpp"
#include "host_sort.hpp"
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

// the strict-sign cull is exact only while no determinant of the predicate can leave int64:
// |det4| <= 24 M^3 (3D), |det3| <= 6 M^2 (2D) with M = max |quantised component|   
bool overflow_free(int nd, double maxabs, u64 factor)
{
  const long double M = floorl((long double)maxabs * (long double)factor) + 1.0L;
  const long double lim = 9223372036854775807.0L;
  return nd == 3 ? 24.0L * M * M * M < lim : 6.0L * M * M < lim;
}

double big_threshold(int nd, u64 factor) { return (double)(nd == 3 ? ftkx::kSafeM3 : ftkx::kSafeM2) / (double)factor; }
bool pow2_factor(u64 factor) { return factor != 0 && (factor & (factor - 1)) == 0 && factor <= (1ull << 53); }

// Masks built under mask_factor serve a sweep under `factor` when they can only cull less than masks built under `factor`
// itself: the sign thresholds need mask_factor <= factor; the per-vertex overflow rule (MaskJob::big) is factor-specific, so a
// larger factor is accepted only when the slice's max |v| shows that no vertex is big under it either.
bool masks_valid(const ftkx_ctx *c, const Slice &s, u64 factor, bool two_level, int u_rows)
{
  if (!s.M.p || (two_level && !s.U.p) || s.mask_factor == 0 || s.mask_factor > factor) return false;
  if (two_level && s.u_rows != u_rows) return false;           // summaries of another geometry (FTKX_MASK_* changed since)
  if (s.mask_big && s.mask_factor == factor) return true;
  return s.max_known() && overflow_free(c->nd, s.maxabs, factor);   // no vertex is big under `factor`: the rule would change nothing
}

// the per-vertex rule costs the marching kernels a few instructions per row: it is switched on only when it can matter
double job_big(const ftkx_ctx *c, const Slice &s, u64 factor, bool *rule_on)
{
  const bool off = s.max_known() && overflow_free(c->nd, s.maxabs, factor);
  *rule_on = !off;
  return off ? HUGE_VAL : big_threshold(c->nd, factor);
}

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

static void temporal_release(ftkx_ctx *c);

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
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "ftkx_set_stream: sweeps pending, collect first");
  if (c->sr_open && !c->sr_internal) return fail(c, FTKX_E_INVALID, "ftkx_set_stream: series passes open (ftkx_sweep_series_submit), complete them first");
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return FTKX_OK;
}

int ftkx_set_options(ftkx_ctx *c, const ftkx_options *o)
{
  if (c) c->ahead.clear();
  if (!c || !o) return fail(c, FTKX_E_INVALID, "null argument");
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "ftkx_set_options: sweeps pending, collect first");
  if (c->sr_open && !c->sr_internal) return fail(c, FTKX_E_INVALID, "ftkx_set_options: series passes open (ftkx_sweep_series_submit), complete them first");
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
  // nothing of the old lattice stays: slices dropped under an open split pass are parked with it, not in `slices` -- its tail is waited for
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

constexpr size_t kSmoothWeights = 729;      // ftkx_ctx::d_conv_w: where the smoothing's weights start

// ---- what every way of making a slice resident shares -----------------------------------------------------------------------------------
// the checks in front of a push of timestep t
static int push_checks(ftkx_ctx *c, int t, int on_device, bool scalar_only, bool have_field)
{
  if (!c->mesh_set) return fail(c, FTKX_E_INVALID, "push: call ftkx_set_mesh first");
  if (t < 0) return fail(c, FTKX_E_INVALID, "push: negative timestep");
  if (on_device < 0 || on_device > 2) return fail(c, FTKX_E_INVALID, "push: on_device must be 0, 1 or 2");
  if (!have_field) return fail(c, FTKX_E_INVALID, "push: missing field pointer");
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "push: sweeps pending, collect first");
  if (c->slices.empty()) c->scalar_mode = -1;
  if (c->scalar_mode >= 0 && c->scalar_mode != (scalar_only ? 1 : 0))
    return fail(c, FTKX_E_INVALID, "push: scalar and vector slices cannot be mixed in one context");
  return FTKX_OK;
}

// a field array of `count` doubles out of the pool, or a new one (a caller that fails afterwards lets it go out of scope: freed, not pooled)
static int take_pooled(ftkx_ctx *c, size_t count, ftkx_block &dst) { return c->arrays.take(c, FTKX_ARRAY_FIELD, count * sizeof(double), dst); }

// ... and back, behind work queued on the context's stream that may still read it: whatever takes it out next is ordered behind that work
// by the same stream (upload.cpp waits for it too); where the pool is full it is freed, once that work is through
static void give_pooled(ftkx_ctx *c, ftkx_block &&b)
{
  if (c->arrays.held[FTKX_ARRAY_FIELD].size() >= kPoolCap) (void)hipStreamSynchronize(c->stream);
  c->arrays.give(FTKX_ARRAY_FIELD, std::move(b), kPoolCap);
}

// the slice of timestep t, where there is one, leaves (its arrays are in the pool for what replaces it)
static void evict_slice(ftkx_ctx *c, int t)
{
  auto it = c->slices.find(t);
  if (it != c->slices.end()) { free_slice(it->second, c); c->slices.erase(it); }
}

// `s` -- arrays the context owns or borrows, complete in the order of its stream -- becomes the resident slice t
static void install_slice(ftkx_ctx *c, int t, Slice &s, bool scalar_only)
{
  s.mask_gen = ++ c->mask_epoch;
  c->slices[t] = std::move(s);
  c->scalar_mode = scalar_only ? 1 : 0;
}

extern "C++" {      // (templates on the source's element type)
// dst -- `count` doubles of the context's own -- becomes the snapshot `src` as a resident slice holds it: widened where T is float,
// convolved where `smooth` says so.  T = double without smoothing is a plain copy into dst.  Otherwise ONE kernel on the context's stream
// reads the source and writes dst (float + smoothing: the convolution stages the floats as doubles itself, no widened copy is written and
// read back).  That kernel reads this device's memory only: a host source, and a device source that lives on another device, goes through
// a staging buffer first -- FP64: a pooled array, which goes back to the pool at once; float32: the context's f32_stage block.
//
// The staging block is written by every float32 push and read by the kernel of the push before, which may still run.  What orders them:
// upload_from_host either copies on the context's stream itself, or -- staged_upload, on DMA streams of its own -- makes those streams wait
// for an event recorded on the context's stream unless that stream is idle (upload.cpp, E.gate); a peer copy is queued on the context's
// stream; a block that has to grow is freed only after the stream of its last reader has been waited for (reserve's drain).  All of that
// holds for ONE stream: where ftkx_set_stream has changed it since the last reader was queued, that reader's stream is waited for here.
//
// Perturbation and clamp (ftkx_set_perturbation, ftkx_set_clamp), where either is on: `t` is the snapshot's number, and the adjust kernel
// (adjust_kernels.hip) is the LAST kernel of the chain -- the stream's order, widen -> conv -> perturb -> clamp.  Without smoothing it is the
// only kernel: a float source goes through adjust_kernel<float> in place of the widen kernel; a host FP64 source (and one on another
// device) is brought straight into dst and adjusted in place, no staging array; an FP64 source on this device is read where it lies and
// written adjusted into dst.  With smoothing the convolution runs as ever and adjust_kernel<double> runs in place on its output.  With
// both settings off nothing here is queued that was not queued before there were such settings.
template <class T> static void queue_adjust(ftkx_ctx *c, const T *from, size_t count, int t, double *dst)
{
  const ftkx::AdjustArgs a{c->adj.sigma, c->adj.seed, t, c->adj.lo, c->adj.hi};
  ftkx::launch_adjust<T>(from, count, c->adj.perturb, c->adj.clamp, a, dst, c->stream);
  if (std::is_same<T, float>::value) c->adj_from_float ++;
  else if ((const void *)from == (const void *)dst) c->adj_in_place ++;
  else c->adj_out_of_place ++;
}

// raw: the array is no snapshot of the stream's (an aux array, ftkx_push_aux_slice): perturbation and clamp pass it by.
template <class T> static int stage_into(ftkx_ctx *c, const T *src, size_t count, int on_device, bool smooth, double *dst, int t, bool raw = false)
{
  constexpr bool f32 = std::is_same<T, float>::value;
  const bool adjust = !raw && c->adj.on();
  if constexpr (!f32) if (!smooth && adjust) {
    const bool here = on_device != 0 && ftkx_pointer_device(src) == c->device;
    if (on_device == 0) { if (int rc = upload_from_host(c, dst, src, count * sizeof(T))) return rc; }
    else if (!here && hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDefault, c->stream) != hipSuccess) return fail(c, FTKX_E_DEVICE, "push: copy of the source failed");
    queue_adjust<double>(c, here ? src : dst, count, t, dst);
    HIP_TRY(c, hipGetLastError());
    return FTKX_OK;
  }
  if (!f32 && !smooth) {
    // 0: host memory; 2: device memory of ANY device (a multi-device tracker hands one snapshot to two contexts), copied
    if (on_device == 0) return upload_from_host(c, dst, src, count * sizeof(T));
    if (hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDefault, c->stream) != hipSuccess) return fail(c, FTKX_E_DEVICE, "push: copy of the source failed");
    return FTKX_OK;
  }
  const T *from = src;
  ftkx_block tmp;
  if (on_device == 0 || ftkx_pointer_device(src) != c->device) {
    void *stage = nullptr;
    if (f32) {
      if (c->f32_stage_reader && c->f32_stage_reader != c->stream) HIP_TRY(c, hipStreamSynchronize(c->f32_stage_reader));
      c->f32_stage_reader = nullptr;
      if (int rc = c->f32_stage.reserve(c, count * sizeof(T), 0, c->stream)) return rc;
      stage = c->f32_stage.p;
    } else {
      if (int rc = take_pooled(c, count, tmp)) return rc;
      stage = tmp.p;
    }
    int rc = FTKX_OK;
    if (on_device == 0) rc = upload_from_host(c, stage, src, count * sizeof(T));
    else if (hipMemcpyAsync(stage, src, count * sizeof(T), hipMemcpyDefault, c->stream) != hipSuccess) rc = fail(c, FTKX_E_DEVICE, "push: copy of the source failed");
    // (a failed copy: nothing of it is in flight any more -- upload.cpp drains its DMA streams before it reports an error, and a
    // hipMemcpyAsync that was refused was never queued -- but what the buffer holds is unknown and the device may be in an error state:
    // a pooled buffer is freed with `tmp`, not pooled; the staging block is overwritten by the next push anyway)
    if (rc) return rc;
    from = static_cast<const T *>(stage);
    if (f32) c->f32_stage_reader = c->stream;
  }
  if (smooth) {
    ftkx::launch_conv<T>(c->nd, from, (int)c->ext_sz[0], (int)c->ext_sz[1], (int)c->ext_sz[2], c->d_conv_w.as<double>() + kSmoothWeights, c->smooth_ksize, dst, c->stream);
    if (f32) c->f32_direct ++;
    if (adjust) queue_adjust<double>(c, dst, count, t, dst);
  } else if constexpr (f32) {
    if (adjust) queue_adjust<float>(c, from, count, t, dst);
    else { ftkx::launch_widen(from, count, dst, c->stream); c->f32_widened ++; }
  }
  const hipError_t e = hipGetLastError();
  if (tmp.p) give_pooled(c, std::move(tmp));
  HIP_TRY(c, e);
  return FTKX_OK;
}

// one array of a push (null: none) into `dst`: an FP64 array on this device from which nothing has to be computed is adopted as it is
// (on_device 1); everything else becomes a pooled array that stage_into fills
template <class T> static int take_array(ftkx_ctx *c, const T *src, size_t count, int on_device, bool smooth, int t, ftkx_block &dst)
{
  if (!src) return FTKX_OK;
  if constexpr (!std::is_same<T, float>::value) if (on_device == 1 && !smooth && !c->adj.on()) { dst = ftkx_block::lent(const_cast<double *>(src), count * sizeof(double)); return FTKX_OK; }
  if (int rc = take_pooled(c, count, dst)) return rc;
  return stage_into(c, src, count, on_device, smooth, dst.as<double>(), t);
}

// ---- vector snapshots given as one array per component (concat_kernels.hip) --------------------------------------------------------------
// what every launch of the concat kernel asks of its arguments (dst null: an array of the context's own, not taken yet); nothing is queued
template <class T> static int planar_args(ftkx_ctx *c, const char *who, const T *const *planes, int nc, size_t count, const double *dst)
{
  if (!planes) return fail(c, FTKX_E_INVALID, "%s: null argument", who);
  if (nc != 2 && nc != 3) return fail(c, FTKX_E_INVALID, "%s: 2 or 3 components, not %d", who, nc);
  if (count < 1) return fail(c, FTKX_E_INVALID, "%s: count must be positive", who);
  for (int k = 0; k < nc; k ++) {
    if (!planes[k]) return fail(c, FTKX_E_INVALID, "%s: plane %d is null", who, k);
    if ((size_t)planes[k] & (sizeof(T) - 1)) return fail(c, FTKX_E_INVALID, "%s: plane %d must be a multiple of its element's size", who, k);
  }
  if (!dst) return FTKX_OK;
  if ((size_t)dst & 7) return fail(c, FTKX_E_INVALID, "%s: dst must be a multiple of 8", who);
  for (int k = 0; k < nc; k ++)
    if ((const char *)planes[k] < (const char *)(dst + count * (size_t)nc) && (const char *)dst < (const char *)(planes[k] + count))
      return fail(c, FTKX_E_INVALID, "%s: plane %d and the output overlap", who, k);
  return FTKX_OK;
}

template <class T> static void queue_concat(ftkx_ctx *c, const T *const *planes, int nc, size_t count, double *dst)
{
  if (ftkx::launch_concat<T>(planes, nc, count, dst, c->stream)) c->planar_vec ++; else c->planar_scalar ++;
}

// dst -- n * nc doubles of the context's own -- becomes what stage_into makes of the host-interleaved array of the nc planes (n elements
// each): the concat kernel writes it, widening where T is float, and adjust_kernel<double> runs in place behind it where perturbation or
// clamp is on (the stream's order: concat -> perturb -> clamp; the noise's index is the flat index of the interleaved array).  The kernel
// reads this device's memory only.  on_device 1 with every plane on this device: read where they lie.  Everything else is staged first,
// plane behind plane in ONE block -- float32: the context's f32_stage, every plane at a multiple of 16 bytes, ordered against its last
// reader as stage_into orders it; FP64: a pooled array of n * nc doubles, which goes back to the pool at once.
template <class T> static int concat_into(ftkx_ctx *c, const T *const *planes, int nc, size_t n, int on_device, double *dst, int t)
{
  constexpr bool f32 = std::is_same<T, float>::value;
  bool here = on_device == 1;
  for (int k = 0; here && k < nc; k ++) here = ftkx_pointer_device(planes[k]) == c->device;
  const T *from[3] = {planes[0], planes[1], nc > 2 ? planes[2] : nullptr};
  ftkx_block tmp;
  if (!here) {
    const size_t bytes = n * sizeof(T), pitch = f32 ? (bytes + 15) & ~(size_t)15 : bytes;
    char *stage = nullptr;
    if (f32) {
      if (c->f32_stage_reader && c->f32_stage_reader != c->stream) HIP_TRY(c, hipStreamSynchronize(c->f32_stage_reader));
      c->f32_stage_reader = nullptr;
      if (int rc = c->f32_stage.reserve(c, pitch * (size_t)nc, 0, c->stream)) return rc;
      stage = static_cast<char *>(c->f32_stage.p);
    } else {
      if (int rc = take_pooled(c, n * (size_t)nc, tmp)) return rc;
      stage = static_cast<char *>(tmp.p);
    }
    for (int k = 0; k < nc; k ++) {
      // (a failed copy: as in stage_into -- `tmp` is freed, not pooled; the staging block is overwritten by the next push)
      if (on_device == 0) { if (int rc = upload_from_host(c, stage + (size_t)k * pitch, planes[k], bytes)) return rc; }
      else if (hipMemcpyAsync(stage + (size_t)k * pitch, planes[k], bytes, hipMemcpyDefault, c->stream) != hipSuccess) return fail(c, FTKX_E_DEVICE, "push: copy of plane %d failed", k);
      from[k] = reinterpret_cast<const T *>(stage + (size_t)k * pitch);
    }
    if (f32) c->f32_stage_reader = c->stream;
  }
  queue_concat<T>(c, from, nc, n, dst);
  if (c->adj.on()) queue_adjust<double>(c, dst, n * (size_t)nc, t, dst);
  const hipError_t e = hipGetLastError();
  if (tmp.p) give_pooled(c, std::move(tmp));
  HIP_TRY(c, e);
  return FTKX_OK;
}

// ftkx_push_slice_planar*: push_common for a V that arrives as nc planes; J and S as there (interleaved)
template <class T> static int push_planar_common(ftkx_ctx *c, int t, const T *const *Vc, int nc, const T *J, const T *S, int on_device)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = push_checks(c, t, on_device, false, Vc != nullptr)) return rc;
  if (nc != c->nd) return fail(c, FTKX_E_INVALID, "push: %d planes for a context of %d dimensions", nc, c->nd);
  const size_t n = n_vertices(c);
  if (int rc = planar_args<T>(c, "push", Vc, nc, n, nullptr)) return rc;
  if (c->smooth_ksize) return fail(c, FTKX_E_UNSUPPORTED, "push: spatial smoothing is set and takes scalar slices only (ftkx_push_scalar_slice)");
  if (c->adj.on() && (J || S)) return fail(c, FTKX_E_UNSUPPORTED, "push: perturbation or clamp is set and takes V alone (no J, no S beside it)");
  HIP_TRY(c, hipSetDevice(c->device));
  evict_slice(c, t);
  Slice s;      // (what was already taken is freed with `s`)
  if (int rc = take_array<T>(c, S, n, on_device, false, t, s.S)) return rc;
  if (int rc = take_pooled(c, n * (size_t)nc, s.V)) return rc;
  if (int rc = concat_into<T>(c, Vc, nc, n, on_device, s.V.as<double>(), t)) return rc;
  if (int rc = take_array<T>(c, J, n * (size_t)nc * (size_t)nc, on_device, false, t, s.J)) return rc;
  // planes on a device are read by the kernel and never adopted: the call returns once they have been read (a host source has been staged)
  if (on_device != 0) HIP_TRY(c, hipStreamSynchronize(c->stream));
  install_slice(c, t, s, false);
  return FTKX_OK;
}

// T: the element type of the caller's arrays (double, or float: ftkx_push_*_f32).  The resident slice is FP64 either way
template <class T> static int push_common(ftkx_ctx *c, int t, const T *V, const T *J, const T *S, int on_device, bool scalar_only)
{
  constexpr bool f32 = std::is_same<T, float>::value;
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = push_checks(c, t, on_device, scalar_only, scalar_only ? S != nullptr : V != nullptr)) return rc;
  // conv_gaussian dispatches on the array's nd(): a vector field would be convolved across its components (conv.hh:213-221) -- not reproduced
  if (c->smooth_ksize && !scalar_only) return fail(c, FTKX_E_UNSUPPORTED, "push: spatial smoothing is set and takes scalar slices only (ftkx_push_scalar_slice)");
  // the stream delivers ONE array, which perturb() and clamp() walk over (all n * nd elements of a vector field, by their flat index)
  const bool adjust = c->adj.on();
  if (adjust && !scalar_only && (J || S)) return fail(c, FTKX_E_UNSUPPORTED, "push: perturbation or clamp is set and takes V alone (no J, no S beside it)");
  HIP_TRY(c, hipSetDevice(c->device));
  evict_slice(c, t);
  Slice s;
  const size_t n = n_vertices(c);
  const int nd = c->nd;
  // (smoothing applies to S alone: vector pushes were refused above)
  auto take = [&](const T *src, size_t count, bool smooth, ftkx_block &dst) -> int { return take_array<T>(c, src, count, on_device, smooth, t, dst); };
  if (int rc = take(S, n, c->smooth_ksize != 0, s.S)) return rc;      // (here and below: what was already taken is freed with `s`)
  if (!scalar_only) {
    if (int rc = take(V, n * nd, false, s.V)) return rc;
    if (int rc = take(J, n * nd * nd, false, s.J)) return rc;
  }
  // scalar input: V = gradient2D/3D(S) is never materialised -- every kernel evaluates it where it needs it, with the
  // reference's exact operations (ndarray/grad.hh), so the slice costs 8 bytes per vertex of HBM instead of 8 + 8*nd.
  // the source buffers may be reused by the caller on return: a device source (2) has to be read first; a host source has been staged
  // completely by upload_from_host (nothing to wait for: the DMAs run on while the caller produces its next snapshot)
  // (smoothing, perturbation or clamp, and a float32 source: a borrowed array (1) is read by the kernel and never adopted -- the call returns once it has been read, like 2)
  if (on_device == 2 || (on_device == 1 && (c->smooth_ksize || f32 || adjust))) HIP_TRY(c, hipStreamSynchronize(c->stream));
  install_slice(c, t, s, scalar_only);
  return FTKX_OK;
}

}  // extern "C++"

int ftkx_push_slice(ftkx_ctx *c, int t, const double *V, const double *J, const double *S, int on_device)
{ return push_common<double>(c, t, V, J, S, on_device, false); }

int ftkx_push_scalar_slice(ftkx_ctx *c, int t, const double *S, int on_device)
{ return push_common<double>(c, t, nullptr, nullptr, S, on_device, true); }

int ftkx_push_slice_f32(ftkx_ctx *c, int t, const float *V, const float *J, const float *S, int on_device)
{ return push_common<float>(c, t, V, J, S, on_device, false); }

int ftkx_push_scalar_slice_f32(ftkx_ctx *c, int t, const float *S, int on_device)
{ return push_common<float>(c, t, nullptr, nullptr, S, on_device, true); }

int ftkx_push_slice_planar(ftkx_ctx *c, int t, const double *const *Vc, int nc, const double *J, const double *S, int on_device)
{ return push_planar_common<double>(c, t, Vc, nc, J, S, on_device); }

int ftkx_push_slice_planar_f32(ftkx_ctx *c, int t, const float *const *Vc, int nc, const float *J, const float *S, int on_device)
{ return push_planar_common<float>(c, t, Vc, nc, J, S, on_device); }

// ---- auxiliary scalar fields sampled at critical points (sample_steps.hpp, sample_kernels.hip) -------------------------------------------
// the aux arrays of timestep t leave: owned ones to the pool (only the sample kernel reads them, and ftkx_sample_aux has waited for it)
static void drop_aux(ftkx_ctx *c, int t)
{
  auto it = c->aux.find(t);
  if (it == c->aux.end()) return;
  for (ftkx_block &b : it->second.A) if (b.p) give_pooled(c, std::move(b));
  c->aux.erase(it);
}

extern "C++" {
template <class T> static int push_aux_common(ftkx_ctx *c, int t, int slot, const T *A, int on_device)
{
  constexpr bool f32 = std::is_same<T, float>::value;
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!c->mesh_set) return fail(c, FTKX_E_INVALID, "ftkx_push_aux_slice: call ftkx_set_mesh first");
  if (t < 0) return fail(c, FTKX_E_INVALID, "ftkx_push_aux_slice: negative timestep");
  if (slot != 1 && slot != 2) return fail(c, FTKX_E_INVALID, "ftkx_push_aux_slice: slot must be 1 or 2, not %d (slot 0 is the scalar field of the sweep)", slot);
  if (on_device < 0 || on_device > 2) return fail(c, FTKX_E_INVALID, "ftkx_push_aux_slice: on_device must be 0, 1 or 2");
  if (!A || ((size_t)A & (sizeof(T) - 1))) return fail(c, FTKX_E_INVALID, "ftkx_push_aux_slice: the array is null or not a multiple of its element's size");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = n_vertices(c);
  ftkx_block b;
  if (!f32 && on_device == 1) b = ftkx_block::lent(const_cast<T *>(A), n * sizeof(double));
  else {
    if (int rc = take_pooled(c, n, b)) return rc;
    if (int rc = stage_into<T>(c, A, n, on_device, false, b.as<double>(), t, true)) return rc;      // (b is freed, not pooled)
    // a device source is read by a copy or by the widen kernel and never adopted: the call returns once it has been read
    if (on_device != 0) HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  ftkx_block &dst = c->aux[t].A[slot - 1];
  if (dst.p) give_pooled(c, std::move(dst));
  dst = std::move(b);
  return FTKX_OK;
}
}  // extern "C++"

int ftkx_push_aux_slice(ftkx_ctx *c, int t, int slot, const double *A, int on_device) { return push_aux_common<double>(c, t, slot, A, on_device); }
int ftkx_push_aux_slice_f32(ftkx_ctx *c, int t, int slot, const float *A, int on_device) { return push_aux_common<float>(c, t, slot, A, on_device); }

// What a launch of the sample kernel needs, on the device when this returns FTKX_OK with slots != 0: the records' (tag, aux word) pairs and
// behind them the table of slice pointers in sm_d_in, room for the results in sm_d_out and sm_h_out.  Every check of ftkx_sample_aux is
// made here, before anything is written anywhere.
// f(begin, end) over the records of a call: on a few host threads from 2^18 records (below that starting the threads costs more than the
// loops: 62 181 records of bench.py's C2 take 0.5 ms on one thread, 0.76 ms on eight)
extern "C++" {
template <class F> static void sample_ranges(size_t n, F f)
{
  if (n < ((size_t)1 << 18)) f((size_t)0, n);
  else ftkx::for_ranges_on_threads(n, f);
}
}  // extern "C++"

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
  m.tag_mode = c->opt.tag_mode;
  m.scalar_mode = c->scalar_mode == 1;
  for (int d = 0; d < 3; d ++) {
    m.dom_lb[d] = (int)c->dom_st[d]; m.dom_sz[d] = (int)c->dom_sz[d];
    m.core_st[d] = (int)c->core_st[d]; m.core_sz[d] = (int)c->core_sz[d];
    m.ext_st[d] = (int)c->ext_st[d]; m.ext_sz[d] = (int)c->ext_sz[d];
  }
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
  std::vector<hipEvent_t> ev(2 * (size_t)reps, nullptr);
  auto run = [&]() -> int {
    for (hipEvent_t &e : ev) HIP_TRY(c, hipEventCreate(&e));
    for (int i = 0; i < reps; i ++) {
      HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i], c->stream));
      ftkx::launch_sample(c->nd, P.m, P.d_in, n, P.d_tab, P.t_min, P.slots, c->sm_d_out.as<double>(), c->stream);
      HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i + 1], c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < reps; i ++) { float t = 0; HIP_TRY(c, hipEventElapsedTime(&t, ev[2 * (size_t)i], ev[2 * (size_t)i + 1])); ms[i] = t; }
    return FTKX_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  return rc;
}

int ftkx_debug_sample_counts(const ftkx_ctx *c, unsigned long long *launches, unsigned long long *records)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (launches) *launches = c->sm_launches;
  if (records) *records = c->sm_records;
  return FTKX_OK;
}

int ftkx_debug_planar_counts(const ftkx_ctx *c, unsigned long long *vec_launches, unsigned long long *scalar_launches)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (vec_launches) *vec_launches = c->planar_vec;
  if (scalar_launches) *scalar_launches = c->planar_scalar;
  return FTKX_OK;
}

int ftkx_debug_f32_counts(const ftkx_ctx *c, unsigned long long *widened, unsigned long long *convolved_direct)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (widened) *widened = c->f32_widened;
  if (convolved_direct) *convolved_direct = c->f32_direct;
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

#define DERIVE_PROLOGUE(c) do { if (!(c)) return fail(nullptr, FTKX_E_INVALID, "null context"); HIP_TRY((c), hipSetDevice((c)->device)); } while (0)

int ftkx_gradient2D(ftkx_ctx *c, const double *S, int DW, int DH, double *V)
{ DERIVE_PROLOGUE(c); ftkx::launch_gradient2d(S, DW, DH, V, c->stream); HIP_TRY(c, hipGetLastError()); HIP_TRY(c, hipStreamSynchronize(c->stream)); return FTKX_OK; }
int ftkx_jacobian2D(ftkx_ctx *c, const double *V, int DW, int DH, int symmetric, double *J)
{ DERIVE_PROLOGUE(c); ftkx::launch_jacobian2d(V, DW, DH, symmetric, J, c->stream); HIP_TRY(c, hipGetLastError()); HIP_TRY(c, hipStreamSynchronize(c->stream)); return FTKX_OK; }
int ftkx_gradient3D(ftkx_ctx *c, const double *S, int DW, int DH, int DD, double *V)
{ DERIVE_PROLOGUE(c); ftkx::launch_gradient3d(S, DW, DH, DD, V, c->stream); HIP_TRY(c, hipGetLastError()); HIP_TRY(c, hipStreamSynchronize(c->stream)); return FTKX_OK; }
int ftkx_jacobian3D(ftkx_ctx *c, const double *V, int DW, int DH, int DD, double *J)
{ DERIVE_PROLOGUE(c); ftkx::launch_jacobian3d(V, DW, DH, DD, J, c->stream); HIP_TRY(c, hipGetLastError()); HIP_TRY(c, hipStreamSynchronize(c->stream)); return FTKX_OK; }


// ---- spatial Gaussian smoothing (ndarray/conv.hh) ----------------------------------------------------------------------------------------
static bool conv_ksize_ok(int ksize) { return ksize >= 1 && ksize <= 9 && (ksize & 1) == 1; }

// gaussian_kernel2D (conv.hh:74-100) / gaussian_kernel3D (165-196) with the host's exp.  The order in which `sum` grows is the reference's
// loop order -- 2D: y outer, x inner; 3D: y outer, then x, then z innermost -- not memory order.
int ftkx_gaussian_kernel(int nd, double sigma, int ksize, double *weights)
{
  if (nd != 2 && nd != 3) return fail(nullptr, FTKX_E_INVALID, "ftkx_gaussian_kernel: nd must be 2 or 3");
  if (!conv_ksize_ok(ksize)) return fail(nullptr, FTKX_E_INVALID, "ftkx_gaussian_kernel: ksize must be odd and in [1, 9] (got %d)", ksize);
  if (!std::isfinite(sigma) || !(sigma > 0)) return fail(nullptr, FTKX_E_INVALID, "ftkx_gaussian_kernel: sigma must be finite and positive");
  if (!weights) return fail(nullptr, FTKX_E_INVALID, "ftkx_gaussian_kernel: null output");
  const double center = static_cast<double>(ksize - 1) * .5;
  const double s = 2. * sigma * sigma;
  double sum = 0.;
  const int nz = nd == 3 ? ksize : 1;
  for (int j = 0; j < ksize; ++ j)
    for (int i = 0; i < ksize; ++ i)
      for (int k = 0; k < nz; ++ k) {
        const double x = static_cast<double>(i) - center, y = static_cast<double>(j) - center, z = static_cast<double>(k) - center;
        const double r = nd == 3 ? x * x + y * y + z * z : x * x + y * y;
        double &w = weights[((size_t)k * ksize + j) * ksize + i];
        w = std::exp(-r / s);
        sum += w;
      }
  const int n = ksize * ksize * nz;
  for (int i = 0; i < n; ++ i) weights[i] /= sum;
  return FTKX_OK;
}

static int conv_weights(ftkx_ctx *c, const double *weights, int n, size_t at)
{
  if (const int rc = c->d_conv_w.reserve(c, 2 * kSmoothWeights * sizeof(double))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_conv_w.as<double>() + at, weights, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return FTKX_OK;
}

extern "C++" {
template <class T> static int conv_common(ftkx_ctx *c, int nd, const T *S, int DW, int DH, int DD, const double *weights, int ksize, double *out)
{
  DERIVE_PROLOGUE(c);
  if (!S || !out || !weights) return fail(c, FTKX_E_INVALID, "ftkx_conv%dD: null argument", nd);
  if (DW < 1 || DH < 1 || DD < 1) return fail(c, FTKX_E_INVALID, "ftkx_conv%dD: extents must be positive", nd);
  if (!conv_ksize_ok(ksize)) return fail(c, FTKX_E_INVALID, "ftkx_conv%dD: ksize must be odd and in [1, 9] (got %d)", nd, ksize);
  const size_t n = (size_t)DW * (size_t)DH * (size_t)DD;
  if ((const char *)S < (const char *)(out + n) && (const char *)out < (const char *)(S + n)) return fail(c, FTKX_E_INVALID, "ftkx_conv%dD: input and output overlap", nd);
  int taps = ksize * ksize * (nd == 3 ? ksize : 1);
  if (int rc = conv_weights(c, weights, taps, 0)) return rc;
  ftkx::launch_conv<T>(nd, S, DW, DH, DD, c->d_conv_w.as<double>(), ksize, out, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the next call may overwrite the weights; the caller may read `out`)
  return FTKX_OK;
}
}  // extern "C++"

int ftkx_conv2D(ftkx_ctx *c, const double *S, int DW, int DH, const double *weights, int ksize, double *out)
{ return conv_common<double>(c, 2, S, DW, DH, 1, weights, ksize, out); }
int ftkx_conv3D(ftkx_ctx *c, const double *S, int DW, int DH, int DD, const double *weights, int ksize, double *out)
{ return conv_common<double>(c, 3, S, DW, DH, DD, weights, ksize, out); }
int ftkx_conv2D_f32(ftkx_ctx *c, const float *S, int DW, int DH, const double *weights, int ksize, double *out)
{ return conv_common<float>(c, 2, S, DW, DH, 1, weights, ksize, out); }
int ftkx_conv3D_f32(ftkx_ctx *c, const float *S, int DW, int DH, int DD, const double *weights, int ksize, double *out)
{ return conv_common<float>(c, 3, S, DW, DH, DD, weights, ksize, out); }

// ---- float32 -> FP64 (widen_kernels.hip) ---------------------------------------------------------------------------------------------------
static int widen_args(ftkx_ctx *c, const char *who, const float *src, size_t count, const double *dst)
{
  if (!src || !dst) return fail(c, FTKX_E_INVALID, "%s: null argument", who);
  if (count < 1) return fail(c, FTKX_E_INVALID, "%s: count must be positive", who);
  if (((size_t)src & 3) || ((size_t)dst & 7)) return fail(c, FTKX_E_INVALID, "%s: src must be a multiple of 4 bytes and dst a multiple of 8", who);
  if ((const char *)src < (const char *)(dst + count) && (const char *)dst < (const char *)(src + count)) return fail(c, FTKX_E_INVALID, "%s: input and output overlap", who);
  return FTKX_OK;
}

int ftkx_widen_f32(ftkx_ctx *c, const float *src, size_t count, double *dst)
{
  DERIVE_PROLOGUE(c);
  if (int rc = widen_args(c, "ftkx_widen_f32", src, count, dst)) return rc;
  ftkx::launch_widen(src, count, dst, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the caller may read `dst`)
  return FTKX_OK;
}

// profiling aid (tools/push_f32_time.py): the widen kernel `reps` times back to back, a pair of events around every launch
int ftkx_debug_widen_relaunch(ftkx_ctx *c, const float *src, size_t count, double *dst, int reps, double *ms)
{
  DERIVE_PROLOGUE(c);
  if (!ms || reps < 1) return fail(c, FTKX_E_INVALID, "ftkx_debug_widen_relaunch: bad argument");
  if (int rc = widen_args(c, "ftkx_debug_widen_relaunch", src, count, dst)) return rc;
  std::vector<hipEvent_t> ev(2 * (size_t)reps, nullptr);
  auto run = [&]() -> int {
    for (hipEvent_t &e : ev) HIP_TRY(c, hipEventCreate(&e));
    for (int i = 0; i < reps; i ++) {
      HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i], c->stream));
      ftkx::launch_widen(src, count, dst, c->stream);
      HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i + 1], c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < reps; i ++) { float t = 0; HIP_TRY(c, hipEventElapsedTime(&t, ev[2 * (size_t)i], ev[2 * (size_t)i + 1])); ms[i] = t; }
    return FTKX_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  return rc;
}

// ---- component planes -> interleaved FP64 (concat_kernels.hip) ------------------------------------------------------------------------------
extern "C++" {
// the kernel alone on device pointers, `reps` times back to back; ms (nullable: reps == 1): a pair of events around every launch
template <class T> static int concat_common(ftkx_ctx *c, const char *who, const T *const *planes, int nc, size_t count, double *dst, int reps, double *ms)
{
  DERIVE_PROLOGUE(c);
  if (!dst || (ms ? reps < 1 : reps != 1)) return fail(c, FTKX_E_INVALID, "%s: bad argument", who);
  if (int rc = planar_args<T>(c, who, planes, nc, count, dst)) return rc;
  std::vector<hipEvent_t> ev(ms ? 2 * (size_t)reps : 0, nullptr);
  auto run = [&]() -> int {
    for (hipEvent_t &e : ev) HIP_TRY(c, hipEventCreate(&e));
    for (int i = 0; i < reps; i ++) {
      if (ms) HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i], c->stream));
      queue_concat<T>(c, planes, nc, count, dst);
      if (ms) HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i + 1], c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the caller may read `dst`)
    for (int i = 0; ms && i < reps; i ++) { float tt = 0; HIP_TRY(c, hipEventElapsedTime(&tt, ev[2 * (size_t)i], ev[2 * (size_t)i + 1])); ms[i] = tt; }
    return FTKX_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  return rc;
}
}  // extern "C++"

int ftkx_concat(ftkx_ctx *c, const double *const *planes, int nc, size_t count, double *dst)
{ return concat_common<double>(c, "ftkx_concat", planes, nc, count, dst, 1, nullptr); }
int ftkx_concat_f32(ftkx_ctx *c, const float *const *planes, int nc, size_t count, double *dst)
{ return concat_common<float>(c, "ftkx_concat_f32", planes, nc, count, dst, 1, nullptr); }

// profiling aid (tools/push_planar_time.py)
int ftkx_debug_concat_relaunch(ftkx_ctx *c, const void *const *planes, int nc, int planes_are_f32, size_t count, double *dst, int reps, double *ms)
{
  if (c && !ms) return fail(c, FTKX_E_INVALID, "ftkx_debug_concat_relaunch: bad argument");
  if (planes_are_f32) return concat_common<float>(c, "ftkx_debug_concat_relaunch", reinterpret_cast<const float *const *>(planes), nc, count, dst, reps, ms);
  return concat_common<double>(c, "ftkx_debug_concat_relaunch", reinterpret_cast<const double *const *>(planes), nc, count, dst, reps, ms);
}

// ---- perturbation and clamp (adjust_kernels.hip) ---------------------------------------------------------------------------------------------
static int adjust_settings(ftkx_ctx *c, const char *who, double sigma, int clamp_on, double lo, double hi, bool need_one)
{
  if (!std::isfinite(sigma) || sigma < 0) return fail(c, FTKX_E_INVALID, "%s: sigma must be finite and not negative", who);
  if (clamp_on && (std::isnan(lo) || std::isnan(hi))) return fail(c, FTKX_E_INVALID, "%s: a clamp bound is NaN", who);
  if (need_one && sigma == 0 && !clamp_on) return fail(c, FTKX_E_INVALID, "%s: neither perturbation (sigma > 0) nor clamp asked for", who);
  return FTKX_OK;
}

static int adjust_not_now(ftkx_ctx *c, const char *who)
{
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "%s: sweeps pending, collect first", who);
  if (c->sr_open && !c->sr_internal) return fail(c, FTKX_E_INVALID, "%s: series passes open (ftkx_sweep_series_submit), complete them first", who);
  return FTKX_OK;
}

int ftkx_set_perturbation(ftkx_ctx *c, double sigma, unsigned long long seed)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = adjust_not_now(c, "ftkx_set_perturbation")) return rc;
  if (int rc = adjust_settings(c, "ftkx_set_perturbation", sigma, 0, 0, 0, false)) return rc;
  c->adj.perturb = sigma > 0; c->adj.sigma = sigma; c->adj.seed = seed;
  return FTKX_OK;
}

int ftkx_set_clamp(ftkx_ctx *c, int on, double lo, double hi)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = adjust_not_now(c, "ftkx_set_clamp")) return rc;
  if (int rc = adjust_settings(c, "ftkx_set_clamp", 0, on, lo, hi, false)) return rc;
  c->adj.clamp = on != 0; c->adj.lo = on ? lo : 0; c->adj.hi = on ? hi : 0;
  return FTKX_OK;
}

extern "C++" {
template <class T> static int adjust_args(ftkx_ctx *c, const char *who, const T *src, size_t count, double sigma, int clamp_on, double lo, double hi, const double *dst)
{
  if (!src || !dst) return fail(c, FTKX_E_INVALID, "%s: null argument", who);
  if (count < 1) return fail(c, FTKX_E_INVALID, "%s: count must be positive", who);
  if (((size_t)src & (sizeof(T) - 1)) || ((size_t)dst & 7)) return fail(c, FTKX_E_INVALID, "%s: src must be a multiple of its element's size and dst a multiple of 8", who);
  if ((const void *)src != (const void *)dst && (const char *)src < (const char *)(dst + count) && (const char *)dst < (const char *)(src + count))
    return fail(c, FTKX_E_INVALID, "%s: input and output overlap (and are not the same array)", who);
  return adjust_settings(c, who, sigma, clamp_on, lo, hi, true);
}

template <class T> static int adjust_common(ftkx_ctx *c, const char *who, const T *src, size_t count, double sigma, unsigned long long seed, int t, int clamp_on, double lo, double hi,
                                            double *dst, int reps, double *ms)
{
  DERIVE_PROLOGUE(c);
  if (ms ? reps < 1 : reps != 1) return fail(c, FTKX_E_INVALID, "%s: bad argument", who);
  if (int rc = adjust_args<T>(c, who, src, count, sigma, clamp_on, lo, hi, dst)) return rc;
  const ftkx::AdjustArgs a{sigma, seed, t, lo, hi};
  std::vector<hipEvent_t> ev(ms ? 2 * (size_t)reps : 0, nullptr);
  auto run = [&]() -> int {
    for (hipEvent_t &e : ev) HIP_TRY(c, hipEventCreate(&e));
    for (int i = 0; i < reps; i ++) {
      if (ms) HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i], c->stream));
      ftkx::launch_adjust<T>(src, count, sigma > 0, clamp_on != 0, a, dst, c->stream);
      if (ms) HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i + 1], c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the caller may read `dst`)
    for (int i = 0; ms && i < reps; i ++) { float tt = 0; HIP_TRY(c, hipEventElapsedTime(&tt, ev[2 * (size_t)i], ev[2 * (size_t)i + 1])); ms[i] = tt; }
    return FTKX_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  return rc;
}
}  // extern "C++"

int ftkx_adjust(ftkx_ctx *c, const double *src, size_t count, double sigma, unsigned long long seed, int t, int clamp_on, double lo, double hi, double *dst)
{ return adjust_common<double>(c, "ftkx_adjust", src, count, sigma, seed, t, clamp_on, lo, hi, dst, 1, nullptr); }
int ftkx_adjust_f32(ftkx_ctx *c, const float *src, size_t count, double sigma, unsigned long long seed, int t, int clamp_on, double lo, double hi, double *dst)
{ return adjust_common<float>(c, "ftkx_adjust_f32", src, count, sigma, seed, t, clamp_on, lo, hi, dst, 1, nullptr); }

// profiling aid (tools/adjust_time.py): the adjust kernel `reps` times back to back, a pair of events around every launch.  In place with
// sigma > 0 every launch perturbs what the one before left: the time is the same, the values are not those of one launch.
int ftkx_debug_adjust_relaunch(ftkx_ctx *c, const void *src, int src_is_f32, size_t count, double sigma, unsigned long long seed, int t, int clamp_on, double lo, double hi,
                               double *dst, int reps, double *ms)
{
  if (c && !ms) return fail(c, FTKX_E_INVALID, "ftkx_debug_adjust_relaunch: bad argument");
  if (src_is_f32) return adjust_common<float>(c, "ftkx_debug_adjust_relaunch", (const float *)src, count, sigma, seed, t, clamp_on, lo, hi, dst, reps, ms);
  return adjust_common<double>(c, "ftkx_debug_adjust_relaunch", (const double *)src, count, sigma, seed, t, clamp_on, lo, hi, dst, reps, ms);
}

int ftkx_debug_adjust_counts(const ftkx_ctx *c, unsigned long long *from_float, unsigned long long *in_place, unsigned long long *out_of_place)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (from_float) *from_float = c->adj_from_float;
  if (in_place) *in_place = c->adj_in_place;
  if (out_of_place) *out_of_place = c->adj_out_of_place;
  return FTKX_OK;
}

// profiling aid (tools/conv_time.py): the convolution kernel `reps` times back to back, a pair of events around every launch
int ftkx_debug_conv_relaunch(ftkx_ctx *c, int nd, const double *S, int DW, int DH, int DD, const double *weights, int ksize, double *out, int reps, double *ms)
{
  DERIVE_PROLOGUE(c);
  if ((nd != 2 && nd != 3) || !S || !out || !weights || !ms || reps < 1 || DW < 1 || DH < 1 || DD < 1 || !conv_ksize_ok(ksize)) return fail(c, FTKX_E_INVALID, "ftkx_debug_conv_relaunch: bad argument");
  if (int rc = conv_weights(c, weights, ksize * ksize * (nd == 3 ? ksize : 1), 0)) return rc;
  std::vector<hipEvent_t> ev(2 * (size_t)reps, nullptr);
  int rc = FTKX_OK;
  auto run = [&]() -> int {
    for (hipEvent_t &e : ev) HIP_TRY(c, hipEventCreate(&e));
    for (int i = 0; i < reps; i ++) {
      HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i], c->stream));
      ftkx::launch_conv(nd, S, DW, DH, nd == 3 ? DD : 1, c->d_conv_w.as<double>(), ksize, out, c->stream);
      HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i + 1], c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < reps; i ++) { float t = 0; HIP_TRY(c, hipEventElapsedTime(&t, ev[2 * (size_t)i], ev[2 * (size_t)i + 1])); ms[i] = t; }
    return FTKX_OK;
  };
  rc = run();
  if (rc) (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  return rc;
}

int ftkx_set_spatial_smoothing(ftkx_ctx *c, double sigma, int ksize)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "ftkx_set_spatial_smoothing: sweeps pending, collect first");
  if (c->sr_open && !c->sr_internal) return fail(c, FTKX_E_INVALID, "ftkx_set_spatial_smoothing: series passes open (ftkx_sweep_series_submit), complete them first");
  if (ksize == 0) { c->smooth_ksize = 0; c->smooth_sigma = 0; return FTKX_OK; }
  double w[kSmoothWeights];
  if (int rc = ftkx_gaussian_kernel(c->nd, sigma, ksize, w)) { c->err = g_last_error; return rc; }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (a push queued under the old weights still reads them)
  if (int rc = conv_weights(c, w, ksize * ksize * (c->nd == 3 ? ksize : 1), kSmoothWeights)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (`w` is this call's)
  c->smooth_ksize = ksize; c->smooth_sigma = sigma;
  return FTKX_OK;
}

// ---- temporal Gaussian smoothing (filters/streaming_filter.hh) ---------------------------------------------------------------------------
// gaussian_kernel (conv.hh:50-72) with the host's exp; `sum` grows in index order
int ftkx_gaussian_kernel1d(double sigma, int ksize, double *weights)
{
  if (!ftkx::temporal_ksize_ok(ksize)) return fail(nullptr, FTKX_E_INVALID, "ftkx_gaussian_kernel1d: ksize must be odd and in [1, 9] (got %d)", ksize);
  if (!std::isfinite(sigma) || !(sigma > 0)) return fail(nullptr, FTKX_E_INVALID, "ftkx_gaussian_kernel1d: sigma must be finite and positive");
  if (!weights) return fail(nullptr, FTKX_E_INVALID, "ftkx_gaussian_kernel1d: null output");
  const double center = static_cast<double>(ksize - 1) * 0.5;
  const double s = 2. * sigma * sigma;
  double sum = 0.;
  for (int i = 0; i < ksize; ++ i) {
    const double x = static_cast<double>(i) - center;
    const double r = x * x;
    weights[i] = std::exp(-r / s);
    sum += weights[i];
  }
  for (int i = 0; i < ksize; ++ i) weights[i] /= sum;
  return FTKX_OK;
}

static int temporal_combine_args(ftkx_ctx *c, const char *who, const double *const *arrays, int ksize, const double *weights, size_t count, const double *out)
{
  if (!arrays || !weights || !out) return fail(c, FTKX_E_INVALID, "%s: null argument", who);
  if (!ftkx::temporal_ksize_ok(ksize)) return fail(c, FTKX_E_INVALID, "%s: ksize must be odd and in [1, 9] (got %d)", who, ksize);
  if (count < 1) return fail(c, FTKX_E_INVALID, "%s: count must be positive", who);
  for (int i = 0; i < ksize; i ++) {
    if (!arrays[i]) return fail(c, FTKX_E_INVALID, "%s: array %d is null", who, i);
    if (arrays[i] < out + count && out < arrays[i] + count) return fail(c, FTKX_E_INVALID, "%s: the output overlaps array %d", who, i);
  }
  return FTKX_OK;
}

int ftkx_temporal_combine(ftkx_ctx *c, const double *const *arrays, int ksize, const double *weights, size_t count, double *out)
{
  DERIVE_PROLOGUE(c);
  if (int rc = temporal_combine_args(c, "ftkx_temporal_combine", arrays, ksize, weights, count, out)) return rc;
  ftkx::launch_temporal(arrays, ksize, weights, count, out, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the caller may read `out`)
  return FTKX_OK;
}

// profiling aid (tools/temporal_time.py): the kernel `reps` times back to back, a pair of events around every launch
int ftkx_debug_temporal_relaunch(ftkx_ctx *c, const double *const *arrays, int ksize, const double *weights, size_t count, double *out, int reps, double *ms)
{
  DERIVE_PROLOGUE(c);
  if (!ms || reps < 1) return fail(c, FTKX_E_INVALID, "ftkx_debug_temporal_relaunch: bad argument");
  if (int rc = temporal_combine_args(c, "ftkx_debug_temporal_relaunch", arrays, ksize, weights, count, out)) return rc;
  std::vector<hipEvent_t> ev(2 * (size_t)reps, nullptr);
  auto run = [&]() -> int {
    for (hipEvent_t &e : ev) HIP_TRY(c, hipEventCreate(&e));
    for (int i = 0; i < reps; i ++) {
      HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i], c->stream));
      ftkx::launch_temporal(arrays, ksize, weights, count, out, c->stream);
      HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i + 1], c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < reps; i ++) { float t = 0; HIP_TRY(c, hipEventElapsedTime(&t, ev[2 * (size_t)i], ev[2 * (size_t)i + 1])); ms[i] = t; }
    return FTKX_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  return rc;
}

// the ring's arrays go back to the pool and the filter is as it was constructed (also from ftkx_set_mesh, in front of the pool's clear())
static void temporal_release(ftkx_ctx *c)
{
  for (ftkx_block &b : c->tm_ring) give_pooled(c, std::move(b));
  c->tm_ring.clear();
  c->tm.restart();
}

int ftkx_set_temporal_smoothing(ftkx_ctx *c, double sigma, int ksize, int t0)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "ftkx_set_temporal_smoothing: sweeps pending, collect first");
  if (c->sr_open && !c->sr_internal) return fail(c, FTKX_E_INVALID, "ftkx_set_temporal_smoothing: series passes open (ftkx_sweep_series_submit), complete them first");
  double w[ftkx::kTemporalMaxK] = {0};
  if (ksize != 0) {
    if (int rc = ftkx_gaussian_kernel1d(sigma, ksize, w)) { c->err = g_last_error; return rc; }
    if (t0 < 0) return fail(c, FTKX_E_INVALID, "ftkx_set_temporal_smoothing: negative first timestep");
  }
  (void)hipSetDevice(c->device);
  temporal_release(c);
  c->tm.ksize = ksize;
  c->tm_sigma = ksize ? sigma : 0;
  for (int i = 0; i < ftkx::kTemporalMaxK; i ++) c->tm_w[i] = w[i];
  c->tm_next = ksize ? t0 : 0;
  return FTKX_OK;
}

// One emission, as a transaction: it becomes the resident slice tm_next (a slice of that timestep which was resident leaves only once the
// emission has been queued).  `next`: the filter's state behind it; `pop`, idx[]: the state machine's answers; `slot`: the snapshot that joins
// the ring (null: a flush).  The taps are read off a view of the ring as it will be; the kernel writes into the array that leaves the ring
// (the emissions that read it are in front of this one in the stream) or, where none leaves, into a pooled one.  Blocks move only once the
// kernel has been queued: after a failure ring, filter and resident slices are as before the call, and what was taken is freed, not pooled.
static int temporal_emit(ftkx_ctx *c, const ftkx::TemporalSeries &next, bool pop, const int *idx, size_t count, ftkx_block *slot, bool scalar, int *t_emitted)
{
  const double *ring[ftkx::kTemporalMaxK + 1], *arrays[ftkx::kTemporalMaxK];
  size_t n = 0;
  for (size_t i = pop ? 1 : 0; i < c->tm_ring.size() && n < (size_t)ftkx::kTemporalMaxK; i ++) ring[n ++] = c->tm_ring[i].as<double>();
  if (slot) ring[n ++] = slot->as<double>();
  for (int i = 0; i < c->tm.ksize; i ++) arrays[i] = ring[(size_t)idx[i]];
  ftkx_block spare;
  auto queue = [&]() -> int {
    if (!pop) { if (int rc = take_pooled(c, count, spare)) return rc; }
    ftkx::launch_temporal(arrays, c->tm.ksize, c->tm_w, count, pop ? c->tm_ring.front().as<double>() : spare.as<double>(), c->stream);
    HIP_TRY(c, hipGetLastError());
    return FTKX_OK;
  };
  if (int rc = queue()) { (void)hipStreamSynchronize(c->stream); return rc; }
  Slice s;
  ftkx_block &out = scalar ? s.S : s.V;
  if (pop) { out = std::move(c->tm_ring.front()); c->tm_ring.pop_front(); } else out = std::move(spare);
  if (slot) c->tm_ring.push_back(std::move(*slot));
  c->tm = next;
  evict_slice(c, c->tm_next);
  install_slice(c, c->tm_next, s, scalar);
  *t_emitted = c->tm_next ++;
  return FTKX_OK;
}

// T: the element type of the caller's snapshot (double, or float: ftkx_temporal_push_f32); the ring holds FP64 arrays either way.
// planes (ftkx_temporal_push_planar*; A is null then): a vector snapshot as nc arrays, one per component
extern "C++" {
template <class T> static int temporal_push_common(ftkx_ctx *c, const T *A, int is_vector, int on_device, int *t_emitted, const T *const *planes = nullptr, int nc = 0)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!t_emitted) return fail(c, FTKX_E_INVALID, "ftkx_temporal_push: null argument");
  *t_emitted = -1;
  switch (ftkx::temporal_admit(c->tm, is_vector)) {
  case ftkx::TEMPORAL_ADMIT_OFF: return fail(c, FTKX_E_INVALID, "ftkx_temporal_push: call ftkx_set_temporal_smoothing first");
  case ftkx::TEMPORAL_ADMIT_FINISHING: return fail(c, FTKX_E_INVALID, "ftkx_temporal_push: the series is being finished (ftkx_temporal_flush until it says -1)");
  case ftkx::TEMPORAL_ADMIT_MIXED: return fail(c, FTKX_E_INVALID, "ftkx_temporal_push: scalar and vector snapshots cannot be mixed in one series");
  default: break;
  }
  const bool scalar = !is_vector;
  if (int rc = push_checks(c, c->tm_next, on_device, scalar, A != nullptr || planes != nullptr)) return rc;
  if (planes) {
    if (nc != c->nd) return fail(c, FTKX_E_INVALID, "ftkx_temporal_push: %d planes for a context of %d dimensions", nc, c->nd);
    if (int rc = planar_args<T>(c, "ftkx_temporal_push", planes, nc, n_vertices(c), nullptr)) return rc;
  }
  if (c->smooth_ksize && !scalar) return fail(c, FTKX_E_UNSUPPORTED, "ftkx_temporal_push: spatial smoothing is set and takes scalar snapshots only");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t count = n_vertices(c) * (scalar ? 1 : (size_t)c->nd);
  if (!c->tm_ring.empty() && c->tm_ring.front().count<double>() != count) return fail(c, FTKX_E_INVALID, "ftkx_temporal_push: the mesh changed within a series");
  // the raw snapshot (spatially smoothed first where that is set: the stream's order) into a ring slot of the context's own
  if (on_device != 0 && !c->tm_read) HIP_TRY(c, hipEventCreateWithFlags(&c->tm_read, hipEventDisableTiming));
  ftkx_block slot;      // (what it holds after a failure is unknown: freed with this call, not pooled)
  if (int rc = take_pooled(c, count, slot)) return rc;
  // widened where it is float32, convolved where smoothing is set, perturbed and clamped where those are set -- as raw snapshot number t0 + the
  // pushes of this series so far, which is the timestep of the emission centred on it
  if (c->tm.kind < 0 && c->tm.size == 0) { c->tm_t0 = c->tm_next; c->tm_pushed = 0; }      // the series' first snapshot
  const int t_raw = c->tm_t0 + (int)c->tm_pushed;
  if (int rc = planes ? concat_into<T>(c, planes, nc, n_vertices(c), on_device, slot.as<double>(), t_raw)
                      : stage_into(c, A, count, on_device, c->smooth_ksize != 0, slot.as<double>(), t_raw)) return rc;
  // A device source has to be read before the caller may overwrite it (a host source has been staged completely by upload_from_host):
  // the call ends by waiting for THIS point of the stream, not for the stream -- sweeps queued before the push (deferred collection) and
  // the emission queued behind it run on.
  if (on_device != 0 && hipEventRecord(c->tm_read, c->stream) != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(c, FTKX_E_DEVICE, "ftkx_temporal_push: hipEventRecord failed"); }
  // the state machine on a copy; the context's is replaced when everything has been queued
  ftkx::TemporalSeries next = c->tm;
  bool pop = false;
  int idx[ftkx::kTemporalMaxK];
  if (ftkx::temporal_push(next, is_vector, &pop, idx)) {
    if (int rc = temporal_emit(c, next, pop, idx, count, &slot, scalar, t_emitted)) return rc;
  } else {
    if (pop) { give_pooled(c, std::move(c->tm_ring.front())); c->tm_ring.pop_front(); }
    c->tm_ring.push_back(std::move(slot));
    c->tm = next;
  }
  c->tm_pushed ++;
  if (on_device != 0) HIP_TRY(c, hipEventSynchronize(c->tm_read));
  return FTKX_OK;
}

}  // extern "C++"

int ftkx_temporal_push(ftkx_ctx *c, const double *A, int is_vector, int on_device, int *t_emitted)
{ return temporal_push_common<double>(c, A, is_vector, on_device, t_emitted); }
int ftkx_temporal_push_f32(ftkx_ctx *c, const float *A, int is_vector, int on_device, int *t_emitted)
{ return temporal_push_common<float>(c, A, is_vector, on_device, t_emitted); }

int ftkx_temporal_push_planar(ftkx_ctx *c, const double *const *Vc, int nc, int on_device, int *t_emitted)
{ return temporal_push_common<double>(c, nullptr, 1, on_device, t_emitted, Vc, nc); }
int ftkx_temporal_push_planar_f32(ftkx_ctx *c, const float *const *Vc, int nc, int on_device, int *t_emitted)
{ return temporal_push_common<float>(c, nullptr, 1, on_device, t_emitted, Vc, nc); }

int ftkx_temporal_flush(ftkx_ctx *c, int *t_emitted)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!t_emitted) return fail(c, FTKX_E_INVALID, "ftkx_temporal_flush: null argument");
  *t_emitted = -1;
  if (!c->tm.ksize) return fail(c, FTKX_E_INVALID, "ftkx_temporal_flush: call ftkx_set_temporal_smoothing first");
  if (!c->pending.empty()) return fail(c, FTKX_E_INVALID, "ftkx_temporal_flush: sweeps pending, collect first");
  HIP_TRY(c, hipSetDevice(c->device));
  ftkx::TemporalSeries next = c->tm;
  bool pop = false;
  int idx[ftkx::kTemporalMaxK];
  if (!ftkx::temporal_finish_step(next, &pop, idx)) { temporal_release(c); return FTKX_OK; }      // the loop stops: the filter as it was constructed, tm_next the next unused timestep
  // the array that leaves the ring takes the emission
  return temporal_emit(c, next, pop, idx, c->tm_ring.front().count<double>(), nullptr, c->tm.kind == 0, t_emitted);
}

}  // extern "C"
