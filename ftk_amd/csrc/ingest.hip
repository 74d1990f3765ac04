// Snapshot ingest: how a caller's array becomes a resident FP64 array of the context.  The plan is ingest_steps.hpp's, ONE executor
// (ingest) carries it out, and every entry point that brings data in is here: the slice pushes, the aux arrays, the temporal ring, the
// settings that shape a push (spatial and temporal smoothing, perturbation, clamp) and the bare-kernel calls of the kernels of the chain.
#include <type_traits>
#include "ctx.hpp"
#include "ingest_steps.hpp"
#include "narrow_steps.hpp"
#include "relaunch.hpp"

using namespace ftkxh;

constexpr size_t kSmoothWeights = 729;      // ftkx_ctx::d_conv_w: where the smoothing's weights start
constexpr size_t kVecSmoothWeights = 2 * kSmoothWeights;      // ... and the vector smoothing's
static_assert(ftkx::NARROW_F64 == FTKX_DTYPE_F64 && ftkx::NARROW_F32 == FTKX_DTYPE_F32 && ftkx::NARROW_F16 == FTKX_DTYPE_F16 && ftkx::NARROW_BF16 == FTKX_DTYPE_BF16 &&
              ftkx::NARROW_U8 == FTKX_DTYPE_U8 && ftkx::NARROW_I8 == FTKX_DTYPE_I8 && ftkx::NARROW_U16 == FTKX_DTYPE_U16 && ftkx::NARROW_I16 == FTKX_DTYPE_I16 &&
              ftkx::NARROW_U32 == FTKX_DTYPE_U32 && ftkx::NARROW_I32 == FTKX_DTYPE_I32 && ftkx::NARROW_DTYPES == 10, "narrow_steps.hpp and ftkx.h number the element types alike");

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

// ---- the executor -----------------------------------------------------------------------------------------------------------------------
template <class T> static void queue_adjust(ftkx_ctx *c, const T *from, size_t count, int t, double *dst)
{
  const ftkx::AdjustArgs a{c->adj.sigma, c->adj.seed, t, c->adj.lo, c->adj.hi};
  ftkx::launch_adjust<T>(from, count, c->adj.perturb, c->adj.clamp, a, dst, c->stream);
  if (std::is_same<T, float>::value) c->adj_from_float ++;
  else if ((const void *)from == (const void *)dst) c->adj_in_place ++;
  else c->adj_out_of_place ++;
}

template <class T> static void queue_concat(ftkx_ctx *c, const T *const *planes, int nc, size_t count, double *dst)
{
  if (ftkx::launch_concat<T>(planes, nc, count, dst, c->stream)) c->planar_vec ++; else c->planar_scalar ++;
}

// one array of a push, beyond its pointers: where the caller says it lies, the snapshot's number (the noise's), and the case for the plan
struct Ingest {
  int on_device, t;
  bool smooth;        // the spatial smoothing applies to this array
  bool adjust;        // perturbation or clamp applies (false for a raw array: an aux array is no snapshot of the stream's)
  bool must_own;      // never adopted (the temporal ring's slots)
  bool vec_smooth;    // a vector snapshot under ftkx_set_vector_smoothing: every component smoothed as the scalar field it is (`smooth` is false)
};

// the vector smoothing's kernel over the context's mesh, counted by the source's form (ftkx_debug_conv_vec_counts)
template <class T> static void queue_conv_vec(ftkx_ctx *c, const ftkx::ConvVecSource<T> &src, bool planar, double *dst)
{
  ftkx::launch_conv_vec<T>(c->nd, src, (int)c->ext_sz[0], (int)c->ext_sz[1], (int)c->ext_sz[2], c->d_conv_w.as<double>() + kVecSmoothWeights, c->vsmooth_ksize, dst, c->stream);
  if (planar) c->conv_vec_planar ++; else c->conv_vec_interleaved ++;
  if (std::is_same<T, float>::value) c->conv_vec_f32 ++;
}

// dst becomes the snapshot `planes` as a resident slice holds it: nc == 1: one (interleaved) array of n elements; nc 2 or 3: a vector
// snapshot as one array per component, n elements each, which dst holds as the host-interleaved array of them.  An FP64 array on this
// device from which nothing has to be computed is adopted as it is (on_device 1): dst borrows it.  Everything else becomes a pooled array of
// the context's own, n * nc doubles: widened where T is float, convolved where `smooth` says so.  T = double without smoothing is a plain
// copy into dst.  Otherwise ONE kernel on the context's stream reads the source and writes dst (float + smoothing: the convolution stages
// the floats as doubles itself, no widened copy is written and read back; planes: the concat kernel, widening where T is float).  That
// kernel reads this device's memory only: a host source, and a device source that lives on another device, goes through a staging buffer
// first -- FP64: a pooled array (planes back to back in ONE array of n * nc doubles), which goes back to the pool at once; float32: the
// context's f32_stage block (planes at a pitch rounded up to 16 bytes).  Planes are read where they lie only for on_device 1.
//
// The staging block is written by every float32 push and read by the kernel of the push before, which may still run.  What orders them:
// upload_from_host either copies on the context's stream itself, or -- staged_upload, on DMA streams of its own -- makes those streams wait
// for an event recorded on the context's stream unless that stream is idle (upload.cpp, E.gate); a peer copy is queued on the context's
// stream; a block that has to grow is freed only after the stream of its last reader has been waited for (reserve's drain).  All of that
// holds for ONE stream: where ftkx_set_stream has changed it since the last reader was queued, that reader's stream is waited for here.
//
// Perturbation and clamp (ftkx_set_perturbation, ftkx_set_clamp), where either is on: `how.t` is the snapshot's number, and the adjust kernel
// (adjust_kernels.hip) is the LAST kernel of the chain -- the stream's order, widen -> conv -> perturb -> clamp, and concat -> perturb ->
// clamp (the noise's index is the flat index of the interleaved array).  Without smoothing it is the only kernel of an interleaved array: a
// float source goes through adjust_kernel<float> in place of the widen kernel; a host FP64 source (and one on another device) is brought
// straight into dst and adjusted in place, no staging array; an FP64 source on this device is read where it lies and written adjusted into
// dst.  With smoothing, and behind the concat kernel, adjust_kernel<double> runs in place on the output.  With both settings off nothing
// here is queued that was not queued before there were such settings.
//
// A vector snapshot under ftkx_set_vector_smoothing (how.vec_smooth; vec_smooth_ingest_plan): staged like any other source, then ONE kernel,
// conv_vec_kernel, reads the interleaved array (nc == 1: n counts its elements, nd per vertex) or the planes and writes the smoothed
// interleaved array -- no concat launch, no widened copy -- and adjust_kernel<double> follows in place.
//
// *waits is set where the call has to wait for the context's stream before it returns (IngestPlan::caller_waits).  After a failure dst is
// the caller's to let go: freed, not pooled.
template <class T> static int ingest(ftkx_ctx *c, const T *const *planes, int nc, size_t n, const Ingest &how, ftkx_block &dst, bool *waits)
{
  constexpr bool f32 = std::is_same<T, float>::value;
  const bool planar = nc > 1;
  bool on_this_device = how.vec_smooth ? ftkx::vec_smooth_asks_where(planar, how.on_device) : ftkx::ingest_asks_where(f32, planar, how.smooth, how.adjust, how.on_device);
  for (int k = 0; on_this_device && k < nc; k ++) on_this_device = ftkx_pointer_device(planes[k]) == c->device;
  const ftkx::IngestPlan p = how.vec_smooth ? ftkx::vec_smooth_ingest_plan(f32, planar, how.adjust, how.on_device, on_this_device)
                                            : ftkx::ingest_plan(f32, planar, how.smooth, how.adjust, how.on_device, on_this_device, how.must_own);
  if (p.caller_waits) *waits = true;
  const size_t count = n * (size_t)nc;
  if (p.adopt) { dst = ftkx_block::lent(const_cast<T *>(planes[0]), count * sizeof(double)); return FTKX_OK; }
  if (int rc = take_pooled(c, count, dst)) return rc;
  double *const out = dst.as<double>();
  // 0: host memory; otherwise device memory of ANY device (a multi-device tracker hands one snapshot to two contexts)
  auto copy = [&](void *to, int k, size_t bytes) -> int {
    if (how.on_device == 0) return upload_from_host(c, to, planes[k], bytes);
    if (hipMemcpyAsync(to, planes[k], bytes, hipMemcpyDefault, c->stream) == hipSuccess) return FTKX_OK;
    return planar ? fail(c, FTKX_E_DEVICE, "push: copy of plane %d failed", k) : fail(c, FTKX_E_DEVICE, "push: copy of the source failed");
  };
  const T *from[3] = {planes[0], nc > 1 ? planes[1] : nullptr, nc > 2 ? planes[2] : nullptr};
  ftkx_block tmp;
  if (p.copy == ftkx::INGEST_COPY_TO_DST) {
    if (int rc = copy(out, 0, count * sizeof(T))) return rc;
    from[0] = reinterpret_cast<const T *>(out);
  } else if (p.copy == ftkx::INGEST_COPY_TO_STAGE) {
    const size_t bytes = n * sizeof(T), pitch = f32 && planar ? (bytes + 15) & ~(size_t)15 : bytes;
    char *stage = nullptr;
    if (p.stage == ftkx::INGEST_STAGE_F32) {
      if (c->f32_stage_reader && c->f32_stage_reader != c->stream) HIP_TRY(c, hipStreamSynchronize(c->f32_stage_reader));
      c->f32_stage_reader = nullptr;
      if (int rc = c->f32_stage.reserve(c, pitch * (size_t)nc, 0, c->stream)) return rc;
      stage = static_cast<char *>(c->f32_stage.p);
    } else {
      if (int rc = take_pooled(c, count, tmp)) return rc;
      stage = static_cast<char *>(tmp.p);
    }
    // (a failed copy: nothing of it is in flight any more -- upload.cpp drains its DMA streams before it reports an error, and a
    // hipMemcpyAsync that was refused was never queued -- but what the buffer holds is unknown and the device may be in an error state:
    // a pooled buffer is freed with `tmp`, not pooled; the staging block is overwritten by the next push anyway)
    for (int k = 0; k < nc; k ++) {
      if (int rc = copy(stage + (size_t)k * pitch, k, bytes)) return rc;
      from[k] = reinterpret_cast<const T *>(stage + (size_t)k * pitch);
    }
    if (p.stage == ftkx::INGEST_STAGE_F32) c->f32_stage_reader = c->stream;
  }
  if (p.first == ftkx::INGEST_NO_KERNEL && !p.then_adjust) return FTKX_OK;
  switch (p.first) {
  case ftkx::INGEST_CONCAT: queue_concat<T>(c, from, nc, n, out); break;
  case ftkx::INGEST_CONV:
    ftkx::launch_conv<T>(c->nd, from[0], (int)c->ext_sz[0], (int)c->ext_sz[1], (int)c->ext_sz[2], c->d_conv_w.as<double>() + kSmoothWeights, c->smooth_ksize, out, c->stream);
    if (f32) c->f32_direct ++;
    break;
  case ftkx::INGEST_ADJUST: queue_adjust<T>(c, from[0], count, how.t, out); break;
  case ftkx::INGEST_WIDEN: if constexpr (f32) { ftkx::launch_widen(from[0], count, out, c->stream); c->f32_widened ++; } break;
  case ftkx::INGEST_CONV_VEC: queue_conv_vec<T>(c, planar ? ftkx::conv_vec_planes<T>(from, nc) : ftkx::conv_vec_interleaved<T>(from[0], c->nd), planar, out); break;
  case ftkx::INGEST_NO_KERNEL: break;
  }
  if (p.then_adjust) queue_adjust<double>(c, out, count, how.t, out);
  const hipError_t e = hipGetLastError();
  if (tmp.p) give_pooled(c, std::move(tmp));
  HIP_TRY(c, e);
  return FTKX_OK;
}

// ---- narrow sources: half, bfloat16, 8- / 16- / 32-bit integers (narrow_kernels.hip) ----------------------------------------------------------
// dst becomes the FP64 array of the `count` elements of type `dtype` (ftkx::narrow_dtype_ok) at src, by ftkx::narrow_ingest_plan: the narrow
// kernel in FRONT of the chain an FP64 source takes.  It reads this device's memory only: a host source, one handed over as "device memory
// of any device" (2) and a pointer of another device go through the context's f32_stage block as they came, count * the element's size
// bytes, under the ordering said above (ingest).  It writes dst -- or, where smoothing is set, a pooled array that conv_kernel<double> reads
// into dst (a vector under ftkx_set_vector_smoothing: conv_vec_kernel<double>) and that goes back to the pool in stream order;
// adjust_kernel<double> follows in place.  Never adopted.
static int ingest_narrow(ftkx_ctx *c, const void *src, int dtype, size_t count, const Ingest &how, ftkx_block &dst, bool *waits)
{
  const bool on_this_device = ftkx::narrow_ingest_asks_where(how.on_device) && ftkx_pointer_device(src) == c->device;
  const ftkx::NarrowIngestPlan p = ftkx::narrow_ingest_plan(how.smooth || how.vec_smooth, how.adjust, how.on_device, on_this_device);
  if (p.caller_waits) *waits = true;
  if (int rc = take_pooled(c, count, dst)) return rc;
  double *const out = dst.as<double>();
  const void *from = src;
  if (p.staged) {
    const size_t bytes = count * ftkx::narrow_dtype_size(dtype);
    if (c->f32_stage_reader && c->f32_stage_reader != c->stream) HIP_TRY(c, hipStreamSynchronize(c->f32_stage_reader));
    c->f32_stage_reader = nullptr;
    if (int rc = c->f32_stage.reserve(c, bytes, 0, c->stream)) return rc;
    if (how.on_device == 0) { if (int rc = upload_from_host(c, c->f32_stage.p, src, bytes)) return rc; }
    else if (hipMemcpyAsync(c->f32_stage.p, src, bytes, hipMemcpyDefault, c->stream) != hipSuccess) return fail(c, FTKX_E_DEVICE, "push: copy of the source failed");
    from = c->f32_stage.p;
    c->f32_stage_reader = c->stream;
  }
  ftkx_block tmp;
  if (p.to_pooled) { if (int rc = take_pooled(c, count, tmp)) return rc; }
  ftkx::launch_narrow(dtype, from, count, p.to_pooled ? tmp.as<double>() : out, c->stream);
  c->narrow_launches[dtype] ++;
  if (p.to_pooled && how.vec_smooth)
    queue_conv_vec<double>(c, ftkx::conv_vec_interleaved<double>(tmp.as<double>(), c->nd), false, out);
  else if (p.to_pooled)
    ftkx::launch_conv<double>(c->nd, tmp.as<double>(), (int)c->ext_sz[0], (int)c->ext_sz[1], (int)c->ext_sz[2], c->d_conv_w.as<double>() + kSmoothWeights, c->smooth_ksize, out, c->stream);
  if (p.then_adjust) queue_adjust<double>(c, out, count, how.t, out);
  const hipError_t e = hipGetLastError();
  if (tmp.p) give_pooled(c, std::move(tmp));
  HIP_TRY(c, e);
  return FTKX_OK;
}

// one interleaved array by the element type of the push: T double or float -> ingest<T>; T void -> narrow elements of type `dtype`
template <class T> static int ingest_array(ftkx_ctx *c, const T *src, int dtype, size_t count, const Ingest &how, ftkx_block &dst, bool *waits)
{
  if constexpr (std::is_void<T>::value) return ingest_narrow(c, src, dtype, count, how, dst, waits);
  else return ingest<T>(c, &src, 1, count, how, dst, waits);
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

// ---- the slice pushes -------------------------------------------------------------------------------------------------------------------
// T: the element type of the caller's arrays (double, or float: ftkx_push_*_f32; void: narrow elements of type `dtype`, ftkx_push_*_typed,
// never planar).  The resident slice is FP64 either way.
// Vc (ftkx_push_slice_planar*; V is null then): V arrives as nc planes; J and S keep their interleaved layout
template <class T> static int push_common(ftkx_ctx *c, int t, const T *V, const T *J, const T *S, int on_device, bool scalar_only, const T *const *Vc = nullptr, int nc = 0, bool planar = false,
                                          int dtype = -1)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = push_checks(c, t, on_device, scalar_only, scalar_only ? S != nullptr : planar ? Vc != nullptr : V != nullptr)) return rc;
  const size_t n = n_vertices(c);
  const int nd = c->nd;
  if constexpr (!std::is_void<T>::value) if (planar) {
    if (nc != nd) return fail(c, FTKX_E_INVALID, "push: %d planes for a context of %d dimensions", nc, nd);
    if (int rc = planar_args<T>(c, "push", Vc, nc, n, nullptr)) return rc;
  }
  // conv_gaussian dispatches on the array's nd(): a vector field would be convolved across its components (conv.hh:213-221) -- not reproduced
  // (ftkx_set_vector_smoothing is the setting for vectors: every component as the scalar field it is; where it is on it decides)
  const bool vec_smooth = !scalar_only && c->vsmooth_ksize != 0;
  if (c->smooth_ksize && !scalar_only && !vec_smooth) return fail(c, FTKX_E_UNSUPPORTED, "push: spatial smoothing is set and takes scalar slices only (ftkx_push_scalar_slice; vectors: ftkx_set_vector_smoothing)");
  // a given Jacobian, or scalar, does not belong to the smoothed field
  if (vec_smooth && (J || S)) return fail(c, FTKX_E_UNSUPPORTED, "push: vector smoothing is set and takes V alone (no J, no S beside it)");
  // the stream delivers ONE array, which perturb() and clamp() walk over (all n * nd elements of a vector field, by their flat index)
  const bool adjust = c->adj.on();
  if (adjust && !scalar_only && (J || S)) return fail(c, FTKX_E_UNSUPPORTED, "push: perturbation or clamp is set and takes V alone (no J, no S beside it)");
  HIP_TRY(c, hipSetDevice(c->device));
  evict_slice(c, t);
  Slice s;      // (here and below: what was already taken is freed with `s`)
  bool waits = false;
  // one interleaved array of the push (null: none); the scalar smoothing applies to S alone, the vector smoothing to V alone
  auto take = [&](const T *src, size_t count, bool smooth, ftkx_block &dst, bool vsmooth = false) -> int {
    return src ? ingest_array<T>(c, src, dtype, count, Ingest{on_device, t, smooth, adjust, false, vsmooth}, dst, &waits) : FTKX_OK;
  };
  auto take_planes = [&]() -> int {
    if constexpr (std::is_void<T>::value) return fail(c, FTKX_E_INVALID, "push: planes of narrow elements are not taken");
    else return ingest<T>(c, Vc, nc, n, Ingest{on_device, t, false, adjust, false, vec_smooth}, s.V, &waits);
  };
  if (int rc = take(S, n, scalar_only && c->smooth_ksize != 0, s.S)) return rc;
  if (!scalar_only) {
    if (int rc = planar ? take_planes() : take(V, n * nd, false, s.V, vec_smooth)) return rc;
    if (int rc = take(J, n * nd * nd, false, s.J)) return rc;
  }
  // scalar input: V = gradient2D/3D(S) is never materialised -- every kernel evaluates it where it needs it, with the
  // reference's exact operations (ndarray/grad.hh), so the slice costs 8 bytes per vertex of HBM instead of 8 + 8*nd.
  // the source buffers may be reused by the caller on return: a device source that was not adopted -- copied (2), or read by a kernel
  // (smoothing, perturbation or clamp, a float32 source, planes) -- has to be read first; a host source has been staged completely by
  // upload_from_host (nothing to wait for: the DMAs run on while the caller produces its next snapshot)
  if (waits) HIP_TRY(c, hipStreamSynchronize(c->stream));
  install_slice(c, t, s, scalar_only);
  return FTKX_OK;
}

namespace ftkxh {

// The library's own push of an array that IS a resident slice's already (slab.cpp: the upper neighbour's first slice): `full` becomes the
// borrowed resident slice t, scalar or vector by the context's mode, behind the checks of a public on_device 1 push -- and as a raw array,
// whatever smoothing (scalar or vector), perturbation or clamp the context has set: its owner's push has applied them.
int adopt_resident_slice(ftkx_ctx *c, int t, const double *full)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  const bool scalar_only = c->scalar_mode == 1;
  if (int rc = push_checks(c, t, 1, scalar_only, full != nullptr)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  evict_slice(c, t);
  Slice s;
  bool waits = false;
  if (int rc = ingest<double>(c, &full, 1, n_vertices(c) * (scalar_only ? 1 : (size_t)c->nd), Ingest{1, t, false, false, false, false}, scalar_only ? s.S : s.V, &waits)) return rc;
  install_slice(c, t, s, scalar_only);
  return FTKX_OK;
}

// ---- auxiliary scalar fields sampled at critical points (sample_steps.hpp, sample_kernels.hip) -------------------------------------------
// An aux array leaves its timestep (dropped, or replaced by a push).  ftkx_sample_aux has waited for its kernel; the sample kernel of an armed
// series pass (ftkx_set_series_sampling) may still be queued.  The decision is free_slice's (ftkx_api.hip): the newest open pass is a SPLIT
// pass -- its tail, on a stream of its own, is in no order with whatever takes the array out of the pool next -- and the array is parked with
// that pass until it has been completed (release_retired); otherwise it goes to the pool, behind the context's stream.
static void retire_aux(ftkx_ctx *c, ftkx_block &&b)
{
  if (c->sr_open > 0) {
    ftkx_series_pending &N = c->sr_pend[c->sr_place(c->sr_open - 1)];
    if (N.open && N.split) { N.parked_aux.push_back(std::move(b)); return; }
  }
  give_pooled(c, std::move(b));
}

// the aux arrays of timestep t leave
void drop_aux(ftkx_ctx *c, int t)
{
  auto it = c->aux.find(t);
  if (it == c->aux.end()) return;
  for (ftkx_block &b : it->second.A) if (b.p) retire_aux(c, std::move(b));
  c->aux.erase(it);
}

// the ring's arrays go back to the pool and the filter is as it was constructed (also from ftkx_set_mesh, in front of the pool's clear())
void temporal_release(ftkx_ctx *c)
{
  for (ftkx_block &b : c->tm_ring) give_pooled(c, std::move(b));
  c->tm_ring.clear();
  c->tm.restart();
}

}  // namespace ftkxh

template <class T> static int push_aux_common(ftkx_ctx *c, int t, int slot, const T *A, int on_device)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!c->mesh_set) return fail(c, FTKX_E_INVALID, "ftkx_push_aux_slice: call ftkx_set_mesh first");
  if (t < 0) return fail(c, FTKX_E_INVALID, "ftkx_push_aux_slice: negative timestep");
  if (slot != 1 && slot != 2) return fail(c, FTKX_E_INVALID, "ftkx_push_aux_slice: slot must be 1 or 2, not %d (slot 0 is the scalar field of the sweep)", slot);
  if (on_device < 0 || on_device > 2) return fail(c, FTKX_E_INVALID, "ftkx_push_aux_slice: on_device must be 0, 1 or 2");
  if (!A || ((size_t)A & (sizeof(T) - 1))) return fail(c, FTKX_E_INVALID, "ftkx_push_aux_slice: the array is null or not a multiple of its element's size");
  HIP_TRY(c, hipSetDevice(c->device));
  ftkx_block b;      // (after a failure: freed, not pooled)
  bool waits = false;
  // a raw array: perturbation and clamp pass it by, and so does the smoothing
  if (int rc = ingest<T>(c, &A, 1, n_vertices(c), Ingest{on_device, t, false, false, false, false}, b, &waits)) return rc;
  // a device source that was not adopted is read by a copy or by the widen kernel: the call returns once it has been read
  if (waits) HIP_TRY(c, hipStreamSynchronize(c->stream));
  ftkx_block &dst = c->aux[t].A[slot - 1];
  if (dst.p) retire_aux(c, std::move(dst));
  dst = std::move(b);
  return FTKX_OK;
}

// ---- temporal Gaussian smoothing (filters/streaming_filter.hh) ---------------------------------------------------------------------------
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
// (void: narrow elements of type `dtype`, ftkx_temporal_push_typed, never planar: widened into the slot, adjusted there)
// planes (ftkx_temporal_push_planar*; A is null then): a vector snapshot as nc arrays, one per component
template <class T> static int temporal_push_common(ftkx_ctx *c, const T *A, int is_vector, int on_device, int *t_emitted, const T *const *planes = nullptr, int nc = 0, int dtype = -1)
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
  if constexpr (!std::is_void<T>::value) if (planes) {
    if (nc != c->nd) return fail(c, FTKX_E_INVALID, "ftkx_temporal_push: %d planes for a context of %d dimensions", nc, c->nd);
    if (int rc = planar_args<T>(c, "ftkx_temporal_push", planes, nc, n_vertices(c), nullptr)) return rc;
  }
  const bool vec_smooth = !scalar && c->vsmooth_ksize != 0;
  if (c->smooth_ksize && !scalar && !vec_smooth) return fail(c, FTKX_E_UNSUPPORTED, "ftkx_temporal_push: spatial smoothing is set and takes scalar snapshots only (vectors: ftkx_set_vector_smoothing)");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t count = n_vertices(c) * (scalar ? 1 : (size_t)c->nd);
  if (!c->tm_ring.empty() && c->tm_ring.front().count<double>() != count) return fail(c, FTKX_E_INVALID, "ftkx_temporal_push: the mesh changed within a series");
  // the raw snapshot (spatially smoothed first where that is set: the stream's order) into a ring slot of the context's own
  if (on_device != 0 && !c->tm_read) HIP_TRY(c, hipEventCreateWithFlags(&c->tm_read, hipEventDisableTiming));
  ftkx_block slot;      // (what it holds after a failure is unknown: freed with this call, not pooled)
  // widened where it is float32, convolved where smoothing is set, perturbed and clamped where those are set -- as raw snapshot number t0 + the
  // pushes of this series so far, which is the timestep of the emission centred on it
  if (c->tm.kind < 0 && c->tm.size == 0) { c->tm_t0 = c->tm_next; c->tm_pushed = 0; }      // the series' first snapshot
  const Ingest how{on_device, c->tm_t0 + (int)c->tm_pushed, scalar && c->smooth_ksize != 0, c->adj.on(), true, vec_smooth};
  bool waits = false;
  auto take_planes = [&]() -> int {
    if constexpr (std::is_void<T>::value) return fail(c, FTKX_E_INVALID, "ftkx_temporal_push: planes of narrow elements are not taken");
    else return ingest<T>(c, planes, nc, n_vertices(c), how, slot, &waits);
  };
  if (int rc = planes ? take_planes() : ingest_array<T>(c, A, dtype, count, how, slot, &waits)) return rc;
  // A device source has to be read before the caller may overwrite it (a host source has been staged completely by upload_from_host):
  // the call ends by waiting for THIS point of the stream, not for the stream -- sweeps queued before the push (deferred collection) and
  // the emission queued behind it run on.
  if (waits && hipEventRecord(c->tm_read, c->stream) != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(c, FTKX_E_DEVICE, "ftkx_temporal_push: hipEventRecord failed"); }
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
  if (waits) HIP_TRY(c, hipEventSynchronize(c->tm_read));
  return FTKX_OK;
}

// ---- the kernels of the chain on their own: argument checks, one launch or a timed row of them (relaunch.hpp) -----------------------------
static bool conv_ksize_ok(int ksize) { return ksize >= 1 && ksize <= 9 && (ksize & 1) == 1; }

static int conv_weights(ftkx_ctx *c, const double *weights, int n, size_t at)
{
  if (const int rc = c->d_conv_w.reserve(c, 3 * kSmoothWeights * sizeof(double))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_conv_w.as<double>() + at, weights, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return FTKX_OK;
}

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

// The vector convolution alone on device pointers: V (interleaved, nd components) or, where V is null, nd planes; `reps` times back to back,
// ms (nullable: reps == 1) the time of every launch.  Argument errors as conv_common's; every source array must stay clear of `out`.
template <class T> static int conv_vec_common(ftkx_ctx *c, const char *who, int nd, const T *V, const T *const *planes, int DW, int DH, int DD, const double *weights, int ksize, double *out,
                                              int reps, double *ms)
{
  DERIVE_PROLOGUE(c);
  if (nd != 2 && nd != 3) return fail(c, FTKX_E_INVALID, "%s: nd must be 2 or 3", who);
  if ((!V && !planes) || !out || !weights || (ms ? reps < 1 : reps != 1)) return fail(c, FTKX_E_INVALID, "%s: null argument", who);
  if (nd == 2) DD = 1;
  if (DW < 1 || DH < 1 || DD < 1) return fail(c, FTKX_E_INVALID, "%s: extents must be positive", who);
  if (!conv_ksize_ok(ksize)) return fail(c, FTKX_E_INVALID, "%s: ksize must be odd and in [1, 9] (got %d)", who, ksize);
  const size_t n = (size_t)DW * (size_t)DH * (size_t)DD;
  if ((size_t)out & 7) return fail(c, FTKX_E_INVALID, "%s: out must be a multiple of 8", who);
  for (int k = 0; k < (V ? 1 : nd); k ++) {
    const T *a = V ? V : planes[k];
    const size_t count = V ? n * (size_t)nd : n;
    if (!a) return fail(c, FTKX_E_INVALID, "%s: plane %d is null", who, k);
    if ((size_t)a & (sizeof(T) - 1)) return fail(c, FTKX_E_INVALID, "%s: an input is not a multiple of its element's size", who);
    if ((const char *)a < (const char *)(out + n * (size_t)nd) && (const char *)out < (const char *)(a + count)) return fail(c, FTKX_E_INVALID, "%s: input and output overlap", who);
  }
  if (int rc = conv_weights(c, weights, ksize * ksize * (nd == 3 ? ksize : 1), 0)) return rc;
  const ftkx::ConvVecSource<T> src = V ? ftkx::conv_vec_interleaved<T>(V, nd) : ftkx::conv_vec_planes<T>(planes, nd);
  // (the stream is waited for: the next call may overwrite the weights; the caller may read `out`)
  return timed_relaunch(c, reps, ms, [&] { ftkx::launch_conv_vec<T>(nd, src, DW, DH, DD, c->d_conv_w.as<double>(), ksize, out, c->stream); });
}

static int widen_args(ftkx_ctx *c, const char *who, const float *src, size_t count, const double *dst)
{
  if (!src || !dst) return fail(c, FTKX_E_INVALID, "%s: null argument", who);
  if (count < 1) return fail(c, FTKX_E_INVALID, "%s: count must be positive", who);
  if (((size_t)src & 3) || ((size_t)dst & 7)) return fail(c, FTKX_E_INVALID, "%s: src must be a multiple of 4 bytes and dst a multiple of 8", who);
  if ((const char *)src < (const char *)(dst + count) && (const char *)dst < (const char *)(src + count)) return fail(c, FTKX_E_INVALID, "%s: input and output overlap", who);
  return FTKX_OK;
}

// the concat kernel alone on device pointers, `reps` times back to back; ms (nullable: reps == 1): the time of every launch
template <class T> static int concat_common(ftkx_ctx *c, const char *who, const T *const *planes, int nc, size_t count, double *dst, int reps, double *ms)
{
  DERIVE_PROLOGUE(c);
  if (!dst || (ms ? reps < 1 : reps != 1)) return fail(c, FTKX_E_INVALID, "%s: bad argument", who);
  if (int rc = planar_args<T>(c, who, planes, nc, count, dst)) return rc;
  return timed_relaunch(c, reps, ms, [&] { queue_concat<T>(c, planes, nc, count, dst); });
}

static int adjust_settings(ftkx_ctx *c, const char *who, double sigma, int clamp_on, double lo, double hi, bool need_one)
{
  if (!std::isfinite(sigma) || sigma < 0) return fail(c, FTKX_E_INVALID, "%s: sigma must be finite and not negative", who);
  if (clamp_on && (std::isnan(lo) || std::isnan(hi))) return fail(c, FTKX_E_INVALID, "%s: a clamp bound is NaN", who);
  if (need_one && sigma == 0 && !clamp_on) return fail(c, FTKX_E_INVALID, "%s: neither perturbation (sigma > 0) nor clamp asked for", who);
  return FTKX_OK;
}

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
  return timed_relaunch(c, reps, ms, [&] { ftkx::launch_adjust<T>(src, count, sigma > 0, clamp_on != 0, a, dst, c->stream); });
}

// the bare narrow kernel's arguments: a dtype it has (float32 is handed to the widen kernel by the callers; FP64 has no kernel: a copy is
// not a conversion), the rest as widen_args
static int narrow_args(ftkx_ctx *c, const char *who, const void *src, int dtype, size_t count, const double *dst)
{
  if (!ftkx::narrow_dtype_ok(dtype)) return fail(c, FTKX_E_INVALID, "%s: dtype %d is not one of FTKX_DTYPE_F16 .. FTKX_DTYPE_I32", who, dtype);
  const size_t esize = ftkx::narrow_dtype_size(dtype);
  if (!src || !dst) return fail(c, FTKX_E_INVALID, "%s: null argument", who);
  if (count < 1) return fail(c, FTKX_E_INVALID, "%s: count must be positive", who);
  if (((size_t)src & (esize - 1)) || ((size_t)dst & 7)) return fail(c, FTKX_E_INVALID, "%s: src must be a multiple of its element's size and dst a multiple of 8", who);
  if ((const char *)src < (const char *)(dst + count) && (const char *)dst < (const char *)src + count * esize) return fail(c, FTKX_E_INVALID, "%s: input and output overlap", who);
  return FTKX_OK;
}

// what a typed push asks of its arrays before the checks of its FP64 counterpart: a narrow dtype, every given pointer a multiple of its size.
// Like every push, refused or not, it ends what was announced ahead (c->ahead).
static int typed_args(ftkx_ctx *c, const char *who, int dtype, const void *const *arrays, int n)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!ftkx::narrow_dtype_ok(dtype)) return fail(c, FTKX_E_INVALID, "%s: dtype %d is not one of FTKX_DTYPE_*", who, dtype);
  for (int k = 0; k < n; k ++)
    if ((size_t)arrays[k] & (ftkx::narrow_dtype_size(dtype) - 1)) return fail(c, FTKX_E_INVALID, "%s: an array is not a multiple of its element's size", who);
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

extern "C" {

int ftkx_push_slice(ftkx_ctx *c, int t, const double *V, const double *J, const double *S, int on_device)
{ return push_common<double>(c, t, V, J, S, on_device, false); }

int ftkx_push_scalar_slice(ftkx_ctx *c, int t, const double *S, int on_device)
{ return push_common<double>(c, t, nullptr, nullptr, S, on_device, true); }

int ftkx_push_slice_f32(ftkx_ctx *c, int t, const float *V, const float *J, const float *S, int on_device)
{ return push_common<float>(c, t, V, J, S, on_device, false); }

int ftkx_push_scalar_slice_f32(ftkx_ctx *c, int t, const float *S, int on_device)
{ return push_common<float>(c, t, nullptr, nullptr, S, on_device, true); }

int ftkx_push_slice_planar(ftkx_ctx *c, int t, const double *const *Vc, int nc, const double *J, const double *S, int on_device)
{ return push_common<double>(c, t, nullptr, J, S, on_device, false, Vc, nc, true); }

int ftkx_push_slice_planar_f32(ftkx_ctx *c, int t, const float *const *Vc, int nc, const float *J, const float *S, int on_device)
{ return push_common<float>(c, t, nullptr, J, S, on_device, false, Vc, nc, true); }

int ftkx_push_aux_slice(ftkx_ctx *c, int t, int slot, const double *A, int on_device) { return push_aux_common<double>(c, t, slot, A, on_device); }
int ftkx_push_aux_slice_f32(ftkx_ctx *c, int t, int slot, const float *A, int on_device) { return push_aux_common<float>(c, t, slot, A, on_device); }

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

int ftkx_debug_adjust_counts(const ftkx_ctx *c, unsigned long long *from_float, unsigned long long *in_place, unsigned long long *out_of_place)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (from_float) *from_float = c->adj_from_float;
  if (in_place) *in_place = c->adj_in_place;
  if (out_of_place) *out_of_place = c->adj_out_of_place;
  return FTKX_OK;
}

// ---- spatial Gaussian smoothing (ndarray/conv.hh) ----------------------------------------------------------------------------------------
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

int ftkx_conv2D(ftkx_ctx *c, const double *S, int DW, int DH, const double *weights, int ksize, double *out)
{ return conv_common<double>(c, 2, S, DW, DH, 1, weights, ksize, out); }
int ftkx_conv3D(ftkx_ctx *c, const double *S, int DW, int DH, int DD, const double *weights, int ksize, double *out)
{ return conv_common<double>(c, 3, S, DW, DH, DD, weights, ksize, out); }
int ftkx_conv2D_f32(ftkx_ctx *c, const float *S, int DW, int DH, const double *weights, int ksize, double *out)
{ return conv_common<float>(c, 2, S, DW, DH, 1, weights, ksize, out); }
int ftkx_conv3D_f32(ftkx_ctx *c, const float *S, int DW, int DH, int DD, const double *weights, int ksize, double *out)
{ return conv_common<float>(c, 3, S, DW, DH, DD, weights, ksize, out); }

// profiling aid (tools/conv_time.py): the convolution kernel `reps` times back to back
int ftkx_debug_conv_relaunch(ftkx_ctx *c, int nd, const double *S, int DW, int DH, int DD, const double *weights, int ksize, double *out, int reps, double *ms)
{
  DERIVE_PROLOGUE(c);
  if ((nd != 2 && nd != 3) || !S || !out || !weights || !ms || reps < 1 || DW < 1 || DH < 1 || DD < 1 || !conv_ksize_ok(ksize)) return fail(c, FTKX_E_INVALID, "ftkx_debug_conv_relaunch: bad argument");
  if (int rc = conv_weights(c, weights, ksize * ksize * (nd == 3 ? ksize : 1), 0)) return rc;
  return timed_relaunch(c, reps, ms, [&] { ftkx::launch_conv(nd, S, DW, DH, nd == 3 ? DD : 1, c->d_conv_w.as<double>(), ksize, out, c->stream); });
}

int ftkx_set_spatial_smoothing(ftkx_ctx *c, double sigma, int ksize)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = settings_not_now(c, "ftkx_set_spatial_smoothing")) return rc;
  if (ksize == 0) { c->smooth_ksize = 0; c->smooth_sigma = 0; return FTKX_OK; }
  double w[kSmoothWeights];
  if (int rc = ftkx_gaussian_kernel(c->nd, sigma, ksize, w)) { c->err = global_error(); return rc; }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (a push queued under the old weights still reads them)
  if (int rc = conv_weights(c, w, ksize * ksize * (c->nd == 3 ? ksize : 1), kSmoothWeights)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (`w` is this call's)
  c->smooth_ksize = ksize; c->smooth_sigma = sigma;
  return FTKX_OK;
}

// ---- spatial smoothing of vector arrays, per component (conv_vec_kernels.hip) ------------------------------------------------------------------
int ftkx_conv2D_vec(ftkx_ctx *c, const double *V, int DW, int DH, const double *weights, int ksize, double *out)
{ return conv_vec_common<double>(c, "ftkx_conv2D_vec", 2, V, nullptr, DW, DH, 1, weights, ksize, out, 1, nullptr); }
int ftkx_conv3D_vec(ftkx_ctx *c, const double *V, int DW, int DH, int DD, const double *weights, int ksize, double *out)
{ return conv_vec_common<double>(c, "ftkx_conv3D_vec", 3, V, nullptr, DW, DH, DD, weights, ksize, out, 1, nullptr); }
int ftkx_conv2D_vec_f32(ftkx_ctx *c, const float *V, int DW, int DH, const double *weights, int ksize, double *out)
{ return conv_vec_common<float>(c, "ftkx_conv2D_vec_f32", 2, V, nullptr, DW, DH, 1, weights, ksize, out, 1, nullptr); }
int ftkx_conv3D_vec_f32(ftkx_ctx *c, const float *V, int DW, int DH, int DD, const double *weights, int ksize, double *out)
{ return conv_vec_common<float>(c, "ftkx_conv3D_vec_f32", 3, V, nullptr, DW, DH, DD, weights, ksize, out, 1, nullptr); }
int ftkx_conv_planar(ftkx_ctx *c, int nd, const double *const *planes, int DW, int DH, int DD, const double *weights, int ksize, double *out)
{ return conv_vec_common<double>(c, "ftkx_conv_planar", nd, nullptr, planes, DW, DH, DD, weights, ksize, out, 1, nullptr); }
int ftkx_conv_planar_f32(ftkx_ctx *c, int nd, const float *const *planes, int DW, int DH, int DD, const double *weights, int ksize, double *out)
{ return conv_vec_common<float>(c, "ftkx_conv_planar_f32", nd, nullptr, planes, DW, DH, DD, weights, ksize, out, 1, nullptr); }

// profiling aid (tools/conv_vec_time.py): the kernel `reps` times back to back
int ftkx_debug_conv_vec_relaunch(ftkx_ctx *c, int nd, const void *const *src, int planar, int src_is_f32, int DW, int DH, int DD, const double *weights, int ksize, double *out, int reps, double *ms)
{
  if (c && (!src || !ms || reps < 1)) return fail(c, FTKX_E_INVALID, "ftkx_debug_conv_vec_relaunch: bad argument");
  if (src_is_f32) return conv_vec_common<float>(c, "ftkx_debug_conv_vec_relaunch", nd, planar || !src ? nullptr : static_cast<const float *>(src[0]), planar ? reinterpret_cast<const float *const *>(src) : nullptr,
                                                DW, DH, DD, weights, ksize, out, reps, ms);
  return conv_vec_common<double>(c, "ftkx_debug_conv_vec_relaunch", nd, planar || !src ? nullptr : static_cast<const double *>(src[0]), planar ? reinterpret_cast<const double *const *>(src) : nullptr,
                                 DW, DH, DD, weights, ksize, out, reps, ms);
}

int ftkx_debug_conv_vec_counts(const ftkx_ctx *c, unsigned long long *interleaved, unsigned long long *planar, unsigned long long *f32)
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (interleaved) *interleaved = c->conv_vec_interleaved;
  if (planar) *planar = c->conv_vec_planar;
  if (f32) *f32 = c->conv_vec_f32;
  return FTKX_OK;
}

int ftkx_set_vector_smoothing(ftkx_ctx *c, double sigma, int ksize)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = settings_not_now(c, "ftkx_set_vector_smoothing")) return rc;
  if (ksize == 0) { c->vsmooth_ksize = 0; c->vsmooth_sigma = 0; return FTKX_OK; }
  double w[kSmoothWeights];
  if (int rc = ftkx_gaussian_kernel(c->nd, sigma, ksize, w)) { c->err = global_error(); return rc; }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (a push queued under the old weights still reads them)
  if (int rc = conv_weights(c, w, ksize * ksize * (c->nd == 3 ? ksize : 1), kVecSmoothWeights)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (`w` is this call's)
  c->vsmooth_ksize = ksize; c->vsmooth_sigma = sigma;
  return FTKX_OK;
}

// ---- float32 -> FP64 (widen_kernels.hip) ---------------------------------------------------------------------------------------------------
int ftkx_widen_f32(ftkx_ctx *c, const float *src, size_t count, double *dst)
{
  DERIVE_PROLOGUE(c);
  if (int rc = widen_args(c, "ftkx_widen_f32", src, count, dst)) return rc;
  ftkx::launch_widen(src, count, dst, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the caller may read `dst`)
  return FTKX_OK;
}

// profiling aid (tools/push_f32_time.py): the widen kernel `reps` times back to back
int ftkx_debug_widen_relaunch(ftkx_ctx *c, const float *src, size_t count, double *dst, int reps, double *ms)
{
  DERIVE_PROLOGUE(c);
  if (!ms || reps < 1) return fail(c, FTKX_E_INVALID, "ftkx_debug_widen_relaunch: bad argument");
  if (int rc = widen_args(c, "ftkx_debug_widen_relaunch", src, count, dst)) return rc;
  return timed_relaunch(c, reps, ms, [&] { ftkx::launch_widen(src, count, dst, c->stream); });
}

// ---- half, bfloat16, integers -> FP64 (narrow_kernels.hip) -----------------------------------------------------------------------------------
size_t ftkx_dtype_size(int dtype) { return ftkx::narrow_dtype_size(dtype); }

int ftkx_push_scalar_slice_typed(ftkx_ctx *c, int t, const void *S, int dtype, int on_device)
{
  if (dtype == FTKX_DTYPE_F64) return ftkx_push_scalar_slice(c, t, static_cast<const double *>(S), on_device);
  if (dtype == FTKX_DTYPE_F32) return ftkx_push_scalar_slice_f32(c, t, static_cast<const float *>(S), on_device);
  const void *a[1] = {S};
  if (int rc = typed_args(c, "ftkx_push_scalar_slice_typed", dtype, a, 1)) return rc;
  return push_common<void>(c, t, nullptr, nullptr, S, on_device, true, nullptr, 0, false, dtype);
}

int ftkx_push_slice_typed(ftkx_ctx *c, int t, const void *V, const void *J, const void *S, int dtype, int on_device)
{
  if (dtype == FTKX_DTYPE_F64) return ftkx_push_slice(c, t, static_cast<const double *>(V), static_cast<const double *>(J), static_cast<const double *>(S), on_device);
  if (dtype == FTKX_DTYPE_F32) return ftkx_push_slice_f32(c, t, static_cast<const float *>(V), static_cast<const float *>(J), static_cast<const float *>(S), on_device);
  const void *a[3] = {V, J, S};
  if (int rc = typed_args(c, "ftkx_push_slice_typed", dtype, a, 3)) return rc;
  return push_common<void>(c, t, V, J, S, on_device, false, nullptr, 0, false, dtype);
}

int ftkx_temporal_push_typed(ftkx_ctx *c, const void *A, int dtype, int is_vector, int on_device, int *t_emitted)
{
  if (dtype == FTKX_DTYPE_F64) return ftkx_temporal_push(c, static_cast<const double *>(A), is_vector, on_device, t_emitted);
  if (dtype == FTKX_DTYPE_F32) return ftkx_temporal_push_f32(c, static_cast<const float *>(A), is_vector, on_device, t_emitted);
  const void *a[1] = {A};
  if (int rc = typed_args(c, "ftkx_temporal_push_typed", dtype, a, 1)) return rc;
  return temporal_push_common<void>(c, A, is_vector, on_device, t_emitted, nullptr, 0, dtype);
}

int ftkx_widen_typed(ftkx_ctx *c, const void *src, int dtype, size_t count, double *dst)
{
  if (dtype == FTKX_DTYPE_F32) return ftkx_widen_f32(c, static_cast<const float *>(src), count, dst);
  DERIVE_PROLOGUE(c);
  if (int rc = narrow_args(c, "ftkx_widen_typed", src, dtype, count, dst)) return rc;
  ftkx::launch_narrow(dtype, src, count, dst, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the caller may read `dst`)
  return FTKX_OK;
}

// profiling aid (tools/push_narrow_time.py): the narrow kernel `reps` times back to back
int ftkx_debug_narrow_relaunch(ftkx_ctx *c, const void *src, int dtype, size_t count, double *dst, int reps, double *ms)
{
  if (dtype == FTKX_DTYPE_F32) return ftkx_debug_widen_relaunch(c, static_cast<const float *>(src), count, dst, reps, ms);
  DERIVE_PROLOGUE(c);
  if (!ms || reps < 1) return fail(c, FTKX_E_INVALID, "ftkx_debug_narrow_relaunch: bad argument");
  if (int rc = narrow_args(c, "ftkx_debug_narrow_relaunch", src, dtype, count, dst)) return rc;
  return timed_relaunch(c, reps, ms, [&] { ftkx::launch_narrow(dtype, src, count, dst, c->stream); });
}

int ftkx_debug_narrow_counts(const ftkx_ctx *c, unsigned long long per_dtype[10])
{
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (!per_dtype) return fail(nullptr, FTKX_E_INVALID, "ftkx_debug_narrow_counts: null argument");
  for (int i = 0; i < 10; i ++) per_dtype[i] = c->narrow_launches[i];
  return FTKX_OK;
}

// ---- component planes -> interleaved FP64 (concat_kernels.hip) ------------------------------------------------------------------------------
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
int ftkx_set_perturbation(ftkx_ctx *c, double sigma, unsigned long long seed)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = settings_not_now(c, "ftkx_set_perturbation")) return rc;
  if (int rc = adjust_settings(c, "ftkx_set_perturbation", sigma, 0, 0, 0, false)) return rc;
  c->adj.perturb = sigma > 0; c->adj.sigma = sigma; c->adj.seed = seed;
  return FTKX_OK;
}

int ftkx_set_clamp(ftkx_ctx *c, int on, double lo, double hi)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = settings_not_now(c, "ftkx_set_clamp")) return rc;
  if (int rc = adjust_settings(c, "ftkx_set_clamp", 0, on, lo, hi, false)) return rc;
  c->adj.clamp = on != 0; c->adj.lo = on ? lo : 0; c->adj.hi = on ? hi : 0;
  return FTKX_OK;
}

int ftkx_adjust(ftkx_ctx *c, const double *src, size_t count, double sigma, unsigned long long seed, int t, int clamp_on, double lo, double hi, double *dst)
{ return adjust_common<double>(c, "ftkx_adjust", src, count, sigma, seed, t, clamp_on, lo, hi, dst, 1, nullptr); }
int ftkx_adjust_f32(ftkx_ctx *c, const float *src, size_t count, double sigma, unsigned long long seed, int t, int clamp_on, double lo, double hi, double *dst)
{ return adjust_common<float>(c, "ftkx_adjust_f32", src, count, sigma, seed, t, clamp_on, lo, hi, dst, 1, nullptr); }

// profiling aid (tools/adjust_time.py): the adjust kernel `reps` times back to back.  In place with sigma > 0 every launch perturbs what the
// one before left: the time is the same, the values are not those of one launch.
int ftkx_debug_adjust_relaunch(ftkx_ctx *c, const void *src, int src_is_f32, size_t count, double sigma, unsigned long long seed, int t, int clamp_on, double lo, double hi,
                               double *dst, int reps, double *ms)
{
  if (c && !ms) return fail(c, FTKX_E_INVALID, "ftkx_debug_adjust_relaunch: bad argument");
  if (src_is_f32) return adjust_common<float>(c, "ftkx_debug_adjust_relaunch", (const float *)src, count, sigma, seed, t, clamp_on, lo, hi, dst, reps, ms);
  return adjust_common<double>(c, "ftkx_debug_adjust_relaunch", (const double *)src, count, sigma, seed, t, clamp_on, lo, hi, dst, reps, ms);
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

int ftkx_temporal_combine(ftkx_ctx *c, const double *const *arrays, int ksize, const double *weights, size_t count, double *out)
{
  DERIVE_PROLOGUE(c);
  if (int rc = temporal_combine_args(c, "ftkx_temporal_combine", arrays, ksize, weights, count, out)) return rc;
  ftkx::launch_temporal(arrays, ksize, weights, count, out, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the caller may read `out`)
  return FTKX_OK;
}

// profiling aid (tools/temporal_time.py): the kernel `reps` times back to back
int ftkx_debug_temporal_relaunch(ftkx_ctx *c, const double *const *arrays, int ksize, const double *weights, size_t count, double *out, int reps, double *ms)
{
  DERIVE_PROLOGUE(c);
  if (!ms || reps < 1) return fail(c, FTKX_E_INVALID, "ftkx_debug_temporal_relaunch: bad argument");
  if (int rc = temporal_combine_args(c, "ftkx_debug_temporal_relaunch", arrays, ksize, weights, count, out)) return rc;
  return timed_relaunch(c, reps, ms, [&] { ftkx::launch_temporal(arrays, ksize, weights, count, out, c->stream); });
}

int ftkx_set_temporal_smoothing(ftkx_ctx *c, double sigma, int ksize, int t0)
{
  if (c) c->ahead.clear();
  if (!c) return fail(nullptr, FTKX_E_INVALID, "null context");
  if (int rc = settings_not_now(c, "ftkx_set_temporal_smoothing")) return rc;
  double w[ftkx::kTemporalMaxK] = {0};
  if (ksize != 0) {
    if (int rc = ftkx_gaussian_kernel1d(sigma, ksize, w)) { c->err = global_error(); return rc; }
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
