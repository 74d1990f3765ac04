// How a caller's array becomes a resident FP64 array of the context: ONE pure function from the case to the steps, free of the device.
// ingest.hip executes the plan (every push, the temporal ring, the aux arrays); tests/test_ingest_plan_host.py walks every case without a
// GPU through tests/hostcheck/ingest_plan.cpp, and tests/test_gpu_ingest_paths.py holds the executor's counters to it.
//
// The case: the source's element type (f32: float, else double), its form (planar: one array per component, else one interleaved array),
// whether the spatial smoothing applies (smooth), whether perturbation or clamp applies (adjust: false for a raw array -- an aux array),
// where the caller says it lies (on_device 0 host, 1 this device and borrowable, 2 device memory of any device) and whether every source
// pointer IS device memory of the context's device (on_this_device).  planar && smooth is never asked of ingest_plan: `smooth` is the SCALAR
// smoothing, which takes no vectors.  A vector snapshot under ftkx_set_vector_smoothing has a plan of its own, vec_smooth_ingest_plan below
// (tests/test_vec_smooth_plan_host.py).
// Sources narrower than a float have a plan of their own, narrow_ingest_plan below (tests/test_narrow_plan_host.py).
#pragma once

namespace ftkx {

enum IngestStage { INGEST_STAGE_NONE = 0, INGEST_STAGE_F32, INGEST_STAGE_POOLED };       // the context's f32_stage block / a pooled field array
enum IngestCopy { INGEST_COPY_NONE = 0, INGEST_COPY_TO_DST, INGEST_COPY_TO_STAGE };      // where the source is copied to
// the first kernel of the chain: it writes dst.  INGEST_ADJUST is adjust_kernel<T> on the source's own type (float: in place of the widen kernel)
enum IngestKernel { INGEST_NO_KERNEL = 0, INGEST_CONCAT, INGEST_CONV, INGEST_ADJUST, INGEST_WIDEN, INGEST_CONV_VEC };
// which of the context's debug counters the chain moves, as bits (planar: planar_vec or planar_scalar, by what launch_concat returns)
enum IngestCounter { INGEST_CNT_FROM_FLOAT = 1, INGEST_CNT_IN_PLACE = 2, INGEST_CNT_OUT_OF_PLACE = 4, INGEST_CNT_F32_WIDENED = 8, INGEST_CNT_F32_DIRECT = 16, INGEST_CNT_PLANAR = 32,
                     INGEST_CNT_VEC_INTERLEAVED = 64, INGEST_CNT_VEC_PLANAR = 128, INGEST_CNT_VEC_F32 = 256 };      // ftkx_debug_conv_vec_counts

struct IngestPlan {
  bool reads_here;        // a kernel may read the caller's pointers where they lie
  bool adopt;             // the array is lent to the context as it is: nothing is taken, nothing is queued
  bool caller_waits;      // the call returns only once the source has been read (a host source has been staged completely by the upload)
  IngestStage stage;
  IngestCopy copy;
  IngestKernel first;     // reads the stage where there is one, dst after a copy into dst, the caller's pointers otherwise
  bool then_adjust;       // adjust_kernel<double> in place on dst behind the first kernel (or behind the copy): the LAST kernel of the chain
  unsigned counters;
};

// Whether the plan depends on on_this_device at all: where it does not, the executor does not ask the runtime where the pointers lie.
inline bool ingest_asks_where(bool f32, bool planar, bool smooth, bool adjust, int on_device)
{
  return (planar ? on_device == 1 : on_device != 0) && (f32 || planar || smooth || adjust);
}

// must_own: the caller keeps the array for itself (the temporal ring owns its slots) and never adopts.
inline IngestPlan ingest_plan(bool f32, bool planar, bool smooth, bool adjust, int on_device, bool on_this_device, bool must_own = false)
{
  IngestPlan p{false, false, false, INGEST_STAGE_NONE, INGEST_COPY_NONE, INGEST_NO_KERNEL, false, 0u};
  // THE TWO DIFFER: planes handed over as "device memory of any device" (2) are always staged, an interleaved array of 2 that lies on this
  // device is read where it lies.  Kept as it was found; making planes read in place is a change of behaviour and speed of its own.
  p.reads_here = (planar ? on_device == 1 : on_device != 0) && on_this_device;
  p.adopt = !must_own && !f32 && !planar && on_device == 1 && !smooth && !adjust;      // (the pointer is not examined)
  p.caller_waits = on_device != 0 && !p.adopt;
  if (p.adopt) return p;
  if (!f32 && !planar && !smooth) {
    // FP64, interleaved, no smoothing: no staging array.  Brought straight into dst (and adjusted there), or -- on this device, with
    // something to compute -- read where it lies and written adjusted into dst
    if (adjust && p.reads_here) { p.first = INGEST_ADJUST; p.counters = INGEST_CNT_OUT_OF_PLACE; }
    else { p.copy = INGEST_COPY_TO_DST; p.then_adjust = adjust; p.counters = adjust ? INGEST_CNT_IN_PLACE : 0u; }
    return p;
  }
  // everything a kernel reads: it reads this device's memory only
  if (!p.reads_here) { p.stage = f32 ? INGEST_STAGE_F32 : INGEST_STAGE_POOLED; p.copy = INGEST_COPY_TO_STAGE; }
  p.first = planar ? INGEST_CONCAT : smooth ? INGEST_CONV : adjust ? INGEST_ADJUST : INGEST_WIDEN;      // (the last two: float by elimination)
  p.then_adjust = adjust && p.first != INGEST_ADJUST;
  p.counters = p.first == INGEST_CONCAT ? INGEST_CNT_PLANAR : p.first == INGEST_CONV ? (f32 ? INGEST_CNT_F32_DIRECT : 0u)
             : p.first == INGEST_ADJUST ? INGEST_CNT_FROM_FLOAT : INGEST_CNT_F32_WIDENED;
  if (p.then_adjust) p.counters |= INGEST_CNT_IN_PLACE;
  return p;
}

// ---- vector snapshots under ftkx_set_vector_smoothing (conv_vec_steps.hpp) ------------------------------------------------------------------
// The case: f32, planar, adjust, on_device and on_this_device as above; `smooth` is not asked (the scalar smoothing passes vectors by).  ONE
// kernel, conv_vec_kernel, reads the source -- an interleaved array or planes, floats widened as they are staged -- and writes the smoothed,
// interleaved FP64 array into dst: no concat launch for planes, no widened copy for floats; adjust_kernel<double> follows in place.  The
// kernel reads this device's memory only, so where the source lies and how it is staged is what ingest_plan says for a smoothed scalar or
// for planes: a pooled array (FP64) or the f32_stage block (floats).  Never adopted, and a device source has been read when the call returns.
inline bool vec_smooth_asks_where(bool planar, int on_device) { return planar ? on_device == 1 : on_device != 0; }

inline IngestPlan vec_smooth_ingest_plan(bool f32, bool planar, bool adjust, int on_device, bool on_this_device)
{
  IngestPlan p{false, false, false, INGEST_STAGE_NONE, INGEST_COPY_NONE, INGEST_CONV_VEC, adjust, 0u};
  p.reads_here = vec_smooth_asks_where(planar, on_device) && on_this_device;
  p.caller_waits = on_device != 0;
  if (!p.reads_here) { p.stage = f32 ? INGEST_STAGE_F32 : INGEST_STAGE_POOLED; p.copy = INGEST_COPY_TO_STAGE; }
  p.counters = (planar ? INGEST_CNT_VEC_PLANAR : INGEST_CNT_VEC_INTERLEAVED) | (f32 ? INGEST_CNT_VEC_F32 : 0u) | (adjust ? INGEST_CNT_IN_PLACE : 0u);
  return p;
}

// ---- narrow sources: half, bfloat16, 8- / 16- / 32-bit integers (narrow_steps.hpp) ----------------------------------------------------------
// They go IN FRONT of the chain above, not into it: the narrow kernel writes the FP64 array, and what follows is what follows an FP64 source
// that was copied into the slice -- conv_kernel<double> (a vector under ftkx_set_vector_smoothing: conv_vec_kernel<double>, and `smooth`
// is that setting) out of a pooled array where smoothing is set, adjust_kernel<double> in place.  Neither
// kernel gets an instantiation per narrow type.  The case: smooth, adjust, on_device and on_this_device as above (always one interleaved
// array; planes of narrow elements are not taken).
struct NarrowIngestPlan {
  bool reads_here;        // the narrow kernel reads the caller's pointer where it lies: on_device 1 and memory of this device, nothing else
  bool staged;            // otherwise the source's bytes (count * the element's size) go into the context's f32_stage block first
  bool adopt;             // never: the resident array is FP64
  bool caller_waits;      // a device source has been read when the call returns (a host source has been staged completely by the upload)
  bool to_pooled;         // the narrow kernel writes a pooled field array, which conv_kernel<double> reads into dst (smoothing); else it writes dst
  bool then_adjust;       // adjust_kernel<double> in place on dst: the LAST kernel of the chain
  unsigned counters;      // INGEST_CNT_IN_PLACE where then_adjust; the float32 and planar counters never move
};

// whether the plan depends on on_this_device at all
inline bool narrow_ingest_asks_where(int on_device) { return on_device == 1; }

inline NarrowIngestPlan narrow_ingest_plan(bool smooth, bool adjust, int on_device, bool on_this_device)
{
  NarrowIngestPlan p{false, false, false, false, false, false, 0u};
  p.reads_here = on_device == 1 && on_this_device;
  p.staged = !p.reads_here;
  p.caller_waits = on_device != 0;
  p.to_pooled = smooth;
  p.then_adjust = adjust;
  p.counters = adjust ? INGEST_CNT_IN_PLACE : 0u;
  return p;
}

}  // namespace ftkx
