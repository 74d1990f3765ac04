// Temporal Gaussian smoothing of a series of snapshots: the state machine that says which snapshots an emission adds up, and what one
// element's sum is, for temporal_kernels.hip and ingest.hip.
//
// Reference (host): include/ftk/filters/streaming_filter.hh, driven by ndarray_stream::modified_callback with
// --temporal-smoothing-kernel[-size] (include/ftk/ndarray/stream.hh); its weights: gaussian_kernel, include/ftk/ndarray/conv.hh:50-72.
// With K the (odd) kernel size, H = (K + 1) / 2 and `data` the deque of raw snapshots:
//     push(a):  data.push_back(a); if |data| > K: data.pop_front(), cursor--
//               if |data| >= H: emit sum_i w[i] * data[max(0, i + cursor - H + 1)], cursor++
//     finish(): loop: data.pop_front(); if |data| >= H: emit sum_i w[i] * data[min(|data| - 1, i)], cursor--; else stop
// Reproduced literally, not as a closed form: a series shorter than K emits fewer arrays than it has snapshots (2 (N - H) + 1 for
// H <= N < K, none below H), because the finishing rule indexes from the front of the shortened deque.
// The sum of one element: the accumulator STARTS as the rounded product w[0] * x0 (the reference's `result` is an empty array that takes
// the first product over), then for i = 1 .. K - 1 one rounded multiply and one rounded add; nothing fused (-ffp-contract=off on both
// sides), and taps that fall on the same snapshot at an edge are not merged: w0 * a + w1 * a, never (w0 + w1) * a.
//
// An emission names up to K snapshots, some of them more than once.  temporal_plan() lists the DISTINCT ones in the order of their first
// use and says which of them every tap reads, so that the kernel loads each array once per element and still does its arithmetic per tap.
//
// Everything here compiles with a plain C++ compiler as well (tests/hostcheck/temporal_steps.cpp).
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define TEMPORAL_HD __host__ __device__ inline
#else
#define TEMPORAL_HD inline
#endif

namespace ftkx {

constexpr int kTemporalMaxK = 9;
constexpr int kTemporalThreads = 256;
constexpr unsigned kTemporalMaxBlocks = 2048;      // the grid's cap (8 workgroups for each of 256 CUs); the rest is taken by the grid-stride loop

inline bool temporal_ksize_ok(int ksize) { return ksize >= 1 && ksize <= kTemporalMaxK && (ksize & 1) == 1; }

// ---- the state machine ---------------------------------------------------------------------------------------------------------------------
// Counts only: whoever owns the snapshots keeps them in a deque of its own and does what the answers say.
struct TemporalSeries {
  int ksize = 0;            // K; 0: no filter
  int size = 0;             // |data|
  int cursor = 0;
  bool finishing = false;
  int kind = -1;            // -1: no snapshot yet; 0: scalar snapshots; 1: vector snapshots
  TEMPORAL_HD int half() const { return (ksize + 1) / 2; }
  TEMPORAL_HD bool ready() const { return size >= half(); }
  TEMPORAL_HD void restart() { size = 0; cursor = 0; finishing = false; kind = -1; }      // the filter as it was constructed
};

enum { TEMPORAL_ADMIT_OK = 0, TEMPORAL_ADMIT_OFF = 1, TEMPORAL_ADMIT_MIXED = 2, TEMPORAL_ADMIT_FINISHING = 3 };

// may a snapshot of this kind be pushed?  (the reference's filter would go on with the finishing rule after finish(); here that is an error)
TEMPORAL_HD int temporal_admit(const TemporalSeries &s, int is_vector)
{
  if (!s.ksize) return TEMPORAL_ADMIT_OFF;
  if (s.finishing) return TEMPORAL_ADMIT_FINISHING;
  if (s.kind >= 0 && s.kind != (is_vector ? 1 : 0)) return TEMPORAL_ADMIT_MIXED;
  return TEMPORAL_ADMIT_OK;
}

// push(): the caller has appended the snapshot to its deque.  *pop_front: the deque's front leaves (before anything is read).  Returns
// whether an array is emitted; idx[0 .. K - 1] are then the deque places (after the pop) the taps read.
TEMPORAL_HD bool temporal_push(TemporalSeries &s, int is_vector, bool *pop_front, int *idx)
{
  s.kind = is_vector ? 1 : 0;
  s.size ++;
  *pop_front = s.size > s.ksize;
  if (*pop_front) { s.size --; s.cursor --; }
  if (!s.ready()) return false;
  for (int i = 0; i < s.ksize; i ++) { const int j = i + s.cursor - s.half() + 1; idx[i] = j > 0 ? j : 0; }
  s.cursor ++;
  return true;
}

// One round of finish()'s loop.  The caller pops its deque's front first whenever *pop_front says so (an empty deque has none: the
// reference's pop_front() of an empty deque is undefined; here the loop just stops).  Returns whether an array is emitted (idx as above);
// false: the loop stops -- the caller releases what is left in its deque, and the filter is as it was constructed.
TEMPORAL_HD bool temporal_finish_step(TemporalSeries &s, bool *pop_front, int *idx)
{
  *pop_front = s.size > 0;
  if (!*pop_front) { s.restart(); return false; }
  s.finishing = true;
  s.size --;
  if (!s.ready()) { s.restart(); return false; }
  for (int i = 0; i < s.ksize; i ++) idx[i] = i < s.size - 1 ? i : s.size - 1;
  s.cursor --;
  return true;
}

// ---- one emission ---------------------------------------------------------------------------------------------------------------------------
struct TemporalArgs {
  const double *src[kTemporalMaxK];      // the distinct arrays, in the order of their first use
  double w[kTemporalMaxK];               // the weight of every tap
  int tap[kTemporalMaxK];                // which of src[] every tap reads; tap[i] <= i, tap[0] == 0
};

// the K arrays of an emission (repeats allowed) -> distinct arrays + taps; returns how many distinct arrays there are
inline int temporal_plan(const double *const *arrays, int ksize, const double *weights, TemporalArgs *a)
{
  int nsrc = 0;
  for (int i = 0; i < kTemporalMaxK; i ++) { a->src[i] = nullptr; a->w[i] = 0.0; a->tap[i] = 0; }
  for (int i = 0; i < ksize; i ++) {
    int s = 0;
    while (s < nsrc && a->src[s] != arrays[i]) s ++;
    if (s == nsrc) a->src[nsrc ++] = arrays[i];
    a->tap[i] = s;
    a->w[i] = weights[i];
  }
  return nsrc;
}

// the value tap i reads, out of the NSRC values of one element: a chain of selects over the places it can be (tap <= i), so that `v`
// stays in registers -- an index that the compiler cannot see through would put it into scratch memory
template <int NSRC> TEMPORAL_HD double temporal_tap(const double (&v)[NSRC], int i, int tap)
{
  double x = v[0];
#pragma unroll
  for (int s = 1; s < NSRC; s ++) if (s <= i) x = tap == s ? v[s] : x;
  return x;
}

// one element of an emission: v[s] = its value in src[s]
template <int K, int NSRC> TEMPORAL_HD double temporal_sum(const double (&v)[NSRC], const TemporalArgs &a)
{
  static_assert(K >= 1 && K <= kTemporalMaxK && (K & 1) == 1 && NSRC >= 1 && NSRC <= K, "odd sizes from 1 to 9, at most K arrays");
  double acc = a.w[0] * v[0];
#pragma unroll
  for (int i = 1; i < K; i ++) {
    const double p = a.w[i] * temporal_tap<NSRC>(v, i, a.tap[i]);
    acc = acc + p;
  }
  return acc;
}

// the W doubles of element e in each of the NSRC arrays -> v[k][s]; W == 2: one 16-byte load per array
template <int NSRC, int W> TEMPORAL_HD void temporal_load(const TemporalArgs &a, size_t e, double (&v)[W][NSRC])
{
#pragma unroll
  for (int s = 0; s < NSRC; s ++) {
    if (W == 2) {
#if defined(__HIP_DEVICE_COMPILE__)
      const double2 t = reinterpret_cast<const double2 *>(a.src[s])[e];
      v[0][s] = t.x; v[W - 1][s] = t.y;
#else
      v[0][s] = a.src[s][e * W]; v[W - 1][s] = a.src[s][e * W + (W - 1)];
#endif
    } else v[0][s] = a.src[s][e];
  }
}

template <int W> TEMPORAL_HD void temporal_store(double *out, size_t e, const double (&r)[W])
{
  if (W == 2) {
#if defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<double2 *>(out)[e] = make_double2(r[0], r[W - 1]);
#else
    out[e * W] = r[0]; out[e * W + (W - 1)] = r[W - 1];
#endif
  } else out[e] = r[0];
}

// what one lane of workgroup `block` does: elements of W doubles in a grid-stride loop; the grid's first lane also takes, one double at a time, the tail that count % W leaves
template <int K, int NSRC, int W>
TEMPORAL_HD void temporal_lane(const TemporalArgs &a, size_t count, double *out, size_t block, size_t nblocks, int tid)
{
  const size_t nvec = count / W, stride = nblocks * (size_t)kTemporalThreads;
  for (size_t e = block * (size_t)kTemporalThreads + (size_t)tid; e < nvec; e += stride) {
    double v[W][NSRC], r[W];
    temporal_load<NSRC, W>(a, e, v);
#pragma unroll
    for (int k = 0; k < W; k ++) r[k] = temporal_sum<K, NSRC>(v[k], a);
    temporal_store<W>(out, e, r);
  }
  if (W > 1 && block == 0 && tid == 0)
    for (size_t e = nvec * W; e < count; e ++) {
      double v[NSRC];
#pragma unroll
      for (int s = 0; s < NSRC; s ++) v[s] = a.src[s][e];
      out[e] = temporal_sum<K, NSRC>(v, a);
    }
}

// how many workgroups an emission of `count` doubles at W doubles per lane is launched with
inline unsigned temporal_blocks(size_t count, int W)
{
  const size_t want = (count / (size_t)W + (size_t)kTemporalThreads - 1) / (size_t)kTemporalThreads;
  return want < 1 ? 1u : want > (size_t)kTemporalMaxBlocks ? kTemporalMaxBlocks : (unsigned)want;
}

// the arrays and the output lie so that 16-byte accesses are allowed
inline bool temporal_aligned16(const TemporalArgs &a, int nsrc, const double *out)
{
  size_t bits = (size_t)out;
  for (int s = 0; s < nsrc; s ++) bits |= (size_t)a.src[s];
  return (bits & 15) == 0;
}

}  // namespace ftkx
