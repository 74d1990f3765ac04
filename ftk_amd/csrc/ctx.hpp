// Shared between the translation units of libftkx.so that implement the C ABI of include/ftkx.h (ftkx_api.hip: context, slices,
// options, one-shot calls; ingest.hip: how snapshots come in -- pushes, smoothing, perturbation and clamp, the temporal ring; prepare.hip: the one-pass mask + reduction pre-pass; collect.hip: the batched sweep; halo.hip: the compact
// t-slab halo; series.hip: the device-driven pass over a resident series).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <vector>

#include "sweep_params.hpp"
#include "split_policy.hpp"
#include "batch_plan.hpp"
#include "series_verdict.hpp"
#include "internal.hpp"
#include "pass2_layout.hpp"
#include "ctx_block.hpp"
#include "temporal_steps.hpp"
#include "adjust_steps.hpp"
#include "sample_steps.hpp"
#include "conv_vec_steps.hpp"

struct ftkx_phase_clock;

namespace ftkx {
void mask_kernel_launches(unsigned long long *out, const char **names);
void launch_tile(const TileParams &p, hipStream_t stream);
void launch_tile_stats_fold(u64 *slots, u64 *counters, hipStream_t stream);
void tile_dims(int nd, int tile[3]);
void launch_masks(const Mesh &m, const MaskJob *d_jobs, int njobs, hipStream_t stream);
void launch_cull(const Mesh &m, const Fields *d_steps, int nsteps, u64 *d_list, u64 cap, hipStream_t stream, const FactorJob *job = nullptr);
void launch_exact(const Mesh &m, const Fields *d_steps, int step_base, const u64 *d_list, u64 cap, hipStream_t stream, int few_wgs = 0);
void launch_records(const Mesh &m, const Fields *d_fields, hipStream_t stream);
void launch_compact_words(const Mesh &m, const unsigned char *U, const unsigned char *M, unsigned *idx, u64 *words, u64 capacity, u64 *counter, hipStream_t st);
void launch_scatter_words(const unsigned *idx, const u64 *words, size_t n, unsigned char *M, size_t mask_words, u64 *bad, hipStream_t st);
void launch_pack_masks(u64 *hdr, const u64 *counter, const unsigned char *U, u64 u_bytes, u64 capacity, int u_rows, int factor_log2, hipStream_t st);
void launch_scatter_packed(const u64 *hdr, const unsigned *idx, const u64 *words, u64 u_bytes, u64 capacity, int u_rows, int max_factor_log2, unsigned char *U, unsigned char *M,
                           size_t mask_words, u64 *bad, hipStream_t st);
void launch_sparse_cells(const Mesh &m, const Fields *d_steps, const u64 *d_list, u64 cap, const double *sparse, u64 *cells, u64 cells_cap, hipStream_t st);
void launch_patches(const Mesh &m, bool scatter, const u64 *cells, size_t n, int ncomp, double *field, double *patches, hipStream_t st);
bool masks_have_summary(const Mesh &m);      // these three: readers of the mask plan (mask_plan.hpp)
int mask_summary_rows(const Mesh &m);
bool march2_supported(const Mesh &m);
void launch_reduce_march(const Mesh &m, const MaskJob *d_jobs, int njobs, hipStream_t stream);
void launch_cull_two_level(const Mesh &m, const Fields *d_steps, int nsteps, u64 *d_refine, u64 refine_cap, u64 *d_list, u64 cap, hipStream_t stream);
void launch_resolution_scalar(const Mesh &m, const double *S, u64 *out2, hipStream_t stream);
void launch_gradient2d(const double *S, int DW, int DH, double *V, hipStream_t st);
void launch_jacobian2d(const double *V, int DW, int DH, int symmetric, double *J, hipStream_t st);
void launch_gradient3d(const double *S, int DW, int DH, int DD, double *V, hipStream_t st);
void launch_jacobian3d(const double *V, int DW, int DH, int DD, double *J, hipStream_t st);
void launch_resolution(const double *p, size_t n, u64 *out2, hipStream_t st);
template <class SRC> void launch_conv(int nd, const SRC *S, int DW, int DH, int DD, const double *d_weights, int ksize, double *out, hipStream_t st);   // conv_kernels.hip: SRC double or float
// conv_vec_kernels.hip: every component of a vector array as the scalar field it is, interleaved FP64 out; SRC double or float
template <class SRC> void launch_conv_vec(int nd, const ConvVecSource<SRC> &src, int DW, int DH, int DD, const double *d_weights, int ksize, double *out, hipStream_t st);
void launch_widen(const float *src, size_t count, double *dst, hipStream_t st);   // widen_kernels.hip
void launch_narrow(int dtype, const void *src, size_t count, double *dst, hipStream_t st);   // narrow_kernels.hip: dtype FTKX_DTYPE_F16 .. _I32
template <class T> void launch_adjust(const T *src, size_t count, bool perturb, bool clamp, const AdjustArgs &a, double *dst, hipStream_t st);   // adjust_kernels.hip: T double or float; src == dst allowed
template <class T> bool launch_concat(const T *const *planes, int nc, size_t count, double *dst, hipStream_t st);   // concat_kernels.hip: T double or float; whether the 16-byte body ran
void launch_temporal(const double *const *arrays, int ksize, const double *weights, size_t count, double *out, hipStream_t st);   // temporal_kernels.hip
void launch_sample(int nd, const SampleMesh &m, const SampleIn *in, size_t n, const SampleSlice *tab, int t_min, unsigned slots, double *out, hipStream_t st);   // sample_kernels.hip
void launch_series_sample(int nd, const SampleMesh &m, ftkx_cp_t *recs, const u64 *counters, u64 capacity, const SampleSlice *tab, int t_min, int ntab, unsigned slots,
                          unsigned workgroups, hipStream_t st);   // sample_kernels.hip: in place over the records of a series pass
void launch_calib_read(const void *p, size_t bytes, double *scratch, hipStream_t stream);
const char *last_mask_kernel();
void launch_cull_coarse(const Mesh &m, const Fields *d_steps, int nsteps, u64 *d_refine, u64 refine_cap, hipStream_t stream, const FactorJob *job = nullptr);
void launch_refine(const Mesh &m, const Fields *d_steps, const u64 *d_refine, u64 refine_cap, u64 *d_list, u64 cap, hipStream_t stream, int few_wgs = 0);
void launch_series_begin(u64 *counters, u64 *red, size_t nslots, unsigned *hist, size_t nbins, u64 *results, size_t nresults, hipStream_t st,
                         const void *desc_src = nullptr, void *desc_dst = nullptr, size_t desc_bytes = 0, unsigned *fetched = nullptr, unsigned fetched_val = 0);
void launch_series_one(const Mesh &m, const OneArgs &a, int nwg, hipStream_t st);
void launch_series_tail_begin(u64 *counters, unsigned *hist, size_t nbins, u64 *results, size_t nresults, hipStream_t st);
void launch_series_factors(Fields *steps, int nsteps, const SeriesSlice *slices, int nslices, const SeriesStep *sinfo, const u64 *red, double running_in, const u64 *running_from,
                           double safe_m, u64 *results, u64 *counters, hipStream_t st);
unsigned launch_bucket_rank(const Mesh &m, const u64 *bucketed, const unsigned *boff, u64 *sorted, u64 *results, hipStream_t st, int few_wgs = 0);   // -> the rank_max it was launched with
void launch_bucket_scan(unsigned *hist, unsigned *boff, unsigned nbins, u64 *counters, hipStream_t st, bool small_wg = false);
void launch_bucket_scatter(const Mesh &m, unsigned *boff, u64 *bucketed, hipStream_t st, int few_wgs = 0);
void launch_series_records(const Mesh &m, const Fields *d_fields, const u64 *sorted, ftkx_cp_t *out, hipStream_t st, bool lean = false);
Mesh coarse_view(const Mesh &m);
void launch_series_small(const Mesh &m, const Mesh &mc, const Fields *d_steps, bool two_level, const u64 *d_refine, const u64 *d_list, ftkx_cp_t *out,
                         u64 *results, size_t nwords, u64 *h_results, unsigned *flag, unsigned seq, unsigned *done, bool report_decline, hipStream_t st);
void launch_series_copy_out(const ftkx_cp_t *src, ftkx_cp_t *dst, u64 capacity, const u64 *results, unsigned *done, unsigned *flag, unsigned seq, hipStream_t st,
                            const unsigned *wait_flag = nullptr, unsigned wait_val = 0);
void launch_series_finish(const Mesh &m, u64 *results, size_t nwords, u64 list_capacity, u64 refine_capacity, u64 *h_results, unsigned *flag, unsigned seq, hipStream_t st);
// dist_kernels.hip: the slab pass
void launch_dist_contrib(const SeriesSlice *slices, int nown, const u64 *red, u64 *contrib, u64 *block, hipStream_t st);
void launch_dist_export(const Mesh &m, const unsigned char *U, const unsigned char *M, u64 u_bytes, u64 *hdr, unsigned *idx, u64 *words, u64 capacity, int factor_log2, u64 *block, hipStream_t st);
void launch_dist_import(const u64 *gathered, int rank, int nranks, double running_in, u64 *block, u64 *results_tail, const u64 *hdr, const unsigned *idx, const u64 *words, u64 u_bytes,
                        u64 capacity, int u_rows, int max_factor_log2, unsigned char *U, unsigned char *M, u64 mask_words, hipStream_t st);
void launch_dist_cells(const Mesh &m, const Fields *d_steps, const u64 *d_list, u64 list_capacity, u64 refine_capacity, const double *halo_field, u64 *request, u64 cap, u64 *block, u64 *results, hipStream_t st);
void launch_dist_patches(const Mesh &m, bool scatter, const u64 *request, u64 cap, int ncomp, double *field, double *patches, u64 *served, hipStream_t st);
// trace_order_kernels.hip: pass 2 from neighbours, degrees and roots to ordered curves (trace_device.hip: ftkx_trace_curves_device)
struct TraceOrder {
  int n, nd, ntypes, maxnb;
  long long sz[3];
  u64 prod[4];
  const u64 *tags; const int *nbr; const unsigned char *deg; const int *root;      // what the three kernels of trace_device.hip left
  u64 *key, *best, *link, *info;     // per record: order key; per root: smallest key; per arc: (link << 32) | distance; per seed: key, record | length << 32
  int *on, *cnt;                     // per record: first / last ordinary neighbour (-1: none); per root: points behind / in front of the seed
  int *cyc, *seedpos, *seedlist;     // per root: the curve is closed, where its seed lies in `indices`; the seeds in no order
  int *indices, *loop, *off, *sorted;   // the curves: points, loop flags; from the host: offsets, the seeds in key order
  unsigned *counters;                // TRO_* words (pass2_layout.hpp), then one "not done" flag per jump launch
};
void launch_trace_check(const u64 *tags, int n, u64 per_step, unsigned *counters, hipStream_t st);
void launch_trace_order_begin(const TraceOrder &o, hipStream_t st);                // keys, ordinary neighbours, seeds, arcs
void launch_trace_order_jump(const TraceOrder &o, int round, hipStream_t st);      // one round of pointer jumping over the arcs
void launch_trace_order_ends(const TraceOrder &o, unsigned nseeds, hipStream_t st);   // chain lengths, closed curves, the seeds' (key, record, length)
void launch_trace_order_scatter(const TraceOrder &o, int ncurves, int npoints, hipStream_t st);   // points to their places, loop flags
// post_process_kernels.hip: the maps and scans of post_process_steps.hpp, queued in order (post_process_device.hip)
constexpr size_t kPostProcAggBytes = 16;                   // per tile of a scan: its total
size_t post_process_tiles(size_t np);                      // how many totals `agg` must hold
hipError_t launch_post_process(const PostProc &p, void *agg, ftkx_phase_clock &clock);   // on the clock's stream, one lap per group of steps
}  // namespace ftkx

// Phase timing of pass 2 on the device (FTKX_TRACE_PHASES, FTKX_POST_PROCESS_PHASES): where it is on, the host waits for the stream after
// every phase and prints "prefix: name, microseconds since the lap before" to stderr.  A measuring aid: the waits cost time of their own.
struct ftkx_phase_clock {
  bool on;
  hipStream_t stream;
  const char *prefix;
  std::chrono::steady_clock::time_point first, last;
  void start() { if (on) first = last = std::chrono::steady_clock::now(); }
  hipError_t lap(const char *what, size_t count)
  {
    if (!on) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(stream);
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "%s: %-32s %8.1f us  (%zu)\n", prefix, what, std::chrono::duration<double, std::micro>(now - last).count(), count);
    last = now;
    return e;
  }
  double us_in_all() const { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - first).count(); }   // since start()
};

using ftkx::Fields;
using ftkx::MaskJob;
using ftkx::Mesh;
using ftkx::TileParams;
using ftkx::u64;

namespace ftkxh {

// 2D scalar slices: gradient2D's (D - 1) scaling folded into exact thresholds of the unscaled differences (MaskJob::tx, ty)
inline MaskJob with_lean_thresholds(MaskJob j, const Mesh &m)
{
  if (m.nd == 2 && m.scalar_mode && j.threshold > 0.0) {
    j.tx = ftkx::exact_threshold(j.threshold, (double)(m.ext_sz[0] - 1));
    j.ty = ftkx::exact_threshold(j.threshold, (double)(m.ext_sz[1] - 1));
  }
  return j;
}

struct Slice {                      // move-only: it owns its arrays
  ftkx_block V, J, S;               // double: out of the context's pool (class field), or lent by the caller (ftkx_block::lent)
  ftkx_block M;                     // unsigned char: vertex sign masks, built lazily for `mask_factor`
  ftkx_block U;                     // unsigned char: per-8-vertex summaries of M (two-level cull)
  unsigned long long mask_factor = 0;   // the (power-of-two) factor M / U were built under; 0 = not built
  int u_rows = 1;                   // rows a byte of U stands for (Mesh::u_rows at the time the masks were built)
  bool mask_big = false;            // built with the per-vertex overflow rule of that factor (MaskJob::big finite)
  bool have_res = false;            // res = ndarray::resolution() of the slice's vector field (exact pre-pass), maxabs with it
  double res = 0, maxabs = 0;
  bool have_fused = false;          // reduction fused into the mask pass (ftkx_slices_prepare): maxabs, and
  double res_below = 0;             //   the smallest non-zero |v| below 1 / fused_factor (DBL_MAX if none)
  unsigned long long fused_factor = 0;
  bool sparse = false;              // a halo slice that exists as masks only: its field array holds just the patches scattered into it
  unsigned long long mask_gen = 0;  // changes whenever the masks are (re)built, dropped or the slice replaced: a series pass collected later marks only what is still its own
  bool max_known() const { return have_res || have_fused || sparse; }
};

// what the batch plan (batch_plan.hpp) is told of a slice
inline SliceFacts slice_facts(const Slice &s) { return SliceFacts{s.M.p != nullptr, s.U.p != nullptr, s.sparse, s.mask_factor, s.mask_big, s.u_rows, s.max_known(), s.maxabs}; }

struct Request { int t, scope; unsigned long long factor; int mode; };      // mode: MODE_* (batch_plan.hpp, request_mode)

enum { K_MASK = 0, K_CULL = 1, K_EXACT = 2, K_TILE = 3, K_N = 4 };


}  // namespace ftkxh

// A series pass that has been queued (ftkx_sweep_series_submit) and not yet collected (ftkx_sweep_series_complete): what the second half
// of the call needs.  Up to ftkx_ctx::kPlaces (three) may be open at a time: the host prepares and queues pass N + 1 while the device still
// works on pass N, and the records of pass N cross PCIe (a copy engine, not a kernel) while the mask kernel of pass N + 1 runs.
struct ftkx_series_pending {
  bool open = false;
  bool by_host = false;             // not queued: the host-driven batch sweeps it when it is collected
  std::vector<int> ts, scopes, slice_ts, red_index;
  std::vector<unsigned long long> gen;   // per slice: Slice::mask_gen as this pass left it
  int n = 0, buf = 0;
  size_t k = 0, nwords = 0, nbins = 0;
  unsigned long long hint = 0;
  bool two_level = false, short_chain = false, small_now = false, to_device = false;
  bool copy_pending = false;        // to_device: the copy kernel has not been queued yet (it goes behind the descriptor fetch of the next pass, or is queued when the pass is collected)
  int u_rows = 1;
  u64 cells = 0;
  unsigned seq = 0;
  unsigned long long uid = 0;       // ftkx_ctx::sr_pass_uid when the pass was queued (owner stamp of the counters and lists)
  double running_in = 0;
  bool chained = false;             // the running minimum came from the pass before it on the device (running_in: what the host knew)
  size_t off_steps = 0, off_slices = 0, off_sinfo = 0, ntodo = 0;
  int shift = 0;                    // order key -> bucket
  const u64 *running_from = nullptr;   // a results block on the device whose SR_RUNNING word this pass continues from (the pass before it, or a slab pass's stub)
  bool refined = false;             // the refine kernel has been queued already (a slab pass lists the halo's cells from its output)
  // split pass (series.hip, "the tail next to the next mask kernel"): begin + masks on the context's stream, the tail -- counters, cull + factors,
  // the kernel chain -- on the tail stream behind an event, next to the mask kernel of the pass queued behind it
  bool split = false;
  int before_buf = -1;              // the place of the split pass that was open when this one was planned (its factor job is waited for by this pass's tail), or -1
  int cal_kind = 0;                 // a pass of the split calibration: 1 measured in order, 2 measured split
  int tail_set = 0;                 // which of ftkx_ctx::sr_tail its tail works on (series.hip: tail_of): 0 unless it is every other split pass of a short mask launch
  bool split_sparse = false;        // ... of a sparse pass: few workgroups per chain kernel, 2^10 buckets
  bool one = false;                 // the one-launch pass for small series (one_kernel.hip)
  std::vector<std::pair<ftkx_block, ftkx_block>> retired;   // (M, U) arrays this pass still reads, replaced in their slices by the pass queued behind it
  std::vector<ftkxh::Slice> parked;        // slices dropped (or replaced) while this split pass was the newest one open: its tail -- on a stream of its own -- may still read
                                    // their arrays, which go back to the pools when it has been completed (release_retired)
  std::vector<ftkx_block> parked_aux;      // aux arrays dropped or replaced meanwhile: the same decision (ingest.hip, retire_aux), the same release
  // an armed pass (ftkx_set_series_sampling) that has a slot to fill: the sample kernel runs behind its record kernel, in place over B.d_out
  unsigned sample_slots = 0;        // bit s: slot s + 1 is sampled (the slot rule, decided when the pass was planned); 0: planned as an unarmed pass
  size_t off_sample = 0;            // its slice table in the descriptor block: SampleSlice per timestep sample_t_min .. + sample_ntab
  int sample_t_min = 0, sample_ntab = 0;
  // slab pass (ftkx_series_dist_*): one rank's part of a series cut into timestep slabs, queued in stages with the caller's collectives between them
  bool dist = false;
  int dist_stage = 0;               // 1 begun (masks, contribution, outgoing masks), 2 culled (request written), 3 served (reply written), 4 finished = open
  int t_halo = -1;                  // the slice this rank's last interval sweep reads and does not own: masks + patches arrive inside the pass; -1: none
  int dist_rank = 0, dist_nranks = 1, dist_upper = -1;     // dist_upper: the rank that owns t_halo (not rank + 1 where slabs are empty)
  const u64 *gathered = nullptr;    // device, kDistContrib words per rank: where the caller's all_gather puts the contributions
  u64 *request_out = nullptr;       // device: this rank's request to its upper neighbour (count, cells)
};

// what one of the passes in flight writes that the host reads, or that a copy engine reads after the pass
struct ftkx_series_buffers {
  ftkx_block results;                                  // u64: the device block
  ftkx_block h_results{FTKX_BLOCK_PINNED_COHERENT};    // u64: its pinned copy; the last 8 words are the flag words (series.hip: series_flag)
  unsigned seq = 0;
  unsigned rank_max = 0;                               // what the rank kernel of the pass on these buffers was launched with (launch_bucket_rank)
  ftkx_block out{FTKX_BLOCK_PINNED_COHERENT};          // ftkx_cp_t: the records as the caller reads them (kind: series.hip, ensure_series_buffers)
  ftkx_block d_out;                                    // ftkx_cp_t: the records of a pass whose way over PCIe is left to the copy kernel on its own stream
  ftkx_block copy_done;                                // unsigned: that kernel's workgroup counter
  hipEvent_t ev_copied = nullptr, ev_export = nullptr;
  hipEvent_t ev_masks = nullptr, ev_factors = nullptr, ev_tail = nullptr;   // split pass: masks done (stream), cull + factor job / tail done (tail stream)
  ftkx_block red;                                      // u64: the reduction slots of this pass's mask jobs (128 words per slice): its own, the next pass's begin kernel must not wipe them
  bool copy_out = false;                               // a copy has been queued since the buffers were last used: the next record kernel waits for it
  ftkx_block h_desc{FTKX_BLOCK_PINNED}, d_desc;
  ftkx_block dist_block;                               // u64: slab pass, DB_N words (sweep_params.hpp)
};

// What the tail of a sweep works on, and the stream a SPLIT pass's tail runs on.  The context has two (ftkx_ctx::sr_tail).  Set 0 is what the
// host-driven batch (collect.hip, prepare.hip, halo.hip) and every pass that is not split work on, in the order of the context's stream.  Set 1
// (same capacities: ensure_set1) is for every other split pass of a short mask launch, so that the tails of two passes can run at the same time --
// a mask launch shorter than one tail next to it (a single 512^3 slice) then still hides half a tail behind every mask kernel.
struct ftkx_tail_set {
  ftkx_block counters;              // u64: CNT_N counters + 128 words (64 {min, max} slots) for the resolution reduction + 8
  ftkx_block list;                  // u64: surviving corners of the fast path
  ftkx_block refine;                // u64: words the summary level could not rule out (two-level cull)
  ftkx_block pass;                  // u64: simplices that passed the integer test, awaiting the record kernel
  ftkx_block fragile;               // u64: 3D records to be re-classified on the host (slot, J[9]): cp_device.hpp, classify3
  ftkx_block bucketed, sorted;      // u64: series pass, the order keys by bucket, and ranked
  ftkx_block hist, boff;            // unsigned: series pass, bucket counts and offsets
  // what the kernels are handed: the element counts of pass, list, refine and fragile (10 words each), set by their ensure_* (ftkx_api.hip)
  // on the line behind the reserve and nowhere else.  `capacity` is how far THIS set's pass array has followed ftkx_ctx::capacity.
  u64 capacity = 0, list_capacity = 0, refine_capacity = 0, fragile_capacity = 0;
  hipStream_t stream = nullptr;     // the tail of a split pass on this set; created where the first such pass is planned
};

// Pass 2 on the device (trace_device.hip, post_process_device.hip): every block it keeps with the context.  A call lays its arrays out
// (pass2_layout.hpp), reserves the blocks for the layout's totals and works on the context's stream, which it waits for before it returns:
// what a block held does not outlive the call, but for the curves of the last trace that went all the way on the device (`order`).
// Every block grows by a quarter more than it is asked for (pass2_room).
inline size_t pass2_room(size_t want) { return want + want / 4; }
struct ftkx_pass2_state {
  ftkx_block trace_dev, trace_host{FTKX_BLOCK_PINNED_NONCOHERENT};   // TraceLayout
  ftkx_block tables;                                                 // the neighbour search's candidate tables of dimension `tables_nd`
  ftkx_block order_dev, order_host{FTKX_BLOCK_PINNED_NONCOHERENT};   // OrderLayout
  ftkx_block pp_dev, pp_host{FTKX_BLOCK_PINNED_NONCOHERENT};         // PpPlan
  int tables_nd = 0;
  ftkx::OrderLayout order;             // of the last trace that ended with path 2: where its curves lie in order_dev
  int trace_last_path = 0;             // which way the last trace went: 0 host, 1 device phases + host walks, 2 all on the device
  int pp_last_path = 0;                // which way the last post-processing went: 0 host, 2 all on the device
};

struct ftkx_ctx {
  int nd = 0, device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  ftkx_options opt;
  long long dom_st[3] = {0, 0, 0}, dom_sz[3] = {1, 1, 1}, core_st[3] = {0, 0, 0}, core_sz[3] = {1, 1, 1}, ext_st[3] = {0, 0, 0}, ext_sz[3] = {1, 1, 1};
  bool mesh_set = false;
  int scalar_mode = -1;             // -1 undecided, 0 vector slices, 1 scalar slices (V = gradient(S) evaluated in flight)
  std::map<int, ftkxh::Slice> slices;
  ftkx_block d_hits;                // ftkx_cp_t
  u64 capacity = 0;                 // records d_hits holds (set in ensure_hit_buffer), and the pass array of every tail set in use
  ftkx_tail_set sr_tail[2];         // [0]: the host-driven batch's and every unsplit pass's
  ftkx_block d_tile_stats;          // u64, 512 words: the tile kernels' statistics in 256 slots (TileParams::stats)
  ftkx_block h_counters{FTKX_BLOCK_PINNED};              // u64, CNT_N words
  ftkx_block h_hits{FTKX_BLOCK_PINNED_NONCOHERENT};      // ftkx_cp_t
  // device-side ordering of the hit records by tag (radix sort of (tag, index) pairs + one gather): collect.hip, sort_hits_on_device
  ftkx_block d_sorted;              // ftkx_cp_t, sort_cap of them
  ftkx_block d_keys, d_idx;         // u64 / unsigned, 2 * sort_cap each
  ftkx_block d_sort_tmp;            // unsigned: digit counts per tile
  // per-batch descriptors: pinned staging + device copies
  ftkx_block h_desc{FTKX_BLOCK_PINNED}, d_desc;
  // field (S / V / J copies), mask and summary arrays of dropped slices, kept for the next slice (ctx_block.hpp).  The padding bytes of a
  // mask or summary array stay valid: kernels never write them.
  ftkx_array_pool arrays;
  ftkx_block d_red;                 // u64: {min, max} slots of a batched resolution reduction, 128 words per slice (ensure_red)
  // physical coordinates (REGULAR_COORDS_RECTILINEAR / _EXPLICIT): device copies
  ftkx_block d_rect[3];             // double
  size_t rect_n[3] = {0, 0, 0};
  ftkx_block d_expl;                // double
  int expl_ncomp = 0;
  size_t expl_n0 = 0, expl_n1 = 0;
  // spatial smoothing (ftkx_set_spatial_smoothing): ksize 0 = off; d_conv_w holds three sets of 9^3 weights -- [0] those of the ftkx_conv2D /
  // ftkx_conv3D / ftkx_conv*_vec / ftkx_conv_planar call in hand (the call waits for its kernel), [1] the smoothing's, [2] the vector
  // smoothing's, each written when it is set and only read afterwards
  int smooth_ksize = 0;
  double smooth_sigma = 0;
  ftkx_block d_conv_w;              // double
  // spatial smoothing of VECTOR snapshots, per component (ftkx_set_vector_smoothing; conv_vec_steps.hpp): a setting of its own, ksize 0 = off.
  // The launches of its kernel by pushes, by the source's form, and how many of them read floats: ftkx_debug_conv_vec_counts.
  int vsmooth_ksize = 0;
  double vsmooth_sigma = 0;
  unsigned long long conv_vec_interleaved = 0, conv_vec_planar = 0, conv_vec_f32 = 0;
  // temporal smoothing (ftkx_set_temporal_smoothing): the filter's state (temporal_steps.hpp), its weights and the ring of RAW snapshots
  // (after the spatial smoothing where that is set) -- at most ksize arrays of one size, taken from and given back to `arrays`.
  // Only kernels on the context's stream read them.  tm_next: the timestep the next emission gets.
  ftkx::TemporalSeries tm;
  double tm_sigma = 0, tm_w[ftkx::kTemporalMaxK] = {0};
  std::deque<ftkx_block> tm_ring;
  int tm_next = 0;
  hipEvent_t tm_read = nullptr;     // behind the staging of a device source: what ftkx_temporal_push waits for before it returns
  // float32 sources (ftkx_push_scalar_slice_f32, ftkx_push_slice_f32, ftkx_temporal_push_f32): a host array, or an array of another device, lies
  // here as it came, 4 bytes per value, until the widen kernel or the convolution has made the FP64 slice of it.  Reserved by the bytes of
  // that very array (count * sizeof(float)), drained by the stream that read it last.  Written by the upload's DMAs or a copy on the
  // context's stream, read by one kernel on the context's stream: how the next push's writes are ordered behind that kernel is said where
  // it is filled (ingest.hip, ingest).
  ftkx_block f32_stage;
  hipStream_t f32_stage_reader = nullptr;      // the stream of the kernel that read it last
  unsigned long long f32_widened = 0, f32_direct = 0;   // ftkx_debug_f32_counts: float32 arrays through the widen kernel / straight through the convolution
  // narrow sources (ftkx_push_*_typed, ftkx_temporal_push_typed: half, bfloat16, 8- / 16- / 32-bit integers): staged in f32_stage as they
  // came, count * the element's size bytes, under the same ordering; the narrow kernel's launches by FTKX_DTYPE_* (ftkx_debug_narrow_counts)
  unsigned long long narrow_launches[10] = {0};
  // perturbation and clamp (ftkx_set_perturbation, ftkx_set_clamp; adjust_steps.hpp): both off by default.  While either is on, every
  // snapshot pushed is adjusted by ONE kernel on the context's stream behind the widening and the spatial smoothing and in front of the
  // temporal ring (the stream's order), with its timestep as the noise's snapshot number.  The counters: ftkx_debug_adjust_counts.
  struct Adjust {
    double sigma = 0, lo = 0, hi = 0;
    unsigned long long seed = 0;
    bool perturb = false, clamp = false;
    bool on() const { return perturb || clamp; }
  } adj;
  unsigned long long tm_pushed = 0;            // raw pushes of the temporal series so far: t0 + tm_pushed is the next raw snapshot's number
  int tm_t0 = 0;
  unsigned long long adj_from_float = 0, adj_in_place = 0, adj_out_of_place = 0;
  // vector snapshots given as one array per component (ftkx_push_slice_planar, ftkx_temporal_push_planar, ftkx_concat; concat_steps.hpp): the
  // launches of the concat kernel by its path -- ftkx_debug_planar_counts.  Host planes are staged like every other source: floats in
  // f32_stage (each plane at a multiple of 16 bytes), doubles in a pooled array.
  unsigned long long planar_vec = 0, planar_scalar = 0;
  // auxiliary scalar fields (ftkx_push_aux_slice, ftkx_sample_aux; sample_steps.hpp): per timestep the arrays that record slots 1 and 2 are
  // sampled from -- field-class arrays out of `arrays`, or lent by the caller -- next to the slices, not in them: no sweep reads them, and a
  // slice that is pushed again keeps them.  They leave with ftkx_drop_slice(t).  Two kernels read them: the sample kernel of
  // ftkx_sample_aux on the context's stream, which the call waits for, and the sample kernel of an armed series pass
  // (ftkx_set_series_sampling), which runs where the pass's tail runs -- on the context's stream, or for a split pass on a tail stream that
  // is in no order with whatever takes the array out of the pool next.  So a dropped or replaced array takes the way a dropped slice's
  // arrays take (free_slice): parked with the newest open pass where that one is split (ftkx_series_pending::parked_aux, released by
  // release_retired), straight back to the pool otherwise.  sm_*: what a call sends up (16 bytes per record, the table of slice pointers)
  // and brings down (8 bytes per record and slot), kept between calls.
  struct AuxSlice { ftkx_block A[2]; };
  std::map<int, AuxSlice> aux;
  ftkx_block sm_h_in{FTKX_BLOCK_PINNED}, sm_d_in, sm_d_out, sm_h_out{FTKX_BLOCK_PINNED_NONCOHERENT}, sm_d_tab;
  unsigned long long sm_launches = 0, sm_records = 0;      // ftkx_debug_sample_counts
  // ftkx_set_series_sampling: series passes fill scalar[1] / scalar[2] themselves (series.hip).  sr_sampled_*: ftkx_series_sampled, of the
  // pass completed last; ss_*: ftkx_debug_series_sample_counts, the in-pass launches, the records of the passes they belonged to (known
  // when a pass completes) and the grid of the last launch
  bool sr_sampling = false;
  unsigned sr_sampled_slots = 0;
  int sr_sampled_where = 0;
  unsigned long long ss_launches = 0, ss_records = 0;
  unsigned ss_last_wgs = 0;
  std::vector<ftkxh::Request> pending;
  // Cull-ahead: the sweeps the caller announced (ftkx_sweep_announce) for the slices of the next ftkx_slices_prepare, and -- once that
  // call has queued their cull right behind the mask kernel -- the survivor list it left on the device.  The cull needs the masks
  // and the list of steps, not the factor: it runs while the host still waits for the reduction, forms the factors and queues the
  // sweeps.  ftkx_sweep_collect takes the list over if the pending sweeps are exactly the announced ones and every mask serves its
  // factor; anything else (and any call that touches slices or masks in between) drops it.
  std::vector<std::pair<int, int>> announced;
  struct AheadStep { int t, scope; const unsigned char *M[2], *U[2]; };
  std::vector<AheadStep> ahead;     // non-empty: survivor list + counters on the device belong to these steps
  ftkx_block h_ahead{FTKX_BLOCK_PINNED_COHERENT}, d_ahead;   // the cull-ahead's own descriptors: pinned staging (read by fetch_desc_kernel) + device copy
  bool ahead_staged = false;        // a fetch out of h_ahead may still be queued (cleared by every full stream synchronise of collect)
  ftkx_block h_red{FTKX_BLOCK_PINNED_COHERENT};   // u64: copy of the reduction slots, written by readback_kernel; its last 8 words hold the flag
  unsigned red_seq = 0;
  int dense_collects = 0;           // > 0: the last fast collect found most cells surviving; fast requests run MODE_TILE_CULL for a while
  unsigned long long uploads_staged = 0, uploads_direct = 0;   // ftkx_debug_upload_counts (upload.cpp)
  int tile_repeat = 1;              // ftkx_debug_tile_repeat: the tile kernel's fan phase that many times per tile (the int-VALU yardstick of bench.py)
  // compact halo: the compacted mask words of the last ftkx_export_masks_size, the surviving cells of the last ftkx_sweep_cull
  ftkx_block d_word_idx, d_words; size_t n_words = 0; int words_t = -1;     // unsigned / u64
  ftkx_block d_cells; size_t n_cells = 0;                                    // u64
  ftkx_block d_patch_cells, d_patches;                                       // u64 / double: staging for host-side callers
  ftkx_block d_packed;                                                       // staging of a packed mask message for host-side callers
  // series pass (series.hip): per pass in flight the results block (device + coherent pinned copy: it also holds the fragile list, the flag
  // lives behind it), the record buffers and the descriptors; shared, in stream order: the ordering buffers
  static constexpr int kPlaces = 3;   // passes in flight at most: two keep the stream fed; the third lets the host run one pass ahead of a split pass's
                                      // tail, which ends behind the mask kernel of the pass after it
  ftkx_series_buffers sr_buf[kPlaces];
  ftkx_series_pending sr_pend[kPlaces];
  int sr_place(int k) const { return (sr_head + k) % kPlaces; }      // the k-th oldest open pass's place
  int sr_open = 0, sr_head = 0;       // passes open, and which of sr_pend is the oldest
  bool sr_internal = false;           // the host-driven batch is sweeping for a series pass: its calls are let through while passes are open
  // which pass the counters and survivor lists of tail set 0 belong to right now: stamped when a pass's
  // cull is queued, cleared whenever the host-driven batch takes them (series.hip: a pass whose fused tail declined may queue the rest of
  // its chain only while they are still its own)
  unsigned long long sr_pass_uid = 0, sr_lists_owner = 0;
  hipStream_t sr_copy_stream = nullptr;
  ftkxh::split_cal sr_cal;              // the split pass's self-check (split_policy.hpp)
  int sr_split_forced = 0;              // the last plan's FTKX_SERIES_HOOKS split setting: 0 auto, 1 forced on (2, 3, 4), 2 forced off (0)
  double sr_last_complete_s = 0;        // host clock of the last completion (0: the pipeline ran empty since)
  int sr_last_complete_kind = 0;        // 1 in order / 2 split, of a calibration pass; 0 otherwise
  unsigned sr_split_seq = 0;          // split passes queued so far: their parity picks the set
  ftkx_block sr_one_scratch;           // u64: the one-launch pass's barrier counters, partial reductions and per-workgroup counts (ONE_WORDS)
  ftkx_block sr_fetch_flag;            // unsigned, device: [0] the number of the last pass whose descriptors have been fetched (series_begin_kernel), [1] its arrival counter
  unsigned sr_fetch_seq = 0;
  hipEvent_t sr_ev_fetched = nullptr;  // slab passes: recorded behind the begin kernel, waited for by the copy of the pass before (no spin-wait there)
  unsigned long long mask_epoch = 0;  // source of Slice::mask_gen values
  double sr_last_running = 0;         // the running minimum the host knew when it last collected a pass (hint of a chained pass)
  ftkxh::tail_policy sr_policy;     // what the passes completed so far say about the form of the next one (series_verdict.hpp)
  int sr_last_buf = 0;               // the buffers of the pass completed last (ftkx_series_dist_status reads its results block)
  size_t sr_last_gathered_off = 0; int sr_last_nranks = 0;   // where its gathered contributions sit in that block (0 ranks: not a slab pass)
  int sr_last_path = 0;              // which way the last ftkx_sweep_series went: 0 the host-driven batch, 1 device-driven (the kernel chain), 2 early single-workgroup tail,
                                     // 4 the one-launch pass, 5 a split pass
  unsigned long long sr_last_status = 0;
  unsigned long long sr_last_order[4] = {0, 0, 0, 0};   // ftkx_debug_series_order: nbins, shift, fullest bucket, rank_max of the pass completed last (zero: not through the bucket chain)
  ftkx_pass2_state p2;
  ftkx_stats stats;
  // optional kernel timing (hipEvents on the context's stream)
  int profiling = 0;               // 0 off, 1 every kernel family, 2 the mask kernel only
  bool ev_open = false;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> events;
  std::vector<hipEvent_t> event_pool;
  double k_ms[ftkxh::K_N] = {0, 0, 0, 0};
  unsigned long long k_launches[ftkxh::K_N] = {0, 0, 0, 0};
  std::string err;
};

namespace ftkx {
// waits for a sequence number a kernel stores, with system scope, into coherent pinned memory (ftkx_api.hip); nullptr or what went wrong
const char *wait_flag(const unsigned *flag, unsigned seq, hipStream_t stream);
}

namespace ftkxh {

int fail(ftkx_ctx *c, int code, const char *fmt, ...);

#define HIP_TRY(c, call)                                                                                   \
  do {                                                                                                     \
    hipError_t e_ = (call);                                                                                \
    if (e_ != hipSuccess) return fail((c), e_ == hipErrorOutOfMemory ? FTKX_E_NOMEM : FTKX_E_DEVICE,       \
                                      "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// what the one-shot calls on device pointers open with
#define DERIVE_PROLOGUE(c) do { if (!(c)) return fail(nullptr, FTKX_E_INVALID, "null context"); HIP_TRY((c), hipSetDevice((c)->device)); } while (0)

// ingest.hip
void temporal_release(ftkx_ctx *c);                             // the temporal ring's arrays back to the pool, the filter as it was constructed
void drop_aux(ftkx_ctx *c, int t);                              // the aux arrays of timestep t leave (parked with the newest open split pass, or to the pool)
int adopt_resident_slice(ftkx_ctx *c, int t, const double *full);   // the library's own borrowing push of an array that has been processed already (slab.cpp)
// ftkx_api.hip
const std::string &global_error();                              // what fail(nullptr, ...) said last on this thread
int settings_not_now(ftkx_ctx *c, const char *who);             // a setting must not change under sweeps pending or series passes open: 0, or fail()'s code
size_t n_vertices(const ftkx_ctx *c);
// the part of the context's mesh and options the samplers read (sample_steps.hpp)
inline ftkx::SampleMesh sample_mesh_of(const ftkx_ctx *c)
{
  ftkx::SampleMesh m;
  m.tag_mode = c->opt.tag_mode;
  m.scalar_mode = c->scalar_mode == 1;
  for (int d = 0; d < 3; d ++) {
    m.dom_lb[d] = (int)c->dom_st[d]; m.dom_sz[d] = (int)c->dom_sz[d];
    m.core_st[d] = (int)c->core_st[d]; m.core_sz[d] = (int)c->core_sz[d];
    m.ext_st[d] = (int)c->ext_st[d]; m.ext_sz[d] = (int)c->ext_sz[d];
  }
  return m;
}
int mask_pitch(const ftkx_ctx *c);
int u_pitch(const ftkx_ctx *c);
size_t u_bytes(const ftkx_ctx *c);
size_t u_bytes_used(const ftkx_ctx *c, const Mesh &m);
size_t mask_bytes(const ftkx_ctx *c);
constexpr size_t kPoolCap = 12;                                 // arrays of a class kept where a slice or a staging array is given back: a batch of steps parked with a split pass comes back at once
void release_slice(Slice &s, ftkx_ctx *c);                      // its arrays back to the context's pool (kPoolCap); `s` is empty afterwards
void free_slice(Slice &s, ftkx_ctx *c);                         // a slice of a live context is dropped: parked with the newest open split pass, or released
void release_retired(ftkx_ctx *c, ftkx_series_pending &P);      // what a pass kept for its tail goes back to the pool: where it completes, where its slot is reused, on abort
int ensure_hit_buffer(ftkx_ctx *c, u64 want);                   // d_hits and set 0's pass array
int ensure_pass(ftkx_ctx *c, ftkx_tail_set &S, u64 want);
int ensure_fragile(ftkx_ctx *c, ftkx_tail_set &S, u64 want);
int ensure_list(ftkx_ctx *c, ftkx_tail_set &S, u64 want);
int ensure_refine(ftkx_ctx *c, ftkx_tail_set &S, u64 want);
int ensure_bins(ftkx_ctx *c, ftkx_tail_set &S, u64 want);       // hist + boff
int ensure_order(ftkx_ctx *c, ftkx_tail_set &S, u64 want);      // bucketed + sorted
hipError_t sync_tails(ftkx_ctx *c);                             // the host waits for whatever is queued on the tail streams
int ensure_desc(ftkx_ctx *c, size_t bytes);
int ensure_red(ftkx_ctx *c, size_t nslices);                    // d_red: 128 words per slice
int ensure_host_buffer(ftkx_ctx *c, size_t want);
void fill_mesh(const ftkx_ctx *c, Mesh &m);
int slice_resolution(ftkx_ctx *c, Slice &s);
bool masks_valid(const ftkx_ctx *c, const Slice &s, u64 factor, bool two_level, int u_rows);   // these two: batch_plan.hpp's, of a slice of this context
double job_big(const ftkx_ctx *c, const Slice &s, u64 factor, bool *rule_on);
int ensure_mask_arrays(ftkx_ctx *c, Slice &s, bool two_level);
int upload_from_host(ftkx_ctx *c, void *dst, const void *src, size_t bytes);       // upload.cpp
int aux_stream_get(ftkx_ctx *c, bool high_priority, hipStream_t *out);       // the library's own streams, kept for the process (ftkx_api.hip)
void aux_stream_put(ftkx_ctx *c, bool high_priority, hipStream_t st);
// trace_device.hip: where the last ftkx_trace_curves_device left its curves on the device (while p2.trace_last_path == 2, until the next trace)
void trace_device_curves(const ftkx_ctx *c, const int **indices, const int **off, const int **loop);
// halo.hip
bool packed_layout(const ftkx_ctx *c, const Mesh &m, size_t *ub, size_t *cap, size_t *off_idx, size_t *off_words, size_t *total);
int ensure_sparse_slice(ftkx_ctx *c, int t, int scalar_input);
// prepare.hip
void launch_init_red(u64 *red, size_t nslots, u64 *counters, hipStream_t st);        // {min = DBL_MAX, max = 0} slots; counters (nullable) zeroed
void launch_fetch_desc(const void *pinned_src, void *device_dst, size_t bytes, hipStream_t st);   // pinned -> device by a kernel (bytes % 8 == 0)
// collect.hip
hipEvent_t ev_take(ftkx_ctx *c);
void ev_give(ftkx_ctx *c, hipEvent_t e);
void ev_begin(ftkx_ctx *c, int kind);
void ev_end(ftkx_ctx *c);
void ev_harvest(ftkx_ctx *c, bool all = true);   // all: after a stream synchronise; otherwise only the pairs that have completed
void ev_drop(ftkx_ctx *c);                       // the pairs of a batch that is replayed: back to the pool, unread
int run_batch(ftkx_ctx *c, const double *sparse_field = nullptr, bool cull_done = false);
int read_counters(ftkx_ctx *c);                  // set 0's CNT_* words into h_counters; waits for the stream
bool ahead_serves_pending(const ftkx_ctx *c, const Mesh &m, bool two_level);
int sort_hits_on_device(ftkx_ctx *c, size_t n, int key_bits);

}  // namespace ftkxh
