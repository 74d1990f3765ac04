/* ftkx -- C ABI of the MI355X-native critical-point space-time simplex sweep.
 *
 * This is the drop-in boundary for ONE hot path of hguo/ftk: the per-timestep sweep of
 *   ftk::critical_point_tracker_2d_regular::update_timestep()   include/ftk/filters/critical_point_tracker_2d_regular.hh:263-433
 *   ftk::critical_point_tracker_3d_regular::update_timestep()   include/ftk/filters/critical_point_tracker_3d_regular.hh:150-308
 * i.e. what the reference hands to its accelerator back-ends through
 *   extract_cp2dt_cuda / extract_cp2dt_sycl   critical_point_tracker_2d_regular.hh:33-63  (call sites 369-384, 399-414)
 *   extract_cp3dt_cuda                        critical_point_tracker_3d_regular.hh:42-56  (call sites 248-260, 274-286)
 * Results follow the reference's CPU path (check_simplex, 2d:584-685, 3d:425-514), not its CUDA/SYCL kernels
 * (those use a different domain and quantisation).
 *
 * Plain C: opaque context, raw pointers and sizes, integer status codes.  No STL, no torch types.  All entry points
 * return FTKX_OK (0) or a negative FTKX_E_* code and never call exit(); ftkx_last_error() gives the message.
 * (The reference's own boundary returns nothing and prints CUDA errors: src/filters/utils.cuh:13-22.)
 *
 * Array layouts are the reference's ndarray layouts (first index fastest, include/ftk/ndarray.hh:103-117):
 *   V[c + nd*(x + DW*(y + DH*z))]            vector field, nd components
 *   J[k + nd*j + nd*nd*(x + DW*(y + DH*z))]  jacobian; the tracker reads Js[j][k] = J(k, j, ...)  (2d:566-582, 3d:405-422)
 *   S[x + DW*(y + DH*z)]                     scalar
 * Resident arrays are FP64.  A caller's array is FP64 too unless the entry says otherwise: the *_f32 entries take float32, the *_typed
 * entries take any element type of FTKX_DTYPE_* -- FP64, float32, IEEE half, bfloat16, 8- / 16- / 32-bit integers -- as it is, at its own
 * bytes per value over the link, and widen it to FP64 on the device, exactly (ndarray<T>::from_array<T1>, include/ftk/ndarray.hh:401-410).
 */
#ifndef FTKX_H
#define FTKX_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* == ftk::feature_point_lite_t (include/ftk/features/feature_point_lite.hh:8-15), 72 bytes */
typedef struct ftkx_cp_t {
  double x[3];              /* lattice coordinates (REGULAR_COORDS_SIMPLE); 2D: x[2] = 0 */
  double t;
  double scalar[3];         /* scalar[0] filled iff a scalar field was given (FTK_CP_MAX_NUM_VARS = 3); [1], [2]: 0 unless ftkx_sample_aux or an armed series pass (ftkx_set_series_sampling) filled them */
  unsigned int type;        /* include/ftk/numeric/critical_point_type.hh:10-36 */
  unsigned long long tag;   /* see ftkx_options.tag_mode */
} ftkx_cp_t;

/* The 4 padding bytes between `type` and `tag` (offset 60; feature_point_lite_t has the same hole) carry what the caller
 * of the reference boundary otherwise has to remember per call (2d:387-395): bit 0 = the simplex type is ordinal,
 * bits 1..31 = current_timestep of the sweep that emitted the record.  Consumers that ignore padding are unaffected. */
static inline unsigned int ftkx_cp_aux(const ftkx_cp_t *cp) { return ((const unsigned int *)cp)[15]; }
static inline int ftkx_cp_ordinal(const ftkx_cp_t *cp) { return (int)(ftkx_cp_aux(cp) & 1u); }
static inline int ftkx_cp_timestep(const ftkx_cp_t *cp) { return (int)(ftkx_cp_aux(cp) >> 1); }

typedef struct ftkx_ctx ftkx_ctx;

enum {
  FTKX_OK = 0,
  FTKX_E_INVALID = -1,      /* bad argument / call order */
  FTKX_E_DEVICE = -2,       /* HIP runtime error */
  FTKX_E_NOMEM = -3,
  FTKX_E_NOSLICE = -4,      /* sweep of a timestep whose slice is not resident */
  FTKX_E_UNSUPPORTED = -5
};

/* ELEMENT_SCOPE_* of include/ftk/mesh/simplicial_regular_mesh.hh:39-43; BOTH = one launch doing both sweeps of a step */
enum { FTKX_SCOPE_ORDINAL = 1, FTKX_SCOPE_INTERVAL = 2, FTKX_SCOPE_BOTH = 3 };

enum {
  FTKX_TAG_WORK_INDEX = 0,  /* index inside `core` for the given scope: what extract_cp*dt_cuda returns (src/filters/critical_point_tracer_2d_regular.cu:162-164).
                               FTKX_SCOPE_BOTH: ftkx_sweep_series only; every record counts inside its OWN scope (ftkx_cp_ordinal says which),
                               so tags of the two scopes may coincide and the records come in element order, not in tag order */
  FTKX_TAG_REFERENCE  = 1,  /* e.to_integer(m) bit-for-bit, including its int32 products (simplicial_regular_mesh.hh:496-502) */
  FTKX_TAG_EXACT64    = 2   /* same formula in 64-bit arithmetic: equal to REFERENCE whenever that does not overflow */
};

typedef struct ftkx_options {
  int jacobian_symmetric;   /* is_jacobian_field_symmetric (critical_point_tracker.hh:176) */
  int robust;               /* enable_robust_detection, 3D only (3d:439-467); 2D always runs the robust test (2d:618-622) */
  int use_type_filter;      /* 2D only (2d:280) */
  unsigned int type_filter;
  int compute_degrees;      /* enable_computing_degrees, 2D only (2d:653-662) */
  int tag_mode;             /* FTKX_TAG_* */
  int exact_only;           /* 1: never apply the sign cull (every simplex gets the full integer test) */
  int derive_jacobian;      /* 1: when a slice has no J, derive it at hit vertices from V exactly like ndarray/grad.hh
                               jacobian2D/3D would (jacobian_field_source == SOURCE_DERIVED); 0: treat J as absent (zeros) */
  int coords_mode;          /* REGULAR_COORDS_* (regular_tracker.hh:12-17; simplex_coordinates 2d:494-527, 3d:342-378):
                               0 SIMPLE (lattice integers), 1 BOUNDS (coords_bounds below), 2 RECTILINEAR and 3 EXPLICIT --
                               the last two are selected by ftkx_set_coords_rectilinear / ftkx_set_coords_explicit, which
                               also carry the arrays */
  double coords_bounds[6];  /* x0,x1,y0,y1[,z0,z1] */
} ftkx_options;

/* ---- context ------------------------------------------------------------------------------------------------- */
int  ftkx_create(ftkx_ctx **ctx, int nd /*2|3*/, int device_id);
void ftkx_destroy(ftkx_ctx *ctx);
int  ftkx_last_error(const ftkx_ctx *ctx, char *buf, size_t n);   /* ctx may be NULL: last error of the calling thread */
int  ftkx_set_stream(ftkx_ctx *ctx, void *hip_stream);            /* NULL = the context's own stream */
int  ftkx_set_options(ftkx_ctx *ctx, const ftkx_options *opt);
void ftkx_default_options(ftkx_options *opt);

/* mesh: `domain` = vertex validity box == tracker `domain` (regular_tracker.hh:116-124; inclusive upper bound st+sz-1,
 * time is [0, INT_MAX]); `core` = corners to enumerate == local_domain; `ext` = array lattice == local_array_domain. */
int ftkx_set_mesh(ftkx_ctx *ctx, const long long domain_st[3], const long long domain_sz[3],
                  const long long core_st[3], const long long core_sz[3],
                  const long long ext_st[3], const long long ext_sz[3]);
/* regular_tracker::set_coords_rectilinear / set_coords_explicit (regular_tracker.hh:39-40).  Host arrays, copied to the device;
 * they replace opt.coords_mode.  Rectilinear: one array per spatial axis, indexed by the vertex coordinate (so n_d must cover the
 * array lattice).  Explicit: ndarray (ncomp, n0, n1) with the first index fastest, read as coords[c + ncomp * (x + n0 * y)];
 * ncomp >= 2 (2D; a third component becomes x[2]) or 3 (3D -- where the reference reads only this z = 0 plane and reports the
 * vertex's z index as its time; reproduced).  ftkx_set_options with coords_mode 0 or 1 switches back. */
int ftkx_set_coords_rectilinear(ftkx_ctx *ctx, const double *x, size_t nx, const double *y, size_t ny, const double *z, size_t nz);
int ftkx_set_coords_explicit(ftkx_ctx *ctx, const double *coords, int ncomp, size_t n0, size_t n1);

/* ---- slices resident in HBM (== field_data_snapshots, critical_point_tracker.hh:155-159) --------------------- */
/* V required; J, S nullable.  on_device = 0: host pointers, copied to the device; 1: device pointers (of this context's device),
 * adopted without a copy and owned by the caller until ftkx_drop_slice(); 2: device pointers of any device, copied (peer copy).
 * Host arrays are in HBM when the call returns (the caller may reuse or free them); pageable ones of 32 MiB and more are staged by a few
 * threads the call starts and joins (FTKX_UPLOAD_THREADS, default 4; 0: the runtime's own copy), pinned ones go by DMA as they are. */
int ftkx_push_slice(ftkx_ctx *ctx, int t, const double *V, const double *J, const double *S, int on_device);
/* scalar input (vector_field_source == SOURCE_DERIVED, 2d:238-250, 3d:125-137): uploads S and derives V = gradient2D/3D(S)
 * on the device bit-for-bit like ndarray/grad.hh.  With options.derive_jacobian the Jacobian at hit vertices is the one
 * jacobian2D<T, true> / jacobian3D would give for that V. */
int ftkx_push_scalar_slice(ftkx_ctx *ctx, int t, const double *S, int on_device);
int ftkx_drop_slice(ftkx_ctx *ctx, int t);
/* ndarray::resolution() of the slice's V (ndarray.hh:770-778): min |v| over non-zero entries (DBL_MAX if none);
 * max_abs (nullable) = max finite |v|, used for the no-overflow guard of the cull. */
int ftkx_slice_resolution(ftkx_ctx *ctx, int t, double *resolution, double *max_abs);
/* A slice received from another GPU (t-slab halo) comes with the reduction its owner already did: hand it over instead of
 * reducing the slice again. */
/* ftkx_slice_resolution for n resident slices with one launch and one synchronise; res / max_abs: n doubles each (nullable) */
int ftkx_slices_resolution(ftkx_ctx *ctx, const int *timesteps, int n, double *res, double *max_abs);
int ftkx_set_slice_resolution(ftkx_ctx *ctx, int t, double resolution, double max_abs);
/* The ONE-PASS form of the pre-pass (what the tracker and bench.py use): a single kernel reads each slice once and produces
 * both the vertex sign masks of the sweep and the reduction update_vector_field_scaling_factor needs, so a slice is read from
 * HBM once per sweep instead of twice.  The masks are built under `factor_hint`, a power of two that must not exceed the factor
 * the sweeps will be given (0 = 256, the smallest factor there is; a streaming caller passes the factor in force before these
 * slices arrived: the reference's factor is a sticky running minimum and only grows).  Masks built under a smaller factor only
 * ever cull less, never wrongly; ftkx_sweep rebuilds them by itself in the one case that is not covered (a larger factor
 * under which the slice has vertices that could overflow a determinant).
 *   res_below[i] = smallest non-zero |v| of slice i that is < 1 / factor_hint, DBL_MAX if there is none.  That is all the scaling
 *                  factor needs: running = min(running, res_below[i]) gives the same nbits = clamp(ceil(log2(1 / running)), 8, 21)
 *                  as the running minimum of ndarray::resolution() (a value >= 1 / factor_hint cannot raise nbits past log2 hint).
 *   max_abs[i]   = max finite |v| (both nullable). */
int ftkx_slices_prepare(ftkx_ctx *ctx, const int *timesteps, int n, unsigned long long factor_hint, double *res_below, double *max_abs);
/* Cull-ahead (optional): the sweeps that will be enqueued after the NEXT ftkx_slices_prepare, in that order.  That call then queues
 * their cull right behind the mask kernel -- the cull needs the masks and the list of steps, not the factor -- so it runs while the
 * host still waits for the reduction and forms the factors (update_vector_field_scaling_factor, critical_point_tracker.hh:850-864).
 * A hint, never an obligation: ftkx_sweep_collect takes the survivor list over only if the pending sweeps are exactly the announced
 * ones and every mask serves its sweep's factor; otherwise, and after any call that touches slices or masks, it culls as usual. */
int ftkx_sweep_announce(ftkx_ctx *ctx, const int *timesteps, const int *scopes, int n);
/* update_vector_field_scaling_factor (critical_point_tracker.hh:850-864): nbits = clamp(ceil(log2(1/res)), 8, 21) */
unsigned long long ftkx_scaling_factor(double resolution, int *nbits);

/* ---- compact t-slab halo (multi-GPU, one process per GPU: DESIGN.md 6) ------------------------------------------------------
 * A rank's last interval sweep [t-1, t] reads the first slice of the NEXT rank's slab.  Instead of that slice (1 GiB for 512^3) its
 * owner can hand over what the sweep really uses of it: the sign masks -- factor-free since round 2: the summary array as it is
 * plus the compacted mask words the summaries do not describe -- and, after the receiver's cull, the input values around the few
 * cells that survived there (6^nd vertices per cell: corner - 2 .. corner + 3 on every axis).
 *   owner:     ftkx_slices_prepare(t) ... ftkx_export_masks_size(t) -> sizes; ftkx_export_masks(t) -> buffers to send
 *   receiver:  ftkx_push_masked_slice(t, ...); ftkx_sweep_enqueue(...) as usual; ftkx_sweep_cull(t) -> n cells;
 *              ftkx_get_sparse_cells -> send to the owner
 *   owner:     ftkx_gather_patches(t, cells) -> send back          receiver: ftkx_scatter_patches(t, cells, patches); ftkx_sweep_collect
 * `*_on_device` = 1: the caller's buffers are device memory of this context's device; 0: host memory.
 * Limits: meshes whose masks carry summaries (even row length multiple of 8, slices < 4 GiB) and sweeps that use the cull; a masked
 * slice whose masks cannot serve the factor of the sweep (FTKX_E_NOSLICE) or any other limit (FTKX_E_UNSUPPORTED) means: send the
 * slice itself (ftkx_push_scalar_slice). */
int ftkx_export_masks_size(ftkx_ctx *ctx, int t, size_t *u_bytes, size_t *n_words, unsigned long long *mask_factor, double *max_abs);
int ftkx_export_masks(ftkx_ctx *ctx, int t, void *U_dst, unsigned *word_index_dst, unsigned long long *words_dst, int dst_on_device);
/* (u_bytes: the size of the summary array as the SENDER exported it; it must equal this context's -- same extents, same mask settings) */
int ftkx_push_masked_slice(ftkx_ctx *ctx, int t, int scalar_input, const void *U, size_t u_bytes, const unsigned *word_index, const unsigned long long *words, size_t n_words,
                           unsigned long long mask_factor, double max_abs, int on_device);
/* The same hand-over as ONE message of a size both sides know from the mesh alone (ftkx_packed_masks_bytes: 32-byte header, the summary
 * array, a capacity-bounded list of mask words).  The owner's export is queued on its stream and the receiver's import reads the header
 * -- word count, geometry -- ON THE DEVICE: neither side waits on the host for the other's numbers.  A message that did not fit (more
 * words than its capacity, another geometry, an index outside the mask array) is found by ftkx_sweep_cull: FTKX_E_NOSLICE, send the
 * slice itself.  mask_factor / max_abs: what the owner prepared the slice under (the factor hint) and its max |v| (it is part of the
 * all_gather of the reductions every rank takes part in anyway). */
size_t ftkx_packed_masks_bytes(const ftkx_ctx *ctx, size_t *word_capacity);
int ftkx_export_masks_packed(ftkx_ctx *ctx, int t, void *dst, int dst_on_device);
int ftkx_push_masked_slice_packed(ftkx_ctx *ctx, int t, int scalar_input, const void *src, int src_on_device, unsigned long long mask_factor, double max_abs);
int ftkx_sweep_cull(ftkx_ctx *ctx, int t_masked, size_t *n_cells);
int ftkx_get_sparse_cells(ftkx_ctx *ctx, unsigned long long *dst, int dst_on_device);
size_t ftkx_patch_doubles(const ftkx_ctx *ctx);      /* doubles per cell in a patch buffer */
int ftkx_gather_patches(ftkx_ctx *ctx, int t, const unsigned long long *cells, size_t n, double *patches, int on_device);
int ftkx_scatter_patches(ftkx_ctx *ctx, int t, const unsigned long long *cells, size_t n, const double *patches, int on_device);

/* ---- the sweep ------------------------------------------------------------------------------------------------- */
/* Sweeps the simplices of `scope` whose corner lies in `core` at time t (interval: [t, t+1], needs slice t+1).
 * `factor` = vector_field_scaling_factor: any non-zero value is honoured (quantisation is trunc(v * factor) like 2d:605-616), but the
 * sign cull that makes the sweep memory-bound needs a power of two <= 2^53 (what update_vector_field_scaling_factor produces);
 * other factors run the full integer test on every simplex.  Records are returned in a context-owned pinned host buffer, sorted by tag,
 * valid until the next call on this context.  Synchronous on the context's stream.
 * Everything in a record is computed on the device; the one exception is the TYPE of a 3D record whose Hessian has an eigenvalue
 * that is zero up to rounding (plateaus, lattice-aligned data): the kernels flag it and hand its Jacobian over, and the class is
 * computed here, with the host's pow / acos / cos -- the libm the reference's eigen_solver3.hh:20-47 runs on, whose last-place
 * rounding is what such a class hangs on (ftkx_stats.reclassified counts them). */
int ftkx_sweep(ftkx_ctx *ctx, int t, int scope, unsigned long long factor, const ftkx_cp_t **out, size_t *n_out);

/* batched form: enqueue only records the request; ftkx_sweep_collect() launches the whole batch (one mask / cull / exact
 * launch covers every enqueued timestep), synchronises and returns the records of ALL of them (sorted by tag). */
int ftkx_sweep_enqueue(ftkx_ctx *ctx, int t, int scope, unsigned long long factor);
int ftkx_sweep_enqueue_many(ftkx_ctx *ctx, const int *timesteps, const int *scopes, const unsigned long long *factors, int n);   /* all or nothing */
int ftkx_sweep_collect(ftkx_ctx *ctx, const ftkx_cp_t **out, size_t *n_out);
int ftkx_sweep_cancel(ftkx_ctx *ctx);    /* forgets the enqueued, not yet collected sweeps */

/* The device-driven pass over a series of resident slices -- what the tracker and bench.py use; the calls above remain for callers
 * that form the factors themselves (several ranks: ftk_amd/tslab.py).  Sweeps the steps (timesteps[i], scopes[i]), timesteps strictly
 * ascending, each under the reference's sticky factor (update_vector_field_scaling_factor, critical_point_tracker.hh:850-864):
 *   factor(i) = scaling_factor(min(*running_resolution, resolution of every slice the steps read with timestep <= timesteps[i] + 1))
 * with the running minimum and nbits formed ON THE DEVICE between the mask kernel and the exact test: the whole pass -- masks and
 * reduction, cull, factors, exact test, records, their ordering by tag and their transfer into the pinned host buffer -- is queued at
 * once and the host waits once.  *running_resolution: in = the minimum before these slices (DBL_MAX: none), out = the minimum after
 * them (as exact as ftkx_slices_prepare's res_below makes it: exact once it is below 2^-8).  factors (nullable): n values out.
 * Whatever the device-driven form does not cover (options that need the tile path, a type filter, wrapped reference tags, a factor that
 * hangs on the last bit of the host's log2, slices with vertices that can overflow a determinant, ...) is swept by the calls above
 * inside this one, with the same result.  Records as for ftkx_sweep_collect: sorted by tag, valid until the next call. */
int ftkx_sweep_series(ftkx_ctx *ctx, const int *timesteps, const int *scopes, int n, double *running_resolution,
                      unsigned long long *factors, const ftkx_cp_t **out, size_t *n_out);
/* The same pass in two halves, for callers that keep the device busy across passes (a streaming tracker, bench.py): _submit queues a
 * pass and returns; _complete waits for the OLDEST open pass and returns what ftkx_sweep_series returns.  At most three passes are open at
 * a time; two keep the device busy -- submit(N), submit(N + 1), complete(N), submit(N + 2), complete(N + 1), ... --, the third lets the
 * host run one pass ahead of a split pass's tail (ftkx_series_last_path = 5), which ends behind the mask kernel of the pass after it
 * (slab passes, ftkx_series_dist_*: two).  While pass N + 1's mask kernel runs, the host
 * collects pass N, and the records of a pass with many of them cross PCIe on a copy engine instead of holding the stream.
 * running_resolution of _submit: the running minimum before this pass, or NULL = continue from the pass queued before it, still open
 * (the minimum is handed on ON THE DEVICE; _complete then reports the chained value).  Between _submit and _complete only slices may be
 * pushed or dropped and further passes submitted; the sweeps above and ftkx_slices_prepare fail until every open pass is complete.
 * Records of a pass: valid until the next _submit OR the next _complete (or any other sweep call) after its own _complete -- a pass that
 * the host-driven batch had to sweep returns the context's shared host buffer, which the next such completion overwrites; a device-driven
 * pass's buffers are taken over by the second _submit after it.  Copy what must live longer.  Results are those of ftkx_sweep_series on
 * the same steps: tests/test_gpu_series.py::test_pipelined_passes_equal_the_plain_ones.
 * _abort: after a failed _submit / _complete (or to give up): waits for whatever the open passes queued, discards them and leaves the
 * context as if no pass had been submitted (masks they were building are rebuilt by the next sweep); FTKX_OK with nothing open. */
int ftkx_sweep_series_submit(ftkx_ctx *ctx, const int *timesteps, const int *scopes, int n, const double *running_resolution);
int ftkx_sweep_series_complete(ftkx_ctx *ctx, double *running_resolution, unsigned long long *factors, const ftkx_cp_t **out, size_t *n_out);
int ftkx_sweep_series_abort(ftkx_ctx *ctx);
/* ---- the slab pass: the device-driven pass of ONE RANK of a series cut into timestep slabs (one process per GPU) ----------
 * The reference's sticky factor (critical_point_tracker.hh:850-864) runs over ALL slices in time order and rank r's last interval sweep
 * reads the first slice of rank r + 1.  Both links are small and both are closed ON THE DEVICE: the pass is queued in four stages, and
 * between them the caller queues its collectives on the context's stream (RCCL: ncclAllGather / ncclSend / ncclRecv, or
 * torch.distributed with that stream current) -- nothing is waited for on the host until ftkx_sweep_series_complete:
 *   _begin   masks + reduction of this rank's slices; `contrib` (4 doubles: min resolution and max |v| of the slab, and of its FIRST slice)
 *            and, with masks_out, the first slice's sign masks as one message of ftkx_packed_masks_bytes() bytes -- built and packed FIRST:
 *            with a side_stream, that stream is made to wait for the message only, so a send queued on it crosses xGMI while the masks
 *            of the slab's other slices are still being built (the caller makes the context's stream wait for the side stream's receive
 *            before _cull)
 *      caller: all_gather(contrib -> gathered, 4 doubles per rank); masks_out -> lower neighbour, upper neighbour's -> masks_in
 *   _cull    the halo's masks imported, the running minimum before this slab from `gathered`, cull + factors, and `request_out`:
 *            1 + ftkx_series_dist_cells() words -- the count of surviving cells whose exact test reads the halo slice and their indices
 *            (-1: send the slice itself)
 *      caller: request_out -> upper neighbour, lower neighbour's -> request_in
 *   _serve   the patches around the lower neighbour's cells, gathered from this rank's first slice into `reply_out`:
 *            ftkx_series_dist_cells() * ftkx_patch_doubles() doubles, a FIXED size (the count is read on the device)
 *      caller: reply_out -> lower neighbour, upper neighbour's -> reply_in
 *   _finish  patches scattered into the halo slice; exact test, records, finish.  The pass is open: ftkx_sweep_series_complete as usual
 * All buffers are device memory of this context's device and must stay untouched until the pass is complete; ranks without a lower /
 * upper neighbour pass NULL for the corresponding buffers (upper = -1: the last step's slices are all this rank's own; with more ranks than
 * timesteps the neighbours are the nearest ranks that own timesteps, not rank - 1 / rank + 1).  Two slab passes
 * may be in flight like any two passes (separate buffers each).  ftkx_sweep_series_complete returns FTKX_E_NOSLICE when the request said
 * -1 (nothing was swept: fetch the slice itself, push it, and sweep with ftkx_sweep_series from the running minimum
 * ftkx_series_dist_status reports); the owner learns the same from `served` = -1.  Options the device-driven pass does not cover:
 * FTKX_E_UNSUPPORTED from _begin (same on every rank: they share options and mesh) -- use ftkx_slices_prepare / ftkx_sweep_enqueue /
 * ftkx_sweep_cull / ftkx_sweep_collect. */
size_t ftkx_series_dist_cells(const ftkx_ctx *ctx);
int ftkx_series_dist_begin(ftkx_ctx *ctx, const int *timesteps, const int *scopes, int n, const double *running_resolution, int rank, int nranks,
                           int upper /* the rank that owns the slice behind this slab, -1: none (every slice the steps read is this rank's own) */,
                           void *contrib, const void *gathered, void *masks_out, void *side_stream /* hipStream_t, nullable */);
int ftkx_series_dist_cull(ftkx_ctx *ctx, const void *masks_in, void *request_out);
int ftkx_series_dist_serve(ftkx_ctx *ctx, const void *request_in, void *reply_out);
int ftkx_series_dist_finish(ftkx_ctx *ctx, const void *reply_in);
/* of the slab pass completed last: what it asked its upper neighbour for and what its lower neighbour asked of it (cells, -1: the whole
 * slice, 0: nothing), and the gathered contributions (4 * nranks doubles, nullable) */
int ftkx_series_dist_status(const ftkx_ctx *ctx, long long *asked, long long *served, double *gathered, int nranks);

/* which way the last ftkx_sweep_series went: 1 = device-driven (the kernel chain), 2 = device-driven and finished by the fused tail
 * kernel (sparse data), 4 = the whole pass in one launch (small series), 5 = split: the kernel chain on a stream of its own next to the
 * mask kernel of the pass queued behind (pipelined passes over sparse data whose mask kernel is long enough to hide it), 0 = host-driven
 * batch; *status (nullable) = the SERIES_* bits the kernels raised (csrc/sweep_params.hpp) */
int ftkx_series_last_path(const ftkx_ctx *ctx, unsigned long long *status);

/* The split pass (path 5) is taken where a pass's mask launch is long enough to hide its tail (sparse data: 1 GB and more; hit-dense data:
 * 4 GB and more) AND -- in the default setting, "auto" -- the context's own measurement found it no slower: the first qualifying passes of
 * a shape run five in order, five split, the host's time between completions is sampled, and the split pass is kept unless it was more
 * than 2 % slower (how two queues share the device is the hardware's business; GPU_MAX_HW_QUEUES alone can turn it).  Deterministic
 * settings: FTKX_SERIES_HOOKS="split=4" (the size rule alone) / "split=0" (never).  This call says which way the context went:
 * *state 0 auto, still measuring; 1 auto, split; 2 auto, in order; 3 forced on; 4 forced off; medians in ms per pass (0: none taken). */
int ftkx_series_split_decision(const ftkx_ctx *ctx, int *state, double *median_in_order_ms, double *median_split_ms);

/* counters of the last collect: simplices visited (work items), cells/simplices surviving the cull, device-side hits */
typedef struct ftkx_stats {
  unsigned long long work_items, cells, cells_survived, simplices_tested, hits;
  int cull_enabled;
  unsigned long long reclassified;   /* 3D records whose Hessian has an eigenvalue that is zero up to rounding: their class was computed
                                        on the host, with the host's libm (the device library's pow / acos / cos differ from it in the
                                        last place, which is all such a class hangs on) */
} ftkx_stats;
int ftkx_get_stats(const ftkx_ctx *ctx, ftkx_stats *st);

/* The vertex sign masks a sweep builds for a slice are kept with the slice (slice t+1 of step t is slice t of step t+1).
 * A caller that rewrites a slice's device memory in place, or a benchmark that must redo all work, drops them with this. */
int ftkx_invalidate_masks(ftkx_ctx *ctx);

/* optional kernel timing with HIP events on the context's stream (for bench.py's roofline figure).  Index: 0 mask_kernel,
 * 1 cull_kernel, 2 exact_kernel (+ everything behind it: the FP64 half of the records, their ordering), 3 tile_kernel (the integer test of
 * every simplex: exact_only, the overflow regime); ms[] = summed device time, launches[] = launches timed since set_profiling(1). */
int ftkx_set_profiling(ftkx_ctx *ctx, int on);      /* 0 off, 1 every kernel family, 2 the mask kernel only (an event pair costs the stream a few us) */
int ftkx_get_kernel_times(const ftkx_ctx *ctx, double ms[4], unsigned long long launches[4]);

/* ---- stateless one-shot calls with the reference boundary's argument list ------------------------------------ */
/* extract_cp2dt_{cuda,sycl}(scope, current_timestep, domain, core, ext, Vc, Vn, Jc, Jn, Sc, Sn, use_explicit_coords, coords)
 * critical_point_tracker_2d_regular.hh:33-63.  Lattices are passed as (start, size) triples; host pointers; the records
 * are malloc'd into *out (release with ftkx_free).  tag = work index inside `core` unless opt->tag_mode says otherwise. */
int ftkx_extract_cp2dt(int scope, int current_timestep,
                       const long long domain_st[3], const long long domain_sz[3],
                       const long long core_st[3], const long long core_sz[3],
                       const long long ext_st[2], const long long ext_sz[2],
                       const double *Vc, const double *Vn, const double *Jc, const double *Jn,
                       const double *Sc, const double *Sn, int use_explicit_coords, const double *coords,
                       unsigned long long factor, const ftkx_options *opt, int device_id,
                       ftkx_cp_t **out, size_t *n_out);
/* extract_cp3dt_cuda(scope, current_timestep, domain4, core4, ext3, Vc, Vl, Jc, Jl, Sc, Sl)  critical_point_tracker_3d_regular.hh:42-56 */
int ftkx_extract_cp3dt(int scope, int current_timestep,
                       const long long domain_st[4], const long long domain_sz[4],
                       const long long core_st[4], const long long core_sz[4],
                       const long long ext_st[3], const long long ext_sz[3],
                       const double *Vc, const double *Vn, const double *Jc, const double *Jn,
                       const double *Sc, const double *Sn,
                       unsigned long long factor, const ftkx_options *opt, int device_id,
                       ftkx_cp_t **out, size_t *n_out);
void ftkx_free(void *p);

/* ---- pass 2 on the hit set: records -> traced curves (host side, like the reference's) --------------------------------
 * Replaces critical_point_tracker::trace_critical_points_offline (include/ftk/filters/critical_point_tracker.hh:668-817) with
 * the neighbourhood of critical_point_tracker_2d_regular.hh:189-197 and geometry/cc2curves.hh:10-122: two hits are neighbours
 * iff their simplices share a (d+1)-cell; hits with more than two neighbours are dropped; every connected component of the rest
 * is one curve whose points come in the reference's order.  `recs[i].tag` must be element tags (FTKX_TAG_EXACT64, or
 * FTKX_TAG_REFERENCE where that did not overflow) of the mesh whose spatial box is (domain_st, domain_sz). */
typedef struct ftkx_curves {
  size_t n_curves, n_points, n_special;   /* n_special: hits dropped for having more than two neighbours */
  long long *offsets;                     /* n_curves + 1 */
  long long *indices;                     /* n_points indices into recs[], curve after curve */
  int *loop;                              /* n_curves: first and last point are neighbours */
} ftkx_curves;
int  ftkx_trace_curves(int nd, const long long domain_st[3], const long long domain_sz[3], const ftkx_cp_t *recs, size_t n, ftkx_curves *out);
void ftkx_free_curves(ftkx_curves *c);
/* The same, with the two phases that are independent per record -- the neighbour search and the component labelling -- on the context's
 * GPU (tags up, neighbours and component roots down; what is serial per curve stays on host threads): identical curves.  Record sets
 * below 4 096 records, or whose tags do not come strictly ascending, take ftkx_trace_curves as it is; ctx == NULL likewise. */
int  ftkx_trace_curves_ctx(ftkx_ctx *ctx, int nd, const long long domain_st[3], const long long domain_sz[3], const ftkx_cp_t *recs, size_t n, ftkx_curves *out);
/* the same on the tags alone (8 bytes per record): a caller that holds its points in another form need not build records around them */
int  ftkx_trace_curves_tags_ctx(ftkx_ctx *ctx, int nd, const long long domain_st[3], const long long domain_sz[3], const unsigned long long *tags, size_t n, ftkx_curves *out);
/* pass 2 with nothing but the result crossing back: neighbour search, component labelling, seeds, walks and compaction on the
 * context's GPU.  tags: n strictly ascending element tags; tags_on_device = 1: a device pointer of this context's device.
 * Curves identical to ftkx_trace_curves.  Any n >= 0 (no size floor).  Sets that the device form does not cover (tags not strictly
 * ascending, n >= 2^30, a timestep >= 2^24 or a mesh whose order key does not fit 64 bits) are traced by ftkx_trace_curves_tags_ctx
 * inside this call, with the same result. */
int  ftkx_trace_curves_device(ftkx_ctx *ctx, int nd, const long long domain_st[3], const long long domain_sz[3],
                              const unsigned long long *tags, size_t n, int tags_on_device, ftkx_curves *out);
/* which way the last trace on this context went: 0 host, 1 device phases + host walks (ftkx_trace_curves_ctx), 2 all on the device */
int  ftkx_trace_last_path(const ftkx_ctx *ctx);

/* enable_streaming_trajectories (critical_point_tracker.hh:38; update_timestep 2d:326-330, 3d:197-201): trajectories that grow while
 * the sweep streams -- trace_critical_points_online (critical_point_tracker.hh:523-639).  After every interval sweep the caller hands
 * over the discrete points found since the last call (they are consumed); open trajectories are continued greedily through the
 * new points, the rest starts new trajectories.  ftkx_online_tracer_curves copies the trajectories out: *points (malloc'ed, release
 * with ftkx_free) holds them one after the other, `out` the offsets / loop flags (indices = 0 .. n_points-1). */
typedef struct ftkx_online_tracer ftkx_online_tracer;
int  ftkx_online_tracer_create(ftkx_online_tracer **out, int nd, const long long domain_st[3], const long long domain_sz[3]);
void ftkx_online_tracer_destroy(ftkx_online_tracer *);
int  ftkx_online_tracer_grow(ftkx_online_tracer *, const ftkx_cp_t *recs, size_t n);
int  ftkx_online_tracer_curves(const ftkx_online_tracer *, ftkx_cp_t **points, ftkx_curves *out);

/* Trajectory post-processing with the defaults of json_interface::post_process (include/ftk/filters/json_interface.hh:758-800):
 * smooth_ordinal_types / smooth_interval_types / rotate, split_all, reorder / adjust_time (features/feature_curve.hh:220-348,
 * features/feature_curve_set.hh:514-532).  recs[] must carry the aux word (ordinal, timestep) the sweep writes.  Per point the
 * smoothed type and adjusted time come back next to the index into recs[]. */
typedef struct ftkx_trajectories {
  size_t n_curves, n_points;
  long long *offsets;
  long long *indices;
  int *loop;
  unsigned int *type;
  double *t;
  int *id;                                /* n_curves: label of the curve in the reference's multimap = index of the traced curve
                                             it came from (split pieces share their parent's label, feature_curve_set.hh:530-531) */
} ftkx_trajectories;
int  ftkx_post_process_curves(const ftkx_cp_t *recs, size_t n, const ftkx_curves *in, ftkx_trajectories *out);
void ftkx_free_trajectories(ftkx_trajectories *c);
/* ftkx_post_process_curves on the context's GPU: the same trajectories, field for field (t bit for bit: the only floating-point
 * operations are max and min).  Every step is a map or a scan over the flat array of points, whatever the curves' lengths.  Per record
 * 16 bytes go up (type, aux word, t), per point 4 and per curve 8; offsets, indices, loop, type, t and id come down once.  What the
 * device form does not cover -- n_points >= 2^30, or a point whose t is not finite (max and min as the host code calls them are not
 * associative with NaN) -- is done by ftkx_post_process_curves inside this call, with the same result.  Argument errors as the host
 * function's (an index outside recs[], offsets that do not ascend or run past n_points: FTKX_E_INVALID); ctx == NULL: FTKX_E_INVALID. */
int  ftkx_post_process_curves_device(ftkx_ctx *ctx, const ftkx_cp_t *recs, size_t n, const ftkx_curves *in, ftkx_trajectories *out);
/* pass 2 in one call: ftkx_trace_curves_device on the records' tags, then the above on the curves where they lie on the device (indices,
 * offsets and loop flags are not sent up again); curves (nullable): the traced curves as well, released with ftkx_free_curves.  A trace
 * that did not go all the way on the device is post-processed by ftkx_post_process_curves, with the same result. */
int  ftkx_pass2_device(ftkx_ctx *ctx, int nd, const long long domain_st[3], const long long domain_sz[3],
                       const ftkx_cp_t *recs, size_t n, ftkx_curves *curves, ftkx_trajectories *out);
/* which way the last post-processing on this context went: 0 host, 2 all on the device */
int  ftkx_post_process_last_path(const ftkx_ctx *ctx);

/* ---- record-stream formats: what `ftk --output-type discrete|traced` writes and reads -------- */
/* binary = diy::serializeToFile, byte-identical to the reference's files; json = nlohmann's compact dump (parses to the
 * same values); text = the ostream print-outs.  Host only.  Errors: ftkx_last_error(NULL, ...). */
enum { FTKX_FORMAT_BINARY = 0, FTKX_FORMAT_JSON = 1, FTKX_FORMAT_TEXT = 2 };
int ftkx_format_from_path(const char *path);     /* "...txt" text, "...json" json, else binary (filters/json_interface.hh:225-231) */
/* critical_point_tracker::write_critical_points_{json,binary,text} (filters/critical_point_tracker.hh:106-108, 339-343,
 * 392-396; point members features/feature_point.hh:143-205).  recs[] carry ordinal/timestep in their aux word.  v (3 per
 * point) and id are nullable: the sweep does not produce them and the reference writes zeros for discrete points.
 * scalar_names: labels of the text format; n_scalar_names < 0 = the tracker's default {"scalar"}. */
int ftkx_write_critical_points(const char *path, int format, const ftkx_cp_t *recs, size_t n, const double *v, const unsigned long long *id,
                               const char *const *scalar_names, int n_scalar_names);
/* read_critical_points_{json,binary} (critical_point_tracker.hh:345-352, 498-508).  *recs (and *v, *id when asked for) are
 * malloc'ed: release with ftkx_free.  There is no text reader (the reference has none): FTKX_E_UNSUPPORTED. */
int ftkx_read_critical_points(const char *path, int format, ftkx_cp_t **recs, size_t *n, double **v, unsigned long long **id);
/* write_traced_critical_points_{json,binary,text} (critical_point_tracker.hh:354-373, 475-484; features/feature_curve.hh:436-510,
 * features/feature_curve_set.hh:75-118, 180-228) of trajectories as ftkx_post_process_curves returns them (or of raw traced
 * curves: fill type/t with NULL to take them from recs).  Per-curve statistics = feature_curve_t::update_statistics. */
int ftkx_write_traced_critical_points(const char *path, int format, const ftkx_cp_t *recs, size_t n, const ftkx_trajectories *trajs,
                                      const char *const *scalar_names, int n_scalar_names);
/* read_traced_critical_points_{json,binary}: points come back as records in file order (indices = 0..n-1), curve labels as
 * the reference assigns them on load.  Release with ftkx_free(*recs) and ftkx_free_trajectories. */
int ftkx_read_traced_critical_points(const char *path, int format, ftkx_cp_t **recs, size_t *n, ftkx_trajectories *trajs);

/* ---- derived fields on the device (ndarray/grad.hh), exposed for callers that keep V/J themselves ------------- */
/* all pointers are DEVICE pointers; results are bit-identical to the reference's host loops */
int ftkx_gradient2D(ftkx_ctx *ctx, const double *S, int DW, int DH, double *V);                    /* grad.hh:10-31   */
int ftkx_jacobian2D(ftkx_ctx *ctx, const double *V, int DW, int DH, int symmetric, double *J);     /* grad.hh:54-86   */
int ftkx_gradient3D(ftkx_ctx *ctx, const double *S, int DW, int DH, int DD, double *V);            /* grad.hh:130-149 */
int ftkx_jacobian3D(ftkx_ctx *ctx, const double *V, int DW, int DH, int DD, double *J);            /* grad.hh:175-212 */

/* ---- spatial Gaussian smoothing of scalar snapshots (ndarray/conv.hh; the stream's --spatial-smoothing-kernel[-size]) ---- */
/* What ndarray_stream::modified_callback does to every snapshot in front of the tracker (stream.hh:1597-1603):
 * conv_gaussian(array, sigma, ksize, ksize / 2), bit for bit -- weights normalised by their sum AND the result divided by ksize^nd, taps
 * outside the array skipped, every product rounded before it is added, kz outer / ky / kx innermost.
 * ftkx_gaussian_kernel: host only.  gaussian_kernel2D / 3D (conv.hh:74-100, 165-196) with the host's exp; `weights` takes ksize^nd
 * doubles, x fastest.  FTKX_E_INVALID: nd not 2 or 3, ksize even or outside [1, 9], sigma not finite or not positive.  (An even ksize
 * makes the reference's output one larger than its input on every axis, which no tracker can consume.) */
int ftkx_gaussian_kernel(int nd, double sigma, int ksize, double *weights);
/* S and out: DEVICE pointers of DW * DH (* DD) doubles that do not overlap; weights: a HOST array of ksize^nd finite doubles, x fastest
 * (ftkx_gaussian_kernel's, or any other).  Queued on the context's stream; the call returns when `out` is complete. */
int ftkx_conv2D(ftkx_ctx *ctx, const double *S, int DW, int DH, const double *weights, int ksize, double *out);
int ftkx_conv3D(ftkx_ctx *ctx, const double *S, int DW, int DH, int DD, const double *weights, int ksize, double *out);
/* ksize 0 (the default): off.  While on, ftkx_push_scalar_slice makes conv(S) the resident slice -- masks, resolution, halo export and
 * patches see the smoothed array.  A host source is staged into a pooled buffer and convolved into the slice's; with on_device = 1 the
 * caller's array is read, never written and NOT adopted: the context owns the smoothed copy and the call returns once the source has been
 * read, as with 2.  ftkx_push_slice (vector input) fails with FTKX_E_UNSUPPORTED while only this setting is on: conv_gaussian dispatches
 * on nd() and would convolve a vector field across its components.  Vector snapshots have a setting of their own, which smooths every
 * component as the scalar field it is: ftkx_set_vector_smoothing (below, behind the planar pushes).
 * Every push is taken for a RAW snapshot.  An array that is smoothed already -- the resident slice of another context, handed over whole
 * where a slab pass asks for its halo slice as a whole (ftkx_series_dist_status: asked < 0) -- must be pushed with smoothing switched off
 * around that push, or it is convolved twice.  ftkx_slab_* (include/ftkx_slab.h) and the tracker's slab mode do that themselves; the compact
 * halo (masks, request, patches) is built from resident slices and needs nothing. */
int ftkx_set_spatial_smoothing(ftkx_ctx *ctx, double sigma, int ksize);
/* profiling aid (tools/conv_time.py): the kernel of ftkx_conv2D / 3D (nd 2: DD ignored) launched `reps` times back to back on the context's
 * stream, a pair of events around every launch; ms: reps device times. */
int ftkx_debug_conv_relaunch(ftkx_ctx *ctx, int nd, const double *S, int DW, int DH, int DD, const double *weights, int ksize, double *out, int reps, double *ms);

/* ---- temporal Gaussian smoothing of a series of snapshots (filters/streaming_filter.hh; the stream's --temporal-smoothing-kernel[-size]) ---- */
/* The filter ndarray_stream::modified_callback puts in front of the tracker, bit for bit, as this state machine (K = ksize, odd;
 * H = (K + 1) / 2; `data` the deque of raw snapshots):
 *     push(a):  data.push_back(a); if |data| > K: data.pop_front(), cursor--
 *               if |data| >= H: emit sum_i w[i] * data[max(0, i + cursor - H + 1)], cursor++
 *     finish(): loop: data.pop_front(); if |data| >= H: emit sum_i w[i] * data[min(|data| - 1, i)], cursor--; else stop
 * Per element the sum starts as the rounded product w[0] * x0; every later tap is a rounded multiply and a rounded add in order; nothing
 * is fused and taps on the same snapshot are not merged.  N >= K snapshots give N emissions, emission n (0-based) being
 * sum_i w[i] * in[clamp(n + i - (H - 1), 0, N - 1)], H - 1 pushes late; H <= N < K give 2 (N - H) + 1, fewer than H none -- the reference's
 * behaviour, reproduced.  Emissions are numbered here, from the series' first timestep t0 (the reference's callback index is not
 * reproduced).  Element-wise: scalar and vector snapshots alike.
 * ftkx_gaussian_kernel1d: host only.  gaussian_kernel (conv.hh:50-72) with the host's exp; ksize doubles.  FTKX_E_INVALID: ksize even or
 * outside [1, 9], sigma not finite or not positive. */
int ftkx_gaussian_kernel1d(double sigma, int ksize, double *weights);
/* The bare kernel: out[e] = the sum above over arrays[0 .. ksize - 1][e], e < count.  arrays: a HOST array of ksize DEVICE pointers of
 * count doubles each, the same pointer allowed several times (it is then read once per element, and still takes part once per tap);
 * weights: ksize doubles on the HOST (any, not only ftkx_gaussian_kernel1d's); out: count doubles on the device that overlap none of the
 * arrays.  Queued on the context's stream; the call returns when `out` is complete. */
int ftkx_temporal_combine(ftkx_ctx *ctx, const double *const *arrays, int ksize, const double *weights, size_t count, double *out);
/* ksize 0 (the default): off, the ring of raw snapshots is released.  Otherwise a series starts whose first emission gets timestep t0
 * (a series that was open is abandoned).  Refused while sweeps are pending or series passes are open, like ftkx_set_spatial_smoothing.
 * The push functions above are not affected by it: they install a slice unfiltered.  ftkx_set_mesh starts the series afresh, too.
 * MEMORY: the ring holds at most ksize raw arrays (n doubles each for scalar, n * nd for vector snapshots); they come from and return to
 * the pool that dropped slices' arrays go to.  With the filter on, the context holds those ksize arrays plus the emitted slices the
 * caller has not dropped (ftkx_drop_slice) -- an emission is written into the array that leaves the ring where one does. */
int ftkx_set_temporal_smoothing(ftkx_ctx *ctx, double sigma, int ksize, int t0);
/* One RAW snapshot: S (n doubles; is_vector == 0) or V (n * nd doubles, no J, no S; is_vector != 0), n the vertices of the mesh's array
 * extent.  on_device: 0 host memory, 1 or 2 device memory -- the ring always owns a copy; with 1 the source is read and never adopted,
 * and the call returns once it has been read (as with 2; it waits for that point of the stream only, not for work queued before or behind it).  Where spatial smoothing is set a scalar snapshot is convolved into its ring
 * slot first (the stream's order); vector input then fails with FTKX_E_UNSUPPORTED.  If the filter emits, the combined array becomes the
 * resident slice *t_emitted in a buffer of the context's own, like one that ftkx_push_scalar_slice / ftkx_push_slice (V only) installed
 * (masks, resolution, halo export, patches); otherwise *t_emitted = -1.  Scalar and vector snapshots cannot be mixed in one series, nor
 * with resident slices of the other kind (FTKX_E_INVALID). */
int ftkx_temporal_push(ftkx_ctx *ctx, const double *A, int is_vector, int on_device, int *t_emitted);
/* One round of finish() per call: the trailing emission becomes the resident slice *t_emitted; or *t_emitted = -1: the reference's loop
 * would stop -- the ring is released, the filter is in its initial state and the next series' first timestep is the next unused one.
 * Between the first flush and that -1, ftkx_temporal_push is refused. */
int ftkx_temporal_flush(ftkx_ctx *ctx, int *t_emitted);
/* profiling aid (tools/temporal_time.py): the kernel of ftkx_temporal_combine launched `reps` times back to back on the context's stream,
 * a pair of events around every launch; ms: reps device times. */
int ftkx_debug_temporal_relaunch(ftkx_ctx *ctx, const double *const *arrays, int ksize, const double *weights, size_t count, double *out, int reps, double *ms);

/* ---- float32 snapshots (the stream's "format": "float32"; ndarray::from_array, ndarray.hh:403-410) ---- */
/* The reference reads a float32 file into an ndarray<float> and widens it on the host, p[i] = static_cast<double>(a[i]).  Here the floats
 * go to the device as they are -- 4 bytes per value over PCIe -- and are widened there, in front of everything else: the resident slice is
 * FP64, and from there on a slice that arrived as float32 cannot be told apart from one that arrived as the widened doubles.  Widening is
 * exact (subnormal floats become normal doubles, -0.0f becomes -0.0, a NaN stays a NaN with its sign), so every entry below gives, byte for
 * byte, what its FP64 counterpart gives for the widened array.  Checks, error codes and refusals are the counterpart's.  float32 and FP64
 * pushes may be mixed in one context.
 * on_device: 0 host memory, uploaded as floats; 2 device memory of any device, copied; 1 device memory of this context's device, READ where
 * it lies and never adopted -- the call returns once it has been read.  In all three the caller may overwrite its array on return.
 * Where spatial smoothing is set the convolution reads the floats itself: one kernel, float source to smoothed FP64 slice. */
int ftkx_push_scalar_slice_f32(ftkx_ctx *ctx, int t, const float *S, int on_device);
int ftkx_push_slice_f32(ftkx_ctx *ctx, int t, const float *V, const float *J, const float *S, int on_device);
int ftkx_temporal_push_f32(ftkx_ctx *ctx, const float *A, int is_vector, int on_device, int *t_emitted);
/* src: `count` floats, dst: `count` doubles, DEVICE pointers that do not overlap; src a multiple of 4 bytes, dst of 8 (16-byte accesses are
 * used where both can be brought to 16 by the same 0-3 leading elements).  The call returns when `dst` is complete. */
int ftkx_widen_f32(ftkx_ctx *ctx, const float *src, size_t count, double *dst);
/* ftkx_conv2D / ftkx_conv3D from a float32 source: what they give for the widened array */
int ftkx_conv2D_f32(ftkx_ctx *ctx, const float *S, int DW, int DH, const double *weights, int ksize, double *out);
int ftkx_conv3D_f32(ftkx_ctx *ctx, const float *S, int DW, int DH, int DD, const double *weights, int ksize, double *out);
/* profiling aid (tools/push_f32_time.py): the kernel of ftkx_widen_f32 launched `reps` times back to back on the context's stream, a pair of
 * events around every launch; ms: reps device times. */
int ftkx_debug_widen_relaunch(ftkx_ctx *ctx, const float *src, size_t count, double *dst, int reps, double *ms);
/* how many float32 arrays this context was pushed went through the widen kernel, and how many straight through the convolution */
int ftkx_debug_f32_counts(const ftkx_ctx *ctx, unsigned long long *widened, unsigned long long *convolved_direct);
/* test aid: the context's slice arrays by class -- [0] field arrays (the S / V / J copies of slices, staging arrays, the temporal ring),
 * [1] mask arrays, [2] summary arrays.  allocated: how many the context has had to allocate since it was made (an array taken out of its
 * pool is not counted; neither is one the caller lent with on_device = 1); pooled: how many lie in the pool right now, held by no slice.
 * Either may be null.  Reads the context, changes nothing. */
int ftkx_debug_array_counts(const ftkx_ctx *ctx, unsigned long long allocated[3], unsigned long long pooled[3]);

/* ---- half, bfloat16 and integer snapshots (ndarray<T>::from_array<T1>, ndarray.hh:401-410) ---- */
/* Image sequences and .vti image data of unsigned char / short, NetCDF variables of NC_BYTE / NC_SHORT / NC_INT, half or bfloat16 fields
 * of an ML surrogate: the reference widens all of them on one host thread, p[i] = static_cast<double>(a[i]).  Here the elements go to the
 * device as they are -- 1, 2 or 4 bytes per value over PCIe -- and ONE kernel widens them there, in front of everything else.  Every value
 * of every type below is a double, so widening is exact (a subnormal half becomes a normal double, a NaN stays a NaN with its sign): each
 * typed entry gives, byte for byte, the resident slice its FP64 counterpart gives for the widened array, and spatial smoothing,
 * perturbation, clamp, the temporal filter and the sweep behind it are that push's.  Checks, error codes and refusals are the
 * counterpart's.  64-bit integers are not exact in FP64 and are not taken. */
enum {
  FTKX_DTYPE_F64 = 0,      /* FP64: a typed entry hands it to the FP64 entry unchanged */
  FTKX_DTYPE_F32 = 1,      /* float32: handed to the _f32 entry unchanged */
  FTKX_DTYPE_F16 = 2,      /* IEEE half */
  FTKX_DTYPE_BF16 = 3,     /* bfloat16: the upper 16 bits of a float32 */
  FTKX_DTYPE_U8 = 4, FTKX_DTYPE_I8 = 5,
  FTKX_DTYPE_U16 = 6, FTKX_DTYPE_I16 = 7,
  FTKX_DTYPE_U32 = 8, FTKX_DTYPE_I32 = 9
};
/* bytes of one element; 0 for a dtype that is none of the above */
size_t ftkx_dtype_size(int dtype);
/* One entry point for every element type.  dtype: FTKX_DTYPE_*, anything else FTKX_E_INVALID; a pointer that is not a multiple of
 * ftkx_dtype_size(dtype) is FTKX_E_INVALID.  ftkx_push_slice_typed: V, J and S (those given) share the one type.
 * on_device: 0 host memory, uploaded as it is; 2 device memory of any device, copied as it is; 1 device memory of this context's device,
 * READ where it lies.  A narrow array is never adopted: the call returns once the source has been read and the caller may overwrite it.
 * A host source, a source given with 2 and a pointer of another device are staged in the context's byte block for narrow sources,
 * count * ftkx_dtype_size(dtype) bytes.  The narrow kernel writes straight into the slice's own array; where spatial smoothing is set it
 * writes a pooled array that the FP64 convolution reads into the slice's array; perturbation and clamp follow in place.
 * ftkx_debug_f32_counts and ftkx_debug_planar_counts do not move for a narrow push; ftkx_debug_adjust_counts moves as for a copied FP64
 * source (in_place).  Narrow and float32 and FP64 pushes may be mixed in one context. */
int ftkx_push_scalar_slice_typed(ftkx_ctx *ctx, int t, const void *S, int dtype, int on_device);
int ftkx_push_slice_typed(ftkx_ctx *ctx, int t, const void *V, const void *J, const void *S, int dtype, int on_device);
int ftkx_temporal_push_typed(ftkx_ctx *ctx, const void *A, int dtype, int is_vector, int on_device, int *t_emitted);
/* src: `count` elements of `dtype`, dst: `count` doubles, DEVICE pointers that do not overlap; src a multiple of its element's size, dst of
 * 8.  A lane takes 4 elements with one load and stores 2 x 16 bytes where source and destination can be brought to 4 elements' bytes and
 * to 16 by the same 0-3 leading elements, and goes element by element otherwise.  The call returns when `dst` is complete.  dtype:
 * FTKX_DTYPE_F16 .. FTKX_DTYPE_I32; FTKX_DTYPE_F32 is handed to ftkx_widen_f32 (below: to ftkx_debug_widen_relaunch); FP64 has nothing to
 * widen and is FTKX_E_INVALID like an unknown code. */
int ftkx_widen_typed(ftkx_ctx *ctx, const void *src, int dtype, size_t count, double *dst);
/* profiling aid (tools/push_narrow_time.py): the kernel of ftkx_widen_typed launched `reps` times back to back on the context's stream, a
 * pair of events around every launch; ms: reps device times. */
int ftkx_debug_narrow_relaunch(ftkx_ctx *ctx, const void *src, int dtype, size_t count, double *dst, int reps, double *ms);
/* per_dtype[FTKX_DTYPE_*]: launches of the narrow kernel by this context's pushes so far, by element type ([0] and [1] stay 0: FP64 and
 * float32 never take it) */
int ftkx_debug_narrow_counts(const ftkx_ctx *ctx, unsigned long long per_dtype[10]);

/* ---- vector snapshots given as one array per component (the stream's "u, v, w in separate variables"; ndarray::concat, ndarray.hh:1157-1172) ---- */
/* The reference reads a vector field that a file keeps as one variable per component into nv arrays and interleaves them on the host,
 * result[i * nv + j] = arrays[j][i].  Here the nc = nd planes go to the device as they are, float32 or FP64, and ONE kernel writes the
 * resident FP64 V from them, widening where they are float32: byte for byte the slice that ftkx_push_slice (ftkx_push_slice_f32) makes of the
 * host-interleaved array, and everything behind it -- perturbation, clamp, the temporal filter, the sweep -- is as for that push.
 * Vc: nc pointers, each to n_vertices elements at a multiple of the element's size; planes may be one another.  nc must be the context's nd.
 * J and S keep the meaning and the (interleaved) layout they have in ftkx_push_slice, and are refused with FTKX_E_UNSUPPORTED while
 * perturbation or clamp is on; spatial smoothing set: FTKX_E_UNSUPPORTED, as for every vector push.  A wrong nc, a null or misaligned plane:
 * FTKX_E_INVALID, nothing is launched.
 * on_device holds for all planes of a call (and for J and S): 0 host memory, staged plane behind plane at the bytes of the interleaved
 * array; 2 device memory of any device, copied; 1 device memory of this context's device, READ where it lies and never adopted -- the call
 * returns once the planes have been read (planes found on another device are copied, like 2).  The caller may overwrite them on return.
 * With perturbation or clamp on, the concat kernel writes the slice and the adjust kernel runs in place behind it (the stream's order:
 * concat -> perturb -> clamp -> temporal filter); the noise's element index is the flat index of the interleaved array. */
int ftkx_push_slice_planar(ftkx_ctx *ctx, int t, const double *const *Vc, int nc, const double *J, const double *S, int on_device);
int ftkx_push_slice_planar_f32(ftkx_ctx *ctx, int t, const float *const *Vc, int nc, const float *J, const float *S, int on_device);
/* ftkx_temporal_push (is_vector = 1) of the snapshot the planes make */
int ftkx_temporal_push_planar(ftkx_ctx *ctx, const double *const *Vc, int nc, int on_device, int *t_emitted);
int ftkx_temporal_push_planar_f32(ftkx_ctx *ctx, const float *const *Vc, int nc, int on_device, int *t_emitted);
/* The kernel alone: dst[v * nc + k] = (double)planes[k][v] for v < count; nc 2 or 3.  planes: a HOST array of nc DEVICE pointers, each a
 * multiple of its element's size; dst: count * nc doubles on the device at a multiple of 8 that overlap no plane (there is no in-place
 * form).  FP64 values are moved as bits (a NaN keeps its payload).  16-byte accesses are used where all planes have the same address
 * modulo 16 and dst can be brought to 16 by the same leading vertices.  Anything else: FTKX_E_INVALID, nothing is launched.  The call returns
 * when `dst` is complete. */
int ftkx_concat(ftkx_ctx *ctx, const double *const *planes, int nc, size_t count, double *dst);
int ftkx_concat_f32(ftkx_ctx *ctx, const float *const *planes, int nc, size_t count, double *dst);
/* profiling aid (tools/push_planar_time.py): the kernel of ftkx_concat (planes_are_f32 != 0: of ftkx_concat_f32) launched `reps` times back to
 * back on the context's stream, a pair of events around every launch; ms: reps device times. */
int ftkx_debug_concat_relaunch(ftkx_ctx *ctx, const void *const *planes, int nc, int planes_are_f32, size_t count, double *dst, int reps, double *ms);
/* launches of the concat kernel by this context so far: with the 16-byte body, and vertex by vertex.  Either may be null. */
int ftkx_debug_planar_counts(const ftkx_ctx *ctx, unsigned long long *vec_launches, unsigned long long *scalar_launches);

/* ---- spatial Gaussian smoothing of VECTOR arrays, every component as the scalar field it is (conv_vec_kernels.hip) ----
 * For an array V of nc components (nc = nd: 2 in 2D, 3 in 3D):
 *     conv_vec(V)[c + nc * i] == conv(plane_c)[i]        with plane_c[i] = V[c + nc * i]
 * where conv is exactly what ftkx_conv2D / ftkx_conv3D compute -- no tolerance: byte for byte that kernel's output per plane, interleaved.
 * Components never mix.  (Not the reference's conv_gaussian on such an array, which would convolve across the component axis.)  ONE launch
 * handles the whole array.  A float32 source is widened as it is staged; planes (ftkx_conv_planar: nd device pointers in a HOST array, DW *
 * DH (* DD) elements each; nd 2: DD ignored) follow the same rule with plane_c given directly and give the same interleaved FP64 output.
 * All array pointers are DEVICE pointers; out: nc * DW * DH (* DD) doubles; weights: a HOST array of ksize^nd doubles.  FTKX_E_INVALID: a
 * null pointer, a non-positive extent, ksize even or outside [1, 9], nd not 2 or 3, an input overlapping the output.  The call returns when
 * `out` is complete. */
int ftkx_conv2D_vec(ftkx_ctx *ctx, const double *V, int DW, int DH, const double *weights, int ksize, double *out);
int ftkx_conv3D_vec(ftkx_ctx *ctx, const double *V, int DW, int DH, int DD, const double *weights, int ksize, double *out);
int ftkx_conv2D_vec_f32(ftkx_ctx *ctx, const float *V, int DW, int DH, const double *weights, int ksize, double *out);
int ftkx_conv3D_vec_f32(ftkx_ctx *ctx, const float *V, int DW, int DH, int DD, const double *weights, int ksize, double *out);
int ftkx_conv_planar(ftkx_ctx *ctx, int nd, const double *const *planes, int DW, int DH, int DD, const double *weights, int ksize, double *out);
int ftkx_conv_planar_f32(ftkx_ctx *ctx, int nd, const float *const *planes, int DW, int DH, int DD, const double *weights, int ksize, double *out);
/* ksize 0 (the default): off.  A setting of its own beside ftkx_set_spatial_smoothing, which keeps refusing vectors where it alone is set;
 * scalar pushes are never touched by this one.  While on, ftkx_push_slice, _f32, _typed, ftkx_push_slice_planar, _f32 and -- with a vector --
 * ftkx_temporal_push, _f32, _typed, ftkx_temporal_push_planar, _f32 make conv_vec(V), under ftkx_gaussian_kernel(nd, sigma, ksize), the
 * resident V (the ring's snapshot): masks, resolution, halo export and patches see the smoothed array, and with derive_jacobian the Jacobian
 * at hits comes from it.  The stream's order holds: widen -> smooth -> perturb -> clamp -> temporal ring.  Planes are smoothed and
 * interleaved by the one kernel (no concat launch: ftkx_debug_planar_counts does not move); floats are widened as the kernel stages them;
 * narrower types are widened into a pooled array that the FP64 kernel reads.  on_device = 1: read before the call returns, never adopted.
 * J or S beside V: FTKX_E_UNSUPPORTED -- a given Jacobian does not belong to the smoothed field.  Every push is taken for a RAW snapshot
 * (see ftkx_set_spatial_smoothing); the slab pass's hand-over of a whole slice sets this setting aside as it does that one.
 * Refused while sweeps are pending or series passes are open. */
int ftkx_set_vector_smoothing(ftkx_ctx *ctx, double sigma, int ksize);
/* profiling aid (tools/conv_vec_time.py): the kernel launched `reps` times back to back, a pair of events around every launch; src: a HOST
 * array of device pointers -- planar: nd planes, else src[0] is the interleaved array; ms: reps device times. */
int ftkx_debug_conv_vec_relaunch(ftkx_ctx *ctx, int nd, const void *const *src, int planar, int src_is_f32, int DW, int DH, int DD, const double *weights, int ksize, double *out,
                                 int reps, double *ms);
/* launches of the kernel by this context's pushes: from an interleaved source, from planes, and how many of either read float32 */
int ftkx_debug_conv_vec_counts(const ftkx_ctx *ctx, unsigned long long *interleaved, unsigned long long *planar, unsigned long long *f32);

/* ---- perturbation and clamp of snapshots (ndarray::perturb, ndarray::clamp; the stream's "perturbation" and "clamp") ---- */
/* The two steps ndarray_stream::modified_callback (stream.hh:1570-1604) runs between the spatial smoothing and the temporal filter:
 *     widen -> conv_gaussian -> perturb(sigma) -> clamp(lo, hi) -> temporal filter -> tracker
 * Both are off by default; with both off every push queues exactly the kernels it queued before.  While either is on, every snapshot pushed
 * (ftkx_push_scalar_slice, ftkx_push_slice with V alone, ftkx_temporal_push, and their _f32 forms) is adjusted on the device by ONE kernel
 * behind the widening and the smoothing: a float32 source goes through it in place of the widen kernel; a host FP64 source is uploaded
 * straight into the slice's array and adjusted in place; a device FP64 source is read where it lies and written adjusted into an array of
 * the context's own; a smoothed snapshot is adjusted in place behind the convolution.  With on_device = 1 the caller's array is read, never
 * written and NOT adopted, and the call returns once it has been read -- what smoothing does.  A snapshot that enters the temporal ring
 * enters it adjusted.  ftkx_push_slice with J or S beside V fails with FTKX_E_UNSUPPORTED: the stream delivers one array.  For a vector
 * snapshot all n * nd values are adjusted, the element index being the flat one.  Like smoothing, every push is taken for a RAW snapshot;
 * ftkx_slab_* set the adjustment aside where they push a neighbour's resident slice whole.
 * clamp: p[i] = std::min(std::max(lo, p[i]), hi), bit for bit -- m = (lo < x) ? x : lo; out = (hi < m) ? hi : m.  A NaN becomes lo (hi
 * where hi < lo); -0.0 under lo = +0.0 becomes +0.0; lo > hi is legal and makes everything hi.  A NaN bound is FTKX_E_INVALID.
 * perturbation: the reference adds std::normal_distribution<>{0, sigma} from an std::mt19937 seeded by std::random_device, different on
 * every run.  Reproduced is the distribution: p[e] += sigma * z, z independent N(0, 1), DEFINED as a pure function of (seed, the
 * snapshot's number t, the element index e) -- Philox4x32-10 with counter (e >> 1, t, 0) and key seed, 52 bits to a uniform in (0, 1),
 * Wichura's AS 241 PPND16 (ftk_amd/csrc/adjust_steps.hpp) -- whatever the launch, the path, the device, the rank or the context: two
 * contexts handed the same snapshot add the same noise.  t is the timestep the snapshot is pushed as; in a temporal series, t0 plus the
 * number of snapshots pushed before it.  sigma 0: off.  A negative or non-finite sigma is FTKX_E_INVALID.
 * Both are refused while sweeps are pending or series passes are open, like ftkx_set_spatial_smoothing. */
int ftkx_set_perturbation(ftkx_ctx *ctx, double sigma, unsigned long long seed);
int ftkx_set_clamp(ftkx_ctx *ctx, int on, double lo, double hi);
/* The bare kernel: dst[e] = clamp(double(src[e]) + sigma * z(seed, t, e), lo, hi) for e < count -- the perturbation left out where sigma is
 * 0, the clamp where clamp_on is 0 (one of them must be asked for).  DEVICE pointers; src a multiple of its element's size, dst of 8 bytes
 * (a pair of elements is one access where src is a multiple of two elements and dst of 16 bytes); dst == src is allowed (ftkx_adjust), any
 * other overlap is not.  The call returns when `dst` is complete. */
int ftkx_adjust(ftkx_ctx *ctx, const double *src, size_t count, double sigma, unsigned long long seed, int t, int clamp_on, double lo, double hi, double *dst);
int ftkx_adjust_f32(ftkx_ctx *ctx, const float *src, size_t count, double sigma, unsigned long long seed, int t, int clamp_on, double lo, double hi, double *dst);
/* profiling aid (tools/adjust_time.py): the kernel of ftkx_adjust (src_is_f32 != 0: of ftkx_adjust_f32) launched `reps` times back to back
 * on the context's stream, a pair of events around every launch; ms: reps device times. */
int ftkx_debug_adjust_relaunch(ftkx_ctx *ctx, const void *src, int src_is_f32, size_t count, double sigma, unsigned long long seed, int t, int clamp_on, double lo, double hi,
                               double *dst, int reps, double *ms);
/* how many snapshots this context was pushed went through the adjust kernel: from a float32 source, FP64 in place, FP64 out of place */
int ftkx_debug_adjust_counts(const ftkx_ctx *ctx, unsigned long long *from_float, unsigned long long *in_place, unsigned long long *out_of_place);

/* ---- auxiliary scalar fields sampled at critical points (critical_point_tracker::set_scalar_components, filters/critical_point_tracker.hh:50-51) ---- */
/* A record has three scalar slots (FTK_CP_MAX_NUM_VARS); the sweep fills scalar[0] from the slice's own S.  Slots 1 and 2 take other fields
 * of the same lattice -- pressure at the critical points of a velocity field, two more variables along an extremum's trajectory -- read at
 * the critical point with the very barycentric weights scalar[0] is read with: mu from the simplex's field values exactly as the record
 * kernels form it (2D: the solve, clamped only where it failed; 3D: the solve, always clamped), then a[0] * mu[0] + a[1] * mu[1] + ... left
 * to right.  Pushing a slice's own S as an aux array gives scalar[0] back bit for bit.  It is ONE pass over finished records, behind any
 * sweep (ftkx_sweep, _collect, _series, the one-shot calls' records with a context of the same mesh): the sweeps, their kernels and their
 * records are not changed by it, and records whose slots nobody asks for keep zeros there.
 * ftkx_push_aux_slice: A holds one value per vertex of the mesh's array extent (the layout of S) and becomes the aux array of slot 1 or 2
 * at timestep t, replacing one that was there.  on_device as for ftkx_push_scalar_slice: 0 host memory, copied; 2 device memory of any
 * device, copied; 1 device memory of this context's device, LENT -- read where it lies, never written, never freed by the library, the
 * caller's until ftkx_drop_slice(t) or ftkx_destroy.  _f32: widened on the device into an array of the context's own (on_device 1: read
 * where it lies, the call returns once it has been read).  Aux arrays come out of and go back to the pool of the slices' field arrays
 * (ftkx_debug_array_counts, class 0).  They belong to timestep t, not to the slice object: they may be pushed before or after the field
 * slice, stay when it is pushed again, and leave with ftkx_drop_slice(t).  Spatial and temporal smoothing, perturbation and clamp NEVER
 * apply to them: an aux array is read as it was pushed.  FTKX_E_INVALID: slot not 1 or 2, a null or misaligned array, no mesh.
 * ftkx_sample_aux: recs are n host records of this context's mesh and options, with the aux word the sweep wrote (they may be the
 * context's own record buffer).  For every slot that has an aux array at ALL timesteps the records read -- a record's own, and the one
 * behind it for an interval record -- scalar[slot] of every record is overwritten; no other byte of a record changes.  Everything is
 * checked before anything is written (all or nothing): a timestep without a resident field slice, or a slot with arrays at some of the
 * timesteps but not all: FTKX_E_NOSLICE; a slice that exists as masks only: FTKX_E_UNSUPPORTED; FTKX_TAG_REFERENCE tags on a mesh and at
 * timesteps where their int32 products may have wrapped (the tag no longer says which element it is): FTKX_E_UNSUPPORTED; a record that is
 * no element of the mesh: FTKX_E_INVALID.  No slot with arrays, or n == 0: FTKX_OK, nothing is done.  16 bytes per record go up, 8 per
 * record and slot come down, through buffers the context keeps; the call waits for its kernel on the context's stream. */
int ftkx_push_aux_slice(ftkx_ctx *ctx, int t, int slot /* 1 | 2 */, const double *A, int on_device);
int ftkx_push_aux_slice_f32(ftkx_ctx *ctx, int t, int slot /* 1 | 2 */, const float *A, int on_device);
int ftkx_sample_aux(ftkx_ctx *ctx, ftkx_cp_t *recs, size_t n);
/* profiling aid (tools/sample_time.py): the kernel of ftkx_sample_aux launched `reps` times back to back on the context's stream, a pair of
 * events around every launch; ms: reps device times.  The records are not written. */
int ftkx_debug_sample_relaunch(ftkx_ctx *ctx, const ftkx_cp_t *recs, size_t n, int reps, double *ms);
/* launches of the sample kernel by ftkx_sample_aux on this context so far, and the records they took.  Either may be null. */
int ftkx_debug_sample_counts(const ftkx_ctx *ctx, unsigned long long *launches, unsigned long long *records);

/* ---- the series pass samples its own records: they leave the device filled ----
 * ftkx_set_series_sampling(ctx, on), default off.  While it is on, the records of ftkx_sweep_series and of ftkx_sweep_series_submit /
 * _complete come back with scalar[1] / scalar[2] filled -- the values ftkx_sample_aux gives, bit for bit; no other byte of a record differs
 * from the pass of a context that is not armed.  The sampling runs in stream order inside the pass, on the records in device memory in
 * front of their copy to the host: nothing goes up, nothing is decoded on the host, and the slices and aux arrays may be dropped as soon
 * as the pass has been submitted.  Which slots are filled is decided at submit, over the slices the pass's steps read (a step's own, and
 * the one behind it for an interval sweep): a slot with an aux array at every one of them is sampled; one with none is left zero; one
 * with an array at some but not all: FTKX_E_NOSLICE, nothing is queued and the context stays usable.  With no aux array at any of them
 * the pass is planned, queued and run exactly as without the switch.  Whatever ftkx_sample_aux refuses for those records and arrays is
 * refused at submit with the same code.  A pass with a slot to fill keeps its records in device memory, takes the kernel chain (not the
 * fused tail, not the one-launch pass: ftkx_series_last_path 1 or 5) and has the copy kernel bring them over; where the host-driven batch
 * takes the pass over (ftkx_series_last_path 0) the batch's records are sampled inside the call before they are returned, and a failure
 * there -- an aux array dropped meanwhile: FTKX_E_NOSLICE -- fails the call.  Slab passes (ftkx_series_dist_*) on an armed context:
 * FTKX_E_UNSUPPORTED.  Changing the switch while a pass is open: FTKX_E_INVALID.
 * Lifetime: an aux array of the context's own that is dropped or replaced under an open pass is kept for as long as that pass may read it
 * (as a dropped slice's arrays are).  A LENT array (on_device = 1) is the caller's to keep alive until every pass submitted while it was
 * resident has been completed.
 * ftkx_series_sampled: of the pass completed last -- *slots the set of slots filled (bit 0: scalar[1], bit 1: scalar[2]), *where 0 not
 * filled, 1 by the kernel inside the pass, 2 behind the host-driven batch inside the call.  Either may be null.
 * ftkx_debug_series_sample_counts: launches of the in-pass kernel on this context so far, the records of the passes they belonged to
 * (counted when a pass completes), and the workgroups of the last launch.  Each may be null.  ftkx_debug_sample_counts keeps its meaning:
 * launches on behalf of ftkx_sample_aux, and of `where` = 2. */
int ftkx_set_series_sampling(ftkx_ctx *ctx, int on);
int ftkx_series_sampled(const ftkx_ctx *ctx, unsigned *slots, int *where);
int ftkx_debug_series_sample_counts(const ftkx_ctx *ctx, unsigned long long *launches, unsigned long long *records, unsigned *workgroups_of_last_launch);

/* test aid: the ordering step of the device-driven pass completed last on this context (ftkx_sweep_series, ftkx_sweep_series_complete), as
 * it ran: out[0] the number of buckets, out[1] the shift that takes an order key to its bucket, out[2] the fullest bucket, out[3] the
 * size up to which a bucket was ranked on the device (fuller ones: the host orders them, status bit 16).  All zero where the pass's records
 * did not come through the bucket chain (ftkx_series_last_path 0, 2, 4).  Reads the context, changes nothing. */
int ftkx_debug_series_order(const ftkx_ctx *ctx, unsigned long long out[4]);
/* test aid: the host-driven batch's ordering step (the radix sort behind ftkx_sweep_collect for 4 096 records and more) on `n` records of
 * the caller's, whatever their number: in -> the context's hit buffer -> the sort -> out, both host memory.  key_bits: 1 .. 64, every
 * tag below 2^key_bits.  Equal tags keep their order.  Not while sweeps are pending or series passes are open. */
int ftkx_debug_sort_records(ftkx_ctx *ctx, const ftkx_cp_t *in, size_t n, int key_bits, ftkx_cp_t *out);

/* profiling aid: streams `bytes` of device memory with the mask kernel's load shape (16 B per lane) and nothing else, so that
 * rocprofv3's FETCH_SIZE can be calibrated on a known byte count (tools/calibrate_fetch.py) */
int ftkx_debug_stream_read(ftkx_ctx *ctx, const void *device_ptr, size_t bytes);

/* profiling aid (bench.py's int-VALU yardstick): from the next sweep on the tile kernel -- exact_only, the overflow regime -- repeats its fan
 * phase, the predicate arithmetic on a tile staged in LDS, `repeat` times per tile and step; records are those of one.  The time the extra
 * repetitions add is the time of the arithmetic alone.  1 = off. */
int ftkx_debug_tile_repeat(ftkx_ctx *ctx, int repeat);

/* profiling aid: the mask-kernel instantiation of the most recent sweep in this process, spelled as rocprofv3 lists it */
const char *ftkx_last_mask_kernel(void);

/* profiling aid: launches per mask-kernel instantiation family in this process (seven of them; returns that number): which shapes the
 * suite / a workload reached -- every kernel behind launch_masks is reachable by some mesh, none is there for history's sake */
int ftkx_debug_mask_kernel_launches(unsigned long long *launches, const char **names, int n);

/* profiling aid: how the host arrays this context was handed (on_device = 0) reached HBM -- staged by the library's copy threads through
 * pinned pieces (pageable sources of 32 MiB and more; FTKX_UPLOAD_THREADS, default 4, 0 = never) or by the runtime's own copy */
int ftkx_debug_upload_counts(const ftkx_ctx *ctx, unsigned long long *staged, unsigned long long *direct);

/* profiling aid (tools/mask_overlap.py): slice t's mask job -- its masks must exist, ftkx_slices_prepare -- launched `reps` times back to
 * back on the context's stream (nstreams 1) or alternately on it and a second stream (2), with a small dependent kernel in front of each
 * launch when with_begin; device time per launch.  What a streaming tracker's one-slice launch pays for its ramp. */
int ftkx_debug_mask_relaunch(ftkx_ctx *ctx, int t, int reps, int nstreams, int with_begin, double *ms_per_launch);

/* library / device identification */
const char *ftkx_version(void);
int ftkx_device_count(void);
int ftkx_pointer_device(const void *p);          /* ordinal of the device the pointer lives on, -1: host memory or unknown */
int ftkx_context_device(const ftkx_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
