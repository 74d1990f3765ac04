// The host-driven batch (collect.hip: ftkx_sweep_enqueue / ftkx_sweep_collect; halo.hip: ftkx_sweep_cull) as decisions: which way a
// request goes, which masks a batch builds in which sub-batch, its tile launches, where its descriptors lie, how many key bits its records
// need, and what follows from the counters a batch left.  No HIP and no context: collect.hip and halo.hip carry the plan out, and
// tests/test_batch_plan_host.py enumerates it on the CPU (tests/hostcheck/batch_plan.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "sweep_params.hpp"

namespace ftkxh {

using ftkx::u64;

// ---- what the host knows of a slice's masks --------------------------------------------------------------------------------------------
struct SliceFacts {
  bool has_M = false, has_U = false;   // the mask / summary arrays exist
  bool sparse = false;                 // a halo slice that exists as masks only: they cannot be rebuilt
  u64 mask_factor = 0;                 // the factor the masks were built under; 0 = not built
  bool mask_big = false;               // ... with the per-vertex overflow rule of that factor
  int u_rows = 1;                      // rows a summary byte stands for
  bool max_known = false;              // maxabs is the slice's largest |v|
  double maxabs = 0;
};

// the strict-sign cull is exact only while no determinant of the predicate can leave int64:
// |det4| <= 24 M^3 (3D), |det3| <= 6 M^2 (2D) with M = max |quantised component|   
inline bool overflow_free(int nd, double maxabs, u64 factor)
{
  const long double M = floorl((long double)maxabs * (long double)factor) + 1.0L;
  const long double lim = 9223372036854775807.0L;
  return nd == 3 ? 24.0L * M * M * M < lim : 6.0L * M * M < lim;
}

inline double big_threshold(int nd, u64 factor) { return (double)(nd == 3 ? ftkx::kSafeM3 : ftkx::kSafeM2) / (double)factor; }
inline bool pow2_factor(u64 factor) { return factor != 0 && (factor & (factor - 1)) == 0 && factor <= (1ull << 53); }

// Masks built under mask_factor serve a sweep under `factor` when they can only cull less than masks built under `factor`
// itself: the sign thresholds need mask_factor <= factor; the per-vertex overflow rule (MaskJob::big) is factor-specific, so a
// larger factor is accepted only when the slice's max |v| shows that no vertex is big under it either.
inline bool masks_valid(int nd, const SliceFacts &s, u64 factor, bool two_level, int u_rows)
{
  if (!s.has_M || (two_level && !s.has_U) || s.mask_factor == 0 || s.mask_factor > factor) return false;
  if (two_level && s.u_rows != u_rows) return false;           // summaries of another geometry (FTKX_MASK_* changed since)
  if (s.mask_big && s.mask_factor == factor) return true;
  return s.max_known && overflow_free(nd, s.maxabs, factor);   // no vertex is big under `factor`: the rule would change nothing
}

// the per-vertex rule costs the marching kernels a few instructions per row: it is switched on only when it can matter
inline double job_big(int nd, const SliceFacts &s, u64 factor, bool *rule_on)
{
  const bool off = s.max_known && overflow_free(nd, s.maxabs, factor);
  *rule_on = !off;
  return off ? HUGE_VAL : big_threshold(nd, factor);
}

// ---- one request -----------------------------------------------------------------------------------------------------------------------
// how a request is swept: MODE_TILE tests every simplex (exact_only, non-robust 3D, odd factors); MODE_FAST = masks -> cull ->
// survivor list -> exact kernel; MODE_TILE_CULL = the tile kernel with its in-tile cull (same per-vertex legality rule), for
// data on which most cells survive the cull anyway (the int64-overflow regime: a survivor list would be as large as the input)
enum { MODE_TILE = 0, MODE_FAST = 1, MODE_TILE_CULL = 2 };

// Is the strict-sign cull usable?  Only with the robust integer test (the FP64 test of the non-robust 3D mode has no such
// property) and a power-of-two factor: the masks test v >= 1/factor on doubles, which equals trunc(v * factor) >= 1 only then
// (the tracker always passes 1 << nbits); any other factor a direct caller hands over takes the tile path, which quantises like
// the reference.  Determinants that could leave int64 are dealt with per vertex (MaskJob::big), not per request.
inline int request_mode(bool exact_only, u64 factor, int nd, bool robust, int dense_collects)
{
  const bool fast = !exact_only && pow2_factor(factor) && (nd == 2 || robust);
  return !fast ? MODE_TILE : dense_collects > 0 ? MODE_TILE_CULL : MODE_FAST;
}
// a masked halo slice has no values to test: it serves the cull of MODE_FAST and nothing else
inline bool sparse_slice_refuses(int mode) { return mode != MODE_FAST; }

// Which tile_kernel<ND, FORM> a request may take: `bound` = the largest |quantised component| it can meet (max |v| x factor), below 0
// where the slices' maxima are not known (the kernel checks every tile anyway); `fan` = FTKX_TILE_FAN (9: as the tiles allow).
inline int tile_form(int nd, bool robust, double bound, int fan)
{
  const double fp_bound = nd == 3 ? 524287.0 : 33554431.0;     // below 2^19 (3D: error-bounded fp64) / 2^25 (2D: exact fp64)
  const int form = (nd == 3 && !robust) ? 0 : bound < 0 ? 1 : bound < fp_bound ? 2 : bound < 2147483647.0 ? 1 : 0;
  return std::min(form, fan == 9 ? 2 : fan);
}

// ---- one batch -------------------------------------------------------------------------------------------------------------------------
struct BatchMesh { int nd; bool robust, two_level; int u_rows; };      // two_level, u_rows: the mask plan's (masks_have_summary, Mesh::u_rows)
struct BatchRequest { int mode, s0, s1; u64 factor; };                 // s0, s1: indices of slice t and slice t + 1 (-1: ordinal sweep only) in the facts
struct BatchKnobs { bool tile_walk; int tile_fan; };                   // FTKX_TILE_WALK (0 = a tile launch per request), FTKX_TILE_FAN

struct BatchMaskJob { int slice; u64 factor; bool rule_on; double big; };
// Fast requests are grouped into sub-batches (one mask / cull / exact launch each); a new one starts whenever a slice's masks would be
// needed under a second factor (the factor is a running minimum, so it changes a few times at the start of a series and then stays put).
struct BatchSub { std::vector<BatchMaskJob> jobs; std::vector<int> steps; };      // steps: request indices
// The tile requests: one launch per run of consecutive tile requests with the same cull setting -- a workgroup walks the run's steps in
// time order with its tile staged in LDS (tile_kernels.hip) -- under the smallest form any of them asks for (every form is correct everywhere)
struct BatchTileRun { int first, nsteps, cull, fan, form; };           // first: index into BatchPlan::tile_steps

enum { BATCH_OK = 0, BATCH_SPARSE_CANNOT_SERVE = 1, BATCH_TOO_MANY = 2 };

struct BatchPlan {
  int status = BATCH_OK;
  int refused = -1;                    // BATCH_SPARSE_CANNOT_SERVE: the request
  std::vector<BatchSub> subs;          // at least one, possibly empty
  std::vector<int> tile_steps;         // the tile requests in order: request indices
  std::vector<BatchTileRun> runs;
  // One block for all descriptors: the mask jobs of each sub-batch (each at a multiple of 256 bytes), then ONE array of Fields for the
  // whole batch -- the steps of sub-batch 0, 1, ... back to back (each cull / exact launch gets its slice of it) and the tile requests
  // behind them; the record kernel looks a simplex's request up in that array by the index its pass descriptor carries.
  std::vector<size_t> job_off, step_base;
  size_t fields_off = 0, tile_base = 0, nfields = 0, bytes = 0;
  std::vector<SliceFacts> facts;       // the slices once the batch's mask launches have run
};

inline size_t batch_round256(size_t v) { return (v + 255) / 256 * 256; }

inline BatchPlan plan_batch(const BatchMesh &m, const std::vector<BatchRequest> &requests, const std::vector<SliceFacts> &slices, const BatchKnobs &knobs)
{
  BatchPlan P;
  P.facts = slices;                    // a later request's masks_valid sees the jobs planned before it
  P.subs.emplace_back();
  for (int i = 0; i < (int)requests.size(); i ++) {
    const BatchRequest &r = requests[i];
    if (r.mode == MODE_FAST) {
      int build[2], nbuild = 0;
      for (int s : {r.s0, r.s1}) {
        if (s < 0 || masks_valid(m.nd, P.facts[s], r.factor, m.two_level, m.u_rows)) continue;     // e.g. built by ftkx_slices_prepare, or by an earlier step
        if (P.facts[s].sparse) { P.status = BATCH_SPARSE_CANNOT_SERVE; P.refused = i; return P; }
        build[nbuild ++] = s;
      }
      // masks of such a slice already (re)built or used in the current sub-batch under another factor -> close it
      bool touched = false;
      for (int b = 0; b < nbuild; b ++) {
        for (const BatchMaskJob &j : P.subs.back().jobs) touched = touched || j.slice == build[b];
        for (int g : P.subs.back().steps) touched = touched || requests[g].s0 == build[b] || requests[g].s1 == build[b];
      }
      if (touched) P.subs.emplace_back();
      for (int b = 0; b < nbuild; b ++) {
        SliceFacts &f = P.facts[build[b]];
        BatchMaskJob j{build[b], r.factor, false, 0.0};
        j.big = job_big(m.nd, f, r.factor, &j.rule_on);
        P.subs.back().jobs.push_back(j);
        f.has_M = true; f.has_U = f.has_U || m.two_level;
        f.mask_factor = r.factor; f.mask_big = j.rule_on; f.u_rows = m.u_rows;
      }
      P.subs.back().steps.push_back(i);
    } else {
      const SliceFacts &a = slices[r.s0];
      const SliceFacts *b = r.s1 >= 0 ? &slices[r.s1] : nullptr;
      double bound = -1.0;
      if (a.max_known && (!b || b->max_known)) bound = std::max(a.maxabs, b ? b->maxabs : 0.0) * (double)r.factor;
      const BatchTileRun p{(int)P.tile_steps.size(), 1, r.mode == MODE_TILE_CULL ? 1 : 0, knobs.tile_fan, tile_form(m.nd, m.robust, bound, knobs.tile_fan)};
      P.tile_steps.push_back(i);
      if (knobs.tile_walk && !P.runs.empty() && P.runs.back().cull == p.cull && P.runs.back().fan == p.fan) {
        P.runs.back().nsteps ++;
        P.runs.back().form = std::min(P.runs.back().form, p.form);
      } else P.runs.push_back(p);
    }
  }
  for (const BatchSub &sb : P.subs) { P.job_off.push_back(P.bytes); P.bytes += batch_round256(sb.jobs.size() * sizeof(ftkx::MaskJob)); }
  P.fields_off = P.bytes;
  for (const BatchSub &sb : P.subs) { P.step_base.push_back(P.nfields); P.nfields += sb.steps.size(); }
  P.tile_base = P.nfields;
  P.nfields += P.tile_steps.size();
  P.bytes += batch_round256(P.nfields * sizeof(ftkx::Fields));
  if ((P.nfields >> (64 - ftkx::kPassStepShift)) != 0) P.status = BATCH_TOO_MANY;      // a pass descriptor carries the request's index above kPassStepShift
  return P;
}

// upper bound of the tags a batch can emit -> number of key bits for the device sort (t_max: the latest timestep it sweeps)
inline int key_bits(int tag_mode, int nd, const long long *core_sz, const long long *dom_sz, int t_max)
{
  if (tag_mode == FTKX_TAG_REFERENCE) return 64;             // REFERENCE tags go through int32 products and may wrap to anything
  const bool work_index = tag_mode == FTKX_TAG_WORK_INDEX;
  long double bound = nd == 2 ? 12.0L : 60.0L;
  for (int d = 0; d < nd; d ++) bound *= (long double)(work_index ? core_sz[d] : dom_sz[d]);
  if (!work_index) bound *= (long double)(t_max + 2);
  int b = 1;
  while (b < 64 && ldexpl(1.0L, b) <= bound) b ++;
  return b;
}

// ---- what follows from the counters a batch left -----------------------------------------------------------------------------------------
// the four buffers a batch can overflow (records / survivors beyond capacity are only counted): as counts, and as capacities
struct BatchSizes { u64 hits, listed, refined, fragile; };
enum { BATCH_DONE = 0, BATCH_REPLAY_DENSE = 1, BATCH_GROW = 2, BATCH_GIVE_UP = 3 };
struct BatchVerdict { int what; BatchSizes want; };      // want: the capacities to replay with, none below the present one

// ftkx_sweep_collect, attempt 0, 1, ...: all fits -> done; else, the fifth time, give up; else, where most cells survive the cull (data
// whose quantised magnitudes can overflow the determinants almost everywhere, SURVEY H1/H3: a survivor list would be as large as the input),
// replay through the tile kernel, which stages each tile's vertices once and applies the same cull rule in LDS; else grow to what this
// batch needs and replay.  fast_cells: the cells of its MODE_FAST requests.
inline BatchVerdict overflow_verdict(const BatchSizes &n, const BatchSizes &cap, bool any_fast, u64 fast_cells, int attempt)
{
  BatchVerdict v{BATCH_DONE, cap};
  if (n.hits <= cap.hits && n.listed <= cap.listed && n.refined <= cap.refined && n.fragile <= cap.fragile) return v;
  if (attempt == 4) { v.what = BATCH_GIVE_UP; return v; }
  const bool truncated = n.listed > cap.listed || n.refined > cap.refined;      // then the hit count is a lower bound: leave generous room
  if (any_fast && truncated && (n.listed > fast_cells / 8 || n.refined * 8 > fast_cells / 8)) {
    v.what = BATCH_REPLAY_DENSE;
    if (n.hits > cap.hits) v.want.hits = 2 * n.hits + 1024;
    return v;
  }
  v.what = BATCH_GROW;
  auto room = [](u64 x) { return x + x / 8 + 1024; };
  if (n.fragile > cap.fragile) v.want.fragile = room(n.fragile);
  if (n.refined > cap.refined) v.want.refined = room(n.refined);
  if (n.listed > cap.listed) v.want.listed = room(n.listed);
  v.want.hits = std::max(cap.hits, std::max<u64>(room(n.hits), truncated ? 2 * n.hits + 1024 : 0));
  return v;
}

// ftkx_sweep_cull stops behind the cull: only the two lists can overflow, the survivor list doubles, and the fourth overflow is the last
inline BatchVerdict cull_verdict(u64 listed, u64 refined, u64 list_cap, u64 refine_cap, int attempt)
{
  BatchVerdict v{BATCH_DONE, BatchSizes{0, list_cap, refine_cap, 0}};
  if (listed <= list_cap && refined <= refine_cap) return v;
  if (attempt == 3) { v.what = BATCH_GIVE_UP; return v; }
  v.what = BATCH_GROW;
  if (refined > refine_cap) v.want.refined = refined + refined / 8 + 1024;
  if (listed > list_cap) v.want.listed = 2 * listed + 1024;
  return v;
}

}  // namespace ftkxh
