// ftk_amd/csrc/batch_plan.hpp as a shared object for tests/test_batch_plan_host.py (through tests/batch_cases.py): every decision of the
// host-driven batch as plain integers.  g++ -O2 -std=c++17 -Wall -Werror -fPIC -shared.
//
// A slice's facts travel as 8 words: has_M, has_U, sparse, mask_factor, mask_big, u_rows, max_known, maxabs (the double's bits).
// A plan comes back as words: status, refused, nsubs, nruns, ntile, fields_off, tile_base, nfields, bytes; per sub-batch job_off,
// step_base, njobs, nsteps, the jobs (slice, factor, rule_on, big's bits) and the steps; the tile requests; the runs (first, nsteps,
// cull, fan, form); the facts afterwards.
#include <cstring>

#ifndef __HIPCC__      // (sweep_params.hpp marks two helpers for both sides: nothing to g++)
#define __host__
#define __device__
#endif
#include "../../ftk_amd/csrc/batch_plan.hpp"

using namespace ftkxh;

namespace {
u64 bits_of(double v) { u64 b; memcpy(&b, &v, 8); return b; }
double double_of(u64 b) { double v; memcpy(&v, &b, 8); return v; }
SliceFacts facts_of(const u64 *w)
{
  SliceFacts f;
  f.has_M = w[0] != 0; f.has_U = w[1] != 0; f.sparse = w[2] != 0; f.mask_factor = w[3]; f.mask_big = w[4] != 0; f.u_rows = (int)w[5];
  f.max_known = w[6] != 0; f.maxabs = double_of(w[7]);
  return f;
}
void words_of(const SliceFacts &f, u64 *w)
{
  w[0] = f.has_M; w[1] = f.has_U; w[2] = f.sparse; w[3] = f.mask_factor; w[4] = f.mask_big; w[5] = (u64)f.u_rows; w[6] = f.max_known; w[7] = bits_of(f.maxabs);
}
}  // namespace

extern "C" {

// MODE_TILE, MODE_FAST, MODE_TILE_CULL; BATCH_OK, _SPARSE_CANNOT_SERVE, _TOO_MANY; BATCH_DONE, _REPLAY_DENSE, _GROW, _GIVE_UP;
// sizeof(MaskJob), sizeof(Fields), the bits a pass descriptor has for a request's index, FTKX_TAG_REFERENCE, FTKX_TAG_WORK_INDEX
void hc_batch_names(long long *out)
{
  const long long v[15] = {MODE_TILE, MODE_FAST, MODE_TILE_CULL, BATCH_OK, BATCH_SPARSE_CANNOT_SERVE, BATCH_TOO_MANY, BATCH_DONE, BATCH_REPLAY_DENSE, BATCH_GROW, BATCH_GIVE_UP,
                           (long long)sizeof(ftkx::MaskJob), (long long)sizeof(ftkx::Fields), 64 - ftkx::kPassStepShift, FTKX_TAG_REFERENCE, FTKX_TAG_WORK_INDEX};
  for (int i = 0; i < 15; i ++) out[i] = v[i];
}

int hc_overflow_free(int nd, double maxabs, u64 factor) { return overflow_free(nd, maxabs, factor) ? 1 : 0; }
double hc_big_threshold(int nd, u64 factor) { return big_threshold(nd, factor); }
int hc_pow2_factor(u64 factor) { return pow2_factor(factor) ? 1 : 0; }
int hc_masks_valid(int nd, const u64 *facts, u64 factor, int two_level, int u_rows) { return masks_valid(nd, facts_of(facts), factor, two_level != 0, u_rows) ? 1 : 0; }
double hc_job_big(int nd, const u64 *facts, u64 factor, int *rule_on)
{
  bool on = false;
  const double big = job_big(nd, facts_of(facts), factor, &on);
  *rule_on = on ? 1 : 0;
  return big;
}

int hc_request_mode(int exact_only, u64 factor, int nd, int robust, int dense_collects) { return request_mode(exact_only != 0, factor, nd, robust != 0, dense_collects); }
int hc_sparse_slice_refuses(int mode) { return sparse_slice_refuses(mode) ? 1 : 0; }
int hc_tile_form(int nd, int robust, double bound, int fan) { return tile_form(nd, robust != 0, bound, fan); }

// requests: (mode, s0, s1) per request; -> the words written, or -(the words needed) where `cap` is too small
long long hc_plan_batch(int nd, int robust, int two_level, int u_rows, int nreq, const int *requests, const u64 *factors, int nslices, const u64 *facts, int tile_walk, int tile_fan,
                        u64 *out, long long cap)
{
  std::vector<BatchRequest> req((size_t)nreq);
  for (int i = 0; i < nreq; i ++) req[i] = BatchRequest{requests[3 * i], requests[3 * i + 1], requests[3 * i + 2], factors[i]};
  std::vector<SliceFacts> sl((size_t)nslices);
  for (int i = 0; i < nslices; i ++) sl[i] = facts_of(facts + 8 * i);
  const std::vector<SliceFacts> before = sl;
  const BatchPlan P = plan_batch(BatchMesh{nd, robust != 0, two_level != 0, u_rows}, req, sl, BatchKnobs{tile_walk != 0, tile_fan});
  for (int i = 0; i < nslices; i ++) { u64 a[8], b[8]; words_of(before[i], a); words_of(sl[i], b); if (memcmp(a, b, sizeof(a))) return 0; }      // its input is const
  std::vector<u64> w = {(u64)P.status, (u64)(long long)P.refused, P.subs.size(), P.runs.size(), P.tile_steps.size(), P.fields_off, P.tile_base, P.nfields, P.bytes};
  for (size_t i = 0; i < P.subs.size(); i ++) {
    const BatchSub &sb = P.subs[i];
    // (a plan that was refused half way has no layout)
    w.insert(w.end(), {i < P.job_off.size() ? (u64)P.job_off[i] : 0, i < P.step_base.size() ? (u64)P.step_base[i] : 0, sb.jobs.size(), sb.steps.size()});
    for (const BatchMaskJob &j : sb.jobs) w.insert(w.end(), {(u64)j.slice, j.factor, (u64)j.rule_on, bits_of(j.big)});
    for (int s : sb.steps) w.push_back((u64)s);
  }
  for (int s : P.tile_steps) w.push_back((u64)s);
  for (const BatchTileRun &r : P.runs) w.insert(w.end(), {(u64)r.first, (u64)r.nsteps, (u64)r.cull, (u64)(long long)r.fan, (u64)(long long)r.form});
  for (const SliceFacts &f : P.facts) { u64 a[8]; words_of(f, a); w.insert(w.end(), a, a + 8); }
  if ((long long)w.size() > cap) return -(long long)w.size();
  memcpy(out, w.data(), w.size() * sizeof(u64));
  return (long long)w.size();
}

int hc_key_bits(int tag_mode, int nd, const long long *core_sz, const long long *dom_sz, int t_max) { return key_bits(tag_mode, nd, core_sz, dom_sz, t_max); }

// n, cap, want: hits, listed, refined, fragile
int hc_overflow_verdict(const u64 *n, const u64 *cap, int any_fast, u64 fast_cells, int attempt, u64 *want)
{
  const BatchVerdict v = overflow_verdict(BatchSizes{n[0], n[1], n[2], n[3]}, BatchSizes{cap[0], cap[1], cap[2], cap[3]}, any_fast != 0, fast_cells, attempt);
  want[0] = v.want.hits; want[1] = v.want.listed; want[2] = v.want.refined; want[3] = v.want.fragile;
  return v.what;
}

// want: listed, refined
int hc_cull_verdict(u64 listed, u64 refined, u64 list_cap, u64 refine_cap, int attempt, u64 *want)
{
  const BatchVerdict v = cull_verdict(listed, refined, list_cap, refine_cap, attempt);
  want[0] = v.want.listed; want[1] = v.want.refined;
  return v.what;
}

}  // extern "C"
