// ftk_amd/csrc/ingest_steps.hpp's plan for a vector snapshot under ftkx_set_vector_smoothing, as plain ints, for
// tests/test_vec_smooth_plan_host.py.  g++ -O2 -std=c++17 -fPIC -shared.
#include "../../ftk_amd/csrc/ingest_steps.hpp"

extern "C" {

// out[8]: reads_here, adopt, caller_waits, stage, copy, first, then_adjust, counters
void hc_vec_smooth_plan(int f32, int planar, int adjust, int on_device, int on_this_device, int *out)
{
  const ftkx::IngestPlan p = ftkx::vec_smooth_ingest_plan(f32 != 0, planar != 0, adjust != 0, on_device, on_this_device != 0);
  out[0] = p.reads_here; out[1] = p.adopt; out[2] = p.caller_waits; out[3] = (int)p.stage; out[4] = (int)p.copy; out[5] = (int)p.first;
  out[6] = p.then_adjust; out[7] = (int)p.counters;
}

int hc_vec_smooth_asks_where(int planar, int on_device) { return ftkx::vec_smooth_asks_where(planar != 0, on_device) ? 1 : 0; }

// stage (3), copy (3), the kernel, the counter bits the plan may name (4)
void hc_vec_smooth_names(int *out)
{
  const int v[11] = {ftkx::INGEST_STAGE_NONE, ftkx::INGEST_STAGE_F32, ftkx::INGEST_STAGE_POOLED, ftkx::INGEST_COPY_NONE, ftkx::INGEST_COPY_TO_DST, ftkx::INGEST_COPY_TO_STAGE,
                     ftkx::INGEST_CONV_VEC, ftkx::INGEST_CNT_IN_PLACE, ftkx::INGEST_CNT_VEC_INTERLEAVED, ftkx::INGEST_CNT_VEC_PLANAR, ftkx::INGEST_CNT_VEC_F32};
  for (int i = 0; i < 11; i ++) out[i] = v[i];
}

}  // extern "C"
