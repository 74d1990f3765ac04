// ftk_amd/csrc/ingest_steps.hpp as a shared object for tests/test_ingest_plan_host.py and tests/test_gpu_ingest_paths.py: the plan of one
// case as plain ints.  g++ -O2 -std=c++17 -fPIC -shared.
#include "../../ftk_amd/csrc/ingest_steps.hpp"

extern "C" {

// out[8]: reads_here, adopt, caller_waits, stage, copy, first, then_adjust, counters
void hc_ingest_plan(int f32, int planar, int smooth, int adjust, int on_device, int on_this_device, int must_own, int *out)
{
  const ftkx::IngestPlan p = ftkx::ingest_plan(f32 != 0, planar != 0, smooth != 0, adjust != 0, on_device, on_this_device != 0, must_own != 0);
  out[0] = p.reads_here; out[1] = p.adopt; out[2] = p.caller_waits; out[3] = (int)p.stage; out[4] = (int)p.copy; out[5] = (int)p.first;
  out[6] = p.then_adjust; out[7] = (int)p.counters;
}

int hc_ingest_asks_where(int f32, int planar, int smooth, int adjust, int on_device)
{
  return ftkx::ingest_asks_where(f32 != 0, planar != 0, smooth != 0, adjust != 0, on_device) ? 1 : 0;
}

// the enums' values, in the order of their declaration: stage (3), copy (3), kernel (5), counter bits (6)
void hc_ingest_names(int *out)
{
  const int v[17] = {ftkx::INGEST_STAGE_NONE, ftkx::INGEST_STAGE_F32, ftkx::INGEST_STAGE_POOLED, ftkx::INGEST_COPY_NONE, ftkx::INGEST_COPY_TO_DST, ftkx::INGEST_COPY_TO_STAGE,
                     ftkx::INGEST_NO_KERNEL, ftkx::INGEST_CONCAT, ftkx::INGEST_CONV, ftkx::INGEST_ADJUST, ftkx::INGEST_WIDEN,
                     ftkx::INGEST_CNT_FROM_FLOAT, ftkx::INGEST_CNT_IN_PLACE, ftkx::INGEST_CNT_OUT_OF_PLACE, ftkx::INGEST_CNT_F32_WIDENED, ftkx::INGEST_CNT_F32_DIRECT, ftkx::INGEST_CNT_PLANAR};
  for (int i = 0; i < 17; i ++) out[i] = v[i];
}

}  // extern "C"
