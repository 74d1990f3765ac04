// ftk_amd/csrc/ingest_steps.hpp's plan for narrow sources as a shared object for tests/test_narrow_plan_host.py: the plan of one case as
// plain ints.  g++ -O2 -std=c++17 -fPIC -shared.
#include "../../ftk_amd/csrc/ingest_steps.hpp"

extern "C" {

// out[7]: reads_here, staged, adopt, caller_waits, to_pooled, then_adjust, counters
void hc_narrow_ingest_plan(int smooth, int adjust, int on_device, int on_this_device, int *out)
{
  const ftkx::NarrowIngestPlan p = ftkx::narrow_ingest_plan(smooth != 0, adjust != 0, on_device, on_this_device != 0);
  out[0] = p.reads_here; out[1] = p.staged; out[2] = p.adopt; out[3] = p.caller_waits; out[4] = p.to_pooled; out[5] = p.then_adjust; out[6] = (int)p.counters;
}

int hc_narrow_ingest_asks_where(int on_device) { return ftkx::narrow_ingest_asks_where(on_device) ? 1 : 0; }

// the counter bits a narrow push may and may not move: in_place, then f32_widened | f32_direct | planar | from_float | out_of_place
void hc_narrow_counter_bits(int *out)
{
  out[0] = ftkx::INGEST_CNT_IN_PLACE;
  out[1] = ftkx::INGEST_CNT_F32_WIDENED | ftkx::INGEST_CNT_F32_DIRECT | ftkx::INGEST_CNT_PLANAR | ftkx::INGEST_CNT_FROM_FLOAT | ftkx::INGEST_CNT_OUT_OF_PLACE;
}

}  // extern "C"
