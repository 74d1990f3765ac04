// One kernel `reps` times back to back on the context's stream, a pair of events around every launch: what the bare-kernel entry points
// and the ftkx_debug_*_relaunch profiling aids (tools/*_time.py) share.  Argument checks, and whatever has to be on the device before the
// first launch, stay with the callers.
#pragma once
#include "ctx.hpp"

namespace ftkxh {

// launch(): queues the kernel once on c->stream.  ms null (reps == 1): no events -- one launch, a check, and the stream is waited for (the
// caller may read what the kernel wrote).  Otherwise ms[i] is the time of launch i.  After an error the stream is waited for all the same.
template <class F> int timed_relaunch(ftkx_ctx *c, int reps, double *ms, F launch)
{
  std::vector<hipEvent_t> ev(ms ? 2 * (size_t)reps : 0, nullptr);
  auto run = [&]() -> int {
    for (hipEvent_t &e : ev) HIP_TRY(c, hipEventCreate(&e));
    for (int i = 0; i < reps; i ++) {
      if (ms) HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i], c->stream));
      launch();
      if (ms) HIP_TRY(c, hipEventRecord(ev[2 * (size_t)i + 1], c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; ms && i < reps; i ++) { float t = 0; HIP_TRY(c, hipEventElapsedTime(&t, ev[2 * (size_t)i], ev[2 * (size_t)i + 1])); ms[i] = t; }
    return FTKX_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  return rc;
}

}  // namespace ftkxh
