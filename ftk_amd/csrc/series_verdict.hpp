// The second half of a series pass (series.hip: series_complete) as decisions, free of the device: what the NEXT pass looks like after what
// this one reported (the tail policy), which way a completed pass leaves (the verdict), what a pass that overflowed grows its buffers to,
// and the path ftkx_series_last_path reports.  No HIP and no context: series.hip carries them out, and tests/test_series_verdict_host.py
// writes the rules out a second time on the CPU (tests/hostcheck/series_verdict.cpp).
#pragma once
#include "sweep_params.hpp"
#include "batch_plan.hpp"   // BatchSizes

namespace ftkxh {

// ---- how a completed pass leaves --------------------------------------------------------------------------------------------------------
enum pass_end {
  PASS_RECORDS = 0,      // the records are ready
  PASS_QUEUE_REST,       // queued in its short form, the fused tail declined: queue the rest of the chain and ask again with the new status
  PASS_PLANNED_BY_HOST,  // the host-driven batch sweeps the steps: the pass was never queued (found up front on the host)
  PASS_DECLINED,         // ... the fused tail declined and the rest cannot be queued any more
  PASS_REDO,             // ... a kernel raised a flag the device-driven form does not cover
  PASS_HALO_FULL         // a slab pass whose halo slice is needed as a whole: nothing was swept
};
struct pass_form { bool by_host, dist, short_chain; };
struct pass_verdict { pass_end end; bool grow; };      // grow: a buffer was too small -- series_growth before the batch
inline bool pass_to_batch(pass_end e) { return e == PASS_PLANNED_BY_HOST || e == PASS_DECLINED || e == PASS_REDO; }

constexpr unsigned long long kSeriesRedo = ftkx::SERIES_AMBIGUOUS | ftkx::SERIES_MASKS_INVALID | ftkx::SERIES_INF | ftkx::SERIES_OVERFLOW;

// open_behind: another pass is open behind this one; lists_own: the counters and survivor lists are still this pass's.  The order matters: a
// halo that is needed as a whole ends a slab pass whatever else it says, and a declined short chain is settled before the redo bits are
// looked at -- they are final only in the status the rest of the chain leaves (asked again then, with SERIES_TAIL_PENDING cleared).
inline pass_verdict series_verdict(unsigned long long status, const pass_form &f, bool open_behind, bool lists_own)
{
  if (f.by_host) return {PASS_PLANNED_BY_HOST, false};
  if (f.dist && (status & ftkx::SERIES_HALO_FULL)) return {PASS_HALO_FULL, false};
  if (f.short_chain && (status & ftkx::SERIES_TAIL_PENDING)) {
    // (the rest of the pass cannot be queued where the counters and lists are not this pass's any more -- the pass queued behind it has them
    // now, or the host-driven batch took them when the pass BEFORE this one fell back: two short-chain passes that both declined, completed
    // back to back.  It happens when sparse data turns dense)
    return {open_behind || !lists_own ? PASS_DECLINED : PASS_QUEUE_REST, false};
  }
  if (status & kSeriesRedo) return {PASS_REDO, (status & ftkx::SERIES_OVERFLOW) != 0};   // (grown here: the batch would find out the same way, one replay later)
  return {PASS_RECORDS, false};
}

// what was too small, grown by an eighth and 1024 (the series pass's own number, not overflow_verdict's rule for hits); the rest as it is
inline BatchSizes series_growth(const BatchSizes &n, const BatchSizes &cap)
{
  auto grown = [](u64 x, u64 have) { return x > have ? x + x / 8 + 1024 : have; };
  return {grown(n.hits, cap.hits), grown(n.listed, cap.listed), grown(n.refined, cap.refined), grown(n.fragile, cap.fragile)};
}

// ftkx_series_last_path of a pass that returned its own records: 4 the one-launch pass, 5 a split pass, 2 the fused tail finished it, 1 the
// kernel chain; order_filled: its records came through the bucket chain (ftkx_debug_series_order)
struct series_path { int path; bool order_filled; };
inline series_path series_path_of(unsigned long long status, bool split)
{
  return {(status & ftkx::SERIES_ONE) ? 4 : split ? 5 : (status & ftkx::SERIES_EARLY) ? 2 : 1, !(status & (ftkx::SERIES_ONE | ftkx::SERIES_EARLY))};
}

// ---- the tail policy: what the passes completed so far say about the form of the next one ----------------------------------------------------
constexpr u64 kSparseMaxRecords = 1024;        // records the fused tail's last workgroup orders (series_kernels.hip: kSmallRank)
constexpr u64 kFusedMaxListed = 4 * 2048ull;   // entries of the pass's own list up to which the fused tail is worth launching (four rounds of its 256 x 8)
constexpr int kSitOutPasses = 16;              // passes a form that has just declined is not tried for
constexpr int kLateStreak = 2;                 // late declines in a row after which the fused tail sits out

struct tail_policy {
  bool short_chain = false;   // the last pass was finished by the fused tail kernel: the next one is queued without the kernels behind it
  bool sparse = false;        // the last pass had few survivors and records (the fused tail's range): a pass whose mask kernel is long enough is split
  int skip_small = 0;         // passes for which the fused tail kernel is not launched (the data was hit-dense a moment ago)
  int late_streak = 0;        // consecutive passes the fused tail declined late
  int one_off = 0;            // asks for which the one-launch form is not tried (it declined a moment ago)
};

// The tail of the pass being queued (hooks: FTKX_SERIES_HOOKS small / short): small_now = the fused tail kernel is launched, short_chain =
// ... without the kernels behind it.  Decided before skip_small counts down, which it does for every pass.  A split pass takes the chain:
// the fused tail does not fit next to a mask kernel.
struct tail_plan { bool small_now, short_chain; };
inline tail_plan tail_plan_next(tail_policy &K, bool small_on, bool short_on, bool to_device, bool split)
{
  const bool small_now = small_on && K.skip_small == 0 && !to_device && !split;
  const tail_plan t{small_now, small_now && short_on && K.short_chain};
  if (K.skip_small > 0) K.skip_small --;
  return t;
}

// may the one-launch form be tried (hook: FTKX_SERIES_HOOKS one)?  Never for a slab pass, whose asks do not count either.
inline bool tail_one_allowed(tail_policy &K, bool one_on, bool dist)
{
  if (one_on && !dist && K.one_off == 0) return true;
  if (K.one_off > 0 && !dist) K.one_off --;
  return false;
}

inline bool tail_sparse(const tail_policy &K) { return K.sparse; }

struct pass_facts {
  unsigned long long status;
  bool one, split, two_level;
  u64 records, list_peak, refine_peak;      // SR_NHITS, CNT_LIST_PEAK, CNT_REFINE_PEAK
};

// the status and the counters the verdict and the policy go by, out of a pass's results block as it stands; returns the status
inline unsigned long long pass_read(pass_facts &p, const u64 *R)
{
  p.records = R[ftkx::SR_NHITS]; p.list_peak = R[ftkx::SR_COUNTERS + ftkx::CNT_LIST_PEAK]; p.refine_peak = R[ftkx::SR_COUNTERS + ftkx::CNT_REFINE_PEAK];
  return p.status = R[ftkx::SR_STATUS];
}

inline void tail_learn(tail_policy &K, pass_end end, const pass_facts &p)
{
  if (end == PASS_QUEUE_REST || end == PASS_PLANNED_BY_HOST) return;      // (nothing has come back yet / nothing was queued)
  if (end != PASS_RECORDS) {
    K.short_chain = false;
    if (end != PASS_REDO) return;
    K.sparse = false;
    if (p.one) K.one_off = kSitOutPasses;      // (more hits than a workgroup parks, or the device was not this kernel's alone: the usual way for a while)
    return;
  }
  const bool early = (p.status & ftkx::SERIES_EARLY) != 0;
  const u64 own_peak = p.two_level ? p.refine_peak : p.list_peak;
  if (!p.one && !p.split) K.short_chain = early;      // (a split pass says nothing about the fused tail)
  if (!p.one) K.sparse = early || (p.records <= kSparseMaxRecords && own_peak <= kFusedMaxListed);
  // (far more survivors than the fused kernel takes: finding nothing to do costs its 256 workgroups of 256-VGPR wavefronts ~15 us)
  if (!early && own_peak > kFusedMaxListed) K.skip_small = kSitOutPasses;
  // (few coarse cells, many records in them: the fused tail declined late, tens of microseconds lost.  Twice in a row: the series is like that)
  K.late_streak = (p.status & ftkx::SERIES_LATE_DECLINE) ? K.late_streak + 1 : 0;
  if (K.late_streak >= kLateStreak) K.skip_small = kSitOutPasses;
}

// the open passes were abandoned (ftkx_sweep_series_abort): nothing is known of the data's form; the counters run on
inline void tail_abort(tail_policy &K) { K.short_chain = false; K.sparse = false; }

}  // namespace ftkxh
