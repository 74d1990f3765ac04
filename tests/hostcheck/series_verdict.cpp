// ftk_amd/csrc/series_verdict.hpp without a GPU: which way a completed series pass leaves, what an overflowed pass grows its buffers to,
// the path it reports, and the tail policy followed step by step through plans and completions.  The rules are stated HERE a second time,
// in numbers and tables of their own, and the header is held against them.  A program of its own: tests/test_series_verdict_host.py
// compiles and runs it, under ASan + UBSan where they are installed.
#include <cstdio>
#include <cstdlib>

#ifndef __HIPCC__      // (sweep_params.hpp marks two helpers for both sides: nothing to g++)
#define __host__
#define __device__
#endif
#include "../../ftk_amd/csrc/series_verdict.hpp"

using namespace ftkxh;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                                                     \
  do {                                                                                       \
    if (!(cond)) { failures ++; if (failures < 40) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } \
  } while (0)

// the status bits by their values (include/ftkx.h documents them; the kernels store them)
constexpr unsigned long long AMBIGUOUS = 1, MASKS_INVALID = 2, INF = 4, OVERFLOW_ = 8, FIX_ORDER = 16, EARLY = 32, LATE_DECLINE = 64, TAIL_PENDING = 128,
                             HALO_FULL = 256, ONE = 512;
static_assert(AMBIGUOUS == ftkx::SERIES_AMBIGUOUS && MASKS_INVALID == ftkx::SERIES_MASKS_INVALID && INF == ftkx::SERIES_INF && OVERFLOW_ == ftkx::SERIES_OVERFLOW &&
              FIX_ORDER == ftkx::SERIES_FIX_ORDER && EARLY == ftkx::SERIES_EARLY && LATE_DECLINE == ftkx::SERIES_LATE_DECLINE &&
              TAIL_PENDING == ftkx::SERIES_TAIL_PENDING && HALO_FULL == ftkx::SERIES_HALO_FULL && ONE == ftkx::SERIES_ONE, "the status word");
const unsigned long long kDeciding[6] = {AMBIGUOUS, MASKS_INVALID, INF, OVERFLOW_, TAIL_PENDING, HALO_FULL};
const unsigned long long kBystanders[4] = {EARLY, ONE, LATE_DECLINE, FIX_ORDER};

unsigned long long pick(const unsigned long long *bits, int nbits, unsigned subset)
{
  unsigned long long s = 0;
  for (int b = 0; b < nbits; b ++) if (subset & (1u << b)) s |= bits[b];
  return s;
}

// ---- the verdict ---------------------------------------------------------------------------------------------------------------------------
enum { RECORDS, REST, BATCH, HALO };      // the four outcomes
int outcome_of(pass_end e) { return e == PASS_RECORDS ? RECORDS : e == PASS_QUEUE_REST ? REST : e == PASS_HALO_FULL ? HALO : BATCH; }

// The rule, as the issue of this header words it.  A pass the host planned for the batch goes there.  Otherwise: a slab pass whose halo is
// needed as a whole fails for it, whatever else is set.  Otherwise a pass queued SHORT whose fused tail declined: the rest is queued while
// nobody else can have touched the lists, else the batch (which grows nothing).  Otherwise any of the four redo bits: the batch, growing
// first exactly when OVERFLOW is among them.  Otherwise the records.
struct Want { int outcome; bool grow; pass_end why; };
Want want_of(unsigned long long s, bool by_host, bool dist, bool short_chain, bool open_behind, bool lists_own)
{
  const bool halo = dist && (s & 256), declined = short_chain && (s & 128), redo = (s & 15) != 0;
  if (by_host) return {BATCH, false, PASS_PLANNED_BY_HOST};
  if (halo) return {HALO, false, PASS_HALO_FULL};
  if (declined && !open_behind && lists_own) return {REST, false, PASS_QUEUE_REST};
  if (declined) return {BATCH, false, PASS_DECLINED};
  if (redo) return {BATCH, (s & 8) != 0, PASS_REDO};
  return {RECORDS, false, PASS_RECORDS};
}

void check_verdict()
{
  long cases = 0, rests = 0;
  for (unsigned d = 0; d < 64; d ++)
    for (unsigned form = 0; form < 32; form ++) {
      const bool by_host = form & 1, dist = form & 2, short_chain = form & 4, open_behind = form & 8, lists_own = form & 16;
      const pass_form f{by_host, dist, short_chain};
      const unsigned long long s = pick(kDeciding, 6, d);
      const Want w = want_of(s, by_host, dist, short_chain, open_behind, lists_own);
      for (unsigned y = 0; y < 16; y ++) {      // (the bits that say HOW the records were made decide nothing here)
        const pass_verdict v = series_verdict(s | pick(kBystanders, 4, y), f, open_behind, lists_own);
        CHECK(outcome_of(v.end) == w.outcome && v.grow == w.grow && v.end == w.why, "status %llx + %llx form %u: end %d grow %d, wanted outcome %d grow %d", s,
              pick(kBystanders, 4, y), form, (int)v.end, (int)v.grow, w.outcome, (int)w.grow);
        CHECK(pass_to_batch(v.end) == (w.outcome == BATCH), "status %llx form %u: pass_to_batch", s, form);
        cases ++;
      }
      if (w.outcome != REST) continue;
      // after the re-queue: whatever the rest of the chain reports, judged with TAIL_PENDING cleared -- never another re-queue, never
      // "declined"; the redo bits still lead to the batch
      rests ++;
      for (unsigned d2 = 0; d2 < 64; d2 ++) {
        const unsigned long long s2 = pick(kDeciding, 6, d2) & ~TAIL_PENDING;
        const pass_verdict v2 = series_verdict(s2, f, open_behind, lists_own);
        const bool halo2 = dist && (s2 & HALO_FULL);
        const int w2 = halo2 ? HALO : (s2 & 15) ? BATCH : RECORDS;
        CHECK(outcome_of(v2.end) == w2 && v2.grow == (!halo2 && (s2 & 8) != 0), "second status %llx form %u: end %d grow %d", s2, form, (int)v2.end, (int)v2.grow);
        CHECK(v2.end != PASS_QUEUE_REST && v2.end != PASS_DECLINED, "second status %llx form %u asks for the rest again", s2, form);
      }
    }
  CHECK(cases == 64 * 32 * 16 && rests > 0, "%ld cases, %ld re-queues", cases, rests);
  // the named ones, spelled out
  const pass_form chain{false, false, false}, shortf{false, false, true}, slab_short{false, true, true}, slab{false, true, false};
  CHECK(series_verdict(HALO_FULL | TAIL_PENDING, slab_short, false, true).end == PASS_HALO_FULL, "HALO_FULL wins over TAIL_PENDING");
  CHECK(series_verdict(HALO_FULL | OVERFLOW_, slab, false, true).end == PASS_HALO_FULL, "HALO_FULL wins over the redo bits");
  CHECK(series_verdict(HALO_FULL | TAIL_PENDING, shortf, false, true).end == PASS_QUEUE_REST, "HALO_FULL means nothing outside a slab pass");
  CHECK(series_verdict(HALO_FULL, chain, false, true).end == PASS_RECORDS, "HALO_FULL means nothing outside a slab pass");
  CHECK(series_verdict(TAIL_PENDING, shortf, false, true).end == PASS_QUEUE_REST, "the rest is queued");
  CHECK(series_verdict(TAIL_PENDING, shortf, true, true).end == PASS_DECLINED, "a pass open behind: the batch");
  CHECK(series_verdict(TAIL_PENDING, shortf, false, false).end == PASS_DECLINED, "the lists gone: the batch");
  CHECK(!series_verdict(TAIL_PENDING | OVERFLOW_, shortf, true, true).grow, "a declined pass grows nothing");
  CHECK(series_verdict(TAIL_PENDING, chain, true, false).end == PASS_RECORDS, "TAIL_PENDING on a pass that was not queued short");
  CHECK(series_verdict(TAIL_PENDING | INF, chain, false, true).end == PASS_REDO, "TAIL_PENDING on a pass that was not queued short");
  for (unsigned r = 1; r < 16; r ++) {
    const pass_verdict v = series_verdict(r, chain, false, true);
    CHECK(v.end == PASS_REDO && v.grow == ((r & 8) != 0), "redo bits %u: grow %d", r, (int)v.grow);
  }
}

// ---- the growth ----------------------------------------------------------------------------------------------------------------------------
void check_growth()
{
  const u64 cap[4] = {65536, 1u << 20, (1u << 20) + 7, 4096};
  for (unsigned over = 0; over < 16; over ++) {
    u64 n[4], want[4];
    for (int i = 0; i < 4; i ++) {
      n[i] = cap[i] + ((over >> i) & 1);      // at capacity: it fits; one over: it does not
      want[i] = ((over >> i) & 1) ? n[i] + n[i] / 8 + 1024 : cap[i];
    }
    const BatchSizes g = series_growth(BatchSizes{n[0], n[1], n[2], n[3]}, BatchSizes{cap[0], cap[1], cap[2], cap[3]});
    CHECK(g.hits == want[0] && g.listed == want[1] && g.refined == want[2] && g.fragile == want[3], "over %u: %llu %llu %llu %llu", over, (unsigned long long)g.hits,
          (unsigned long long)g.listed, (unsigned long long)g.refined, (unsigned long long)g.fragile);
  }
  const BatchSizes g = series_growth(BatchSizes{0, 5, 0, 1}, BatchSizes{0, 4, 0, 0});
  CHECK(g.hits == 0 && g.listed == 5 + 0 + 1024 && g.refined == 0 && g.fragile == 1025, "small counts");
  CHECK(series_growth(BatchSizes{65537, 0, 0, 0}, BatchSizes{65536, 0, 0, 0}).hits == 65537 + 8192 + 1024, "an eighth and 1024, not the batch's rule");
}

// ---- the reported path ---------------------------------------------------------------------------------------------------------------------
void check_path()
{
  const unsigned long long all[10] = {AMBIGUOUS, MASKS_INVALID, INF, OVERFLOW_, FIX_ORDER, EARLY, LATE_DECLINE, TAIL_PENDING, HALO_FULL, ONE};
  for (unsigned sub = 0; sub < 1024; sub ++)
    for (int split = 0; split < 2; split ++) {
      const unsigned long long s = pick(all, 10, sub);
      int want = 1;
      if (s & 32) want = 2;
      if (split) want = 5;
      if (s & 512) want = 4;
      const series_path p = series_path_of(s, split != 0);
      CHECK(p.path == want, "status %llx split %d: path %d, wanted %d", s, split, p.path, want);
      CHECK(p.order_filled == !((s & 512) || (s & 32)), "status %llx split %d: order block", s, split);
    }
}

// ---- the tail policy -----------------------------------------------------------------------------------------------------------------------
bool same(const tail_policy &a, bool short_chain, bool sparse, int skip_small, int late_streak, int one_off)
{
  return a.short_chain == short_chain && a.sparse == sparse && a.skip_small == skip_small && a.late_streak == late_streak && a.one_off == one_off;
}
#define CHECK_POLICY(K, sc, sp, sk, ls, oo, what) \
  CHECK(same(K, sc, sp, sk, ls, oo), "%s: short_chain %d sparse %d skip_small %d late_streak %d one_off %d", what, (int)(K).short_chain, (int)(K).sparse, (K).skip_small, (K).late_streak, (K).one_off)

// a pass that returned its own records
void records(tail_policy &K, unsigned long long status, bool one, bool split, bool two_level, u64 nrec, u64 list_peak, u64 refine_peak)
{
  tail_learn(K, PASS_RECORDS, pass_facts{status, one, split, two_level, nrec, list_peak, refine_peak});
}
void ended(tail_policy &K, pass_end how, bool one) { tail_learn(K, how, pass_facts{OVERFLOW_ | EARLY | LATE_DECLINE, one, false, false, 3, 100000, 100000}); }
bool plan_is(tail_policy &K, bool small_on, bool short_on, bool to_device, bool split, bool want_small, bool want_short)
{
  const tail_plan t = tail_plan_next(K, small_on, short_on, to_device, split);
  return t.small_now == want_small && t.short_chain == want_short;
}

void check_policy()
{
  {      // (a) the short chain and who takes it
    tail_policy K;
    CHECK(plan_is(K, true, true, false, false, true, false), "(a) a fresh context launches the fused tail with the chain behind it");
    records(K, EARLY, false, false, true, 12, 0, 40);
    CHECK_POLICY(K, true, true, 0, 0, 0, "(a) after an EARLY pass");
    CHECK(plan_is(K, true, true, false, true, false, false), "(a) a split pass takes the chain");
    records(K, 0, false, true, true, 12, 0, 40);      // (that split pass, completed by the chain: it says nothing about the fused tail)
    CHECK(K.short_chain, "(a) a split pass cleared the short chain");
    CHECK(plan_is(K, true, true, true, false, false, false), "(a) a pass whose records stay on the device takes the chain");
    CHECK(K.short_chain, "(a) planning a to_device pass cleared the short chain");
    CHECK(plan_is(K, true, false, false, false, true, false), "(a) hook short off");
    CHECK(plan_is(K, false, true, false, false, false, false), "(a) hook small off");
    CHECK(plan_is(K, true, true, false, false, true, true), "(a) the next unsplit, host-bound pass is queued short");
    records(K, 0, false, false, true, 12, 0, 40);
    CHECK(!K.short_chain && plan_is(K, true, true, false, false, true, false), "(a) a pass the chain finished ends it");
    records(K, EARLY, true, false, true, 12, 0, 40);
    CHECK(!K.short_chain, "(a) a one-launch pass says nothing about the fused tail");
  }
  {      // (b) a list too long for the fused tail: sixteen plans sat out
    tail_policy K;
    records(K, 0, false, false, false, 5000, 8192, 0);
    CHECK_POLICY(K, false, false, 0, 0, 0, "(b) a peak of 8192");
    records(K, EARLY, false, false, false, 5000, 8193, 0);
    CHECK(K.skip_small == 0, "(b) 8193 with EARLY");
    records(K, 0, false, false, true, 5000, 1u << 20, 8192);
    CHECK(K.skip_small == 0, "(b) two-level: the refine peak counts, not the list's");
    records(K, 0, false, false, true, 5000, 0, 8193);
    CHECK(K.skip_small == 16, "(b) two-level: a refine peak of 8193");
    K = tail_policy();
    records(K, 0, false, false, false, 5000, 8193, 1);
    CHECK_POLICY(K, false, false, 16, 0, 0, "(b) a peak of 8193");
    for (int i = 0; i < 16; i ++) {
      const bool split = i % 3 == 1;                       // (split plans count among the sixteen)
      CHECK(plan_is(K, true, true, false, split, false, false), "(b) plan %d of the sixteen launched the fused tail", i + 1);
      CHECK(K.skip_small == 15 - i, "(b) plan %d: %d left", i + 1, K.skip_small);
    }
    CHECK(plan_is(K, true, true, false, false, true, false) && K.skip_small == 0, "(b) the seventeenth plan");
  }
  {      // (c) late declines
    tail_policy K;
    records(K, LATE_DECLINE, false, false, true, 2000, 0, 50);
    CHECK_POLICY(K, false, false, 0, 1, 0, "(c) one late decline");
    records(K, 0, false, false, true, 2000, 0, 50);
    CHECK_POLICY(K, false, false, 0, 0, 0, "(c) a pass in between");
    records(K, LATE_DECLINE, false, false, true, 2000, 0, 50);
    CHECK_POLICY(K, false, false, 0, 1, 0, "(c) one again");
    records(K, LATE_DECLINE, false, false, true, 2000, 0, 50);
    CHECK_POLICY(K, false, false, 16, 2, 0, "(c) two in a row");
  }
  {      // (d) the one-launch form after a redo
    tail_policy K;
    CHECK(tail_one_allowed(K, true, false) && !tail_one_allowed(K, false, false) && !tail_one_allowed(K, true, true) && K.one_off == 0, "(d) a fresh context");
    ended(K, PASS_REDO, false);
    CHECK(K.one_off == 0, "(d) a redo of another form");
    ended(K, PASS_REDO, true);
    CHECK(K.one_off == 16, "(d) a redo of a one-launch pass");
    int asks = 0;
    for (int i = 0; i < 16; i ++) {
      CHECK(!tail_one_allowed(K, true, true) && !tail_one_allowed(K, false, true) && K.one_off == 16 - i, "(d) a slab ask counted (%d)", i);
      CHECK(!tail_one_allowed(K, i % 4 != 2, false), "(d) ask %d was let through", i + 1);      // (every fourth with the hook off: it counts)
      asks ++;
      CHECK(K.one_off == 16 - asks, "(d) ask %d: %d left", asks, K.one_off);
    }
    CHECK(!tail_one_allowed(K, true, true) && tail_one_allowed(K, true, false) && K.one_off == 0, "(d) the seventeenth ask");
  }
  {      // (e) sparse
    for (int two_level = 0; two_level < 2; two_level ++)
      for (u64 nrec = 1024; nrec <= 1025; nrec ++)
        for (u64 peak = 8192; peak <= 8193; peak ++)
          for (int early = 0; early < 2; early ++) {
            tail_policy K;
            records(K, early ? EARLY : 0, false, false, two_level != 0, nrec, two_level ? 1u << 22 : peak, two_level ? peak : 1u << 22);
            CHECK(K.sparse == (early || (nrec == 1024 && peak == 8192)), "(e) two_level %d records %llu peak %llu early %d: sparse %d", two_level, (unsigned long long)nrec,
                  (unsigned long long)peak, early, (int)K.sparse);
            CHECK(tail_sparse(K) == K.sparse, "(e) the reading");
          }
    tail_policy K;
    records(K, 0, false, true, false, 3, 9, 0);            // (a split pass does say)
    CHECK(K.sparse, "(e) a split pass");
    records(K, 0, true, false, false, 50000, 90000, 0);
    CHECK(K.sparse, "(e) a dense one-launch pass cleared it");
    ended(K, PASS_REDO, false);
    CHECK(!K.sparse, "(e) a redo");
    records(K, EARLY | ONE, true, false, false, 3, 9, 0);
    CHECK(!K.sparse, "(e) a sparse one-launch pass set it");
    K.sparse = true;
    tail_abort(K);
    CHECK(!K.sparse, "(e) abort");
  }
  {      // (f) the ways out without records, (g) abort: from a state with every member set
    const tail_policy full{true, true, 5, 1, 3};
    tail_policy K = full;
    ended(K, PASS_HALO_FULL, true);
    CHECK_POLICY(K, false, true, 5, 1, 3, "(f) the halo needed as a whole");
    K = full; ended(K, PASS_DECLINED, true);
    CHECK_POLICY(K, false, true, 5, 1, 3, "(f) declined, the lists gone");
    K = full; ended(K, PASS_REDO, false);
    CHECK_POLICY(K, false, false, 5, 1, 3, "(f) redo");
    K = full; ended(K, PASS_REDO, true);
    CHECK_POLICY(K, false, false, 5, 1, 16, "(f) redo of a one-launch pass");
    K = full; ended(K, PASS_PLANNED_BY_HOST, true);
    CHECK_POLICY(K, true, true, 5, 1, 3, "(f) a pass the host planned for the batch");
    K = full; ended(K, PASS_QUEUE_REST, true);
    CHECK_POLICY(K, true, true, 5, 1, 3, "(f) the rest still to be queued");
    K = full; tail_abort(K);
    CHECK_POLICY(K, false, false, 5, 1, 3, "(g) abort");
  }
}

void check_read()
{
  u64 R[ftkx::SR_HEAD];
  for (int i = 0; i < ftkx::SR_HEAD; i ++) R[i] = 1000 + (u64)i;
  pass_facts p{0, true, false, true, 0, 0, 0};
  CHECK(pass_read(p, R) == 1000 && p.status == 1000 && p.records == 1002 && p.list_peak == 1007 + 4 && p.refine_peak == 1007 + 6 && p.one && !p.split && p.two_level, "pass_read");
}

}  // namespace

int main()
{
  check_verdict();
  check_growth();
  check_path();
  check_policy();
  check_read();
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("series_verdict checks complete\n");
  return 0;
}
