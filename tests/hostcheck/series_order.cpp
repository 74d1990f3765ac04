// ftk_amd/csrc/series_order.hpp without a GPU: the bucket geometry of the device-driven pass's ordering step, and the host's repair of
// the buckets that were too full to rank on the device (SERIES_FIX_ORDER), against std::sort.  What the repair is handed is stated HERE
// as the rank kernel leaves it: runs of records, every tag of a run below every tag of the next, a run either in order (ranked on the
// device) or in any order (left to the host).  A program of its own: tests/test_series_order_host.py compiles and runs it, under
// ASan + UBSan where they are installed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../../ftk_amd/csrc/series_order.hpp"

using namespace ftkxh;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                                                     \
  do {                                                                                       \
    if (!(cond)) { failures ++; if (failures < 40) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } \
  } while (0)

struct Rec { double x; unsigned long long tag; int id; };   // (the tag is not the first member, and a record carries more than its tag)

// the repair on a copy of `tags` (one guard record on either side, which it must not touch) against std::sort
void check_repair(const std::vector<unsigned long long> &tags, const char *what)
{
  const size_t n = tags.size();
  std::vector<Rec> h(n + 2);
  h[0] = Rec{-1.0, ~0ull, -1}; h[n + 1] = Rec{-1.0, 0ull, -2};      // (guards that WOULD be pulled in if the repair looked past its ends)
  for (size_t i = 0; i < n; i ++) h[i + 1] = Rec{(double)tags[i], tags[i], (int)i};
  series_fix_order(h.data() + 1, n);
  std::vector<unsigned long long> want(tags);
  std::sort(want.begin(), want.end());
  bool same = true, whole = true;
  std::vector<char> seen(n, 0);
  for (size_t i = 0; i < n; i ++) {
    const Rec &r = h[i + 1];
    same = same && r.tag == want[i];
    // every record is one of the input's, once, with its other members
    whole = whole && r.id >= 0 && (size_t)r.id < n && !seen[(size_t)r.id] && tags[(size_t)r.id] == r.tag && r.x == (double)r.tag;
    if (r.id >= 0 && (size_t)r.id < n) seen[(size_t)r.id] = 1;
  }
  CHECK(same, "%s: n %zu not in tag order", what, n);
  CHECK(whole, "%s: n %zu records lost, doubled or torn", what, n);
  CHECK(h[0].id == -1 && h[0].tag == ~0ull && h[n + 1].id == -2 && h[n + 1].tag == 0ull, "%s: n %zu wrote outside the records", what, n);
}

// runs[i] = (length, shuffled?): tags ascending from run to run with gaps; `dups`: tags inside a run may repeat
std::vector<unsigned long long> concat_runs(const std::vector<std::pair<size_t, bool>> &runs, std::mt19937_64 &rng, bool dups)
{
  std::vector<unsigned long long> out;
  unsigned long long next = rng() % 5;
  for (const auto &r : runs) {
    std::vector<unsigned long long> t(r.first);
    for (auto &v : t) { v = next; if (!dups || rng() % 3) next += 1 + rng() % 3; }
    if (dups && !t.empty() && t.back() == next) next ++;   // (the next run starts above this one)
    if (r.second) std::shuffle(t.begin(), t.end(), rng);
    out.insert(out.end(), t.begin(), t.end());
  }
  return out;
}

void check_repairs()
{
  check_repair({}, "n = 0");
  check_repair({7}, "n = 1");
  check_repair({7, 7}, "two equal");
  check_repair({9, 7}, "two, swapped");
  // every permutation of up to 8 distinct tags, and of 8 tags with repeats
  for (size_t n = 2; n <= 8; n ++) {
    std::vector<unsigned long long> t(n);
    std::iota(t.begin(), t.end(), 10ull);
    do check_repair(t, "permutation"); while (std::next_permutation(t.begin(), t.end()));
  }
  {
    std::vector<unsigned long long> t = {1, 1, 2, 3, 3, 3, 5, 8};
    do check_repair(t, "permutation with repeats"); while (std::next_permutation(t.begin(), t.end()));
  }
  std::mt19937_64 rng(20240607ull);
  // random concatenations of runs, each in order or shuffled
  for (int it = 0; it < 20000; it ++) {
    std::vector<std::pair<size_t, bool>> runs(1 + rng() % 9);
    for (auto &r : runs) r = {(size_t)(rng() % 12), (rng() & 1) != 0};
    check_repair(concat_runs(runs, rng, (it & 1) != 0), "random runs");
  }
  // fat runs -- buckets past rank_max -- first, last, side by side, alone, and between thin ones that are in order
  const size_t fat = 5000;
  using R = std::vector<std::pair<size_t, bool>>;
  const R thin = {{3, false}, {1, false}, {40, false}, {2, false}};
  for (int dups = 0; dups < 2; dups ++) {
    R a = {{fat, true}}; a.insert(a.end(), thin.begin(), thin.end());
    check_repair(concat_runs(a, rng, dups != 0), "a fat run first");
    R b = thin; b.push_back({fat, true});
    check_repair(concat_runs(b, rng, dups != 0), "a fat run last");
    R c = thin; c.push_back({fat, true}); c.push_back({fat + 17, true}); c.insert(c.end(), thin.begin(), thin.end());
    check_repair(concat_runs(c, rng, dups != 0), "two fat runs side by side");
    check_repair(concat_runs({{fat, true}}, rng, dups != 0), "one fat run and nothing else");
    check_repair(concat_runs({{fat, true}, {fat, true}, {fat, true}}, rng, dups != 0), "nothing but fat runs");
    R d = thin; d.push_back({fat, true}); d.insert(d.end(), thin.begin(), thin.end()); d.push_back({fat, true}); d.insert(d.end(), thin.begin(), thin.end());
    check_repair(concat_runs(d, rng, dups != 0), "fat runs between thin ones");
  }
  // tags at the top of the range: nothing in the repair may depend on a tag having room above it
  check_repair({~0ull, ~0ull - 1, 3, ~0ull, 0}, "tags at both ends of 64 bits");
}

void check_geometry_at(unsigned long long n, unsigned long long cells, int bins, std::mt19937_64 &rng)
{
  const unsigned long long max_key = n * cells * 64ull;
  const bucket_geometry g = series_bucket_geometry(n, cells, bins);
  CHECK(g.shift >= 0 && g.shift < 64, "n %llu cells %llu bins %d: shift %d", n, cells, bins, g.shift);
  if (g.shift < 0 || g.shift >= 64) return;
  CHECK(((max_key - 1) >> g.shift) + 1 == (unsigned long long)g.nbins, "n %llu cells %llu bins %d: nbins %zu, shift %d", n, cells, bins, g.nbins, g.shift);
  CHECK(g.nbins >= 1 && g.nbins <= ((size_t)1 << 16), "n %llu cells %llu bins %d: nbins %zu", n, cells, bins, g.nbins);
  const int asked = std::max(0, std::min(bins, 16));
  CHECK(g.nbins <= ((size_t)1 << asked), "n %llu cells %llu bins %d: nbins %zu, more than asked for", n, cells, bins, g.nbins);
  // (no fewer than half of what was asked for, where the keys allow it: the buckets are not coarser than they have to be)
  CHECK(g.shift == 0 || 2 * g.nbins > ((size_t)1 << asked), "n %llu cells %llu bins %d: nbins %zu, shift %d: too coarse", n, cells, bins, g.nbins, g.shift);
  // every key below max_key lands in a bucket below nbins: the ends, the bucket borders next to them, random ones
  std::vector<unsigned long long> keys = {0, 1, max_key - 1, max_key / 2, (max_key - 1) >> 1};
  if (g.shift > 0) { keys.push_back(((max_key - 1) >> g.shift) << g.shift); keys.push_back((((max_key - 1) >> g.shift) << g.shift) - 1); keys.push_back((1ull << g.shift) - 1); keys.push_back(1ull << g.shift); }
  for (int i = 0; i < 64; i ++) keys.push_back(rng() % max_key);
  for (unsigned long long k : keys) {
    if (k >= max_key) continue;
    CHECK((k >> g.shift) < (unsigned long long)g.nbins, "n %llu cells %llu bins %d: key %llu in bucket %llu of %zu", n, cells, bins, k, k >> g.shift, g.nbins);
  }
}

void check_geometry()
{
  std::mt19937_64 rng(99);
  const int bins[] = {0, 1, 10, 14, 16, -3, 17, 40};       // (the last three: clamped to 0 and 16)
  // n * cells * 64 around powers of two: cells = 2^e + d, n = 1; and n > 1 with cells that make the product straddle one
  for (int e = 0; e <= 44; e ++)
    for (long long d = -2; d <= 2; d ++) {
      const long long cells = (1ll << e) + d;
      if (cells < 1) continue;
      for (int b : bins) {
        check_geometry_at(1, (unsigned long long)cells, b, rng);
        check_geometry_at(3, (unsigned long long)cells, b, rng);
        check_geometry_at(4, (unsigned long long)cells, b, rng);
        check_geometry_at(100, (unsigned long long)cells, b, rng);
      }
    }
  // the test series of tests/test_gpu_ordering.py and a full-size one
  for (int b : bins) {
    check_geometry_at(4, 59ull * 43, b, rng);
    check_geometry_at(3, 35ull * 31 * 15, b, rng);
    check_geometry_at(128, 2043ull * 1019, b, rng);
    check_geometry_at(16, 507ull * 507 * 507, b, rng);
  }
  // clamping: what is asked for outside 0 .. 16 is what its nearest end gives
  for (unsigned long long cells : {1ull, 77ull, 1ull << 20}) {
    const bucket_geometry lo = series_bucket_geometry(5, cells, -3), lo0 = series_bucket_geometry(5, cells, 0);
    const bucket_geometry hi = series_bucket_geometry(5, cells, 17), hi16 = series_bucket_geometry(5, cells, 16);
    CHECK(lo.shift == lo0.shift && lo.nbins == lo0.nbins && lo.nbins == 1, "cells %llu: bins below 0", cells);
    CHECK(hi.shift == hi16.shift && hi.nbins == hi16.nbins, "cells %llu: bins above 16", cells);
  }
}

}  // namespace

int main()
{
  check_geometry();
  check_repairs();
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("series_order checks complete\n");
  return 0;
}
