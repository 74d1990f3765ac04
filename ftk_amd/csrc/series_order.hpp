// The host's share of the device-driven pass's ordering step (series.hip), free of the device: how the order keys of a pass are spread
// over buckets, and the repair of the runs that bucket_rank_kernel leaves unordered (SERIES_FIX_ORDER).  No HIP in it:
// tests/test_series_order_host.py drives both without a GPU through tests/hostcheck/series_order.cpp.
#pragma once
#include <algorithm>
#include <cstddef>

namespace ftkxh {

constexpr int kSeriesMaxBinsLog2 = 16;      // 2^this buckets at most (sweep_params.hpp: kSeriesMaxBins)

struct bucket_geometry { int shift; size_t nbins; };   // bucket = order key >> shift; nbins of them over the keys the pass can produce

// A pass of n steps over `cells` cells produces order keys below n * cells * 64.  2^bins_log2 buckets (clamped to 0 .. kSeriesMaxBinsLog2)
// over the smallest power of two that holds them all: nbins = the bucket of the largest key + 1 <= 2^bins_log2.
inline bucket_geometry series_bucket_geometry(unsigned long long n, unsigned long long cells, int bins_log2)
{
  bins_log2 = std::max(0, std::min(bins_log2, kSeriesMaxBinsLog2));
  const unsigned long long max_key = n * cells * 64ull;
  int key_bits = 1;
  while (key_bits < 63 && (1ull << key_bits) < max_key) key_bits ++;
  bucket_geometry g;
  g.shift = std::max(0, key_bits - bins_log2);
  g.nbins = (size_t)((max_key - 1) >> g.shift) + 1;
  return g;
}

// Records whose `tag` member is in order but for the buckets that were too full to rank on the device: the records of such a bucket sit
// in their own run, unordered among themselves; everything before the run is smaller, everything behind it larger.  Find each such run
// from an inversion, widen it until both ends are in order with their neighbours, sort it.
template <class Rec>
inline void series_fix_order(Rec *h, size_t nrec)
{
  auto less = [](const Rec &p, const Rec &q) { return p.tag < q.tag; };
  for (size_t a = 0; a + 1 < nrec; a ++) {
    if (h[a].tag <= h[a + 1].tag) continue;
    size_t lo = a, hi = a + 2;
    unsigned long long mn = std::min(h[a].tag, h[a + 1].tag), mx = std::max(h[a].tag, h[a + 1].tag);
    for (bool grown = true; grown;) {
      grown = false;
      while (lo > 0 && h[lo - 1].tag > mn) { lo --; mn = std::min(mn, h[lo].tag); mx = std::max(mx, h[lo].tag); grown = true; }
      while (hi < nrec && h[hi].tag < mx) { mn = std::min(mn, h[hi].tag); mx = std::max(mx, h[hi].tag); hi ++; grown = true; }
    }
    std::sort(h + lo, h + hi, less);
    a = hi - 2;                                              // (the loop's increment moves on to the run's last element)
  }
}

}  // namespace ftkxh
