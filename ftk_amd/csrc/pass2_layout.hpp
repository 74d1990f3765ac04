// Pass 2 on the device: where every array of one call lies inside the context's blocks (ctx.hpp: ftkx_pass2_state).  A layout is a
// function of the call's sizes, never of a block's capacity: a block is reserved for the layout's total, so whatever the layout addresses
// lies inside it.  Each array's element count is written once, here.  No HIP in this file: tests/hostcheck/pass2_layout.cpp checks the
// layouts without a GPU.
#pragma once
#include <cstddef>
#include "post_process_steps.hpp"

namespace ftkx {

struct Span {
  size_t at = 0, bytes = 0;
  size_t end() const { return at + bytes; }
  template <class T> T *in(void *base) const { return base ? (T *)((char *)base + at) : nullptr; }
};

// arrays one behind the other, each beginning on 16 bytes
struct Carver {
  size_t total = 0;
  Span take(size_t count, size_t elem) { const Span s{total, count * elem}; total += (s.bytes + 15) & ~(size_t)15; return s; }
};

// ---- the trace's front (trace_device.hip): tags | nbr | root | deg on both sides -- nbr .. deg come down in one copy -- and the
// union-find's parents behind them on the device
struct TraceLayout {
  Span tags, nbr, root, deg, parent;
  size_t host_bytes, dev_bytes;
  TraceLayout(int maxnb, size_t n)
  {
    Carver c;
    tags = c.take(n, 8); nbr = c.take(n * (size_t)maxnb, 4); root = c.take(n, 4); deg = c.take(n, 1);
    host_bytes = c.total;
    parent = c.take(n, 4);
    dev_bytes = c.total;
  }
  size_t down_bytes() const { return deg.end() - nbr.at; }
};

// ---- the ordering (trace_order_kernels.hip: TraceOrder) and its pinned staging, laid out for n + 2 records
enum { TRO_SEEDS = 0, TRO_SPECIAL = 1, TRO_ERROR = 2, TRO_CHECK = 3, TRO_FLAGS = 8, TRO_WORDS = 128 };

struct OrderLayout {
  Span key, best, info, link, on, cnt, cyc, seedpos, seedlist, indices, loop, off, sorted, counters;   // device
  Span h_info, h_off, h_sorted, h_indices, h_loop, h_counters;                                          // pinned
  size_t dev_bytes, host_bytes;
  explicit OrderLayout(size_t n = 0)
  {
    const size_t m = n + 2;
    Carver d;
    key = d.take(m, 8); best = d.take(m, 8); info = d.take(2 * m, 8); link = d.take(2 * m, 8);
    on = d.take(2 * m, 4); cnt = d.take(2 * m, 4); cyc = d.take(m, 4); seedpos = d.take(m, 4); seedlist = d.take(m, 4);
    indices = d.take(m, 4); loop = d.take(m, 4); off = d.take(m, 4); sorted = d.take(m, 4);
    counters = d.take(TRO_WORDS, 4);
    dev_bytes = d.total;
    Carver h;
    h_info = h.take(2 * m, 8); h_off = h.take(m, 4); h_sorted = h.take(m, 4); h_indices = h.take(m, 4); h_loop = h.take(m, 4);
    h_counters = h.take(TRO_WORDS, 4);
    host_bytes = h.total;
  }
};

// ---- post-processing (post_process_device.hip).  The input block has the same shape on both sides -- records | indices | offsets |
// loop flags -- so that it goes up in one copy; behind it the results on the pinned side, the work arrays on the device.
struct PpPlan {
  size_t n_rec, np, nc, agg_bytes;
  Span in_rec, in_indices, in_off, in_loop;                  // both sides
  size_t in_end;
  Span h_counters, h_t, h_idx, h_type, h_poff, h_ploop, h_pcurve;
  size_t host_bytes, dev_bytes;
  PostProc p;                                                // device pointers, filled by bind()
  void *agg;

  // agg_bytes: the scans' tile totals (post_process_tiles(np) * kPostProcAggBytes)
  PpPlan(size_t n_rec_, size_t np_, size_t nc_, size_t agg_bytes_) : n_rec(n_rec_), np(np_), nc(nc_), agg_bytes(agg_bytes_)
  {
    Carver h;
    in_rec = h.take(n_rec, sizeof(PpRecord)); in_indices = h.take(np, 4); in_off = h.take(nc + 1, 4); in_loop = h.take(nc, 4);
    in_end = h.total;
    h_counters = h.take(PPC_WORDS, 4); h_t = h.take(np, 8); h_idx = h.take(np, 4); h_type = h.take(np, 4);
    h_poff = h.take(np + 1, 4); h_ploop = h.take(np, 4); h_pcurve = h.take(np, 4);
    host_bytes = h.total;
    bind(nullptr);
  }

  // the device block at `base` (nullptr: only counts its bytes)
  void bind(void *base)
  {
    Carver d;
    d.total = in_end;
    auto ints = [&](size_t count) { return d.take(count, 4).in<int>(base); };
    auto words = [&](size_t count) { return d.take(count, 4).in<unsigned>(base); };
    auto doubles = [&](size_t count) { return d.take(count, 8).in<double>(base); };
    p.n_rec = (int)n_rec; p.nc = (int)nc; p.np = (int)np;
    p.rec = in_rec.in<const PpRecord>(base); p.indices = in_indices.in<const int>(base); p.off = in_off.in<const int>(base); p.loop = in_loop.in<const int>(base);
    p.cid = ints(np); p.first = ints(nc + 1);
    p.type_a = words(np); p.type_b = words(np); p.aux = words(np); p.t = doubles(np);
    p.rank = ints(np + 1); p.olist = ints(np + 1); p.last = ints(np + 1);
    p.type_r = words(np); p.aux_r = words(np); p.t_r = doubles(np); p.idx_r = ints(np);
    p.type_c = words(np); p.aux_c = words(np); p.t_c = doubles(np); p.idx_c = ints(np); p.pid_c = ints(np);
    p.poff = ints(np + 1); p.ploop = ints(np); p.pcurve = ints(np);
    p.idx_o = ints(np); p.type_o = words(np); p.flag_o = words(np);
    p.t_o = doubles(np); p.t_f = doubles(np); p.t_out = doubles(np);
    p.counters = words(PPC_WORDS);
    agg = d.take(agg_bytes, 1).in<void>(base);
    dev_bytes = d.total;
  }
};

}  // namespace ftkx
