// ftk_amd/csrc/pass2_layout.hpp without a GPU: every array of the trace's, the ordering's and the post-processing's layout lies inside its
// total, overlaps no other, starts on its element's alignment; the shared prefixes agree on both sides; and a block reserved for one
// call (its total and a quarter more) holds every array of any later call that is let into it.  The element counts stated HERE are
// what the kernels address (trace_device.hip, trace_order_kernels.hip, post_process_steps.hpp: PostProc), written down a second time on
// purpose.  A program of its own: tests/test_pass2_layout_host.py compiles and runs it, under ASan + UBSan where they are installed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ftk_amd/csrc/pass2_layout.hpp"

using namespace ftkx;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                                                     \
  do {                                                                                       \
    if (!(cond)) { failures ++; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
  } while (0)

struct Arr { const char *name; size_t at, need, align; };     // need: the bytes the kernels and copies address

Arr arr(const char *name, const Span &s, size_t count, size_t elem) { return Arr{name, s.at, count * elem, elem}; }

// what is addressed lies inside [0, total), starts aligned, and no two overlap
void check_block(const char *what, int maxnb, size_t n, const std::vector<Arr> &a, size_t total)
{
  for (size_t i = 0; i < a.size(); i ++) {
    CHECK(a[i].at + a[i].need <= total, "%s maxnb %d n %zu: %s ends at %zu of %zu", what, maxnb, n, a[i].name, a[i].at + a[i].need, total);
    CHECK(a[i].at % a[i].align == 0, "%s maxnb %d n %zu: %s at %zu is not aligned to %zu", what, maxnb, n, a[i].name, a[i].at, a[i].align);
    for (size_t j = 0; j < i; j ++) {
      const bool apart = a[i].at + a[i].need <= a[j].at || a[j].at + a[j].need <= a[i].at;
      CHECK(apart, "%s maxnb %d n %zu: %s and %s overlap", what, maxnb, n, a[i].name, a[j].name);
    }
  }
}

std::vector<Arr> trace_dev(const TraceLayout &L, int maxnb, size_t n)
{
  return {arr("tags", L.tags, n, 8), arr("nbr", L.nbr, n * (size_t)maxnb, 4), arr("root", L.root, n, 4), arr("deg", L.deg, n, 1), arr("parent", L.parent, n, 4)};
}

void check_trace(int maxnb, size_t n)
{
  const TraceLayout L(maxnb, n);
  std::vector<Arr> dev = trace_dev(L, maxnb, n), host(dev.begin(), dev.end() - 1);      // the pinned side: the same offsets, no parent
  check_block("trace, device", maxnb, n, dev, L.dev_bytes);
  check_block("trace, pinned", maxnb, n, host, L.host_bytes);
  CHECK(L.host_bytes <= L.parent.at, "trace maxnb %d n %zu: parent at %zu inside the shared prefix of %zu", maxnb, n, L.parent.at, L.host_bytes);
  // nbr .. deg: one range that holds nothing else, in this order, with less than one rounding step between neighbours
  CHECK(L.tags.end() <= L.nbr.at && L.nbr.end() <= L.root.at && L.root.end() <= L.deg.at && L.deg.end() <= L.parent.at, "trace maxnb %d n %zu: order", maxnb, n);
  CHECK(L.root.at - L.nbr.end() < 16 && L.deg.at - L.root.end() < 16, "trace maxnb %d n %zu: holes in nbr .. deg", maxnb, n);
  CHECK(L.nbr.at + L.down_bytes() == L.deg.at + n && L.nbr.at + L.down_bytes() <= L.host_bytes, "trace maxnb %d n %zu: the download is %zu bytes from %zu", maxnb, n, L.down_bytes(), L.nbr.at);
}

void check_order(size_t n)
{
  const OrderLayout L(n);
  // device: init writes best, cyc, cnt[2i + 1], indices for i < n; arcs 2u + s < 2n; info two words per seed (at most n); the host sends n + 1 offsets
  check_block("order, device", 0, n,
              {arr("key", L.key, n, 8), arr("best", L.best, n, 8), arr("info", L.info, 2 * n, 8), arr("link", L.link, 2 * n, 8), arr("on", L.on, 2 * n, 4), arr("cnt", L.cnt, 2 * n, 4),
               arr("cyc", L.cyc, n, 4), arr("seedpos", L.seedpos, n, 4), arr("seedlist", L.seedlist, n, 4), arr("indices", L.indices, n, 4), arr("loop", L.loop, n, 4),
               arr("off", L.off, n + 1, 4), arr("sorted", L.sorted, n, 4), arr("counters", L.counters, TRO_WORDS, 4)},
              L.dev_bytes);
  check_block("order, pinned", 0, n,
              {arr("h_info", L.h_info, 2 * n, 8), arr("h_off", L.h_off, n + 1, 4), arr("h_sorted", L.h_sorted, n, 4), arr("h_indices", L.h_indices, n, 4), arr("h_loop", L.h_loop, n, 4),
               arr("h_counters", L.h_counters, TRO_WORDS, 4)},
              L.host_bytes);
  // laid out for n + 2 records: no array below that (info, link, on, cnt: two per record)
  CHECK(L.key.bytes >= (n + 2) * 8 && L.info.bytes >= 2 * (n + 2) * 8 && L.link.bytes >= 2 * (n + 2) * 8 && L.on.bytes >= 2 * (n + 2) * 4 && L.cnt.bytes >= 2 * (n + 2) * 4 &&
        L.sorted.bytes >= (n + 2) * 4 && L.h_info.bytes >= 2 * (n + 2) * 8 && L.h_loop.bytes >= (n + 2) * 4, "order n %zu: fewer than n + 2 records", n);
}

size_t agg_bytes(size_t np) { return ((np + 2047) / 2048 + 1) * 16; }     // post_process_kernels.hip: a total of 16 bytes per tile of 2 048 points, and one

void check_post_process(size_t n_rec, size_t np, size_t nc)
{
  PpPlan pl(n_rec, np, nc, agg_bytes(np));
  std::vector<char> block(pl.dev_bytes);                     // a real block: ASan sees whatever bind() would hand out beyond it
  pl.bind(block.data());
  const PostProc &p = pl.p;
  auto dev = [&](const char *name, const void *ptr, size_t count, size_t elem) { return Arr{name, (size_t)((const char *)ptr - block.data()), count * elem, elem}; };
  const std::vector<Arr> in = {arr("rec", pl.in_rec, 2 * n_rec, 8) /* 16 bytes per record */, arr("indices", pl.in_indices, np, 4), arr("off", pl.in_off, nc + 1, 4), arr("loop", pl.in_loop, nc, 4)};
  std::vector<Arr> d = {dev("rec", p.rec, 2 * n_rec, 8), dev("indices", p.indices, np, 4), dev("off", p.off, nc + 1, 4), dev("loop", p.loop, nc, 4),
                        dev("cid", p.cid, np, 4), dev("first", p.first, nc + 1, 4), dev("type_a", p.type_a, np, 4), dev("type_b", p.type_b, np, 4), dev("aux", p.aux, np, 4), dev("t", p.t, np, 8),
                        dev("rank", p.rank, np + 1, 4), dev("olist", p.olist, np + 1, 4), dev("last", p.last, np + 1, 4),
                        dev("type_r", p.type_r, np, 4), dev("aux_r", p.aux_r, np, 4), dev("t_r", p.t_r, np, 8), dev("idx_r", p.idx_r, np, 4),
                        dev("type_c", p.type_c, np, 4), dev("aux_c", p.aux_c, np, 4), dev("t_c", p.t_c, np, 8), dev("idx_c", p.idx_c, np, 4), dev("pid_c", p.pid_c, np, 4),
                        dev("poff", p.poff, np + 1, 4), dev("ploop", p.ploop, np, 4), dev("pcurve", p.pcurve, np, 4),
                        dev("idx_o", p.idx_o, np, 4), dev("type_o", p.type_o, np, 4), dev("flag_o", p.flag_o, np, 4), dev("t_o", p.t_o, np, 8), dev("t_f", p.t_f, np, 8), dev("t_out", p.t_out, np, 8),
                        dev("counters", p.counters, PPC_WORDS, 4), dev("agg", pl.agg, agg_bytes(np) / 8, 8)};
  check_block("post-process, device", 0, np, d, pl.dev_bytes);
  for (size_t k = 0; k < in.size(); k ++)                    // the input block: the same place on both sides, one copy of in_end bytes
    CHECK(d[k].at == in[k].at && in[k].at + in[k].need <= pl.in_end, "post-process np %zu nc %zu: input %s at %zu on the device, %zu pinned", np, nc, in[k].name, d[k].at, in[k].at);
  std::vector<Arr> h = in;
  const std::vector<Arr> res = {arr("h_counters", pl.h_counters, PPC_WORDS, 4), arr("h_t", pl.h_t, np, 8), arr("h_idx", pl.h_idx, np, 4), arr("h_type", pl.h_type, np, 4),
                                arr("h_poff", pl.h_poff, np + 1, 4), arr("h_ploop", pl.h_ploop, np, 4), arr("h_pcurve", pl.h_pcurve, np, 4)};
  h.insert(h.end(), res.begin(), res.end());
  check_block("post-process, pinned", 0, np, h, pl.host_bytes);
  for (const Arr &x : d) memset(block.data() + x.at, 0, x.need);
}

// what a pass-2 block (ctx.hpp: pass2_room) holds for a request of `want` bytes
size_t capacity_for(size_t want) { return want + want / 4; }

}  // namespace

int main()
{
  const int maxnbs[] = {6, 8};
  const size_t ns[] = {1, 2, 5, 100, 150, 4096, 4097};
  for (int maxnb : maxnbs) for (size_t n : ns) check_trace(maxnb, n);
  for (size_t n : ns) {
    check_order(n);
    check_post_process(n, n, 1);
    check_post_process(n, n, n);
  }
  // a block sized by call a, reused by every call b that fits into it by its own total: b's arrays, parent included, end inside
  // ((8, 100) then (6, 150) is among the pairs: sized by bytes alone, a block for the first let the second in with too few parents)
  int reused = 0;
  bool met_3d_100_then_2d_150 = false;
  for (int ma : maxnbs) for (size_t na : ns) for (int mb : maxnbs) for (size_t nb : ns) {
    const TraceLayout A(ma, na), B(mb, nb);
    const size_t cap = capacity_for(A.dev_bytes);
    met_3d_100_then_2d_150 = met_3d_100_then_2d_150 || (ma == 8 && na == 100 && mb == 6 && nb == 150);
    if (B.dev_bytes > cap) continue;
    reused ++;
    for (const Arr &x : trace_dev(B, mb, nb))
      CHECK(x.at + x.need <= cap, "a block for (maxnb %d, n %zu) of %zu bytes, reused by (maxnb %d, n %zu): %s ends at %zu", ma, na, cap, mb, nb, x.name, x.at + x.need);
  }
  CHECK(met_3d_100_then_2d_150, "the pair (8, 100) then (6, 150) is not among the cases");
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("pass2_layout checks complete: %d reuses\n", reused);
  return 0;
}
