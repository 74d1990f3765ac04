// ftk_amd/csrc/post_process_steps.hpp on the CPU: post_process_steps() through two Run types, for tests/test_post_process_steps_host.py.
//
//   SerialRun   a map is a loop, a scan is ONE left fold: op(op(op(identity, x0), x1), x2) ...
//   TiledRun    the association of post_process_kernels.hip restated in plain C++, function for function and line for line where the
//               operands meet: 8 items per thread folded in order; an inclusive scan over the 64 lanes of a wave in six doubling steps
//               (what __shfl_up hands a lane is the value of lane - d before the step); the 4 wave totals folded in order; tiles of
//               2 048 padded with identity(); up to kSingle points one "workgroup" that carries a value from tile to tile; above that
//               the tiles' totals, the spine over them in batches of 256 with a carry, and the tiles again with their prefix
//
// Both must give what ftkx_post_process_curves gives, t bit for bit: that holds the operators to being associative with identity() as a
// two-sided identity, and every level of the tiled scan to op(left, right).  The entry arithmetic of ftkx_post_process_curves_device
// (offsets[0] != 0, empty curves taken out and put back as empty trajectories) is restated here too.
//
// With -DPP_STEPS_MAIN: a program of its own (for a sanitizer build, not for loading into Python): post_process_steps IN OUT [IN OUT ...]
// reads sets as tests/test_post_process_steps_host.py writes them, runs both Run types, compares them with each other and writes the
// trajectories to OUT.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ftk_amd/csrc/post_process_steps.hpp"

using namespace ftkx;

namespace {

constexpr int kItems = 8, kThreads = 256, kTile = kThreads * kItems, kSingle = 4 * kTile;

struct SerialRun {
  template <class F> void map(const F &f) { for (int i = 0; i < f.n(); i ++) f(i); }
  template <class S> void scan(const S &s)
  {
    typename S::T run = S::identity();
    for (int i = 0; i < s.n(); i ++) {
      const typename S::T incl = S::op(run, s.load(i));
      s.store(i, incl, run);
      run = incl;
    }
  }
  void phase(const char *) {}
};

struct TiledRun {
  int np;                                                   // the launch is sized by the points that came in; n() may be fewer

  // exclusive scan of one value per thread in thread order over the workgroup: excl[256]; returns the total of all 256
  template <class S> static typename S::T block_scan_exclusive(const typename S::T *v, typename S::T *excl)
  {
    typedef typename S::T T;
    T inc[kThreads], wave_total[4];
    for (int t = 0; t < kThreads; t ++) inc[t] = v[t];
    for (int w = 0; w < 4; w ++) {
      for (unsigned d = 1; d < 64; d <<= 1) {
        T up[64];                                           // what the shuffle hands every lane: the wave's values before this step
        for (int lane = 0; lane < 64; lane ++) up[lane] = inc[w * 64 + (lane >= (int)d ? lane - (int)d : lane)];
        for (int lane = 0; lane < 64; lane ++) {
          const int t = w * 64 + lane;
          const T o = up[lane];
          if (lane >= (int)d) inc[t] = S::op(o, inc[t]);
        }
      }
      wave_total[w] = inc[w * 64 + 63];
    }
    T prefix[4];
    T total = S::identity();
    for (int k = 0; k < 4; k ++) { prefix[k] = total; total = S::op(total, wave_total[k]); }
    for (int t = 0; t < kThreads; t ++) {
      const int lane = t & 63, w = t >> 6;
      excl[t] = lane ? S::op(prefix[w], inc[t - 1]) : prefix[w];
    }
    return total;
  }

  template <class S> static typename S::T tile_total(const S &s, int tile, int n)
  {
    typedef typename S::T T;
    T acc[kThreads], excl[kThreads];
    for (int t = 0; t < kThreads; t ++) {
      const long long base = (long long)tile * kTile + (long long)t * kItems;
      acc[t] = S::identity();
      for (int k = 0; k < kItems; k ++) if (base + k < n) acc[t] = S::op(acc[t], s.load((int)(base + k)));
    }
    return block_scan_exclusive<S>(acc, excl);
  }

  // the tile's elements with `carry` in front of them; returns the tile's total
  template <class S> static typename S::T tile_scan(const S &s, int tile, int n, typename S::T carry)
  {
    typedef typename S::T T;
    std::vector<T> item((size_t)kTile);
    T acc[kThreads], excl[kThreads];
    for (int t = 0; t < kThreads; t ++) {
      const long long base = (long long)tile * kTile + (long long)t * kItems;
      acc[t] = S::identity();
      for (int k = 0; k < kItems; k ++) {
        item[t * kItems + k] = base + k < n ? s.load((int)(base + k)) : S::identity();
        acc[t] = S::op(acc[t], item[t * kItems + k]);
      }
    }
    const T total = block_scan_exclusive<S>(acc, excl);
    for (int t = 0; t < kThreads; t ++) {
      const long long base = (long long)tile * kTile + (long long)t * kItems;
      T run = S::op(carry, excl[t]);
      for (int k = 0; k < kItems; k ++) {
        const T incl = S::op(run, item[t * kItems + k]);
        if (base + k < n) s.store((int)(base + k), incl, run);
        run = incl;
      }
    }
    return total;
  }

  template <class S> static void scan_single(const S &s)
  {
    const int n = s.n();
    typename S::T carry = S::identity();
    for (int tile = 0; (long long)tile * kTile < n; tile ++) carry = S::op(carry, tile_scan(s, tile, n, carry));
  }

  // the tiles' totals -> what lies before every tile
  template <class S> static void scan_spine(typename S::T *agg, int ntiles)
  {
    typedef typename S::T T;
    T carry = S::identity();
    for (int b = 0; b < ntiles; b += kThreads) {
      T v[kThreads], before[kThreads];
      for (int t = 0; t < kThreads; t ++) v[t] = b + t < ntiles ? agg[b + t] : S::identity();
      const T total = block_scan_exclusive<S>(v, before);
      for (int t = 0; t < kThreads; t ++) {
        const int k = b + t;
        if (k < ntiles) agg[k] = S::op(carry, before[t]);
      }
      carry = S::op(carry, total);
    }
  }

  template <class F> void map(const F &f) { for (int i = 0; i < np; i ++) if (i < f.n()) f(i); }
  template <class S> void scan(const S &s)
  {
    if (np <= kSingle) { scan_single(s); return; }
    const int ntiles = (np + kTile - 1) / kTile;
    std::vector<typename S::T> agg((size_t)ntiles);
    for (int tile = 0; tile < ntiles; tile ++) agg[tile] = tile_total(s, tile, s.n());
    scan_spine<S>(agg.data(), ntiles);
    const int n = s.n();
    for (int tile = 0; tile < ntiles; tile ++) if ((long long)tile * kTile < n) (void)tile_scan(s, tile, n, agg[tile]);
  }
  void phase(const char *) {}
};

// one call's work arrays: what bind() of post_process_device.hip lays out in the context's block, zeroed
struct Work {
  std::vector<int> ints[13];
  std::vector<unsigned> words[10];
  std::vector<double> reals[6];
  std::vector<unsigned> counters;
  void bind(PostProc &p, size_t np, size_t nc)
  {
    int ki = 0, kw = 0, kr = 0;
    auto I = [&](size_t n) { ints[ki].assign(n, 0); return ints[ki ++].data(); };
    auto W = [&](size_t n) { words[kw].assign(n, 0u); return words[kw ++].data(); };
    auto R = [&](size_t n) { reals[kr].assign(n, 0.0); return reals[kr ++].data(); };
    p.cid = I(np); p.first = I(nc + 1);
    p.type_a = W(np); p.type_b = W(np); p.aux = W(np); p.t = R(np);
    p.rank = I(np + 1); p.olist = I(np + 1); p.last = I(np + 1);
    p.type_r = W(np); p.aux_r = W(np); p.t_r = R(np); p.idx_r = I(np);
    p.type_c = W(np); p.aux_c = W(np); p.t_c = R(np); p.idx_c = I(np); p.pid_c = I(np);
    p.poff = I(np + 1); p.ploop = I(np); p.pcurve = I(np);
    p.idx_o = I(np); p.type_o = W(np); p.flag_o = W(np);
    p.t_o = R(np); p.t_f = R(np); p.t_out = R(np);
    counters.assign(PPC_WORDS, 0u);
    p.counters = counters.data();
  }
};

}  // namespace

extern "C" {

// mode 0: SerialRun, 1: TiledRun.  Curves as ftkx_curves holds them (nc + 1 offsets into `indices`, which has n_idx entries).  out_counts: trajectories,
// points; out_offsets, out_loop, out_id: room for nc + np + 1; out_indices, out_type, out_t: room for np.  -> 0, -1 (invalid input), 1 (a t that
// is not finite: the device entry point hands such a set to the host), -2 (counts that cannot be)
int hc_post_process_steps(int mode, const PpRecord *rec, long long n_rec, const long long *offsets, long long nc, const long long *indices, long long n_idx, const int *loop,
                          long long *out_counts, long long *out_offsets, long long *out_indices, unsigned *out_type, double *out_t, int *out_loop, int *out_id)
{
  size_t empty = 0;
  for (long long k = 0; k < nc; k ++) {
    if (offsets[k] < 0 || offsets[k + 1] < offsets[k] || offsets[k + 1] > n_idx) return -1;
    empty += offsets[k + 1] == offsets[k];
  }
  const long long first = nc ? offsets[0] : 0, np = nc ? offsets[nc] - first : 0;
  std::vector<int> h_indices((size_t)np), h_off, h_loop, orig;
  for (long long k = 0; k < np; k ++) {
    const long long i = indices[first + k];
    if (i < 0 || i >= n_rec) return -1;
    h_indices[(size_t)k] = (int)i;
  }
  for (long long k = 0; k < nc; k ++) {
    if (offsets[k + 1] == offsets[k]) continue;
    h_off.push_back((int)(offsets[k] - first)); h_loop.push_back(loop[k]); orig.push_back((int)k);
  }
  h_off.push_back((int)np);
  size_t M = 0, P = 0;
  PostProc p;
  Work work;
  if (np > 0) {
    memset(&p, 0, sizeof(p));
    p.n_rec = (int)n_rec; p.nc = (int)orig.size(); p.np = (int)np;
    p.rec = rec; p.indices = h_indices.data(); p.off = h_off.data(); p.loop = h_loop.data();
    work.bind(p, (size_t)np, orig.size());
    if (mode == 0) { SerialRun run; post_process_steps(p, run); }
    else { TiledRun run{(int)np}; post_process_steps(p, run); }
    if (p.counters[PPC_BAD_INDEX]) return -1;
    if (p.counters[PPC_NONFINITE]) return 1;
    M = p.counters[PPC_POINTS]; P = p.counters[PPC_PIECES];
    if (M > (size_t)np || P > M || P < orig.size()) return -2;
    for (size_t k = 0; k < M; k ++) { out_indices[k] = p.idx_o[k]; out_type[k] = p.type_o[k]; out_t[k] = p.t_out[k]; }
  }
  size_t r = 0, k = 0, next = 0;                            // trajectory, piece, place in orig
  for (long long cu = 0; cu < nc; cu ++) {
    if (next < orig.size() && orig[next] == cu) {
      for (; k < P && (size_t)p.pcurve[k] == next; k ++, r ++) { out_offsets[r] = p.poff[k]; out_loop[r] = p.ploop[k]; out_id[r] = (int)cu; }
      next ++;
    } else { out_offsets[r] = k < P ? p.poff[k] : (long long)M; out_loop[r] = loop[cu]; out_id[r] = (int)cu; r ++; }
  }
  if (k != P) return -2;
  out_offsets[r] = (long long)M;
  out_counts[0] = (long long)r; out_counts[1] = (long long)M;
  return 0;
}

}  // extern "C"

#ifdef PP_STEPS_MAIN
namespace {

template <class T> bool read_n(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T> bool write_n(FILE *f, const std::vector<T> &v, size_t n) { return n == 0 || fwrite(v.data(), sizeof(T), n, f) == n; }

struct Result {
  long long counts[2] = {0, 0};
  std::vector<long long> offsets, indices;
  std::vector<unsigned> type;
  std::vector<double> t;
  std::vector<int> loop, id;
};

}  // namespace

// IN: int64 n_rec, nc, n_idx | n_rec PpRecord | nc + 1 int64 offsets | n_idx int64 indices | nc int32 loop flags
// OUT: int64 trajectories, points | offsets | indices | types | t | loop flags | ids
int main(int argc, char **argv)
{
  if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: %s IN OUT [IN OUT ...]\n", argv[0]); return 2; }
  for (int a = 1; a < argc; a += 2) {
    FILE *f = fopen(argv[a], "rb");
    long long head[3];
    if (!f || fread(head, 8, 3, f) != 3) { fprintf(stderr, "%s: cannot read\n", argv[a]); return 2; }
    const size_t n_rec = (size_t)head[0], nc = (size_t)head[1], n_idx = (size_t)head[2];
    std::vector<PpRecord> rec; std::vector<long long> offsets, indices; std::vector<int> loop;
    if (!read_n(f, rec, n_rec) || !read_n(f, offsets, nc + 1) || !read_n(f, indices, n_idx) || !read_n(f, loop, nc)) { fprintf(stderr, "%s: short\n", argv[a]); return 2; }
    fclose(f);
    const size_t np = nc ? (size_t)(offsets[nc] - offsets[0]) : 0;
    Result res[2];
    for (int mode = 0; mode < 2; mode ++) {
      Result &r = res[mode];
      r.offsets.resize(nc + np + 1); r.loop.resize(nc + np + 1); r.id.resize(nc + np + 1);
      r.indices.resize(np); r.type.resize(np); r.t.resize(np);
      const int rc = hc_post_process_steps(mode, rec.data(), (long long)n_rec, offsets.data(), (long long)nc, indices.data(), (long long)n_idx, loop.data(),
                                           r.counts, r.offsets.data(), r.indices.data(), r.type.data(), r.t.data(), r.loop.data(), r.id.data());
      if (rc != 0) { fprintf(stderr, "%s: mode %d: rc %d\n", argv[a], mode, rc); return 1; }
    }
    const size_t R = (size_t)res[0].counts[0], M = (size_t)res[0].counts[1];
    const bool same = res[1].counts[0] == res[0].counts[0] && res[1].counts[1] == res[0].counts[1]
                      && !memcmp(res[0].offsets.data(), res[1].offsets.data(), (R + 1) * 8) && !memcmp(res[0].indices.data(), res[1].indices.data(), M * 8)
                      && !memcmp(res[0].type.data(), res[1].type.data(), M * 4) && !memcmp(res[0].t.data(), res[1].t.data(), M * 8)
                      && !memcmp(res[0].loop.data(), res[1].loop.data(), R * 4) && !memcmp(res[0].id.data(), res[1].id.data(), R * 4);
    if (!same) { fprintf(stderr, "%s: the tiled scan and the left fold differ\n", argv[a]); return 1; }
    FILE *o = fopen(argv[a + 1], "wb");
    const Result &r = res[1];
    if (!o || fwrite(r.counts, 8, 2, o) != 2 || !write_n(o, r.offsets, R + 1) || !write_n(o, r.indices, M) || !write_n(o, r.type, M) || !write_n(o, r.t, M)
        || !write_n(o, r.loop, R) || !write_n(o, r.id, R) || fclose(o) != 0) { fprintf(stderr, "%s: cannot write\n", argv[a + 1]); return 2; }
    printf("%s: %zu points in %zu curves -> %zu in %zu, left fold == tiled\n", argv[a], np, nc, M, R);
  }
  printf("post_process_steps run complete\n");
  return 0;
}
#endif
