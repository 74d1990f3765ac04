// Trajectory post-processing on the flat point array: what every point does in each step of ftkx_post_process_curves_device, and what
// every scan over the points adds up.  trace.cpp's ftkx_post_process_curves works curve by curve; here every step is either a map over
// the points of ALL curves or a scan over them, with the curves' heads (the ordinal points, the pieces' heads) as segment borders:
//
//   gather        per point: its curve (binary search in the offsets), type, aux word (ordinal bit, timestep) and t through `indices`
//   ScanOrdinals  exclusive count of the ordinal flag -> rank[]; olist[] = the ordinal points' positions, one curve after the other
//   smooth        smooth_ordinal_types(2): an ordinal of rank r in [2, count - 2) reads its four neighbours in olist[] (type_a -> type_b)
//   ScanLast<InGap>    last point so far whose type differs from that of the ordinal before it: with it
//   interval      smooth_interval_types: head, tail, gaps of equal ends, and in a gap (lt, rt) everything from the first type != lt on
//   ScanLast<OffFirst> last point so far whose type differs from its curve's first: with it
//   first, rotate the first such point of every curve (no atomics: the one whose predecessor has none before it); the rotation as an index map
//   ScanLast<Anchor>   split_all's state machine: the head of a run of equal types is dropped unless the run before it had length 1 and
//                 lost its own head; along runs of length 1 drop and keep alternate from the last anchor (a point behind a run longer
//                 than 1: dropped; a curve's first point: kept) -- the parity of the distance to it
//   ScanKept      kept points and piece heads counted -> every kept point's place and piece; the pieces' offsets, loop flags and curves
//   reorder       a piece that is no loop runs backwards if it starts later than it ends (timestep, then t): an index map again
//   ScanTimeForward / ScanTimeBackward   adjust_time: a running max that restarts at piece heads and ordinal points, then a running
//                 min over its result from the other end.  std::max / std::min as trace.cpp calls them keep their FIRST argument -- the
//                 running value -- on a tie (-0.0 against 0.0): the scans keep operand order, so the bits are the same
//
// A scan is described by: T, n(), identity(), op(left, right) (associative, not commutative), load(i), store(i, inclusive, exclusive).
// Everything here compiles for the host as well: the same code runs serially wherever no GPU is at hand.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PP_HD __host__ __device__ inline
#else
#define PP_HD inline
#endif

namespace ftkx {

struct PpRecord { unsigned type, aux; double t; };       // what post-processing reads of a record: 16 of its 72 bytes
enum { PPC_POINTS = 0, PPC_PIECES = 1, PPC_NONFINITE = 2, PPC_BAD_INDEX = 3, PPC_WORDS = 8 };
enum { PPF_ORDINAL = 1, PPF_HEAD = 2, PPF_END = 4 };

struct PostProc {
  int n_rec, nc, np;                                   // records, curves (none empty), points
  const PpRecord *rec;
  const int *indices, *off, *loop;                     // the traced curves: np, nc + 1, nc
  int *cid, *first;                                    // per point: its curve; per curve: first point whose type is not the curve's first (-1: none)
  unsigned *type_a, *type_b, *aux; double *t;          // gathered; type_b: smoothed
  int *rank, *olist, *last;                            // np + 1: ordinals before the point; the ordinals' positions; the scan in hand's "last flagged point so far"
  unsigned *type_r, *aux_r; double *t_r; int *idx_r;   // rotated
  unsigned *type_c, *aux_c; double *t_c; int *idx_c, *pid_c;   // kept points, in order, and their pieces
  int *poff, *ploop, *pcurve;                          // per piece: np + 1 offsets, loop flags, parent curves
  int *idx_o; unsigned *type_o, *flag_o; double *t_o, *t_f, *t_out;   // re-ordered: PPF_* flags, t as gathered / after the forward / the backward pass
  unsigned *counters;                                  // PPC_*
};

PP_HD bool pp_finite(double v)
{
  union { double d; uint64_t u; } x;
  x.d = v;
  return ((x.u >> 52) & 0x7ffu) != 0x7ffu;
}

// ---- maps -----------------------------------------------------------------------------------------------------------------------
struct PpGather {
  PostProc p;
  PP_HD int n() const { return p.np; }
  PP_HD void operator()(int i) const
  {
    int lo = 0, hi = p.nc;                              // the last curve that begins at or before i
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p.off[mid] <= i) lo = mid; else hi = mid; }
    int r = p.indices[i];
    if (r < 0 || r >= p.n_rec) { p.counters[PPC_BAD_INDEX] = 1; r = 0; }
    const PpRecord rec = p.rec[r];
    if (!pp_finite(rec.t)) p.counters[PPC_NONFINITE] = 1;
    p.cid[i] = lo; p.type_a[i] = rec.type; p.aux[i] = rec.aux; p.t[i] = rec.t;
    if (i == p.off[lo]) p.first[lo] = -1;
  }
};

struct PpSmooth {
  PostProc p;
  PP_HD int n() const { return p.np; }
  PP_HD void operator()(int i) const
  {
    unsigned ty = p.type_a[i];
    if (p.aux[i] & 1u) {
      const int c = p.cid[i], g = p.rank[i], gb = p.rank[p.off[c]], cnt = p.rank[p.off[c + 1]] - gb, r = g - gb;
      if (cnt >= 5 && r >= 2 && r < cnt - 2) {
        unsigned consistent = p.type_a[p.olist[g - 2]];
        if (p.type_a[p.olist[g - 1]] != consistent || p.type_a[p.olist[g + 1]] != consistent || p.type_a[p.olist[g + 2]] != consistent) consistent = 0;
        if (consistent != 0) ty = consistent;
      }
    }
    p.type_b[i] = ty;
  }
};

struct PpInterval {
  PostProc p;
  PP_HD int n() const { return p.np; }
  PP_HD void operator()(int i) const
  {
    if (p.aux[i] & 1u) return;                           // (ordinal points keep their type)
    const int c = p.cid[i], gb = p.rank[p.off[c]], cnt = p.rank[p.off[c + 1]] - gb, q = p.rank[i + 1] - gb;
    if (cnt == 0) return;
    if (q == 0) { p.type_b[i] = p.type_b[p.olist[gb]]; return; }
    const int ol = p.olist[gb + q - 1];
    const unsigned lt = p.type_b[ol];
    if (q == cnt) { p.type_b[i] = lt; return; }
    const unsigned rt = p.type_b[p.olist[gb + q]];
    p.type_b[i] = (lt != rt && p.last[i] >= ol) ? rt : lt;
  }
};

struct PpFirst {
  PostProc p;
  PP_HD int n() const { return p.np; }
  PP_HD void operator()(int i) const
  {
    const int c = p.cid[i], b0 = p.off[c];
    if (i > b0 && p.type_b[i] != p.type_b[b0] && p.last[i - 1] < b0) p.first[c] = i - b0;
  }
};

struct PpRotate {
  PostProc p;
  PP_HD int n() const { return p.np; }
  PP_HD void operator()(int i) const
  {
    const int c = p.cid[i], b0 = p.off[c], e0 = p.off[c + 1], len = e0 - b0;
    const int r = (p.loop[c] && p.type_b[b0] == p.type_b[e0 - 1] && p.first[c] >= 0) ? p.first[c] : 0;
    const int pos = i - b0, dest = b0 + (pos >= r ? pos - r : pos - r + len);
    p.type_r[dest] = p.type_b[i]; p.aux_r[dest] = p.aux[i]; p.t_r[dest] = p.t[i]; p.idx_r[dest] = p.indices[i];
  }
};

// split_all on the rotated curves
PP_HD bool pp_split_mode(const PostProc &p, int c) { return p.first[c] >= 0 || p.type_r[p.off[c]] == 0; }
PP_HD bool pp_run_head(const PostProc &p, int i, int b0) { return i == b0 || p.type_r[i] != p.type_r[i - 1]; }
PP_HD bool pp_kept(const PostProc &p, int i, int b0)     // (of a curve in split mode)
{
  if (!pp_run_head(p, i, b0)) return true;
  const int j = p.last[i];
  return (((j == b0 ? 0 : 1) ^ (i - j)) & 1) == 0;
}

struct PpReorder {
  PostProc p;
  PP_HD int n() const { return (int)p.counters[PPC_POINTS]; }
  PP_HD void operator()(int i) const
  {
    const int pc = p.pid_c[i], b = p.poff[pc], e = p.poff[pc + 1];
    bool reverse = false;
    if (!p.ploop[pc]) {
      const unsigned tb = p.aux_c[b] >> 1, te = p.aux_c[e - 1] >> 1;
      reverse = tb == te ? p.t_c[b] > p.t_c[e - 1] : tb > te;
    }
    const int src = reverse ? b + (e - 1 - i) : i;
    p.idx_o[i] = p.idx_c[src]; p.type_o[i] = p.type_c[src]; p.t_o[i] = p.t_c[src];
    p.flag_o[i] = (p.aux_c[src] & 1u ? PPF_ORDINAL : 0) | (i == b ? PPF_HEAD : 0) | (i == e - 1 ? PPF_END : 0);
  }
};

// ---- scans ----------------------------------------------------------------------------------------------------------------------
struct ScanOrdinals {
  typedef int T;
  PostProc p;
  PP_HD int n() const { return p.np; }
  PP_HD static T identity() { return 0; }
  PP_HD static T op(T a, T b) { return a + b; }
  PP_HD T load(int i) const { return (int)(p.aux[i] & 1u); }
  PP_HD void store(int i, T incl, T excl) const
  {
    p.rank[i] = excl;
    if (incl != excl) p.olist[excl] = i;
    if (i == p.np - 1) p.rank[p.np] = incl;
  }
};

// the last point so far for which Pred holds (-1: none yet) -> last[]
template <class Pred> struct ScanLast {
  typedef int T;
  PostProc p;
  PP_HD int n() const { return p.np; }
  PP_HD static T identity() { return -1; }
  PP_HD static T op(T a, T b) { return a > b ? a : b; }
  PP_HD T load(int i) const { return Pred::holds(p, i) ? i : -1; }
  PP_HD void store(int i, T incl, T) const { p.last[i] = incl; }
};
struct PredInGap {      // a point behind an ordinal of its curve whose type is not that ordinal's
  PP_HD static bool holds(const PostProc &p, int i)
  {
    const int gb = p.rank[p.off[p.cid[i]]], q = p.rank[i + 1] - gb;
    return q > 0 && p.type_b[i] != p.type_b[p.olist[gb + q - 1]];
  }
};
struct PredOffFirst {   // a point whose type is not that of its curve's first point
  PP_HD static bool holds(const PostProc &p, int i) { return p.type_b[i] != p.type_b[p.off[p.cid[i]]]; }
};
struct PredAnchor {     // a curve's first point, or a point whose predecessor is no head of a run
  PP_HD static bool holds(const PostProc &p, int i) { const int b0 = p.off[p.cid[i]]; return i == b0 || !pp_run_head(p, i - 1, b0); }
};

struct ScanKept {
  struct T { int kept, heads; };
  PostProc p;
  PP_HD int n() const { return p.np; }
  PP_HD static T identity() { return T{0, 0}; }
  PP_HD static T op(T a, T b) { return T{a.kept + b.kept, a.heads + b.heads}; }
  PP_HD T load(int i) const
  {
    const int c = p.cid[i], b0 = p.off[c];
    if (!pp_split_mode(p, c)) return T{1, i == b0 ? 1 : 0};
    if (!pp_kept(p, i, b0)) return T{0, 0};
    return T{1, (pp_run_head(p, i, b0) || !pp_kept(p, i - 1, b0)) ? 1 : 0};
  }
  PP_HD void store(int i, T incl, T excl) const
  {
    if (incl.kept != excl.kept) {
      const int w = excl.kept, pc = incl.heads - 1;
      p.type_c[w] = p.type_r[i]; p.aux_c[w] = p.aux_r[i]; p.t_c[w] = p.t_r[i]; p.idx_c[w] = p.idx_r[i]; p.pid_c[w] = pc;
      if (incl.heads != excl.heads) {
        const int c = p.cid[i];
        p.poff[pc] = w; p.pcurve[pc] = c; p.ploop[pc] = pp_split_mode(p, c) ? 0 : p.loop[c];
      }
    }
    if (i == p.np - 1) { p.counters[PPC_POINTS] = (unsigned)incl.kept; p.counters[PPC_PIECES] = (unsigned)incl.heads; p.poff[incl.heads] = incl.kept; }
  }
};

struct PpTime { double v; int fresh; int pad; };        // a running value, and whether a restart lies inside what it stands for
struct ScanTimeForward {
  typedef PpTime T;
  PostProc p;
  PP_HD int n() const { return (int)p.counters[PPC_POINTS]; }
  PP_HD static T identity() { return T{-__builtin_huge_val(), 0, 0}; }
  PP_HD static T op(T a, T b) { return T{b.fresh ? b.v : (a.v < b.v ? b.v : a.v), a.fresh | b.fresh, 0}; }   // std::max(a, b)
  PP_HD T load(int i) const { return T{p.t_o[i], (p.flag_o[i] & (PPF_ORDINAL | PPF_HEAD)) ? 1 : 0, 0}; }
  PP_HD void store(int i, T incl, T) const { p.t_f[i] = incl.v; }
};
struct ScanTimeBackward {                                // element k of the scan is point n - 1 - k
  typedef PpTime T;
  PostProc p;
  PP_HD int n() const { return (int)p.counters[PPC_POINTS]; }
  PP_HD static T identity() { return T{__builtin_huge_val(), 0, 0}; }
  PP_HD static T op(T a, T b) { return T{b.fresh ? b.v : (b.v < a.v ? b.v : a.v), a.fresh | b.fresh, 0}; }   // std::min(a, b)
  PP_HD T load(int k) const { const int i = n() - 1 - k; return T{p.t_f[i], (p.flag_o[i] & (PPF_ORDINAL | PPF_END)) ? 1 : 0, 0}; }
  PP_HD void store(int k, T incl, T) const { p.t_out[n() - 1 - k] = incl.v; }
};

// the steps in order: `Run` has map(F) and scan(F), and phase(name) between the groups
template <class Run> void post_process_steps(const PostProc &p, Run &run)
{
  run.map(PpGather{p});
  run.phase("gather");
  run.scan(ScanOrdinals{p});
  run.map(PpSmooth{p});
  run.scan(ScanLast<PredInGap>{p});
  run.map(PpInterval{p});
  run.phase("types: ranks, smoothing, gaps");
  run.scan(ScanLast<PredOffFirst>{p});
  run.map(PpFirst{p});
  run.map(PpRotate{p});
  run.phase("rotate");
  run.scan(ScanLast<PredAnchor>{p});
  run.scan(ScanKept{p});
  run.phase("split, compaction");
  run.map(PpReorder{p});
  run.scan(ScanTimeForward{p});
  run.scan(ScanTimeBackward{p});
  run.phase("reorder, adjust_time");
}

}  // namespace ftkx
