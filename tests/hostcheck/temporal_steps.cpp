// ftk_amd/csrc/temporal_steps.hpp on the CPU, as a program of its own (for a sanitizer build): the state machine drives a deque of arrays
// the way ftkx_api.hip drives the context's ring, and every emission is added up by temporal_kernels.hip's loops restated around the
// header's own functions -- temporal_plan(), the workgroups of temporal_blocks() in order, temporal_lane() for each of their 256 lanes.
// What the GPU adds is parallelism only.
//
//   temporal_steps run IN OUT [IN OUT ...]
//     IN : int64 ksize, N, count, offset; double weights[ksize]; double data[N][count]
//     OUT: int64 n_emitted, n_steps; int64 steps[n_steps][2 + ksize] (0 push / 1 finish, emitted, the deque places of the taps);
//          double out[n_emitted][count]
//     offset 1: every array and the output start 8 bytes off a multiple of 16 (the kernel's 8-byte path); 0: on one (16-byte path).
//     Every array ends where its allocation ends, so a read or a store behind one is seen.
//   temporal_steps admit         prints what temporal_admit() says to scalar after scalar, vector after scalar, scalar after vector,
//                                a push with the filter off, a push while finishing
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>
#include "../../ftk_amd/csrc/temporal_steps.hpp"

using namespace ftkx;

namespace {

struct Array {      // `count` doubles at the asked offset from a multiple of 16, ending where the allocation ends
  void *base = nullptr;
  double *p = nullptr;
  Array(size_t count, int offset)
  {
    if (posix_memalign(&base, 16, count * 8 + (offset ? 8 : 0))) base = nullptr;
    if (base) p = reinterpret_cast<double *>(static_cast<char *>(base) + (offset ? 8 : 0));
  }
  ~Array() { free(base); }
  Array(const Array &) = delete;
};

template <int K, int NSRC, int W> void emit_knw(const TemporalArgs &a, size_t count, double *out)
{
  const unsigned blocks = temporal_blocks(count, W);
  for (unsigned b = 0; b < blocks; b ++)
    for (int tid = 0; tid < kTemporalThreads; tid ++) temporal_lane<K, NSRC, W>(a, count, out, b, blocks, tid);
}

template <int K, int NSRC> struct Emit {
  static int go(int nsrc, const TemporalArgs &a, size_t count, double *out)
  {
    if (nsrc != NSRC) return Emit<K, NSRC - 1>::go(nsrc, a, count, out);
    if (temporal_aligned16(a, NSRC, out)) emit_knw<K, NSRC, 2>(a, count, out); else emit_knw<K, NSRC, 1>(a, count, out);
    return 0;
  }
};
template <int K> struct Emit<K, 0> { static int go(int, const TemporalArgs &, size_t, double *) { return -1; } };

int emit(const double *const *arrays, int ksize, const double *w, size_t count, double *out)
{
  TemporalArgs a;
  const int nsrc = temporal_plan(arrays, ksize, w, &a);
  switch (ksize) {
  case 1: return Emit<1, 1>::go(nsrc, a, count, out);
  case 3: return Emit<3, 3>::go(nsrc, a, count, out);
  case 5: return Emit<5, 5>::go(nsrc, a, count, out);
  case 7: return Emit<7, 7>::go(nsrc, a, count, out);
  case 9: return Emit<9, 9>::go(nsrc, a, count, out);
  default: return -1;
  }
}

int run(const char *in, const char *outp)
{
  FILE *f = fopen(in, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", in); return 1; }
  long long h[4];
  if (fread(h, 8, 4, f) != 4) return 1;
  const int ksize = (int)h[0], N = (int)h[1], offset = (int)h[3];
  const size_t count = (size_t)h[2];
  if (!temporal_ksize_ok(ksize)) { fprintf(stderr, "ksize %d\n", ksize); return 1; }
  std::vector<double> w((size_t)ksize);
  if (fread(w.data(), 8, (size_t)ksize, f) != (size_t)ksize) return 1;
  TemporalSeries s;
  s.ksize = ksize;
  std::deque<Array *> ring;
  std::vector<Array *> emitted;
  std::vector<long long> steps;
  auto emission = [&](int phase, bool emits, const int *idx) -> int {
    steps.push_back(phase); steps.push_back(emits ? 1 : 0);
    for (int i = 0; i < ksize; i ++) steps.push_back(emits ? idx[i] : -1);
    if (!emits) return 0;
    const double *arrays[kTemporalMaxK];
    for (int i = 0; i < ksize; i ++) {
      if (idx[i] < 0 || idx[i] >= (int)ring.size() || s.size != (int)ring.size()) { fprintf(stderr, "tap %d reads place %d of %zu\n", i, idx[i], ring.size()); return 1; }
      arrays[i] = ring[(size_t)idx[i]]->p;
    }
    Array *o = new Array(count, offset);
    emitted.push_back(o);
    return emit(arrays, ksize, w.data(), count, o->p);
  };
  for (int k = 0; k < N; k ++) {
    if (temporal_admit(s, 0) != TEMPORAL_ADMIT_OK) return 1;
    Array *a = new Array(count, offset);
    if (!a->p || fread(a->p, 8, count, f) != count) return 1;
    ring.push_back(a);
    bool pop = false;
    int idx[kTemporalMaxK];
    const bool emits = temporal_push(s, 0, &pop, idx);
    if (pop) { delete ring.front(); ring.pop_front(); }
    if (emission(0, emits, idx)) return 1;
  }
  fclose(f);
  for (;;) {
    bool pop = false;
    int idx[kTemporalMaxK];
    const bool emits = temporal_finish_step(s, &pop, idx);
    if (pop) { delete ring.front(); ring.pop_front(); }
    if (emission(1, emits, idx)) return 1;
    if (!emits) break;
  }
  if (s.size != 0 || s.cursor != 0 || s.finishing || s.kind != -1) { fprintf(stderr, "the filter is not in its initial state\n"); return 1; }
  for (Array *a : ring) delete a;
  f = fopen(outp, "wb");
  if (!f) return 1;
  const long long head[2] = {(long long)emitted.size(), (long long)(steps.size() / (size_t)(2 + ksize))};
  fwrite(head, 8, 2, f);
  fwrite(steps.data(), 8, steps.size(), f);
  for (Array *a : emitted) { fwrite(a->p, 8, count, f); delete a; }
  fclose(f);
  return 0;
}

}  // namespace

int main(int argc, char **argv)
{
  if (argc == 2 && !strcmp(argv[1], "admit")) {
    TemporalSeries s;
    const int off = temporal_admit(s, 0);
    s.ksize = 5;
    bool pop; int idx[kTemporalMaxK];
    const int first = temporal_admit(s, 0);
    temporal_push(s, 0, &pop, idx);
    const int ss = temporal_admit(s, 0), sv = temporal_admit(s, 1);
    TemporalSeries v; v.ksize = 3;
    temporal_push(v, 1, &pop, idx);
    const int vs = temporal_admit(v, 0), vv = temporal_admit(v, 1);
    temporal_push(s, 0, &pop, idx); temporal_push(s, 0, &pop, idx); temporal_push(s, 0, &pop, idx);
    temporal_finish_step(s, &pop, idx);
    const int fin = temporal_admit(s, 0);
    while (temporal_finish_step(s, &pop, idx)) {}
    const int again = temporal_admit(s, 1);      // a new series may be of the other kind
    printf("admit off=%d first=%d scalar_scalar=%d scalar_vector=%d vector_scalar=%d vector_vector=%d finishing=%d after=%d\n", off, first, ss, sv, vs, vv, fin, again);
    return 0;
  }
  if (argc < 4 || strcmp(argv[1], "run") || (argc & 1)) { fprintf(stderr, "usage: temporal_steps run IN OUT [IN OUT ...] | admit\n"); return 2; }
  for (int a = 2; a + 1 < argc; a += 2) if (run(argv[a], argv[a + 1])) { fprintf(stderr, "failed on %s\n", argv[a]); return 1; }
  printf("temporal_steps run complete\n");
  return 0;
}
