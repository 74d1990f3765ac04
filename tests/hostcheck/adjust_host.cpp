// ftk_amd/csrc/adjust_steps.hpp on the CPU, for tests/test_adjust_host.py and as the oracle of tests/test_gpu_adjust.py: the pieces of the
// noise one by one, the scalar function of (seed, t, e), and the plan of a launch driven lane by lane.
//
//   hc_philox(ctr[4], key[2], out[4])                   Philox4x32-10
//   hc_uniform(w_hi, w_lo)                              the element's two words -> u
//   hc_ppnd16(u, out, n), hc_log(x, out, n)             AS 241 and the header's own log, n values each
//   hc_clamp(x, n, lo, hi, out)                         the reference's min(max(lo, x), hi)
//   hc_adjust_f64 / hc_adjust_f32(src, count, e0, perturb, sigma, seed, t, clamp, lo, hi, out)
//                                                       out[i] = the scalar function for element e0 + i holding src[i]
//   hc_plan_f64 / hc_plan_f32(values, count, src_off, dst_off, in_place, perturb, sigma, seed, t, clamp, lo, hi, out)
//                                                       the launch adjust_kernels.hip would make for a source `src_off` elements and a destination
//                                                       `dst_off` doubles behind a 16-byte border (in_place: the destination IS the source, doubles
//                                                       only), every lane of every workgroup in turn.  0, or which rule was broken: 1 a store outside
//                                                       [0, count), 2 an element written twice, 3 an element never written, 4 a value that is not the
//                                                       scalar function's, 5 a plan that breaks its own promises, 6 a source that changed (out of place).
//                                                       out: the result.
//
// With -DADJUST_HOST_MAIN: a program of its own (for a sanitizer build, not for loading into Python) that runs the plan over cases it makes up.
// The source is allocated at exactly its size, so a read behind it is seen; the destination has canaries on both sides.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ftk_amd/csrc/adjust_steps.hpp"

using namespace ftkx;

namespace {

constexpr size_t kMargin = 4;                                // doubles on either side of the destination

uint64_t bits_of(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

void *aligned16(size_t bytes)
{
  void *p = nullptr;
  if (posix_memalign(&p, 16, bytes ? bytes : 16) != 0) return nullptr;
  return p;
}

template <class T> double scalar(T x, size_t e, bool perturb, bool clamp, const AdjustArgs &a)
{
  if (perturb && clamp) return adjust_one<T, true, true>(x, e, a);
  if (perturb) return adjust_one<T, true, false>(x, e, a);
  if (clamp) return adjust_one<T, false, true>(x, e, a);
  return static_cast<double>(x);
}

template <class T> void lane(const T *src, const AdjustPlan &p, bool perturb, bool clamp, const AdjustArgs &a, double *dst, size_t b, size_t nb, int tid)
{
  if (perturb && clamp) adjust_lane<T, true, true>(src, p, a, dst, b, nb, tid);
  else if (perturb) adjust_lane<T, true, false>(src, p, a, dst, b, nb, tid);
  else adjust_lane<T, false, true>(src, p, a, dst, b, nb, tid);
}

// Out of place the destination starts as canaries and every store is seen at once.  In place the destination starts as the values: a
// store is seen where the scalar function changes the value, and the final sweep holds every element to the function either way.
template <class T> int plan(const T *values, size_t count, int src_off, int dst_off, bool in_place, bool perturb, bool clamp, const AdjustArgs &a, double *out)
{
  if (!perturb && !clamp) return -1;
  if (in_place && sizeof(T) != sizeof(double)) return -1;
  const uint64_t canary = 0x7ff8dead0badbeefull;
  T *sbase = static_cast<T *>(aligned16(((size_t)src_off + count) * sizeof(T)));            // exactly: a read behind the source is the sanitizer's
  const size_t total = 2 * kMargin + (size_t)dst_off + count, at = kMargin + (size_t)dst_off;
  double *dbase = static_cast<double *>(aligned16(total * sizeof(double)));
  if (!sbase || !dbase) return -1;
  T *src = sbase + src_off;
  double *dst = dbase + at;
  if (count) memcpy(src, values, count * sizeof(T));
  for (size_t i = 0; i < total; i ++) memcpy(dbase + i, &canary, 8);
  if (in_place) { if (count) memcpy(dst, values, count * sizeof(double)); }
  const T *from = in_place ? reinterpret_cast<const T *>(dst) : src;
  int rc = 0;
  const AdjustPlan p = adjust_plan<T>(from, count, dst);
  const unsigned nblocks = adjust_blocks(p);
  if (p.count != count || p.npair != count / 2) rc = 5;
  if (p.vec && ((((size_t)from) & (2 * sizeof(T) - 1)) || (((size_t)dst) & 15))) rc = 5;
  if (nblocks < 1 || nblocks > kAdjustMaxBlocks || (nblocks < kAdjustMaxBlocks && (size_t)nblocks * kAdjustThreads < p.npair)) rc = 5;      // (below the cap: a lane per pair)
  std::vector<unsigned char> written(count, 0);
  std::vector<double> seen(total);
  memcpy(seen.data(), dbase, total * sizeof(double));
  for (unsigned b = 0; b < nblocks && !rc; b ++)
    for (int tid = 0; tid < kAdjustThreads && !rc; tid ++) {
      // what this lane may touch: its pairs, and (lane 0 of workgroup 0) the tail -- everything else is compared with what was there
      lane<T>(from, p, perturb, clamp, a, dst, b, nblocks, tid);
      const size_t stride = (size_t)nblocks * kAdjustThreads;
      for (size_t g = (size_t)b * kAdjustThreads + (size_t)tid; g < p.npair && !rc; g += stride)
        for (size_t e = 2 * g; e < 2 * g + 2; e ++) {
          if (written[e] ++) { rc = 2; break; }
          if (bits_of(dst[e]) != bits_of(scalar<T>(values[e], e, perturb, clamp, a))) { rc = 4; break; }
          seen[at + e] = dst[e];
        }
      if (b == 0 && tid == 0 && (count & 1) && !rc) {
        const size_t e = count - 1;
        if (written[e] ++) rc = 2;
        else if (bits_of(dst[e]) != bits_of(scalar<T>(values[e], e, perturb, clamp, a))) rc = 4;
        seen[at + e] = dst[e];
      }
    }
  // nothing but what the lanes were entitled to has changed: canaries, and elements of other lanes
  if (!rc && memcmp(seen.data(), dbase, total * sizeof(double)) != 0) {
    rc = 1;
    for (size_t e = 0; e < count; e ++) if (bits_of(seen[at + e]) != bits_of(dst[e])) rc = 2;
  }
  for (size_t i = 0; i < total && !rc; i ++) if ((i < at || i >= at + count) && bits_of(dbase[i]) != canary) rc = 1;
  for (size_t e = 0; e < count && !rc; e ++) if (written[e] != 1) rc = 3;
  if (!in_place && count && !rc && memcmp(src, values, count * sizeof(T)) != 0) rc = 6;
  if (out && count) memcpy(out, dst, count * sizeof(double));
  free(sbase); free(dbase);
  return rc;
}

}  // namespace

extern "C" void hc_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out) { philox4x32_10(ctr, key, out); }
extern "C" double hc_uniform(uint32_t w_hi, uint32_t w_lo) { return adjust_uniform(w_hi, w_lo); }
extern "C" void hc_ppnd16(const double *u, double *out, size_t n) { for (size_t i = 0; i < n; i ++) out[i] = adjust_ppnd16(u[i]); }
extern "C" void hc_log(const double *x, double *out, size_t n) { for (size_t i = 0; i < n; i ++) out[i] = adjust_log(x[i]); }
extern "C" void hc_clamp(const double *x, size_t n, double lo, double hi, double *out) { for (size_t i = 0; i < n; i ++) out[i] = adjust_clamp(x[i], lo, hi); }

extern "C" void hc_adjust_f64(const double *src, size_t count, size_t e0, int perturb, double sigma, unsigned long long seed, int t, int clamp, double lo, double hi, double *out)
{
  const AdjustArgs a{sigma, seed, t, lo, hi};
  for (size_t i = 0; i < count; i ++) out[i] = scalar<double>(src[i], e0 + i, perturb != 0, clamp != 0, a);
}

extern "C" void hc_adjust_f32(const float *src, size_t count, size_t e0, int perturb, double sigma, unsigned long long seed, int t, int clamp, double lo, double hi, double *out)
{
  const AdjustArgs a{sigma, seed, t, lo, hi};
  for (size_t i = 0; i < count; i ++) out[i] = scalar<float>(src[i], e0 + i, perturb != 0, clamp != 0, a);
}

extern "C" int hc_plan_f64(const double *values, size_t count, int src_off, int dst_off, int in_place, int perturb, double sigma, unsigned long long seed, int t, int clamp,
                           double lo, double hi, double *out)
{
  const AdjustArgs a{sigma, seed, t, lo, hi};
  return plan<double>(values, count, src_off, dst_off, in_place != 0, perturb != 0, clamp != 0, a, out);
}

extern "C" int hc_plan_f32(const float *values, size_t count, int src_off, int dst_off, int in_place, int perturb, double sigma, unsigned long long seed, int t, int clamp,
                           double lo, double hi, double *out)
{
  const AdjustArgs a{sigma, seed, t, lo, hi};
  return plan<float>(values, count, src_off, dst_off, in_place != 0, perturb != 0, clamp != 0, a, out);
}

#ifdef ADJUST_HOST_MAIN
int main()
{
  uint64_t state = 12345u;
  auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state; };
  const uint64_t named[] = {0ull, 0x8000000000000000ull, 1ull, 0x8000000000000001ull, 0x7ff0000000000000ull, 0xfff0000000000000ull, 0x7ff8000000000000ull, 0xfff8000000000000ull,
                            0x7fefffffffffffffull, 0xffefffffffffffffull, 0x3ff0000000000000ull, 0xbff0000000000000ull};
  const size_t counts[] = {0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, (size_t)2048 * 256 * 2 - 1, (size_t)2048 * 256 * 2, (size_t)2048 * 256 * 2 + 1};
  for (size_t count : counts) {
    const bool big = count > 2000;
    std::vector<double> v(count), out(count);
    std::vector<float> vf(count);
    for (size_t i = 0; i < count; i ++) {
      uint64_t b = i < sizeof(named) / 8 ? named[i] : next();
      if (i >= sizeof(named) / 8 && (i & 3)) { const double d = (double)(int64_t)b / 9223372036854775808.0 * 2.0; memcpy(&b, &d, 8); }      // mostly values near the bounds
      memcpy(&v[i], &b, 8);
      const uint32_t bf = (uint32_t)(b >> 32);
      memcpy(&vf[i], &bf, 4);
    }
    for (int so = 0; so < 4; so ++)
      for (int dof = 0; dof < 2; dof ++)
        for (int mode = 1; mode <= 3; mode ++) {
          if (big && !(so == 1 && dof == 1 && mode == 3) && !(so == 0 && dof == 0 && mode == 2)) continue;      // (the large counts: two variants each)
          const int perturb = mode & 1, clamp = mode >> 1;
          int rc = hc_plan_f64(v.data(), count, so & 1, dof, 0, perturb, 0.25, 12345ull, 7, clamp, -1.0, 1.0, out.data());
          if (rc) { fprintf(stderr, "hc_plan_f64(count %zu, src + %d, dst + %d, mode %d): %d\n", count, so & 1, dof, mode, rc); return 1; }
          rc = hc_plan_f64(v.data(), count, 0, dof, 1, perturb, 0.25, 12345ull, 7, clamp, -1.0, 1.0, out.data());
          if (rc) { fprintf(stderr, "hc_plan_f64(count %zu, in place at + %d, mode %d): %d\n", count, dof, mode, rc); return 1; }
          rc = hc_plan_f32(vf.data(), count, so, dof, 0, perturb, 0.25, 12345ull, 7, clamp, -1.0, 1.0, out.data());
          if (rc) { fprintf(stderr, "hc_plan_f32(count %zu, src + %d, dst + %d, mode %d): %d\n", count, so, dof, mode, rc); return 1; }
        }
  }
  printf("adjust_host run complete\n");
  return 0;
}
#endif
