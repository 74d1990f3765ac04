// ftk_amd/csrc/concat_steps.hpp on the CPU, for tests/test_concat_host.py: the plan of a concat launch driven lane by lane -- the direct
// form as the kernel's grid-stride loop, the LDS-staged form (the 16-byte body of float planes) tile by tile and phase by phase, the fill of
// all lanes of a workgroup in front of their drain as the kernel's barrier has it.
//
//   hc_concat(f32, nc, values, count, plane_off, dst_off, nblocks, out, took_vec)
//       the launch concat_kernels.hip would make for nc planes of `count` elements (values: plane k at values + k * count elements, floats
//       where f32, else doubles), plane k starting plane_off[k] ELEMENTS and the destination dst_off doubles behind a 16-byte border,
//       with `nblocks` workgroups (0: as many as concat_blocks says), every lane of every workgroup in turn.
//       0, or which rule was broken: 1 a store outside [0, count * nc), 2 an element written twice, 3 an element never written, 4 a value
//       that is not the widened float / the double's own bits, 5 a plan that breaks its own promises (head, tail, the alignment of the
//       16-byte body, head + G * nvec + tail = count, the grid), 6 the 16-byte body chosen where the rule forbids it or not chosen where it
//       allows it, 7 a staged tile's fill that stored to the destination.  out (nullable): the result; took_vec (nullable): which path ran.
//
// With -DCONCAT_HOST_MAIN: a program of its own (for a sanitizer build, not for loading into Python) that runs cases it makes up.
// Every plane, and the staged form's LDS image, is allocated at exactly its size, so an access behind it is seen; the destination has canaries
// on both sides.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ftk_amd/csrc/concat_steps.hpp"

using namespace ftkx;

namespace {

constexpr uint64_t kUntouched = 0x7ff8dead0badbeefull;      // (the callers keep it out of their FP64 values; no float widens to it)
constexpr size_t kMargin = 4;                                // doubles on either side of the destination

void *aligned16(size_t bytes)
{
  void *p = nullptr;
  if (posix_memalign(&p, 16, bytes ? bytes : 16) != 0) return nullptr;
  return p;
}

uint64_t expected_bits(float f) { const double d = static_cast<double>(f); uint64_t u; memcpy(&u, &d, 8); return u; }
uint64_t expected_bits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

template <class T, int NC> int concat_case(const T *values, size_t count, const int *plane_off, int dst_off, unsigned nblocks, double *out, int *took_vec)
{
  constexpr int G = concat_group<T>();
  T *base[NC];
  ConcatPlanes<T, NC> pl;
  for (int k = 0; k < NC; k ++) {
    base[k] = static_cast<T *>(aligned16(((size_t)plane_off[k] + count) * sizeof(T)));       // exactly: a read behind a plane is the sanitizer's
    if (!base[k]) return -1;
    if (count) memcpy(base[k] + plane_off[k], values + (size_t)k * count, count * sizeof(T));
    pl.p[k] = base[k] + plane_off[k];
  }
  const size_t total = 2 * kMargin + (size_t)dst_off + count * NC, at = kMargin + (size_t)dst_off;
  double *dbase = static_cast<double *>(aligned16(total * sizeof(double))), *blank = static_cast<double *>(aligned16(total * sizeof(double)));
  if (!dbase || !blank) return -1;
  for (size_t i = 0; i < total; i ++) { memcpy(dbase + i, &kUntouched, 8); memcpy(blank + i, &kUntouched, 8); }
  double *dst = dbase + at;
  int rc = 0;
  const ConcatPlan p = concat_plan<T, NC>(pl, count, dst);
  if (took_vec) *took_vec = p.vec ? 1 : 0;
  // the rule, restated: all planes at one address modulo 16, and the destination 16-byte aligned behind the head that brings them there
  bool same = true;
  for (int k = 1; k < NC; k ++) same = same && ((uintptr_t)pl.p[k] & 15) == ((uintptr_t)pl.p[0] & 15);
  const size_t h = ((16 - ((uintptr_t)pl.p[0] & 15)) & 15) / sizeof(T);
  const bool rule = same && (((uintptr_t)(dst + h * NC)) & 15) == 0;
  if (p.vec != rule) rc = 6;
  const size_t tail = count - p.tail_at();
  if (!rc && (p.count != count || p.group != G || p.tail_at() > count)) rc = 5;
  if (!rc && p.vec && (p.head >= (size_t)G || p.head > count || tail >= (size_t)G || p.head + (size_t)G * p.nvec + tail != count)) rc = 5;
  if (!rc && p.vec && p.nvec)
    for (int k = 0; k < NC; k ++) if ((uintptr_t)(pl.p[k] + p.head) & 15) rc = 5;
  if (!rc && p.vec && p.nvec && ((uintptr_t)(dst + p.head * NC) & 15)) rc = 5;
  if (!rc && !p.vec && (p.head != 0 || p.nvec != count || tail != 0)) rc = 5;
  const unsigned planned = concat_blocks(p);
  if (!rc && (planned < 1 || planned > kConcatMaxBlocks || (planned < kConcatMaxBlocks && (size_t)planned * kConcatThreads < p.nvec))) rc = 5;      // (below the cap: a lane per group)
  if (!nblocks) nblocks = planned;
  std::vector<int> written(count * NC, 0);
  // what the call of one lane stored: counted, held to its value, and made untouched again; false: it stored nothing
  auto account = [&]() {
    if (!memcmp(dbase, blank, total * sizeof(double))) return false;
    for (size_t i = 0; i < total && !rc; i ++) {
      uint64_t u;
      memcpy(&u, dbase + i, 8);
      if (u == kUntouched) continue;
      if (i < at || i >= at + count * NC) { rc = 1; break; }
      const size_t e = i - at;
      if (written[e] ++) { rc = 2; break; }
      if (u != expected_bits(values[(e % NC) * count + e / NC])) { rc = 4; break; }
      if (out) memcpy(out + e, &u, 8);
      memcpy(dbase + i, &kUntouched, 8);
    }
    return true;
  };
  if (p.vec && concat_staged<T>()) {
    std::vector<unsigned long long> lds((size_t)concat_tile_words<T, NC>());      // (exactly a tile: an access behind it is the sanitizer's)
    const size_t ntiles = concat_tiles(p);
    for (unsigned b = 0; b < nblocks && !rc; b ++) {
      for (size_t tile = b; tile < ntiles && !rc; tile += nblocks) {
        for (int tid = 0; tid < kConcatThreads && !rc; tid ++) { concat_tile_fill<T, NC>(pl, p, tile, tid, lds.data()); if (account()) rc = 7; }
        for (int tid = 0; tid < kConcatThreads && !rc; tid ++) { concat_tile_drain<T, NC>(lds.data(), p, tile, tid, dst); account(); }
      }
      for (int tid = 0; b == 0 && tid < kConcatThreads && !rc; tid ++) { concat_edges<T, NC>(pl, p, dst, tid); account(); }
    }
  } else {
    for (unsigned b = 0; b < nblocks && !rc; b ++)
      for (int tid = 0; tid < kConcatThreads && !rc; tid ++) {
        if (p.vec) concat_lane<T, NC, true>(pl, p, dst, b, nblocks, tid); else concat_lane<T, NC, false>(pl, p, dst, b, nblocks, tid);
        account();
      }
  }
  for (size_t e = 0; e < count * NC && !rc; e ++) if (written[e] != 1) rc = 3;
  for (int k = 0; k < NC && !rc; k ++)
    if (count && memcmp(base[k] + plane_off[k], values + (size_t)k * count, count * sizeof(T))) rc = 1;       // (the planes are read, never written)
  for (int k = 0; k < NC; k ++) free(base[k]);
  free(dbase); free(blank);
  return rc;
}

}  // namespace

extern "C" int hc_concat(int f32, int nc, const void *values, size_t count, const int *plane_off, int dst_off, unsigned nblocks, double *out, int *took_vec)
{
  if (nc != 2 && nc != 3) return -1;
  if (f32) {
    const float *v = static_cast<const float *>(values);
    return nc == 2 ? concat_case<float, 2>(v, count, plane_off, dst_off, nblocks, out, took_vec) : concat_case<float, 3>(v, count, plane_off, dst_off, nblocks, out, took_vec);
  }
  const double *v = static_cast<const double *>(values);
  return nc == 2 ? concat_case<double, 2>(v, count, plane_off, dst_off, nblocks, out, took_vec) : concat_case<double, 3>(v, count, plane_off, dst_off, nblocks, out, took_vec);
}

extern "C" int hc_concat_group(int f32) { return f32 ? concat_group<float>() : concat_group<double>(); }

#ifdef CONCAT_HOST_MAIN
int main()
{
  // bit patterns from a linear congruential generator (all exponents, NaNs and infinities among them) behind the named values
  uint64_t state = 88172645463325252ull;
  auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state; };
  const uint32_t named32[] = {0u, 0x80000000u, 1u, 0x80000001u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u};
  const uint64_t named64[] = {0ull, 0x8000000000000000ull, 1ull, 0x8000000000000001ull, 0x7ff0000000000000ull, 0xfff0000000000000ull, 0x7ff8000000000000ull, 0xfff8000000000000ull,
                              0x7ff0000000000001ull, 0xfff4000000abcdefull, 0x7fefffffffffffffull, 0x0010000000000000ull};
  long cases = 0;
  for (int f32 = 0; f32 < 2; f32 ++) {
    const int G = hc_concat_group(f32);
    std::vector<size_t> counts;
    for (size_t c = 0; c <= (size_t)(3 * G + 1); c ++) counts.push_back(c);
    counts.push_back(257); counts.push_back(515);
    for (int nc = 2; nc <= 3; nc ++)
      for (size_t count : counts) {
        std::vector<float> v32(count * nc);
        std::vector<double> v64(count * nc);
        for (size_t i = 0; i < count * nc; i ++) {
          uint64_t u = i < 12 ? named64[i] : next();
          if (u == kUntouched) u ^= 1;
          memcpy(&v64[i], &u, 8);
          const uint32_t w = i < 12 ? named32[i] : (uint32_t)(next() >> 32);
          memcpy(&v32[i], &w, 4);
        }
        const void *values = f32 ? (const void *)v32.data() : (const void *)v64.data();
        for (int o = 0; o < G; o ++)
          for (int k = -1; k < nc; k ++)              // -1: all planes at offset o; else plane k at every other offset
            for (int o2 = 0; o2 < G; o2 ++) {
              if (k < 0 ? o2 != 0 : o2 == o) continue;
              int off[3] = {o, o, o};
              if (k >= 0) off[k] = o2;
              for (int dof = 0; dof < 2; dof ++)
                for (unsigned nb = 1; nb <= 3; nb ++) {
                  int vec = -1;
                  std::vector<double> out(count * nc);
                  const int rc = hc_concat(f32, nc, values, count, off, dof, nb, out.data(), &vec);
                  if (rc || (k >= 0 && vec != 0)) {
                    fprintf(stderr, "hc_concat(f32 %d, nc %d, count %zu, planes + %d %d %d, dst + %d, %u blocks): %d (vec %d)\n", f32, nc, count, off[0], off[1], off[2], dof, nb, rc, vec);
                    return 1;
                  }
                  cases ++;
                }
            }
      }
  }
  printf("concat_host run complete (%ld cases)\n", cases);
  return 0;
}
#endif
