// ftk_amd/csrc/narrow_steps.hpp on the CPU, for tests/test_narrow_host.py: the conversion of one element of every narrow type, and the plan of
// a narrow launch driven lane by lane.
//
//   hc_narrow_one(dtype, values, count, out)                  out[i] = narrow_one(values[i]) for `count` elements of type `dtype` (FTKX_DTYPE_*)
//   hc_narrow(dtype, values, count, src_off, dst_off, out)    the launch narrow_kernels.hip would make for a source `src_off` ELEMENTS behind a border
//                                                             of 4 elements' bytes and a destination `dst_off` doubles behind a 16-byte border,
//                                                             every lane of every workgroup in turn.  0, or which rule was broken: 1 a store outside
//                                                             [0, count), 2 an element written twice, 3 an element never written, 4 a value that is
//                                                             not narrow_one of its element, 5 a plan that breaks its own promises (head, alignment
//                                                             of the body, grid), -1 an unknown dtype.  out: the result.
//   hc_narrow_grid(..., nblocks, out)                         hc_narrow with a grid of `nblocks` workgroups instead of the plan's: fewer lanes than groups, so
//                                                             that the grid-stride loop goes round (two groups a turn, then the odd one) at small counts
//   hc_narrow_form(dtype, count, src_off, dst_off)            1: that launch takes the 4-element body, 0: it goes element by element
//
// With -DNARROW_HOST_MAIN: a program of its own (for a sanitizer build, not for loading into Python) that runs both over cases it makes up.
// The source of a case is allocated at exactly its size, so a read behind it is seen; the destination has canaries on both sides.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ftk_amd/csrc/narrow_steps.hpp"

using namespace ftkx;

namespace {

constexpr uint64_t kUntouched = 0x7ff8dead0badbeefull;      // a NaN nothing narrow widens to (the low 29 bits of every widened value are zero)
constexpr size_t kMargin = 4;                                // doubles on either side of the destination

uint64_t bits_of(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

void *aligned16(size_t bytes)
{
  void *p = nullptr;
  if (posix_memalign(&p, 16, bytes ? bytes : 16) != 0) return nullptr;
  return p;
}

template <class T> void one(const void *values, size_t count, double *out)
{
  const T *v = static_cast<const T *>(values);
  for (size_t i = 0; i < count; i ++) out[i] = narrow_one(v[i]);
}

template <class T> int run(const void *values, size_t count, int src_off, int dst_off, double *out, int *form, unsigned grid = 0)
{
  T *sbase = static_cast<T *>(aligned16(((size_t)src_off + count) * sizeof(T)));            // exactly: a read behind the source is the sanitizer's
  double *dbase = static_cast<double *>(aligned16((2 * kMargin + (size_t)dst_off + count) * sizeof(double)));
  if (!sbase || !dbase) return -1;
  T *src = sbase + src_off;
  double *dst = dbase + kMargin + dst_off;
  const size_t total = 2 * kMargin + (size_t)dst_off + count;
  const T *vals = static_cast<const T *>(values);
  if (count && values) memcpy(src, values, count * sizeof(T));
  for (size_t i = 0; i < total; i ++) memcpy(dbase + i, &kUntouched, 8);
  int rc = 0;
  const NarrowPlan p = narrow_plan(src, sizeof(T), count, dst);
  const unsigned planned = narrow_blocks(p), nblocks = grid ? grid : planned;
  const size_t load = 4 * sizeof(T);
  if (form) *form = p.vec ? 1 : 0;
  if (p.head > 3 || p.head > count || p.tail_at() > count || count - p.tail_at() > 3) rc = 5;
  if (p.vec && ((((size_t)(src + p.head)) & (load - 1)) || (((size_t)(dst + p.head)) & 15) || p.head + p.nvec * 4 > count)) rc = 5;
  if (!p.vec && (p.head != 0 || p.nvec != count)) rc = 5;
  if (planned < 1 || planned > kWidenMaxBlocks || (planned < kWidenMaxBlocks && (size_t)planned * kWidenThreads < p.nvec)) rc = 5;      // (below the cap: a lane per group)
  std::vector<int> written(count, 0);
  for (unsigned b = 0; b < nblocks && !rc && values; b ++)
    for (int tid = 0; tid < kWidenThreads && !rc; tid ++) {
      if (p.vec) narrow_lane<T, true>(src, p, dst, b, nblocks, tid); else narrow_lane<T, false>(src, p, dst, b, nblocks, tid);
      for (size_t i = 0; i < total && !rc; i ++) {
        if (bits_of(dbase[i]) == kUntouched) continue;
        const size_t at = kMargin + (size_t)dst_off;
        if (i < at || i >= at + count) { rc = 1; break; }
        const size_t e = i - at;
        if (written[e] ++) { rc = 2; break; }
        if (bits_of(dbase[i]) != bits_of(narrow_one(vals[e]))) { rc = 4; break; }
        if (out) out[e] = dbase[i];
        memcpy(dbase + i, &kUntouched, 8);
      }
    }
  for (size_t e = 0; e < count && !rc && values; e ++) if (written[e] != 1) rc = 3;
  free(sbase); free(dbase);
  return rc;
}

}  // namespace

#define NARROW_CASES(call) \
  switch (dtype) { \
  case NARROW_F16: return call(NarrowHalf); case NARROW_BF16: return call(NarrowBf16); \
  case NARROW_U8: return call(uint8_t); case NARROW_I8: return call(int8_t); case NARROW_U16: return call(uint16_t); case NARROW_I16: return call(int16_t); \
  case NARROW_U32: return call(uint32_t); case NARROW_I32: return call(int32_t); \
  default: return -1; \
  }

extern "C" int hc_narrow_one(int dtype, const void *values, size_t count, double *out)
{
#define ONE(T) (one<T>(values, count, out), 0)
  NARROW_CASES(ONE)
#undef ONE
}

extern "C" int hc_narrow(int dtype, const void *values, size_t count, int src_off, int dst_off, double *out)
{
#define RUN(T) run<T>(values, count, src_off, dst_off, out, nullptr)
  NARROW_CASES(RUN)
#undef RUN
}

extern "C" int hc_narrow_grid(int dtype, const void *values, size_t count, int src_off, int dst_off, unsigned nblocks, double *out)
{
#define RUN(T) run<T>(values, count, src_off, dst_off, out, nullptr, nblocks)
  NARROW_CASES(RUN)
#undef RUN
}

extern "C" int hc_narrow_form(int dtype, size_t count, int src_off, int dst_off)
{
  int form = -1;
#define FORM(T) (run<T>(nullptr, count, src_off, dst_off, nullptr, &form) == 0 ? form : -2)
  NARROW_CASES(FORM)
#undef FORM
}

extern "C" size_t hc_narrow_dtype_size(int dtype) { return narrow_dtype_size(dtype); }

#ifdef NARROW_HOST_MAIN
int main()
{
  uint32_t state = 12345u;
  auto next = [&]() { state = state * 1664525u + 1013904223u; return state; };
  const size_t counts[] = {0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025};
  int forms[2] = {0, 0};
  for (int dtype = NARROW_F16; dtype <= NARROW_I32; dtype ++) {
    const size_t esize = narrow_dtype_size(dtype);
    for (size_t count : counts)
      for (int so = 0; so < 4; so ++)
        for (int dof = 0; dof < 2; dof ++) {
          std::vector<uint32_t> v((count * esize + 3) / 4 + 1);      // random bit patterns: every value of the 8- and 16-bit types' classes among them
          for (uint32_t &w : v) w = next() ^ (next() >> 16);
          std::vector<double> out(count);
          const int rc = hc_narrow(dtype, v.data(), count, so, dof, out.data());
          if (rc) { fprintf(stderr, "hc_narrow(dtype %d, count %zu, src + %d, dst + %d): %d\n", dtype, count, so, dof, rc); return 1; }
          const int f = hc_narrow_form(dtype, count, so, dof);
          if (f < 0) { fprintf(stderr, "hc_narrow_form(dtype %d, count %zu, src + %d, dst + %d): %d\n", dtype, count, so, dof, f); return 1; }
          forms[f] ++;
        }
  }
  // a grid smaller than the body: 1 - 5 turns of the loop per lane, pairs and the odd one
  for (int dtype = NARROW_F16; dtype <= NARROW_I32; dtype ++)
    for (size_t count : {(size_t)1029, (size_t)2100, (size_t)5003})
      for (unsigned grid = 1; grid <= 2; grid ++) {
        std::vector<uint32_t> v(count + 1);
        for (uint32_t &w : v) w = next();
        std::vector<double> out(count);
        const int rc = hc_narrow_grid(dtype, v.data(), count, 1, 1, grid, out.data());
        if (rc) { fprintf(stderr, "hc_narrow_grid(dtype %d, count %zu, grid %u): %d\n", dtype, count, grid, rc); return 1; }
      }
  if (!forms[0] || !forms[1]) { fprintf(stderr, "one of the two forms was never taken\n"); return 1; }
  // every pattern of the 16-bit types through narrow_one
  std::vector<uint16_t> all(65536);
  for (size_t i = 0; i < all.size(); i ++) all[i] = (uint16_t)i;
  std::vector<double> out(all.size());
  for (int dtype : {(int)NARROW_F16, (int)NARROW_BF16, (int)NARROW_U16, (int)NARROW_I16})
    if (hc_narrow_one(dtype, all.data(), all.size(), out.data())) return 1;
  printf("narrow_host run complete\n");
  return 0;
}
#endif
