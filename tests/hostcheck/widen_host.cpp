// ftk_amd/csrc/widen_steps.hpp on the CPU, for tests/test_widen_host.py: the plan of a widen launch driven lane by lane, and the float-source
// staging of the convolution (conv_steps.hpp, conv_stage) against the double-source one on the widened array.
//
//   hc_widen(values, count, src_off, dst_off, out)      the launch widen_kernels.hip would make for a source `src_off` floats and a destination
//                                                       `dst_off` doubles behind a 16-byte border, every lane of every workgroup in turn.
//                                                       0, or which rule was broken: 1 a store outside [0, count), 2 an element written twice,
//                                                       3 an element never written, 4 a value that is not static_cast<double>, 5 a plan that
//                                                       breaks its own promises (head, alignment of the 16-byte body, grid).  out: the result.
//   hc_conv_f32(nd, ksize, S32, DW, DH, DD, w, out)     every tile staged from the floats AND from the widened doubles: the number of staged
//                                                       values whose bits differ (-1: a size the kernel does not have); out (nullable): the
//                                                       convolution computed from the float-staged tiles, with the kernel's loops.
//
// With -DWIDEN_HOST_MAIN: a program of its own (for a sanitizer build, not for loading into Python) that runs both over cases it makes up.
// The source of a widen case is allocated at exactly its size, so a read behind it is seen; the destination has canaries on both sides.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ftk_amd/csrc/conv_steps.hpp"
#include "../../ftk_amd/csrc/widen_steps.hpp"

using namespace ftkx;

namespace {

constexpr uint64_t kUntouched = 0x7ff8dead0badbeefull;      // a NaN no float widens to (the low 29 bits of a widened float are zero)
constexpr size_t kMargin = 4;                                // doubles on either side of the destination

uint64_t bits_of(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

void *aligned16(size_t bytes)
{
  void *p = nullptr;
  if (posix_memalign(&p, 16, bytes ? bytes : 16) != 0) return nullptr;
  return p;
}

template <int ND, int K, class SRC> void stage_tile(const SRC *S, const ConvDims &d, int x0, int y0, int z0, double *tile)
{
  typedef ConvTile<ND, K> T;
  for (int tid = 0; tid < kConvThreads; tid ++)
    for (int i = tid; i < T::STAGED; i += kConvThreads) conv_stage<ND, K>(S, d, x0, y0, z0, i, tile);
}

template <int ND, int K> long conv_f32(const float *S, const ConvDims &d, const double *w, double *out)
{
  typedef ConvTile<ND, K> T;
  const size_t n = (size_t)d.DW * (size_t)d.DH * (size_t)d.DD;
  std::vector<double> wide(n);
  for (size_t i = 0; i < n; i ++) wide[i] = widen_one(S[i]);
  double *tf = static_cast<double *>(aligned16(sizeof(double) * T::DOUBLES)), *td = static_cast<double *>(aligned16(sizeof(double) * T::DOUBLES));
  for (int i = 0; i < T::DOUBLES; i ++) { memcpy(tf + i, &kUntouched, 8); memcpy(td + i, &kUntouched, 8); }
  long differ = 0;
  const size_t ntiles = conv_tiles<ND, K>(d);
  for (size_t t = 0; t < ntiles; t ++) {
    int x0, y0, z0;
    conv_tile_origin<ND, K>(d, t, &x0, &y0, &z0);
    stage_tile<ND, K, float>(S, d, x0, y0, z0, tf);
    stage_tile<ND, K, double>(wide.data(), d, x0, y0, z0, td);
    for (int i = 0; i < T::DOUBLES; i ++) differ += bits_of(tf[i]) != bits_of(td[i]);
    if (!out) continue;
    for (int tid = 0; tid < kConvThreads; tid ++) {
      int tx, ty, tz;
      conv_lane<ND, K>(tid, &tx, &ty, &tz);
      const int gx = x0 + tx * T::R, gy = y0 + ty;
      for (int oz = tz; oz < T::TZ; oz += T::LZ) {
        const int gz = z0 + oz;
        if (gx >= d.DW || gy >= d.DH || gz >= d.DD) continue;
        double res[T::R];
        conv_outputs<ND, K>(tf + (oz * T::PY + ty) * T::PX + tx * T::R, w, res);
        double *o = out + ((size_t)gz * (size_t)d.DH + (size_t)gy) * (size_t)d.DW + (size_t)gx;
        for (int r = 0; r < T::R; r ++) if (gx + r < d.DW) o[r] = res[r];
      }
    }
  }
  free(tf); free(td);
  return differ;
}

}  // namespace

extern "C" int hc_widen(const float *values, size_t count, int src_off, int dst_off, double *out)
{
  float *sbase = static_cast<float *>(aligned16(((size_t)src_off + count) * sizeof(float)));            // exactly: a read behind the source is the sanitizer's
  double *dbase = static_cast<double *>(aligned16((2 * kMargin + (size_t)dst_off + count) * sizeof(double)));
  if (!sbase || !dbase) return -1;
  float *src = sbase + src_off;
  double *dst = dbase + kMargin + dst_off;
  const size_t total = 2 * kMargin + (size_t)dst_off + count;
  if (count) memcpy(src, values, count * sizeof(float));
  for (size_t i = 0; i < total; i ++) memcpy(dbase + i, &kUntouched, 8);
  int rc = 0;
  const WidenPlan p = widen_plan(src, count, dst);
  const unsigned nblocks = widen_blocks(p);
  if (p.head > 3 || p.head > count || p.tail_at() > count || count - p.tail_at() > 3) rc = 5;
  if (p.vec && ((((size_t)(src + p.head)) & 15) || (((size_t)(dst + p.head)) & 15) || p.head + p.nvec * 4 > count)) rc = 5;
  if (!p.vec && (p.head != 0 || p.nvec != count)) rc = 5;
  if (nblocks < 1 || nblocks > kWidenMaxBlocks || (nblocks < kWidenMaxBlocks && (size_t)nblocks * kWidenThreads < p.nvec)) rc = 5;      // (below the cap: a lane per group)
  std::vector<int> written(count, 0);
  for (unsigned b = 0; b < nblocks && !rc; b ++)
    for (int tid = 0; tid < kWidenThreads && !rc; tid ++) {
      if (p.vec) widen_lane<true>(src, p, dst, b, nblocks, tid); else widen_lane<false>(src, p, dst, b, nblocks, tid);
      for (size_t i = 0; i < total && !rc; i ++) {
        if (bits_of(dbase[i]) == kUntouched) continue;
        const size_t at = kMargin + (size_t)dst_off;
        if (i < at || i >= at + count) { rc = 1; break; }
        const size_t e = i - at;
        if (written[e] ++) { rc = 2; break; }
        if (bits_of(dbase[i]) != bits_of(static_cast<double>(values[e]))) { rc = 4; break; }
        if (out) out[e] = dbase[i];
        memcpy(dbase + i, &kUntouched, 8);
      }
    }
  for (size_t e = 0; e < count && !rc; e ++) if (written[e] != 1) rc = 3;
  free(sbase); free(dbase);
  return rc;
}

extern "C" long hc_conv_f32(int nd, int ksize, const float *S, int DW, int DH, int DD, const double *w, double *out)
{
  const ConvDims d{DW, DH, nd == 2 ? 1 : DD};
#define CONV_CASE(k) case k: return nd == 2 ? conv_f32<2, k>(S, d, w, out) : conv_f32<3, k>(S, d, w, out)
  if (nd != 2 && nd != 3) return -1;
  switch (ksize) { CONV_CASE(1); CONV_CASE(3); CONV_CASE(5); CONV_CASE(7); CONV_CASE(9); default: return -1; }
#undef CONV_CASE
}

#ifdef WIDEN_HOST_MAIN
int main()
{
  // floats of every kind: bit patterns from a linear congruential generator (all exponents, NaNs and infinities among them), then the named ones
  uint32_t state = 12345u;
  auto next_float = [&]() { state = state * 1664525u + 1013904223u; float f; memcpy(&f, &state, 4); return f; };
  const uint32_t named[] = {0u, 0x80000000u, 1u, 0x80000001u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u};
  const size_t counts[] = {0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025};
  for (size_t count : counts)
    for (int so = 0; so < 4; so ++)
      for (int dof = 0; dof < 2; dof ++) {
        std::vector<float> v(count);
        for (size_t i = 0; i < count; i ++) { if (i < sizeof(named) / 4) memcpy(&v[i], &named[i], 4); else v[i] = next_float(); }
        std::vector<double> out(count);
        const int rc = hc_widen(v.data(), count, so, dof, out.data());
        if (rc) { fprintf(stderr, "hc_widen(count %zu, src + %d, dst + %d): %d\n", count, so, dof, rc); return 1; }
      }
  const int shapes[][4] = {{2, 6, 5, 1}, {2, 1, 1, 1}, {2, 33, 33, 1}, {2, 65, 2, 1}, {3, 4, 3, 3}, {3, 1, 2, 1}, {3, 33, 9, 5}, {3, 31, 7, 9}};
  for (const auto &s : shapes)
    for (int k = 1; k <= 9; k += 2) {
      const size_t n = (size_t)s[1] * s[2] * s[3];
      std::vector<float> a(n);
      for (size_t i = 0; i < n; i ++) a[i] = (float)((double)(int32_t)(state = state * 1664525u + 1013904223u) / 2147483648.0);
      std::vector<double> w(729, 1.0 / 729), out(n);
      const long differ = hc_conv_f32(s[0], k, a.data(), s[1], s[2], s[3], w.data(), out.data());
      if (differ) { fprintf(stderr, "hc_conv_f32(nd %d, k %d, %d x %d x %d): %ld\n", s[0], k, s[1], s[2], s[3], differ); return 1; }
    }
  printf("widen_host run complete\n");
  return 0;
}
#endif
