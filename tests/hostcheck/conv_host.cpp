// ftk_amd/csrc/conv_steps.hpp on the CPU, for tests/test_conv_steps_host.py: conv_kernels.hip's loops restated around the header's own
// functions -- tiles in order, the staging loop of 256 "lanes" into a tile of the kernel's size and pitch, conv_lane() for every lane's
// place, conv_outputs() from the lane's corner of the tile, the kernel's bounds on what is stored.  What the GPU adds is parallelism only.
//
//   hc_conv(nd, ksize, S, DW, DH, DD, weights, out)        0, or -1 for sizes the kernel does not have
//
// With -DCONV_HOST_MAIN: a program of its own (for a sanitizer build, not for loading into Python): conv_host IN OUT [IN OUT ...]
//   IN : int64 nd, ksize, DW, DH, DD; double weights[ksize^nd]; double data[DW * DH * DD]        OUT: double out[DW * DH * DD]
// `out` is allocated at exactly its size and the tile at exactly ConvTile::DOUBLES, so a store or a read past either is seen.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../ftk_amd/csrc/conv_steps.hpp"

using namespace ftkx;

namespace {

template <int ND, int K> void conv_host(const double *S, const ConvDims &d, const double *w, double *out)
{
  typedef ConvTile<ND, K> T;
  // (over-aligned like the kernel's: conv_outputs() tells the compiler that every row read starts at a multiple of 16 bytes)
  double *tile = static_cast<double *>(aligned_alloc(16, (sizeof(double) * T::DOUBLES + 15) / 16 * 16));
  const size_t ntiles = conv_tiles<ND, K>(d);
  for (size_t t = 0; t < ntiles; t ++) {
    int x0, y0, z0;
    conv_tile_origin<ND, K>(d, t, &x0, &y0, &z0);
    for (int tid = 0; tid < kConvThreads; tid ++)
      for (int i = tid; i < T::STAGED; i += kConvThreads) conv_stage<ND, K>(S, d, x0, y0, z0, i, tile);
    for (int tid = 0; tid < kConvThreads; tid ++) {
      int tx, ty, tz;
      conv_lane<ND, K>(tid, &tx, &ty, &tz);
      const int gx = x0 + tx * T::R, gy = y0 + ty;
      for (int oz = tz; oz < T::TZ; oz += T::LZ) {
        const int gz = z0 + oz;
        if (gx >= d.DW || gy >= d.DH || gz >= d.DD) continue;
        double res[T::R];
        conv_outputs<ND, K>(tile + (oz * T::PY + ty) * T::PX + tx * T::R, w, res);
        double *o = out + ((size_t)gz * (size_t)d.DH + (size_t)gy) * (size_t)d.DW + (size_t)gx;
        for (int r = 0; r < T::R; r ++) if (gx + r < d.DW) o[r] = res[r];
      }
    }
  }
  free(tile);
}

// every lane has a place of its own, and the places fill the workgroup's box
template <int ND, int K> bool lanes_ok()
{
  typedef ConvTile<ND, K> T;
  std::vector<int> seen(kConvThreads, 0);
  for (int tid = 0; tid < kConvThreads; tid ++) {
    int tx, ty, tz;
    conv_lane<ND, K>(tid, &tx, &ty, &tz);
    if (tx < 0 || tx >= T::LX || ty < 0 || ty >= T::LY || tz < 0 || tz >= T::LZ) return false;
    seen[(tz * T::LY + ty) * T::LX + tx] ++;
  }
  for (int v : seen) if (v != 1) return false;
  return true;
}

}  // namespace

extern "C" int hc_conv(int nd, int ksize, const double *S, int DW, int DH, int DD, const double *w, double *out)
{
  const ConvDims d{DW, DH, nd == 2 ? 1 : DD};
#define CONV_CASE(k) case k: if (!(nd == 2 ? lanes_ok<2, k>() : lanes_ok<3, k>())) return -2; \
                             if (nd == 2) conv_host<2, k>(S, d, w, out); else conv_host<3, k>(S, d, w, out); return 0
  if (nd != 2 && nd != 3) return -1;
  switch (ksize) { CONV_CASE(1); CONV_CASE(3); CONV_CASE(5); CONV_CASE(7); CONV_CASE(9); default: return -1; }
#undef CONV_CASE
}

#ifdef CONV_HOST_MAIN
int main(int argc, char **argv)
{
  for (int a = 1; a + 1 < argc; a += 2) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 1; }
    long long h[5];
    if (fread(h, 8, 5, f) != 5) return 1;
    const size_t n = (size_t)h[2] * (size_t)h[3] * (size_t)h[4];
    size_t taps = 1;
    for (int d = 0; d < (int)h[0]; d ++) taps *= (size_t)h[1];
    std::vector<double> w(taps), S(n);
    if (fread(w.data(), 8, taps, f) != taps || fread(S.data(), 8, n, f) != n) return 1;
    fclose(f);
    double *out = static_cast<double *>(malloc(n * sizeof(double)));      // exactly n: the sanitizer sees a store behind it
    const int rc = hc_conv((int)h[0], (int)h[1], S.data(), (int)h[2], (int)h[3], (int)h[4], w.data(), out);
    if (rc) { fprintf(stderr, "hc_conv: %d\n", rc); return 1; }
    f = fopen(argv[a + 1], "wb");
    if (!f || fwrite(out, 8, n, f) != n) return 1;
    fclose(f);
    free(out);
  }
  printf("conv_host run complete\n");
  return 0;
}
#endif
