// ftk_amd/csrc/conv_vec_steps.hpp on the CPU, for tests/test_conv_vec_host.py: conv_vec_kernels.hip's loops restated around the headers' own
// functions -- tiles in order, per tile the components one after the other through ONE tile of the kernel's size and pitch, the staging loop
// of 256 "lanes", conv_lane() for every lane's place, conv_outputs() from the lane's corner, the kernel's bounds on what is stored and its
// index into the interleaved output.  What the GPU adds is parallelism only.
//
//   hc_conv_vec(nd, ksize, f32, planar, src, DW, DH, DD, weights, out)        0, or -1 for sizes the kernel does not have
//       src: nd pointers -- planar: one plane each; interleaved: src[0] is the array (the others are ignored); f32: floats, else doubles
//       out: nd * DW * DH * DD doubles, interleaved
//   hc_conv_vec_lds_bytes(nd, ksize)                                          ConvVecTile::LDS_BYTES, or -1
//
// With -DCONV_VEC_HOST_MAIN: a program of its own (for a sanitizer build, not for loading into Python): conv_vec_host IN OUT [IN OUT ...]
//   IN : int64 nd, ksize, DW, DH, DD, f32, planar; double weights[ksize^nd]; the source's nd * DW * DH * DD elements (planes back to back)
//   OUT: double out[nd * DW * DH * DD]
// `out`, every plane and the tile are allocated at exactly their sizes, so a store or a read past any of them is seen.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ftk_amd/csrc/conv_vec_steps.hpp"

using namespace ftkx;

namespace {

template <int ND, int K, class SRC> void conv_vec_host(const ConvVecSource<SRC> &src, const ConvDims &d, const double *w, double *out)
{
  typedef ConvTile<ND, K> T;
  constexpr int NC = ConvVecTile<ND, K>::NC;
  static_assert(ConvVecTile<ND, K>::LDS_BYTES == T::DOUBLES * 8, "one plane");
  double *tile = static_cast<double *>(aligned_alloc(16, ((size_t)ConvVecTile<ND, K>::LDS_BYTES + 15) / 16 * 16));
  const size_t ntiles = conv_tiles<ND, K>(d);
  for (size_t t = 0; t < ntiles; t ++) {
    int x0, y0, z0;
    conv_tile_origin<ND, K>(d, t, &x0, &y0, &z0);
    for (int c = 0; c < NC; c ++) {
      const SRC *base = conv_vec_base(src, c);
      for (int tid = 0; tid < kConvThreads; tid ++)
        for (int i = tid; i < T::STAGED; i += kConvThreads) conv_vec_stage<ND, K>(base, src.stride, d, x0, y0, z0, i, tile);
      for (int tid = 0; tid < kConvThreads; tid ++) {
        int tx, ty, tz;
        conv_lane<ND, K>(tid, &tx, &ty, &tz);
        const int gx = x0 + tx * T::R, gy = y0 + ty;
        for (int oz = tz; oz < T::TZ; oz += T::LZ) {
          const int gz = z0 + oz;
          if (gx >= d.DW || gy >= d.DH || gz >= d.DD) continue;
          double res[T::R];
          conv_outputs<ND, K>(tile + (oz * T::PY + ty) * T::PX + tx * T::R, w, res);
          double *o = out + conv_vec_out_index(d, NC, c, gx, gy, gz);
          for (int r = 0; r < T::R; r ++) if (gx + r < d.DW) o[(size_t)r * NC] = res[r];
        }
      }
    }
  }
  free(tile);
}

template <class SRC> int run(int nd, int ksize, int planar, const void *const *src, const ConvDims &d, const double *w, double *out)
{
  const SRC *p[3] = {static_cast<const SRC *>(src[0]), planar ? static_cast<const SRC *>(src[1]) : nullptr, planar && nd == 3 ? static_cast<const SRC *>(src[2]) : nullptr};
  const ConvVecSource<SRC> s = planar ? conv_vec_planes<SRC>(p, nd) : conv_vec_interleaved<SRC>(p[0], nd);
#define CONV_CASE(k) case k: if (nd == 2) conv_vec_host<2, k, SRC>(s, d, w, out); else conv_vec_host<3, k, SRC>(s, d, w, out); return 0
  switch (ksize) { CONV_CASE(1); CONV_CASE(3); CONV_CASE(5); CONV_CASE(7); CONV_CASE(9); default: return -1; }
#undef CONV_CASE
}

}  // namespace

extern "C" int hc_conv_vec(int nd, int ksize, int f32, int planar, const void *const *src, int DW, int DH, int DD, const double *w, double *out)
{
  if (nd != 2 && nd != 3) return -1;
  const ConvDims d{DW, DH, nd == 2 ? 1 : DD};
  return f32 ? run<float>(nd, ksize, planar, src, d, w, out) : run<double>(nd, ksize, planar, src, d, w, out);
}

extern "C" int hc_conv_vec_lds_bytes(int nd, int ksize)
{
#define CONV_CASE(k) case k: return nd == 2 ? ConvVecTile<2, k>::LDS_BYTES : ConvVecTile<3, k>::LDS_BYTES
  if (nd != 2 && nd != 3) return -1;
  switch (ksize) { CONV_CASE(1); CONV_CASE(3); CONV_CASE(5); CONV_CASE(7); CONV_CASE(9); default: return -1; }
#undef CONV_CASE
}

#ifdef CONV_VEC_HOST_MAIN
int main(int argc, char **argv)
{
  for (int a = 1; a + 1 < argc; a += 2) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 1; }
    long long h[7];
    if (fread(h, 8, 7, f) != 7) return 1;
    const int nd = (int)h[0], f32 = (int)h[5], planar = (int)h[6];
    if (nd != 2 && nd != 3) return 1;
    const size_t n = (size_t)h[2] * (size_t)h[3] * (size_t)h[4], esize = f32 ? 4 : 8;
    size_t taps = 1;
    for (int d = 0; d < nd; d ++) taps *= (size_t)h[1];
    std::vector<double> w(taps);
    if (fread(w.data(), 8, taps, f) != taps) return 1;
    // exactly their sizes: the sanitizer sees a read behind a plane, or behind the interleaved array
    void *src[3] = {nullptr, nullptr, nullptr};
    const int arrays = planar ? nd : 1;
    const size_t each = (planar ? n : n * (size_t)nd) * esize;
    for (int k = 0; k < arrays; k ++) {
      src[k] = malloc(each);
      if (!src[k] || fread(src[k], 1, each, f) != each) return 1;
    }
    fclose(f);
    double *out = static_cast<double *>(malloc(n * (size_t)nd * sizeof(double)));      // exactly nd * n: a store behind it is seen
    const int rc = hc_conv_vec(nd, (int)h[1], f32, planar, src, (int)h[2], (int)h[3], (int)h[4], w.data(), out);
    if (rc) { fprintf(stderr, "hc_conv_vec: %d\n", rc); return 1; }
    f = fopen(argv[a + 1], "wb");
    if (!f || fwrite(out, 8, n * (size_t)nd, f) != n * (size_t)nd) return 1;
    fclose(f);
    free(out);
    for (int k = 0; k < arrays; k ++) free(src[k]);
  }
  printf("conv_vec_host run complete\n");
  return 0;
}
#endif
