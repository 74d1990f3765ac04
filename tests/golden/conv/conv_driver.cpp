// Writes what the reference's spatial smoothing makes of an array: its Gaussian weights and conv_gaussian(array, sigma, ksize, ksize / 2),
// the call of ndarray_stream::modified_callback (include/ftk/ndarray/stream.hh:1597-1603).  Built and run by make_golden_conv.py against the
// reference's headers, outside this repository; only what it writes is kept (tests/golden/conv/*.npz).
//
//   conv_driver IN OUT
//   IN : int64 nd, ksize, n[nd] (x first); double sigma; double data[prod n]      (x fastest)
//   OUT: int64 nout[nd]; double weights[ksize^nd]; double out[prod nout]
#include <ftk/ndarray.hh>
#include <ftk/ndarray/conv.hh>
#include <cstdio>
#include <cstdlib>
#include <vector>

static void must(bool ok, const char *what) { if (!ok) { fprintf(stderr, "conv_driver: %s\n", what); exit(1); } }

int main(int argc, char **argv)
{
  must(argc == 3, "usage: conv_driver IN OUT");
  FILE *f = fopen(argv[1], "rb");
  must(f, "cannot open IN");
  long long nd = 0, ksize = 0, n[3] = {1, 1, 1};
  double sigma = 0;
  must(fread(&nd, 8, 1, f) == 1 && fread(&ksize, 8, 1, f) == 1 && (nd == 2 || nd == 3), "bad header");
  must(fread(n, 8, (size_t)nd, f) == (size_t)nd && fread(&sigma, 8, 1, f) == 1, "bad header");
  std::vector<size_t> shape(n, n + nd);
  ftk::ndarray<double> data(shape);
  must(fread(data.data(), 8, data.nelem(), f) == data.nelem(), "short data");
  fclose(f);
  const ftk::ndarray<double> w = nd == 2 ? ftk::gaussian_kernel2D<double>(sigma, ksize, ksize) : ftk::gaussian_kernel3D<double>(sigma, ksize, ksize, ksize);
  const ftk::ndarray<double> out = ftk::conv_gaussian<double>(data, sigma, (size_t)ksize, (size_t)(ksize / 2));
  f = fopen(argv[2], "wb");
  must(f, "cannot open OUT");
  for (int d = 0; d < nd; d ++) { long long m = (long long)out.dim(d); fwrite(&m, 8, 1, f); }
  fwrite(w.data(), 8, w.nelem(), f);
  fwrite(out.data(), 8, out.nelem(), f);
  fclose(f);
  return 0;
}
