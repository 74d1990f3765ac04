// Writes what the reference's temporal smoothing makes of a series of arrays: its Gaussian weights and every array that
// ftk::streaming_filter<ndarray<double>, double> hands to its callback, in order -- push() per input array, then finish() -- the filter
// ndarray_stream::modified_callback runs with --temporal-smoothing-kernel[-size] (include/ftk/ndarray/stream.hh,
// include/ftk/filters/streaming_filter.hh).  Built and run by make_golden_temporal.py against the reference's headers, outside this
// repository; only what it writes is kept (tests/golden/temporal/*.npz).
//
//   temporal_driver IN OUT
//   IN : int64 ksize, N, nd, n[nd] (fastest first); double sigma; double data[N][prod n]
//   OUT: int64 n_emitted; double weights[ksize]; double out[n_emitted][prod n]
// The callback's index argument is not written (it depends on the compiler's order of evaluation).  N == 0: finish() is not called
// (it pops an empty deque).
#include <ftk/ndarray.hh>
#include <ftk/filters/streaming_filter.hh>
#include <cstdio>
#include <cstdlib>
#include <vector>

static void must(bool ok, const char *what) { if (!ok) { fprintf(stderr, "temporal_driver: %s\n", what); exit(1); } }

int main(int argc, char **argv)
{
  must(argc == 3, "usage: temporal_driver IN OUT");
  FILE *f = fopen(argv[1], "rb");
  must(f, "cannot open IN");
  long long ksize = 0, N = 0, nd = 0, n[4] = {1, 1, 1, 1};
  double sigma = 0;
  must(fread(&ksize, 8, 1, f) == 1 && fread(&N, 8, 1, f) == 1 && fread(&nd, 8, 1, f) == 1 && nd >= 1 && nd <= 4, "bad header");
  must(fread(n, 8, (size_t)nd, f) == (size_t)nd && fread(&sigma, 8, 1, f) == 1, "bad header");
  const std::vector<size_t> shape(n, n + nd);
  std::vector<ftk::ndarray<double>> emitted;
  ftk::streaming_filter<ftk::ndarray<double>, double> filter;
  filter.set_gaussian_kernel(sigma, (int)ksize);
  filter.set_callback([&](int, const ftk::ndarray<double> &a) { emitted.push_back(a); });
  for (long long k = 0; k < N; k ++) {
    ftk::ndarray<double> a(shape);
    must(fread(a.data(), 8, a.nelem(), f) == a.nelem(), "short data");
    filter.push(a);
  }
  fclose(f);
  if (N > 0) filter.finish();
  f = fopen(argv[2], "wb");
  must(f, "cannot open OUT");
  const long long ne = (long long)emitted.size();
  fwrite(&ne, 8, 1, f);
  fwrite(filter.get_kernel().data(), 8, filter.get_kernel().size(), f);
  for (const ftk::ndarray<double> &a : emitted) fwrite(a.data(), 8, a.nelem(), f);
  fclose(f);
  return 0;
}
