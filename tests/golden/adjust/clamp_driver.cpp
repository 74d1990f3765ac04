// Writes what the reference's ndarray<double>::clamp(lo, hi) (include/ftk/ndarray.hh:1344-1350, numeric/clamp.hh:15-20) makes of an array,
// the call of ndarray_stream::modified_callback (include/ftk/ndarray/stream.hh:1570-1604).  Built and run by make_golden_adjust.py against
// the reference's headers, outside this repository; only what it writes is kept (tests/golden/adjust/clamp.npz).
//
//   clamp_driver IN OUT
//   IN : int64 n; double lo, hi; double data[n]
//   OUT: double out[n]
#include <ftk/ndarray.hh>
#include <cstdio>
#include <cstdlib>
#include <vector>

static void must(bool ok, const char *what) { if (!ok) { fprintf(stderr, "clamp_driver: %s\n", what); exit(1); } }

int main(int argc, char **argv)
{
  must(argc == 3, "usage: clamp_driver IN OUT");
  FILE *f = fopen(argv[1], "rb");
  must(f, "cannot open IN");
  long long n = 0;
  double lo = 0, hi = 0;
  must(fread(&n, 8, 1, f) == 1 && n >= 1 && fread(&lo, 8, 1, f) == 1 && fread(&hi, 8, 1, f) == 1, "bad header");
  ftk::ndarray<double> data(std::vector<size_t>{(size_t)n});
  must(fread(data.data(), 8, data.nelem(), f) == data.nelem(), "short data");
  fclose(f);
  data.clamp(lo, hi);
  f = fopen(argv[2], "wb");
  must(f, "cannot open OUT");
  fwrite(data.data(), 8, data.nelem(), f);
  fclose(f);
  return 0;
}
