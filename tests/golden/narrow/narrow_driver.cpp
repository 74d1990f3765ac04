// Writes what the reference makes of an array that is not stored as doubles: ndarray<double>::from_array(ndarray<T1>)
// (include/ftk/ndarray.hh:401-410), and nothing else.  Built and run by make_golden_narrow.py against the reference's headers, outside this
// repository; only what it writes is kept (tests/golden/narrow/*.npz).
//
//   narrow_driver IN OUT
//   IN : int64 kind, nd, n[nd] (x first); prod n elements of type `kind` (x fastest)
//        kind: 1 float, 4 unsigned char, 5 signed char, 6 unsigned short, 7 short, 8 unsigned int, 9 int (the library's FTKX_DTYPE_* codes)
//   OUT: int64 nd_out, shape[nd_out] (first index fastest); double out[prod shape]
#include <ftk/ndarray.hh>
#include <cstdio>
#include <cstdlib>
#include <vector>

static void must(bool ok, const char *what) { if (!ok) { fprintf(stderr, "narrow_driver: %s\n", what); exit(1); } }

template <class T1> static void widened(FILE *f, const std::vector<size_t> &shape, ftk::ndarray<double> &out)
{
  ftk::ndarray<T1> a(shape);
  must(fread(a.data(), sizeof(T1), a.nelem(), f) == a.nelem(), "short data");
  out.from_array(a);
}

int main(int argc, char **argv)
{
  must(argc == 3, "usage: narrow_driver IN OUT");
  FILE *f = fopen(argv[1], "rb");
  must(f, "cannot open IN");
  long long kind = 0, nd = 0, n[3] = {1, 1, 1};
  must(fread(&kind, 8, 1, f) == 1 && fread(&nd, 8, 1, f) == 1 && nd >= 1 && nd <= 3, "bad header");
  must(fread(n, 8, (size_t)nd, f) == (size_t)nd, "bad header");
  const std::vector<size_t> shape(n, n + nd);
  ftk::ndarray<double> out;
  switch (kind) {
  case 1: widened<float>(f, shape, out); break;
  case 4: widened<unsigned char>(f, shape, out); break;
  case 5: widened<signed char>(f, shape, out); break;
  case 6: widened<unsigned short>(f, shape, out); break;
  case 7: widened<short>(f, shape, out); break;
  case 8: widened<unsigned int>(f, shape, out); break;
  case 9: widened<int>(f, shape, out); break;
  default: must(false, "unknown kind");
  }
  fclose(f);
  f = fopen(argv[2], "wb");
  must(f, "cannot open OUT");
  const long long nd_out = (long long)out.nd();
  fwrite(&nd_out, 8, 1, f);
  for (long long d = 0; d < nd_out; d ++) { long long m = (long long)out.dim(d); fwrite(&m, 8, 1, f); }
  fwrite(out.data(), 8, out.nelem(), f);
  fclose(f);
  return 0;
}
