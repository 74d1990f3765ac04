// Writes what the reference's stream makes of a vector field kept as one variable per component: ndarray<T>::concat of the nc arrays
// (include/ftk/ndarray/stream.hh:1347-1354, 1371-1378, 1423-1433), and -- where they are floats -- ndarray<double>::from_array of that, the
// widening of a "float32" source.  Built and run by make_golden_concat.py against the reference's headers, outside this repository; only
// what it writes is kept (tests/golden/concat/*.npz).
//
//   concat_driver IN OUT
//   IN : int64 is_f32, nc, nd, n[nd] (x first); nc planes of prod n elements each (float where is_f32, else double; x fastest)
//   OUT: int64 nd_out, shape[nd_out] (first index fastest); double out[prod shape]
#include <ftk/ndarray.hh>
#include <cstdio>
#include <cstdlib>
#include <vector>

static void must(bool ok, const char *what) { if (!ok) { fprintf(stderr, "concat_driver: %s\n", what); exit(1); } }

template <class T> static ftk::ndarray<T> joined(FILE *f, long long nc, const std::vector<size_t> &shape)
{
  std::vector<ftk::ndarray<T>> planes;
  for (long long k = 0; k < nc; k ++) {
    ftk::ndarray<T> a(shape);
    must(fread(a.data(), sizeof(T), a.nelem(), f) == a.nelem(), "short data");
    planes.push_back(a);
  }
  return ftk::ndarray<T>::concat(planes);
}

int main(int argc, char **argv)
{
  must(argc == 3, "usage: concat_driver IN OUT");
  FILE *f = fopen(argv[1], "rb");
  must(f, "cannot open IN");
  long long is_f32 = 0, nc = 0, nd = 0, n[3] = {1, 1, 1};
  must(fread(&is_f32, 8, 1, f) == 1 && fread(&nc, 8, 1, f) == 1 && fread(&nd, 8, 1, f) == 1 && nc >= 1 && nd >= 1 && nd <= 3, "bad header");
  must(fread(n, 8, (size_t)nd, f) == (size_t)nd, "bad header");
  const std::vector<size_t> shape(n, n + nd);
  ftk::ndarray<double> out;
  if (is_f32) out.from_array(joined<float>(f, nc, shape));
  else out = joined<double>(f, nc, shape);
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
