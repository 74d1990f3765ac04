// ftk_amd/csrc/sample_steps.hpp on the CPU, for tests/test_sample_steps_host.py, as the oracle of tests/test_gpu_aux.py and as the host
// figure of tools/sample_time.py.
//
//   hs_sample(nd, mesh[20], tags, aux, n, t_min, ntab, S, V, A1, A2, slots, nthreads, out1, out2, ok)
//       mesh: the 20 ints of ftkx::SampleMesh in its order (tag_mode, scalar_mode, dom_lb[3], dom_sz[3], core_st[3], core_sz[3], ext_st[3],
//       ext_sz[3]); S, V, A1, A2: ntab pointers each, entry k the arrays of timestep t_min + k (null where there is none); slots: bit 0 fill
//       out1 from A1, bit 1 out2 from A2; the records are dealt to nthreads threads in contiguous ranges.  ok[i] (nullable): record i decoded
//       to a simplex inside the arrays and every array it reads is there.  Returns the number of records that did not (their outputs are 0).
//   hs_element(nd, mesh[20], tag, aux, corner[4], type)   step 1 alone: 1 decoded, 0 not
//   hs_reference_ok(nd, dom_sz[3], t_max)                 the bound under which FTKX_TAG_REFERENCE tags equal the 64-bit ones
//
// With -DSAMPLE_HOST_MAIN: a program of its own (for a sanitizer build, not for loading into Python): every simplex type at every corner of a
// small 2D and 3D mesh under the three tag modes, the arrays allocated at exactly their size -- once with the array lattice at 0 and core =
// domain, once with the array lattice at (5, 7, 3) and a core one vertex inside the domain on every face.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "../../ftk_amd/csrc/sample_steps.hpp"

using namespace ftkx;

namespace {

SampleMesh mesh_of(const int *p)
{
  SampleMesh m;
  static_assert(sizeof(SampleMesh) == 20 * sizeof(int), "SampleMesh is twenty ints");
  memcpy(&m, p, sizeof(m));
  return m;
}

// which slices a decoded record reads: all there?
template <int ND>
bool arrays_present(const SampleMesh &m, const fan_table<ND + 1> &fan, int type, int at, int ntab, const std::vector<SampleSlice> &tab, unsigned slots)
{
  const int last = fan.ordinal[type] ? at : at + 1;
  if (at < 0 || last >= ntab) return false;
  for (int k = at; k <= last; k ++) {
    if (m.scalar_mode ? !tab[(size_t)k].S : !tab[(size_t)k].V) return false;
    for (int s = 0; s < 2; s ++) if (((slots >> s) & 1u) && !tab[(size_t)k].A[s]) return false;
  }
  return true;
}

template <int ND>
size_t run(const SampleMesh &m, const fan_table<ND + 1> &fan, const u64 *tags, const unsigned *aux, size_t b, size_t e, int t_min, int ntab,
           const std::vector<SampleSlice> &tab, unsigned slots, double *out1, double *out2, unsigned char *ok)
{
  size_t bad = 0;
  for (size_t i = b; i < e; i ++) {
    const SampleIn in{tags[i], aux[i], 0u};
    int corner[ND + 1], type = 0;
    double r[2] = {0.0, 0.0};
    bool good = sample_element<ND>(m, fan, in.tag, in.aux, corner, type);
    good = good && arrays_present<ND>(m, fan, type, corner[ND] - t_min, ntab, tab, slots);
    if (good) sample_record<ND>(m, fan, in, tab.data(), t_min, slots, r);
    else bad ++;
    if (out1 && (slots & 1u)) out1[i] = r[0];
    if (out2 && (slots & 2u)) out2[i] = r[1];
    if (ok) ok[i] = good ? 1 : 0;
  }
  return bad;
}

}  // namespace

extern "C" size_t hs_sample(int nd, const int *mesh, const unsigned long long *tags, const unsigned *aux, size_t n, int t_min, int ntab, const double *const *S,
                            const double *const *V, const double *const *A1, const double *const *A2, unsigned slots, int nthreads, double *out1, double *out2,
                            unsigned char *ok)
{
  const SampleMesh m = mesh_of(mesh);
  std::vector<SampleSlice> tab((size_t)(ntab > 0 ? ntab : 0));
  for (int k = 0; k < ntab; k ++) tab[(size_t)k] = SampleSlice{S ? S[k] : nullptr, V ? V[k] : nullptr, {A1 ? A1[k] : nullptr, A2 ? A2[k] : nullptr}};
  if (nthreads < 1) nthreads = 1;
  std::vector<size_t> bad((size_t)nthreads, 0);
  auto part = [&](int k) {
    const size_t b = n * (size_t)k / (size_t)nthreads, e = n * (size_t)(k + 1) / (size_t)nthreads;
    bad[(size_t)k] = nd == 2 ? run<2>(m, k_fan3, tags, aux, b, e, t_min, ntab, tab, slots, out1, out2, ok) : run<3>(m, k_fan4, tags, aux, b, e, t_min, ntab, tab, slots, out1, out2, ok);
  };
  if (nthreads == 1) part(0);
  else {
    std::vector<std::thread> th;
    for (int k = 0; k < nthreads; k ++) th.emplace_back(part, k);
    for (std::thread &t : th) t.join();
  }
  size_t total = 0;
  for (size_t v : bad) total += v;
  return total;
}

extern "C" int hs_element(int nd, const int *mesh, unsigned long long tag, unsigned aux, int *corner, int *type)
{
  const SampleMesh m = mesh_of(mesh);
  return (nd == 2 ? sample_element<2>(m, k_fan3, tag, aux, corner, *type) : sample_element<3>(m, k_fan4, tag, aux, corner, *type)) ? 1 : 0;
}

extern "C" int hs_reference_ok(int nd, const long long *dom_sz, int t_max) { return sample_reference_tags_exact(nd, dom_sz, t_max) ? 1 : 0; }

#ifdef SAMPLE_HOST_MAIN
// the tag of (corner, type) at timestep t, as sweep_device.hpp forms it (element_tag, core_linear)
template <int ND>
u64 tag_of(const SampleMesh &m, const fan_table<ND + 1> &fan, const int *corner, int t, int type)
{
  constexpr int N = ND + 1;
  if (m.tag_mode == FTKX_TAG_WORK_INDEX) {
    u64 lin = 0, stride = 1;
    for (int d = 0; d < ND; d ++) { lin += (u64)(corner[d] - m.core_st[d]) * stride; stride *= (u64)m.core_sz[d]; }
    return lin * (u64)(fan.ordinal[type] ? fan_table<N>::NORD : fan_table<N>::NINT) + fan.local_index[type];
  }
  u64 ci = 0, prod = 1;
  for (int d = 0; d < ND; d ++) { ci += (u64)(corner[d] - m.dom_lb[d]) * prod; prod *= (u64)m.dom_sz[d]; }
  ci += (u64)t * prod;
  return ci * (u64)fan_table<N>::NTYPES + (u64)type;
}

template <int ND>
int sweep_all(const fan_table<ND + 1> &fan, int scalar_mode, bool origin)
{
  constexpr int N = ND + 1;
  SampleMesh m;
  memset(&m, 0, sizeof(m));
  m.scalar_mode = scalar_mode;
  const int ext[3] = {origin ? 10 : 9, origin ? 9 : 7, ND == 3 ? (origin ? 8 : 6) : 1}, lo = scalar_mode ? 2 : 1, start[3] = {5, 7, 3}, in = origin ? 1 : 0;
  size_t nv = 1;
  for (int d = 0; d < 3; d ++) {
    m.ext_st[d] = origin && d < ND ? start[d] : 0; m.ext_sz[d] = ext[d];
    m.dom_lb[d] = d < ND ? m.ext_st[d] + lo : 0; m.dom_sz[d] = d < ND ? ext[d] - 2 * lo : 1;
    m.core_st[d] = d < ND ? m.dom_lb[d] + in : 0; m.core_sz[d] = d < ND ? m.dom_sz[d] - 2 * in : 1;
    nv *= (size_t)ext[d];
  }
  const int nt = 3, t0 = 5;
  // exactly sized arrays: a read past one is the sanitizer's
  std::vector<std::vector<double>> S(nt), V(nt), A(nt);
  uint64_t state = 99u;
  auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(int64_t)state / 9223372036854775808.0; };
  std::vector<SampleSlice> tab(nt);
  for (int k = 0; k < nt; k ++) {
    S[k].resize(nv); V[k].resize(nv * ND); A[k].resize(nv);
    for (double &x : S[k]) x = next();
    for (double &x : V[k]) x = next();
    for (double &x : A[k]) x = next();
    tab[k] = SampleSlice{S[k].data(), scalar_mode ? nullptr : V[k].data(), {A[k].data(), S[k].data()}};
  }
  for (int mode = 0; mode < 3; mode ++) {
    m.tag_mode = mode;
    for (int t = t0; t < t0 + nt; t ++)
      for (int type = 0; type < fan_table<N>::NTYPES; type ++) {
        if (!fan.ordinal[type] && t == t0 + nt - 1) continue;
        int c[4] = {0, 0, 0, t};
        // the core's corners whose cell lies inside the array: up to the domain's last vertex but one
        auto end = [&](int d) { const int a = m.core_st[d] + m.core_sz[d], b = m.dom_lb[d] + m.dom_sz[d] - 1; return a < b ? a : b; };
        for (c[2] = m.core_st[2]; c[2] < (ND == 3 ? end(2) : 1); c[2] ++)
          for (c[1] = m.core_st[1]; c[1] < end(1); c[1] ++)
            for (c[0] = m.core_st[0]; c[0] < end(0); c[0] ++) {
              int corner[N];
              for (int d = 0; d < ND; d ++) corner[d] = c[d];
              corner[ND] = t;
              const SampleIn in{tag_of<ND>(m, fan, corner, t, type), ((unsigned)t << 1) | (fan.ordinal[type] ? 1u : 0u), 0u};
              int got[N], gtype = -1;
              if (!sample_element<ND>(m, fan, in.tag, in.aux, got, gtype) || gtype != type || memcmp(got, corner, sizeof(corner)) != 0) {
                fprintf(stderr, "decode: nd %d origin %d mode %d t %d type %d corner %d %d %d\n", ND, (int)origin, mode, t, type, c[0], c[1], c[2]);
                return 1;
              }
              double r[2];
              if (!sample_record<ND>(m, fan, in, tab.data(), t0, 3u, r)) return 1;
            }
      }
  }
  return 0;
}

int main()
{
  for (int origin = 0; origin < 2; origin ++)
    if (sweep_all<2>(k_fan3, 1, origin != 0) || sweep_all<2>(k_fan3, 0, origin != 0) || sweep_all<3>(k_fan4, 1, origin != 0) || sweep_all<3>(k_fan4, 0, origin != 0)) return 1;
  printf("sample_host run complete\n");
  return 0;
}
#endif
