// The loop body of series_sample_kernel (ftk_amd/csrc/sample_steps.hpp, series_sample_lane) on the CPU, for tests/test_series_sample_host.py:
// the kernel's grid walked lane by lane -- `workgroups` x 256 lanes, lane l of workgroup w starting at record w * 256 + l with the grid's
// stride -- over records in host memory, and the slot rule of an armed pass.
//
//   hss_run(nd, mesh[20], recs, counter, capacity, t_min, ntab, S, V, A1, A2, slots, workgroups, stores)
//       recs: at least `capacity` ftkx_cp_t, worked on in place; counter: what the kernel reads from counters[CNT_PASS] (clamped to capacity as
//       the kernel clamps it); mesh, S, V, A1, A2: as hs_sample of sample_host.cpp; stores (nullable): 2 * capacity counters, [2 * i + s] the
//       stores into scalar[s + 1] of record i.  Returns the number of records the kernel works on.
//   hss_slots(ts, scopes, n, aux_ts, aux_bits, naux, slice_ts, k, slots)
//       the slices the steps read (slice_ts: room for 2 * n, *k of them) and the slot rule over them, with aux arrays resident as listed
//       (aux_bits[i]: bit s = slot s + 1 has an array at timestep aux_ts[i]).  Returns 0, or the slot that is there at some slices only.
//
// With -DSERIES_SAMPLE_HOST_MAIN: a program of its own for a sanitizer build -- every simplex of a small 2D and 3D mesh as a record, the record
// array and the field arrays allocated at exactly their size, grids of 1, 3 and 7 workgroups, a counter of 0 and one beyond the capacity.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct CountingStore {
  ftkx_cp_t *recs;
  unsigned *stores;
  void operator()(double *at, double v) const
  {
    *at = v;
    if (!stores) return;
    const size_t byte = (size_t)((const char *)at - (const char *)recs), i = byte / sizeof(ftkx_cp_t);
    const size_t s = (byte - i * sizeof(ftkx_cp_t) - offsetof(ftkx_cp_t, scalar)) / sizeof(double) - 1;
    stores[2 * i + s] ++;
  }
};

template <int ND>
size_t walk(const SampleMesh &m, const fan_table<ND + 1> &fan, ftkx_cp_t *recs, unsigned long long counter, unsigned long long capacity, const SampleSlice *tab, int t_min,
            int ntab, unsigned slots, int workgroups, unsigned *stores)
{
  const size_t n = (size_t)(counter > capacity ? capacity : counter);      // (the kernel: n = min(counters[CNT_PASS], capacity))
  const size_t stride = (size_t)workgroups * (size_t)kSampleThreads;
  for (int w = 0; w < workgroups; w ++)
    for (int l = 0; l < kSampleThreads; l ++)
      series_sample_lane<ND>(m, fan, recs, n, tab, t_min, ntab, slots, (size_t)w * (size_t)kSampleThreads + (size_t)l, stride, CountingStore{recs, stores});
  return n;
}

}  // namespace

extern "C" size_t hss_run(int nd, const int *mesh, ftkx_cp_t *recs, unsigned long long counter, unsigned long long capacity, int t_min, int ntab, const double *const *S,
                          const double *const *V, const double *const *A1, const double *const *A2, unsigned slots, int workgroups, unsigned *stores)
{
  const SampleMesh m = mesh_of(mesh);
  std::vector<SampleSlice> tab((size_t)(ntab > 0 ? ntab : 0));
  for (int k = 0; k < ntab; k ++) tab[(size_t)k] = SampleSlice{S ? S[k] : nullptr, V ? V[k] : nullptr, {A1 ? A1[k] : nullptr, A2 ? A2[k] : nullptr}};
  return nd == 2 ? walk<2>(m, k_fan3, recs, counter, capacity, tab.data(), t_min, ntab, slots, workgroups, stores)
                 : walk<3>(m, k_fan4, recs, counter, capacity, tab.data(), t_min, ntab, slots, workgroups, stores);
}

extern "C" int hss_slots(const int *ts, const int *scopes, int n, const int *aux_ts, const unsigned char *aux_bits, int naux, int *slice_ts, int *k, unsigned *slots)
{
  std::vector<int> st;
  series_slice_timesteps(ts, scopes, n, st);
  std::vector<unsigned char> have(st.size(), 0);
  for (size_t j = 0; j < st.size(); j ++) {
    slice_ts[j] = st[j];
    for (int i = 0; i < naux; i ++) if (aux_ts[i] == st[j]) have[j] |= aux_bits[i];
  }
  *k = (int)st.size();
  return series_sample_slots(have.data(), have.size(), slots);
}

#ifdef SERIES_SAMPLE_HOST_MAIN
template <int ND>
u64 tag_of(const SampleMesh &m, const int *corner, int t, int type)
{
  u64 ci = 0, prod = 1;
  for (int d = 0; d < ND; d ++) { ci += (u64)(corner[d] - m.dom_lb[d]) * prod; prod *= (u64)m.dom_sz[d]; }
  ci += (u64)t * prod;
  return ci * (u64)fan_table<ND + 1>::NTYPES + (u64)type;
}

template <int ND>
int sweep_all(const fan_table<ND + 1> &fan, int scalar_mode)
{
  constexpr int N = ND + 1;
  SampleMesh m;
  memset(&m, 0, sizeof(m));
  m.scalar_mode = scalar_mode;
  m.tag_mode = FTKX_TAG_EXACT64;
  const int ext[3] = {9, 7, ND == 3 ? 6 : 1}, lo = scalar_mode ? 2 : 1;
  size_t nv = 1;
  for (int d = 0; d < 3; d ++) {
    m.ext_st[d] = 0; m.ext_sz[d] = ext[d];
    m.dom_lb[d] = d < ND ? lo : 0; m.dom_sz[d] = d < ND ? ext[d] - 2 * lo : 1;
    m.core_st[d] = m.dom_lb[d]; m.core_sz[d] = m.dom_sz[d];
    nv *= (size_t)ext[d];
  }
  const int nt = 3, t0 = 5;
  std::vector<std::vector<double>> S(nt), V(nt), A(nt);      // exactly sized arrays: a read past one is the sanitizer's
  uint64_t state = 4242u;
  auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(int64_t)state / 9223372036854775808.0; };
  std::vector<SampleSlice> tab(nt);
  for (int k = 0; k < nt; k ++) {
    S[k].resize(nv); V[k].resize(nv * ND); A[k].resize(nv);
    for (double &x : S[k]) x = next();
    for (double &x : V[k]) x = next();
    for (double &x : A[k]) x = next();
    tab[k] = SampleSlice{S[k].data(), scalar_mode ? nullptr : V[k].data(), {A[k].data(), S[k].data()}};
  }
  std::vector<ftkx_cp_t> made;
  for (int t = t0; t < t0 + nt; t ++)
    for (int type = 0; type < fan_table<N>::NTYPES; type ++) {
      if (!fan.ordinal[type] && t == t0 + nt - 1) continue;
      int c[3] = {0, 0, 0};
      for (c[2] = m.dom_lb[2]; c[2] < m.dom_lb[2] + (ND == 3 ? m.dom_sz[2] - 1 : 1); c[2] ++)
        for (c[1] = m.dom_lb[1]; c[1] < m.dom_lb[1] + m.dom_sz[1] - 1; c[1] ++)
          for (c[0] = m.dom_lb[0]; c[0] < m.dom_lb[0] + m.dom_sz[0] - 1; c[0] ++) {
            ftkx_cp_t r;
            memset(&r, 0x5a, sizeof(r));
            r.tag = tag_of<ND>(m, c, t, type);
            reinterpret_cast<unsigned *>(&r)[15] = ((unsigned)t << 1) | (fan.ordinal[type] ? 1u : 0u);
            made.push_back(r);
          }
    }
  const size_t n = made.size();
  // a record in the middle that is no element of the mesh, and one whose timestep lies outside the table: both are left as they are
  made[n / 2].tag = 1ull << 62;
  reinterpret_cast<unsigned *>(&made[n / 3])[15] = ((unsigned)(t0 + nt + 7) << 1) | 1u;
  for (int wgs : {1, 3, 7})
    for (int variant = 0; variant < 3; variant ++) {
      // variant 0: the counter is the number of records; 1: zero; 2: beyond the capacity, which is n - 5 (exactly the array's size)
      const size_t capacity = variant == 2 ? n - 5 : n;
      const unsigned long long counter = variant == 1 ? 0 : variant == 2 ? n + 1000 : n;
      std::vector<ftkx_cp_t> recs(made.begin(), made.begin() + (long)capacity);
      std::vector<unsigned> stores(2 * capacity, 0);
      const size_t worked = walk<ND>(m, fan, recs.data(), counter, capacity, tab.data(), t0, nt, 3u, wgs, stores.data());
      if (worked != (variant == 1 ? 0 : capacity)) return 1;
      for (size_t i = 0; i < capacity; i ++) {
        ftkx_cp_t want = made[i];
        const bool skipped = i >= worked || i == n / 2 || i == n / 3;
        if (!skipped) {
          const SampleIn in{made[i].tag, reinterpret_cast<const unsigned *>(&made[i])[15], 0u};
          double r[2];
          if (!sample_record<ND>(m, fan, in, tab.data(), t0, 3u, r)) return 1;
          want.scalar[1] = r[0]; want.scalar[2] = r[1];
        }
        if (memcmp(&want, &recs[i], sizeof(want)) != 0 || stores[2 * i] != (skipped ? 0u : 1u) || stores[2 * i + 1] != (skipped ? 0u : 1u)) {
          fprintf(stderr, "series_sample_lane: nd %d wgs %d variant %d record %zu\n", ND, wgs, variant, i);
          return 1;
        }
      }
    }
  return 0;
}

int main()
{
  if (sweep_all<2>(k_fan3, 1) || sweep_all<2>(k_fan3, 0) || sweep_all<3>(k_fan4, 1) || sweep_all<3>(k_fan4, 0)) return 1;
  // the slot rule: all, none, some
  const unsigned char all[3] = {3, 3, 3}, none[3] = {0, 0, 0}, some[3] = {1, 3, 1}, one[3] = {2, 2, 2};
  unsigned slots = 9;
  if (series_sample_slots(all, 3, &slots) != 0 || slots != 3u) return 1;
  if (series_sample_slots(none, 3, &slots) != 0 || slots != 0u) return 1;
  if (series_sample_slots(some, 3, &slots) != 2 || slots != 0u) return 1;
  if (series_sample_slots(one, 3, &slots) != 0 || slots != 2u) return 1;
  printf("series_sample_host run complete\n");
  return 0;
}
#endif
