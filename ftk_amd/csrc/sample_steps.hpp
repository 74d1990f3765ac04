// Auxiliary scalar fields sampled at critical points: what one record's scalar[1] / scalar[2] become, for sample_kernels.hip.
//
// Reference: critical_point_tracker::set_scalar_components (filters/critical_point_tracker.hh:50-51, 178, 516-519) names up to
// FTK_CP_MAX_NUM_VARS = 3 scalars per point; the trackers interpolate every component with the critical point's barycentric weights
// (critical_point_tracker_2d_unstructured.hh:94-96, 216-217), the way the regular trackers fill scalar[0] (2d:633-640, 3d:472-480; lerp_s2 /
// lerp_s3 of numeric/linear_interpolation.hh).
//
// For one record (tag + the aux word of include/ftkx.h) this header
//   1. finds the element: timestep and the ordinal bit from the aux word, corner and type from the tag under the mesh's tag_mode -- the
//      inverse of core_linear x (types of the scope) + fan.local_index (FTKX_TAG_WORK_INDEX) or of element_tag (FTKX_TAG_EXACT64, and
//      FTKX_TAG_REFERENCE while its int32 products cannot have wrapped: sample_reference_tags_exact);
//   2. takes the simplex's nd + 1 vertices from fan_tables.hpp, bit nd of a vertex mask selecting slice t or t + 1;
//   3. forms the weights mu exactly as make_record_impl does (sweep_device.hpp): v from the stored V or the gradient of S, 2D
//      solve_barycentric2 and clamp_barycentric<3> only where the solve failed, 3D solve_barycentric3 and clamp_barycentric<4> always;
//   4. lerps the aux arrays: acc = a[0] * mu[0]; acc = acc + a[i] * mu[i], left to right -- the order scalar[0] takes.
// Sampling a slice's own S therefore gives scalar[0] bit for bit (tests/test_sample_steps_host.py holds that against the reference's
// records).  Build with -ffp-contract=off.
//
// sweep_device.hpp's clampi / gradient_at / vector_at are device functions of a header that does not compile without HIP; they are
// restated here over SampleMesh (the part of Mesh the sampler reads), same FP64 operations in the same order.  Everything compiles with a
// plain C++ compiler (tests/hostcheck/sample_host.cpp).
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/ftkx.h"
#include "cp_device.hpp"
#include "fan_tables.hpp"

namespace ftkx {

constexpr int kSampleThreads = 256;

struct SampleMesh {
  int tag_mode;              // FTKX_TAG_*
  int scalar_mode;           // 1: v = gradient2D/3D(S) evaluated at the vertices; 0: stored V
  int dom_lb[3], dom_sz[3];  // the tracker's domain (element tags count inside it)
  int core_st[3], core_sz[3];
  int ext_st[3], ext_sz[3];  // the array lattice
};

// the arrays of one timestep (device pointers in the kernel); A[s]: the aux array of slot s + 1, or null
struct SampleSlice {
  const double *S, *V;
  const double *A[2];
};

// what goes up per record: 16 bytes
struct SampleIn {
  u64 tag;
  unsigned aux;              // bit 0 ordinal, bits 1.. timestep (include/ftkx.h)
  unsigned pad;
};

// FTKX_TAG_REFERENCE: every int32 product of element::to_integer stays below 2^31 for timesteps up to t_max + 1 -- the bound the
// device-driven pass uses (series.hip, series_applicable) -- so the tags equal the 64-bit ones
inline bool sample_reference_tags_exact(int nd, const long long dom_sz[3], int t_max)
{
  long double bound = nd == 2 ? 12.0L : 60.0L;
  for (int d = 0; d < nd; d ++) bound *= (long double)dom_sz[d];
  return bound * ((long double)t_max + 2.0L) < 2147483648.0L;
}

FTKX_HD inline int sample_clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

// gradient2D / gradient3D of ndarray/grad.hh at one vertex (sweep_device.hpp, gradient_at)
template <int ND>
FTKX_HD inline void sample_gradient_at(const SampleMesh &m, const double *S, int i, int j, int k, double g[ND])
{
  const int DW = m.ext_sz[0], DH = m.ext_sz[1];
  if constexpr (ND == 2) {
    const int ip = sample_clampi(i + 1, 0, DW - 1), im = sample_clampi(i - 1, 0, DW - 1), jp = sample_clampi(j + 1, 0, DH - 1), jm = sample_clampi(j - 1, 0, DH - 1);
    const int ic = sample_clampi(i, 0, DW - 1), jc = sample_clampi(j, 0, DH - 1);
    g[0] = (S[(size_t)ip + (size_t)DW * jc] - S[(size_t)im + (size_t)DW * jc]) * (double)(DW - 1);
    g[1] = (S[(size_t)ic + (size_t)DW * jp] - S[(size_t)ic + (size_t)DW * jm]) * (double)(DH - 1);
  } else {
    const int DD = m.ext_sz[2];
    if (i >= 1 && i < DW - 1 && j >= 1 && j < DH - 1 && k >= 1 && k < DD - 1) {
      const size_t sy = (size_t)DW, sz = (size_t)DW * DH, c = (size_t)i + sy * j + sz * k;
      g[0] = 0.5 * (S[c + 1] - S[c - 1]);
      g[1] = 0.5 * (S[c + sy] - S[c - sy]);
      g[2] = 0.5 * (S[c + sz] - S[c - sz]);
    } else { g[0] = 0.0; g[1] = 0.0; g[2] = 0.0; }
  }
}

// a linear index over a box of nd sizes (x fastest) -> the offsets; 32-bit divisions where the box has fewer than 2^32 cells
template <int ND>
FTKX_HD inline void sample_unravel(const int *sz, u64 lin, int *off)
{
  u64 cells = 1;
  for (int d = 0; d < ND; d ++) cells *= (u64)sz[d];
  if (lin < (1ull << 32) && cells < (1ull << 32)) {
    unsigned l = (unsigned)lin;
    for (int d = 0; d < ND; d ++) { const unsigned s = (unsigned)sz[d], q = l / s; off[d] = (int)(l - q * s); l = q; }
  } else
    for (int d = 0; d < ND; d ++) { off[d] = (int)(lin % (u64)sz[d]); lin /= (u64)sz[d]; }
}

// step 1: the element of a record.  false: the tag is not one of this mesh under its tag mode (a type past the fan, a corner index past
// the box, a type whose scope is not the aux word's), or a vertex of the simplex lies outside the array -- nothing may be read for it
template <int ND>
FTKX_HD inline bool sample_element(const SampleMesh &m, const fan_table<ND + 1> &fan, u64 tag, unsigned aux, int corner[ND + 1], int &type)
{
  constexpr int N = ND + 1;
  const bool ordinal = (aux & 1u) != 0;
  const int t = (int)(aux >> 1);
  corner[ND] = t;
  u64 lin, cells = 1;
  int off[ND];
  if (m.tag_mode == FTKX_TAG_WORK_INDEX) {
    const unsigned nt = ordinal ? (unsigned)fan_table<N>::NORD : (unsigned)fan_table<N>::NINT;
    unsigned local;
    if (tag < (1ull << 32)) { const unsigned g = (unsigned)tag, q = g / nt; local = g - q * nt; lin = q; }
    else { lin = tag / nt; local = (unsigned)(tag - lin * nt); }
    type = ordinal ? fan.ord_types[local] : fan.int_types[local];
    for (int d = 0; d < ND; d ++) cells *= (u64)m.core_sz[d];
    if (lin >= cells) return false;
    sample_unravel<ND>(m.core_sz, lin, off);
    for (int d = 0; d < ND; d ++) corner[d] = m.core_st[d] + off[d];
  } else {
    constexpr unsigned nt = (unsigned)fan_table<N>::NTYPES;
    if (tag < (1ull << 32)) { const unsigned g = (unsigned)tag, q = g / nt; type = (int)(g - q * nt); lin = q; }
    else { lin = tag / nt; type = (int)(tag - lin * nt); }
    for (int d = 0; d < ND; d ++) cells *= (u64)m.dom_sz[d];
    const u64 base = (u64)t * cells;                    // the time axis is the slowest one and counts from 0
    if (lin < base || lin - base >= cells) return false;
    sample_unravel<ND>(m.dom_sz, lin - base, off);
    for (int d = 0; d < ND; d ++) corner[d] = m.dom_lb[d] + off[d];
    if ((fan.ordinal[type] != 0) != ordinal) return false;
  }
  for (int d = 0; d < ND; d ++) { const int a = corner[d] - m.ext_st[d]; if (a < 0 || a + 1 >= m.ext_sz[d]) return false; }
  return true;
}

// steps 2-4.  tab[0] / tab[1]: the arrays of the record's timestep and of the one behind it (read only where a vertex lies in it).
// slots: bit s set = out[s] = the lerp of A[s] (slot s + 1 of the record)
template <int ND>
FTKX_HD inline void sample_simplex(const SampleMesh &m, const fan_table<ND + 1> &fan, const int *corner, int type, const SampleSlice &s0, const SampleSlice &s1,
                                   unsigned slots, double out[2])
{
  constexpr int N = ND + 1;
  unsigned vms[N];
  for (int i = 0; i < N; i ++) vms[i] = fan.vert[type][i];
  double v[N][ND], a[2][N];
  // every load of the record first: the gathers of the N vertices do not depend on one another
  for (int i = 0; i < N; i ++) {
    const unsigned vm = vms[i];
    const bool next = ((vm >> ND) & 1u) != 0;
    const int ai = corner[0] + (int)(vm & 1u) - m.ext_st[0], aj = corner[1] + (int)((vm >> 1) & 1u) - m.ext_st[1],
              ak = ND == 3 ? corner[2] + (int)((vm >> 2) & 1u) - m.ext_st[2] : 0;
    size_t at = (size_t)ai + (size_t)m.ext_sz[0] * (size_t)aj;
    if (ND == 3) at += (size_t)m.ext_sz[0] * (size_t)m.ext_sz[1] * (size_t)ak;
    const double *const S = next ? s1.S : s0.S, *const V = next ? s1.V : s0.V;
    if (m.scalar_mode) sample_gradient_at<ND>(m, S, ai, aj, ak, v[i]);
    else for (int c = 0; c < ND; c ++) v[i][c] = V[at * ND + c];
    for (int s = 0; s < 2; s ++) {
      const double *const A = next ? s1.A[s] : s0.A[s];
      a[s][i] = ((slots >> s) & 1u) ? A[at] : 0.0;
    }
  }
  double mu[N];
  if constexpr (ND == 2) {
    if (!solve_barycentric2(v, mu)) clamp_barycentric<3>(mu);      // 2d:626-631
  } else {
    solve_barycentric3(v, mu);
    clamp_barycentric<4>(mu);                                      // 3d:470, unconditional
  }
  for (int s = 0; s < 2; s ++) {
    double acc = a[s][0] * mu[0];
    for (int i = 1; i < N; i ++) acc = acc + a[s][i] * mu[i];
    out[s] = acc;
  }
}

// one record: tab is indexed by timestep - t_min and has an entry for every timestep a record reads
template <int ND>
FTKX_HD inline bool sample_record(const SampleMesh &m, const fan_table<ND + 1> &fan, const SampleIn &in, const SampleSlice *tab, int t_min, unsigned slots, double out[2])
{
  int corner[ND + 1], type = 0;
  out[0] = 0.0; out[1] = 0.0;
  if (!sample_element<ND>(m, fan, in.tag, in.aux, corner, type)) return false;
  const int at = corner[ND] - t_min;
  const SampleSlice s0 = tab[at];
  const SampleSlice s1 = fan.ordinal[type] ? s0 : tab[at + 1];
  sample_simplex<ND>(m, fan, corner, type, s0, s1, slots, out);
  return true;
}

// ---- the series pass samples its own records (ftkx_set_series_sampling; series_sample_kernel in sample_kernels.hip, queued by series.hip) ----
// One lane of the kernel's grid-stride loop, in place over the records the pass left in device memory: records first, first + stride, ...
// below n.  A lane loads the tag and word 15 (the aux word) of its record, samples it (sample_record: every gather before the solve) and
// hands the armed slots to `store(address, value)` -- the kernel stores with the scope the record kernel's stores have, the host build
// (tests/hostcheck/series_sample_host.cpp) plainly.  No other byte of a record is written.  A record that is no element of the mesh, or
// whose timestep has no entry in the table (tab[0 .. ntab): timestep t_min + k, null arrays where the pass reads no slice), is left as it
// is: the records of a pass are its own steps', so this is a guard against reading outside the table, not a path that is taken.
template <int ND, class Store>
FTKX_HD inline void series_sample_lane(const SampleMesh &m, const fan_table<ND + 1> &fan, ftkx_cp_t *recs, size_t n, const SampleSlice *tab, int t_min, int ntab,
                                       unsigned slots, size_t first, size_t stride, Store store)
{
  for (size_t i = first; i < n; i += stride) {
    const SampleIn in{recs[i].tag, reinterpret_cast<const unsigned *>(recs + i)[15], 0u};
    const long long at = (long long)(in.aux >> 1) - (long long)t_min, last = (in.aux & 1u) ? at : at + 1;
    if (at < 0 || last >= (long long)ntab) continue;
    if (m.scalar_mode ? (!tab[at].S || !tab[last].S) : (!tab[at].V || !tab[last].V)) continue;
    double r[2];
    if (!sample_record<ND>(m, fan, in, tab, t_min, slots, r)) continue;
    if (slots & 1u) store(&recs[i].scalar[1], r[0]);
    if (slots & 2u) store(&recs[i].scalar[2], r[1]);
  }
}

// the slices the steps of a pass read, in time order: a step's own, and the one behind it for an interval sweep (series.hip: P.slice_ts)
inline void series_slice_timesteps(const int *ts, const int *scopes, int n, std::vector<int> &slice_ts)
{
  for (int i = 0; i < n; i ++) {
    if (slice_ts.empty() || slice_ts.back() != ts[i]) slice_ts.push_back(ts[i]);
    if (scopes[i] & FTKX_SCOPE_INTERVAL) slice_ts.push_back(ts[i] + 1);
  }
}

// The slot rule of an armed pass, decided when it is submitted.  have[j]: bit s set = slot s + 1 has an aux array at the j-th of the k
// slices the pass reads.  A slot with an array at every one of them is sampled (bit s of *slots), one with none is left zero.  Returns 0,
// or the slot (1 | 2) that has an array at some of the slices but not all: the pass is refused (FTKX_E_NOSLICE) and *slots is 0.
inline int series_sample_slots(const unsigned char *have, size_t k, unsigned *slots)
{
  *slots = 0;
  unsigned all = 0;
  for (int s = 0; s < 2; s ++) {
    size_t with = 0;
    for (size_t j = 0; j < k; j ++) with += (have[j] >> s) & 1u;
    if (with != 0 && with != k) { *slots = 0; return s + 1; }
    if (with != 0) all |= 1u << s;
  }
  *slots = all;
  return 0;
}

}  // namespace ftkx
