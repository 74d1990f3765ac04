// A vector snapshot given as one array per component, interleaved on the device: the value of one element, the plan of a launch and what
// the lanes of it do, for concat_kernels.hip.
//
// Reference (one host thread): ndarray_stream reads "u, v, w in separate variables" as nv arrays and joins them with ndarray<T>::concat
// (include/ftk/ndarray/stream.hh:1347-1354, 1371-1378, 1423-1433; include/ftk/ndarray.hh:1157-1172): result[i * n1 + j] = arrays[j][i], the
// components fastest.  Here dst[v * NC + k] = (double)plane_k[v] for v < count, NC 2 or 3, T float or double.  A float is widened with
// widen_one (widen_steps.hpp: exact).  A double is moved as 64 bits and never passes through arithmetic: the payload of a NaN, a
// signalling one included, arrives as it left.
//
// The plan generalises WidenPlan.  The body works in groups of G = 16 / sizeof(T) vertices: a lane reads one 16-byte piece of every plane
// (NC loads), which make NC * G doubles that lie in one run of the output (float: 96 or 64 bytes, double: 48 or 32).  That is possible only
// where all NC planes have the same address modulo 16 -- one common `head` of 0 .. G - 1 vertices brings them to 16 bytes together -- and
// dst + head * NC is a multiple of 16 as well.  Then the head's vertices go one by one to lanes 0 .. G - 1 of workgroup 0 and the up to
// G - 1 vertices behind the last whole group to its lanes G .. 2G - 1.  Otherwise every vertex goes on its own (NC narrow loads, NC 8-byte
// stores): head 0, nvec = count, no tail.  Planes start at any multiple of sizeof(T), dst at any multiple of 8, dst overlaps no plane (the
// callers check, ingest.hip); planes may be one another.
//
// How the body's doubles reach memory was decided by measurement (NOTES, "Planar vector snapshots"), per element type:
//   double planes: DIRECT.  The lane that loaded a group stores its run itself, as 16-byte stores; groups are dealt to the lanes of a capped
//     grid in a grid-stride loop (concat_lane).  A wavefront's store instruction writes 64 pieces 48 or 32 bytes apart.
//   float planes: STAGED through LDS.  A workgroup takes tiles of kConcatThreads groups (tile = block, block + nblocks, ...).  Fill: the lane
//     leaves its group's doubles in LDS where they will lie in the tile's output (concat_tile_fill).  Behind a barrier, drain: store
//     instruction i of lane `tid` writes 16-byte piece i * kConcatThreads + tid of that image (concat_tile_drain), so a wavefront's store is
//     1 KiB of consecutive addresses.  A second barrier ends the tile; head and tail go to workgroup 0 afterwards (concat_edges).
// The vertex-wise variant is the direct one for both.
//
// Everything here compiles with a plain C++ compiler as well (tests/hostcheck/concat_host.cpp drives it lane by lane, a staged tile phase by
// phase): the host build of these functions is the kernel's oracle.
#pragma once
#include <cstddef>

#include "widen_steps.hpp"

#if defined(__HIPCC__)
#define CONCAT_HD __host__ __device__ inline
#else
#define CONCAT_HD inline
#endif

namespace ftkx {

constexpr int kConcatThreads = 256;
constexpr unsigned kConcatMaxBlocks = 2048;     // the grid's cap (8 workgroups for each of 256 CUs); the rest is taken by the loops
template <class T> constexpr int concat_group() { return 16 / (int)sizeof(T); }      // vertices per 16-byte load of a plane
template <class T> constexpr bool concat_staged() { return sizeof(T) == 4; }         // the 16-byte body goes through LDS
// LDS of the 16-byte body's kernel, bytes per workgroup (tests/test_concat_kernel_budget.py reads these and holds the compiler's figures to them)
constexpr int kConcatLdsBytesFloat3 = 24576;
constexpr int kConcatLdsBytesFloat2 = 16384;
constexpr int kConcatLdsBytesDouble = 0;
template <class T, int NC> constexpr int concat_tile_words() { return kConcatThreads * NC * concat_group<T>(); }      // a tile's output, 64-bit words
static_assert(concat_tile_words<float, 3>() * 8 == kConcatLdsBytesFloat3 && concat_tile_words<float, 2>() * 8 == kConcatLdsBytesFloat2, "the stated LDS sizes are the tiles'");
static_assert(concat_staged<float>() && !concat_staged<double>() && kConcatLdsBytesDouble == 0, "double planes take the direct form");

// the planes of one launch, by value (a kernel argument)
template <class T, int NC> struct ConcatPlanes { const T *p[NC]; };

// one element, as the 64 bits that are stored
CONCAT_HD unsigned long long concat_bits(const float *p)
{
  const double d = widen_one(*p);
  unsigned long long u;
  __builtin_memcpy(&u, &d, 8);
  return u;
}
CONCAT_HD unsigned long long concat_bits(const double *p)
{
  unsigned long long u;
  __builtin_memcpy(&u, p, 8);
  return u;
}
CONCAT_HD void concat_store(double *dst, unsigned long long u) { __builtin_memcpy(dst, &u, 8); }

struct ConcatPlan {
  size_t count;      // vertices in all
  size_t head;       // [0, head): one by one, lanes 0 .. head - 1 of workgroup 0
  size_t nvec;       // vec: groups of G vertices from `head` on; otherwise the vertices themselves
  int group;         // G
  bool vec;          // the body's accesses are 16 bytes wide
  CONCAT_HD size_t tail_at() const { return vec ? head + nvec * (size_t)group : count; }     // [tail_at, count): one by one, lanes G .. 2G - 1 of workgroup 0
};

template <class T, int NC> inline ConcatPlan concat_plan(const ConcatPlanes<T, NC> &pl, size_t count, const double *dst)
{
  constexpr int G = concat_group<T>();
  ConcatPlan p;
  p.count = count;
  p.group = G;
  const size_t head = ((16 - ((size_t)pl.p[0] & 15)) & 15) / sizeof(T);
  bool vec = (((size_t)(dst + head * NC)) & 15) == 0;
  for (int k = 1; k < NC; k ++) vec = vec && (((size_t)pl.p[k] ^ (size_t)pl.p[0]) & 15) == 0;
  p.vec = vec;
  p.head = !vec ? 0 : head > count ? count : head;
  p.nvec = vec ? (count - p.head) / (size_t)G : count;
  return p;
}

// tiles of the staged body == workgroups a lane per group (or vertex) would take
CONCAT_HD size_t concat_tiles(const ConcatPlan &p) { return (p.nvec + (size_t)kConcatThreads - 1) / (size_t)kConcatThreads; }

// how many workgroups the plan is launched with
inline unsigned concat_blocks(const ConcatPlan &p)
{
  const size_t want = concat_tiles(p);
  return want < 1 ? 1u : want > (size_t)kConcatMaxBlocks ? kConcatMaxBlocks : (unsigned)want;
}

// vertex v on its own: NC narrow loads, NC 8-byte stores
template <class T, int NC> CONCAT_HD void concat_vertex(const ConcatPlanes<T, NC> &pl, size_t v, double *dst)
{
  unsigned long long u[NC];
  for (int k = 0; k < NC; k ++) u[k] = concat_bits(pl.p[k] + v);
  for (int k = 0; k < NC; k ++) concat_store(dst + v * NC + k, u[k]);
}

// the group of G vertices at v of the body: one 16-byte load per plane, the NC * G doubles they make to `out` (global memory or LDS, a
// multiple of 16 bytes) as a run of 16-byte stores
template <class T, int NC> CONCAT_HD void concat_group_to(const ConcatPlanes<T, NC> &pl, size_t v, void *out)
{
  constexpr int G = concat_group<T>();
  unsigned long long w[NC * G];
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned __attribute__((ext_vector_type(4))) piece_t;          // 16 bytes of a plane, as they lie
  typedef unsigned long long __attribute__((ext_vector_type(2))) pair_t;
  piece_t in[NC];
#pragma unroll
  for (int k = 0; k < NC; k ++) in[k] = *reinterpret_cast<const piece_t *>(pl.p[k] + v);
#pragma unroll
  for (int k = 0; k < NC; k ++)
#pragma unroll
    for (int j = 0; j < G; j ++) {
      if constexpr (sizeof(T) == 4) w[j * NC + k] = (unsigned long long)__double_as_longlong(widen_one(__uint_as_float(in[k][j])));
      else w[j * NC + k] = (unsigned long long)in[k][2 * j] | ((unsigned long long)in[k][2 * j + 1] << 32);
    }
#pragma unroll
  for (int i = 0; i < NC * G / 2; i ++) { pair_t q; q[0] = w[2 * i]; q[1] = w[2 * i + 1]; static_cast<pair_t *>(out)[i] = q; }
#else
  for (int k = 0; k < NC; k ++)
    for (int j = 0; j < G; j ++) w[j * NC + k] = concat_bits(pl.p[k] + v + j);
  __builtin_memcpy(out, w, sizeof(w));
#endif
}

// head and tail: lanes 0 .. 2G - 1 of workgroup 0
template <class T, int NC> CONCAT_HD void concat_edges(const ConcatPlanes<T, NC> &pl, const ConcatPlan &p, double *dst, int tid)
{
  constexpr int G = concat_group<T>();
  if (tid < G) { if ((size_t)tid < p.head) concat_vertex<T, NC>(pl, (size_t)tid, dst); }
  else if (tid < 2 * G) { const size_t v = p.tail_at() + (size_t)(tid - G); if (v < p.count) concat_vertex<T, NC>(pl, v, dst); }
}

// DIRECT (the 16-byte body of double planes; the vertex-wise variant of both types): what lane `tid` of workgroup `block` does
template <class T, int NC, bool VEC> CONCAT_HD void concat_lane(const ConcatPlanes<T, NC> &pl, const ConcatPlan &p, double *dst, size_t block, size_t nblocks, int tid)
{
  constexpr int G = concat_group<T>();
  const size_t stride = nblocks * (size_t)kConcatThreads;
  for (size_t g = block * (size_t)kConcatThreads + (size_t)tid; g < p.nvec; g += stride) {
    if (VEC) concat_group_to<T, NC>(pl, p.head + g * (size_t)G, dst + (p.head + g * (size_t)G) * NC);
    else concat_vertex<T, NC>(pl, g, dst);
  }
  if (VEC && block == 0) concat_edges<T, NC>(pl, p, dst, tid);
}

// STAGED (the 16-byte body of float planes), phase 1 of tile `tile`: lane `tid` leaves its group in lds (concat_tile_words<T, NC>() words)
template <class T, int NC> CONCAT_HD void concat_tile_fill(const ConcatPlanes<T, NC> &pl, const ConcatPlan &p, size_t tile, int tid, unsigned long long *lds)
{
  constexpr int G = concat_group<T>();
  const size_t g = tile * (size_t)kConcatThreads + (size_t)tid;
  if (g < p.nvec) concat_group_to<T, NC>(pl, p.head + g * (size_t)G, lds + (size_t)tid * (NC * G));
}

// ... phase 2, behind a barrier: lane `tid` stores pieces tid, kConcatThreads + tid, ... of the tile's image (another barrier follows)
template <class T, int NC> CONCAT_HD void concat_tile_drain(const unsigned long long *lds, const ConcatPlan &p, size_t tile, int tid, double *dst)
{
  constexpr int P = NC * concat_group<T>() / 2;                   // 16-byte pieces per group
  const size_t first = tile * (size_t)kConcatThreads * P, end = p.nvec * (size_t)P;      // pieces of the body: this tile's first, and behind the last
  double *body = dst + p.head * NC;
  for (int i = 0; i < P; i ++) {
    const size_t q = (size_t)i * kConcatThreads + (size_t)tid;
    if (first + q >= end) break;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned long long __attribute__((ext_vector_type(2))) pair_t;
    reinterpret_cast<pair_t *>(body)[first + q] = reinterpret_cast<const pair_t *>(lds)[q];
#else
    concat_store(body + 2 * (first + q), lds[2 * q]);
    concat_store(body + 2 * (first + q) + 1, lds[2 * q + 1]);
#endif
  }
}

}  // namespace ftkx
