// Float32 snapshots widened to FP64 on the device: the conversion of one element, the plan of a launch and what one lane of it does, for
// widen_kernels.hip.
//
// Reference (one host thread): ndarray_stream::request_timestep_file_binary<float> (include/ftk/ndarray/stream.hh:986-987, 1066-1069)
// reads a "float32" file into an ndarray<float> and widens it with ndarray::from_array, p[i] = static_cast<T>(array1[i])
// (include/ftk/ndarray.hh:403-410).  Every float is a double -- subnormals, which become normal doubles, and both zeros included -- so the
// conversion is exact and there is nothing to round; a NaN stays a NaN with its sign (which payload it carries is not specified).
//
// The plan.  A lane of the body reads 4 floats with one 16-byte load and writes them as two 16-byte stores.  Pooled and hipMalloc'ed arrays
// are aligned; a borrowed source may start at any multiple of 4 bytes and a destination at any multiple of 8.  `head` elements (0 to 3)
// are peeled so that the source of the body is a multiple of 16; if the destination is one behind that same head, the body is made of
// `nvec` groups of four and at most three elements are left behind it (the tail).  Otherwise source and destination cannot be brought
// to 16 bytes together, and every element goes on its own (4 bytes in, 8 out): head 0, nvec = count, no tail.
// Groups are dealt to the lanes of a capped grid in a grid-stride loop; lanes 0-2 of workgroup 0 take the head, its lanes 4-6 the tail.
//
// Everything here compiles with a plain C++ compiler as well (tests/hostcheck/widen_host.cpp drives it lane by lane).
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define WIDEN_HD __host__ __device__ inline
#else
#define WIDEN_HD inline
#endif

namespace ftkx {

constexpr int kWidenThreads = 256;
constexpr unsigned kWidenMaxBlocks = 2048;      // the grid's cap (8 workgroups for each of 256 CUs); the rest is taken by the grid-stride loop
constexpr int kWidenGroup = 4;                  // floats per 16-byte load

// one element
WIDEN_HD double widen_one(float f) { return static_cast<double>(f); }

struct WidenPlan {
  size_t count;      // elements in all
  size_t head;       // [0, head): one by one, lanes 0 .. head - 1 of workgroup 0
  size_t nvec;       // vec: groups of four from `head` on; otherwise the elements themselves
  bool vec;          // the body's accesses are 16 bytes wide
  WIDEN_HD size_t tail_at() const { return vec ? head + nvec * (size_t)kWidenGroup : count; }     // [tail_at, count): one by one, lanes 4 .. 6 of workgroup 0
};

// src: a multiple of 4 bytes, dst: a multiple of 8 (checked by the callers, ingest.hip)
inline WidenPlan widen_plan(const float *src, size_t count, const double *dst)
{
  WidenPlan p;
  p.count = count;
  size_t head = ((16 - ((size_t)src & 15)) & 15) / sizeof(float);
  if (head > count) head = count;
  p.vec = (((size_t)(src + head)) & 15) == 0 && (((size_t)(dst + head)) & 15) == 0;
  p.head = p.vec ? head : 0;
  p.nvec = p.vec ? (count - head) / (size_t)kWidenGroup : count;
  return p;
}

// how many workgroups the plan is launched with
inline unsigned widen_blocks(const WidenPlan &p)
{
  const size_t want = (p.nvec + (size_t)kWidenThreads - 1) / (size_t)kWidenThreads;
  return want < 1 ? 1u : want > (size_t)kWidenMaxBlocks ? kWidenMaxBlocks : (unsigned)want;
}

// group g of the body: 16 bytes in, 32 out
WIDEN_HD void widen_group(const float *src, double *dst)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const float4 v = *reinterpret_cast<const float4 *>(src);
  reinterpret_cast<double2 *>(dst)[0] = make_double2(widen_one(v.x), widen_one(v.y));
  reinterpret_cast<double2 *>(dst)[1] = make_double2(widen_one(v.z), widen_one(v.w));
#else
  const float v[kWidenGroup] = {src[0], src[1], src[2], src[3]};
  for (int k = 0; k < kWidenGroup; k ++) dst[k] = widen_one(v[k]);
#endif
}

// what lane `tid` of workgroup `block` does
template <bool VEC> WIDEN_HD void widen_lane(const float *src, const WidenPlan &p, double *dst, size_t block, size_t nblocks, int tid)
{
  const size_t stride = nblocks * (size_t)kWidenThreads;
  for (size_t g = block * (size_t)kWidenThreads + (size_t)tid; g < p.nvec; g += stride) {
    if (VEC) widen_group(src + p.head + g * (size_t)kWidenGroup, dst + p.head + g * (size_t)kWidenGroup);
    else dst[g] = widen_one(src[g]);
  }
  if (VEC && block == 0) {
    if (tid < kWidenGroup) { if ((size_t)tid < p.head) dst[tid] = widen_one(src[tid]); }
    else if (tid < 2 * kWidenGroup) { const size_t e = p.tail_at() + (size_t)(tid - kWidenGroup); if (e < p.count) dst[e] = widen_one(src[e]); }
  }
}

}  // namespace ftkx
