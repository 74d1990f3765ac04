// Half, bfloat16 and 8- / 16- / 32-bit integer snapshots widened to FP64 on the device: the conversion of one element, the plan of a launch
// and what one lane of it does, for narrow_kernels.hip.  widen_steps.hpp generalised by the element's size.
//
// Reference (one host thread): ndarray<T>::from_array<T1>, p[i] = static_cast<T>(array1[i]) (include/ftk/ndarray.hh:401-410), which is what
// image data of unsigned char / short (from_vtk_data_array, ndarray.hh:556-575) and NetCDF variables of NC_BYTE / NC_SHORT / NC_INT
// (nc_get_vara_double, ndarray/ndarray_base.hh:383-391) go through.  Every value of every type here is a double, so the conversion is exact
// and there is nothing to round; a NaN of a half or a bfloat16 stays a NaN with its sign (which payload it carries is not specified).
//
// The plan.  A lane of the body takes a group of 4 elements with ONE load of 4 * sizeof(T) bytes -- a dword, two or four of them -- and
// writes them as two 16-byte stores: whatever the kernel reads, it writes 8 bytes per element and its stores are what it is bound by, so
// every lane's output stays at 32 consecutive bytes and a wavefront's store instruction at 1 KiB of consecutive addresses.  (A lane that
// took 16 source bytes of a 1- or 2-byte type would write runs of 128 / 64 bytes, the shape concat_steps.hpp had to stage through LDS.)
// The sub-word types are unpacked from the loaded dwords with shifts and sign extension.  A source may start at any multiple of its
// element's size and a destination at any multiple of 8: `head` elements (0 to 3) are peeled so that the source of the body is a multiple
// of 4 * sizeof(T); if the destination is a multiple of 16 behind that same head, the body is made of `nvec` groups of four and at most
// three elements are left behind it (the tail).  Otherwise both cannot be had, and every element goes on its own: head 0, nvec = count, no
// tail.  Groups are dealt to the lanes of a capped grid in a grid-stride loop, two groups (one grid apart) a turn, so that a second load is
// under way while the first group is extracted, converted and stored; lanes 0-2 of workgroup 0 take the head, its lanes 4-6 the tail.
// Every index is size_t.
//
// Everything here compiles with a plain C++ compiler as well (tests/hostcheck/narrow_host.cpp drives it lane by lane); the host build
// converts a half with integer operations on its 16 bits and needs no _Float16.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "widen_steps.hpp"      // the grid: kWidenThreads, kWidenMaxBlocks

#if defined(__HIPCC__)
#include <hip/hip_fp16.h>
#endif

namespace ftkx {

// the element types by their code: the values of FTKX_DTYPE_* (include/ftkx.h)
enum NarrowDtype { NARROW_F64 = 0, NARROW_F32, NARROW_F16, NARROW_BF16, NARROW_U8, NARROW_I8, NARROW_U16, NARROW_I16, NARROW_U32, NARROW_I32, NARROW_DTYPES };

inline size_t narrow_dtype_size(int dtype)
{
  switch (dtype) {
  case NARROW_F64: return 8;
  case NARROW_F32: case NARROW_U32: case NARROW_I32: return 4;
  case NARROW_F16: case NARROW_BF16: case NARROW_U16: case NARROW_I16: return 2;
  case NARROW_U8: case NARROW_I8: return 1;
  default: return 0;
  }
}

// the types this file is about: everything narrower than a double but float32, which has widen_steps.hpp
inline bool narrow_dtype_ok(int dtype) { return dtype >= NARROW_F16 && dtype <= NARROW_I32; }

// the two floating types as their 16 bits
struct NarrowHalf { uint16_t bits; };
struct NarrowBf16 { uint16_t bits; };

constexpr int kNarrowGroup = 4;      // elements per load, whatever their size

// IEEE half -> double with integer operations: subnormals (normalised by shifting), both zeros, infinities; a NaN keeps its sign and its
// payload's bits at the top of the double's
WIDEN_HD double narrow_half_by_bits(uint16_t h)
{
  const uint64_t sign = (uint64_t)(h >> 15) << 63;
  uint32_t e = (h >> 10) & 31u, m = h & 1023u;
  uint64_t u;
  if (e == 31u) u = sign | 0x7ff0000000000000ull | ((uint64_t)m << 42);
  else if (e != 0u) u = sign | ((uint64_t)(e + 1008u) << 52) | ((uint64_t)m << 42);      // 1023 - 15
  else if (m == 0u) u = sign;
  else {
    // m * 2^-24, 0 < m < 1024: shifted up until bit 10 is set, the exponent counted down from that of the smallest normal half
    uint32_t ex = 1009u;
    while (!(m & 1024u)) { m <<= 1; ex --; }
    u = sign | ((uint64_t)ex << 52) | ((uint64_t)(m & 1023u) << 42);
  }
  double d;
  memcpy(&d, &u, 8);
  return d;
}

// one element
WIDEN_HD double narrow_one(uint8_t v) { return static_cast<double>(v); }
WIDEN_HD double narrow_one(int8_t v) { return static_cast<double>(v); }
WIDEN_HD double narrow_one(uint16_t v) { return static_cast<double>(v); }
WIDEN_HD double narrow_one(int16_t v) { return static_cast<double>(v); }
WIDEN_HD double narrow_one(uint32_t v) { return static_cast<double>(v); }
WIDEN_HD double narrow_one(int32_t v) { return static_cast<double>(v); }
WIDEN_HD double narrow_one(NarrowBf16 v)
{
  const uint32_t w = (uint32_t)v.bits << 16;      // a bfloat16 is the top half of a float32
  float f;
  memcpy(&f, &w, 4);
  return static_cast<double>(f);
}
WIDEN_HD double narrow_one(NarrowHalf v)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return static_cast<double>(__half2float(__ushort_as_half(v.bits)));      // the hardware's conversion
#else
  return narrow_half_by_bits(v.bits);
#endif
}

// element k (0 .. 3) of a group out of the dwords it was loaded as (little endian): sizeof(T) dwords
template <class T> struct NarrowUnpack;
template <> struct NarrowUnpack<uint8_t> { static WIDEN_HD uint8_t at(const uint32_t *w, int k) { return (uint8_t)((w[0] >> (8 * k)) & 0xffu); } };
template <> struct NarrowUnpack<int8_t> { static WIDEN_HD int8_t at(const uint32_t *w, int k) { return (int8_t)((int32_t)(w[0] << (24 - 8 * k)) >> 24); } };
template <> struct NarrowUnpack<uint16_t> { static WIDEN_HD uint16_t at(const uint32_t *w, int k) { return (uint16_t)((w[k >> 1] >> (16 * (k & 1))) & 0xffffu); } };
template <> struct NarrowUnpack<int16_t> { static WIDEN_HD int16_t at(const uint32_t *w, int k) { return (int16_t)((int32_t)(w[k >> 1] << (16 - 16 * (k & 1))) >> 16); } };
template <> struct NarrowUnpack<uint32_t> { static WIDEN_HD uint32_t at(const uint32_t *w, int k) { return w[k]; } };
template <> struct NarrowUnpack<int32_t> { static WIDEN_HD int32_t at(const uint32_t *w, int k) { return (int32_t)w[k]; } };
template <> struct NarrowUnpack<NarrowHalf> { static WIDEN_HD NarrowHalf at(const uint32_t *w, int k) { return NarrowHalf{NarrowUnpack<uint16_t>::at(w, k)}; } };
template <> struct NarrowUnpack<NarrowBf16> { static WIDEN_HD NarrowBf16 at(const uint32_t *w, int k) { return NarrowBf16{NarrowUnpack<uint16_t>::at(w, k)}; } };

struct NarrowPlan {
  size_t count;      // elements in all
  size_t head;       // [0, head): one by one, lanes 0 .. head - 1 of workgroup 0
  size_t nvec;       // vec: groups of four from `head` on; otherwise the elements themselves
  bool vec;          // the body loads 4 * sizeof(T) bytes and stores 2 x 16
  WIDEN_HD size_t tail_at() const { return vec ? head + nvec * (size_t)kNarrowGroup : count; }     // [tail_at, count): one by one, lanes 4 .. 6 of workgroup 0
};

// src: a multiple of esize (1, 2 or 4) bytes, dst: a multiple of 8 (checked by the callers, ingest.hip)
inline NarrowPlan narrow_plan(const void *src, size_t esize, size_t count, const double *dst)
{
  NarrowPlan p;
  p.count = count;
  const size_t load = (size_t)kNarrowGroup * esize;      // a power of two
  size_t head = ((load - ((size_t)src & (load - 1))) & (load - 1)) / esize;
  if (head > count) head = count;
  p.vec = (((size_t)src + head * esize) & (load - 1)) == 0 && (((size_t)(dst + head)) & 15) == 0;
  p.head = p.vec ? head : 0;
  p.nvec = p.vec ? (count - head) / (size_t)kNarrowGroup : count;
  return p;
}

// how many workgroups the plan is launched with
inline unsigned narrow_blocks(const NarrowPlan &p)
{
  const size_t want = (p.nvec + (size_t)kWidenThreads - 1) / (size_t)kWidenThreads;
  return want < 1 ? 1u : want > (size_t)kWidenMaxBlocks ? kWidenMaxBlocks : (unsigned)want;
}

// group g of the body: 4 * sizeof(T) bytes in with one load (narrow_load), 32 out with two stores (narrow_store)
template <class T> struct NarrowWords { uint32_t w[sizeof(T)]; };

template <class T> WIDEN_HD NarrowWords<T> narrow_load(const T *src)
{
  NarrowWords<T> v;
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (sizeof(T) == 1) v.w[0] = *reinterpret_cast<const uint32_t *>(src);
  else if constexpr (sizeof(T) == 2) { const uint2 q = *reinterpret_cast<const uint2 *>(src); v.w[0] = q.x; v.w[1] = q.y; }
  else { const uint4 q = *reinterpret_cast<const uint4 *>(src); v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w; }
#else
  memcpy(v.w, src, sizeof(v.w));
#endif
  return v;
}

template <class T> WIDEN_HD void narrow_store(const NarrowWords<T> &v, double *dst)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const double a = narrow_one(NarrowUnpack<T>::at(v.w, 0)), b = narrow_one(NarrowUnpack<T>::at(v.w, 1));
  const double c = narrow_one(NarrowUnpack<T>::at(v.w, 2)), d = narrow_one(NarrowUnpack<T>::at(v.w, 3));
  reinterpret_cast<double2 *>(dst)[0] = make_double2(a, b);
  reinterpret_cast<double2 *>(dst)[1] = make_double2(c, d);
#else
  for (int k = 0; k < kNarrowGroup; k ++) dst[k] = narrow_one(NarrowUnpack<T>::at(v.w, k));
#endif
}

// what lane `tid` of workgroup `block` does
template <class T, bool VEC> WIDEN_HD void narrow_lane(const T *src, const NarrowPlan &p, double *dst, size_t block, size_t nblocks, int tid)
{
  const size_t stride = nblocks * (size_t)kWidenThreads;
  size_t g = block * (size_t)kWidenThreads + (size_t)tid;
  if (VEC) {
    // two groups a turn, one grid apart: both loads are under way before the first conversion waits for one of them
    const T *s = src + p.head;
    double *d = dst + p.head;
    for (; g + stride < p.nvec; g += 2 * stride) {
      const NarrowWords<T> v0 = narrow_load<T>(s + g * (size_t)kNarrowGroup), v1 = narrow_load<T>(s + (g + stride) * (size_t)kNarrowGroup);
      narrow_store<T>(v0, d + g * (size_t)kNarrowGroup);
      narrow_store<T>(v1, d + (g + stride) * (size_t)kNarrowGroup);
    }
    if (g < p.nvec) narrow_store<T>(narrow_load<T>(s + g * (size_t)kNarrowGroup), d + g * (size_t)kNarrowGroup);
  } else {
    for (; g < p.nvec; g += stride) dst[g] = narrow_one(src[g]);
  }
  if (VEC && block == 0) {
    if (tid < kNarrowGroup) { if ((size_t)tid < p.head) dst[tid] = narrow_one(src[tid]); }
    else if (tid < 2 * kNarrowGroup) { const size_t e = p.tail_at() + (size_t)(tid - kNarrowGroup); if (e < p.count) dst[e] = narrow_one(src[e]); }
  }
}

}  // namespace ftkx
