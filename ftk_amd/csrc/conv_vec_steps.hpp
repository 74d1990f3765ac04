// Spatial Gaussian smoothing of a VECTOR snapshot, every component as the scalar field it is: what conv_vec_kernels.hip adds to conv_steps.hpp.
//
// The rule: for an array V of nc components (nc = nd, like every V of this library)
//     conv_vec(V)[c + nc * i] == conv(plane_c)[i]        with plane_c[i] = V[c + nc * i]
// where conv is what conv_kernel computes -- byte for byte: the tile (ConvTile), the lanes' places (conv_lane), the tiles' order
// (conv_tile_origin), the per-output arithmetic (conv_outputs, conv_tap) are conv_steps.hpp's own, used as they are.  Components never mix.
// (Not the reference's conv_gaussian on such an array: that dispatches on nd() and would convolve a (2, W, H) array ACROSS its components.)
//
// What is new is how a component of the source is found: (base pointer, element stride).  An interleaved array V: V + c, stride nc; planes:
// planes[c], stride 1.  One staging function, and one kernel template, serve both.  A workgroup takes all nc components of its tile one after
// the other through ONE staged plane, so its LDS is the scalar kernel's.
//
// Compiles with a plain C++ compiler as well (tests/hostcheck/conv_vec_host.cpp restates the kernel's loops around it); -ffp-contract=off is
// part of the contract on both sides.
#pragma once
#include "conv_steps.hpp"

namespace ftkx {

// The nc components of a source; stride in elements, the same for all of them.
template <class SRC> struct ConvVecSource {
  const SRC *base[3];
  size_t stride;
};
template <class SRC> CONV_HD ConvVecSource<SRC> conv_vec_interleaved(const SRC *V, int nc)
{
  return ConvVecSource<SRC>{{V, V + 1, nc > 2 ? V + 2 : nullptr}, (size_t)nc};
}
template <class SRC> CONV_HD ConvVecSource<SRC> conv_vec_planes(const SRC *const *planes, int nc)
{
  return ConvVecSource<SRC>{{planes[0], planes[1], nc > 2 ? planes[2] : nullptr}, (size_t)1};
}
// (a select, not an index: a kernel argument indexed by a variable is copied to scratch first)
template <class SRC> CONV_HD const SRC *conv_vec_base(const ConvVecSource<SRC> &s, int c) { return c == 0 ? s.base[0] : c == 1 ? s.base[1] : s.base[2]; }

// what a workgroup of conv_vec_kernel<ND, K, SRC> holds in LDS: one staged plane, the scalar kernel's (tests/test_conv_vec_kernel_budget.py)
template <int ND, int K> struct ConvVecTile {
  static constexpr int NC = ND;
  static constexpr int LDS_BYTES = ConvTile<ND, K>::DOUBLES * (int)sizeof(double);
};
// 2D: K = 1, 3, 5, 7, 9 -> 34 x 32, 34 x 34, 38 x 36, 38 x 38, 42 x 40 doubles; 3D: 34 x 8 x 8, 34 x 10 x 10, 38 x 12 x 12, 38 x 14 x 10, 42 x 16 x 12
static_assert(ConvVecTile<2, 1>::LDS_BYTES == 8704 && ConvVecTile<2, 3>::LDS_BYTES == 9248 && ConvVecTile<2, 5>::LDS_BYTES == 10944 &&
              ConvVecTile<2, 7>::LDS_BYTES == 11552 && ConvVecTile<2, 9>::LDS_BYTES == 13440, "LDS of the 2D instantiations");
static_assert(ConvVecTile<3, 1>::LDS_BYTES == 17408 && ConvVecTile<3, 3>::LDS_BYTES == 27200 && ConvVecTile<3, 5>::LDS_BYTES == 43776 &&
              ConvVecTile<3, 7>::LDS_BYTES == 42560 && ConvVecTile<3, 9>::LDS_BYTES == 64512, "LDS of the 3D instantiations");

// staged value number `i` (0 <= i < STAGED, x fastest) of the tile at (x0, y0, z0) of ONE component (base, stride): conv_stage with a stride.
// Outside the array: +0.0.  A float source is widened as it is staged.
template <int ND, int K, class SRC> CONV_HD void conv_vec_stage(const SRC *base, size_t stride, const ConvDims &d, int x0, int y0, int z0, int i, double *tile)
{
  typedef ConvTile<ND, K> T;
  const int lx = i % T::SX, ly = (i / T::SX) % T::PY, lz = i / (T::SX * T::PY);
  const int gx = x0 - T::H + lx, gy = y0 - T::H + ly, gz = ND == 2 ? 0 : z0 - T::H + lz;
  double v = 0.0;
  if (gx >= 0 && gx < d.DW && gy >= 0 && gy < d.DH && gz >= 0 && gz < d.DD)
    v = static_cast<double>(base[(((size_t)gz * (size_t)d.DH + (size_t)gy) * (size_t)d.DW + (size_t)gx) * stride]);
  tile[(lz * T::PY + ly) * T::PX + lx] = v;
}

// where output (gx, gy, gz) of component c lies in the interleaved output of nc components
CONV_HD size_t conv_vec_out_index(const ConvDims &d, int nc, int c, int gx, int gy, int gz)
{
  return (((size_t)gz * (size_t)d.DH + (size_t)gy) * (size_t)d.DW + (size_t)gx) * (size_t)nc + (size_t)c;
}

}  // namespace ftkx
