// Spatial Gaussian smoothing of a scalar snapshot: what one workgroup stages and what one lane adds up, for conv_kernels.hip.
//
// Reference (single-threaded host loops): include/ftk/ndarray/conv.hh -- gaussian_kernel2D 74-100, gaussian_kernel3D 165-196, conv2D 11-47,
// conv3D 117-163 -- called with padding = ksize / 2 by ndarray_stream::modified_callback (include/ftk/ndarray/stream.hh:1597-1603).
// Per output voxel the reference starts from +0.0 and runs kz outer, ky, kx innermost over the taps inside the array:
//     res += data(x - p + kx, y - p + ky, z - p + kz) * w(kx, ky, kz)        one rounded multiply, then one rounded add (no contraction)
// and ends with res /= ksize^nd (a true division, on top of the normalised weights).  Taps outside the array are skipped there; here they
// are staged as +0.0 and take part: for finite weights the product is a zero of either sign, and the accumulator -- which starts at +0.0 and
// can never become -0.0 -- is unchanged by adding one, so the bits are the same.
//
// The tile: TX = 32 outputs along x by TY by TZ, staged with a halo of K / 2 on every side.  A lane owns R = 4 consecutive outputs along x:
// it reads a row of K + R - 1 staged values once and feeds its R accumulation chains from registers -- each chain still adds its own
// K^nd products in the reference's order.  A row read is (K + 3) / 2 16-byte LDS reads (ds_read_b128; 8-byte reads fused in pairs run at
// half its rate), which the LDS serves in groups of 16 lanes -- lanes {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of each half of the
// wavefront -- and a group is conflict-free when its 16 reads fall on 16 different 16-byte slots of the 256-byte bank row.  Lanes along
// x are 32 bytes apart: eight of them take every other slot, so a group is made of TWO staged rows, eight lanes each, whose distance is
// an odd number of slots: the row pitch PX is 2 mod 4 doubles, and conv_lane() deals the lanes of a group to the rows (0, 1) / (2, 3).
//
// Everything here compiles with a plain C++ compiler as well (tests/hostcheck/conv_host.cpp restates the kernel's loops around it).
// -ffp-contract=off is part of the contract on both sides.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define CONV_HD __host__ __device__ inline
#else
#define CONV_HD inline
#endif

namespace ftkx {

constexpr int kConvMaxK = 9;
constexpr int kConvThreads = 256;

template <int ND, int K> struct ConvTile {
  static_assert(ND == 2 || ND == 3, "2D or 3D");
  static_assert(K >= 1 && K <= kConvMaxK && (K & 1) == 1, "odd sizes from 1 to 9");
  static constexpr int R = 4;                                  // outputs per lane along x
  static constexpr int LX = 8;                                 // lanes along x
  static constexpr int LY = ND == 2 ? 32 : 8;                  // lanes along y
  static constexpr int LZ = ND == 2 ? 1 : 4;                   // lanes along z
  static constexpr int TX = LX * R;                            // 32
  static constexpr int TY = LY;
  static constexpr int TZ = ND == 2 ? 1 : (K <= 5 ? 8 : 4);    // (3D: a lane takes TZ / LZ outputs along z, one after the other)
  static constexpr int H = K / 2;
  static constexpr int SX = TX + K - 1;                        // staged values per row
  static constexpr int PX = (SX + 1) / 4 * 4 + 2;              // row pitch: the smallest one >= SX that is 2 mod 4
  static constexpr int PY = TY + K - 1;
  static constexpr int PZ = ND == 2 ? 1 : TZ + K - 1;
  static constexpr int STAGED = SX * PY * PZ;                  // values a workgroup loads
  static constexpr int DOUBLES = PX * PY * PZ;                 // the tile's doubles in LDS
  static constexpr int TAPS = ND == 2 ? K * K : K * K * K;
  static_assert(LX * LY * LZ == kConvThreads, "one lane per (x group, y, z group)");
  static_assert(PX >= SX && PX % 4 == 2, "pitch");
  static_assert(DOUBLES * 8 <= 64 * 1024, "fits the LDS a workgroup may have without asking");
};

struct ConvDims { int DW, DH, DD; };                           // 2D: DD = 1

// how many tiles cover the array, and where tile number `t` starts (x fastest)
template <int ND, int K> CONV_HD size_t conv_tiles(const ConvDims &d)
{
  typedef ConvTile<ND, K> T;
  return (size_t)((d.DW + T::TX - 1) / T::TX) * (size_t)((d.DH + T::TY - 1) / T::TY) * (size_t)((d.DD + T::TZ - 1) / T::TZ);
}
template <int ND, int K> CONV_HD void conv_tile_origin(const ConvDims &d, size_t t, int *x0, int *y0, int *z0)
{
  typedef ConvTile<ND, K> T;
  const size_t nx = (size_t)((d.DW + T::TX - 1) / T::TX), ny = (size_t)((d.DH + T::TY - 1) / T::TY);
  *x0 = (int)(t % nx) * T::TX;
  *y0 = (int)((t / nx) % ny) * T::TY;
  *z0 = (int)(t / (nx * ny)) * T::TZ;
}

// lane `tid` of the workgroup -> its place (tx, ty, tz) among the LX x LY x LZ lanes.  Four consecutive lanes are consecutive along x; the
// eight quads of half a wavefront are dealt so that each of the LDS's 16-lane groups holds all eight x places of two neighbouring rows.
template <int ND, int K> CONV_HD void conv_lane(int tid, int *tx, int *ty, int *tz)
{
  typedef ConvTile<ND, K> T;
  const int quad = (tid >> 2) & 7, half = tid >> 5;            // half: which 32 lanes (8 x 4 places) of the workgroup
  const int qx[8] = {0, 0, 4, 4, 0, 0, 4, 4}, qy[8] = {0, 3, 3, 0, 2, 1, 1, 2};
  *tx = qx[quad] + (tid & 3);
  *ty = 4 * (half % (T::LY / 4)) + qy[quad];
  *tz = half / (T::LY / 4);
}

// staged value number `i` (0 <= i < STAGED, x fastest) of the tile at (x0, y0, z0): where it goes in the tile and what it is.  SRC: double, or
// float -- a float32 snapshot is widened (exactly: widen_steps.hpp) as it is staged, and the tile holds doubles either way
template <int ND, int K, class SRC> CONV_HD void conv_stage(const SRC *S, const ConvDims &d, int x0, int y0, int z0, int i, double *tile)
{
  typedef ConvTile<ND, K> T;
  const int lx = i % T::SX, ly = (i / T::SX) % T::PY, lz = i / (T::SX * T::PY);
  const int gx = x0 - T::H + lx, gy = y0 - T::H + ly, gz = ND == 2 ? 0 : z0 - T::H + lz;
  double v = 0.0;
  if (gx >= 0 && gx < d.DW && gy >= 0 && gy < d.DH && gz >= 0 && gz < d.DD)
    v = static_cast<double>(S[((size_t)gz * (size_t)d.DH + (size_t)gy) * (size_t)d.DW + (size_t)gx]);
  tile[(lz * T::PY + ly) * T::PX + lx] = v;
}

// one tap of one output: the product is rounded before it is added
CONV_HD double conv_tap(double acc, double v, double w) { const double p = v * w; return acc + p; }

// The R outputs (x .. x + R - 1, y, z) of one lane.  `at` points to the staged value of (x - H, y - H, z - H), i.e. to
// tile[(lz * PY + ly) * PX + lx] for the output at tile position (lx, ly, lz); w: K^ND weights, x fastest.
template <int ND, int K> CONV_HD void conv_outputs(const double *at, const double *w, double *out /* [R] */)
{
  typedef ConvTile<ND, K> T;
  double acc[T::R];
  for (int r = 0; r < T::R; r ++) acc[r] = 0.0;
  for (int kz = 0; kz < (ND == 2 ? 1 : K); kz ++) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int ky = 0; ky < K; ky ++) {
      const double *row = (const double *)__builtin_assume_aligned(at + (kz * T::PY + ky) * T::PX, 16);
      const double *wr = w + (kz * K + ky) * K;
      double v[K + T::R - 1];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int j = 0; j < K + T::R - 1; j ++) v[j] = row[j];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int kx = 0; kx < K; kx ++) {
        const double wk = wr[kx];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int r = 0; r < T::R; r ++) acc[r] = conv_tap(acc[r], v[r + kx], wk);
      }
    }
  }
  for (int r = 0; r < T::R; r ++) out[r] = acc[r] / (double)T::TAPS;
}

}  // namespace ftkx
