// Spatial Gaussian smoothing of a scalar snapshot on the device: 2D and 3D FP64 convolution with K^nd given weights, out of place; the source
// is FP64 or float32 (widened as the tile is staged: the arithmetic is the same).
//
// Reference (a single-threaded host loop): include/ftk/ndarray/conv.hh, conv2D 11-47 / conv3D 117-163 with padding = ksize / 2, called per
// snapshot by ndarray_stream::modified_callback (include/ftk/ndarray/stream.hh:1597-1603).  The kernel reproduces it bit for bit: per
// output the same products in the same order, each rounded before it is added (-ffp-contract=off), then the division by K^nd -- the
// arithmetic and the tile live in conv_steps.hpp, which tests/hostcheck/conv_host.cpp runs on the CPU.  The fixed order rules out the
// FP64 MFMA (it fuses and reorders) and any split of one output's sum over lanes.
//
// Not a streaming kernel like those of derive_kernels.hip: at K = 5 in 3D an output costs 125 multiplies and 125 adds against 8 bytes in
// and 8 out, so the FP64 VALU is the limit.  One workgroup of 256 lanes stages a tile with its halo in LDS once (outside the array: +0.0),
// then every lane adds up R = 4 neighbouring outputs along x from one row read per (ky, kz): K + 3 LDS reads serve 4 K taps, and the four
// chains are independent, which hides the latency of the dependent adds of one.  The weights are read through a uniform pointer with
// uniform indices: scalar loads into SGPRs, no per-lane traffic.  All addressing of the arrays is size_t; tiles are taken in a
// grid-stride loop, so no extent is limited by the grid.
#include <hip/hip_runtime.h>

#include "conv_steps.hpp"

namespace ftkx {

template <int ND, int K, class SRC>
__global__ __launch_bounds__(kConvThreads) void conv_kernel(const SRC *__restrict__ S, ConvDims d, const double *__restrict__ w, double *__restrict__ out)
{
  typedef ConvTile<ND, K> T;
  __shared__ __attribute__((aligned(16))) double tile[T::DOUBLES];
  const int tid = (int)threadIdx.x;
  int tx, ty, tz;
  conv_lane<ND, K>(tid, &tx, &ty, &tz);
  const size_t ntiles = conv_tiles<ND, K>(d);
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int x0, y0, z0;
    conv_tile_origin<ND, K>(d, t, &x0, &y0, &z0);
    for (int i = tid; i < T::STAGED; i += kConvThreads) conv_stage<ND, K>(S, d, x0, y0, z0, i, tile);
    __syncthreads();
    const int gx = x0 + tx * T::R, gy = y0 + ty;
    for (int oz = tz; oz < T::TZ; oz += T::LZ) {
      const int gz = z0 + oz;
      if (gx >= d.DW || gy >= d.DH || gz >= d.DD) continue;          // (nothing to store; the lane still meets the barrier below)
      double res[T::R];
      conv_outputs<ND, K>(tile + (oz * T::PY + ty) * T::PX + tx * T::R, w, res);
      double *o = out + ((size_t)gz * (size_t)d.DH + (size_t)gy) * (size_t)d.DW + (size_t)gx;
#pragma unroll
      for (int r = 0; r < T::R; r ++) if (gx + r < d.DW) o[r] = res[r];
    }
    __syncthreads();                                                  // the tile is overwritten by the next round
  }
}

template <int ND, int K, class SRC> static void launch_conv_k(const SRC *S, const ConvDims &d, const double *d_weights, double *out, hipStream_t st)
{
  const size_t ntiles = conv_tiles<ND, K>(d);
  const unsigned grid = (unsigned)(ntiles < (size_t)(1u << 30) ? ntiles : (size_t)(1u << 30));
  hipLaunchKernelGGL((conv_kernel<ND, K, SRC>), dim3(grid), dim3(kConvThreads), 0, st, S, d, d_weights, out);
}

// nd 2 or 3 (2D: DD == 1), ksize odd in [1, 9], extents >= 1: checked by the callers (ingest.hip).  d_weights: ksize^nd doubles on the device.
// SRC double or float: a float32 source is widened where the tile is staged, so no widened copy of it is written and read back.
template <class SRC> void launch_conv(int nd, const SRC *S, int DW, int DH, int DD, const double *d_weights, int ksize, double *out, hipStream_t st)
{
  const ConvDims d{DW, DH, nd == 2 ? 1 : DD};
#define CONV_CASE(k) case k: if (nd == 2) launch_conv_k<2, k>(S, d, d_weights, out, st); else launch_conv_k<3, k>(S, d, d_weights, out, st); break
  switch (ksize) { CONV_CASE(1); CONV_CASE(3); CONV_CASE(5); CONV_CASE(7); CONV_CASE(9); default: break; }
#undef CONV_CASE
}
template void launch_conv<double>(int, const double *, int, int, int, const double *, int, double *, hipStream_t);
template void launch_conv<float>(int, const float *, int, int, int, const double *, int, double *, hipStream_t);

}  // namespace ftkx
