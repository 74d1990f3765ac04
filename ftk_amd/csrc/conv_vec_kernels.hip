// Spatial Gaussian smoothing of a vector snapshot on the device, every component as the scalar field it is (conv_vec_steps.hpp has the rule):
// one launch for the whole array, interleaved FP64 out; the source is an interleaved array or one plane per component, FP64 or float32.
//
// Per component the kernel IS conv_kernel (conv_kernels.hip): the same tile, lanes, row reads and chains -- conv_steps.hpp's functions, used as
// they are -- so its output is that kernel's per plane, byte for byte.  What differs is the walk: a workgroup takes ALL nc components of its
// tile, one after the other through one staged plane (LDS and workgroups per CU of the scalar kernel), and only then moves on.  The nc passes
// over an interleaved tile ask for the same cache lines within one workgroup's lifetime, nc - 1 of them from the cache; the nc stores of a
// lane to one line (stride nc doubles, one component each) meet in the L2 before the line leaves.  Each byte moves to and from HBM once.
//
// The other admissible shapes were not taken (NOTES, "Vector smoothing"): results held in registers until all components are through and
// stored as nc * R contiguous doubles need the component loop unrolled around conv_outputs, which costs 3D K = 3 all 256 VGPRs plus scratch
// and 2D K = 5 three of its five waves per SIMD; nc staged planes cost 3D its three workgroups per CU.
//
// All addressing of the arrays is size_t; tiles are taken in a grid-stride loop; a lane whose outputs lie outside still meets every barrier.
#include <hip/hip_runtime.h>

#include "conv_vec_steps.hpp"

namespace ftkx {

template <int ND, int K, class SRC>
__global__ __launch_bounds__(kConvThreads) void conv_vec_kernel(ConvVecSource<SRC> src, ConvDims d, const double *__restrict__ w, double *__restrict__ out)
{
  typedef ConvTile<ND, K> T;
  constexpr int NC = ConvVecTile<ND, K>::NC;
  __shared__ __attribute__((aligned(16))) double tile[T::DOUBLES];
  static_assert(sizeof(tile) == (size_t)ConvVecTile<ND, K>::LDS_BYTES, "the LDS conv_vec_steps.hpp states");
  const int tid = (int)threadIdx.x;
  int tx, ty, tz;
  conv_lane<ND, K>(tid, &tx, &ty, &tz);
  const size_t ntiles = conv_tiles<ND, K>(d);
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int x0, y0, z0;
    conv_tile_origin<ND, K>(d, t, &x0, &y0, &z0);
    const int gx = x0 + tx * T::R, gy = y0 + ty;
    for (int c = 0; c < NC; c ++) {
      const SRC *base = conv_vec_base(src, c);
      for (int i = tid; i < T::STAGED; i += kConvThreads) conv_vec_stage<ND, K>(base, src.stride, d, x0, y0, z0, i, tile);
      __syncthreads();
      for (int oz = tz; oz < T::TZ; oz += T::LZ) {
        const int gz = z0 + oz;
        if (gx >= d.DW || gy >= d.DH || gz >= d.DD) continue;          // (nothing to store; the lane still meets the barrier below)
        double res[T::R];
        conv_outputs<ND, K>(tile + (oz * T::PY + ty) * T::PX + tx * T::R, w, res);
        double *o = out + conv_vec_out_index(d, NC, c, gx, gy, gz);
#pragma unroll
        for (int r = 0; r < T::R; r ++) if (gx + r < d.DW) o[(size_t)r * NC] = res[r];
      }
      __syncthreads();                                                  // the tile is overwritten by the next component, or the next round
    }
  }
}

template <int ND, int K, class SRC> static void launch_conv_vec_k(const ConvVecSource<SRC> &src, const ConvDims &d, const double *d_weights, double *out, hipStream_t st)
{
  const size_t ntiles = conv_tiles<ND, K>(d);
  const unsigned grid = (unsigned)(ntiles < (size_t)(1u << 30) ? ntiles : (size_t)(1u << 30));
  hipLaunchKernelGGL((conv_vec_kernel<ND, K, SRC>), dim3(grid), dim3(kConvThreads), 0, st, src, d, d_weights, out);
}

// nd 2 or 3 (2D: DD == 1), nd components, ksize odd in [1, 9], extents >= 1, no source overlapping out: checked by the callers (ingest.hip).
// d_weights: ksize^nd doubles on the device; out: nd * DW * DH * DD doubles, interleaved.
template <class SRC> void launch_conv_vec(int nd, const ConvVecSource<SRC> &src, int DW, int DH, int DD, const double *d_weights, int ksize, double *out, hipStream_t st)
{
  const ConvDims d{DW, DH, nd == 2 ? 1 : DD};
#define CONV_CASE(k) case k: if (nd == 2) launch_conv_vec_k<2, k>(src, d, d_weights, out, st); else launch_conv_vec_k<3, k>(src, d, d_weights, out, st); break
  switch (ksize) { CONV_CASE(1); CONV_CASE(3); CONV_CASE(5); CONV_CASE(7); CONV_CASE(9); default: break; }
#undef CONV_CASE
}
template void launch_conv_vec<double>(int, const ConvVecSource<double> &, int, int, int, const double *, int, double *, hipStream_t);
template void launch_conv_vec<float>(int, const ConvVecSource<float> &, int, int, int, const double *, int, double *, hipStream_t);

}  // namespace ftkx
