// Perturbation and clamp of a snapshot on the device: what one element becomes, the noise as a function of (seed, snapshot, element), the
// plan of a launch and what one lane of it does, for adjust_kernels.hip.
//
// Reference (one host thread): ndarray_stream::modified_callback (include/ftk/ndarray/stream.hh:1570-1604) runs, between the spatial
// smoothing and the temporal filter, ndarray::perturb(sigma) (include/ftk/ndarray.hh:1331-1341: p[i] += d(gen), std::mt19937 seeded from
// std::random_device, std::normal_distribution<>{0, sigma}) and ndarray::clamp(lo, hi) (ndarray.hh:1344-1350, numeric/clamp.hh:15-20:
// p[i] = std::min(std::max(lo, p[i]), hi)).
//
// The clamp is reproduced bit for bit: std::max(lo, x) is (lo < x) ? x : lo and std::min(m, hi) is (hi < m) ? hi : m -- two compares and
// two selects, NOT fmax / fmin (v_max_f64 / v_min_f64), which answer differently for a NaN and for zeros of unlike sign.  A NaN becomes lo
// (hi where hi < lo), -0.0 under lo = +0.0 becomes +0.0, lo > hi makes everything hi.
//
// The perturbation of the reference differs from run to run, so what is reproduced is its distribution: independent N(0, sigma^2) noise on
// every element of every snapshot, DEFINED here as a pure function of (seed, snapshot number t, element index e) and of nothing else -- not
// the launch's geometry, the path the snapshot took, the device, or which rank or context pushed it:
//   bits     Philox4x32-10, counter (p & 0xffffffff, p >> 32, (uint32)t, 0) with p = e >> 1, key (seed & 0xffffffff, seed >> 32); an even e
//            takes output words 0, 1, an odd e words 2, 3: one call serves two neighbouring elements
//   uniform  k = (w_hi << 20) | (w_lo >> 12), 52 bits, w_hi the first of the element's two words; u = (k + 0.5) * 2^-52, exact, in
//            [2^-53, 1 - 2^-53]  (53 bits would not do: (2^53 - 1) + 0.5 rounds to 2^53 and u would be 1)
//   normal   z = PPND16(u), Wichura's algorithm AS 241 (Applied Statistics 37 (3), 1988): the inverse of the normal CDF
//   result   x + sigma * z: a rounded multiply, then a rounded add (-ffp-contract=off)
// Only integer operations, FP64 + - * /, compares and sqrt are used, all of them correctly rounded on the host and on gfx950
// (-fno-fast-math): the host build of this header is the exact oracle of the kernel.  The C library's log is NOT used -- ocml's and glibc's
// are different functions -- adjust_log below takes its place in the tail branch of PPND16.
//
// The plan.  A lane takes the two elements (2g, 2g + 1) that share a Philox call -- pairs by INDEX, whatever the pointers are.  Where source
// and destination both lie so that such a pair is one aligned access (destination and FP64 source a multiple of 16 bytes, float source a
// multiple of 8), the pair is loaded and stored whole (16 bytes on the FP64 side); otherwise element by element.  No head is peeled: a pair
// shifted by one element would straddle two Philox calls and double the arithmetic of every lane, for accesses that coalesce across the
// wavefront either way.  An odd count leaves one element behind the pairs (the tail, lane 0 of workgroup 0); its call's other half belongs
// to an element that does not exist.  Pairs are dealt to the lanes of a capped grid in a grid-stride loop; every index is size_t.
// Source == destination (T = double) is allowed: a lane has read its pair before it writes it, and no other lane touches it.
//
// Everything here compiles with a plain C++ compiler as well (tests/hostcheck/adjust_host.cpp drives it lane by lane).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define ADJUST_HD __host__ __device__ inline
#else
#define ADJUST_HD inline
#endif

namespace ftkx {

constexpr int kAdjustThreads = 256;
constexpr unsigned kAdjustMaxBlocks = 2048;     // the grid's cap (8 workgroups for each of 256 CUs); the rest is taken by the grid-stride loop

struct AdjustArgs {
  double sigma;                  // PERTURB: the noise's standard deviation
  unsigned long long seed;
  int t;                         // the snapshot's number
  double lo, hi;                 // CLAMP
};

// ---- bits --------------------------------------------------------------------------------------------------------------------------------
ADJUST_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 10; r ++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of the call that elements 2p and 2p + 1 of snapshot t share
ADJUST_HD void adjust_words(unsigned long long seed, int t, size_t p, uint32_t w[4])
{
  const uint32_t ctr[4] = {(uint32_t)((uint64_t)p & 0xffffffffu), (uint32_t)((uint64_t)p >> 32), (uint32_t)t, 0u};
  const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
  philox4x32_10(ctr, key, w);
}

// ---- uniform -----------------------------------------------------------------------------------------------------------------------------
ADJUST_HD double adjust_uniform(uint32_t w_hi, uint32_t w_lo)
{
  const uint64_t k = ((uint64_t)w_hi << 20) | (uint64_t)(w_lo >> 12);
  return ((double)k + 0.5) * 2.220446049250313080847263336181640625e-16;      // 2^-52
}

// ---- log ---------------------------------------------------------------------------------------------------------------------------------
// The natural logarithm of a positive, finite, NORMAL double (PPND16 hands it min(u, 1 - u) >= 2^-53), from + - * / alone: x = m * 2^k with
// m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s) = 2 s + 2 s z (1/3 + z/5 + ... + z^11 / 25) with s = (m - 1) / (m + 1), z = s * s <= 0.0295
// (the first term left out is below 2e-20 of the sum), plus k * ln 2 in two parts, the high one with 21 trailing zero bits so that
// k * ln2_hi is exact.  Within about an ulp of the true value; the same bits wherever + - * / are correctly rounded.
ADJUST_HD double adjust_log(double x)
{
  uint64_t b;
  memcpy(&b, &x, 8);
  int k = (int)((b >> 52) & 0x7ff) - 1023;
  b = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;      // m in [1, 2)
  if ((b & 0x000fffffffffffffull) >= 0x0006a09e667f3bcdull) { b -= 0x0010000000000000ull; k ++; }      // m >= sqrt(2): halved
  double m;
  memcpy(&m, &b, 8);
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double q = 1.0 / 25.0;
  q = q * z + 1.0 / 23.0;
  q = q * z + 1.0 / 21.0;
  q = q * z + 1.0 / 19.0;
  q = q * z + 1.0 / 17.0;
  q = q * z + 1.0 / 15.0;
  q = q * z + 1.0 / 13.0;
  q = q * z + 1.0 / 11.0;
  q = q * z + 1.0 / 9.0;
  q = q * z + 1.0 / 7.0;
  q = q * z + 1.0 / 5.0;
  q = q * z + 1.0 / 3.0;
  const double s2 = s + s;
  const double lm = s2 + (s2 * z) * q;
  const double dk = (double)k;
  return dk * 6.93147180369123816490e-01 + (lm + dk * 1.90821492927058770002e-10);
}

// ---- normal ------------------------------------------------------------------------------------------------------------------------------
// AS 241, PPND16: u in (0, 1) -> z with Phi(z) = u, to about 1e-16.  The coefficients and the order of the operations are the published
// ones (Python's statistics.NormalDist.inv_cdf is the same algorithm over the C library's log).
ADJUST_HD double adjust_ppnd16(double u)
{
  const double q = u - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                           1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                           5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r + 4.2313330701600911252e+1) * r + 1.0);
    return num / den;
  }
  double r = q <= 0.0 ? u : 1.0 - u;
  r = sqrt(-adjust_log(r));
  double num, den;
  if (r <= 5.0) {
    r = r - 1.6;
    num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r + 1.27045825245236838258e+0) * r +
              3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
              6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r + 2.05319162663775882187e+0) * r + 1.0);
  } else {
    r = r - 5.0;
    num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
              2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
    den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
              1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r + 5.99832206555887937690e-1) * r + 1.0);
  }
  const double x = num / den;
  return q < 0.0 ? -x : x;
}

// the noise of one element, before sigma: its two words -> N(0, 1)
ADJUST_HD double adjust_normal(uint32_t w_hi, uint32_t w_lo) { return adjust_ppnd16(adjust_uniform(w_hi, w_lo)); }

// ---- one element -------------------------------------------------------------------------------------------------------------------------
ADJUST_HD double adjust_clamp(double x, double lo, double hi)
{
  const double m = (lo < x) ? x : lo;      // std::max(lo, x)
  return (hi < m) ? hi : m;                // std::min(m, hi)
}

// x (widened already) -> perturbed, then clamped; (w_hi, w_lo): the element's words (unused without PERTURB)
template <bool PERTURB, bool CLAMP> ADJUST_HD double adjust_value(double x, uint32_t w_hi, uint32_t w_lo, const AdjustArgs &a)
{
  if (PERTURB) { const double d = a.sigma * adjust_normal(w_hi, w_lo); x = x + d; }
  if (CLAMP) x = adjust_clamp(x, a.lo, a.hi);
  return x;
}

// element e of snapshot a.t, by the definition alone (what every path must give)
template <class T, bool PERTURB, bool CLAMP> ADJUST_HD double adjust_one(T x, size_t e, const AdjustArgs &a)
{
  uint32_t w[4] = {0, 0, 0, 0};
  if (PERTURB) adjust_words(a.seed, a.t, e >> 1, w);
  return (e & 1) ? adjust_value<PERTURB, CLAMP>(static_cast<double>(x), w[2], w[3], a) : adjust_value<PERTURB, CLAMP>(static_cast<double>(x), w[0], w[1], a);
}

// ---- the plan of a launch ------------------------------------------------------------------------------------------------------------------
struct AdjustPlan {
  size_t count;      // elements in all
  size_t npair;      // pairs (2g, 2g + 1), g < npair; an odd count's last element is the tail
  bool vec;          // a pair is one aligned access on either side
};

// src: a multiple of sizeof(T) bytes, dst: a multiple of 8; src == dst or no overlap (checked by the callers, ingest.hip)
template <class T> inline AdjustPlan adjust_plan(const T *src, size_t count, const double *dst)
{
  AdjustPlan p;
  p.count = count;
  p.npair = count / 2;
  p.vec = (((size_t)src) & (2 * sizeof(T) - 1)) == 0 && (((size_t)dst) & 15) == 0;
  return p;
}

// how many workgroups the plan is launched with
inline unsigned adjust_blocks(const AdjustPlan &p)
{
  const size_t want = (p.npair + (size_t)kAdjustThreads - 1) / (size_t)kAdjustThreads;
  return want < 1 ? 1u : want > (size_t)kAdjustMaxBlocks ? kAdjustMaxBlocks : (unsigned)want;
}

ADJUST_HD void adjust_load_pair(const double *src, bool vec, double &x0, double &x1)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (vec) { const double2 v = *reinterpret_cast<const double2 *>(src); x0 = v.x; x1 = v.y; return; }
#endif
  x0 = src[0]; x1 = src[1];
}

ADJUST_HD void adjust_load_pair(const float *src, bool vec, double &x0, double &x1)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (vec) { const float2 v = *reinterpret_cast<const float2 *>(src); x0 = static_cast<double>(v.x); x1 = static_cast<double>(v.y); return; }
#endif
  x0 = static_cast<double>(src[0]); x1 = static_cast<double>(src[1]);
}

ADJUST_HD void adjust_store_pair(double *dst, bool vec, double r0, double r1)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (vec) { *reinterpret_cast<double2 *>(dst) = make_double2(r0, r1); return; }
#endif
  dst[0] = r0; dst[1] = r1;
}

// what lane `tid` of workgroup `block` does
template <class T, bool PERTURB, bool CLAMP>
ADJUST_HD void adjust_lane(const T *src, const AdjustPlan &p, const AdjustArgs &a, double *dst, size_t block, size_t nblocks, int tid)
{
  const size_t stride = nblocks * (size_t)kAdjustThreads;
  for (size_t g = block * (size_t)kAdjustThreads + (size_t)tid; g < p.npair; g += stride) {
    double x0, x1;
    adjust_load_pair(src + 2 * g, p.vec, x0, x1);
    uint32_t w[4] = {0, 0, 0, 0};
    if (PERTURB) adjust_words(a.seed, a.t, g, w);
    const double r0 = adjust_value<PERTURB, CLAMP>(x0, w[0], w[1], a), r1 = adjust_value<PERTURB, CLAMP>(x1, w[2], w[3], a);
    adjust_store_pair(dst + 2 * g, p.vec, r0, r1);
  }
  if (block == 0 && tid == 0 && (p.count & 1)) { const size_t e = p.count - 1; dst[e] = adjust_one<T, PERTURB, CLAMP>(src[e], e, a); }
}

}  // namespace ftkx
