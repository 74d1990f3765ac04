// Which mask kernel takes a mesh, with what launch geometry, and what summary geometry it writes: ONE pure function of the mesh's shape and the
// test hooks, free of the device.  launch_masks (mask_kernels.hip) launches what plan_masks returns; march2_supported, masks_have_summary and
// mask_summary_rows -- what fill_mesh, the pre-pass, the cull, the halo and the series pass ask -- read the same plan, so the summaries the cull
// reads are by construction the ones the kernel wrote.  tests/test_mask_plan.py drives it without a GPU through tests/hostcheck.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace ftkx {

// The z extent of a slice in PIECES of unequal length, the same for every tile column, pieces in order of decreasing length.  The
// hardware hands workgroups out in order of their index as slots free up -- a queue --, so the long pieces (up to half a column) go out
// first and the launch ends on pieces of a few planes: the device stays full until a few microseconds before the end whatever the size
// of the series (equal chunks of 32 planes: 256^3 x 16 is 5.3 rounds of workgroups, a 512^3 slice on its own 2.7).  (Persistent
// workgroups pulling such pieces from a queue of their own were built and measured: the loop state costs the kernel 36 more SGPR spills
// and 12 VGPRs of scratch at three wavefronts per SIMD -- 7.6 ms against 5.7 on 512^3 x 32.)
// Every piece starts by fetching two planes that its predecessor in z fetches as well (its last plane and that plane's halo): 46 of 512
// planes on a 512^3 slice.  Whether the second fetch is served by a cache is a matter of WHERE and WHEN the two pieces run, that is of
// the order in which blockIdx.z enumerates (slice, piece) -- zplan_decode below, three orders:
//   piece by piece over all slices (njobs > 0): bz = piece * njobs + slice.  A column's next piece follows one round of njobs x columns
//     workgroups behind; where that round is a whole number of rounds of 8 placement groups (remap_block), on the same XCD;
//   slice by slice (njobs < 0, sgroup == 0): bz = slice * npieces + piece, the pieces of a slice back to back: neighbouring pieces of
//     a slice run at the same time;
//   slices in groups of about `sgroup`, piece by piece inside a group (njobs < 0, sgroup >= 1): bz enumerates (group, piece, slice
//     in the group), the slice fastest.  A column's next piece follows its predecessor by one round of (slices of the group) x columns
//     workgroups.  Groups are as even as possible (32 slices at a cap of 6: 6, 6, 5, 5, 5, 5 -- a short last group would put its
//     columns' pieces several rounds apart).  sgroup == 1 is slice by slice, sgroup >= |njobs| piece by piece.
// What was measured, and which order a launch gets: plan_masks, "Order of the workgroups".
struct ZPlan {
  unsigned npieces;
  unsigned z0[47], len[47];
  unsigned sgroup;      // slices per group of the third order; 0: one of the first two
};

#if defined(__HIPCC__)
#define FTKX_PLAN_HD __host__ __device__
#else
#define FTKX_PLAN_HD
#endif

// blockIdx.z (after remap_block) -> the job and the piece of a tile column, for all three orders: the one place that knows them (the
// kernel and tests/test_mask_order.py both call it).  njobs as MaskPlan::njobs carries it: negative unless piece by piece over all slices.
struct ZWhere { unsigned job, piece; };
FTKX_PLAN_HD inline ZWhere zplan_decode(const ZPlan &plan, int njobs, unsigned bz)
{
  ZWhere w;
  if (njobs >= 0) { w.piece = bz / (unsigned)njobs; w.job = bz - w.piece * (unsigned)njobs; return w; }
  const unsigned nj = (unsigned)-njobs, t = bz / plan.npieces;       // t: whole slices' worth of workgroups in front of this one
  if (plan.sgroup == 0) { w.piece = bz - t * plan.npieces; w.job = t; return w; }
  // ngroups groups, the first `extra` of them of small + 1 slices, the others of small
  const unsigned ngroups = (nj + plan.sgroup - 1) / plan.sgroup, small = nj / ngroups, extra = nj - small * ngroups, head = extra * (small + 1);
  const unsigned size = t < head ? small + 1 : small;
  const unsigned first = t < head ? t / size * size : head + (t - head) / size * size;      // the group's first slice
  const unsigned r = bz - first * plan.npieces;
  w.piece = r / size; w.job = first + (r - w.piece * size);
  return w;
}

// The test hooks of the mask kernels, parsed once per plan -- still at every use: tests switch them inside one process.
// FTKX_MASK_PLAN="name=value,...": launch geometry; FTKX_U_ROWS: rows per summary byte (1 / 4 / 16; -1: no summaries, the one-level cull).
constexpr long kHookUnset = -0x7fffffffL;
struct MaskHooks {
  long swizzle = kHookUnset, yg = kHookUnset, zchunk = kHookUnset, lmin = kHookUnset, lcap = kHookUnset, order = kHookUnset, sgroup = kHookUnset, rows = kHookUnset, lean = kHookUnset;
  long u_rows = 0;                    // (0: unset)
};
inline long hook_or(long v, long dflt) { return v == kHookUnset ? dflt : v; }

inline MaskHooks parse_mask_hooks(const char *plan, const char *u_rows)
{
  MaskHooks h;
  const struct { const char *name; long MaskHooks::*knob; } knobs[] = {{"swizzle", &MaskHooks::swizzle}, {"yg", &MaskHooks::yg}, {"zchunk", &MaskHooks::zchunk},
    {"lmin", &MaskHooks::lmin}, {"lcap", &MaskHooks::lcap}, {"order", &MaskHooks::order}, {"sgroup", &MaskHooks::sgroup}, {"rows", &MaskHooks::rows}, {"lean", &MaskHooks::lean}};
  for (const char *p = plan ? plan : ""; *p;) {
    while (*p == ',' || *p == ' ') p ++;
    for (const auto &k : knobs) {
      const size_t n = strlen(k.name);
      if (!strncmp(p, k.name, n) && p[n] == '=' && h.*k.knob == kHookUnset) h.*k.knob = atol(p + n + 1);      // (a knob named twice: the first one counts)
    }
    while (*p && *p != ',') p ++;
  }
  if (u_rows) h.u_rows = atoi(u_rows);
  return h;
}
inline MaskHooks read_mask_hooks() { return parse_mask_hooks(getenv("FTKX_MASK_PLAN"), getenv("FTKX_U_ROWS")); }

// what the plan needs of a Mesh (sweep_params.hpp)
struct MaskShape { int nd, scalar_mode, ext_sz[3], mask_pitch; };

// The kernel families; also the index of the launch counters and their names (mask_kernels.hip: mask_kernel_launches).
enum MaskFamily { MASK_MARCH6 = 0 /* 3D scalar */, MASK_MARCH4 = 1 /* 2D scalar */, MASK_ROWS2 = 2 /* 2D scalar, long rows */,
                  MASK_REDUCE = 3 /* mask_march4_kernel<reduce>: the exact stand-alone reduction */, MASK_VEC2 = 4 /* vector input, block summaries */,
                  MASK_VEC = 5 /* vector input */, MASK_GENERIC = 6, MASK_FAMILIES = 7 };
constexpr unsigned kMaskThreads = 256;      // (= kThreads of sweep_device.hpp)

struct MaskPlan {
  MaskFamily family;
  const char *name;           // the instantiation as rocprofv3 prints it
  bool march2;                // can the 128-column marching kernels (which also carry the exact pre-pass reduction) walk this mesh?
  bool has_summary;           // does launch_masks produce the summaries for this mesh?  (the 128-column marching kernels and the fast vector kernels do)
  int u_rows;                 // rows a summary byte stands for (Mesh::u_rows)
  unsigned grid[3], block, lds_bytes;
  // kernel arguments (0 where the family's kernel takes no such argument): the packed placement word (remap_block), planes per chunk (mask_march4_kernel),
  // groups of 8 rows a wavefront marches (mask_rows2_kernel), the job count -- negative: slice by slice, or in groups of z.sgroup slices (mask_march6_kernel) --, the pieces of a column
  int swizzle, zchunk, groups, njobs;
  ZPlan z;
};

inline MaskPlan plan_masks(const MaskShape &s, const MaskHooks &h, int njobs, bool reduce)
{
  MaskPlan p = MaskPlan();
  const int DW = s.ext_sz[0], DH = s.ext_sz[1], DD = s.nd == 3 ? s.ext_sz[2] : 1;
  const size_t nrows = (size_t)DH * (size_t)DD;
  p.march2 = s.scalar_mode && (DW % 2) == 0 && DW >= 2 && (size_t)DW * nrows * 8 < (1ull << 32);
  // does this mesh take the fast vector-input kernel?
  const bool vec_fast = !s.scalar_mode && DW >= 8 && (DW % 8) == 0;
  // ... its form with block summaries (mask_vec2_kernel)?  Rows of at least 64 groups, byte offsets that fit 31 bits.  FTKX_MASK_PLAN lean=0: never
  const bool vec_lean = vec_fast && DW >= 256 && hook_or(h.lean, 1) != 0 && (size_t)DW * nrows * 8 * (size_t)s.nd < (1ull << 31) && (size_t)s.mask_pitch * nrows < (1ull << 31);
  p.has_summary = h.u_rows >= 0 && (s.scalar_mode ? p.march2 && (DW % 8) == 0 : vec_fast);      // (FTKX_U_ROWS=-1: no summaries at all, the one-level cull)
  // Rows a summary byte stands for.  mask_march6_kernel with four rows per wavefront writes ONE byte per 8 x 4 block of vertices
  // (aligned in y): a quarter of the summary bytes to write (what they cost: DESIGN.md) and for the coarse cull to read.  Everything
  // else writes one byte per word of 8.
  if (!p.has_summary || h.u_rows == 1) p.u_rows = 1;
  else if (!s.scalar_mode) p.u_rows = vec_lean ? 4 : 1;            // mask_vec2_kernel / mask_vec_kernel
  else if (s.nd == 3) p.u_rows = h.u_rows == 4 ? 4 : 16;           // mask_march6_kernel: the workgroup's sixteen rows (FTKX_U_ROWS=4: a wavefront's four)
  else p.u_rows = 4;                                               // mask_march4_kernel<2, ...>: a wavefront's rows in blocks of four
  p.njobs = njobs;
  p.block = kMaskThreads;
  p.grid[1] = p.grid[2] = 1;
  if (p.march2) {
    // scalar slices with an even row length below 4 GiB: the marching kernels on 128-column, line-aligned tiles
    int swizzle = 8;   // grouped placement -- the x tiles of some row groups on one XCD -- cuts the fabric reads from 47.7 to 41.4 GB per 512^3 x 32 launch
    // 2D: the rows of a wavefront's block that no other wavefront reads (all but its first and last two) are loaded non-temporally -- they are
    // read once, and keeping them out of the caches leaves the halo rows there for the neighbours: woven 1024^2 x 64 0.115 -> 0.102 ms (all
    // loads non-temporal: 0.106; 3D, where the planes are re-read by the z march: 256^3 x 16 -1 %, 512^3 x 32 +1.3 %: left as it is.  The
    // vector-input kernel, whose every value is read once, does NOT like non-temporal loads: double_gyre 0.73 -> 1.30 ms)
    if (s.nd == 2) swizzle |= 16;
    swizzle = (int)hook_or(h.swizzle, swizzle);
    int zchunk = 32;
    const bool zforced = hook_or(h.zchunk, 0) > 0;
    if (zforced) zchunk = (int)h.zchunk;
    // the height of a placement group in workgroups (FTKX_MASK_PLAN yg=n), packed into the placement word next to the mode bits
    auto yg_of = [&](int dflt) { const long v = h.yg == kHookUnset ? dflt : h.yg > 0 ? h.yg : 1; return (int)(v > 255 ? 255 : v); };
    auto grouped = [](int sw, int yg) { return (sw & 0xff) | (yg << 8); };
    p.grid[0] = (unsigned)((DW + 127) / 128);
    if (s.nd == 3 && !reduce) {
      // 3D: mask_march6_kernel -- 128 x 16 tiles as four wavefronts of 4 rows that all load (LDS-DMA) and classify, TWO row slots in
      // LDS (37 KB: three workgroups = twelve wavefronts per CU, which its 164 VGPRs allow), one barrier per plane; grouped placement:
      // 16 row groups (all of a 256^2 plane's, half of a 512^2 plane's tiles) of one piece of planes share an XCD's L2 (4: +3.5 %, 8: +0.5 %)
      const int yg_want = yg_of(16);
      // The pieces a tile column is marched in (ZPlan): at most 24 planes, at most half of what is left of the column, at least 6,
      // multiples of 3 (the march is unrolled three planes deep), handed out longest first.  Measured, not derived (tools/ab_mask.py,
      // interleaved on one box): against equal chunks of 32 planes 256^3 x 16 0.418 -> 0.405 ms, one 512^3 slice 0.206 -> 0.197, four
      // 0.756 -> 0.748, 512^3 x 32 5.72 -> 5.69.  LONGER marches are slower although they pay fewer start-up planes (caps of 28 / 32 / 48:
      // +9 / +5 / +1..2 % on 512^3 x 32; half columns +3.7 %: the tiles of a group drift apart and stop sharing their halo rows in the L2),
      // equal chunks swing by +-3 % with their length (24: 5.89, 27: 5.68, 30: 5.98, 32: 5.72, 33: 5.84 ms -- what is left over at a
      // column's top decides).
      // Order of the workgroups (ZPlan).  Where a slice alone does not fill the device: piece by piece over all slices (256^3 x 16: 0.374
      // against 0.388 ms slice by slice; a round is 512 workgroups = 8 placement groups, a column's next piece runs one round behind
      // its predecessor on the same XCD and finds the two start-up planes in that L2: 1.062 x the algorithmic bytes at the fabric).
      // Where a slice alone fills the device (768 workgroups, three per CU): piece by piece over all 32 slices of 512^3 x 32 is a round of
      // 4 096 workgroups -- 1.5 GB between a plane's two fetches, 5.75 ms --, slice by slice six neighbouring pieces start together and
      // the later one of a pair wants the planes ~45 us before the earlier one fetches them (5.45 ms, 1.119 x).  In between: slices in
      // groups of S, piece by piece inside a group.  Interleaved in one process, 15 rounds, 512^3 x 32 (tools/ab_mask.py; slice by slice
      // twice: 5.449 / 5.443): S = 2 5.403, S = 4 5.309, S = 6 5.352, S = 8 5.361 ms.  S = 4 is the 256^3 x 16 geometry -- 512 workgroups a
      // round, a whole number of rounds of 8 placement groups, the device's 768 not exceeded -- and that is the rule below; four 512^3
      // slices (one group: piece by piece) 0.704 against 0.709 / 0.703, inside that run's noise.  One slice per launch stays as it was.
      // FTKX_MASK_PLAN (test hooks): zchunk=n: equal chunks of n planes; lcap / lmin: the two bounds; order=0: slice by slice, order=1: piece
      // by piece over all slices, order=2: groups of slices at any shape; sgroup=n: the slices of a group, clamped to [1, njobs]
      int lmin = 6, lcap = 24;
      if (hook_or(h.lmin, 0) >= 1) lmin = (int)h.lmin;
      if (hook_or(h.lcap, 0) >= 1) lcap = (int)h.lcap;
      if (lcap < lmin) lcap = lmin;
      std::vector<int> lens;
      int rem = DD;
      if (zforced) while (rem > 0) { const int l = rem < zchunk ? rem : zchunk; lens.push_back(l); rem -= l; }
      while (rem > 0) {
        int l = (rem + 1) / 2;
        if (l > lcap) l = lcap;
        if (l < lmin) l = lmin;
        if (l >= 3) l -= l % 3;      // (the march is unrolled three planes deep: a length that is no multiple of 3 pays for up to two empty steps)
        if (l > rem || rem - l < (lmin + 1) / 2) l = rem;
        lens.push_back(l); rem -= l;
      }
      while (lens.size() > 47) { const int l = lens.back(); lens.pop_back(); lens.back() += l; }      // (more pieces than the table holds: merged from the end)
      std::stable_sort(lens.begin(), lens.end(), [](int a, int b) { return a > b; });
      p.z.npieces = (unsigned)lens.size();
      int z = 0;
      for (size_t i = 0; i < lens.size(); i ++) { p.z.z0[i] = (unsigned)z; p.z.len[i] = (unsigned)lens[i]; z += lens[i]; }
      constexpr int NS6 = 2, CY6 = 4, RY6 = 4, rows = CY6 * RY6;      // (the instantiation launch_masks launches)
      p.family = MASK_MARCH6; p.name = "ftkx::mask_march6_kernel<2, 4, 4, false>";
      p.block = 64u * CY6;
      p.grid[1] = (unsigned)((DH + rows - 1) / rows); p.grid[2] = p.z.npieces * (unsigned)njobs;
      p.swizzle = swizzle;
      // grouped placement needs a y extent that is a multiple of the group height: pad it (workgroups past the last row leave at once)
      if (swizzle & 8) { int yg = yg_want; if (yg > (int)p.grid[1]) yg = (int)p.grid[1]; p.grid[1] = (p.grid[1] + (unsigned)yg - 1) / (unsigned)yg * (unsigned)yg; p.swizzle = grouped(swizzle, yg); }
      p.lds_bytes = (unsigned)NS6 * (unsigned)(rows + 2) * 1024u + (unsigned)(NS6 + 1) * 256u + 128u;   // row slots, edge ring, the summaries' exchange
      bool slice_major = (size_t)p.grid[0] * ((DH + rows - 1) / rows) * p.z.npieces >= 768;      // a slice alone fills the device (three workgroups per CU)
      bool grouped_slices = slice_major && njobs > 1;
      if (h.order != kHookUnset) { slice_major = h.order == 0 || h.order == 2; grouped_slices = h.order == 2; }
      if (slice_major) p.njobs = -njobs;
      if (grouped_slices) {
        // the largest group whose round the device holds (768 workgroups) and, with grouped placement, is whole rounds of 8 placement
        // groups -- a column's next piece then lands on its predecessor's XCD; where there is none, the largest the device holds
        const unsigned per_piece = p.grid[0] * p.grid[1], pgroups = (p.swizzle & 8) ? p.grid[1] / (((unsigned)p.swizzle >> 8) & 0xffu) : 0;
        unsigned fits = 768 / per_piece, sg = 0;
        if (fits > (unsigned)njobs) fits = (unsigned)njobs;
        for (unsigned c = fits; c >= 1 && !sg; c --) if (pgroups && (c * pgroups) % 8 == 0) sg = c;
        if (!sg) sg = fits >= 1 ? fits : 1;
        if (h.sgroup != kHookUnset) sg = (unsigned)(h.sgroup < 1 ? 1 : h.sgroup > njobs ? njobs : h.sgroup);
        p.z.sgroup = sg;
      }
      return p;
    }
    // 2D, and the exact stand-alone reduction (ftkx_slice_resolution) of either dimension: mask_march4_kernel -- every wavefront loads
    // its rows into registers (4 wavefronts of 8 rows in 2D, of 4 rows marching along z in 3D)
    const int RY = (s.nd == 3) ? 4 : 8, wpb = 4;
    p.block = (unsigned)(64 * wpb);
    // mask_rows2_kernel: a wavefront marches down `groups` groups of 8 rows (FTKX_MASK_PLAN rows=n, test hook; rows=0: the kernel below).
    // Measured (tools/ab_mask.py, interleaved on one box, 4 groups against the kernel below): 4096^2 x 16 0.428 -> 0.384 ms, 2048^2 x 64
    // 0.412 -> 0.397 (8 groups: 0.390), but 1024^2 x 64 0.096 -> 0.109 and 1024^2 x 256 0.379 -> 0.399: with rows of 8 KB the short
    // wavefronts of the kernel below, whose neighbours in x run together, read whole rows; taken for rows of 32 KB and more
    int groups = 0;
    if (s.nd == 2 && !reduce) {
      groups = (int)hook_or(h.rows, (DW >= 4096 && DH >= 512) ? 4 : 0);
      if (groups > 64) groups = 64;
    }
    const int wg_rows = groups >= 1 ? wpb * RY * groups : wpb * RY;
    p.grid[1] = (unsigned)((DH + wg_rows - 1) / wg_rows);
    if (swizzle & 8) {     // (the group height must divide the grid's y extent)
      int yg = yg_of(4);
      while (yg > 1 && p.grid[1] % (unsigned)yg) yg --;
      swizzle = grouped(swizzle, yg);
    }
    p.swizzle = swizzle;
    if (groups >= 1) { p.family = MASK_ROWS2; p.name = "ftkx::mask_rows2_kernel<8>"; p.groups = groups; p.grid[2] = (unsigned)njobs; return p; }
    const int nzc = s.nd == 3 ? (DD + zchunk - 1) / zchunk : 1;
    p.grid[2] = (unsigned)(nzc * njobs);
    p.zchunk = zchunk;
    p.family = reduce ? MASK_REDUCE : MASK_MARCH4;
    p.name = !reduce ? "ftkx::mask_march4_kernel<2, false, 1, 8>" : s.nd == 2 ? "ftkx::mask_march4_kernel<2, true, 1, 8>" : "ftkx::mask_march4_kernel<3, true, 1, 4>";
    return p;
  }
  p.grid[1] = (unsigned)njobs;
  if (vec_fast) {
    const size_t groups = (size_t)(DW / 4) * nrows;
    size_t bx = (groups + kMaskThreads - 1) / kMaskThreads;
    if (bx > 2048) bx = 2048;               // grid-stride the rest: 8 workgroups per CU per job
    // ... and at least four groups per lane where the slice has them: the per-wavefront fixed costs (index arithmetic, the two
    // reduction atomics) are paid per 16 KB instead of per 4 KB (double_gyre 2048 x 1024 x 128: 0.795 -> 0.746 ms)
    while (bx > 256 && bx * kMaskThreads * 4 > groups) bx /= 2;
    // mask_vec2_kernel (units of 4 rows x 64 groups, one summary byte per 8 x 4 block): where the mesh carries block summaries
    if (p.u_rows == 4) {
      const size_t units = (size_t)((DW / 4 + 63) / 64) * ((DH + 3) / 4) * (size_t)DD;
      bx = (units + 7) / 8;                 // two units (32 KB) per wavefront where the slice has them (four: +1.3 %, one: +0.3 % on double_gyre 2048 x 1024 x 128)
      if (bx > 2048) bx = 2048;
    }
    p.grid[0] = (unsigned)bx;
    p.family = p.u_rows == 4 ? MASK_VEC2 : MASK_VEC;
    p.name = p.u_rows == 4 ? (s.nd == 2 ? "ftkx::mask_vec2_kernel<2>" : "ftkx::mask_vec2_kernel<3>") : (s.nd == 2 ? "ftkx::mask_vec_kernel<2>" : "ftkx::mask_vec_kernel<3>");
    return p;
  }
  // the one generic form (odd row lengths, slices of 4 GiB and more, vector rows that are not a multiple of 8): one lane per mask byte
  const size_t n = (size_t)s.mask_pitch * nrows;
  size_t bx = (n + kMaskThreads - 1) / kMaskThreads;
  if (bx > 4096) bx = 4096;                 // grid-stride the rest
  p.grid[0] = (unsigned)bx;
  p.family = MASK_GENERIC; p.name = s.nd == 2 ? "ftkx::mask_kernel<2>" : "ftkx::mask_kernel<3>";
  return p;
}

}  // namespace ftkx
