// Drives ftkx::critical_point_tracker_regular (include/ftkx_tracker.hh) over one series TWICE with a reset() in between -- reset() has no
// C handle, so tests/test_gpu_parity.py reaches it through this program -- and writes both runs' records.
//   reset_run <in> <out> plain|deferred3|multi
//     in:  int32 nd, nv, DW, DH, DD, DT; then DT snapshots as float64 arrays (nv == 1: the scalar field, otherwise nd components per vertex)
//     out: per run: u64 last scaling factor, u64 n, n records (ftkx_cp_t, ordinal and timestep in the padding word as include/ftkx.h reads them)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <ftkx_tracker.hh>

int main(int argc, char **argv)
{
  if (argc < 4) return 2;
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  int32_t h[6];
  if (fread(h, 4, 6, fp) != 6) return 2;
  const int nd = h[0], nv = h[1], DT = h[5];
  const long long D[3] = {h[2], h[3], h[4]};
  const size_t len = (size_t)D[0] * D[1] * (nd == 3 ? D[2] : 1) * (nv == 1 ? 1 : nd);
  std::vector<std::vector<double>> steps(DT, std::vector<double>(len));
  for (auto &s : steps) if (fread(s.data(), 8, len, fp) != len) { perror("read"); return 2; }
  fclose(fp);
  const std::string mode = argv[3];
  FILE *out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  try {
    // the set-up of tests/gpu_common.py: json_interface.hh:634-656
    std::unique_ptr<ftkx::critical_point_tracker_regular> owner(mode == "multi" ? new ftkx::critical_point_tracker_regular(nd, std::vector<int>{0, 0}, 1)
                                                                                 : new ftkx::critical_point_tracker_regular(nd, 0));
    ftkx::critical_point_tracker_regular &tr = *owner;
    const int margin = nv == 1 ? 2 : 1;
    std::vector<long long> st(nd, margin), sz(nd), zero(nd, 0), all(D, D + nd);
    for (int d = 0; d < nd; d ++) sz[d] = D[d] - margin - 1;
    tr.set_scalar_field_source(nv == 1 ? ftkx::SOURCE_GIVEN : ftkx::SOURCE_NONE);
    tr.set_vector_field_source(nv == 1 ? ftkx::SOURCE_DERIVED : ftkx::SOURCE_GIVEN);
    tr.set_jacobian_field_source(ftkx::SOURCE_DERIVED);
    tr.set_jacobian_symmetric(nv == 1);
    tr.set_domain(ftkx::lattice(st, sz));
    tr.set_array_domain(ftkx::lattice(zero, all));
    tr.initialize();
    if (mode == "deferred3") tr.set_deferred_collection(true, 3);
    for (int run = 0; run < 2; run ++) {
      if (run) tr.reset();
      for (int k = 0; k < DT; k ++) {
        if (nv == 1) tr.push_scalar_field_snapshot(steps[k].data()); else tr.push_vector_field_snapshot(steps[k].data());
        if (k != 0) tr.advance_timestep();
        if (k == DT - 1) tr.update_timestep();
      }
      const uint64_t factor = tr.get_vector_field_scaling_factor();
      const std::vector<ftkx::feature_point_t> pts = tr.get_critical_points();
      const uint64_t n = pts.size();
      fwrite(&factor, 8, 1, out);
      fwrite(&n, 8, 1, out);
      for (const ftkx::feature_point_t &cp : pts) {
        ftkx_cp_t r;
        std::memset(&r, 0, sizeof(r));
        for (int q = 0; q < 3; q ++) { r.x[q] = cp.x[q]; r.scalar[q] = cp.scalar[q]; }
        r.t = cp.t; r.type = cp.type; r.tag = cp.tag;
        const uint32_t aux = ((uint32_t)cp.timestep << 1) | (cp.ordinal ? 1u : 0u);
        std::memcpy((char *)&r + 60, &aux, 4);
        fwrite(&r, sizeof(r), 1, out);
      }
    }
  } catch (const std::exception &e) { fprintf(stderr, "%s\n", e.what()); return 1; }
  fclose(out);
  return 0;
}
