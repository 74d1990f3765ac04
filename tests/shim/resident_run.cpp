// Runs ftkx::resident_sweep (include/ftkx_shim.hh), instantiated with this repo's own lattice / record types, through a script of
// commands and writes what every sweep returned: tests/test_gpu_shim_resident.py (against libftkx.so) and
// tests/test_shim_resident_host.py (against tests/shim/ftkx_stub.cpp) write the scripts and read the results.
//   resident_run <script> <arrays> <out>
// arrays: a file of float64 values; a command names an array by the index of its first value ("-": no array).
// script: one command per line, '#' starts a comment
//   open nd device  dom_start[nd] dom_size[nd]  core_start[nd] core_size[nd]  dims[nd]
//   options name=value ...         every ftkx_options field not named is 0 (tag_mode too: resident_sweep sets it); coords_bounds=b0,b1,...
//                                  the options are handed to set_options() here and, like the patched tracker does, in front of every push
//   rect x [y [z]]                 set_coords_rectilinear: one array per axis, as long as the axis of `dims`
//   explicit ncomp n0 n1 a         set_coords_explicit
//   push_scalar t S                push_scalar(t, S)
//   push t V J S                   push(t, V, J, S)
//   running max                    the running resolution handed to the next sweep starts anew (DBL_MAX); otherwise it is what the last sweep returned
//   sweep t interval               sweep(t, interval != 0, running, ...)
//   pop | clear | close
//   expect_throw <command>         the command must throw std::runtime_error; the object is used again afterwards
// out, one entry per sweep / pop / clear / expect_throw, in script order:
//   u32 1, i32 t, i32 interval, f64 running in, f64 running out, u64 factor, u64 n ordinal, u64 n interval, the ordinal records, the interval records
//   u32 2, u32 thrown (0 | 1)
//   u32 3, u32 what pop_front() returned (clear: 1), u64 size() afterwards, i32 front_timestep(), u32 active()
// It makes no GPU call of its own.
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include <ftkx_shim.hh>
#include <ftkx_tracker.hh>

namespace {

[[noreturn]] void die(const std::string &m) { fprintf(stderr, "resident_run: %s\n", m.c_str()); exit(2); }

struct runner {
  ftkx::resident_sweep rs;
  std::vector<double> arrays;
  ftkx_options opt;
  bool have_opt = false;
  int nd = 0;
  size_t dims[3] = {1, 1, 1};
  double running = DBL_MAX;
  FILE *out = nullptr;

  template <class T> void put(T v) { fwrite(&v, sizeof v, 1, out); }

  const double *array(const std::string &tok, size_t n) const
  {
    if (tok == "-") return nullptr;
    const size_t a = (size_t)std::stoull(tok);
    if (a + n > arrays.size()) die("array " + tok + " + " + std::to_string(n) + " values: past the end of the arrays file");
    return arrays.data() + a;
  }
  size_t nv() const { return dims[0] * dims[1] * dims[2]; }

  static void options(std::istringstream &in, ftkx_options &o)
  {
    std::memset(&o, 0, sizeof o);
    std::string kv;
    while (in >> kv) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) die("options: " + kv);
      const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
      if (k == "jacobian_symmetric") o.jacobian_symmetric = std::stoi(v);
      else if (k == "robust") o.robust = std::stoi(v);
      else if (k == "use_type_filter") o.use_type_filter = std::stoi(v);
      else if (k == "type_filter") o.type_filter = (unsigned)std::stoul(v);
      else if (k == "compute_degrees") o.compute_degrees = std::stoi(v);
      else if (k == "tag_mode") o.tag_mode = std::stoi(v);
      else if (k == "exact_only") o.exact_only = std::stoi(v);
      else if (k == "derive_jacobian") o.derive_jacobian = std::stoi(v);
      else if (k == "coords_mode") o.coords_mode = std::stoi(v);
      else if (k == "coords_bounds") {
        std::istringstream bs(v); std::string b;
        for (int i = 0; i < 6 && std::getline(bs, b, ','); i ++) o.coords_bounds[i] = std::stod(b);
      } else die("options: unknown field " + k);
    }
  }

  void before_push() { if (have_opt && rs.active()) rs.set_options(opt); }   // (patches/ftk-xl-hip.patch: hip_push_snapshot)

  void run(const std::string &cmd, std::istringstream &in)
  {
    if (cmd == "open") {
      int device = 0;
      in >> nd >> device;
      if (nd != 2 && nd != 3) die("open: nd");
      std::vector<long long> v(4 * nd);
      for (auto &x : v) in >> x;
      dims[0] = dims[1] = dims[2] = 1;
      for (int d = 0; d < nd; d ++) in >> dims[d];
      if (!in) die("open: too few values");
      const ftkx::lattice dom(std::vector<long long>(v.begin(), v.begin() + nd), std::vector<long long>(v.begin() + nd, v.begin() + 2 * nd)),
          core(std::vector<long long>(v.begin() + 2 * nd, v.begin() + 3 * nd), std::vector<long long>(v.begin() + 3 * nd, v.end()));
      rs.open(nd, device, dom, core, dims);
    } else if (cmd == "options") {
      options(in, opt); have_opt = true;
      rs.set_options(opt);
    } else if (cmd == "rect") {
      std::string a[3] = {"-", "-", "-"};
      for (int d = 0; d < nd; d ++) in >> a[d];
      rs.set_coords_rectilinear(array(a[0], dims[0]), dims[0], array(a[1], dims[1]), dims[1], nd == 3 ? array(a[2], dims[2]) : nullptr, nd == 3 ? dims[2] : 0);
    } else if (cmd == "explicit") {
      int ncomp = 0; size_t n0 = 0, n1 = 0; std::string a;
      in >> ncomp >> n0 >> n1 >> a;
      if (!in) die("explicit: too few values");
      rs.set_coords_explicit(array(a, (size_t)ncomp * n0 * n1), ncomp, n0, n1);
    } else if (cmd == "push_scalar") {
      int t = 0; std::string s;
      in >> t >> s;
      if (!in) die("push_scalar: too few values");
      before_push();
      rs.push_scalar(t, array(s, nv()));
    } else if (cmd == "push") {
      int t = 0; std::string v, j, s;
      in >> t >> v >> j >> s;
      if (!in) die("push: too few values");
      before_push();
      rs.push(t, array(v, nv() * nd), array(j, nv() * nd * nd), array(s, nv()));
    } else if (cmd == "running") {
      running = DBL_MAX;
    } else if (cmd == "sweep") {
      int t = 0, interval = 0;
      in >> t >> interval;
      if (!in) die("sweep: too few values");
      std::vector<ftkx_cp_t> ordinal, between;
      unsigned long long factor = 0;
      double r = running;
      rs.sweep(t, interval != 0, r, factor, ordinal, between);          // (throws before it writes anything)
      put<uint32_t>(1); put<int32_t>(t); put<int32_t>(interval); put<double>(running); put<double>(r); put<uint64_t>(factor);
      put<uint64_t>(ordinal.size()); put<uint64_t>(between.size());
      if (!ordinal.empty()) fwrite(ordinal.data(), sizeof(ftkx_cp_t), ordinal.size(), out);
      if (!between.empty()) fwrite(between.data(), sizeof(ftkx_cp_t), between.size(), out);
      running = r;
    } else if (cmd == "pop" || cmd == "clear") {
      bool popped = true;
      if (cmd == "pop") popped = rs.pop_front(); else rs.clear();
      put<uint32_t>(3); put<uint32_t>(popped); put<uint64_t>(rs.size()); put<int32_t>(rs.front_timestep()); put<uint32_t>(rs.active());
    } else if (cmd == "close") {
      rs.close();
    } else if (cmd == "expect_throw") {
      std::string inner;
      in >> inner;
      if (!in || inner == "expect_throw") die("expect_throw: no command");
      bool thrown = false;
      try { run(inner, in); } catch (const std::runtime_error &e) { thrown = true; fprintf(stderr, "(expected) %s\n", e.what()); }
      put<uint32_t>(2); put<uint32_t>(thrown);
    } else die("unknown command " + cmd);
  }
};

}  // namespace

int main(int argc, char **argv)
{
  if (argc < 4) die("usage: resident_run <script> <arrays> <out>");
  runner r;
  {
    std::ifstream f(argv[2], std::ios::binary | std::ios::ate);
    if (!f) die(std::string("cannot read ") + argv[2]);
    const std::streamoff bytes = f.tellg();
    r.arrays.resize((size_t)bytes / 8);
    f.seekg(0);
    if (bytes) f.read(reinterpret_cast<char *>(r.arrays.data()), (std::streamsize)(r.arrays.size() * 8));
  }
  std::ifstream script(argv[1]);
  if (!script) die(std::string("cannot read ") + argv[1]);
  r.out = fopen(argv[3], "wb");
  if (!r.out) die(std::string("cannot write ") + argv[3]);
  std::string line;
  int lineno = 0, rc = 0;
  while (std::getline(script, line)) {
    lineno ++;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    try { r.run(cmd, in); }
    catch (const std::exception &e) { fprintf(stderr, "resident_run: line %d (%s): %s\n", lineno, cmd.c_str(), e.what()); rc = 1; break; }
  }
  fclose(r.out);
  return rc;
}
