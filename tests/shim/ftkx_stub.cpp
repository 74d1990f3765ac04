// A recording stand-in for libftkx.so, for tests/test_shim_resident_host.py: the C entry points that ftkx::resident_sweep
// (include/ftkx_shim.hh) calls, and nothing else.  Every call appends one line to the file named by FTKX_STUB_LOG:
//   <entry point> ctx=<serial number of the context> <name>=<value> ...      (structs and arrays as hex bytes)
// A context's serial number is never used twice, so a context re-created at the address of a destroyed one is still another context.
// The stub keeps the timesteps each context holds, so that a drop of a slice that is not resident fails as it does in the library.
// ftkx_sweep_series returns no records.  There is no sweep, no kernel and no GPU call behind any of this.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include <ftkx.h>

struct ftkx_ctx {
  unsigned long long serial;
  int nd;
  long long ext[3];
  std::set<int> slices;
};

namespace {
unsigned long long g_serial = 0;
std::string g_error;

FILE *logfile()
{
  static FILE *fp = nullptr;
  if (!fp) {
    const char *p = getenv("FTKX_STUB_LOG");
    fp = p ? fopen(p, "a") : stderr;
    if (!fp) { perror(p); exit(3); }
  }
  return fp;
}
void begin(const char *what, const ftkx_ctx *c) { fprintf(logfile(), "%s ctx=%llu", what, c ? c->serial : 0ULL); }
void hex(const char *name, const void *p, size_t bytes)
{
  fprintf(logfile(), " %s=", name);
  if (!p) { fprintf(logfile(), "null"); return; }
  for (size_t i = 0; i < bytes; i ++) fprintf(logfile(), "%02x", ((const unsigned char *)p)[i]);
}
void num(const char *name, long long v) { fprintf(logfile(), " %s=%lld", name, v); }
int end(int rc, const char *msg = "")
{
  fprintf(logfile(), " rc=%d\n", rc);
  fflush(logfile());
  if (rc != FTKX_OK) g_error = msg;
  return rc;
}
}  // namespace

extern "C" {

int ftkx_create(ftkx_ctx **ctx, int nd, int device_id)
{
  ftkx_ctx *c = new ftkx_ctx();
  c->serial = ++ g_serial; c->nd = nd; c->ext[0] = c->ext[1] = c->ext[2] = 1;
  *ctx = c;
  begin("ftkx_create", c); num("nd", nd); num("device", device_id);
  return end(FTKX_OK);
}

void ftkx_destroy(ftkx_ctx *ctx)
{
  begin("ftkx_destroy", ctx); num("resident", ctx ? (long long)ctx->slices.size() : 0);
  end(FTKX_OK);
  delete ctx;
}

int ftkx_last_error(const ftkx_ctx *, char *buf, size_t n)
{
  if (buf && n) { strncpy(buf, g_error.c_str(), n - 1); buf[n - 1] = 0; }
  return FTKX_OK;
}

int ftkx_set_mesh(ftkx_ctx *ctx, const long long domain_st[3], const long long domain_sz[3], const long long core_st[3], const long long core_sz[3],
                  const long long ext_st[3], const long long ext_sz[3])
{
  begin("ftkx_set_mesh", ctx);
  hex("domain_st", domain_st, 24); hex("domain_sz", domain_sz, 24); hex("core_st", core_st, 24); hex("core_sz", core_sz, 24);
  hex("ext_st", ext_st, 24); hex("ext_sz", ext_sz, 24);
  if (!ctx) return end(FTKX_E_INVALID, "stub: no context");
  for (int d = 0; d < 3; d ++) ctx->ext[d] = ext_sz[d];
  return end(FTKX_OK);
}

int ftkx_set_options(ftkx_ctx *ctx, const ftkx_options *opt)
{
  begin("ftkx_set_options", ctx); hex("opt", opt, sizeof *opt);
  if (!ctx || !opt) return end(FTKX_E_INVALID, "stub: no context");
  return end(FTKX_OK);
}

int ftkx_set_coords_rectilinear(ftkx_ctx *ctx, const double *x, size_t nx, const double *y, size_t ny, const double *z, size_t nz)
{
  begin("ftkx_set_coords_rectilinear", ctx);
  hex("x", x, 8 * nx); hex("y", y, 8 * ny); hex("z", z, 8 * nz);
  if (!ctx) return end(FTKX_E_INVALID, "stub: no context");
  return end(FTKX_OK);
}

int ftkx_set_coords_explicit(ftkx_ctx *ctx, const double *coords, int ncomp, size_t n0, size_t n1)
{
  begin("ftkx_set_coords_explicit", ctx);
  num("ncomp", ncomp); num("n0", (long long)n0); num("n1", (long long)n1); hex("coords", coords, 8 * (size_t)ncomp * n0 * n1);
  if (!ctx) return end(FTKX_E_INVALID, "stub: no context");
  return end(FTKX_OK);
}

static int push(const char *what, ftkx_ctx *ctx, int t, const double *V, const double *J, const double *S, int on_device)
{
  begin(what, ctx); num("t", t);
  const size_t nv = ctx ? (size_t)(ctx->ext[0] * ctx->ext[1] * ctx->ext[2]) : 0, nd = ctx ? (size_t)ctx->nd : 0;
  hex("V", V, 8 * nv * nd); hex("J", J, 8 * nv * nd * nd); hex("S", S, 8 * nv); num("on_device", on_device);
  if (!ctx) return end(FTKX_E_INVALID, "stub: no context");
  if (!ctx->slices.insert(t).second) return end(FTKX_E_INVALID, "stub: the slice is resident already");
  return end(FTKX_OK);
}

int ftkx_push_slice(ftkx_ctx *ctx, int t, const double *V, const double *J, const double *S, int on_device)
{
  return push("ftkx_push_slice", ctx, t, V, J, S, on_device);
}

int ftkx_push_scalar_slice(ftkx_ctx *ctx, int t, const double *S, int on_device)
{
  return push("ftkx_push_scalar_slice", ctx, t, nullptr, nullptr, S, on_device);
}

int ftkx_drop_slice(ftkx_ctx *ctx, int t)
{
  begin("ftkx_drop_slice", ctx); num("t", t);
  if (!ctx) return end(FTKX_E_INVALID, "stub: no context");
  if (!ctx->slices.erase(t)) return end(FTKX_E_NOSLICE, "stub: the slice is not resident");
  return end(FTKX_OK);
}

int ftkx_sweep_series(ftkx_ctx *ctx, const int *timesteps, const int *scopes, int n, double *running_resolution,
                      unsigned long long *factors, const ftkx_cp_t **out, size_t *n_out)
{
  begin("ftkx_sweep_series", ctx); num("n", n);
  hex("timesteps", timesteps, 4 * (size_t)n); hex("scopes", scopes, 4 * (size_t)n); hex("running", running_resolution, 8);
  if (!ctx) return end(FTKX_E_INVALID, "stub: no context");
  for (int i = 0; i < n; i ++)
    if (!ctx->slices.count(timesteps[i]) || ((scopes[i] & FTKX_SCOPE_INTERVAL) && !ctx->slices.count(timesteps[i] + 1)))
      return end(FTKX_E_NOSLICE, "stub: sweep of a slice that is not resident");
  for (int i = 0; factors && i < n; i ++) factors[i] = 0;
  *out = nullptr; *n_out = 0;
  return end(FTKX_OK);
}

}  // extern "C"
