// ftk_amd/csrc/ctx_block.hpp without a GPU: ftkx_block over malloc and free.  The three raw functions are defined HERE -- they count their
// calls, remember their order and can be told to fail the next allocation -- so that every rule of reserve(), of moving and of destruction
// is checked on the host, under ASan (with leak detection) and UBSan where they are installed.  The same for the lent kind and for
// ftkx_array_pool, the pool of the slice arrays.  A program of its own: tests/test_ctx_block_host.py compiles and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

#include "../../include/ftkx.h"
#include "../../ftk_amd/csrc/ctx_block.hpp"

namespace {

int failures = 0;

#define CHECK(cond, ...)                                                                     \
  do {                                                                                       \
    if (!(cond)) { failures ++; fprintf(stderr, "FAILED %s (line %d): ", #cond, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
  } while (0)

int n_alloc = 0, n_free = 0, n_drain = 0;
size_t last_alloc_bytes = 0;
ftkx_block_kind last_alloc_kind = FTKX_BLOCK_DEVICE, last_free_kind = FTKX_BLOCK_DEVICE;
void *last_freed = nullptr, *last_drained = nullptr;
bool fail_next_alloc = false;
std::string order;                       // 'd' drain, 'f' free, 'a' allocation, in the order they happened

void reset() { n_alloc = n_free = n_drain = 0; last_alloc_bytes = 0; last_freed = last_drained = nullptr; order.clear(); }

}  // namespace

int ftkx_block_alloc(ftkx_ctx *, ftkx_block_kind kind, size_t bytes, void **p)
{
  *p = nullptr;
  if (kind == FTKX_BLOCK_LENT) return FTKX_E_INVALID;    // (as ftkx_api.hip's: nothing is ever allocated for a lent block)
  if (fail_next_alloc) { fail_next_alloc = false; return FTKX_E_NOMEM; }
  *p = malloc(bytes ? bytes : 1);
  if (!*p) return FTKX_E_NOMEM;
  memset(*p, 0xa5, bytes);               // (every byte of what was asked for is writable: ASan would say otherwise)
  n_alloc ++; last_alloc_bytes = bytes; last_alloc_kind = kind; order += 'a';
  return FTKX_OK;
}

void ftkx_block_free(ftkx_block_kind kind, void *p) { if (kind == FTKX_BLOCK_LENT) { fprintf(stderr, "FAILED: a lent block reached ftkx_block_free\n"); failures ++; return; } n_free ++; last_freed = p; last_free_kind = kind; order += 'f'; free(p); }

int ftkx_block_drain(ftkx_ctx *, void *stream) { n_drain ++; last_drained = stream; order += 'd'; return FTKX_OK; }

namespace {

void check_reserve()
{
  reset();
  int stream_tag = 0;
  void *stream = &stream_tag;
  {
    ftkx_block b;
    bool fresh = true;
    CHECK(b.p == nullptr && b.bytes == 0 && b.kind == FTKX_BLOCK_DEVICE, "a new block is empty device memory");
    CHECK(b.reserve(nullptr, 0, 0, stream, &fresh) == FTKX_OK && !fresh && n_alloc == 0 && n_drain == 0, "nothing is reserved for nothing");
    // the first allocation: nothing to drain, nothing to free
    CHECK(b.reserve(nullptr, 100, 0, stream, &fresh) == FTKX_OK && fresh, "first reserve");
    CHECK(n_alloc == 1 && n_free == 0 && n_drain == 0 && last_alloc_bytes == 100 && b.bytes == 100 && b.p, "first reserve: %d allocations, %d frees, %d drains, %zu bytes", n_alloc, n_free, n_drain, b.bytes);
    CHECK(b.count<double>() == 12 && b.count<char>() == 100 && b.as<char>() == (char *)b.p, "count<T>() is bytes / sizeof(T)");
    // at or below `bytes`: nothing happens, the pointer stays
    void *p0 = b.p;
    for (size_t need : {(size_t)0, (size_t)1, (size_t)99, (size_t)100}) {
      fresh = true;
      CHECK(b.reserve(nullptr, need, 4096, stream, &fresh) == FTKX_OK && !fresh && b.p == p0 && b.bytes == 100, "reserve(%zu) of 100 bytes", need);
    }
    CHECK(n_alloc == 1 && n_free == 0 && n_drain == 0, "no call at or below `bytes`");
    // growth with slack and a drain stream: drained, THEN freed once, then `alloc` bytes allocated; fresh memory reported
    reset();
    CHECK(b.reserve(nullptr, 101, 256, stream, &fresh) == FTKX_OK && fresh, "growing reserve");
    CHECK(order == "dfa", "order of drain, free, allocation: %s", order.c_str());
    CHECK(n_free == 1 && last_freed == p0 && n_alloc == 1 && last_alloc_bytes == 256 && b.bytes == 256 && last_drained == stream, "growth: freed %d, allocated %zu", n_free, last_alloc_bytes);
    // growth without a drain stream: no drain
    reset();
    CHECK(b.reserve(nullptr, 300) == FTKX_OK && order == "fa" && b.bytes == 300 && n_drain == 0, "growth without a stream: %s", order.c_str());
    // `alloc` below `need` never shortens the block
    CHECK(b.reserve(nullptr, 400, 10) == FTKX_OK && b.bytes == 400, "alloc < need allocates need");
    // a failed allocation: the block is empty, the status is the out-of-memory one; the next reserve succeeds
    reset();
    fail_next_alloc = true;
    fresh = true;
    CHECK(b.reserve(nullptr, 1000, 2000, stream, &fresh) == FTKX_E_NOMEM && !fresh, "failed allocation: status");
    CHECK(b.p == nullptr && b.bytes == 0 && n_free == 1 && n_alloc == 0, "failed allocation leaves the block empty");
    reset();
    CHECK(b.reserve(nullptr, 1000, 2000, stream, &fresh) == FTKX_OK && fresh && b.bytes == 2000 && order == "a", "reserve after a failure: %s (an empty block is neither drained nor freed)", order.c_str());
    reset();
  }
  CHECK(n_free == 1 && n_drain == 0 && order == "f", "destroying an owning block frees exactly once: %s", order.c_str());
  reset();
  { ftkx_block empty(FTKX_BLOCK_PINNED); }
  CHECK(n_free == 0, "destroying an empty block frees nothing");
}

void check_kinds()
{
  for (ftkx_block_kind k : {FTKX_BLOCK_DEVICE, FTKX_BLOCK_PINNED, FTKX_BLOCK_PINNED_COHERENT, FTKX_BLOCK_PINNED_NONCOHERENT}) {
    reset();
    {
      ftkx_block b(k);
      CHECK(b.reserve(nullptr, 64) == FTKX_OK && last_alloc_kind == k, "allocation by kind %d", (int)k);
    }
    CHECK(n_free == 1 && last_free_kind == k, "free by kind %d", (int)k);
  }
}

void check_move()
{
  reset();
  {
    ftkx_block a(FTKX_BLOCK_PINNED_COHERENT);
    CHECK(a.reserve(nullptr, 64) == FTKX_OK, "reserve");
    void *p = a.p;
    ftkx_block b(std::move(a));
    CHECK(a.p == nullptr && a.bytes == 0, "moving a block empties its source");
    CHECK(b.p == p && b.bytes == 64 && b.kind == FTKX_BLOCK_PINNED_COHERENT && n_free == 0, "the target owns what the source held");
    { ftkx_block gone(std::move(a)); }                       // (the emptied source, moved again and destroyed)
    CHECK(n_free == 0, "destroying an emptied source frees nothing");
    // move assignment: what the target held is freed, once; an empty block assigned releases (ftkx_set_coords_*: a new array every time)
    ftkx_block c;
    CHECK(c.reserve(nullptr, 32) == FTKX_OK, "reserve");
    void *pc = c.p;
    c = std::move(b);
    CHECK(n_free == 1 && last_freed == pc && c.p == p && c.kind == FTKX_BLOCK_PINNED_COHERENT && b.p == nullptr && b.bytes == 0, "move assignment");
    c = ftkx_block();
    CHECK(n_free == 2 && last_freed == p && c.p == nullptr && c.bytes == 0 && c.kind == FTKX_BLOCK_DEVICE, "assigning an empty block releases");
  }
  CHECK(n_free == 2 && n_alloc == 2, "every allocation freed exactly once: %d of %d", n_free, n_alloc);
}

// The staging of patches for host-side callers (halo.hip, patches_common).  Four cells of a 2D scalar slice take 4 * 36 doubles; the same
// four cells of a 2D vector slice take 4 * 72.  The rule this replaces admitted the second call by CELLS -- "capacity 4 >= 4 cells", no
// growth -- and the kernel then wrote 4 * 72 doubles into 4 * 36.  Admitted by the bytes of the buffer itself, the second call grows it.
void check_patch_sequence()
{
  reset();
  ftkx_block patches;
  const size_t cells = 4, scalar_bytes = cells * 36 * sizeof(double), vector_bytes = cells * 72 * sizeof(double);
  CHECK(patches.reserve(nullptr, scalar_bytes) == FTKX_OK && patches.bytes == scalar_bytes, "scalar patches");
  const size_t old_rule_capacity = cells;                    // what patch_cap would have held
  CHECK(old_rule_capacity >= cells, "the old rule lets the vector call in without growth");
  bool fresh = false;
  CHECK(patches.reserve(nullptr, vector_bytes, 0, nullptr, &fresh) == FTKX_OK && fresh, "vector patches grow the buffer");
  CHECK(patches.bytes >= vector_bytes && n_alloc == 2 && n_free == 1, "%zu bytes for %zu", patches.bytes, vector_bytes);
  memset(patches.p, 0, vector_bytes);                        // what the kernel writes and the copy back reads (ASan checks the extent)
  // and back to scalar: the larger buffer serves
  CHECK(patches.reserve(nullptr, scalar_bytes, 0, nullptr, &fresh) == FTKX_OK && !fresh && n_alloc == 2, "scalar again: no growth");
}

// Memory the caller lent (ftkx_push_scalar_slice with on_device = 1): never freed, never pooled, never reserved.
void check_lent()
{
  reset();
  double callers[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  {
    ftkx_block a = ftkx_block::lent(callers, sizeof(callers));
    CHECK(a.p == callers && a.bytes == sizeof(callers) && a.kind == FTKX_BLOCK_LENT && a.as<double>()[7] == 8 && a.count<double>() == 8, "a lent block is the caller's memory");
    ftkx_block b(std::move(a));
    CHECK(a.p == nullptr && a.bytes == 0 && b.p == callers && b.bytes == sizeof(callers) && b.kind == FTKX_BLOCK_LENT, "moving a lent block empties its source");
    bool fresh = true;
    for (size_t need : {(size_t)0, (size_t)8, sizeof(callers), 2 * sizeof(callers)})
      CHECK(b.reserve(nullptr, need, 0, nullptr, &fresh) == FTKX_E_INVALID && !fresh && b.p == callers && b.bytes == sizeof(callers), "reserve(%zu) on a lent block is an error and leaves it alone", need);
    ftkx_block d;
    CHECK(d.reserve(nullptr, 16) == FTKX_OK, "reserve");
    d = std::move(b);                                        // (what the target owned is freed; what it now holds is not its own)
    CHECK(n_free == 1 && d.p == callers && d.kind == FTKX_BLOCK_LENT && b.p == nullptr, "move assignment of a lent block");
    ftkx_array_pool pool;
    pool.give(FTKX_ARRAY_FIELD, std::move(d), 12);
    CHECK(d.p == nullptr && d.bytes == 0 && pool.held[FTKX_ARRAY_FIELD].empty(), "a lent block cannot be given to the pool: it is let go");
    ftkx_block again = ftkx_block::lent(callers, sizeof(callers));
  }
  CHECK(n_free == 1 && n_alloc == 1 && n_drain == 0 && callers[0] == 1 && callers[7] == 8, "no lent block was freed (%d frees), the caller's memory is as it was", n_free);
}

void check_pool()
{
  reset();
  const ftkx_array_class F = FTKX_ARRAY_FIELD, M = FTKX_ARRAY_MASK, U = FTKX_ARRAY_SUMMARY;
  {
    ftkx_array_pool pool;
    ftkx_block a, b, c3;
    bool fresh = false;
    CHECK(pool.take(nullptr, F, 64, a, &fresh) == FTKX_OK && fresh && a.bytes == 64 && pool.allocated[F] == 1 && n_alloc == 1, "an empty pool allocates");
    void *pa = a.p;
    pool.give(F, std::move(a), 12);
    CHECK(a.p == nullptr && pool.held[F].size() == 1 && n_free == 0, "given back: held, not freed");
    // another class, a larger and a smaller request: never the held array
    CHECK(pool.take(nullptr, M, 64, b, &fresh) == FTKX_OK && fresh && b.p != pa && pool.held[F].size() == 1 && pool.allocated[M] == 1, "a block is not returned for another class");
    CHECK(pool.take(nullptr, F, 128, c3, &fresh) == FTKX_OK && fresh && c3.p != pa && c3.bytes == 128 && pool.held[F].size() == 1, "... nor for a request larger than its bytes");
    memset(c3.p, 0, 128);                                   // (what a kernel of the larger lattice writes: ASan checks the extent)
    CHECK(pool.take(nullptr, F, 32, c3, &fresh) == FTKX_OK && fresh && c3.p != pa && c3.bytes == 32 && pool.held[F].size() == 1, "... nor for a smaller one");
    CHECK(pool.allocated[F] == 3 && pool.allocated[M] == 1 && pool.allocated[U] == 0, "allocations are counted by class");
    // the same class and bytes: the same memory, not fresh, nothing allocated
    const int allocs = n_alloc;
    CHECK(pool.take(nullptr, F, 64, a, &fresh) == FTKX_OK && !fresh && a.p == pa && a.bytes == 64 && n_alloc == allocs && pool.allocated[F] == 3 && pool.held[F].empty(), "take after give returns the same memory");
    // newest first
    void *pb = b.p;
    pool.give(M, std::move(b)); pool.take(nullptr, M, 64, b); pool.give(M, std::move(b));      // (held: pb)
    ftkx_block m2;
    CHECK(pool.take(nullptr, M, 64, m2, &fresh) == FTKX_OK && !fresh && m2.p == pb, "the pooled mask array comes out again");
    ftkx_block m3;
    CHECK(pool.take(nullptr, M, 64, m3, &fresh) == FTKX_OK && fresh, "a second one is new");
    void *p3 = m3.p;
    pool.give(M, std::move(m2)); pool.give(M, std::move(m3));
    CHECK(pool.take(nullptr, M, 64, m2) == FTKX_OK && m2.p == p3 && pool.held[M].size() == 1 && pool.held[M][0].p == pb, "newest first");
    pool.give(M, std::move(m2));
    // the cap: the surplus is freed, once
    reset();
    ftkx_block u[3];
    for (ftkx_block &x : u) CHECK(pool.take(nullptr, U, 16, x) == FTKX_OK, "take");
    void *surplus = u[2].p;
    for (ftkx_block &x : u) pool.give(U, std::move(x), 2);
    CHECK(pool.held[U].size() == 2 && n_free == 1 && last_freed == surplus && !u[2].p, "the cap frees the surplus exactly once (%d frees)", n_free);
    ftkx_block empty;
    pool.give(U, std::move(empty), 12);
    CHECK(pool.held[U].size() == 2, "an empty block is not pooled");
    // a failed allocation leaves nothing behind
    reset();
    const size_t held_f = pool.held[F].size();
    fail_next_alloc = true;
    fresh = true;
    CHECK(pool.take(nullptr, F, 4096, c3, &fresh) == FTKX_E_NOMEM && !fresh && c3.p == nullptr && c3.bytes == 0, "failed allocation: status, an empty block");
    CHECK(pool.allocated[F] == 3 && pool.held[F].size() == held_f && n_alloc == 0 && n_free == 1, "failed allocation: nothing counted, the pool as it was (what the target held was freed: %d)", n_free);
    // clear() frees all
    reset();
    const size_t held = pool.held[F].size() + pool.held[M].size() + pool.held[U].size();
    pool.clear();
    CHECK(held == 4 && (size_t)n_free == held && pool.held[F].empty() && pool.held[M].empty() && pool.held[U].empty(), "clear frees all: %d of %zu", n_free, held);
    pool.give(F, std::move(a), 12);                          // (... and what is held when the pool dies goes with it)
  }
  CHECK(n_free == 5, "the pool's destructor frees what it holds");
}

// ftkx_set_mesh under an open split pass.  Slices dropped while the pass was open are parked with it; the mesh grows, the pool is cleared,
// the pass completes and its parked arrays -- of the OLD lattice -- come back: stragglers.  The rule this replaces kept field arrays as
// (pointer, count) with the count recomputed from the context's CURRENT mesh when the array was given back, and mask arrays with no size
// at all: the straggler went in under the new lattice's count, and the next push took it for the larger lattice and wrote past its end.
// That is the old overrun.  An array that carries its own bytes cannot be taken out for more than it holds.
void check_mesh_sequence()
{
  reset();
  const size_t old_bytes = 16 * 16 * sizeof(double), new_bytes = 48 * 40 * sizeof(double);
  ftkx_array_pool pool;
  ftkx_block parked, filler[3], got;
  CHECK(pool.take(nullptr, FTKX_ARRAY_FIELD, old_bytes, parked) == FTKX_OK, "take");
  for (ftkx_block &f : filler) CHECK(pool.take(nullptr, FTKX_ARRAY_FIELD, old_bytes, f) == FTKX_OK, "take");
  for (ftkx_block &f : filler) pool.give(FTKX_ARRAY_FIELD, std::move(f), 12);
  pool.clear();                                              // the mesh changes
  CHECK(n_free == 3 && pool.held[FTKX_ARRAY_FIELD].empty(), "the pool of the old lattice is freed");
  void *straggler = parked.p;
  pool.give(FTKX_ARRAY_FIELD, std::move(parked), 12);        // the pass completes after the change
  // the old rule: tagged with the current lattice's count, so a request for that count finds it
  const size_t old_rule_tag = new_bytes / sizeof(double), request = new_bytes / sizeof(double);
  CHECK(old_rule_tag == request, "under the old rule the straggler is returned for the new lattice: the old overrun");
  bool fresh = false;
  CHECK(pool.take(nullptr, FTKX_ARRAY_FIELD, new_bytes, got, &fresh) == FTKX_OK && fresh && got.p != straggler && got.bytes == new_bytes, "a take at the larger size allocates");
  memset(got.p, 0, new_bytes);                               // (what the upload writes: ASan checks the extent)
  CHECK(pool.held[FTKX_ARRAY_FIELD].size() == 1 && pool.held[FTKX_ARRAY_FIELD][0].p == straggler && pool.held[FTKX_ARRAY_FIELD][0].bytes == old_bytes, "the straggler stays in the pool under its own bytes");
  // (and it still serves the old lattice, should the mesh go back)
  CHECK(pool.take(nullptr, FTKX_ARRAY_FIELD, old_bytes, got, &fresh) == FTKX_OK && !fresh && got.p == straggler, "the straggler serves a request of its own size");
}

}  // namespace

int main()
{
  check_reserve();
  check_kinds();
  check_move();
  check_patch_sequence();
  check_lent();
  check_pool();
  check_mesh_sequence();
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("ctx_block checks complete\n");
  return 0;
}
