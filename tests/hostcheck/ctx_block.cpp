// ftk_amd/csrc/ctx_block.hpp without a GPU: ftkx_block over malloc and free.  The three raw functions are defined HERE -- they count their
// calls, remember their order and can be told to fail the next allocation -- so that every rule of reserve(), of moving and of destruction
// is checked on the host, under ASan (with leak detection) and UBSan where they are installed.  A program of its own:
// tests/test_ctx_block_host.py compiles and runs it.
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
  if (fail_next_alloc) { fail_next_alloc = false; return FTKX_E_NOMEM; }
  *p = malloc(bytes ? bytes : 1);
  if (!*p) return FTKX_E_NOMEM;
  memset(*p, 0xa5, bytes);               // (every byte of what was asked for is writable: ASan would say otherwise)
  n_alloc ++; last_alloc_bytes = bytes; last_alloc_kind = kind; order += 'a';
  return FTKX_OK;
}

void ftkx_block_free(ftkx_block_kind kind, void *p) { n_free ++; last_freed = p; last_free_kind = kind; order += 'f'; free(p); }

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

}  // namespace

int main()
{
  check_reserve();
  check_kinds();
  check_move();
  check_patch_sequence();
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("ctx_block checks complete\n");
  return 0;
}
