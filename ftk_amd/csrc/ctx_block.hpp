// One owning block of memory: what every buffer of a context is (ctx.hpp), the slice arrays included.  A block knows its pointer, its size
// IN BYTES and what kind of memory it is; it is admitted by the bytes of the very buffer that is about to be indexed (`reserve`), and its
// destructor gives it back.  Behind it the pool the slice arrays come out of and go back to (ftkx_array_pool): blocks by class and by
// their own bytes.  No HIP in here: the three raw functions are ftkx_api.hip's, or a host check's own.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

struct ftkx_ctx;

enum ftkx_block_kind {
  FTKX_BLOCK_DEVICE = 0,
  FTKX_BLOCK_PINNED,                // the runtime's default mapping
  FTKX_BLOCK_PINNED_COHERENT,       // fine-grained: a kernel's system-scope stores are seen by a host that polls
  FTKX_BLOCK_PINNED_NONCOHERENT,    // ordinary cached memory for the CPU, read after a synchronise
  FTKX_BLOCK_LENT                   // the caller's device memory, adopted as it is (ftkx_block::lent): never freed, never pooled, never reserved
};

int ftkx_block_alloc(ftkx_ctx *c, ftkx_block_kind kind, size_t bytes, void **p);   // 0, or fail()'s code (FTKX_E_NOMEM / FTKX_E_DEVICE; FTKX_E_INVALID for a lent block) with *p null
void ftkx_block_free(ftkx_block_kind kind, void *p);
int ftkx_block_drain(ftkx_ctx *c, void *stream);                                   // the host waits for the stream; 0 or fail()'s code

struct ftkx_block {
  void *p = nullptr;
  size_t bytes = 0;
  ftkx_block_kind kind;
  explicit ftkx_block(ftkx_block_kind k = FTKX_BLOCK_DEVICE) : kind(k) {}
  ftkx_block(const ftkx_block &) = delete;
  ftkx_block &operator=(const ftkx_block &) = delete;
  ftkx_block(ftkx_block &&o) noexcept : p(o.p), bytes(o.bytes), kind(o.kind) { o.p = nullptr; o.bytes = 0; }
  ftkx_block &operator=(ftkx_block &&o) noexcept
  {
    if (this != &o) { drop(); p = o.p; bytes = o.bytes; kind = o.kind; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~ftkx_block() { drop(); }
  static ftkx_block lent(void *p, size_t bytes) { ftkx_block b(FTKX_BLOCK_LENT); b.p = p; b.bytes = bytes; return b; }

  // At least `need` bytes.  Nothing happens while the block holds them; otherwise what it held is freed -- after `drain`, a stream that may
  // still read it, has been waited for -- and `alloc` bytes (0: `need`) are allocated: contents are not kept, `*fresh` says that the memory
  // is new.  A failed allocation leaves the block empty.  A lent block is left as it is: the raw function's error.
  int reserve(ftkx_ctx *c, size_t need, size_t alloc = 0, void *drain = nullptr, bool *fresh = nullptr)
  {
    if (fresh) *fresh = false;
    if (kind == FTKX_BLOCK_LENT) { void *none; return ftkx_block_alloc(c, kind, need, &none); }
    if (bytes >= need) return 0;
    if (p && drain) { if (const int rc = ftkx_block_drain(c, drain)) return rc; }
    drop();
    if (alloc < need) alloc = need;
    if (const int rc = ftkx_block_alloc(c, kind, alloc, &p)) { p = nullptr; return rc; }
    bytes = alloc;
    if (fresh) *fresh = true;
    return 0;
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
  template <class T> size_t count() const { return bytes / sizeof(T); }

private:
  void drop() { if (p && kind != FTKX_BLOCK_LENT) ftkx_block_free(kind, p); p = nullptr; bytes = 0; }
};

// The slice arrays of a context that no slice holds right now (a streaming tracker pushes and pops one slice per step: an allocation and a
// free per step cost more than the sweep itself).  An array is taken out for exactly the class and the bytes it was allocated with, so one
// of another lattice is never handed out.  WHEN an array may come back depends on stream order and stays with the callers (ftkx_api.hip, ingest.hip:
// free_slice, release_retired, give_pooled); whatever takes it out next is ordered behind its last reader by the context's stream,
// whichever array it is: every class is searched newest first (what was given back last is what the caches may still hold).
enum ftkx_array_class { FTKX_ARRAY_FIELD = 0, FTKX_ARRAY_MASK, FTKX_ARRAY_SUMMARY, FTKX_ARRAY_CLASSES };

struct ftkx_array_pool {
  std::vector<ftkx_block> held[FTKX_ARRAY_CLASSES];
  unsigned long long allocated[FTKX_ARRAY_CLASSES] = {0, 0, 0};      // arrays take() had to allocate, since the context was made

  // a pooled array of this class and of exactly `bytes`, or a new one (`*fresh`: its contents are undefined; a pooled mask or summary array
  // keeps the neutral padding of its first life).  A failed allocation leaves `out` empty and the pool as it was.
  int take(ftkx_ctx *c, ftkx_array_class k, size_t bytes, ftkx_block &out, bool *fresh = nullptr)
  {
    std::vector<ftkx_block> &v = held[k];
    for (size_t i = v.size(); i -- > 0; )
      if (v[i].bytes == bytes) { out = std::move(v[i]); v.erase(v.begin() + (long)i); if (fresh) *fresh = false; return 0; }
    out = ftkx_block();
    const int rc = out.reserve(c, bytes, 0, nullptr, fresh);
    if (rc == 0) allocated[k] ++;
    return rc;
  }
  // `b` goes into the pool, or -- `cap` arrays of its class are there already -- is freed; empty afterwards either way.  A lent block is let go.
  void give(ftkx_array_class k, ftkx_block &&b, size_t cap = (size_t)-1)
  {
    ftkx_block mine(std::move(b));
    if (mine.p && mine.kind == FTKX_BLOCK_DEVICE && held[k].size() < cap) held[k].push_back(std::move(mine));
  }
  void clear() { for (std::vector<ftkx_block> &v : held) v.clear(); }
};
