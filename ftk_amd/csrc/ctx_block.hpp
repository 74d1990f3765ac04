// One owning block of memory: what every buffer of a context is (ctx.hpp), but for the slice arrays and their pools.  A block knows its
// pointer, its size IN BYTES and what kind of memory it is; it is admitted by the bytes of the very buffer that is about to be indexed
// (`reserve`), and its destructor gives it back.  No HIP in here: the three raw functions are ftkx_api.hip's, or a host check's own.
#pragma once
#include <cstddef>

struct ftkx_ctx;

enum ftkx_block_kind {
  FTKX_BLOCK_DEVICE = 0,
  FTKX_BLOCK_PINNED,                // the runtime's default mapping
  FTKX_BLOCK_PINNED_COHERENT,       // fine-grained: a kernel's system-scope stores are seen by a host that polls
  FTKX_BLOCK_PINNED_NONCOHERENT     // ordinary cached memory for the CPU, read after a synchronise
};

int ftkx_block_alloc(ftkx_ctx *c, ftkx_block_kind kind, size_t bytes, void **p);   // 0, or fail()'s code (FTKX_E_NOMEM / FTKX_E_DEVICE) with *p null
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

  // At least `need` bytes.  Nothing happens while the block holds them; otherwise what it held is freed -- after `drain`, a stream that may
  // still read it, has been waited for -- and `alloc` bytes (0: `need`) are allocated: contents are not kept, `*fresh` says that the memory
  // is new.  A failed allocation leaves the block empty.
  int reserve(ftkx_ctx *c, size_t need, size_t alloc = 0, void *drain = nullptr, bool *fresh = nullptr)
  {
    if (fresh) *fresh = false;
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
  void drop() { if (p) ftkx_block_free(kind, p); p = nullptr; bytes = 0; }
};
