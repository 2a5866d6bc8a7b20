// Pieces shared by every network executor: the TRY / RUN macros, the workspace arena and its allocator, the element-wise
// launch grid and the answer of a *_workspace_bytes dry run.
#pragma once
#include <map>

#include "common.h"

#define TRY(expr)                        \
  do {                                   \
    int _rc = (expr);                    \
    if (_rc != HEDIT_OK) return _rc;     \
  } while (0)

// launch unless the executor context `f` is planning its workspace
#define RUN(f, expr)            \
  do {                          \
    if (!(f).dry()) TRY(expr);  \
  } while (0)

namespace {

// first-fit arena over the caller's workspace; "dry" mode only records the peak
struct Arena {
  char* base = nullptr;
  size_t cap = 0, peak = 0;
  bool dry = false;
  std::map<size_t, size_t> used;   // offset -> size
  bool failed = false;

  void* alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    size_t pos = 0;
    for (auto& kv : used) {
      if (kv.first >= pos + bytes) break;
      pos = kv.first + kv.second;
    }
    if (!dry && pos + bytes > cap) { failed = true; return nullptr; }
    used[pos] = bytes;
    if (pos + bytes > peak) peak = pos + bytes;
    return dry ? reinterpret_cast<void*>(pos + 4096) : base + pos;
  }
  void free(void* p) {
    if (!p) return;
    size_t off = dry ? reinterpret_cast<size_t>(p) - 4096 : (size_t)(reinterpret_cast<char*>(p) - base);
    used.erase(off);
  }
};

inline Arena& arena_of(Arena& a) { return a; }
template <class F>
auto arena_of(F& f) -> decltype((f.ar)) { return f.ar; }

// n elements of T from an Arena, or from the arena `ar` of an executor context
template <class F, class T>
int aalloc(F& f, T** out, size_t n) {
  Arena& ar = arena_of(f);
  *out = reinterpret_cast<T*>(ar.alloc(n * sizeof(T)));
  if (!*out) {
    hedit_set_error("workspace too small (need more than " + std::to_string(ar.cap) + " bytes)");
    return HEDIT_ERR_ARG;
  }
  return HEDIT_OK;
}

// what a *_workspace_bytes entry answers after its dry run: the arena's peak plus slack, 0 if the walk failed
inline size_t dry_run_bytes(int rc, size_t peak) { return rc == HEDIT_OK ? peak + 4096 : 0; }

inline dim3 egrid(long total) { return dim3(ew_grid(total)); }

}  // namespace
