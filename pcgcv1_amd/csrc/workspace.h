// Caller-allocated workspaces, host side.  The rule for every one of them: ONE layout function X_layout(args..., base) carves
// the regions; pcgc_X_workspace_bytes is its argument check and X_layout(args..., nullptr).bytes, the entry points pass the real
// base.  What sizes a workspace is what carves it.  Plain C++17, no HIP: tests/workspace_check.cpp.
#pragma once
#include <cstddef>

namespace pcgc {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Bump allocator over byte offsets from a 256-byte aligned base: net_plan.h's workspace plan and weight blob
struct Arena {
  size_t end = 0;
  size_t take(size_t bytes, size_t align) { const size_t at = (end + align - 1) / align * align; end = at + bytes; return at; }
};

// Typed regions in order from a base that may be null (then every pointer is null and only bytes() counts).  A region starts
// where the one before it ended: take() rounds its length up to 256 bytes, take_unrounded() is for a last region whose
// workspace size was never rounded.  A carver handed on by value goes on where this one stands (a layout inside a layout).
struct Carver {
  char* base;
  size_t at = 0;
  Carver(void* workspace = nullptr) : base(static_cast<char*>(workspace)) {}
  template <class T> T* take_unrounded(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
    at += count * sizeof(T);
    return p;
  }
  template <class T> T* take(size_t count) { T* p = take_unrounded<T>(count); at = align256(at); return p; }
  size_t bytes() const { return at; }
};

}  // namespace pcgc
