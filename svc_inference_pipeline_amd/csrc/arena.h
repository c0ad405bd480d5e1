// The workspace arena: a bump allocator that grows and never shrinks, sized by the buffer list of the stage that
// uses it (plan). Plain C++: the device allocation behind reserve is engine.hip's, so a host program that includes this
// header alone can define reserve (and set_error) itself and back an arena with host memory (tests/arena_check.cpp).
#pragma once
#include <stddef.h>

#ifndef SVC_ERR_STATE
#define SVC_ERR_STATE 3  // common.h's, for a program without it
#endif

namespace svc {

void set_error(const char* fmt, ...);

struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0;
  // at least `bytes` of capacity: a larger block replaces the present one (whose contents are dropped), a smaller
  // request changes nothing
  int reserve(size_t bytes);
  void reset() { off = 0; }
  // n elements of T at the next multiple of 256 bytes; NULL where they do not fit, and off advances either way, so an
  // arena without memory only counts what a sequence of gets asks for
  template <typename T>
  T* get(size_t n) {
    const size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
    T* p = bytes <= cap && off <= cap - bytes ? reinterpret_cast<T*>(base + off) : nullptr;
    off += bytes;
    return p;
  }
  // Lays a stage's buffers out: `layout` (gets and arithmetic only, the same on every run) runs once on an arena
  // that only counts and, once this one holds that many bytes, again on this one from offset 0. Every get of the
  // second run fits then; a layout that asked for something else the second time is SVC_ERR_STATE, before any pointer
  // of it is used.
  template <typename Layout>
  int plan(Layout&& layout) {
    Arena count;
    layout(count);
    if (int st = reserve(count.off)) return st;
    reset();
    layout(*this);
    if (off == count.off) return 0;
    set_error("workspace layout: %zu bytes on the counting pass, %zu on the second", count.off, off);
    return SVC_ERR_STATE;
  }
};

}  // namespace svc
