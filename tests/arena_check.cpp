// The workspace arena (csrc/arena.h) on host memory: a plain C++ program, built with -fsanitize=address,undefined and run
// by tests/test_arena_host.py. It supplies the two functions the library defines in engine.hip: Arena::reserve (malloc
// here, so the sanitizer sees every byte past a block's end) and set_error.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "arena.h"

namespace svc {

static char g_err[256] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static int g_allocs = 0;
int Arena::reserve(size_t bytes) {
  if (bytes <= cap) return 0;
  free(base);
  base = static_cast<char*>(aligned_alloc(256, bytes));  // (every counted total is a multiple of 256)
  cap = base ? bytes : 0;
  ++g_allocs;
  return base ? 0 : 2;
}

}  // namespace svc

using svc::Arena;

static int g_fail = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++g_fail;                                                  \
    }                                                            \
  } while (0)

// a stage-like layout: mixed types, odd sizes, an empty buffer and a single byte, `scale` times over
struct Bufs {
  float* a;
  uint16_t* b;
  char* empty;
  char* one;
  double* c;
  char* last;
  size_t last_n;
  std::vector<size_t> offs;  // the arena's offset before every get
};
static void layout(Arena& ws, Bufs& u, size_t scale) {
  u.offs.clear();
  auto mark = [&] { u.offs.push_back(ws.off); };
  mark(), u.a = ws.get<float>(100 * scale + 1);
  mark(), u.b = ws.get<uint16_t>(127 * scale);
  mark(), u.empty = ws.get<char>(0);
  mark(), u.one = ws.get<char>(1);
  mark(), u.c = ws.get<double>(33 * scale);
  u.last_n = 300 * scale + 7;
  mark(), u.last = ws.get<char>(u.last_n);
  mark();
}

int main() {
  // ---- same offsets, alignment, exact fit
  Bufs count, real;
  Arena counting;
  layout(counting, count, 1);
  CHECK(counting.base == nullptr && counting.cap == 0);
  CHECK(count.a == nullptr && count.last == nullptr);  // a counting pass hands out nothing to use
  const size_t total = counting.off;
  CHECK(total % 256 == 0 && total == 512 + 256 + 0 + 256 + 512 + 512);

  Arena ws;
  CHECK(ws.plan([&](Arena& a) { layout(a, real, 1); }) == 0);
  CHECK(ws.cap == total && ws.off == total);  // capacity is the counted total, to the byte
  CHECK(real.offs == count.offs);
  const char* ptrs[] = {(char*)real.a, (char*)real.b, real.empty, real.one, (char*)real.c, real.last};
  for (int i = 0; i < 6; ++i) {
    CHECK(ptrs[i] != nullptr && (uintptr_t)ptrs[i] % 256 == 0);
    CHECK(ptrs[i] == ws.base + real.offs[i]);
  }
  CHECK(real.offs[3] == real.offs[2]);        // the empty buffer takes no room
  CHECK(real.offs[4] == real.offs[3] + 256);  // one byte takes one 256-byte unit
  memset(real.a, 1, (100 + 1) * sizeof(float));
  memset(real.c, 2, 33 * sizeof(double));
  real.last[real.last_n - 1] = 3;                   // the last buffer's final byte
  ws.base[total - 1] = 4;                           // and the arena's
  CHECK(ws.get<char>(0) == ws.base + total);        // nothing more fits but nothing
  CHECK(ws.get<char>(1) == nullptr);

  // one byte less: the get that does not fit is refused, and the offset still shows what was asked for
  {
    Arena small;
    small.base = ws.base;
    small.cap = total - 1;
    Bufs u;
    layout(small, u, 1);
    CHECK(u.c != nullptr && u.last == nullptr);
    CHECK(small.off == total && small.off > small.cap);
  }

  // ---- growth: a larger plan replaces the block, a smaller one leaves cap and base alone
  {
    const int allocs0 = svc::g_allocs;
    Bufs big;
    CHECK(ws.plan([&](Arena& a) { layout(a, big, 3); }) == 0);
    CHECK(svc::g_allocs == allocs0 + 1 && ws.cap > total && ws.off == ws.cap);
    big.last[big.last_n - 1] = 5;
    const size_t cap_big = ws.cap;
    char* base_big = ws.base;
    Bufs again;
    CHECK(ws.plan([&](Arena& a) { layout(a, again, 1); }) == 0);
    CHECK(svc::g_allocs == allocs0 + 1 && ws.cap == cap_big && ws.base == base_big);
    CHECK(again.offs == count.offs && ws.off == total && again.a == (float*)base_big);
  }

  // ---- a layout that differs between its passes is an error, in either direction, and overruns nothing
  for (int more = 0; more < 2; ++more) {
    Arena w2;
    int pass = 0;
    char* p = nullptr;
    svc::g_err[0] = 0;
    const int st = w2.plan([&](Arena& a) {
      const bool second = pass++ == 1;
      p = a.get<char>(second ? (more ? 1000 : 10) : 500);
    });
    CHECK(st == SVC_ERR_STATE && pass == 2);
    CHECK(strstr(svc::g_err, "workspace layout") != nullptr);
    CHECK(w2.cap == 512);
    CHECK(more ? p == nullptr : p == w2.base);
    free(w2.base);
  }
  // an empty layout plans nothing
  {
    Arena w3;
    CHECK(w3.plan([](Arena&) {}) == 0 && w3.base == nullptr && w3.cap == 0);
  }
  free(ws.base);
  if (g_fail) return 1;
  printf("arena_check: ok\n");
  return 0;
}
