// (diagnostics) The pooled voiced median's histogram pass in its counting forms, side by side on one input:
//   plain         one LDS atomic per cell (median_pass_kernel<0>)
//   aggregated R  lanes that share the first active lane's digit are counted with a ballot and added once, for up to R
//                 distinct digits per wave-load, the lanes left over one by one (median_pass_kernel<R>, R = 1, 2, 4)
// Voiced F0 shares its sign and most of its exponent, so the top passes hit a handful of bins (csrc/median.h).
// The input is seeded: n cells, a `voiced` share of them log-uniform in 65..800 Hz, the rest 0. Every form must give the
// bits of the host's np.median restatement; each is then timed as whole calls (all 10 stream operations) in rounds
// that alternate the forms, and one JSON line is printed (per-call microseconds: the median over rounds, min, max).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Isvc_inference_pipeline_amd/csrc tools/median_ab.hip \
//       -o tools/median_ab && tools/median_ab [n=223087] [rounds=30] [calls=50] [voiced=0.78]
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "median.h"

namespace svc {
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
}  // namespace svc

#define CHECK(expr)                                                                   \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      fprintf(stderr, "%s:%d %s -> %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
      return 2;                                                                       \
    }                                                                                 \
  } while (0)

static double host_median(std::vector<double> v) {
  if (v.empty()) return NAN;
  const size_t n = v.size();
  std::nth_element(v.begin(), v.begin() + n / 2, v.end());
  const double hi = v[n / 2];
  if (n & 1) return hi;
  const double lo = *std::max_element(v.begin(), v.begin() + n / 2);
  return (lo + hi) / 2.0;
}

struct Stat {
  double med, lo, hi;
};
static Stat stat_of(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return {v[v.size() / 2], v.front(), v.back()};
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 223087;
  const int rounds = argc > 2 ? atoi(argv[2]) : 30;
  const int calls = argc > 3 ? atoi(argv[3]) : 50;
  const double share = argc > 4 ? atof(argv[4]) : 0.78;
  if (n < 1 || rounds < 1 || calls < 1) return 1;
  std::vector<double> h(n), voiced;
  uint64_t z = 0x9E3779B97F4A7C15ull;
  auto rnd = [&] {  // splitmix64 -> [0, 1)
    z += 0x9E3779B97F4A7C15ull;
    uint64_t x = z;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return (double)((x ^ (x >> 31)) >> 11) / 9007199254740992.0;
  };
  for (int i = 0; i < n; ++i) {
    h[i] = rnd() < share ? 65.0 * std::exp(rnd() * std::log(800.0 / 65.0)) : 0.0;
    if (h[i] != 0.0) voiced.push_back(h[i]);
  }
  const double want = host_median(voiced);

  double *d = nullptr, *med = nullptr;
  long long* cnt = nullptr;
  uint32_t* hist = nullptr;
  svc::MedianState* state = nullptr;
  CHECK(hipMalloc(&d, (size_t)n * 8));
  CHECK(hipMalloc(&med, 8));
  CHECK(hipMalloc(&cnt, 8));
  CHECK(hipMalloc(&hist, svc::kMedianHistWords * 4));
  CHECK(hipMalloc(&state, (svc::kMedianPasses + 1) * sizeof(svc::MedianState)));
  CHECK(hipMemcpy(d, h.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  hipStream_t s;
  CHECK(hipStreamCreate(&s));
  constexpr int kForms = 4;
  const char* names[kForms] = {"plain_us", "aggregated1_us", "aggregated2_us", "aggregated4_us"};
  auto run = [&](int form) {
    switch (form) {
      case 0: return svc::median_enqueue<0>(d, 1, n, nullptr, hist, state, med, cnt, s);
      case 1: return svc::median_enqueue<1>(d, 1, n, nullptr, hist, state, med, cnt, s);
      case 2: return svc::median_enqueue<2>(d, 1, n, nullptr, hist, state, med, cnt, s);
      default: return svc::median_enqueue<4>(d, 1, n, nullptr, hist, state, med, cnt, s);
    }
  };
  for (int form = 0; form < kForms; ++form) {  // same bits as the host, and the warm-up of both forms
    for (int i = 0; i < 10; ++i)
      if (run(form)) return 2;
    CHECK(hipStreamSynchronize(s));
    double got;
    long long c;
    CHECK(hipMemcpy(&got, med, 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&c, cnt, 8, hipMemcpyDeviceToHost));
    if (memcmp(&got, &want, 8) != 0 || c != (long long)voiced.size()) {
      fprintf(stderr, "form %d: median %.17g (%lld voiced), host %.17g (%zu)\n", form, got, c, want, voiced.size());
      return 3;
    }
  }
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<double> us[kForms];
  for (int r = 0; r < rounds; ++r)
    for (int form = 0; form < kForms; ++form) {
      CHECK(hipEventRecord(e0, s));
      for (int i = 0; i < calls; ++i)
        if (run(form)) return 2;
      CHECK(hipEventRecord(e1, s));
      CHECK(hipEventSynchronize(e1));
      float ms = 0.f;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      us[form].push_back(1e3 * ms / calls);
    }
  printf("{\"n\": %d, \"voiced\": %zu, \"workgroups\": %d, \"launches_per_call\": %d, \"rounds\": %d, "
         "\"calls_per_round\": %d, \"library_form\": \"%s\"",
         n, voiced.size(), (n + svc::kMedianTile - 1) / svc::kMedianTile, svc::kMedianLaunches, rounds, calls,
         names[svc::kMedianRounds == 4 ? 3 : svc::kMedianRounds]);
  for (int form = 0; form < kForms; ++form) {
    const Stat t = stat_of(us[form]);
    printf(", \"%s\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}", names[form], t.med, t.lo, t.hi);
  }
  printf("}\n");
  return 0;
}
