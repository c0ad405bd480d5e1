// The pooled voiced median's kernels (svc_f0_voiced_median; elementwise.hip launches them) and the order-preserving
// keys they share with pitch_shift_kernel. A header, so that tools/median_ab.hip can time the counting forms side by
// side: the library itself instantiates the measured one only (kMedianRounds).
#pragma once
#include "common.h"

namespace svc {

// Cells of the flattened [B * T] input per workgroup of a pass: 256 threads x 8 cells. A pooled input of 4096 cells
// is two workgroups already; the reference's 223,087 target frames are 109.
constexpr int kMedianTile = 2048;
// stream operations per call: one clear of the histograms, 8 digit passes, the final step
constexpr int kMedianLaunches = 10;
// the counting form the library runs (median_count's ROUNDS; tools/median_ab.hip times 0, 1, 2 and 4): one LDS atomic
// per cell. Wave aggregation measured no faster at any size tried (223,087 cells: 46.6 us a call plain, 49.7 / 56.6 /
// 58.5 us with 1 / 2 / 4 rounds; 8 M cells: 250.0 against 250.1 / 257.4 / 260.3 us; DESIGN.md "A4 per singer")
constexpr int kMedianRounds = 0;

__device__ __forceinline__ uint64_t dkey(double v) {
  uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// ============================================================================ pooled voiced median
// np.median of every voiced (nonzero) cell of a ragged batch, pooled (utils/acoustic_feature_extraction.py:21-30
// get_target_f0_median): a radix select over dkey()'s keys in 8 digit passes of 8 bits, most significant first, on as
// many workgroups as the data has tiles of kMedianTile cells. A pass is a kernel: every workgroup first resolves the
// pass before it from that pass's finished global histogram (the same integers in every workgroup, so the same
// answer), then counts the digit of each cell that still matches the chosen prefix into a histogram in LDS and adds
// that into the pass's global histogram with integer atomics. Both ranks of an even count, (n - 1) / 2 and n / 2
// (n = the total of pass 0's histogram), ride the same sweeps: they share a histogram until their prefixes part,
// from where the upper rank has its own. No workgroup waits for another inside a kernel; the counts are integers, so
// the result does not depend on the order of arrival.
struct MedianState {
  uint64_t prefix[2];  // chosen digits of the lower / upper rank so far (high bits)
  uint32_t k[2];       // their ranks among the cells that match the prefix
  uint32_t n;          // pooled voiced count
  uint32_t pad_;
};
constexpr int kMedianPasses = 8;
constexpr int kMedianBins = 256;
constexpr size_t kMedianHistWords = (size_t)kMedianPasses * 2 * kMedianBins;
constexpr int kMedianItems = kMedianTile / 256;  // cells per thread

// inclusive prefix sum of one value per thread over the 256 threads of the workgroup
__device__ __forceinline__ uint32_t scan256(uint32_t v, uint32_t* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t x = v;
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  for (int i = 0; i < w; ++i) x += wsum[i];
  return x;
}

// The state after pass `pass` from the state before it (`in`; pass 0: none) and its histogram hist [2][256]; every
// thread of the workgroup returns the same value. sh: 8 words of LDS.
__device__ inline MedianState median_resolve(const MedianState* in, const uint32_t* __restrict__ hist, int pass, uint32_t* sh) {
  MedianState st;
  if (pass == 0) {
    st.prefix[0] = st.prefix[1] = 0;
    st.k[0] = st.k[1] = 0;
    st.n = 0;
  } else {
    st = *in;
    if (st.n == 0) return st;
  }
  const bool split = st.prefix[0] != st.prefix[1];
  const uint32_t c0 = hist[threadIdx.x];
  const uint32_t i0 = scan256(c0, sh);
  if (pass == 0) {
    if (threadIdx.x == 255) sh[4] = i0;
    __syncthreads();
    st.n = sh[4];
    if (st.n == 0) return st;
    st.k[0] = (st.n - 1) / 2;
    st.k[1] = st.n / 2;
  }
  uint32_t c1 = c0, i1 = i0;
  if (split) {
    c1 = hist[kMedianBins + threadIdx.x];
    i1 = scan256(c1, sh);
  }
  __syncthreads();
  // exactly one bin holds each rank: cells below it <= k < cells up to and including it
  if (i0 - c0 <= st.k[0] && st.k[0] < i0) {
    sh[4] = threadIdx.x;
    sh[5] = st.k[0] - (i0 - c0);
  }
  if (i1 - c1 <= st.k[1] && st.k[1] < i1) {
    sh[6] = threadIdx.x;
    sh[7] = st.k[1] - (i1 - c1);
  }
  __syncthreads();
  const int shift = 56 - 8 * pass;
  st.prefix[0] |= (uint64_t)sh[4] << shift;
  st.k[0] = sh[5];
  st.prefix[1] |= (uint64_t)sh[6] << shift;
  st.k[1] = sh[7];
  return st;
}

// One more cell of digit `digit` (where active) into the LDS histogram h; every lane of the wave calls it.
// ROUNDS = 0: one LDS atomic per active lane. ROUNDS > 0 (the measured alternative): the lanes whose digit equals the
// first active lane's are counted with a ballot and added once, for up to ROUNDS distinct digits (voiced F0 shares its
// sign and most of its exponent, so the top passes hit a handful of bins); lanes still left then add one each.
template <int ROUNDS>
__device__ __forceinline__ void median_count(uint32_t* h, bool active, uint32_t digit) {
  if (ROUNDS > 0) {
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int r = 0; r < ROUNDS; ++r) {
      const unsigned long long act = __ballot(active);
      if (!act) return;
      const int leader = __ffsll(act) - 1;
      const uint32_t ld = (uint32_t)__shfl((int)digit, leader);
      const bool mine = active && digit == ld;
      const unsigned long long m = __ballot(mine);
      if (lane == leader) atomicAdd(&h[ld], (uint32_t)__popcll(m));
      if (mine) active = false;
    }
  }
  if (active) atomicAdd(&h[digit], 1u);
}

// pass `pass` of the select. hist: [kMedianPasses][2][256], zero before pass 0; state: [kMedianPasses + 1], entry p
// the state before pass p (entry 0 unused), written by workgroup 0. frames: device int32 [B] or NULL.
template <int ROUNDS>
__global__ __launch_bounds__(256) void median_pass_kernel(const double* __restrict__ f0, int T, int64_t total,
                                                          const int* __restrict__ frames, uint32_t* hist,
                                                          MedianState* state, int pass) {
  __shared__ uint32_t lh[2][kMedianBins];
  __shared__ uint32_t sh[8];
  MedianState st;
  st.prefix[0] = st.prefix[1] = 0;
  st.n = 1;
  if (pass > 0) {
    st = median_resolve(&state[pass - 1], hist + (size_t)(pass - 1) * 2 * kMedianBins, pass - 1, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[pass] = st;
    if (st.n == 0) return;
  }
  const bool split = st.prefix[0] != st.prefix[1];
  lh[0][threadIdx.x] = 0;
  lh[1][threadIdx.x] = 0;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  // the bits above this pass's digit (none in pass 0)
  const uint64_t mask = pass ? ~0ull << (shift + 8) : 0ull;
  const int64_t base = (int64_t)blockIdx.x * kMedianTile;
#pragma unroll 1
  for (int j = 0; j < kMedianItems; ++j) {
    const int64_t i = base + (int64_t)j * 256 + threadIdx.x;
    bool in = i < total;
    double v = 0.0;
    if (in) {
      if (frames) {
        const uint32_t b = (uint32_t)i / (uint32_t)T;  // total < 2^31
        in = (int)((uint32_t)i - b * (uint32_t)T) < frames[b];
      }
      if (in) v = f0[i];
    }
    const bool voiced = in && v != 0.0;
    const uint64_t key = dkey(v);
    const uint32_t digit = (uint32_t)(key >> shift) & 0xFFu;
    median_count<ROUNDS>(lh[0], voiced && (key & mask) == st.prefix[0], digit);
    if (split) median_count<ROUNDS>(lh[1], voiced && (key & mask) == st.prefix[1], digit);
  }
  __syncthreads();
  uint32_t* g = hist + (size_t)pass * 2 * kMedianBins;
  if (lh[0][threadIdx.x]) atomicAdd(&g[threadIdx.x], lh[0][threadIdx.x]);
  if (split && lh[1][threadIdx.x]) atomicAdd(&g[kMedianBins + threadIdx.x], lh[1][threadIdx.x]);
}

// after the last pass both prefixes are whole keys: the median as pitch_shift_kernel forms it
static __global__ __launch_bounds__(256) void median_final_kernel(const uint32_t* hist, const MedianState* state,
                                                           double* median, long long* voiced) {
  __shared__ uint32_t sh[8];
  const MedianState st = median_resolve(&state[kMedianPasses - 1],
                                        hist + (size_t)(kMedianPasses - 1) * 2 * kMedianBins, kMedianPasses - 1, sh);
  if (threadIdx.x) return;
  if (voiced) *voiced = (long long)st.n;
  if (st.n == 0) {
    *median = __longlong_as_double(0x7FF8000000000000ll);  // np.median of an empty selection is NaN
    return;
  }
  double r[2];
  for (int q = 0; q < 2; ++q) {
    const uint64_t p = st.prefix[q];
    const uint64_t b = (p >> 63) ? (p & 0x7FFFFFFFFFFFFFFFull) : ~p;
    r[q] = __longlong_as_double((long long)b);
  }
  *median = (st.n & 1) ? r[0] : (r[0] + r[1]) / 2.0;
}

// Enqueues the kMedianLaunches operations of one select on s. hist: kMedianHistWords words, state: kMedianPasses + 1
// entries (device); ROUNDS: the counting form (median_count; DESIGN.md "A4 per singer" has the measurement).
template <int ROUNDS>
int median_enqueue(const double* f0, int B, int T, const int* frames_dev, uint32_t* hist, MedianState* state,
                   double* median, long long* voiced, hipStream_t s) {
  const int64_t total = (int64_t)B * T;
  SVC_HIP_CHECK(hipMemsetAsync(hist, 0, kMedianHistWords * sizeof(uint32_t), s));
  const dim3 grid((unsigned)((total + kMedianTile - 1) / kMedianTile));
  for (int p = 0; p < kMedianPasses; ++p) {
    hipLaunchKernelGGL(median_pass_kernel<ROUNDS>, grid, dim3(256), 0, s, f0, T, total, frames_dev, hist, state, p);
    SVC_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(median_final_kernel, dim3(1), dim3(256), 0, s, hist, state, median, voiced);
  SVC_LAUNCH_CHECK();
  return SVC_OK;
}

}  // namespace svc
