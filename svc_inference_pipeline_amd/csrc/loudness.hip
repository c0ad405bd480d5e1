// Loudness envelope transfer (so-vits-svc's "loudness envelope adjustment", per-frame form): the vocoder output takes
// the source's slow RMS envelope. Two memory-bound launches over a ragged batch; the arithmetic is
// audio.loudness_match's (DESIGN.md "Loudness envelope transfer"):
//   K     = 1 + n_out / H frames for both signals; frame k covers samples [kH - W/2, kH - W/2 + W), zero outside [0, n)
//   P_k   = (sum (double)s^2) / W,  E_k = sqrt(P_k)
//   g_k   = pow(E1_k / max(E2_k, floor_rms), 1 - mix), capped at max_gain when that is > 0      (1 source, 2 output)
//   out_i = (float)((double)y_i * (g_k0 + frac * (g_k1 - g_k0))),  k0 = i / H, frac = (i - k0 H) / H, k1 = min(k0 + 1, K - 1)
// Every product (double)s * (double)s is exact (48 significant bits), so the only freedom in P_k is the order of the f64
// additions: it is fixed by the frame's own sample range (below), never by the batch or by a pointer's alignment. The
// lerp is written as the host writes it, multiply then add: no contraction in this file.
#include "../../include/svc_hip.h"
#include "common.h"
#include "kernels.h"
#include "prims.h"

#pragma clang fp contract(off)

namespace svc {

namespace {

constexpr int kThreads = 256;
constexpr int kSpan = 2048;  // samples of one clip per apply block: two 16-byte chunks per thread
// gains one apply block needs: frames i / H of its samples and one more for the lerp's right end. H = 1 is the worst
// case, kSpan + 1 (for any H it is at most (kSpan - 2) / H + 3)
constexpr int kGainsMax = kSpan + 2;

// power[(sig * B + b) * K_max + k] = P_k of signal sig (0: the source, 1: the output) of clip b, 0 for k >= K_b.
// One block per (k, b, sig). The frame's samples inside the signal are [lo, hi); thread t adds, in ascending order, the
// squares of samples lo + 4 q .. lo + 4 q + 3 for q = t, t + 256, ...; then the 64-lane butterfly, then the four waves'
// sums in wave order. lo, hi and so the whole order follow from k, H, W and the signal's own length.
__global__ __launch_bounds__(kThreads) void loudness_power_kernel(const float* src, int64_t S_src, const float* wav,
                                                                  int64_t S, const int64_t* __restrict__ n_out,
                                                                  const int64_t* __restrict__ n_src, int B, int K_max,
                                                                  int W, int H, double* __restrict__ power) {
  const int k = blockIdx.x % K_max;
  const int bs = blockIdx.x / K_max;  // sig * B + b
  const int sig = bs / B, b = bs - sig * B;
  const int tid = threadIdx.x;
  const int64_t K = 1 + n_out[b] / H;
  const int64_t n = sig ? n_out[b] : n_src[b];
  const float* row = sig ? wav + (int64_t)b * S : src + (int64_t)b * S_src;
  const int64_t start = (int64_t)k * H - W / 2;
  const int64_t lo = start > 0 ? start : 0;
  const int64_t hi = start + W < n ? start + W : n;
  double acc = 0.0;
  if (k < K) {
    for (int64_t i0 = lo + 4 * (int64_t)tid; i0 < hi; i0 += 4 * kThreads) {
      float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // a zero adds nothing: acc + 0 = acc
      if (i0 + 4 <= hi) {
        load4(row, i0, n, x);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i0 + j < hi) x[j] = row[i0 + j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += (double)x[j] * (double)x[j];
    }
  }
  acc = wave_sum(acc);
  __shared__ double wave_acc[kThreads / 64];
  if ((tid & 63) == 0) wave_acc[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double p = wave_acc[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) p += wave_acc[w];
    power[(int64_t)bs * K_max + k] = p / (double)W;
  }
}

// g_k of clip b from the two power rows (k < K_b)
__device__ __forceinline__ double frame_gain(const double* __restrict__ p_src, const double* __restrict__ p_out, int64_t k,
                                             double expo, double floor_rms, double max_gain) {
  const double e1 = sqrt(p_src[k]);
  const double e2 = sqrt(p_out[k]);
  double g = pow(e1 / (e2 > floor_rms ? e2 : floor_rms), expo);
  if (max_gain > 0.0 && g > max_gain) g = max_gain;
  return g;
}

// out[b][i] = the adjusted sample for i < n_out[b], 0 from there to S. Block (b, blk) takes samples
// [blk * kSpan, min(.. + kSpan, S)) of row b: it computes the gains of the frames those samples touch once into LDS,
// then streams the span in 16-byte chunks that start on 16-byte boundaries of `out` (rows may start at any 4-byte
// boundary: the first and last chunk of a span are partial and stored sample by sample). Each sample is read and then
// written by one thread, so out may be wav itself. gain_out [B][K_out] (optional): the block also writes g_k of the
// frames whose first hop sample lies in its span (the row's last block: all that remain), 0 for k >= K_b.
__global__ __launch_bounds__(kThreads) void loudness_apply_kernel(const float* wav, int64_t S,
                                                                  const int64_t* __restrict__ n_out, int B, int K_max,
                                                                  int H, const double* __restrict__ power, double mix,
                                                                  double floor_rms, double max_gain, int blocks_per_row,
                                                                  float* out, double* __restrict__ gain_out,
                                                                  int64_t K_out) {
  const int b = blockIdx.x / blocks_per_row;
  const int blk = blockIdx.x - b * blocks_per_row;
  const int tid = threadIdx.x;
  const int64_t n = n_out[b];
  const int64_t K = 1 + n / H;
  const int64_t s0 = (int64_t)blk * kSpan;
  const int64_t s1 = s0 + kSpan < S ? s0 + kSpan : S;
  const double* p_src = power + (int64_t)b * K_max;
  const double* p_out = power + ((int64_t)B + b) * K_max;
  const double expo = 1.0 - mix;
  __shared__ double gains[kGainsMax];
  const int64_t k_first = s0 / H;
  const uint32_t r_first = (uint32_t)(s0 - k_first * H);  // s0's offset in its hop, < H
  if (s0 < n) {
    const int64_t e = s1 < n ? s1 : n;
    const int64_t k_last = (e - 1) / H + 1 < K - 1 ? (e - 1) / H + 1 : K - 1;
    const int cnt = (int)(k_last - k_first + 1);  // <= kSpan + 1
    for (int j = tid; j < cnt && j < kGainsMax; j += kThreads)
      gains[j] = frame_gain(p_src, p_out, k_first + j, expo, floor_rms, max_gain);
  }
  if (gain_out) {
    const int64_t ka = (s0 + H - 1) / H;
    const int64_t kb = blk == blocks_per_row - 1 ? K_out : (s1 + H - 1) / H;
    for (int64_t k = ka + tid; k < kb; k += kThreads)
      gain_out[(int64_t)b * K_out + k] = k < K ? frame_gain(p_src, p_out, k, expo, floor_rms, max_gain) : 0.0;
  }
  __syncthreads();
  const float* row = wav + (int64_t)b * S;
  float* orow = out + (int64_t)b * S;
  const int off = (int)((reinterpret_cast<uintptr_t>(orow + s0) >> 2) & 3);
  const int rel_last = (int)(K - 1 - k_first);  // the lerp's k1 clamp, relative to gains[0]
  for (int q = tid; q <= kSpan / 4; q += kThreads) {
    const int64_t j0 = s0 - off + 4 * (int64_t)q;  // < s0 in the span's first chunk
    if (j0 >= s1) break;
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool whole = j0 >= s0 && j0 + 4 <= s1;
    if (whole && j0 + 4 <= n) {
      load4(row, j0, n, x);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j0 + j >= s0 && j0 + j < s1 && j0 + j < n) x[j] = row[j0 + j];
    }
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      y[j] = 0.0f;
      const int64_t i = j0 + j;
      if (i >= s0 && i < s1 && i < n) {  // i - s0 < kSpan
        const uint32_t r = r_first + (uint32_t)(i - s0);
        const uint32_t dk = r / (uint32_t)H;
        const double frac = (double)(r - dk * (uint32_t)H) / (double)H;
        const int k0 = (int)dk, k1 = k0 + 1 < rel_last ? k0 + 1 : rel_last;
        const double g0 = gains[k0], g1 = gains[k1];
        y[j] = (float)((double)x[j] * (g0 + frac * (g1 - g0)));
      }
    }
    if (whole) {
      *reinterpret_cast<float4*>(orow + j0) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j0 + j >= s0 && j0 + j < s1) orow[j0 + j] = y[j];
    }
  }
}

}  // namespace

// The per-call device table: int64 n_out[B], int64 n_src[B] (staged by the caller, stream-ordered before
// loudness_match()), then the f64 frame powers [2][B][K_max], which the first launch writes whole.
size_t loudness_lens_bytes(int B) { return (size_t)B * 16; }
size_t loudness_power_bytes(int B, int64_t K_max) { return (size_t)2 * B * (size_t)K_max * 8; }

// wav f32 [B][S], src f32 [B][S_src] -> out f32 [B][S] (out == wav allowed). table: as above (device); K_max =
// 1 + (largest n_out) / hop (host). gain_out: optional device f64 [B][K_out].
int loudness_match(const float* wav, const float* src, int B, int64_t S, int64_t S_src, void* table, int64_t K_max,
                   int window, int hop, double mix, double floor_rms, double max_gain, float* out, double* gain_out,
                   int64_t K_out, hipStream_t s) {
  const int64_t* n_out = reinterpret_cast<const int64_t*>(table);
  const int64_t* n_src = n_out + B;
  double* power = reinterpret_cast<double*>(reinterpret_cast<char*>(table) + loudness_lens_bytes(B));
  const int64_t bpr = cdiv64(S, kSpan);
  SVC_REQUIRE(2 * (int64_t)B * K_max < (1ll << 31) && bpr * B < (1ll << 31),
              "loudness_match: batch of %d x %lld samples at hop %d too large", B, (long long)S, hop);
  {
    const int tok = prof_begin("loudness_power", 0.0, 2.0 * B * (double)K_max * (double)window * 4.0, s);
    hipLaunchKernelGGL(loudness_power_kernel, dim3((unsigned)(2 * (int64_t)B * K_max)), dim3(kThreads), 0, s, src, S_src,
                       wav, S, n_out, n_src, B, (int)K_max, window, hop, power);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
  }
  const int tok = prof_begin("loudness_apply", 0.0, (double)B * (double)S * 8.0, s);
  hipLaunchKernelGGL(loudness_apply_kernel, dim3((unsigned)(bpr * B)), dim3(kThreads), 0, s, wav, S, n_out, B,
                     (int)K_max, hop, power, mix, floor_rms, max_gain, (int)bpr, out, gain_out, K_out);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  return SVC_OK;
}

}  // namespace svc

extern "C" int64_t svc_loudness_frames(int64_t n_out, int hop) {
  if (n_out < 0 || hop < 1) return -1;
  return 1 + n_out / hop;
}
