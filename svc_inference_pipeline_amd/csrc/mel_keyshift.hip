// The key-shifted log-mel (svc_mel_keyshift): the 24 kHz log-mel of features.hip with utterance b's STFT window and
// transform length stretched to n_new = rint(n_fft * factor[b]), the hop held (Diff-SVC's key-shifted mel; the
// reference's utils/mel.py:43-117 get_mel(keyshift=) also stretches the hop, which changes the frame count). The first
// n_fft / 2 + 1 bins are kept (zeros where n_new / 2 < n_fft / 2), scaled by n_fft / n_new, and go through the
// context's filterbank and log: harmonics at f0 land where a voice at factor * f0 has them, so shallow diffusion's start
// state agrees with the shifted F0 the conditioner sees.
// factor is device memory and n_new any integer in [n_fft / 2, 2 n_fft], so no radix plan fits: a direct DFT. One
// workgroup takes FR consecutive frames of one utterance:
//   1. the utterance's twiddles W^m = (cos, -sin)(2 pi m / n_new), m < n_new, by sincospi in f64 -> LDS, a linear
//      table (step 3's stride-k reads meet about 3 ways on a bank, what a random gather would; an XOR swizzle measured
//      no fewer and costs two instructions per read: DESIGN.md);
//   2. the FR windowed frames -> LDS as f64, frame-interleaved ([j][FR]: step 3 reads one 64-B broadcast per j); the
//      periodic Hann window comes from the cosines of step 1, the multiply is f32 as in dft_mel_kernel;
//   3. thread t owns bins 1 + t and 1 + NT + t: over j it carries each bin's phase index (k j) mod n_new as an integer
//      (add k, subtract n_new on overflow: exact phases, no sincos in the loop); the input is real, so a (k, j) pair is
//      two f64 FMAs per frame, and one twiddle read serves all FR frames. Bin 0 is a plain sum: 32 lanes per frame;
//   4. |X| (spec_value, f32) * n_fft / n_new -> LDS over the frames, then dft_mel_kernel's filterbank and log.
#include "common.h"
#include "kernels.h"
#include "spectral.h"

namespace svc {

constexpr int KS_FR = 8, KS_NT = 256;
static_assert(KS_FR * 32 == KS_NT, "bin 0: 32 lanes per frame");

// n_new of utterance b and its info word (bit 0: factor not finite or <= 0, taken as 1; bit 1: clamped)
__device__ __forceinline__ int ks_n_new(double f, int n, int* info) {
  *info = 0;
  if (!(f > 0.0) || isinf(f)) {  // NaN too
    *info = 1;
    return n;
  }
  const double r = rint((double)n * f);  // half to even
  if (r < (double)(n / 2)) {
    *info = 2;
    return n / 2;
  }
  if (r > (double)(2 * n)) {
    *info = 2;
    return 2 * n;
  }
  return (int)r;
}

// step 3 for NB bins per thread (k[i] == 0: none, its sums are not used)
template <int NB>
__device__ __forceinline__ void ks_dft(const double* __restrict__ xs, const double2* __restrict__ tw, int n_new,
                                       const int* k, double (*re)[KS_FR], double (*im)[KS_FR]) {
  int idx[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    idx[i] = 0;
#pragma unroll
    for (int f = 0; f < KS_FR; ++f) re[i][f] = im[i][f] = 0.0;
  }
  // one wave per SIMD (the workgroup holds the CU's LDS), so nothing else hides an LDS read: sample j + 1's reads are
  // issued before sample j's FMAs (two register sets, the loop unrolled by hand over them; sched_barrier keeps the
  // reads ahead), and their latency is behind 32 f64 FMAs instead of in front of them
  double2 xa[KS_FR / 2], wa[NB], xb[KS_FR / 2], wb[NB];
  // the next sample's phase indices, then its reads (past the end: the last sample once more, not used)
  const auto load = [&](int j, double2* xv, double2* wv) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      idx[i] += k[i];
      idx[i] = min((unsigned)idx[i], (unsigned)(idx[i] - n_new));  // -= n_new where idx >= n_new
    }
    const double2* xp = reinterpret_cast<const double2*>(xs + (size_t)min(j, n_new - 1) * KS_FR);
#pragma unroll
    for (int f = 0; f < KS_FR / 2; ++f) xv[f] = xp[f];
#pragma unroll
    for (int i = 0; i < NB; ++i) wv[i] = tw[idx[i]];
    __builtin_amdgcn_sched_barrier(0);
  };
  const auto fmas = [&](const double2* xv, const double2* wv) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
#pragma unroll
      for (int f = 0; f < KS_FR / 2; ++f) {
        re[i][2 * f] = fma(xv[f].x, wv[i].x, re[i][2 * f]);
        im[i][2 * f] = fma(xv[f].x, wv[i].y, im[i][2 * f]);
        re[i][2 * f + 1] = fma(xv[f].y, wv[i].x, re[i][2 * f + 1]);
        im[i][2 * f + 1] = fma(xv[f].y, wv[i].y, im[i][2 * f + 1]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
#pragma unroll
  for (int f = 0; f < KS_FR / 2; ++f) xa[f] = reinterpret_cast<const double2*>(xs)[f];
#pragma unroll
  for (int i = 0; i < NB; ++i) wa[i] = tw[0];  // W^0
  int j = 0;
  for (; j + 1 < n_new; j += 2) {
    load(j + 1, xb, wb);
    fmas(xa, wa);
    load(j + 2, xa, wa);
    fmas(xb, wb);
  }
  if (j < n_new) fmas(xa, wa);  // n_new odd
}

__global__ __launch_bounds__(KS_NT) void mel_keyshift_kernel(KeyshiftArgs a) {
  constexpr int FR = KS_FR, NT = KS_NT;
  extern __shared__ __align__(16) unsigned char dsm[];
  const int n = a.n_fft, nb = n / 2 + 1;
  double2* tw = reinterpret_cast<double2*>(dsm);                       // [2 n] slots, n_new in use
  double* xs = reinterpret_cast<double*>(dsm + (size_t)2 * n * 16);    // [n_new][FR] windowed frames
  float* sp = reinterpret_cast<float*>(xs);                            // after step 3: [FR][nb] |X| ...
  float* fbs = sp + FR * nb;                                           // ... and the packed filterbank bands
  const int f0 = blockIdx.x * FR;
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  int info;
  const int n_new = ks_n_new(a.factor[b], n, &info);
  if (a.info && blockIdx.x == 0 && tid == 0) a.info[b] = info;
  const int n_frames = a.Tb ? min(a.n_frames, a.Tb[b]) : a.n_frames;
  if (f0 >= n_frames) return;  // block-uniform, before any barrier (zero_tail_rows clears those rows)
  const int nf = min(FR, n_frames - f0);
  const float* w = a.wav + (int64_t)b * a.wav_stride;
  const int64_t len = a.nb ? a.nb[b] : a.n_samples;
  // 1. twiddles
  for (int m = tid; m < n_new; m += NT) {
    double sn, cs;
    sincospi((double)(2 * m) / (double)n_new, &sn, &cs);
    tw[m] = make_double2(cs, -sn);
  }
  __syncthreads();
  // 2. frames: sample j of frame t is wav[t hop + j - (n_new - hop) / 2], reflected once at either end of the
  // utterance's own length (the host checked that one reflection of the widest window stays inside)
  const int pad = (n_new - a.hop) / 2;
  for (int j = tid; j < n_new; j += NT) {
    const float wj = (float)(0.5 - 0.5 * tw[j].x);
#pragma unroll
    for (int fr = 0; fr < FR; ++fr) {
      float x = 0.f;
      if (fr < nf) {
        int64_t idx = (int64_t)(f0 + fr) * a.hop + j - pad;
        if (idx < 0) idx = -idx;
        if (idx >= len) idx = 2 * (len - 1) - idx;
        x = (idx >= 0 && idx < len) ? w[idx] : 0.f;
      }
      xs[(size_t)j * FR + fr] = (double)(x * wj);
    }
  }
  __syncthreads();
  // 3. bins 0 .. K - 1, K = min(n, n_new) / 2 + 1
  const int K = min(n, n_new) / 2 + 1;
  const int k[2] = {1 + tid < K ? 1 + tid : 0, 1 + NT + tid < K ? 1 + NT + tid : 0};
  double re[2][FR], im[2][FR];
  if (K > 1 + NT) ks_dft<2>(xs, tw, n_new, k, re, im);  // block-uniform
  else ks_dft<1>(xs, tw, n_new, k, re, im);
  double dc = 0.0;  // bin 0 of frame tid / 32
  for (int j = tid & 31; j < n_new; j += 32) dc += xs[(size_t)j * FR + (tid >> 5)];
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) dc += __shfl_xor(dc, o);
  __syncthreads();  // xs is read: sp and fbs take its place
  // 4. magnitudes, rescaled; bins past n_new / 2 are exact zeros
  const bool scaled = n_new != n;
  const float sn = (float)n, sd = (float)n_new;
  const auto mag = [&](double r, double i) {
    float m = spec_value(r, i, 0);
    if (scaled) m = m * sn / sd;
    return m;
  };
  if ((tid & 31) == 0) sp[(tid >> 5) * nb] = mag(dc, 0.0);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (k[i] == 0 || (i == 1 && K <= 1 + NT)) continue;
#pragma unroll
    for (int f = 0; f < FR; ++f) sp[f * nb + k[i]] = mag(re[i][f], im[i][f]);
  }
  for (int i = tid; i < FR * (nb - K); i += NT) {
    const int f = i / (nb - K);
    sp[f * nb + K + (i - f * (nb - K))] = 0.f;
  }
  for (int i = tid; i < a.fb_len; i += NT) fbs[i] = a.fb[i];
  __syncthreads();
  const int64_t row0 = (int64_t)b * a.n_frames + f0;
  for (int i = tid; i < nf * a.n_mels; i += NT) {
    const int f = i / a.n_mels, m = i - f * a.n_mels;
    const int lo = a.band[3 * m], hi = a.band[3 * m + 1];
    const float* fbm = fbs + a.band[3 * m + 2] - lo;
    const float* x = sp + f * nb;
    float acc = 0.f;
    for (int kk = lo; kk < hi; ++kk) acc = fmaf(fbm[kk], x[kk], acc);
    a.out[row0 * a.n_mels + i] = logf(fmaxf(acc, 1e-5f));
  }
}

int mel_keyshift(const KeyshiftArgs& a, int B, hipStream_t s) {
  SVC_REQUIRE((a.n_fft == 512 || a.n_fft == 1024) && a.hop > 0 && a.hop <= a.n_fft / 2 && a.n_frames > 0 && a.fb &&
                  a.band && a.n_mels > 0 && a.fb_len > 0 && a.factor && a.wav && a.out && B > 0,
              "mel_keyshift: n_fft=%d hop=%d frames=%d mels=%d", a.n_fft, a.hop, a.n_frames, a.n_mels);
  const size_t tw_bytes = (size_t)2 * a.n_fft * 16, xs_bytes = (size_t)KS_FR * 2 * a.n_fft * 8;
  SVC_REQUIRE(((size_t)KS_FR * (a.n_fft / 2 + 1) + a.fb_len) * 4 <= xs_bytes && tw_bytes + xs_bytes <= 160 * 1024,
              "mel_keyshift: %zu B of LDS, filterbank of %d floats", tw_bytes + xs_bytes, a.fb_len);
  if (int st = ensure_dyn_lds((const void*)mel_keyshift_kernel, 160 * 1024)) return st;
  KeyshiftArgs p = a;
  hipLaunchKernelGGL(mel_keyshift_kernel, dim3(cdiv(a.n_frames, KS_FR), B), dim3(KS_NT), tw_bytes + xs_bytes, s, p);
  SVC_LAUNCH_CHECK();
  return SVC_OK;
}

}  // namespace svc
