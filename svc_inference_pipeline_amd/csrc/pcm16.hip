// A16: save_audio's sample conversion (utils/util.py:20-37) on the device: per-utterance peak, scale to volume_peak,
// fs / 20 zeros on each side, round to 16-bit PCM. Two memory-bound launches over a ragged batch; the RIFF header and
// the file stay on the host (audio.write_wav_pcm16). The arithmetic is audio.to_pcm16's, bit for bit:
//   peak  = max |x| over the utterance's own samples
//   ratio = turn_up ? (float)(volume_peak / (double)peak) : 1.0f     (numpy: f32 array * Python float scalar)
//   q     = clip(rint((x * ratio) * 32768), -32768, 32767)            (x * ratio rounded to f32 first; * 2^15 is exact;
//                                                                       rint = round half to even, as np.round)
// so no factor is folded into another and the file is built without fast-math. A silent or empty utterance
// (peak 0) gives zeros where the host function divides by zero; non-finite input is undefined (svc_hip.h).
#include "../../include/svc_hip.h"
#include "common.h"
#include "kernels.h"

namespace svc {

namespace {

constexpr int kThreads = 256;
constexpr int kPeakChunk = 8192;  // samples of one utterance per peak block: 8 x 16-byte loads per thread
// u32 words between two utterances' peak words: a 128-byte line each. Device-scope atomics on one line serialise
// (32 x 239,872 samples: one atomic per wave into adjacent words 36 us, one per block 14.4 us, one per block into
// a line of its own 9.6 us, then the same for 4096 / 8192 / 16384-sample chunks; profiles/pcm16_peak_scratch_ab.txt)
constexpr int kPeakStride = 32;
constexpr int kQuantPer = 8;      // output samples per quantise thread: one 16-byte store

__device__ __forceinline__ unsigned abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// peak_bits[b * kPeakStride] = max over i < nb[b] of the bit pattern of |wav[b][i]| (non-negative floats order as unsigned integers,
// so the atomic maximum is exact and independent of the order in which blocks arrive). Block (b, chunk) reads samples
// [chunk * kPeakChunk, min(.., nb[b])) of row b only: a scalar head up to the first 16-byte boundary, 16-byte loads,
// a scalar tail. peak_bits is zero on entry.
__global__ __launch_bounds__(kThreads) void pcm16_peak_kernel(const float* __restrict__ wav, int64_t S,
                                                              const int64_t* __restrict__ nb, int blocks_per_row,
                                                              unsigned* __restrict__ peak_bits) {
  const int b = blockIdx.x / blocks_per_row;
  const int64_t lo = (int64_t)(blockIdx.x - b * blocks_per_row) * kPeakChunk;
  const int64_t n = nb[b];
  if (lo >= n) return;
  const int64_t hi = lo + kPeakChunk < n ? lo + kPeakChunk : n;
  const float* row = wav + (int64_t)b * S;
  const int tid = threadIdx.x;
  const int head = (int)((0 - (reinterpret_cast<uintptr_t>(row + lo) >> 2)) & 3);
  const int64_t a = lo + head < hi ? lo + head : hi;  // first 16-byte aligned sample (or hi)
  unsigned m = 0;
  if (lo + tid < a) m = abs_bits(row[lo + tid]);
  const int nvec = (int)((hi - a) >> 2);
  const float4* v = reinterpret_cast<const float4*>(row + a);
#pragma unroll 4
  for (int i = tid; i < nvec; i += kThreads) {
    const float4 x = v[i];
    m = umax(umax(m, abs_bits(x.x)), umax(abs_bits(x.y), umax(abs_bits(x.z), abs_bits(x.w))));
  }
  const int64_t t0 = a + 4 * (int64_t)nvec;
  if (t0 + tid < hi) m = umax(m, abs_bits(row[t0 + tid]));
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = umax(m, (unsigned)__shfl_xor((int)m, off));
  // one atomic per block
  __shared__ unsigned wave_max[kThreads / 64];
  if ((tid & 63) == 0) wave_max[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) m = umax(m, wave_max[w]);
    if (m) atomicMax(&peak_bits[b * kPeakStride], m);
  }
}

__device__ __forceinline__ int quantise(float x, float ratio) {
  const float v = x * ratio;
  float r = rintf(v * 32768.0f);
  r = fminf(fmaxf(r, -32768.0f), 32767.0f);
  return (int)r;
}

// pcm[b][j], j < L = S + 2 sil: sample i = j - sil of utterance b converted where 0 <= i < nb[b], zero elsewhere (the
// leading and trailing silence and the rest of the padded row). Thread chunks of 8 output samples start on 16-byte
// boundaries of the output (rows may start at any 2-byte boundary: the first and last chunk of a row are partial and
// stored sample by sample). The 8 input samples come from 16-byte loads too where the chunk lies inside the utterance:
// two when they are aligned, else the three aligned quads that cover them.
__global__ __launch_bounds__(kThreads) void pcm16_quant_kernel(const float* __restrict__ wav, int64_t S,
                                                               const int64_t* __restrict__ nb,
                                                               const unsigned* __restrict__ peak_bits,
                                                               int blocks_per_row, int sil, int64_t L, int turn_up,
                                                               double volume_peak, int16_t* __restrict__ pcm,
                                                               float* __restrict__ peak_out) {
  const int b = blockIdx.x / blocks_per_row;
  const int blk = blockIdx.x - b * blocks_per_row;
  int16_t* orow = pcm + (int64_t)b * L;
  const int off = (int)((reinterpret_cast<uintptr_t>(orow) >> 1) & 7);
  const int64_t j0 = ((int64_t)blk * kThreads + threadIdx.x) * kQuantPer - off;  // row-relative, < 0 in the first chunk
  const float peak = __uint_as_float(peak_bits[b * kPeakStride]);
  if (blk == 0 && threadIdx.x == 0 && peak_out) peak_out[b] = peak;
  if (j0 >= L) return;
  const float ratio = (turn_up && peak > 0.0f) ? (float)(volume_peak / (double)peak) : 1.0f;
  const int64_t n = nb[b];
  const int64_t i0 = j0 - sil;
  const float* row = wav + (int64_t)b * S;
  float x[kQuantPer];
#pragma unroll
  for (int k = 0; k < kQuantPer; ++k) x[k] = 0.0f;
  if (i0 >= 0 && i0 + kQuantPer <= n) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(row + i0) >> 2) & 3);
    if (mis == 0) {
      const float4 p = *reinterpret_cast<const float4*>(row + i0);
      const float4 q = *reinterpret_cast<const float4*>(row + i0 + 4);
      x[0] = p.x, x[1] = p.y, x[2] = p.z, x[3] = p.w, x[4] = q.x, x[5] = q.y, x[6] = q.z, x[7] = q.w;
    } else if (i0 - mis >= 0 && i0 - mis + 12 <= n) {
      const float4* a = reinterpret_cast<const float4*>(row + i0 - mis);
      const float4 p = a[0], q = a[1], r = a[2];
      const float t[12] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w, r.x, r.y, r.z, r.w};
      if (mis == 1) {
#pragma unroll
        for (int k = 0; k < kQuantPer; ++k) x[k] = t[k + 1];
      } else if (mis == 2) {
#pragma unroll
        for (int k = 0; k < kQuantPer; ++k) x[k] = t[k + 2];
      } else {
#pragma unroll
        for (int k = 0; k < kQuantPer; ++k) x[k] = t[k + 3];
      }
    } else {
#pragma unroll
      for (int k = 0; k < kQuantPer; ++k) x[k] = row[i0 + k];
    }
  } else if (i0 < n && i0 + kQuantPer > 0) {
#pragma unroll
    for (int k = 0; k < kQuantPer; ++k)
      if (i0 + k >= 0 && i0 + k < n) x[k] = row[i0 + k];
  }
  int q[kQuantPer];
#pragma unroll
  for (int k = 0; k < kQuantPer; ++k) q[k] = quantise(x[k], ratio);
  if (j0 >= 0 && j0 + kQuantPer <= L) {
    uint4 w;
    w.x = (unsigned)(q[0] & 0xffff) | ((unsigned)q[1] << 16);
    w.y = (unsigned)(q[2] & 0xffff) | ((unsigned)q[3] << 16);
    w.z = (unsigned)(q[4] & 0xffff) | ((unsigned)q[5] << 16);
    w.w = (unsigned)(q[6] & 0xffff) | ((unsigned)q[7] << 16);
    *reinterpret_cast<uint4*>(orow + j0) = w;
  } else {
#pragma unroll
    for (int k = 0; k < kQuantPer; ++k)
      if (j0 + k >= 0 && j0 + k < L) orow[j0 + k] = (int16_t)q[k];
  }
}

}  // namespace

// The per-call device table: int64 n[B] (samples per utterance), then the peak scratch, one u32 per utterance every
// kPeakStride words. The caller stages it whole, the scratch as zeros, stream-ordered before pcm16().
size_t pcm16_table_bytes(int B) { return (size_t)B * 8 + (size_t)B * kPeakStride * 4; }

// wav f32 [B][S] -> pcm int16 [B][L], L = S + 2 sil. table: as above (device), max_nb the largest n[b] (host). The
// scratch is left holding the bit patterns of the peaks (zeros when need_peak is 0: the peak pass is skipped).
// peak_out: optional device f32 [B].
int pcm16(const float* wav, int B, int64_t S, void* table, int64_t max_nb, int sil, int64_t L, int turn_up,
          double volume_peak, int16_t* pcm, float* peak_out, int need_peak, hipStream_t s) {
  const int64_t* nb = reinterpret_cast<const int64_t*>(table);
  unsigned* peak_bits = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(table) + (size_t)B * 8);
  const int64_t bpr_peak = cdiv64(max_nb, kPeakChunk);
  const int64_t bpr_quant = cdiv64((L + 7) / kQuantPer + 1, kThreads);  // chunks of a row whose start is misaligned by <= 7
  SVC_REQUIRE(bpr_peak * B < (1ll << 31) && bpr_quant * B < (1ll << 31), "pcm16: batch of %d x %lld samples too large", B,
              (long long)S);
  if (need_peak && bpr_peak > 0) {
    const int tok = prof_begin("pcm16_peak", 0.0, (double)B * (double)max_nb * 4.0, s);
    hipLaunchKernelGGL(pcm16_peak_kernel, dim3((unsigned)(bpr_peak * B)), dim3(kThreads), 0, s, wav, S, nb,
                       (int)bpr_peak, peak_bits);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
  }
  const int tok = prof_begin("pcm16_quant", 0.0, (double)B * ((double)max_nb * 4.0 + (double)L * 2.0), s);
  hipLaunchKernelGGL(pcm16_quant_kernel, dim3((unsigned)(bpr_quant * B)), dim3(kThreads), 0, s, wav, S, nb, peak_bits,
                     (int)bpr_quant, sil, L, turn_up, volume_peak, pcm, peak_out);
  prof_end(tok, s);
  SVC_LAUNCH_CHECK();
  return SVC_OK;
}

}  // namespace svc

extern "C" int64_t svc_pcm16_len(int64_t n_samples, int fs, int add_silence) {
  if (n_samples < 0 || fs < 1) return -1;
  return n_samples + 2 * (int64_t)(add_silence ? fs / 20 : 0);
}
