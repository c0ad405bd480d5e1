// A1: the input end of infer.py on the device. The data-chunk payloads of B wav files (one byte buffer, any byte
// offsets) -> the two ragged batches the pipeline consumes: the source waveform at the model rate
// (utils/audio.py:10-55 load_audio_torch -> audio.load_audio) and Whisper's 16 kHz mono int16-grid copy
// (utils/whisper_extractor/audio.py:22-49 load_audio -> audio.load_whisper_audio), and with svc_load_pcm_ex HuBERT /
// ContentVec's float mono copy at the same rate (utils/hubert.py:137-143 librosa.load(path, sr=16000) ->
// audio.load_contentvec_audio). At most three launches per call, whatever B is and whichever rows are asked for: the
// channel-0 peak (only when some utterance holds float samples), the source rows, the mono rows (both of them).
//
// The arithmetic restates the per-file host path bit for bit (each row is np.array_equal to that path on the file alone):
//   decode   audio.read_wav's f64 values: u8 (v - 128) / 128, s16 / 2^15, s24 / 2^23, s32 / 2^31, f32 / f64 as stored
//   source   channel 0; mx = max |x64| (NaN when a NaN is present, as np.amax gives); max_mag = 2^31 + 1 when
//            mx > 2^15, else 2^15 + 1 when mx > 1.01, else 1; x = (float)x64 / (float)max_mag, computed as the f64
//            quotient of the two floats rounded once (equal to the IEEE f32 division: f64 holds more than twice f32's
//            significand); a row whose rate already is sr_src holds these samples unfiltered
//   mono     numpy's mean over the channels in f64 (sequential sum for 1-7 channels, ((c0+c1)+(c2+c3))+((c4+c5)+(c6+c7))
//            for 8; then / channels), (float), the filter (also when up = down = 1), rint(v * 32768) clipped, / 32768
//   float    the same (float) means; a row at another rate than sr_mono holds the filter's (float)acc, the value the
//            mono row is about to round (audio.resample(quantize16=False)), a row already at sr_mono the means
//            themselves, unfiltered (librosa.load does not resample at the native rate)
//   filter   resample.hip's plan, index arithmetic and ascending-r sum, one fused multiply-add per tap in f64
//            (resample_kernel's loop compiles to v_fmac_f64; fma() is written out here), (float) at the end
// so nothing is folded or reordered and the file is built without fast-math.
//
// Shape: block (b, chunk) owns kChunk consecutive output samples of row b. It walks them in tiles (the plan's `tile`,
// the most outputs whose input span fits the LDS buffer), decodes a tile's input span once into LDS as f32 (s24 and
// misaligned payloads make per-tap decoding the expensive part) and reads its taps phase-major, so one thread's taps
// are contiguous. Outputs past the utterance's own length are written as zeros. The mono launch writes both mono rows
// from the one decoded tile and the one pass over the taps: v to the float row, the rounded v to the quantised row; an
// unfiltered float row copies the decoded mean out of the tile.
#include "../../include/svc_hip.h"
#include "common.h"
#include "kernels.h"

#include <numeric>
#include <vector>

namespace svc {

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 1024;      // output samples of one row per block
constexpr int kSpan = 8192;       // f32 input samples a tile may span (32 KiB of LDS)
constexpr int kPeakChunk = 4096;  // frames of one utterance per peak block (tests place peaks on its boundary)
constexpr int kPeakStride = 16;   // u64 words between two utterances' peak words: a 128-byte line each (pcm16.hip)

struct PcmUtt {
  int64_t off, frames, n_src, n_mono;  // payload byte offset, frames, output samples of the two rows
  int32_t fmt, ch, plan_src, plan_mono;  // plan index into the call's plan table; -1: the row is the decoded samples
  int32_t float_copy, pad_;              // the float mono row is the decoded means (the file already is at sr_mono)
};
struct PcmPlan {
  const double* hpm;
  int up, down, pre_remove, taps, per_phase, tile;
};

// sample `idx` (frame * channels + channel) of a payload as audio.read_wav's f64 value; byte loads: no alignment
__device__ __forceinline__ double decode(const uint8_t* __restrict__ p, int fmt, int64_t idx) {
  if (fmt == SVC_PCM_U8) return ((double)p[idx] - 128.0) / 128.0;
  if (fmt == SVC_PCM_S16) {
    const uint8_t* q = p + idx * 2;
    const int v = (int)(int16_t)((unsigned)q[0] | ((unsigned)q[1] << 8));
    return (double)v / 32768.0;
  }
  if (fmt == SVC_PCM_S24) {
    const uint8_t* q = p + idx * 3;
    const unsigned u = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
    const int v = (int)(u << 8) >> 8;
    return (double)v / 8388608.0;
  }
  const uint8_t* q = p + idx * (fmt == SVC_PCM_F64 ? 8 : 4);
  const unsigned lo = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
  if (fmt == SVC_PCM_S32) return (double)(int)lo / 2147483648.0;
  if (fmt == SVC_PCM_F32) return (double)__uint_as_float(lo);
  const unsigned hi = (unsigned)q[4] | ((unsigned)q[5] << 8) | ((unsigned)q[6] << 16) | ((unsigned)q[7] << 24);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// numpy's ndarray.mean(axis=1) of one frame: its pairwise sum (fewer than 8 elements: sequential from 0; exactly 8:
// eight partial sums combined as below), then the true division by the count
__device__ __forceinline__ double frame_mean(const uint8_t* __restrict__ p, int fmt, int ch, int64_t frame) {
  const int64_t base = frame * ch;
  double s;
  if (ch == 8) {
    double c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = decode(p, fmt, base + k);
    s = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
  } else {
    s = decode(p, fmt, base);
    for (int k = 1; k < ch; ++k) s += decode(p, fmt, base + k);
  }
  return s / (double)ch;
}

__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// peak_bits[b * kPeakStride] = max over the frames of utterance b of the bit pattern of |channel 0| as f64, for the
// utterances that hold float samples (integer formats cannot exceed 1: their word stays 0). Non-negative doubles order
// as unsigned integers, a NaN's pattern above +inf's, so the atomic maximum is exact, independent of the order in which
// blocks arrive, and NaN when a NaN is present (np.amax's answer). peak_bits is zero on entry.
__global__ __launch_bounds__(kThreads) void load_pcm_peak_kernel(const uint8_t* __restrict__ raw,
                                                                 const PcmUtt* __restrict__ utt, int blocks_per_row,
                                                                 unsigned long long* __restrict__ peak_bits) {
  const int b = blockIdx.x / blocks_per_row;
  const PcmUtt u = utt[b];
  if (u.fmt != SVC_PCM_F32 && u.fmt != SVC_PCM_F64) return;
  const int64_t lo = (int64_t)(blockIdx.x - b * blocks_per_row) * kPeakChunk;
  if (lo >= u.frames) return;
  const int64_t hi = lo + kPeakChunk < u.frames ? lo + kPeakChunk : u.frames;
  const uint8_t* p = raw + u.off;
  unsigned long long m = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads)
    m = umax64(m, (unsigned long long)__double_as_longlong(decode(p, u.fmt, i * u.ch)) & 0x7fffffffffffffffull);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = umax64(m, (unsigned long long)__shfl_xor((long long)m, off));
  __shared__ unsigned long long wave_max[kThreads / 64];
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) m = umax64(m, wave_max[w]);
    if (m) atomicMax(&peak_bits[b * kPeakStride], m);
  }
}

// MONO = false: the source row's sample of frame i, (float)x64 / mag (mag 1: the float itself);
// MONO = true: the mono row's filter input, (float)mean
template <bool MONO>
__device__ __forceinline__ float input_sample(const uint8_t* __restrict__ p, const PcmUtt& u, int64_t i, float mag) {
  if (MONO) return (float)frame_mean(p, u.fmt, u.ch, i);
  const float x = (float)decode(p, u.fmt, i * u.ch);
  return mag == 1.0f ? x : (float)((double)x / (double)mag);
}

// y[b][n], n < S: row b's sample n where n < its own length, zero after. See the head of the file. yf (MONO only, or
// null): the float mono rows, same shape; y may then be null (a plan of -1 then means an unfiltered float row).
template <bool MONO>
__global__ __launch_bounds__(kThreads) void load_pcm_kernel(const uint8_t* __restrict__ raw,
                                                            const PcmUtt* __restrict__ utt,
                                                            const PcmPlan* __restrict__ plans,
                                                            const unsigned long long* __restrict__ peak_bits,
                                                            int blocks_per_row, int64_t S, float* __restrict__ y,
                                                            float* __restrict__ yf, int32_t* __restrict__ info) {
  __shared__ float xs[kSpan];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / blocks_per_row;
  const int chunk = blockIdx.x - b * blocks_per_row;
  const PcmUtt u = utt[b];
  float* row = y ? y + (int64_t)b * S : nullptr;
  float* rowf = MONO && yf ? yf + (int64_t)b * S : nullptr;
  const int64_t n_lo = (int64_t)chunk * kChunk;
  const int64_t n_hi = n_lo + kChunk < S ? n_lo + kChunk : S;
  const int64_t n_out = MONO ? u.n_mono : u.n_src;
  const int plan_idx = MONO ? u.plan_mono : u.plan_src;
  const uint8_t* p = raw + u.off;
  // the normalisation class and the non-finite flag follow from the peak alone: (float) is monotonic, so some sample
  // is non-finite as a float exactly when the largest magnitude is (a NaN peak included)
  const double mx = __longlong_as_double((long long)peak_bits[b * kPeakStride]);
  const int cls = mx > 32768.0 ? 2 : (mx > 1.01 ? 1 : 0);
  const float mag = cls == 2 ? 2147483648.0f : (cls == 1 ? 32769.0f : 1.0f);  // (float)(2^31 + 1) = 2^31
  if (info && chunk == 0 && tid == 0) {
    const float mf = (float)mx;
    info[b] = cls | ((mf - mf == 0.0f) ? 0 : 4);
  }
  if (plan_idx < 0) {
    float* dst = MONO ? rowf : row;
    for (int64_t n = n_lo + tid; n < n_hi; n += kThreads) dst[n] = n < n_out ? input_sample<MONO>(p, u, n, mag) : 0.0f;
    return;
  }
  const bool copy_f = MONO && rowf && u.float_copy;
  const PcmPlan pl = plans[plan_idx];
  const int64_t n_in = u.frames;
  for (int64_t t0 = n_lo; t0 < n_hi; t0 += pl.tile) {
    const int64_t t1 = t0 + pl.tile < n_hi ? t0 + pl.tile : n_hi;
    int64_t lo = 0, span = 0;
    if (t0 < n_out) {  // (block-uniform) decode the inputs of outputs [t0, min(t1, n_out)) once
      const int64_t c1 = t1 < n_out ? t1 : n_out;
      lo = (t0 + pl.pre_remove) * pl.down / pl.up - (pl.per_phase - 1);
      if (lo < 0) lo = 0;
      int64_t hi = (c1 - 1 + pl.pre_remove) * pl.down / pl.up;
      if (hi > n_in - 1) hi = n_in - 1;
      span = hi - lo + 1;
      if (span > kSpan) return;  // never: the host sized `tile` for kSpan (the row keeps the caller's fill)
      __syncthreads();           // the previous tile's reads
      for (int64_t i = tid; i < span; i += kThreads) xs[i] = input_sample<MONO>(p, u, lo + i, mag);
      __syncthreads();
    }
    for (int64_t n = t0 + tid; n < t1; n += kThreads) {
      float v = 0.0f, vf = 0.0f;
      if (n < n_out) {
        const int64_t j = (n + pl.pre_remove) * pl.down;  // resample_kernel's indices
        const int k0 = (int)(j % pl.up);
        const int64_t i0 = j / pl.up;
        int64_t r_lo = i0 - (n_in - 1);
        if (r_lo < 0) r_lo = 0;
        int64_t r_hi = (pl.taps - 1 - k0) / pl.up;
        if (r_hi > i0) r_hi = i0;
        const double* h = pl.hpm + (int64_t)k0 * pl.per_phase;
        const float* x0 = xs + (i0 - lo);
        double acc = 0.0;
        for (int64_t r = r_lo; r <= r_hi; ++r) acc = fma(h[r], (double)x0[-r], acc);
        v = (float)acc;
        if (MONO) {
          // the float row: v, or sample n itself where the file is at sr_mono (in the tile: up = down = 1)
          vf = !copy_f ? v : (n >= lo && n - lo < span) ? xs[n - lo] : input_sample<MONO>(p, u, n, mag);
          // resample_kernel's quantize16
          double q = rint((double)v * 32768.0);
          q = q < -32768.0 ? -32768.0 : (q > 32767.0 ? 32767.0 : q);
          v = (float)(q / 32768.0);
        }
      }
      if (row) row[n] = v;
      if (MONO && rowf) rowf[n] = vf;
    }
  }
}

struct RatePlan {
  int up, down, taps, per_phase, tile;
};
// the integers of resample.hip's design_plan for a rate pair, and the tile that keeps a tile's input span in kSpan:
// outputs [t0, t0 + tile) read inputs from i0(t0) - (per_phase - 1) to i0(t0 + tile - 1), at most
// (tile - 1) * down / up + per_phase + 1 samples
RatePlan rate_plan(int sr_in, int sr_out) {
  RatePlan r;
  const int g = std::gcd(sr_in, sr_out);
  r.up = sr_out / g;
  r.down = sr_in / g;
  const int64_t R = std::max(r.up, r.down), half = 10 * R;
  const int64_t taps = (r.down - half % r.down) + 2 * half + 1;
  r.taps = taps > 0x7fffffff ? -1 : (int)taps;
  r.per_phase = (int)((taps - 1) / r.up + 1);
  const int64_t room = (int64_t)kSpan - r.per_phase - 1;
  const int64_t tile = room < 0 ? 0 : room * r.up / r.down + 1;
  r.tile = (int)std::min<int64_t>(tile, kChunk);
  return r;
}

}  // namespace

// The host half of svc_load_pcm and svc_load_pcm_ex (`ex`: which of the two words the messages; stage_features.hip owns the context and its ring): argument checks before any HIP call, one
// staged table [PcmUtt x B | PcmPlan x n_plans | zeroed peak words], then the launches. `ring` and `device` point into
// the context and are read only after the checks.
int load_pcm(StageRing* ring, const int* device, const void* raw, int B, const int64_t* byte_off, const int64_t* n_frames,
             const int32_t* format, const int32_t* channels, const int32_t* sr_in, int sr_src, int64_t S_src,
             float* y_src, int sr_mono, int64_t S_mono, float* y_mono, float* y_mono_float, bool ex, int32_t* info,
             hipStream_t s) {
  SVC_REQUIRE(raw, "load_pcm: null raw");
  SVC_REQUIRE(byte_off && n_frames && format && channels && sr_in, "load_pcm: null %s table",
              !byte_off ? "byte_off" : !n_frames ? "n_frames" : !format ? "format" : !channels ? "channels" : "sr_in");
  SVC_REQUIRE(y_src || y_mono || y_mono_float, "load_pcm: null y_src and y_mono%s (nothing to compute)",
              ex ? " and y_mono_float" : "");
  const bool want_mono = y_mono || y_mono_float;
  SVC_REQUIRE(B >= 1, "load_pcm: B=%d", B);
  SVC_REQUIRE(!y_src || (sr_src >= 1 && S_src >= 1), "load_pcm: sr_src=%d S_src=%lld", sr_src, (long long)S_src);
  SVC_REQUIRE(!want_mono || (sr_mono >= 1 && S_mono >= 1), "load_pcm: sr_mono=%d S_mono=%lld", sr_mono, (long long)S_mono);
  std::vector<PcmUtt> utt(B);
  std::vector<std::pair<int, int>> rates;  // the call's distinct (sr_in, sr_out)
  std::vector<RatePlan> rplans;
  auto plan_index = [&](int si, int so) {
    for (size_t i = 0; i < rates.size(); ++i)
      if (rates[i] == std::make_pair(si, so)) return (int)i;
    rates.push_back({si, so});
    rplans.push_back(rate_plan(si, so));
    return (int)rates.size() - 1;
  };
  bool any_float = false;
  int64_t max_frames = 0;
  for (int b = 0; b < B; ++b) {
    SVC_REQUIRE(format[b] >= SVC_PCM_U8 && format[b] <= SVC_PCM_F64, "load_pcm: utterance %d: unknown format %d", b,
                format[b]);
    SVC_REQUIRE(channels[b] >= 1 && channels[b] <= 8, "load_pcm: utterance %d: %d channels (1..8)", b, channels[b]);
    SVC_REQUIRE(sr_in[b] >= 1, "load_pcm: utterance %d: rate %d", b, sr_in[b]);
    SVC_REQUIRE(n_frames[b] >= 0 && byte_off[b] >= 0, "load_pcm: utterance %d: negative length or offset (%lld frames at %lld)",
                b, (long long)n_frames[b], (long long)byte_off[b]);
    PcmUtt& u = utt[b];
    u.off = byte_off[b];
    u.frames = n_frames[b];
    u.fmt = format[b];
    u.ch = channels[b];
    u.n_src = u.n_mono = 0;
    u.plan_src = u.plan_mono = -1;
    u.float_copy = u.pad_ = 0;
    any_float |= u.fmt == SVC_PCM_F32 || u.fmt == SVC_PCM_F64;
    max_frames = std::max(max_frames, u.frames);
    if (y_src) {
      u.n_src = svc_resample_len(u.frames, sr_in[b], sr_src);
      SVC_REQUIRE(u.n_src <= S_src, "load_pcm: utterance %d: %lld source samples, S_src %lld", b, (long long)u.n_src,
                  (long long)S_src);
      if (sr_in[b] != sr_src) u.plan_src = plan_index(sr_in[b], sr_src);
    }
    if (want_mono) {
      u.n_mono = svc_resample_len(u.frames, sr_in[b], sr_mono);
      SVC_REQUIRE(u.n_mono <= S_mono, "load_pcm: utterance %d: %lld mono samples, S_mono %lld", b, (long long)u.n_mono,
                  (long long)S_mono);
      u.float_copy = y_mono_float && sr_in[b] == sr_mono;
      // the quantised row always goes through the filter; a float row alone needs no plan where it is a copy
      if (y_mono || !u.float_copy) u.plan_mono = plan_index(sr_in[b], sr_mono);
    }
  }
  for (size_t i = 0; i < rplans.size(); ++i)
    SVC_REQUIRE(rplans[i].taps > 0 && rplans[i].tile >= 1, "load_pcm: rate ratio %d -> %d is too large for the filter tile",
                rates[i].first, rates[i].second);
  const int64_t bpr_src = y_src ? cdiv64(S_src, kChunk) : 0, bpr_mono = want_mono ? cdiv64(S_mono, kChunk) : 0;
  const int64_t bpr_peak = cdiv64(max_frames, kPeakChunk);
  SVC_REQUIRE(bpr_src * B < (1ll << 31) && bpr_mono * B < (1ll << 31) && bpr_peak * B < (1ll << 31),
              "load_pcm: batch of %d rows too large", B);

  SVC_HIP_CHECK(hipSetDevice(*device));
  const size_t n_plans = rates.size();
  const size_t off_plans = (size_t)B * sizeof(PcmUtt), off_peak = off_plans + n_plans * sizeof(PcmPlan);
  std::vector<char> buf(off_peak + (size_t)B * kPeakStride * 8, 0);
  memcpy(buf.data(), utt.data(), off_plans);
  PcmPlan* hp = reinterpret_cast<PcmPlan*>(buf.data() + off_plans);
  for (size_t i = 0; i < n_plans; ++i) {
    const double* hpm = nullptr;
    int up = 0, down = 0, pre_remove = 0, taps = 0, per_phase = 0;
    SVC_REQUIRE(get_plan_pm(rates[i].first, rates[i].second, &hpm, &up, &down, &pre_remove, &taps, &per_phase) == 0,
                "load_pcm: filter upload failed");
    SVC_REQUIRE(up == rplans[i].up && down == rplans[i].down && taps == rplans[i].taps &&
                    per_phase == rplans[i].per_phase,
                "load_pcm: plan %d -> %d disagrees with the resampler's", rates[i].first, rates[i].second);
    hp[i] = PcmPlan{hpm, up, down, pre_remove, taps, per_phase, rplans[i].tile};
  }
  RingRetire retire_(*ring, s);
  void* dev = nullptr;
  if (int st = ring->put(buf.data(), buf.size(), s, &dev)) return st;
  const PcmUtt* d_utt = reinterpret_cast<const PcmUtt*>(dev);
  const PcmPlan* d_plans = reinterpret_cast<const PcmPlan*>(reinterpret_cast<char*>(dev) + off_plans);
  unsigned long long* d_peak = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(dev) + off_peak);
  const uint8_t* r8 = reinterpret_cast<const uint8_t*>(raw);
  int32_t* info_left = info;  // written by the first row kernel that runs
  if (any_float && bpr_peak > 0 && (y_src || info)) {
    const int tok = prof_begin("load_pcm_peak", 0.0, 0.0, s);
    hipLaunchKernelGGL(load_pcm_peak_kernel, dim3((unsigned)(bpr_peak * B)), dim3(kThreads), 0, s, r8, d_utt,
                       (int)bpr_peak, d_peak);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
  }
  if (y_src && bpr_src > 0) {
    const int tok = prof_begin("load_pcm_src", 0.0, 0.0, s);
    hipLaunchKernelGGL(load_pcm_kernel<false>, dim3((unsigned)(bpr_src * B)), dim3(kThreads), 0, s, r8, d_utt, d_plans,
                       d_peak, (int)bpr_src, S_src, y_src, (float*)nullptr, info_left);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
    info_left = nullptr;
  }
  if (want_mono && bpr_mono > 0) {
    const int tok = prof_begin("load_pcm_mono", 0.0, 0.0, s);
    hipLaunchKernelGGL(load_pcm_kernel<true>, dim3((unsigned)(bpr_mono * B)), dim3(kThreads), 0, s, r8, d_utt, d_plans,
                       d_peak, (int)bpr_mono, S_mono, y_mono, y_mono_float, info_left);
    prof_end(tok, s);
    SVC_LAUNCH_CHECK();
  }
  return SVC_OK;
}

}  // namespace svc
