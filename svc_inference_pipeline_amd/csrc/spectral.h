// Spectral front-end launch arguments (features.hip), shared with the stage files that launch it.
#pragma once
#include "common.h"

namespace svc {

struct DftArgs {
  const float* wav; int64_t wav_stride; int64_t n_valid;  // samples per utterance actually present
  int64_t n_logical;  // length of the (zero-extended) signal the reflection is taken on
  int n_fft, hop, pad, n_frames, nbins;
  const float* window;  // [n_fft]
  const double2* twiddle;  // [n_fft] W^m = (cos, -sin)(2 pi m / n_fft)
  int mode;             // 0: sqrt(|X|^2 + 1e-9) -> ln(max(mel, 1e-5)) ; 1: |X|^2 -> log10(max(mel, 1e-10))
  const float* fb;      // the filterbank's nonzero band of each filter, packed: fb_len floats
  const int* band;      // [n_mels][3]: band [lo, hi) of each filter and its offset in fb
  int fb_len;
  int n_mels;
  float* out;           // [B*n_frames][n_mels] log-mel
  float* energy;        // optional [B*n_frames]: sqrt(sum_m exp(mel)^2) (utils/mel.py:199)
  // ragged batches (optional): utterance b has nb[b] samples (its n_valid and n_logical) and Tb[b] frames
  const int64_t* nb;
  const int* Tb;
  // per-row table (optional, device int64 [B][2]): row b reads rows[2b + 1] valid samples starting at wav + rows[2b]
  // (in place of wav + b * wav_stride and n_valid; n_logical stays the reflection length). The Whisper windows of a
  // ragged batch are framed in place that way, without a gather copy
  const int64_t* rows;
};

// windowed frames -> f64 FFT -> |X| or |X|^2 -> filterbank -> ln / log10 (-> energy), one launch
int dft_mel(const DftArgs& a, int B, hipStream_t s);
bool dft_mel_supported(int n_fft);  // 400, 512, 1024, 2048

// a transform's bin in f32, as torch forms it: mode 0 sqrt(|X|^2 + 1e-9), mode 1 |X|^2
__device__ __forceinline__ float spec_value(double re, double im, int mode) {
  const float r = (float)re, i = (float)im;
  if (mode == 0) return sqrtf(r * r + i * i + 1e-9f);
  const float m = sqrtf(r * r + i * i);
  return m * m;
}

// The key-shifted log-mel (mel_keyshift.hip): DftArgs' mode-0 mel with utterance b's window and transform length
// n_new = rint(n_fft * factor[b]) clamped to [n_fft / 2, 2 n_fft], the hop held
struct KeyshiftArgs {
  const float* wav; int64_t wav_stride; int64_t n_samples;  // [B][wav_stride], n_samples each where nb is NULL
  int n_fft, hop, n_frames;
  const double* factor;  // device [B]
  const float* fb;       // packed filterbank bands, band, fb_len, n_mels: as in DftArgs
  const int* band;
  int fb_len;
  int n_mels;
  float* out;            // [B*n_frames][n_mels] log-mel
  int32_t* info;         // optional device [B]: bit 0 factor not finite or <= 0 (taken as 1), bit 1 n_new clamped
  const int64_t* nb;     // ragged batches (optional, device): utterance b's samples and frames
  const int* Tb;
};
// n_fft 512 or 1024, hop <= n_fft / 2; every utterance longer than (2 n_fft - hop + 1) / 2 samples (the caller's check)
int mel_keyshift(const KeyshiftArgs& a, int B, hipStream_t s);

}  // namespace svc
