// The waveform-side stages: mel + energy, the F0 front ends, 16-bit PCM output and wav payload decoding.
#include "engine.h"

extern "C" {

// ---------------------------------------------------------------------------- mel + energy
// mel frames of an n-sample clip (utils/mel.py:148-167: reflect pad (n_fft - hop) / 2 each side, center=False)
static int64_t mel_frames_of(const svc_ctx* c, int64_t n) {
  const int pad = (c->n_fft - c->hop) / 2;
  return (n + 2 * pad - c->n_fft) / c->hop + 1;
}

// ragged batches: validate the per-utterance sample counts (host) and stage them with their mel frame counts
// (int64 n[B] then int T[B]) to the device through `ring`
static int stage_samples(svc_ctx* c, StageRing& ring, const int64_t* n_samples, int B, int64_t n, hipStream_t s,
                         const int64_t** nb_dev, const int** Tb_dev, std::vector<int>* Tb_host) {
  *nb_dev = nullptr;
  *Tb_dev = nullptr;
  if (!n_samples) return SVC_OK;
  const int pad = (c->n_fft - c->hop) / 2;
  std::vector<char> buf((size_t)B * (8 + 4));
  int64_t* nv = reinterpret_cast<int64_t*>(buf.data());
  int* tv = reinterpret_cast<int*>(buf.data() + (size_t)B * 8);
  Tb_host->resize(B);
  for (int b = 0; b < B; ++b) {
    SVC_REQUIRE(n_samples[b] > pad && n_samples[b] <= n, "utterance %d: %lld samples (batch length %lld)", b,
                (long long)n_samples[b], (long long)n);
    nv[b] = n_samples[b];
    tv[b] = (int)mel_frames_of(c, n_samples[b]);
    (*Tb_host)[b] = tv[b];
  }
  void* dev = nullptr;
  int st = ring.put(buf.data(), buf.size(), s, &dev);
  if (st) return st;
  *nb_dev = reinterpret_cast<const int64_t*>(dev);
  *Tb_dev = reinterpret_cast<const int*>(reinterpret_cast<char*>(dev) + (size_t)B * 8);
  return SVC_OK;
}

svc_status svc_mel_energy(svc_ctx* c, const float* wav, int B, int64_t n, const int64_t* n_samples, float* mel,
                          float* energy, void* stream) {
  CTX_READY(c);
  hipStream_t s = (hipStream_t)stream;
  const int pad = (c->n_fft - c->hop) / 2;
  const int64_t T64 = mel_frames_of(c, n);
  SVC_REQUIRE(B > 0 && n > pad && T64 > 0 && T64 < (1 << 30), "mel_energy: n=%lld", (long long)n);
  const int T = (int)T64, nb = c->n_fft / 2 + 1;
  const int64_t* nb_dev;
  const int* Tb_dev;
  std::vector<int> Tb_host;
  RingRetire retire_(c->lens_feat, s);
  int st0 = stage_samples(c, c->lens_feat, n_samples, B, n, s, &nb_dev, &Tb_dev, &Tb_host);
  if (st0) return st0;
  int st;
  DftArgs a{};
  a.wav = wav;
  a.wav_stride = n;
  a.n_valid = n;
  a.n_logical = n;
  a.n_fft = c->n_fft;
  a.hop = c->hop;
  a.pad = pad;
  a.n_frames = T;
  a.nbins = nb;
  a.window = c->win_mel;
  a.twiddle = reinterpret_cast<const double2*>(c->tw24);
  a.mode = 0;
  a.fb = c->fb24;
  a.band = c->band24;
  a.fb_len = c->fb24_len;
  a.n_mels = c->n_mels;
  a.out = mel;
  a.energy = energy;
  a.nb = nb_dev;
  a.Tb = Tb_dev;
  if ((st = dft_mel(a, B, s))) return st;
  if (Tb_dev && ((st = zero_tail_rows(mel, B, T, c->n_mels, Tb_dev, s)) || (st = zero_tail_rows(energy, B, T, 1, Tb_dev, s))))
    return st;
  return SVC_OK;
}

// ---------------------------------------------------------------------------- key-shifted mel
svc_status svc_mel_keyshift(svc_ctx* c, const float* wav, int B, int64_t n, const int64_t* n_samples,
                            const double* factor, float* mel, int32_t* info, void* stream) {
  // every argument check comes before the first HIP call
  TuningScope tuning_scope_(c ? &c->tune : nullptr);
  SVC_REQUIRE(c, "null context");
  SVC_REQUIRE(wav && factor && mel, "mel_keyshift: null %s", !wav ? "wav" : !factor ? "factor" : "mel");
  SVC_REQUIRE(B >= 1, "mel_keyshift: B=%d", B);
  if (!c->finalized) {
    set_error("context not finalized");
    return SVC_ERR_STATE;
  }
  SVC_REQUIRE(c->n_fft == 512 || c->n_fft == 1024, "mel_keyshift: n_fft %d (512 or 1024)", c->n_fft);
  SVC_REQUIRE(c->hop > 0 && c->hop <= c->n_fft / 2, "mel_keyshift: hop %d with n_fft %d", c->hop, c->n_fft);
  SVC_REQUIRE(c->fb24 && c->band24 && c->fb24_len > 0, "mel_keyshift: the context has no mel filterbank");
  // the widest window (2 n_fft) reflects (2 n_fft - hop) / 2 samples at the start and up to one more at the end: each
  // utterance must hold them
  const int64_t min_len = (2 * (int64_t)c->n_fft - c->hop + 1) / 2;
  const int64_t T64 = mel_frames_of(c, n);
  SVC_REQUIRE(n > min_len && T64 > 0 && T64 < (1 << 30), "mel_keyshift: n=%lld (more than %lld samples)", (long long)n,
              (long long)min_len);
  if (n_samples)
    for (int b = 0; b < B; ++b)
      SVC_REQUIRE(n_samples[b] > min_len && n_samples[b] <= n,
                  "mel_keyshift: utterance %d: %lld samples (more than %lld, batch length %lld)", b,
                  (long long)n_samples[b], (long long)min_len, (long long)n);
  SVC_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const int T = (int)T64;
  const int64_t* nb_dev;
  const int* Tb_dev;
  std::vector<int> Tb_host;
  RingRetire retire_(c->lens_feat, s);
  int st = stage_samples(c, c->lens_feat, n_samples, B, n, s, &nb_dev, &Tb_dev, &Tb_host);
  if (st) return st;
  KeyshiftArgs a{};
  a.wav = wav;
  a.wav_stride = n;
  a.n_samples = n;
  a.n_fft = c->n_fft;
  a.hop = c->hop;
  a.n_frames = T;
  a.factor = factor;
  a.fb = c->fb24;
  a.band = c->band24;
  a.fb_len = c->fb24_len;
  a.n_mels = c->n_mels;
  a.out = mel;
  a.info = info;
  a.nb = nb_dev;
  a.Tb = Tb_dev;
  if ((st = mel_keyshift(a, B, s))) return st;
  if (Tb_dev && (st = zero_tail_rows(mel, B, T, c->n_mels, Tb_dev, s))) return st;
  return SVC_OK;
}

// ---------------------------------------------------------------------------- F0
svc_status svc_f0_ac(svc_ctx* c, const float* wav, int B, int64_t n, const int64_t* n_samples, int T, double* f0,
                     void* stream) {
  CTX_READY(c);
  const double ts = (double)c->hop / c->fs;
  int st;
  std::vector<int> Tb;
  if (n_samples) {
    Tb.resize(B);
    for (int b = 0; b < B; ++b) Tb[b] = (int)mel_frames_of(c, n_samples[b]);
  }
  const double key[2] = {(double)c->fs, c->f0_min};
  double* f0_tab = c->f0_tabs.find(key, 2);
  if (!f0_tab) {
    std::vector<double> tab(f0_table_doubles(c->fs, c->f0_min));
    if ((st = f0_tables(c->fs, c->f0_min, tab.data()))) return st;
    void* p = nullptr;
    SVC_HIP_CHECK(hipMalloc(&p, tab.size() * 8));
    const hipError_t me = hipMemcpy(p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice);
    if (me != hipSuccess) (void)hipFree(p);
    SVC_HIP_CHECK(me);
    f0_tab = reinterpret_cast<double*>(p);
    if ((st = c->f0_tabs.insert(key, 2, f0_tab))) return st;
  }
  RingRetire retire_(c->lens_feat, (hipStream_t)stream);
  return f0_praat_ac(wav, B, n, c->fs, ts, c->f0_min, c->f0_max, 0.6, T, f0, c->auxws, f0_tab, (hipStream_t)stream,
                     n_samples, n_samples ? Tb.data() : nullptr, &c->lens_feat);
}

svc_status svc_f0_pyin(svc_ctx* c, const float* wav, int B, int64_t n, const int64_t* n_samples, double fs,
                       int win_length, int hop_length, double f0_min, double f0_max, int T, double* f0, void* stream) {
  SVC_REQUIRE(c, "null context");
  TuningScope tuning_scope_(&c->tune);
  SVC_HIP_CHECK(hipSetDevice(c->device));
  const int FL = 2048;  // librosa.pyin frame_length default (utils/f0.py:107 leaves it unset)
  const size_t nt = pyin_table_doubles(fs, f0_min, f0_max, FL, win_length, hop_length);
  if (!nt) return SVC_ERR_INVALID;  // (pyin_plan set the error)
  SVC_REQUIRE(B > 0 && n > 0 && T > 0, "pyin: B=%d n=%lld T=%d", B, (long long)n, T);
  int st;
  // the tables depend only on (fs, f0_min, f0_max, win, hop): built and uploaded once per parameter set
  const double key[5] = {fs, f0_min, f0_max, (double)win_length, (double)hop_length};
  double* pyin_tab = c->pyin_tabs.find(key, 5);
  if (!pyin_tab) {
    std::vector<double> tab(nt);
    if ((st = pyin_tables(fs, f0_min, f0_max, FL, win_length, hop_length, tab.data()))) return st;
    void* p = nullptr;
    SVC_HIP_CHECK(hipMalloc(&p, nt * 8));
    const hipError_t me = hipMemcpy(p, tab.data(), nt * 8, hipMemcpyHostToDevice);
    if (me != hipSuccess) (void)hipFree(p);
    SVC_HIP_CHECK(me);
    pyin_tab = reinterpret_cast<double*>(p);
    if ((st = c->pyin_tabs.insert(key, 5, pyin_tab))) return st;
  }
  // only the per-call lengths are staged (the ring retires its last slot)
  hipStream_t s = (hipStream_t)stream;
  RingRetire retire_(c->lens_feat, s);
  const int64_t* nb_dev = nullptr;
  if (n_samples) {
    void* dev = nullptr;
    if ((st = c->lens_feat.put(n_samples, (size_t)B * 8, s, &dev))) return st;
    nb_dev = reinterpret_cast<const int64_t*>(dev);
  }
  return f0_pyin(wav, B, n, nb_dev, n_samples, fs, f0_min, f0_max, FL, win_length, hop_length, T, f0, c->auxws,
                 pyin_tab, s);
}

svc_status svc_pitch_shift(svc_ctx* c, double* f0, int B, int T, double target_median, void* stream) {
  SVC_REQUIRE(c && f0 && B > 0 && T > 0, "pitch_shift: bad args");
  SVC_HIP_CHECK(hipSetDevice(c->device));
  return pitch_shift(f0, B, T, target_median, (hipStream_t)stream);
}

svc_status svc_pitch_shift_ex(svc_ctx* c, double* f0, int B, int T, const double* target_median, const double* scale,
                              void* stream) {
  SVC_REQUIRE(c, "pitch_shift_ex: null context");
  SVC_REQUIRE(f0 && target_median && B > 0 && T > 0, "pitch_shift_ex: bad args (B=%d T=%d)", B, T);
  // one staged table: f64 target[B], then f64 scale[B] where given; checked before any HIP call
  const int cols = scale ? 2 : 1;
  std::vector<double> tab((size_t)B * cols);
  for (int b = 0; b < B; ++b) {
    SVC_REQUIRE(std::isfinite(target_median[b]) && target_median[b] > 0.0,
                "pitch_shift_ex: utterance %d: target median %g (must be finite and positive)", b, target_median[b]);
    tab[b] = target_median[b];
    if (scale) {
      SVC_REQUIRE(std::isfinite(scale[b]) && scale[b] > 0.0,
                  "pitch_shift_ex: utterance %d: scale %g (must be finite and positive)", b, scale[b]);
      tab[(size_t)B + b] = scale[b];
    }
  }
  SVC_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  RingRetire retire_(c->lens_feat, s);
  void* dev = nullptr;
  if (int st = c->lens_feat.put(tab.data(), tab.size() * sizeof(double), s, &dev)) return st;
  const double* td = reinterpret_cast<const double*>(dev);
  return pitch_shift_ex(f0, B, T, td, scale ? td + B : nullptr, s);
}

svc_status svc_pitch_factor(svc_ctx* c, const double* f0, int B, int T, const double* target_median,
                            const double* scale, double* factor, void* stream) {
  SVC_REQUIRE(c, "pitch_factor: null context");
  SVC_REQUIRE(f0 && target_median && factor && B > 0 && T > 0, "pitch_factor: bad args (B=%d T=%d)", B, T);
  // svc_pitch_shift_ex's staged table: f64 target[B], then f64 scale[B] where given; checked before any HIP call
  const int cols = scale ? 2 : 1;
  std::vector<double> tab((size_t)B * cols);
  for (int b = 0; b < B; ++b) {
    SVC_REQUIRE(std::isfinite(target_median[b]) && target_median[b] > 0.0,
                "pitch_factor: utterance %d: target median %g (must be finite and positive)", b, target_median[b]);
    tab[b] = target_median[b];
    if (scale) {
      SVC_REQUIRE(std::isfinite(scale[b]) && scale[b] > 0.0,
                  "pitch_factor: utterance %d: scale %g (must be finite and positive)", b, scale[b]);
      tab[(size_t)B + b] = scale[b];
    }
  }
  SVC_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  RingRetire retire_(c->lens_feat, s);
  void* dev = nullptr;
  if (int st = c->lens_feat.put(tab.data(), tab.size() * sizeof(double), s, &dev)) return st;
  const double* td = reinterpret_cast<const double*>(dev);
  return pitch_factor(f0, B, T, td, scale ? td + B : nullptr, factor, s);
}

svc_status svc_f0_voiced_median(svc_ctx* c, const double* f0, int B, int T, const int32_t* frames, double* median,
                                int64_t* voiced, void* stream) {
  SVC_REQUIRE(c, "f0_voiced_median: null context");
  SVC_REQUIRE(f0 && median && B > 0 && T > 0, "f0_voiced_median: bad args (B=%d T=%d)", B, T);
  SVC_REQUIRE((int64_t)B * T < (1ll << 31), "f0_voiced_median: B * T = %lld cells (must be below 2^31)",
              (long long)B * T);
  if (frames)
    for (int b = 0; b < B; ++b)
      SVC_REQUIRE(frames[b] >= 0 && frames[b] <= T, "f0_voiced_median: utterance %d: %d frames (row length %d)", b,
                  frames[b], T);
  SVC_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  RingRetire retire_(c->lens_feat, s);
  const int* frames_dev = nullptr;
  if (frames) {
    void* dev = nullptr;
    if (int st = c->lens_feat.put(frames, (size_t)B * sizeof(int32_t), s, &dev)) return st;
    frames_dev = reinterpret_cast<const int*>(dev);
  }
  return f0_voiced_median(f0, B, T, frames_dev, median, reinterpret_cast<long long*>(voiced), c->auxws, s);
}

// ---------------------------------------------------------------------------- 16-bit PCM (A16)
svc_status svc_pcm16(svc_ctx* c, const float* wav, int B, int64_t S, const int64_t* utt_samples, int fs,
                     int add_silence, int turn_up, double volume_peak, void* pcm, float* peak_out, void* stream) {
  SVC_REQUIRE(c, "pcm16: null context");
  SVC_REQUIRE(wav && pcm, "pcm16: null %s", wav ? "pcm" : "wav");
  SVC_REQUIRE(B >= 1 && S >= 1, "pcm16: B=%d S=%lld", B, (long long)S);
  SVC_REQUIRE(fs >= 1, "pcm16: fs=%d", fs);
  SVC_REQUIRE(!turn_up || volume_peak > 0.0, "pcm16: volume_peak %g (must be positive with turn_up)", volume_peak);
  // one staged table (pcm16.hip): int64 n[B], then the peak scratch, whose zeros the same stream-ordered copy writes
  std::vector<char> buf(pcm16_table_bytes(B), 0);
  int64_t* nv = reinterpret_cast<int64_t*>(buf.data());
  int64_t max_nb = 0;
  for (int b = 0; b < B; ++b) {
    nv[b] = utt_samples ? utt_samples[b] : S;
    SVC_REQUIRE(nv[b] >= 0 && nv[b] <= S, "pcm16: utterance %d: %lld samples (batch length %lld)", b, (long long)nv[b],
                (long long)S);
    max_nb = std::max(max_nb, nv[b]);
  }
  SVC_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const int sil = add_silence ? fs / 20 : 0;
  RingRetire retire_(c->lens_pcm, s);
  void* dev = nullptr;
  if (int st = c->lens_pcm.put(buf.data(), buf.size(), s, &dev)) return st;
  return pcm16(wav, B, S, dev, max_nb, sil, S + 2 * (int64_t)sil, turn_up ? 1 : 0, volume_peak,
               reinterpret_cast<int16_t*>(pcm), peak_out, (turn_up || peak_out) ? 1 : 0, s);
}

// ---------------------------------------------------------------------------- loudness envelope transfer
svc_status svc_loudness_match(svc_ctx* c, const float* wav, const float* src, int B, int64_t S, int64_t S_src,
                              const int64_t* utt_samples, const int64_t* src_samples, int window, int hop, double mix,
                              double floor_rms, double max_gain, float* out, double* gain_out, void* stream) {
  SVC_REQUIRE(c, "loudness_match: null context");
  SVC_REQUIRE(wav && src && out, "loudness_match: null %s", !wav ? "wav" : !src ? "src" : "out");
  SVC_REQUIRE(B >= 1 && S >= 1 && S_src >= 1, "loudness_match: B=%d S=%lld S_src=%lld", B, (long long)S,
              (long long)S_src);
  SVC_REQUIRE(window >= 1 && hop >= 1, "loudness_match: window=%d hop=%d", window, hop);
  SVC_REQUIRE(mix >= 0.0 && mix <= 1.0, "loudness_match: mix %g (must lie in [0, 1])", mix);
  SVC_REQUIRE(floor_rms > 0.0, "loudness_match: floor_rms %g (must be positive)", floor_rms);
  {  // out is wav itself or shares no byte with it (a block reads only the samples it writes), and none with src
    const uintptr_t w0 = reinterpret_cast<uintptr_t>(wav), o0 = reinterpret_cast<uintptr_t>(out);
    const uintptr_t r0 = reinterpret_cast<uintptr_t>(src);
    const uintptr_t nb = (uintptr_t)B * (uintptr_t)S * 4, nr = (uintptr_t)B * (uintptr_t)S_src * 4;
    SVC_REQUIRE(o0 == w0 || o0 + nb <= w0 || w0 + nb <= o0, "loudness_match: out overlaps wav without being wav");
    SVC_REQUIRE(o0 + nb <= r0 || r0 + nr <= o0, "loudness_match: out overlaps src");
  }
  // one staged table (loudness.hip): int64 n_out[B], int64 n_src[B]; the frame powers lie behind it in the same slot
  std::vector<int64_t> lens((size_t)2 * B);
  int64_t max_n = 0;
  for (int b = 0; b < B; ++b) {
    lens[b] = utt_samples ? utt_samples[b] : S;
    lens[B + b] = src_samples ? src_samples[b] : S_src;
    SVC_REQUIRE(lens[b] >= 0 && lens[b] <= S, "loudness_match: utterance %d: %lld samples (batch length %lld)", b,
                (long long)lens[b], (long long)S);
    SVC_REQUIRE(lens[B + b] >= 0 && lens[B + b] <= S_src,
                "loudness_match: utterance %d: %lld source samples (batch length %lld)", b, (long long)lens[B + b],
                (long long)S_src);
    max_n = std::max(max_n, lens[b]);
  }
  const int64_t K_max = 1 + max_n / hop;
  SVC_REQUIRE(loudness_power_bytes(B, K_max) <= ((size_t)64 << 20),
              "loudness_match: %lld frames x %d utterances: hop %d too small for this batch", (long long)K_max, B, hop);
  SVC_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  RingRetire retire_(c->lens_loud, s);
  void* dev = nullptr;
  if (int st = c->lens_loud.put(lens.data(), loudness_lens_bytes(B), s, &dev, loudness_power_bytes(B, K_max))) return st;
  return loudness_match(wav, src, B, S, S_src, dev, K_max, window, hop, mix, floor_rms, max_gain, out, gain_out,
                        1 + S / hop, s);
}

// ---------------------------------------------------------------------------- long-form conversion: the join
svc_status svc_stitch(svc_ctx* c, const float* const* rows, int B, const int64_t* n, const int64_t* lead,
                      const int64_t* body, const int32_t* joined, const int64_t* out_off, int xfade, int search,
                      double eps, float* out, int64_t out_len, int32_t* shift_out, double* q_out, void* stream) {
  SVC_REQUIRE(c, "stitch: null context");
  // the context is read only once the arguments have passed (stitch.hip checks them before any HIP call)
  return stitch(&c->lens_stitch, &c->device, rows, B, n, lead, body, joined, out_off, xfade, search, eps, out, out_len,
                shift_out, q_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------- wav payloads -> the input batches (A1)
svc_status svc_load_pcm(svc_ctx* c, const void* raw, int B, const int64_t* byte_off, const int64_t* n_frames,
                        const int32_t* format, const int32_t* channels, const int32_t* sr_in, int sr_src,
                        int64_t S_src, float* y_src, int sr_mono, int64_t S_mono, float* y_mono, int32_t* info,
                        void* stream) {
  SVC_REQUIRE(c, "load_pcm: null context");
  // the context is read only once the arguments have passed (load_pcm.hip checks them before any HIP call)
  return load_pcm(&c->lens_load, &c->device, raw, B, byte_off, n_frames, format, channels, sr_in, sr_src, S_src, y_src,
                  sr_mono, S_mono, y_mono, nullptr, false, info, (hipStream_t)stream);
}

svc_status svc_load_pcm_ex(svc_ctx* c, const void* raw, int B, const int64_t* byte_off, const int64_t* n_frames,
                           const int32_t* format, const int32_t* channels, const int32_t* sr_in, int sr_src,
                           int64_t S_src, float* y_src, int sr_mono, int64_t S_mono, float* y_mono,
                           float* y_mono_float, int32_t* info, void* stream) {
  SVC_REQUIRE(c, "load_pcm: null context");
  return load_pcm(&c->lens_load, &c->device, raw, B, byte_off, n_frames, format, channels, sr_in, sr_src, S_src, y_src,
                  sr_mono, S_mono, y_mono, y_mono_float, true, info, (hipStream_t)stream);
}

}  // extern "C"
