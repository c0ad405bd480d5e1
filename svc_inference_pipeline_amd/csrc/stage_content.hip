// The content encoders (Whisper, HuBERT / ContentVec), their frame mappings and the conditioner.
#include <math.h>
#include <stdlib.h>

#include <cmath>

#include "engine.h"

extern "C" {

// ---------------------------------------------------------------------------- whisper
static const int64_t kWhisperSamples = 480000;  // utils/whisper_extractor/audio.py:18 (30 s @ 16 kHz)
static const int64_t kWhisperWindow = 478720;   // samples per window of a long clip: 29.92 s = 1496 encoder rows
static const int kWindowFrames = 2805;          // = 1496 * 15 / 8 mel frames, so every window starts on a mel frame
static const int kMaxMapped = 2812;             // utils/whisper.py:56 (1500 * 15 // 8): the single 30 s window's frames

// The encoder over B 30 s windows. rows (device int64 [B][2], or NULL): window b holds rows[2b + 1] samples starting at
// wav16 + rows[2b] (DftArgs::rows), zeros after them; NULL is the uniform batch, window b = wav16[b][0 .. min(n, 30 s)).
// feats f32 [B][n_ctx][n_state], or NULL: taken from the workspace; *feats_used receives the buffer either way.
static int whisper_encode_impl(svc_ctx* c, const float* wav16, int B, int64_t n, const int64_t* rows, float* feats,
                               float** feats_used, hipStream_t s) {
  SVC_REQUIRE(c->has_whisper, "whisper weights not loaded");
  const int64_t NS = kWhisperSamples;
  const int F = 3000, D = c->wD, L = c->wctx;
  SVC_REQUIRE(B > 0 && (rows || n > 0), "whisper: B=%d n=%lld", B, (long long)n);
  SVC_REQUIRE(L * 2 == F, "whisper: n_ctx %d != 1500", L);
  SVC_REQUIRE((int64_t)B * F < (1LL << 31), "whisper: %d windows of %d rows overflow the row count", B, F);
  const int nb = 201;
  const size_t rows1 = (size_t)B * F, rows2 = (size_t)B * L;
  const int X3 = c->content_split ? 3 : 1;  // split-fp16 block operands are [hi | lo | hi] rows
  const int XS = c->content_mode != 0 ? 3 : 1;  // the conv stem is split-fp16 in both split modes
  const int LDM = XS == 3 ? c->wstem_ld : c->wmels;  // the stem operand's row stride
  float *fws = nullptr, *ls, *mx, *x;
  f16 *lm16, *h1, *n16, *qkv, *o16, *h16;
  int st = c->ws.plan([&](Arena& ws) {
    if (!feats) fws = ws.get<float>(rows2 * D);
    ls = ws.get<float>(rows1 * c->wmels);
    lm16 = ws.get<f16>(rows1 * LDM);
    mx = ws.get<float>(B);
    h1 = ws.get<f16>(rows1 * D * XS);
    x = ws.get<float>(rows2 * D);
    n16 = ws.get<f16>(rows2 * D * X3);
    qkv = ws.get<f16>(rows2 * 3 * D);
    o16 = ws.get<f16>(rows2 * D);
    h16 = ws.get<f16>(rows2 * 4 * D * X3);
  });
  if (st) return st;
  if (!feats) feats = fws;
  if (feats_used) *feats_used = feats;
  DftArgs a{};
  a.wav = wav16;
  a.wav_stride = n;
  a.n_valid = std::min<int64_t>(n, NS);
  a.n_logical = NS;
  a.rows = rows;
  a.n_fft = 400;
  a.hop = 160;
  a.pad = 200;
  a.n_frames = F;
  a.nbins = nb;
  a.window = c->win16;
  a.twiddle = reinterpret_cast<const double2*>(c->tw16);
  a.mode = 1;
  a.fb = c->fb16;
  a.band = c->band16;
  a.fb_len = c->fb16_len;
  a.n_mels = c->wmels;
  a.out = ls;
  if ((st = dft_mel(a, B, s))) return st;
  if ((st = whisper_normalize(ls, mx, lm16, B, (int64_t)F * c->wmels, s, XS == 3 ? c->wmels : 0, c->bf16, LDM)))
    return st;
  // conv stem
  EpiArgs e = epi();
  e.act = ACT_GELU;
  e.out16 = h1;
  e.ld16 = D * XS;
  e.split16 = XS == 3 ? D : 0;
  if ((st = run_gemm(c->wconv1, lm16, LDM, LDM, B, F, F, e, s, "whisper.conv1"))) return st;
  e = epi();
  e.act = ACT_GELU;
  e.add_t = c->wpos;
  e.ld_add_t = D;
  e.out32 = x;
  e.ld32 = D;
  if ((st = run_gemm(c->wconv2, h1, D * XS, D * XS, B, F, L, e, s, "whisper.conv2"))) return st;
  const float qk_scale = powf((float)(D / c->wH), -0.25f);
  // whisper_streams = n > 1 runs the 24 blocks as utterance-aligned sub-batches on n streams (as the sampler
  // does): rows are time-major per utterance, so a sub-batch is a row range of every buffer, and one sub-batch's
  // HBM-bound GEMM epilogues / layer norms run beside the other's MFMA phases. Default 1: with the F0 stage on its
  // side stream the single full-batch stream measured 0.3-0.4 % faster end to end (three A/B pairs, r01i kernels).
  SubBatches sb;
  if ((st = sb.fork(c, tuning().whisper_streams, B, s))) return st;
  for (int i = 0; i < c->wL; ++i) {
    WBlock& b = c->wblocks[i];
    for (int h = 0; h < sb.n; ++h) {
      const int b0 = sb.b0(h), Bh = sb.b0(h + 1) - b0;
      const size_t r = (size_t)b0 * L, rows_h = (size_t)Bh * L;
      hipStream_t hs = sb.stream(h);
      float* xh = x + r * D;
      f16* n16h = n16 + r * D * X3;
      f16* qkvh = qkv + r * 3 * D;
      f16* o16h = o16 + r * D;
      f16* h16h = h16 + r * 4 * D * X3;
      auto ln16 = [&](const float* g, const float* bb) {
        return X3 == 3 ? layernorm_f16x3(xh, g, bb, n16h, (int)rows_h, D, hs, c->bf16)
                       : layernorm_f16(xh, g, bb, n16h, (int)rows_h, D, D, hs, c->bf16);
      };
      if ((st = ln16(b.ln1_g, b.ln1_b))) return st;
      e = epi();
      e.out16 = qkvh;
      e.ld16 = 3 * D;
      e.scale_cols = 2 * D;
      e.col_scale = qk_scale;
      e.scale_cols2 = D;  // q also carries log2(e): the attention kernel's scores are in exp2 units
      e.col_scale2 = qk_scale * ATT_LOG2E;
      if ((st = run_gemm(b.qkv, n16h, D * X3, D * X3, Bh, L, L, e, hs, "whisper.qkv"))) return st;
      if (b.split_v) {
        e = epi();
        e.out16 = qkvh + 2 * D;
        e.ld16 = 3 * D;
        if ((st = run_gemm(b.v, n16h, D * X3, D * X3, Bh, L, L, e, hs, "whisper.v"))) return st;
      }
      if ((st = attention(qkvh, o16h, Bh, L, D, hs, c->bf16))) return st;
      e = epi();
      e.add_row = xh;
      e.ld_add_row = D;
      e.out32 = xh;
      e.ld32 = D;
      if ((st = run_gemm(b.out, o16h, D, D, Bh, L, L, e, hs, "whisper.out"))) return st;
      if ((st = ln16(b.ln2_g, b.ln2_b))) return st;
      e = epi();
      e.act = ACT_GELU;
      e.out16 = h16h;
      e.ld16 = 4 * D * X3;
      e.split16 = X3 == 3 ? 4 * D : 0;
      if ((st = run_gemm(b.fc1, n16h, D * X3, D * X3, Bh, L, L, e, hs, "whisper.fc1"))) return st;
      e = epi();
      e.add_row = xh;
      e.ld_add_row = D;
      e.out32 = xh;
      e.ld32 = D;
      if ((st = run_gemm(b.fc2, h16h, 4 * D * X3, 4 * D * X3, Bh, L, L, e, hs, "whisper.fc2"))) return st;
    }
  }
  if ((st = sb.join())) return st;
  return layernorm_f32(x, c->wlnp_g, c->wlnp_b, feats, (int)rows2, D, D, s);
}

svc_status svc_whisper_encode(svc_ctx* c, const float* wav16, int B, int64_t n, float* feats, void* stream) {
  CTX_READY(c);
  SVC_REQUIRE(feats, "whisper: null feats");
  return whisper_encode_impl(c, wav16, B, n, nullptr, feats, nullptr, (hipStream_t)stream);
}

int svc_whisper_windows(int frames) {
  if (frames < 1) return -1;
  return frames <= kMaxMapped ? 1 : (frames - 1) / kWindowFrames + 1;
}

// A ragged Whisper batch: every window that exists goes through the encoder once, in one pass, framed in place from
// the padded batch through the per-window table; one mapping launch writes each utterance's frames from its own
// windows. Table in the main length ring: int64 [W][2] (source offset, valid samples), then int32 [B][2] (first
// window, frames).
svc_status svc_whisper_content_ragged(svc_ctx* c, const float* wav16, int B, int64_t n, const int64_t* utt_samples,
                                      int T, const int32_t* frames, void* out16, int ld_out, float* feats_out,
                                      void* stream) {
  SVC_REQUIRE(c, "whisper_content_ragged: null context");
  SVC_REQUIRE(wav16 && out16, "whisper_content_ragged: null %s", wav16 ? "out" : "wav16k");
  SVC_REQUIRE(B > 0 && n >= 0 && T >= 1, "whisper_content_ragged: B=%d n_samples=%lld T=%d", B, (long long)n, T);
  TuningScope tuning_scope_(&c->tune);
  if (!c->finalized) {
    set_error("context not finalized");
    return SVC_ERR_STATE;
  }
  SVC_REQUIRE(c->has_whisper, "whisper weights not loaded");
  const int D = c->wD, L = c->wctx;
  SVC_REQUIRE(ld_out >= D, "whisper_content_ragged: ld_out=%d < D=%d", ld_out, D);
  SVC_REQUIRE((int64_t)B * T < (1LL << 31), "whisper_content_ragged: B=%d x T=%d rows overflow the row count", B, T);
  int64_t W64 = 0;
  for (int b = 0; b < B; ++b) {
    const int tb = frames ? frames[b] : T;
    const int64_t nb = utt_samples ? utt_samples[b] : n;
    SVC_REQUIRE(tb >= 1 && tb <= T, "whisper_content_ragged: utterance %d: %d of %d frames", b, tb, T);
    SVC_REQUIRE(nb >= 0 && nb <= n, "whisper_content_ragged: utterance %d: %lld of %lld samples", b, (long long)nb,
                (long long)n);
    W64 += svc_whisper_windows(tb);
  }
  SVC_REQUIRE(W64 * 3000 < (1LL << 31), "whisper_content_ragged: %lld windows overflow the row count", (long long)W64);
  const int W = (int)W64;
  std::vector<char> buf((size_t)W * 16 + (size_t)B * 8);
  int64_t* wt = reinterpret_cast<int64_t*>(buf.data());
  int* ut = reinterpret_cast<int*>(buf.data() + (size_t)W * 16);
  int w0 = 0;
  for (int b = 0; b < B; ++b) {
    const int tb = frames ? frames[b] : T;
    const int64_t nb = utt_samples ? utt_samples[b] : n;
    const int Wb = svc_whisper_windows(tb);
    for (int w = 0; w < Wb; ++w) {
      const int64_t start = Wb == 1 ? 0 : w * kWhisperWindow, cap = Wb == 1 ? kWhisperSamples : kWhisperWindow;
      wt[2 * (w0 + w)] = (int64_t)b * n + start;
      wt[2 * (w0 + w) + 1] = std::min(std::max<int64_t>(nb - start, 0), cap);
    }
    ut[2 * b] = w0;
    ut[2 * b + 1] = tb;
    w0 += Wb;
  }
  SVC_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  RingRetire retire_(c->lens_main, s);
  void* dev = nullptr;
  int st = c->lens_main.put(buf.data(), buf.size(), s, &dev);
  if (st) return st;
  float* feats = nullptr;
  if ((st = whisper_encode_impl(c, wav16, W, n, reinterpret_cast<const int64_t*>(dev), feats_out, &feats, s))) return st;
  const int* utab = reinterpret_cast<const int*>(reinterpret_cast<char*>(dev) + (size_t)W * 16);
  return content_map_windows(feats, B, L, D, T, D, (f16*)out16, ld_out, utab, s, c->bf16);
}

svc_status svc_map_content(svc_ctx* c, const float* feats, int B, int src_rows, int T, int D, void* out, void* stream) {
  SVC_REQUIRE(c && feats && out, "map_content: null");
  SVC_HIP_CHECK(hipSetDevice(c->device));
  return content_map(feats, B, src_rows, D, T, D, (f16*)out, D, (hipStream_t)stream, c->bf16);
}

svc_status svc_map_content_ex(svc_ctx* c, const float* feats, int B, int src_rows, int T, int D, int mode, void* out,
                              int ld_out, void* stream) {
  SVC_REQUIRE(c && feats && out && B > 0 && D > 0 && ld_out >= D, "map_content_ex: bad args");
  SVC_REQUIRE(mode == 0 || mode == 1, "map_content_ex: mode %d", mode);
  SVC_HIP_CHECK(hipSetDevice(c->device));
  if (mode == 0) return content_map(feats, B, src_rows, D, T, D, (f16*)out, ld_out, (hipStream_t)stream, c->bf16);
  return content_map_hubert(feats, B, src_rows, D, T, D, (f16*)out, ld_out, (hipStream_t)stream, c->bf16);
}

svc_status svc_map_content_ragged(svc_ctx* c, const float* feats, int B, int src_rows, const int32_t* utt_src_rows,
                                  int T, const int32_t* frames, int D, int mode, void* out, int ld_out, void* stream) {
  SVC_REQUIRE(c, "map_content_ragged: null context");
  SVC_REQUIRE(feats && out && B > 0 && D > 0 && ld_out >= D && src_rows >= 1 && T >= 1,
              "map_content_ragged: bad args (B=%d src_rows=%d T=%d D=%d ld_out=%d)", B, src_rows, T, D, ld_out);
  SVC_REQUIRE(mode == 0 || mode == 1, "map_content_ragged: mode %d", mode);
  if (!utt_src_rows && !frames) return svc_map_content_ex(c, feats, B, src_rows, T, D, mode, out, ld_out, stream);
  // each utterance is checked as content_map / content_map_hubert check a batch of its shape, before any HIP call
  std::vector<int> tab((size_t)2 * B);
  for (int b = 0; b < B; ++b) {
    const int sb = utt_src_rows ? utt_src_rows[b] : src_rows, tb = frames ? frames[b] : T;
    SVC_REQUIRE(sb >= 1 && sb <= src_rows && tb >= 1 && tb <= T,
                "map_content_ragged: utterance %d: %d of %d source rows, %d of %d frames", b, sb, src_rows, tb, T);
    if (mode == 0) {
      SVC_REQUIRE(tb <= 2812 && tb * 8 / 15 + 1 <= sb, "content_map: utterance %d: T=%d src_rows=%d", b, tb, sb);
      tab[B + b] = tb;
    } else {
      const int n_down = (int)((int64_t)sb * 15 / 8);
      SVC_REQUIRE(n_down >= 1 && std::abs(tb - n_down) <= 3,
                  "content_map_hubert: utterance %d: %d content frames map to %d rows but T=%d (|diff| > 3; "
                  "utils/hubert.py:114-120)", b, sb, n_down, tb);
      tab[B + b] = n_down;
    }
    tab[b] = tb;
  }
  SVC_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  RingRetire retire_(c->lens_main, s);
  void* dev = nullptr;
  int st = c->lens_main.put(tab.data(), tab.size() * sizeof(int), s, &dev);
  if (st) return st;
  return content_map_ragged(feats, B, src_rows, D, T, D, (f16*)out, ld_out, (const int*)dev, s, c->bf16);
}

// ---------------------------------------------------------------------------- hubert / contentvec (A8)
static int64_t hubert_len(int64_t n, int upto) {
  static const int k[7] = {10, 3, 3, 3, 3, 2, 2}, st[7] = {5, 2, 2, 2, 2, 2, 2};
  for (int i = 0; i < upto; ++i) n = n < k[i] ? 0 : (n - k[i]) / st[i] + 1;
  return n;
}

// utt (host int64 [B], validated by the caller, or NULL): ragged batch. Three things look across time and take the
// utterance's own length: the GroupNorm statistics (its own t1 rows and chunk partition), the positional conv (its
// 16-bit input operand is zeroed from row F_b on, the zero padding the clip has alone) and the attention (keys and
// queries stop at F_b). The valid convs make frame i < F_b depend on samples < n_b only and the GEMMs and LayerNorms
// are row-wise, so they run over the padded batch unchanged; rows >= F_b of feats are zeroed at the end.
static int hubert_encode_impl(svc_ctx* c, const float* wav16, int B, int64_t n, const int64_t* utt, float* feats,
                              hipStream_t s) {
  SVC_REQUIRE(c->has_hubert, "hubert weights not loaded");
  const int64_t F64 = hubert_len(n, 7);
  SVC_REQUIRE(B > 0 && F64 >= 1 && (int64_t)B * hubert_len(n, 1) < (1LL << 31), "hubert: B=%d n=%lld", B,
              (long long)n);
  int64_t t[8];
  for (int i = 0; i <= 7; ++i) t[i] = hubert_len(n, i);  // t[0] = n samples, t[7] = frames
  const int Cc = c->hC, D = c->hD, F = (int)F64;
  const int Fd = c->hblocks[0].fc1.N;
  const bool sp = c->content_mode != 0;  // HuBERT: split-fp16 in both split modes
  const int X3 = sp ? 3 : 1;  // split-fp16 operands are [hi | lo | hi] rows
  const int w5 = sp ? 16 : 8;
  const int64_t R5 = cdiv64(n, 5);
  const size_t rows0 = (size_t)B * t[1], rowsF = (size_t)B * F;
  const int kChunks = 64;
  int st;
  // per-utterance tables: samples (int64 [B]), then conv_layers[0] rows t1 and frames F (int32 [B] each)
  const int64_t* nb_dev = nullptr;
  const int *t1_dev = nullptr, *F_dev = nullptr;
  int nck_max = 0, F_min = F;
  RingRetire retire_(c->lens_main, s);
  if (utt) {
    std::vector<char> buf((size_t)B * 16);
    int64_t* nv = reinterpret_cast<int64_t*>(buf.data());
    int* tv = reinterpret_cast<int*>(buf.data() + (size_t)B * 8);
    for (int b = 0; b < B; ++b) {
      nv[b] = utt[b];
      tv[b] = (int)hubert_len(utt[b], 1);
      tv[B + b] = (int)hubert_len(utt[b], 7);
      F_min = std::min(F_min, tv[B + b]);
      const int chunks = std::max(1, std::min(kChunks, cdiv(tv[b], 256)));
      nck_max = std::max(nck_max, cdiv(tv[b], cdiv(tv[b], chunks)));
    }
    void* dev = nullptr;
    if ((st = c->lens_main.put(buf.data(), buf.size(), s, &dev))) return st;
    nb_dev = reinterpret_cast<const int64_t*>(dev);
    t1_dev = reinterpret_cast<const int*>(reinterpret_cast<char*>(dev) + (size_t)B * 8);
    F_dev = t1_dev + B;
  }
  f16 *f5, *g16, *pa, *pb, *ln16, *x16, *qkv, *o16, *h16;
  float *c0, *c6, *x;
  double* part;
  float2* gss;
  if ((st = c->ws.plan([&](Arena& ws) {
        f5 = ws.get<f16>((size_t)B * R5 * w5);
        c0 = ws.get<float>(rows0 * Cc);
        g16 = ws.get<f16>(rows0 * Cc * X3);
        part = ws.get<double>((size_t)B * kChunks * Cc * 2);
        gss = ws.get<float2>((size_t)B * Cc);
        pa = ws.get<f16>((size_t)B * t[2] * Cc * X3);
        pb = ws.get<f16>((size_t)B * t[3] * Cc * X3);
        c6 = ws.get<float>(rowsF * Cc);
        ln16 = ws.get<f16>(rowsF * Cc * X3);
        x = ws.get<float>(rowsF * D);
        x16 = ws.get<f16>(rowsF * D * X3);
        qkv = ws.get<f16>(rowsF * 3 * D);
        o16 = ws.get<f16>(rowsF * D);
        h16 = ws.get<f16>(rowsF * Fd * X3);
      })))
    return st;
  // ---- feature extractor (wav2vec2 ConvFeatureExtractionModel, mode "default")
  if ((st = hubert_frames5(wav16, B, n, f5, sp, s, c->bf16, nb_dev))) return st;
  EpiArgs e = epi();
  e.out32 = c0;
  e.ld32 = Cc;
  if ((st = run_gemm(c->hconv[0], f5, w5, w5, B, (int)R5, (int)t[1], e, s, "hubert.conv0"))) return st;
  if ((st = groupnorm_gelu(c0, B, (int)t[1], Cc, c->hgn_g, c->hgn_b, part, kChunks, gss, g16, sp, s, c->bf16, t1_dev,
                           nck_max)))
    return st;
  const f16* in = g16;
  for (int i = 1; i < 7; ++i) {
    e = epi();
    e.act = ACT_GELU;
    if (i == 6) {
      e.out32 = c6;
      e.ld32 = Cc;
    } else {
      e.out16 = (i & 1) ? pa : pb;
      e.ld16 = Cc * X3;
      e.split16 = sp ? Cc : 0;
    }
    if ((st = run_gemm(c->hconv[i], in, Cc * X3, Cc * X3, B, (int)t[i], (int)t[i + 1], e, s, "hubert.convs"))) return st;
    in = e.out16;
  }
  // ---- HubertModel.forward_features tail: LayerNorm(C) -> post_extract_proj
  if ((st = sp ? layernorm_f16x3(c6, c->hln_g, c->hln_b, ln16, (int)rowsF, Cc, s, c->bf16)
               : layernorm_f16(c6, c->hln_g, c->hln_b, ln16, (int)rowsF, Cc, Cc, s, c->bf16)))
    return st;
  e = epi();
  e.out32 = x;
  e.ld32 = D;
  if (!sp) {
    e.out16 = x16;
    e.ld16 = D;
  }
  if ((st = run_gemm(c->hproj, ln16, Cc * X3, Cc * X3, B, F, F, e, s, "hubert.proj"))) return st;
  // ---- TransformerEncoder: x += GELU(pos_conv(x)) per group, then LayerNorm (layer_norm_first = False)
  const int Cg = D / c->hPosG;
  if (sp && (st = f32_to_f16x3_grouped(x, x16, (int)rowsF, D, Cg, s, c->bf16))) return st;  // group g: [hi | lo | hi] x Cg
  // ragged: pos_conv (k = 128, pad 64) reads up to 64 rows past an utterance's end, which alone are its zero padding.
  // Only the padding rows of the operand are rewritten (the projection's f32 output x keeps them: row-wise from here)
  if (F_dev && (st = zero_tail_rows16(x16, B, F, D * X3, F_dev, F - F_min, s))) return st;
  for (int gi = 0; gi < c->hPosG; ++gi) {
    e = epi();
    e.act = ACT_GELU;
    e.add_row = x + gi * Cg;
    e.ld_add_row = D;
    e.out32 = x + gi * Cg;
    e.ld32 = D;
    if ((st = run_gemm(c->hpos[gi], x16 + (size_t)gi * Cg * X3, D * X3, Cg * X3, B, F, F, e, s, "hubert.pos_conv")))
      return st;
  }
  if ((st = layernorm_dual(x, c->henc_ln_g, c->henc_ln_b, x, x16, (int)rowsF, D, sp, s, c->bf16))) return st;
  const float qk_scale = powf(64.0f, -0.25f);  // q * dh^-1/2 split over q and k
  for (int i = 0; i < c->hLayers; ++i) {
    HBlock& b = c->hblocks[i];
    e = epi();
    e.out16 = qkv;
    e.ld16 = 3 * D;
    e.scale_cols = 2 * D;
    e.col_scale = qk_scale;
    e.scale_cols2 = D;
    e.col_scale2 = qk_scale * ATT_LOG2E;
    if ((st = run_gemm(b.qkv, x16, D * X3, D * X3, B, F, F, e, s, "hubert.qkv"))) return st;
    if ((st = attention(qkv, o16, B, F, D, s, c->bf16, F_dev))) return st;
    e = epi();
    e.add_row = x;
    e.ld_add_row = D;
    e.out32 = x;
    e.ld32 = D;
    if ((st = run_gemm(b.out, o16, D, D, B, F, F, e, s, "hubert.out"))) return st;
    if ((st = layernorm_dual(x, b.ln1_g, b.ln1_b, x, x16, (int)rowsF, D, sp, s, c->bf16))) return st;
    e = epi();
    e.act = ACT_GELU;
    e.out16 = h16;
    e.ld16 = Fd * X3;
    e.split16 = sp ? Fd : 0;
    if ((st = run_gemm(b.fc1, x16, D * X3, D * X3, B, F, F, e, s, "hubert.fc1"))) return st;
    e = epi();
    e.add_row = x;
    e.ld_add_row = D;
    e.out32 = x;
    e.ld32 = D;
    if ((st = run_gemm(b.fc2, h16, Fd * X3, Fd * X3, B, F, F, e, s, "hubert.fc2"))) return st;
    if ((st = layernorm_dual(x, b.ln2_g, b.ln2_b, x, x16, (int)rowsF, D, sp, s, c->bf16))) return st;
  }
  e = epi();
  e.out32 = feats;
  e.ld32 = c->hFinal;
  if ((st = run_gemm(c->hfinal, x16, D * X3, D * X3, B, F, F, e, s, "hubert.final_proj"))) return st;
  return F_dev ? zero_tail_rows(feats, B, F, c->hFinal, F_dev, s) : SVC_OK;
}

svc_status svc_hubert_encode(svc_ctx* c, const float* wav16, int B, int64_t n, float* feats, void* stream) {
  CTX_READY(c);
  return hubert_encode_impl(c, wav16, B, n, nullptr, feats, (hipStream_t)stream);
}

svc_status svc_hubert_encode_ragged(svc_ctx* c, const float* wav16, int B, int64_t n, const int64_t* utt_samples,
                                    float* feats, void* stream) {
  // the arguments and the length table are checked before the context is touched (no HIP call)
  SVC_REQUIRE(c, "hubert_encode_ragged: null context");
  SVC_REQUIRE(wav16 && feats, "hubert_encode_ragged: null %s", wav16 ? "feats" : "wav16k");
  SVC_REQUIRE(B > 0, "hubert_encode_ragged: B=%d", B);
  for (int b = 0; utt_samples && b < B; ++b)
    SVC_REQUIRE(utt_samples[b] >= 400 && utt_samples[b] <= n,
                "hubert_encode_ragged: utterance %d: %lld samples (at least 400 for one frame, batch length %lld)", b,
                (long long)utt_samples[b], (long long)n);
  CTX_READY(c);
  return hubert_encode_impl(c, wav16, B, n, utt_samples, feats, (hipStream_t)stream);
}

int64_t svc_hubert_frames(int64_t n_samples) { return hubert_len(n_samples, 7); }

int svc_hubert_dims(svc_ctx* c, int* final_dim, int* embed_dim) {
  SVC_REQUIRE(c && c->has_hubert, "hubert weights not loaded");
  if (final_dim) *final_dim = c->hFinal;
  if (embed_dim) *embed_dim = c->hD;
  return SVC_OK;
}

// ---------------------------------------------------------------------------- feature retrieval
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

svc_status svc_index_norms(svc_ctx* c, const void* index16, int64_t N, int D, int ld, float* norms, void* stream) {
  SVC_REQUIRE(c, "index_norms: null context");
  SVC_REQUIRE(index16 && norms, "index_norms: null %s", index16 ? "norms" : "index16");
  SVC_REQUIRE(N >= 1 && N < (1LL << 31), "index_norms: N=%lld (1 <= N < 2^31)", (long long)N);
  SVC_REQUIRE(D >= 8 && D <= 2048 && D % 8 == 0, "index_norms: D=%d (a multiple of 8 in [8, 2048])", D);
  SVC_REQUIRE(ld >= D, "index_norms: ld=%d < D=%d", ld, D);
  SVC_REQUIRE(ld % 8 == 0 && aligned16(index16), "index_norms: index16 rows must start on 16-byte boundaries (ld=%d)",
              ld);
  SVC_REQUIRE(!c->bf16 && cfgv(c, "operands.bf16", 0) == 0, "index_norms: fp16 only (this context has operands.bf16)");
  SVC_HIP_CHECK(hipSetDevice(c->device));
  return index_norms((const f16*)index16, N, D, ld, norms, (hipStream_t)stream);
}

svc_status svc_content_retrieve(svc_ctx* c, const void* content16, int B, int T, const int32_t* frames,
                                const int32_t* sel, int D, int ld, const void* index16, const float* norms, int64_t N,
                                int ld_index, int k, double rate, double dist_floor, void* out16, int ld_out,
                                int32_t* idx_out, float* dist_out, void* stream) {
  SVC_REQUIRE(c, "content_retrieve: null context");
  SVC_REQUIRE(content16 && index16 && norms && out16, "content_retrieve: null %s",
              !content16 ? "content16" : !index16 ? "index16" : !norms ? "norms" : "out16");
  SVC_REQUIRE(B >= 1 && T >= 1 && (int64_t)B * T < (1LL << 31) - 128, "content_retrieve: B=%d T=%d", B, T);
  SVC_REQUIRE(k >= 1 && k <= 8, "content_retrieve: k=%d (1 <= k <= 8)", k);
  SVC_REQUIRE(D >= 8 && D <= 2048 && D % 8 == 0, "content_retrieve: D=%d (a multiple of 8 in [8, 2048])", D);
  SVC_REQUIRE(N >= 1 && N < (1LL << 31), "content_retrieve: N=%lld (1 <= N < 2^31)", (long long)N);
  SVC_REQUIRE(ld >= D && ld_index >= D && ld_out >= D, "content_retrieve: ld=%d ld_index=%d ld_out=%d (D=%d)", ld,
              ld_index, ld_out, D);
  SVC_REQUIRE(ld % 8 == 0 && ld_index % 8 == 0 && ld_out % 8 == 0 && aligned16(content16) && aligned16(index16) &&
                  aligned16(out16),
              "content_retrieve: rows must start on 16-byte boundaries (ld=%d ld_index=%d ld_out=%d)", ld, ld_index,
              ld_out);
  SVC_REQUIRE(rate >= 0.0 && rate <= 1.0, "content_retrieve: rate %g (must lie in [0, 1])", rate);
  SVC_REQUIRE(dist_floor > 0.0 && (float)dist_floor > 0.0f && std::isfinite(dist_floor),
              "content_retrieve: dist_floor %g (must be positive)", dist_floor);
  // one staged table (retrieve.hip): int32 frames[B], int32 sel[B]
  std::vector<int32_t> tab((size_t)2 * B);
  for (int b = 0; b < B; ++b) {
    tab[b] = frames ? frames[b] : T;
    tab[(size_t)B + b] = sel ? (sel[b] != 0 ? 1 : 0) : 1;
    SVC_REQUIRE(tab[b] >= 0 && tab[b] <= T, "content_retrieve: utterance %d: %d frames (row length %d)", b, tab[b], T);
  }
  {  // out is content itself (same rows) or shares no byte with it; it shares none with the index or the norms
    const uintptr_t rows = (uintptr_t)B * (uintptr_t)T;
    const uintptr_t q0 = reinterpret_cast<uintptr_t>(content16), o0 = reinterpret_cast<uintptr_t>(out16);
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(index16), n0 = reinterpret_cast<uintptr_t>(norms);
    const uintptr_t nq = ((rows - 1) * (uintptr_t)ld + D) * 2, no = ((rows - 1) * (uintptr_t)ld_out + D) * 2;
    const uintptr_t nx = ((uintptr_t)(N - 1) * (uintptr_t)ld_index + D) * 2, nn = (uintptr_t)N * 4;
    SVC_REQUIRE((o0 == q0 && ld_out == ld) || o0 + no <= q0 || q0 + nq <= o0,
                "content_retrieve: out16 overlaps content16 without being content16");
    SVC_REQUIRE(o0 + no <= x0 || x0 + nx <= o0, "content_retrieve: out16 overlaps index16");
    SVC_REQUIRE(o0 + no <= n0 || n0 + nn <= o0, "content_retrieve: out16 overlaps norms");
  }
  SVC_REQUIRE(!c->bf16 && cfgv(c, "operands.bf16", 0) == 0,
              "content_retrieve: fp16 only (this context has operands.bf16)");
  TuningScope tuning_scope_(&c->tune);
  SVC_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  RingRetire retire_(c->lens_retr, s);
  void* dev = nullptr;
  if (int st = c->lens_retr.put(tab.data(), tab.size() * sizeof(int32_t), s, &dev)) return st;
  return content_retrieve((const f16*)content16, B, T, D, ld, reinterpret_cast<const int*>(dev), (const f16*)index16,
                          norms, (int)N, ld_index, k, rate, dist_floor, (f16*)out16, ld_out, idx_out, dist_out, c->ws, s);
}

// ---------------------------------------------------------------------------- index compaction (k-means)
// svc_index_norms' checks of one set of f16 rows, under the entry point's name
#define INDEX_ROWS_OK(fn, what, ptr, ldv, D)                                                                      \
  do {                                                                                                            \
    SVC_REQUIRE((ldv) >= (D), fn ": " what " ld=%d < D=%d", (ldv), (D));                                          \
    SVC_REQUIRE((ldv) % 8 == 0 && aligned16(ptr), fn ": " what " rows must start on 16-byte boundaries (ld=%d)", \
                (ldv));                                                                                           \
  } while (0)
#define INDEX_SHAPE_OK(fn, N, D, K)                                                                              \
  do {                                                                                                           \
    SVC_REQUIRE((N) >= 1 && (N) <= (1LL << 22), fn ": N=%lld (1 <= N <= 2^22)", (long long)(N));                 \
    SVC_REQUIRE((D) >= 8 && (D) <= 2048 && (D) % 8 == 0, fn ": D=%d (a multiple of 8 in [8, 2048])", (D));       \
    SVC_REQUIRE((K) >= 1 && (K) <= (N) && (K) <= (1 << 20), fn ": K=%d (1 <= K <= min(N, 2^20), N=%lld)", (K),   \
                (long long)(N));                                                                                 \
  } while (0)

static bool disjoint(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 + na <= b0 || b0 + nb <= a0;
}
static size_t rows_bytes(int64_t n, int ld, int D) { return ((size_t)(n - 1) * (size_t)ld + (size_t)D) * 2; }

svc_status svc_index_assign(svc_ctx* c, const void* rows16, int64_t N, int D, int ld, const void* cent16,
                            const float* cent_norms, int K, int ld_cent, int32_t* labels, int32_t* counts,
                            double* inertia, void* stream) {
  SVC_REQUIRE(c, "index_assign: null context");
  SVC_REQUIRE(rows16 && cent16 && cent_norms && labels, "index_assign: null %s",
              !rows16 ? "rows16" : !cent16 ? "cent16" : !cent_norms ? "cent_norms" : "labels");
  INDEX_SHAPE_OK("index_assign", N, D, K);
  INDEX_ROWS_OK("index_assign", "rows16", rows16, ld, D);
  INDEX_ROWS_OK("index_assign", "cent16", cent16, ld_cent, D);
  SVC_REQUIRE(!c->bf16 && cfgv(c, "operands.bf16", 0) == 0, "index_assign: fp16 only (this context has operands.bf16)");
  TuningScope tuning_scope_(&c->tune);
  SVC_HIP_CHECK(hipSetDevice(c->device));
  return index_assign((const f16*)rows16, N, D, ld, (const f16*)cent16, cent_norms, K, ld_cent, labels, counts, inertia,
                      c->ws, (hipStream_t)stream);
}

svc_status svc_index_update(svc_ctx* c, const void* rows16, int64_t N, int D, int ld, const int32_t* labels, int K,
                            const void* prev16, int ld_prev, void* out16, int ld_out, float* norms_out, int32_t* counts,
                            void* stream) {
  SVC_REQUIRE(c, "index_update: null context");
  SVC_REQUIRE(rows16 && labels && prev16 && out16 && norms_out, "index_update: null %s",
              !rows16 ? "rows16" : !labels ? "labels" : !prev16 ? "prev16" : !out16 ? "out16" : "norms_out");
  INDEX_SHAPE_OK("index_update", N, D, K);
  INDEX_ROWS_OK("index_update", "rows16", rows16, ld, D);
  INDEX_ROWS_OK("index_update", "prev16", prev16, ld_prev, D);
  INDEX_ROWS_OK("index_update", "out16", out16, ld_out, D);
  SVC_REQUIRE((out16 == prev16 && ld_out == ld_prev) ||
                  disjoint(out16, rows_bytes(K, ld_out, D), prev16, rows_bytes(K, ld_prev, D)),
              "index_update: out16 overlaps prev16 without being prev16");
  SVC_REQUIRE(disjoint(out16, rows_bytes(K, ld_out, D), rows16, rows_bytes(N, ld, D)),
              "index_update: out16 overlaps rows16");
  SVC_REQUIRE(!c->bf16 && cfgv(c, "operands.bf16", 0) == 0, "index_update: fp16 only (this context has operands.bf16)");
  SVC_HIP_CHECK(hipSetDevice(c->device));
  return index_update((const f16*)rows16, N, D, ld, labels, K, (const f16*)prev16, ld_prev, (f16*)out16, ld_out,
                      norms_out, counts, c->ws, (hipStream_t)stream);
}

svc_status svc_index_kmeans(svc_ctx* c, const void* rows16, int64_t N, int D, int ld, int K, int iters, void* cent16,
                            int ld_cent, float* cent_norms, int32_t* labels, int32_t* counts, double* inertia,
                            void* stream) {
  SVC_REQUIRE(c, "index_kmeans: null context");
  SVC_REQUIRE(rows16 && cent16 && cent_norms, "index_kmeans: null %s",
              !rows16 ? "rows16" : !cent16 ? "cent16" : "cent_norms");
  INDEX_SHAPE_OK("index_kmeans", N, D, K);
  SVC_REQUIRE(iters >= 0 && iters <= 1000, "index_kmeans: iters=%d (0 <= iters <= 1000)", iters);
  INDEX_ROWS_OK("index_kmeans", "rows16", rows16, ld, D);
  INDEX_ROWS_OK("index_kmeans", "cent16", cent16, ld_cent, D);
  SVC_REQUIRE(disjoint(cent16, rows_bytes(K, ld_cent, D), rows16, rows_bytes(N, ld, D)),
              "index_kmeans: cent16 overlaps rows16");
  SVC_REQUIRE(!c->bf16 && cfgv(c, "operands.bf16", 0) == 0, "index_kmeans: fp16 only (this context has operands.bf16)");
  TuningScope tuning_scope_(&c->tune);
  SVC_HIP_CHECK(hipSetDevice(c->device));
  return index_kmeans((const f16*)rows16, N, D, ld, K, iters, (f16*)cent16, ld_cent, cent_norms, labels, counts, inertia,
                      c->ws, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------- conditioner
svc_status svc_condition_indices(svc_ctx* c, const double* f0, const float* energy, int n, int32_t* melody_idx,
                                 int32_t* loudness_idx, void* stream) {
  CTX_READY(c);
  SVC_REQUIRE(c->has_mapper, "mapper weights not loaded");
  SVC_REQUIRE(n >= 0 && (n == 0 || (f0 && energy && melody_idx && loudness_idx)), "condition_indices: n %d", n);
  if (n == 0) return SVC_OK;
  return bucketize(f0, energy, c->mbins, c->ebins, c->n_bins - 1, melody_idx, loudness_idx, n, (hipStream_t)stream);
}

svc_status svc_condition(svc_ctx* c, const void* content16, const double* f0, const float* energy,
                         const int32_t* singer, int B, int T, float* cond, void* stream) {
  CTX_READY(c);
  SVC_REQUIRE(c->has_mapper, "mapper weights not loaded");
  hipStream_t s = (hipStream_t)stream;
  const int rows = B * T;
  int *im, *ie;
  int st = c->ws.plan([&](Arena& ws) {
    im = ws.get<int>(rows);
    ie = ws.get<int>(rows);
  });
  if (st || (st = bucketize(f0, energy, c->mbins, c->ebins, c->n_bins - 1, im, ie, rows, s))) return st;
  EpiArgs e = epi();
  e.kind = EPI_COND;
  e.idx_m = im;
  e.idx_l = ie;
  e.singer = singer;
  e.emb_m = c->emb_m;
  e.emb_l = c->emb_l;
  e.emb_s = c->emb_s;
  e.ld_emb = c->C;
  e.out32 = cond;
  e.ld32 = c->C;
  return run_gemm(c->content_lin, (const f16*)content16, c->content_dim, c->content_dim, B, T, T, e, s, "cond.content");
}

}  // extern "C"
