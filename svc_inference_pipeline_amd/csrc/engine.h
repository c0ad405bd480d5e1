// The engine's own types and the helpers its files share: the context (svc_ctx), packed weights and the sub-batch
// fork / join (the workspace arena is arena.h). Included by engine.hip, finalize.hip, the stage_*.hip files and ops.hip
// only.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/svc_hip.h"
#include "kernels.h"

namespace svc {

constexpr int kMaxSubStreams = 8;

struct PackedGemm {
  f16* W = nullptr;
  float* bias = nullptr;
  int N = 0, Npad = 0, K = 0, Kpad = 0, Cp = 0, Cin = 0, taps = 0;
  int tap_mul = 1, tap_add = 0, istride = 1;
  bool bf16 = false;  // W (and so the GEMM's operands) in bfloat16 (the bf16 operand variant, common.h Op16)
  f16* Wfrag = nullptr;  // W in a kernel's fragment order: the DiffSVC residual projections (res_proj.hip), the dilated
                         // convs (gate_ws.hip)
};

// host-side rounding of a weight to the 16-bit operand format: binary16 (default) or bfloat16 (round to nearest even)
static inline uint16_t bf16_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline f16 enc16_host(float v, bool bf) {
  if (!bf) return (f16)v;
  const uint16_t b = bf16_bits(v);
  f16 h;
  memcpy(&h, &b, 2);
  return h;
}
static inline float round16_host(float v, bool bf) {
  if (!bf) return (float)(f16)v;
  const uint32_t u = (uint32_t)bf16_bits(v) << 16;
  float r;
  memcpy(&r, &u, 4);
  return r;
}

struct Param {
  const float* host = nullptr;
  std::vector<int64_t> shape;
  int64_t numel = 0;
};

struct WBlock {
  float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  PackedGemm qkv, out, fc1, fc2;
  PackedGemm v;         // value projection as its own GEMM when its weight split differs from q / k's
  bool split_v = false;  // (then qkv holds the q and k columns only)
};

struct HBlock {  // post-LN fairseq TransformerSentenceEncoderLayer
  float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  PackedGemm qkv, out, fc1, fc2;
};

struct ActP {
  float *alpha, *beta, *filt;
};

struct VStage {
  int cin, cout, rate, k;
  std::vector<PackedGemm> phases;
  // rate-2 ConvTranspose as ONE conv over the input rows (tune.amp_ups): output columns r * cout + n of input row t are
  // output row 2t + r, so [L][2 cout] is the time-major output; 3 taps at offsets +1, 0, -1 (each phase's two taps in
  // its own GEMM's order, zeros for the tap it lacks); run by amp_conv's plain-conv form (cin = 2 cout = 48 / 96 / 192)
  PackedGemm upc;
  bool up_comb = false;
  // resblocks j: convs1[l], convs2[l], acts[2l], acts[2l+1]
  std::vector<std::vector<PackedGemm>> c1, c2;
  std::vector<std::vector<ActP>> acts;
  std::vector<int> rk;
  std::vector<std::vector<int>> rd;
};

}  // namespace svc

using namespace svc;  // svc_ctx and the C-ABI entry points are global (include/svc_hip.h)

// Device tables keyed by a parameter set (F0 front ends): an entry is built once and reused by every call with the same
// key, so a server alternating between parameter sets allocates nothing after the first call of each. At most kMax
// entries: beyond that the least recently used one is freed after the device has drained (a call in flight on any
// stream may still read it).
struct TableCache {
  static constexpr int kMax = 8;
  struct Entry {
    std::vector<double> key;
    double* dev;
    uint64_t used;
  };
  std::vector<Entry> e;
  uint64_t clock = 0;
  double* find(const double* key, int nk) {
    for (auto& x : e)
      if ((int)x.key.size() == nk && memcmp(x.key.data(), key, nk * sizeof(double)) == 0) {
        x.used = ++clock;
        return x.dev;
      }
    return nullptr;
  }
  // takes ownership of dev (hipMalloc'd)
  int insert(const double* key, int nk, double* dev) {
    if ((int)e.size() >= kMax) {
      size_t lru = 0;
      for (size_t i = 1; i < e.size(); ++i)
        if (e[i].used < e[lru].used) lru = i;
      SVC_HIP_CHECK(hipDeviceSynchronize());
      (void)hipFree(e[lru].dev);
      e.erase(e.begin() + (long)lru);
    }
    e.push_back(Entry{std::vector<double>(key, key + nk), dev, ++clock});
    return SVC_OK;
  }
  void clear() {
    for (auto& x : e) (void)hipFree(x.dev);
    e.clear();
  }
};

struct svc_ctx {
  int device = 0;
  Tuning tune, tune0;  // kernel switches (tune0: their values at creation, for "tune.reset")
  // ragged-batch length tables, one ring per stage (the feature stages run on their own stream)
  StageRing lens_feat, lens_main;
  StageRing lens_pcm;  // svc_pcm16: the length table and, behind it in the same slot, the zeroed peak scratch
  StageRing lens_loud;  // svc_loudness_match: the two length tables and, behind them in the same slot, the frame powers
  StageRing lens_stitch;  // svc_stitch: the chunk and song tables and, behind them in the same slot, the displacements
  StageRing lens_retr;  // svc_content_retrieve: the frames and sel tables
  StageRing lens_load;  // svc_load_pcm: the utterance and plan tables and the zeroed peak scratch (load_pcm.hip)
  std::map<std::string, Param> params;
  std::map<std::string, double> cfg;
  bool finalized = false;
  std::vector<void*> allocs;
  int64_t weight_bytes = 0;
  Arena ws;
  Arena auxws;  // workspace of the 24 kHz feature stages (mel / energy, F0): they may run on a side stream beside
               // the content encoder, which uses ws

  // features
  float *fb24 = nullptr, *fb16 = nullptr, *win_mel = nullptr, *win16 = nullptr;
  int *band24 = nullptr, *band16 = nullptr;  // [n_mels][3] nonzero band of each filter (lo, hi, offset in fb)
  int fb24_len = 0, fb16_len = 0;              // fb24 / fb16 hold only those bands, packed
  double *tw24 = nullptr, *tw16 = nullptr;     // FFT twiddles: [n_fft] (cos, -sin)(2 pi m / n_fft)
  int n_fft = 1024, hop = 256, n_mels = 100, fs = 24000;
  double fmin = 0, fmax = 12000, f0_min = 65, f0_max = 800;
  // content encoders in split-fp16 precision ("content.split" = 1 at finalize): every GEMM operand of Whisper /
  // HuBERT except the attention path is [hi | lo | hi] against [W_hi; W_hi; W_lo] weights (3x MFMA work)
  bool content_split = false;  // content_mode == 1
  int content_mode = 0;         // "content.split": 0 fp16, 1 split-fp16 operands (x3), 2 weight-split (x2, Whisper)
  bool head_split = true;  // DiffSVC skip_projection / output_projection on split-fp16 operands ("mapper.head_split")
  // bf16 operand variant ("operands.bf16" at finalize, BASELINE configs[4]'s fp16-vs-bf16 sweep): the DiffSVC,
  // conditioner and content-encoder GEMMs (and Whisper / HuBERT attention) take bfloat16 operands on
  // v_mfma_f32_16x16x32_bf16; BigVGAN stays binary16. pack_bf16: the weights being packed are for such a GEMM.
  bool bf16 = false;
  bool pack_bf16 = false;
  // whisper
  bool has_whisper = false;
  int wD = 0, wH = 0, wL = 0, wctx = 0, wmels = 80;
  PackedGemm wconv1, wconv2;
  int wstem_ld = 0;  // row stride (halves) of the conv stem's log-mel operand (split: 3 n_mels padded to 64)
  float *wpos = nullptr, *wlnp_g = nullptr, *wlnp_b = nullptr;
  std::vector<WBlock> wblocks;
  // hubert / contentvec (A8)
  bool has_hubert = false;
  int hC = 512, hD = 768, hH = 12, hLayers = 9, hFinal = 256, hPosK = 128, hPosG = 16;
  std::vector<PackedGemm> hconv;    // feature extractor conv_layers 0..6 (layer 0 as a 2-tap GEMM over 5-sample rows)
  std::vector<int> hconv_k, hconv_s;
  float *hgn_g = nullptr, *hgn_b = nullptr, *hln_g = nullptr, *hln_b = nullptr, *henc_ln_g = nullptr, *henc_ln_b = nullptr;
  PackedGemm hproj, hfinal;
  std::vector<PackedGemm> hpos;     // one GEMM per pos_conv group
  std::vector<HBlock> hblocks;
  // mapper
  bool has_mapper = false;
  int C = 384, n_mel = 100, n_layers = 20, dil_cycle = 4, steps = 1000, content_dim = 1024, n_bins = 256;
  PackedGemm content_lin, cp_all, melpre, skipproj, outproj;
  std::vector<PackedGemm> dil, outres;  // per layer: dilated conv (paired), residual half of output_projection
  PackedGemm skip_all;                  // skip halves of all layers' output_projection, K = layers * C
  float *emb_m = nullptr, *emb_l = nullptr, *emb_s = nullptr, *mbins = nullptr, *ebins = nullptr;
  float* dproj = nullptr;  // [steps][layers][C]
  std::vector<float> alphas_cumprod_f32, sra, srm1, pc1, pc2, plogvar;
  float *mel_min = nullptr, *mel_max = nullptr;
  // vocoder
  bool has_vocoder = false;
  int v_in = 100, v_c0 = 1536;
  bool v_rb2 = false;  // vocoder resblocks are AMPBlock2 (config resblock "2")
  PackedGemm vpre;
  std::vector<VStage> vstages;
  ActP vact_post;
  float* vpost_w = nullptr;
  float vpost_b = 0;
  float* fade = nullptr;
  int nfade = 5120;
  // sampler sub-batch streams (svc_diffsvc_sample), created on first use
  hipStream_t sub_streams[kMaxSubStreams] = {};
  hipEvent_t ev_fork = nullptr, ev_join[kMaxSubStreams] = {};
  int n_sub_streams = 0;
  int ensure_sub_streams(int n) {
    if (!ev_fork && hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess) return SVC_ERR_HIP;
    for (; n_sub_streams < n; ++n_sub_streams) {
      if (hipStreamCreateWithFlags(&sub_streams[n_sub_streams], hipStreamNonBlocking) != hipSuccess) return SVC_ERR_HIP;
      if (hipEventCreateWithFlags(&ev_join[n_sub_streams], hipEventDisableTiming) != hipSuccess) return SVC_ERR_HIP;
    }
    return SVC_OK;
  }
  int hop_out = 256;
  // pYIN's device tables (beta priors, banded log-transitions, bin frequencies) per (fs, f0_min, f0_max, win, hop), and
  // Praat-AC F0's window / window autocorrelation / FFT twiddle tables per (fs, f0_min) (f0.hip f0_tables): built once per
  // parameter set and reused by every later call with that set (TableCache)
  TableCache pyin_tabs, f0_tabs;
  ~svc_ctx() {
    pyin_tabs.clear();
    f0_tabs.clear();
  }
};

namespace svc {

// engine.hip
double cfgv(svc_ctx* c, const char* k, double d);
const f16* zero_page();
int run_gemm(const PackedGemm& g, const f16* X, int ldx, int Cvalid, int B, int T_in, int T_out, EpiArgs e,
             hipStream_t s, const char* site = "", const int* tv = nullptr, int tv_mul = 1);
EpiArgs epi();
// finalize.hip
int pack_conv1d(svc_ctx* c, PackedGemm& g, const float* w, const float* bias, int Cout, int Cin, int k, int Cp,
                int dil, int pad, int stride, const std::vector<int>* perm = nullptr, const float* wn_g = nullptr);
int pack_conv_transpose(svc_ctx* c, std::vector<PackedGemm>& phases, const float* v, const float* wn_g,
                        const float* bias, int Cin, int Cout, int k, int s, int pad);
int pack_conv_transpose_comb(svc_ctx* c, VStage& S, const float* v, const float* wn_g, const float* bias);
int pack_conv1d_opt(svc_ctx* c, PackedGemm& g, const float* w, const float* bias, int Cout, int Cin, int k, int Cp,
                    int dil, int pad, int stride, bool split);
std::vector<int> pair_perm(int C);
int pack_skip_all(svc_ctx* c, PackedGemm& g, const float* const* ow, const float* const* ob, int C, int NL);
int pack_cond_all(svc_ctx* c, PackedGemm& g, const float* const* cpw, const float* const* cpb, int C, int NL,
                  int cond_sz);
int build_features(svc_ctx* c);
int build_whisper(svc_ctx* c);
int build_hubert(svc_ctx* c);
int build_mapper(svc_ctx* c);
int build_stats(svc_ctx* c);
int build_vocoder(svc_ctx* c);
// stage_diffsvc.hip
int stage_frames(StageRing& ring, const int32_t* frames, int B, int T, hipStream_t s, const int** dev_out);
// The denoiser's steps, one launcher choice each (denoise / project_cond run them; the svc_op_diffsvc_* entry points
// run them one at a time). C: the residual channels; hi / lo: the split residual stream [B*T][C].
// mel_preprocess + ReLU + add (the layer-0 diffusion projection) into hi / lo
int diffsvc_melpre(const PackedGemm& melpre, const f16* x16, int ldx16, int n_mel, const float* add, f16* hi, f16* lo,
                   int C, int B, int T, hipStream_t s);
// dilated conv + conditioner projection (cp [B*T][2C], paired order) + gate into y16 [B*T][C]
int diffsvc_gate(const PackedGemm& dil, const f16* x16, const f16* cp, f16* y16, int C, int B, int T, const int* tv,
                 hipStream_t s);
// res_proj's row lanes as the kernel switches give them, -1: the tiled GEMM
int diffsvc_res_lanes();
// (hi + lo) - sub + g16 @ W_res + b, / sqrt(2), + add, back into hi / lo in place; lanes_cap: diffsvc_res_lanes().
// store_lo false (res_proj only; the tiled GEMM always writes lo): lo is read and not written
int diffsvc_residual(const PackedGemm& outres, const f16* g16, const float* sub, const float* add, f16* hi, f16* lo,
                     int C, int B, int T, int lanes_cap, bool store_lo, hipStream_t s);
// sum over the NL layer-major gate outputs (layer stride g_ls elements) of rows `rows` / sqrt(NL) into s16
// ([hi | lo | hi] of 3C when head_split, else C)
int diffsvc_skipsum(const PackedGemm& skip_all, const f16* g16, size_t g_ls, int NL, f16* s16, int C, bool head_split,
                    int rows, hipStream_t s);
// relu(skip_projection) and output_projection: one launch (diff_head) where it fits, else two GEMMs through u16
int diffsvc_head(const PackedGemm& skipproj, const PackedGemm& outproj, const f16* s16, f16* u16, float* eps, int C,
                 int n_mel, bool head_split, int B, int T, hipStream_t s);
// cond f32 [B*T][C] -> cond16 [hi | lo | hi] -> every layer's conditioner projection, layer-major (stride cp_ls)
int diffsvc_condproj(const PackedGemm& cp_all, const float* cond, f16* cond16, f16* cp16, size_t cp_ls, int C,
                     bool bf16, int B, int T, hipStream_t s);
// ops.hip
int op_ws(svc_ctx** tmp);

// Utterance-aligned sub-batches of a batch of B on the context's sub-streams: sub-batch h is the utterances
// [b0(h), b0(h + 1)) on stream(h). With one sub-batch that is the caller's stream, and fork / join enqueue nothing.
struct SubBatches {
  svc_ctx* c = nullptr;
  hipStream_t s = nullptr;  // the caller's stream
  int B = 0, n = 1;         // n = clamp(requested, 1, min(B, kMaxSubStreams))
  int b0(int h) const { return h * B / n; }
  hipStream_t stream(int h) const { return n == 1 ? s : c->sub_streams[h]; }
  // the sub-streams wait for what is enqueued on s so far
  int fork(svc_ctx* ctx, int requested, int batch, hipStream_t caller) {
    c = ctx;
    s = caller;
    B = batch;
    n = std::max(1, std::min(std::min(requested, B), (int)kMaxSubStreams));
    if (int st = c->ensure_sub_streams(n)) return st;
    if (n == 1) return SVC_OK;
    SVC_HIP_CHECK(hipEventRecord(c->ev_fork, s));
    for (int h = 0; h < n; ++h) SVC_HIP_CHECK(hipStreamWaitEvent(c->sub_streams[h], c->ev_fork, 0));
    return SVC_OK;
  }
  // s waits for what is enqueued on every sub-stream
  int join() const {
    if (n == 1) return SVC_OK;
    for (int h = 0; h < n; ++h) {
      SVC_HIP_CHECK(hipEventRecord(c->ev_join[h], c->sub_streams[h]));
      SVC_HIP_CHECK(hipStreamWaitEvent(s, c->ev_join[h], 0));
    }
    return SVC_OK;
  }
};

}  // namespace svc

#define CTX_READY(c)                                                        \
  TuningScope tuning_scope_((c) ? &(c)->tune : nullptr);                    \
  do {                                                                      \
    SVC_REQUIRE((c), "null context");                                       \
    if (!(c)->finalized) {                                                  \
      set_error("context not finalized");                                   \
      return SVC_ERR_STATE;                                                 \
    }                                                                       \
    SVC_HIP_CHECK(hipSetDevice((c)->device));                               \
  } while (0)
