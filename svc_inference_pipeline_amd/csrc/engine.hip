// Native runtime of the SVC hot path: error state, live profiling, kernel switches, the implicit-GEMM dispatch
// (run_gemm) and the context's lifecycle and configuration behind the C-ABI (include/svc_hip.h). Weight packing is
// finalize.hip, the stages' orchestration the stage_*.hip files, the op-level test entry points ops.hip.
#include <ctype.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <set>
#include <tuple>

#include "engine.h"

namespace svc {

// ---------------------------------------------------------------------------- errors
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* get_error() { return g_err; }

// ---------------------------------------------------------------------------- live profiling
struct ProfRec {
  std::string name;
  hipEvent_t a, b;
  double flops, bytes;
};
static bool g_prof = false;
static std::string g_prof_filter;  // when non-empty, only kernels whose name starts with it are recorded
static std::vector<ProfRec> g_prof_recs;
static std::vector<hipEvent_t> g_ev_pool;

static hipEvent_t ev_get() {
  if (!g_ev_pool.empty()) {
    hipEvent_t e = g_ev_pool.back();
    g_ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

static thread_local const char* g_site = "";
void prof_site(const char* site) { g_site = site ? site : ""; }

int prof_begin(const char* name, double flops, double bytes, hipStream_t s) {
  if (!g_prof) return -1;
  if (!g_prof_filter.empty() && strncmp(name, g_prof_filter.c_str(), g_prof_filter.size()) != 0) return -1;
  std::string full = std::string(name) + (g_site[0] ? std::string("@") + g_site : std::string());
  ProfRec r{full, ev_get(), ev_get(), flops, bytes};
  if (!r.a || !r.b) return -1;
  (void)hipEventRecord(r.a, s);
  g_prof_recs.push_back(r);
  return (int)g_prof_recs.size() - 1;
}

void prof_end(int tok, hipStream_t s) {
  if (tok >= 0 && tok < (int)g_prof_recs.size()) (void)hipEventRecord(g_prof_recs[tok].b, s);
}

// ---------------------------------------------------------------------------- kernel switches
static thread_local const Tuning* t_tuning = nullptr;

// the switches by name: (tune.<name>, SVC_<NAME> environment override at context creation)
template <typename T>
static int* tuning_field(T& t, const char* name) {
  struct {
    const char* name;
    int* v;
  } ints[] = {{"gemm_variant", &t.gemm_variant},       {"gemm3_direct", &t.gemm3_direct},
              {"whisper_streams", &t.whisper_streams}, {"sampler_streams", &t.sampler_streams},
              {"vocoder_streams", &t.vocoder_streams}, {"diff_head", &t.diff_head},
              {"amp_maxc", &t.amp_maxc},               {"res_proj", &t.res_proj},
              {"gate_ws", &t.gate_ws},                 {"amp_ups", &t.amp_ups},
              {"retrieve_splits", &t.retrieve_splits}};
  for (auto& it : ints)
    if (strcmp(it.name, name) == 0) return it.v;
  return nullptr;
}

void Tuning::from_env() {
  for (const char* name : {"gemm_variant", "gemm3_direct", "whisper_streams", "sampler_streams", "vocoder_streams",
                           "diff_head", "amp_maxc", "res_proj", "gate_ws", "amp_ups", "retrieve_splits"}) {
    std::string env = "SVC_";
    for (const char* q = name; *q; ++q) env += (char)toupper((unsigned char)*q);
    if (const char* v = getenv(env.c_str())) *tuning_field(*this, name) = atoi(v);
  }
  if (const char* v = getenv("SVC_SITE_VARIANT")) site_variant = v;
}

bool Tuning::set(const char* name, double v) {
  int* f = tuning_field(*this, name);
  if (f) *f = (int)v;
  return f != nullptr;
}

bool Tuning::get(const char* name, double* v) const {
  int* f = tuning_field(const_cast<Tuning&>(*this), name);
  if (f) *v = *f;
  return f != nullptr;
}

const Tuning& tuning() {
  static const Tuning env_default = [] {
    Tuning t;
    t.from_env();
    return t;
  }();
  return t_tuning ? *t_tuning : env_default;
}
TuningScope::TuningScope(const Tuning* t) : prev(t_tuning) { t_tuning = t; }
TuningScope::~TuningScope() { t_tuning = prev; }
int ensure_dyn_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::tuple<const void*, int, int>> done;
  int dev = 0;
  SVC_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (done.count({fn, dev, bytes})) return SVC_OK;
  SVC_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.insert({fn, dev, bytes});
  return SVC_OK;
}

// the arena's device memory (arena.h). hipFree waits for the device, so no launch still reads the block it replaces.
int Arena::reserve(size_t bytes) {
  if (bytes <= cap) return SVC_OK;
  if (base) SVC_HIP_CHECK(hipFree(base));
  base = nullptr;
  cap = 0;
  SVC_HIP_CHECK(hipMalloc(&base, bytes));
  cap = bytes;
  return SVC_OK;
}

double cfgv(svc_ctx* c, const char* k, double d) {
  auto it = c->cfg.find(k);
  return it == c->cfg.end() ? d : it->second;
}

// 4 KiB of zeros: the LDS-DMA source of padded / out-of-range conv rows (conv_gemm2)
const f16* zero_page() {
  static f16* z = nullptr;
  if (!z) {
    if (hipMalloc(&z, 4096) != hipSuccess) return nullptr;
    if (hipMemset(z, 0, 4096) != hipSuccess) return nullptr;
  }
  return z;
}

// the kernel arguments of one implicit-GEMM launch over the packed weights g (run_gemm, the dual launches)
static ConvGemmArgs gemm_args(const PackedGemm& g, const f16* X, int ldx, int Cvalid, int B, int T_in, int T_out,
                              EpiArgs& e) {
  ConvGemmArgs a{};
  a.X = X;
  a.ldx = ldx;
  a.T_in = T_in;
  a.Cp = g.Cp;
  a.Cvalid = Cvalid;
  a.W = g.W;
  a.K = g.K;
  a.Kpad = g.Kpad;
  a.tap_mul = g.tap_mul;
  a.tap_add = g.tap_add;
  a.istride = g.istride;
  a.B = B;
  a.T_out = T_out;
  a.N = g.N;
  a.bf16 = g.bf16 ? 1 : 0;
  a.Wfrag = g.Wfrag;
  if (e.T_ostore == 0) {
    e.T_ostore = T_out;
    e.ostride = 1;
    e.ophase = 0;
  }
  if (!e.bias) e.bias = g.bias;
  return a;
}

// tv / tv_mul: ragged batches, utterance b's valid input rows are tv[b] * tv_mul (ConvGemmArgs::tv; NULL = all)
int run_gemm(const PackedGemm& g, const f16* X, int ldx, int Cvalid, int B, int T_in, int T_out, EpiArgs e,
             hipStream_t s, const char* site, const int* tv, int tv_mul) {
  prof_site(site);
  const Tuning& tu = tuning();
  // conv_gemm3's register epilogues (gemm3_direct mask, gemm3.hip) stay off inside the DiffSVC sampler unless
  // bit 8 is set: there its sub-batch GEMMs run beside the gate GEMMs of the other streams, which then ran slower
  if (!(tu.gemm3_direct & 8) && site && strncmp(site, "diffsvc.", 8) == 0) e.no_reg_epi = 1;
  ConvGemmArgs a = gemm_args(g, X, ldx, Cvalid, B, T_in, T_out, e);
  a.tv = tv;
  a.tv_mul = tv_mul;
  const bool pair = e.kind == EPI_GATE;
  // gemm_variant: 15 (default) = conv_gemm3 with the fitted tile choice, except the DiffSVC gate GEMM (paired
  // epilogue, K = 1152) which runs conv_gemm4 with its register gate epilogue (24; 3-9 % faster than conv_gemm3);
  // 10..14 = a fixed conv_gemm3 tile; 20 / 24 = conv_gemm4 with the LDS-staged / register gate epilogue.
  int variant = tu.gemm_variant;
  // site_variant = "site=variant,...": per-call-site override (tile / kernel A/B runs, e.g. diffsvc.outproj=20)
  if (!tu.site_variant.empty()) {
    const char* senv = tu.site_variant.c_str();
    const size_t sl = site ? strlen(site) : 0;
    for (const char* p = senv; sl && (p = strstr(p, site)) != nullptr; p += sl)
      if ((p == senv || p[-1] == ',') && p[sl] == '=') {
        variant = atoi(p + sl + 1);
        break;
      }
  }
  // the DiffSVC dilated conv + gate: the weight-stationary row stream (gate_ws.hip) where it fits, else conv_gemm4
  if (variant == 15 && pair && tu.gate_ws && gate_ws_fits(a, e)) return gate_ws(a, e, s);
  if (variant == 15 && pair) variant = 24;
  // The skip-sum GEMM of a sampler sub-batch (K = 20 x 384, M <= 20 k rows) takes conv_gemm3's 256 x 128 tile although
  // pick3's fit prefers narrower-M tiles alone: beside the other sampler stream it measured +1.5 % end to end (826-828
  // vs 813-818 audio-s/s in three alternating rounds, profiles/r03w_skipsum_tile_ab.txt)
  if (variant == 15 && site && strcmp(site, "diffsvc.skipsum") == 0 && (int64_t)B * T_out <= 20000) variant = 12;
  SVC_REQUIRE((variant >= 10 && variant <= 16) || variant == 20 || variant == 24, "gemm_variant %d: 10..16, 20 or 24",
              variant);
  // N <= 64 (the last BigVGAN up-sampling phases, 48 / 24 channels) takes conv_gemm3's 128 x 128 tile: 1.9 vs
  // 3.0 ms per step on the round-1 256 x 64 / 256 x 32 tiles (tools/ab_ups.sh), although 63-81 % of its N is padding
  if (variant == 20 || variant == 24) {
    if (pair || g.N > 64) return conv_gemm4(a, e, zero_page(), s, variant == 24);
    variant = 15;  // conv_gemm4's tiles are 128 wide in N: small-N GEMMs keep conv_gemm3
  }
  return conv_gemm3(a, e, zero_page(), variant - 10, s);
}

EpiArgs epi() {
  EpiArgs e{};
  e.kind = EPI_GENERIC;
  e.acc_div = 1.0f;
  return e;
}

}  // namespace svc

// ============================================================================ C-ABI
extern "C" {

const char* svc_last_error(void) { return get_error(); }
// 2: ragged-batch length tables (utt_samples / frames) in the stage entry points
int svc_abi_version(void) { return 3; }

svc_status svc_ctx_create(int device, svc_ctx** out) {
  SVC_REQUIRE(out, "svc_ctx_create: null out");
  int n = 0;
  SVC_HIP_CHECK(hipGetDeviceCount(&n));
  SVC_REQUIRE(device >= 0 && device < n, "svc_ctx_create: device %d of %d", device, n);
  SVC_HIP_CHECK(hipSetDevice(device));
  svc_ctx* c = new svc_ctx();
  c->device = device;
  c->tune.from_env();
  c->tune0 = c->tune;
  *out = c;
  return SVC_OK;
}

svc_status svc_ctx_destroy(svc_ctx* c) {
  if (!c) return SVC_OK;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->ws.base) (void)hipFree(c->ws.base);
  if (c->auxws.base) (void)hipFree(c->auxws.base);
  for (int i = 0; i < c->n_sub_streams; ++i) {
    (void)hipStreamDestroy(c->sub_streams[i]);
    (void)hipEventDestroy(c->ev_join[i]);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  c->lens_feat.release();
  c->lens_main.release();
  c->lens_pcm.release();
  c->lens_loud.release();
  c->lens_stitch.release();
  c->lens_retr.release();
  c->lens_load.release();
  delete c;
  return SVC_OK;
}

// the configuration keys the context reads (config.json's, flattened as SVCEngine._set_config writes them, and the
// precision keys): a misspelt or obsolete key fails instead of silently leaving its default in place
static bool known_config_key(const char* key) {
  static const char* exact[] = {
      "fs", "n_fft", "hop_length", "win_length", "n_mels", "fmin", "fmax", "f0_min", "f0_max",
      "mapper.residual_channels", "mapper.residual_layer_num", "mapper.n_mel", "mapper.diffusion_fc_size",
      "mapper.dilation_cycle_length", "mapper.residual_kernel_size", "mapper.noise_schedule_factors.0",
      "mapper.noise_schedule_factors.1", "mapper.head_split", "content.split", "content.wsplit_attn",
      "content.wsplit_mlp", "content.wsplit_qk", "content.wsplit_v", "content.wsplit_out", "hubert.output_layer",
      "vocoder.n_stages", "vocoder.n_kernels", "vocoder.upsample_initial_channel", "vocoder.input_dim",
      "vocoder.resblock", "vocoder.snake", "vocoder.snake_logscale", "operands.bf16"};
  for (const char* k : exact)
    if (strcmp(key, k) == 0) return true;
  // indexed lists: <prefix><i> or, for the dilations, <prefix><j>.n / <prefix><j>.<l>
  static const char* indexed[] = {"vocoder.upsample_rates.", "vocoder.upsample_kernel_sizes.",
                                  "vocoder.resblock_kernel_sizes.", "vocoder.resblock_dilation_sizes."};
  for (int i = 0; i < 4; ++i) {
    const size_t n = strlen(indexed[i]);
    if (strncmp(key, indexed[i], n) != 0) continue;
    const char* p = key + n;
    if (!isdigit((unsigned char)*p)) return false;
    while (isdigit((unsigned char)*p)) ++p;
    if (i < 3) return *p == 0;
    if (*p++ != '.') return false;
    if (strcmp(p, "n") == 0) return true;
    if (!isdigit((unsigned char)*p)) return false;
    while (isdigit((unsigned char)*p)) ++p;
    return *p == 0;
  }
  return false;
}

svc_status svc_ctx_set_config(svc_ctx* c, const char* key, double value) {
  SVC_REQUIRE(key, "set_config: null key");
  if (strncmp(key, "tune.", 5) == 0) {  // kernel switches (Tuning); NULL context: the op-level entry points'
    if (!c) op_ws(&c);
    if (strcmp(key + 5, "reset") == 0) {
      c->tune = c->tune0;
      return SVC_OK;
    }
    SVC_REQUIRE(c->tune.set(key + 5, value), "set_config: unknown kernel switch %s", key);
    return SVC_OK;
  }
  SVC_REQUIRE(c, "set_config: null context");
  SVC_REQUIRE(known_config_key(key), "set_config: unknown configuration key %s", key);
  c->cfg[key] = value;
  return SVC_OK;
}

int svc_config_key_known(const char* key) { return key && known_config_key(key) ? 1 : 0; }

svc_status svc_ctx_get_config(svc_ctx* c, const char* key, double* value) {
  SVC_REQUIRE(key && value, "get_config: null argument");
  if (strncmp(key, "tune.", 5) == 0) {
    if (!c) op_ws(&c);
    SVC_REQUIRE(c->tune.get(key + 5, value), "get_config: unknown kernel switch %s", key);
    return SVC_OK;
  }
  SVC_REQUIRE(c, "get_config: null context");
  auto it = c->cfg.find(key);
  SVC_REQUIRE(it != c->cfg.end(), "get_config: %s is not set", key);
  *value = it->second;
  return SVC_OK;
}

svc_status svc_ctx_add_param(svc_ctx* c, const char* name, const float* host, int ndim, const int64_t* shape) {
  SVC_REQUIRE(c && name && host && ndim >= 0 && ndim <= 8, "add_param: bad args");
  if (c->finalized) {
    set_error("add_param after finalize");
    return SVC_ERR_STATE;
  }
  Param p;
  p.host = host;
  p.numel = 1;
  for (int i = 0; i < ndim; ++i) {
    p.shape.push_back(shape[i]);
    p.numel *= shape[i];
  }
  c->params[name] = p;
  return SVC_OK;
}

svc_status svc_ctx_finalize(svc_ctx* c) {
  SVC_REQUIRE(c, "finalize: null");
  if (c->finalized) {
    set_error("finalize called twice");
    return SVC_ERR_STATE;
  }
  SVC_HIP_CHECK(hipSetDevice(c->device));
  int st;
  if ((st = build_features(c))) return st;
  bool any_w = false, any_m = false, any_v = false, any_h = false;
  for (auto& kv : c->params) {
    any_w |= kv.first.rfind("whisper.", 0) == 0;
    any_h |= kv.first.rfind("hubert.", 0) == 0;
    any_m |= kv.first.rfind("mapper.", 0) == 0;
    any_v |= kv.first.rfind("vocoder.", 0) == 0;
  }
  c->content_mode = (int)cfgv(c, "content.split", 0);
  SVC_REQUIRE(c->content_mode >= 0 && c->content_mode <= 2, "content.split %d: 0 fp16, 1 split-fp16, 2 weight-split",
              c->content_mode);
  c->content_split = c->content_mode == 1;
  c->bf16 = cfgv(c, "operands.bf16", 0) != 0;
  c->pack_bf16 = c->bf16;  // the content encoders, the conditioner and DiffSVC
  if (any_w && (st = build_whisper(c))) return st;
  if (any_h && (st = build_hubert(c))) return st;
  if (any_m && (st = build_mapper(c))) return st;
  if (!any_m && c->params.count("stats.mel_min") && (st = build_stats(c))) return st;  // vocoder-only copy-synthesis
  c->pack_bf16 = false;  // BigVGAN stays binary16
  if (any_v && (st = build_vocoder(c))) return st;
  c->params.clear();  // host arrays are no longer referenced
  c->finalized = true;
  return SVC_OK;
}

// One of the context's own sub-streams (created on first use, the same ones the sampler / vocoder / Whisper
// sub-batches run on), so a host pipeline can overlap stage calls without adding a stream (measured: 737 -> 644
// audio-s/s when the F0 stage got a stream of its own, presumably from sharing the 4 hardware queues).
svc_status svc_ctx_stream(svc_ctx* c, int index, void** stream) {
  SVC_REQUIRE(c && stream && index >= 0 && index < kMaxSubStreams, "ctx_stream: bad args");
  SVC_HIP_CHECK(hipSetDevice(c->device));
  int st;
  if ((st = c->ensure_sub_streams(index + 1))) return st;
  *stream = (void*)c->sub_streams[index];
  return SVC_OK;
}

svc_status svc_ctx_memory(svc_ctx* c, int64_t* wb, int64_t* wsb) {
  SVC_REQUIRE(c, "memory: null");
  if (wb) *wb = c->weight_bytes;
  if (wsb) *wsb = (int64_t)c->ws.cap;
  return SVC_OK;
}

svc_status svc_profile_enable(int enable) {
  if (!enable || !g_prof) {
    for (auto& r : g_prof_recs) {
      g_ev_pool.push_back(r.a);
      g_ev_pool.push_back(r.b);
    }
    g_prof_recs.clear();
  }
  g_prof = enable != 0;
  return SVC_OK;
}

svc_status svc_profile_filter(const char* kernel_prefix) {
  g_prof_filter = kernel_prefix ? kernel_prefix : "";
  return SVC_OK;
}

svc_status svc_profile_read(int idx, char* name, int name_len, double* total_ms, int64_t* launches, double* flops,
                            double* bytes, int* n_kernels) {
  // aggregate by kernel name (synchronises on the recorded events)
  std::vector<std::string> names;
  std::map<std::string, std::tuple<double, int64_t, double, double>> agg;
  for (auto& r : g_prof_recs) {
    SVC_HIP_CHECK(hipEventSynchronize(r.b));
    float ms = 0;
    SVC_HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
    if (!agg.count(r.name)) names.push_back(r.name);
    auto& t = agg[r.name];
    std::get<0>(t) += ms;
    std::get<1>(t) += 1;
    std::get<2>(t) += r.flops;
    std::get<3>(t) += r.bytes;
  }
  if (n_kernels) *n_kernels = (int)names.size();
  if (idx < 0 || idx >= (int)names.size()) return SVC_OK;
  auto& t = agg[names[idx]];
  if (name && name_len > 0) snprintf(name, name_len, "%s", names[idx].c_str());
  if (total_ms) *total_ms = std::get<0>(t);
  if (launches) *launches = std::get<1>(t);
  if (flops) *flops = std::get<2>(t);
  if (bytes) *bytes = std::get<3>(t);
  return SVC_OK;
}

}  // extern "C"
