// svc_ctx_finalize's work: the feature tables, and each model's weights folded (weight_norm) and packed into the
// kernels' MFMA layouts (build_features / build_whisper / build_hubert / build_mapper / build_vocoder).
#include <math.h>

#include "engine.h"

namespace svc {

// ---------------------------------------------------------------------------- host helpers
static std::vector<float> slaney_mel(int sr, int n_fft, int n_mels, double f_lo, double f_hi) {
  auto hz2mel = [](double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
  };
  auto mel2hz = [](double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
  };
  const int nb = 1 + n_fft / 2;
  std::vector<double> fftf(nb), melf(n_mels + 2);
  // np.fft.rfftfreq(n, 1/sr) = k * (1 / (n * (1/sr)))
  const double val = 1.0 / ((double)n_fft * (1.0 / (double)sr));
  for (int k = 0; k < nb; ++k) fftf[k] = k * val;
  const double m0 = hz2mel(f_lo), m1 = hz2mel(f_hi);
  // np.linspace(start, stop, num): step = (stop-start)/(num-1); y = arange*step + start; y[-1] = stop
  const int num = n_mels + 2;
  const double step = (m1 - m0) / (num - 1);
  for (int i = 0; i < num; ++i) melf[i] = mel2hz(i == num - 1 ? m1 : i * step + m0);
  std::vector<float> w((size_t)n_mels * nb);
  for (int i = 0; i < n_mels; ++i) {
    const double fd0 = melf[i + 1] - melf[i], fd1 = melf[i + 2] - melf[i + 1];
    const double enorm = 2.0 / (melf[i + 2] - melf[i]);
    for (int k = 0; k < nb; ++k) {
      double lower = -(melf[i] - fftf[k]) / fd0;
      double upper = (melf[i + 2] - fftf[k]) / fd1;
      double v = fmax(0.0, fmin(lower, upper));
      float vf = (float)v;                      // weights[i] = ... stored in the f32 array
      w[(size_t)i * nb + k] = (float)((double)vf * enorm);  // weights *= enorm (f32 *= f64)
    }
  }
  return w;
}

// W_n^m = exp(-2 pi i m / n) as interleaved (re, im) f64 pairs
static std::vector<double> fft_twiddles(int n) {
  std::vector<double> t(2 * (size_t)n);
  for (int m = 0; m < n; ++m) {
    const double a = 2.0 * M_PI * (double)m / (double)n;
    t[2 * (size_t)m] = cos(a);
    t[2 * (size_t)m + 1] = -sin(a);
  }
  return t;
}

// The nonzero band [lo, hi) of each filter row, packed (the DFT kernel keeps only those weights, in LDS):
// band[3m .. 3m+2] = lo, hi, offset of the band in the packed weights
struct FilterBands {
  std::vector<float> w;
  std::vector<int> band;
};
static FilterBands filter_bands(const std::vector<float>& fb, int n_mels) {
  const int nb = (int)(fb.size() / n_mels);
  FilterBands r;
  r.band.assign(3 * n_mels, 0);
  for (int m = 0; m < n_mels; ++m) {
    int lo = nb, hi = 0;
    for (int k = 0; k < nb; ++k)
      if (fb[(size_t)m * nb + k] != 0.f) {
        lo = std::min(lo, k);
        hi = k + 1;
      }
    if (hi == 0) lo = 0;
    r.band[3 * m] = lo;
    r.band[3 * m + 1] = hi;
    r.band[3 * m + 2] = (int)r.w.size();
    for (int k = lo; k < hi; ++k) r.w.push_back(fb[(size_t)m * nb + k]);
  }
  return r;
}

static std::vector<float> hann_periodic(int n) {
  std::vector<float> w(n);
  for (int j = 0; j < n; ++j) w[j] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * j / n));
  return w;
}

namespace {

int dev_upload(svc_ctx* c, const void* host, size_t bytes, void** out) {
  void* p = nullptr;
  SVC_HIP_CHECK(hipMalloc(&p, bytes > 0 ? bytes : 16));
  if (bytes) SVC_HIP_CHECK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
  c->allocs.push_back(p);
  c->weight_bytes += (int64_t)bytes;
  *out = p;
  return SVC_OK;
}

template <typename T>
int upload_vec(svc_ctx* c, const std::vector<T>& v, T** out) {
  return dev_upload(c, v.data(), v.size() * sizeof(T), reinterpret_cast<void**>(out));
}

const Param* getp(svc_ctx* c, const std::string& name, std::initializer_list<int64_t> shape) {
  auto it = c->params.find(name);
  if (it == c->params.end()) {
    set_error("missing parameter '%s'", name.c_str());
    return nullptr;
  }
  std::vector<int64_t> want(shape);
  if (want.size() != it->second.shape.size()) {
    set_error("parameter '%s': expected %zu dims, got %zu", name.c_str(), want.size(), it->second.shape.size());
    return nullptr;
  }
  for (size_t i = 0; i < want.size(); ++i)
    if (want[i] >= 0 && want[i] != it->second.shape[i]) {
      set_error("parameter '%s': dim %zu expected %lld got %lld", name.c_str(), i, (long long)want[i],
                (long long)it->second.shape[i]);
      return nullptr;
    }
  return &it->second;
}

#define GETP(var, name, ...)                           \
  const Param* var = getp(c, (name), {__VA_ARGS__});   \
  if (!var) return SVC_ERR_INVALID;

int upload_param(svc_ctx* c, const Param* p, float** out) {
  return dev_upload(c, p->host, (size_t)p->numel * sizeof(float), reinterpret_cast<void**>(out));
}

// generic packer: W16[n][tap*Cp + ci] = wget(n, ci, tap), bias[n] = bget(n)
template <typename WG, typename BG>
int pack_gemm(svc_ctx* c, PackedGemm& g, int N, int Cin, int Cp, int taps, WG wget, BG bget) {
  g.N = N;
  g.Cin = Cin;
  g.Cp = Cp;
  g.taps = taps;
  g.K = taps * Cp;
  g.Kpad = (int)round_up(g.K, 64);
  g.Npad = (int)std::max(round_up(N, 256), round_up(N, 384));  // every conv_gemm2/3 tile width fits
  g.bf16 = c->pack_bf16;
  std::vector<f16> w((size_t)g.Npad * g.Kpad, (f16)0.0f);  // +0 in both formats
  std::vector<float> b((size_t)g.Npad, 0.0f);
  for (int n = 0; n < N; ++n) {
    for (int t = 0; t < taps; ++t)
      for (int ci = 0; ci < Cin; ++ci)
        w[(size_t)n * g.Kpad + (size_t)t * Cp + ci] = enc16_host(wget(n, ci, t), g.bf16);
    b[n] = bget(n);
  }
  int st = upload_vec(c, w, &g.W);
  if (st) return st;
  return upload_vec(c, b, &g.bias);
}

// Split-fp16 packing of a 1-tap GEMM for the [x_hi | x_lo | x_hi] operand of f32_to_f16x3:
// W'[n] = [f16(w) | f16(w) | f16(w - f16(w))] over K = 3 * Cin.
// Cp > 3 * Cin: each tap's K segment padded to Cp (zero weights), e.g. to a multiple of 64 for the buffer-descriptor
// K-loop (the Whisper conv stem: 3 x 80 -> 256 per tap, its operand rows padded to match).
template <typename WG, typename BG>
int pack_gemm_split3(svc_ctx* c, PackedGemm& g, int N, int Cin, WG wget, BG bget, int taps = 1, int Cp = 0) {
  return pack_gemm(
      c, g, N, 3 * Cin, Cp > 0 ? Cp : 3 * Cin, taps,
      [&](int n, int ci, int t) {
        const int seg = ci / Cin;
        const float w = wget(n, ci - seg * Cin, t);
        const float hi = round16_host(w, c->pack_bf16);
        return seg < 2 ? hi : w - hi;
      },
      bget);
}

// Weight-split packing of a 1-tap GEMM (plain f16 operand): W'[n] = [f16(w) | f16(w - f16(w))] as TWO taps with a
// zero row shift, so the implicit-GEMM A loader reads the same activation row for both and the product carries the
// weights to ~22 significand bits at 2x the MFMA work, with no extra activation bytes. The weight rounding is the
// larger share of an fp16 linear's error (precision).
template <typename WG, typename BG>
int pack_gemm_wsplit2(svc_ctx* c, PackedGemm& g, int N, int Cin, WG wget, BG bget) {
  int st = pack_gemm(
      c, g, N, Cin, Cin, 2,
      [&](int n, int ci, int t) {
        const float w = wget(n, ci, 0);
        const float hi = round16_host(w, c->pack_bf16);
        return t == 0 ? hi : w - hi;
      },
      bget);
  g.tap_mul = 0;
  g.tap_add = 0;
  g.istride = 1;
  return st;
}

// a content-encoder linear in precision mode `mode` (0 fp16, 1 split-fp16 operands, 2 weight-split)
template <typename WG, typename BG>
int pack_linear_mode(svc_ctx* c, PackedGemm& g, int N, int Cin, int mode, WG wget, BG bget) {
  if (mode == 1) return pack_gemm_split3(c, g, N, Cin, wget, bget);
  if (mode == 2) return pack_gemm_wsplit2(c, g, N, Cin, wget, bget);
  return pack_gemm(c, g, N, Cin, Cin, 1, wget, bget);
}

}  // namespace

// Conv1d weight [Cout][Cin][k] (optionally weight-normed along dim 0) into a packed GEMM
int pack_conv1d(svc_ctx* c, PackedGemm& g, const float* w, const float* bias, int Cout, int Cin, int k, int Cp,
                int dil, int pad, int stride, const std::vector<int>* perm, const float* wn_g) {
  std::vector<double> scale(Cout, 1.0);
  if (wn_g) {
    for (int o = 0; o < Cout; ++o) {
      double s = 0;
      for (int64_t i = 0; i < (int64_t)Cin * k; ++i) {
        double v = w[(int64_t)o * Cin * k + i];
        s += v * v;
      }
      scale[o] = (double)wn_g[o] / sqrt(s);
    }
  }
  auto src = [&](int n) { return perm ? (*perm)[n] : n; };
  int st = pack_gemm(
      c, g, Cout, Cin, Cp, k,
      [&](int n, int ci, int t) {
        int o = src(n);
        return (float)((double)w[((int64_t)o * Cin + ci) * k + t] * scale[o]);
      },
      [&](int n) { return bias ? bias[src(n)] : 0.0f; });
  g.tap_mul = dil;
  g.tap_add = -pad;
  g.istride = stride;
  return st;
}

// Conv1d [Cout][Cin][k] (+ bias) packed for a split-fp16 operand when `split`, else as pack_conv1d
int pack_conv1d_opt(svc_ctx* c, PackedGemm& g, const float* w, const float* bias, int Cout, int Cin, int k, int Cp,
                    int dil, int pad, int stride, bool split) {
  if (!split) return pack_conv1d(c, g, w, bias, Cout, Cin, k, Cp, dil, pad, stride);
  int st = pack_gemm_split3(
      c, g, Cout, Cin, [&](int n, int ci, int t) { return w[((int64_t)n * Cin + ci) * k + t]; },
      [&](int n) { return bias ? bias[n] : 0.0f; }, k);
  g.tap_mul = dil;
  g.tap_add = -pad;
  g.istride = stride;
  return st;
}

// ConvTranspose1d weight [Cin][Cout][k] (weight-normed along dim 0 = Cin) into `stride` phase GEMMs
int pack_conv_transpose(svc_ctx* c, std::vector<PackedGemm>& phases, const float* v, const float* wn_g,
                        const float* bias, int Cin, int Cout, int k, int s, int pad) {
  std::vector<double> scale(Cin, 1.0);
  if (wn_g) {
    for (int i = 0; i < Cin; ++i) {
      double acc = 0;
      for (int64_t j = 0; j < (int64_t)Cout * k; ++j) {
        double x = v[(int64_t)i * Cout * k + j];
        acc += x * x;
      }
      scale[i] = (double)wn_g[i] / sqrt(acc);
    }
  }
  if (k % s != 0) {
    set_error("conv_transpose: kernel %d not a multiple of stride %d", k, s);
    return SVC_ERR_INVALID;
  }
  phases.assign(s, PackedGemm());
  for (int r = 0; r < s; ++r) {
    const int base = (r + pad) % s, add = (r + pad) / s;
    int st = pack_gemm(
        c, phases[r], Cout, Cin, Cin, k / s,
        [&](int n, int ci, int j) {
          int kk = base + s * j;
          return (float)((double)v[((int64_t)ci * Cout + n) * k + kk] * scale[ci]);
        },
        [&](int n) { return bias ? bias[n] : 0.0f; });
    if (st) return st;
    phases[r].tap_mul = -1;
    phases[r].tap_add = add;
    phases[r].istride = 1;
  }
  return SVC_OK;
}

// The combined form of a rate-2 ConvTranspose (VStage::upc): phase r's tap j reads input row t + add_r - j with weight
// tap base_r + 2j (pack_conv_transpose); here tap q reads row t + 1 - q (amp_conv with k = 3, d = -1), so q = 1 - add_r + j.
// Built only where each phase's taps lie within offsets -1..1 and cin = 2 cout is an amp_conv plain-conv width. At cin 96 /
// 192 every 32-deep MFMA step lies within one tap, so each phase sums exactly its GEMM's products in its GEMM's order;
// at cin 48 the steps straddle taps and the zero tap shifts phase 0's grouping (fp32 summation order only).
int pack_conv_transpose_comb(svc_ctx* c, VStage& S, const float* v, const float* wn_g, const float* bias) {
  const int Cin = S.cin, Cout = S.cout, k = S.k, s = S.rate, pad = (S.k - S.rate) / 2;
  S.up_comb = false;
  if (s != 2 || k % s != 0 || Cin != 2 * Cout || !(Cin == 48 || Cin == 96 || Cin == 192)) return SVC_OK;
  for (int r = 0; r < s; ++r) {
    const int add = (r + pad) / s;
    if (add > 1 || add - (k / s - 1) < -1) return SVC_OK;
  }
  std::vector<double> scale(Cin, 1.0);
  if (wn_g) {
    for (int i = 0; i < Cin; ++i) {
      double acc = 0;
      for (int64_t j = 0; j < (int64_t)Cout * k; ++j) {
        double x = v[(int64_t)i * Cout * k + j];
        acc += x * x;
      }
      scale[i] = (double)wn_g[i] / sqrt(acc);
    }
  }
  int st = pack_gemm(
      c, S.upc, 2 * Cout, Cin, Cin, 3,
      [&](int n, int ci, int q) {
        const int r = n / Cout, o = n - r * Cout;
        const int base = (r + pad) % s, add = (r + pad) / s;
        const int j = q - 1 + add;
        if (j < 0 || j >= k / s) return 0.0f;
        return (float)((double)v[((int64_t)ci * Cout + o) * k + base + s * j] * scale[ci]);
      },
      [&](int n) { return bias ? bias[n % Cout] : 0.0f; });
  if (st) return st;
  S.up_comb = true;
  return SVC_OK;
}

// paired packing order (conv_gemm2 epilogue): packed n -> original channel ((n & 32) ? C : 0) + (n >> 6) * 32 + (n & 31)
std::vector<int> pair_perm(int C) {
  std::vector<int> p(2 * C);
  for (int n = 0; n < 2 * C; ++n) p[n] = ((n & 32) ? C : 0) + (n >> 6) * 32 + (n & 31);
  return p;
}

// The DiffSVC skip sum: sum over layers of skip_l = g_l @ Wskip_l + bskip_l as ONE GEMM over the concatenated gate
// outputs [g_0 .. g_{NL-1}] (K = NL * C): no per-layer f32 skip read-modify-write. ow[l] [C][C] / ob[l] [C]: the skip
// half of layer l's output_projection (its rows C..2C-1, modules/diffsvc.py:229-231)
int pack_skip_all(svc_ctx* c, PackedGemm& g, const float* const* ow, const float* const* ob, int C, int NL) {
  return pack_gemm(
      c, g, C, NL * C, NL * C, 1,
      [&](int n, int ci, int) {
        const int l = ci / C, k = ci % C;
        return ow[l][(int64_t)n * C + k];
      },
      [&](int n) {
        double b = 0;
        for (int l = 0; l < NL; ++l) b += ob[l][n];
        return (float)b;
      });
}

// All NL conditioner projections (cpw[l] [2C][cond_sz], cpb[l] [2C]) as one GEMM in split-fp16 precision, each layer's
// 2C columns in the paired order of its gate GEMM (pair_perm)
int pack_cond_all(svc_ctx* c, PackedGemm& g, const float* const* cpw, const float* const* cpb, int C, int NL,
                  int cond_sz) {
  const std::vector<int> perm = pair_perm(C);
  return pack_gemm_split3(
      c, g, NL * 2 * C, cond_sz,
      [&](int n, int ci, int) {
        int layer = n / (2 * C), o = perm[n % (2 * C)];
        return cpw[layer][(int64_t)o * cond_sz + ci];
      },
      [&](int n) {
        int layer = n / (2 * C), o = perm[n % (2 * C)];
        return cpb[layer][o];
      });
}

// ---------------------------------------------------------------------------- finalize: whisper
int build_whisper(svc_ctx* c) {
  GETP(c1w, "whisper.encoder.conv1.weight", -1, -1, 3);
  const int D = (int)c1w->shape[0];
  const int nm = (int)c1w->shape[1];
  GETP(pos, "whisper.encoder.positional_embedding", -1, D);
  c->wD = D;
  c->wH = D / 64;
  c->wmels = nm;
  c->wctx = (int)pos->shape[0];
  int L = 0;
  while (c->params.count("whisper.encoder.blocks." + std::to_string(L) + ".attn.query.weight")) ++L;
  c->wL = L;
  GETP(c1b, "whisper.encoder.conv1.bias", D);
  GETP(c2w, "whisper.encoder.conv2.weight", D, D, 3);
  GETP(c2b, "whisper.encoder.conv2.bias", D);
  // precision: the conv stem is split-fp16 in both split modes; the blocks' linears follow content_mode
  const int mode = c->content_mode;
  const bool sp = mode != 0;
  SVC_REQUIRE(!sp || nm % 8 == 0, "whisper split precision: n_mels %d", nm);
  // the split stem's operand rows [hi | lo | hi] (3 n_mels = 240 wide) are stored 256 wide with a zero pad, and each
  // tap's K segment padded to match, so a K-tile of 64 lies in one tap (the K-loop's buffer-descriptor form):
  // 768 instead of 720-deep K, but no per-lane tap arithmetic
  int st;
  if (sp) {
    c->wstem_ld = (int)round_up(3 * nm, 64);
    st = pack_gemm_split3(
        c, c->wconv1, D, nm, [&](int n, int ci, int t) { return c1w->host[((int64_t)n * nm + ci) * 3 + t]; },
        [&](int n) { return c1b->host[n]; }, 3, c->wstem_ld);
    c->wconv1.tap_mul = 1;
    c->wconv1.tap_add = -1;
    c->wconv1.istride = 1;
  } else {
    c->wstem_ld = (int)round_up(nm, 8);
    st = pack_conv1d(c, c->wconv1, c1w->host, c1b->host, D, nm, 3, c->wstem_ld, 1, 1, 1);
  }
  if (st) return st;
  st = pack_conv1d_opt(c, c->wconv2, c2w->host, c2b->host, D, D, 3, D, 1, 1, 2, sp);
  if (st) return st;
  if ((st = upload_param(c, pos, &c->wpos))) return st;
  c->wblocks.resize(L);
  // default: the attention linears of every block and the MLP linears of blocks 0-3 (tools/precision_sweep.py, three
  // clips: de-normalised mel-L1 0.76-0.78e-3 against 0.72-0.74e-3 with every linear split and 0.84-0.86e-3 with the
  // attention linears only; the error enters early and through the attention; DESIGN.md "precision")
  const uint64_t wsplit_attn = (uint64_t)cfgv(c, "content.wsplit_attn", 9007199254740991.0);  // 2^53 - 1: all blocks
  const uint64_t wsplit_mlp = (uint64_t)cfgv(c, "content.wsplit_mlp", 15.0);
  // finer masks for the attention linears (default: wsplit_attn for each): q / k, v, out
  const uint64_t wsplit_qk = (uint64_t)cfgv(c, "content.wsplit_qk", (double)wsplit_attn);
  const uint64_t wsplit_v = (uint64_t)cfgv(c, "content.wsplit_v", (double)wsplit_attn);
  const uint64_t wsplit_out = (uint64_t)cfgv(c, "content.wsplit_out", (double)wsplit_attn);
  for (int i = 0; i < L; ++i) {
    std::string p = "whisper.encoder.blocks." + std::to_string(i) + ".";
    WBlock& b = c->wblocks[i];
    GETP(qw, p + "attn.query.weight", D, D);
    GETP(qb, p + "attn.query.bias", D);
    GETP(kw, p + "attn.key.weight", D, D);
    GETP(vw, p + "attn.value.weight", D, D);
    GETP(vb, p + "attn.value.bias", D);
    GETP(ow, p + "attn.out.weight", D, D);
    GETP(ob, p + "attn.out.bias", D);
    GETP(l1g, p + "attn_ln.weight", D);
    GETP(l1b, p + "attn_ln.bias", D);
    GETP(l2g, p + "mlp_ln.weight", D);
    GETP(l2b, p + "mlp_ln.bias", D);
    GETP(f1w, p + "mlp.0.weight", 4 * D, D);
    GETP(f1b, p + "mlp.0.bias", 4 * D);
    GETP(f2w, p + "mlp.2.weight", D, 4 * D);
    GETP(f2b, p + "mlp.2.bias", D);
    auto qkv_w = [&](int n, int ci, int) {
      const Param* w = n < D ? qw : (n < 2 * D ? kw : vw);
      return w->host[(int64_t)(n % D) * D + ci];
    };
    auto qkv_b = [&](int n) { return n < D ? qb->host[n] : (n < 2 * D ? 0.0f : vb->host[n - 2 * D]); };
    auto lin = [&](const Param* w) { return [w](int n, int ci, int) { return w->host[(int64_t)n * (w->shape[1]) + ci]; }; };
    auto bias = [&](const Param* b0) { return [b0](int n) { return b0->host[n]; }; };
    // weight-split mode: "content.wsplit_attn" / "content.wsplit_mlp" (bit i: block i) choose the blocks whose
    // attention linears (qkv, out) / MLP linears (fc1, fc2) get [W_hi; W_lo]; the others run on plain fp16 weights.
    // "content.wsplit_qk" / "content.wsplit_v" / "content.wsplit_out" refine the attention mask per linear (bits 1 /
    // 16 / 2 of lmode); fc1 / fc2 are bits 4 / 8
    auto lmode = [&](int bit) {
      if (mode != 2) return mode;
      const uint64_t m = bit == 1 ? wsplit_qk : bit == 2 ? wsplit_out : bit == 16 ? wsplit_v : wsplit_mlp;
      return ((m >> (i < 53 ? i : 52)) & 1) ? 2 : 0;
    };
    b.split_v = lmode(1) != lmode(16);
    if (!b.split_v) {
      if ((st = pack_linear_mode(c, b.qkv, 3 * D, D, lmode(1), qkv_w, qkv_b))) return st;
    } else {  // q | k on one GEMM, v on another, each with its own operand precision
      if ((st = pack_linear_mode(c, b.qkv, 2 * D, D, lmode(1), qkv_w, qkv_b))) return st;
      if ((st = pack_linear_mode(c, b.v, D, D, lmode(16), lin(vw), bias(vb)))) return st;
    }
    // the attention output (A of `out`) is fp16 (the attention kernel's P.V path is fp16 either way): split3 would
    // only split the weights, which the weight-split mode does at 2x
    if ((st = pack_linear_mode(c, b.out, D, D, mode == 2 ? lmode(2) : 0, lin(ow), bias(ob)))) return st;
    if ((st = pack_linear_mode(c, b.fc1, 4 * D, D, lmode(4), lin(f1w), bias(f1b)))) return st;
    if ((st = pack_linear_mode(c, b.fc2, D, 4 * D, lmode(8), lin(f2w), bias(f2b)))) return st;
    if ((st = upload_param(c, l1g, &b.ln1_g)) || (st = upload_param(c, l1b, &b.ln1_b)) ||
        (st = upload_param(c, l2g, &b.ln2_g)) || (st = upload_param(c, l2b, &b.ln2_b)))
      return st;
  }
  GETP(lpg, "whisper.encoder.ln_post.weight", D);
  GETP(lpb, "whisper.encoder.ln_post.bias", D);
  if ((st = upload_param(c, lpg, &c->wlnp_g)) || (st = upload_param(c, lpb, &c->wlnp_b))) return st;
  c->has_whisper = true;
  return SVC_OK;
}

// ---------------------------------------------------------------------------- finalize: hubert (A8)
// fairseq HubertModel (ContentVec) as utils/hubert.py:14-47 drives it; parameter names are fairseq's.
int build_hubert(svc_ctx* c) {
  GETP(c0, "hubert.feature_extractor.conv_layers.0.0.weight", -1, 1, 10);
  const int Cc = (int)c0->shape[0];
  GETP(pw, "hubert.post_extract_proj.weight", -1, Cc);
  const int D = (int)pw->shape[0];
  SVC_REQUIRE(D % 64 == 0 && D <= 1024 && Cc % 64 == 0 && Cc <= 1024, "hubert: embed %d / conv dim %d", D, Cc);
  c->hC = Cc;
  c->hD = D;
  c->hH = D / 64;
  int L = 0;
  while (c->params.count("hubert.encoder.layers." + std::to_string(L) + ".fc1.weight")) ++L;
  const int want = (int)cfgv(c, "hubert.output_layer", 9);
  SVC_REQUIRE(want >= 1 && L >= 1, "hubert: output_layer %d, %d layers", want, L);
  c->hLayers = std::min(want, L);  // fairseq's TransformerEncoder runs every layer when output_layer exceeds them
  int st;
  // conv_layers[0]: W0[n][0][tap*5 + j] -> packed K index tap*8 + j over rows of 5 samples
  c->hconv.assign(7, PackedGemm());
  c->hconv_k = {10, 3, 3, 3, 3, 2, 2};
  c->hconv_s = {5, 2, 2, 2, 2, 2, 2};
  const bool sp = c->content_mode != 0;  // HuBERT: split-fp16 in both split modes
  if (sp)  // split-fp16 frames rows [hi(5) | lo(5) | hi(5) | 0] against [W_hi | W_hi | W_lo | 0] per tap
    st = pack_gemm(
        c, c->hconv[0], Cc, 16, 16, 2,
        [&](int n, int ci, int t) {
          if (ci >= 15) return 0.0f;
          const int seg = ci / 5;
          const float w = c0->host[(int64_t)n * 10 + t * 5 + (ci - seg * 5)];
          const float hi = round16_host(w, c->pack_bf16);
          return seg < 2 ? hi : w - hi;
        },
        [&](int) { return 0.0f; });
  else
    st = pack_gemm(
        c, c->hconv[0], Cc, 5, 8, 2, [&](int n, int ci, int t) { return c0->host[(int64_t)n * 10 + t * 5 + ci]; },
        [&](int) { return 0.0f; });
  if (st) return st;
  c->hconv[0].tap_mul = 1;
  c->hconv[0].tap_add = 0;
  c->hconv[0].istride = 1;
  for (int i = 1; i < 7; ++i) {
    GETP(w, "hubert.feature_extractor.conv_layers." + std::to_string(i) + ".0.weight", Cc, Cc, c->hconv_k[i]);
    if ((st = pack_conv1d_opt(c, c->hconv[i], w->host, nullptr, Cc, Cc, c->hconv_k[i], Cc, 1, 0, 2, sp))) return st;
  }
  GETP(gng, "hubert.feature_extractor.conv_layers.0.2.weight", Cc);
  GETP(gnb, "hubert.feature_extractor.conv_layers.0.2.bias", Cc);
  GETP(lng, "hubert.layer_norm.weight", Cc);
  GETP(lnb, "hubert.layer_norm.bias", Cc);
  GETP(pb, "hubert.post_extract_proj.bias", D);
  if ((st = upload_param(c, gng, &c->hgn_g)) || (st = upload_param(c, gnb, &c->hgn_b)) ||
      (st = upload_param(c, lng, &c->hln_g)) || (st = upload_param(c, lnb, &c->hln_b)))
    return st;
  if ((st = pack_conv1d_opt(c, c->hproj, pw->host, pb->host, D, Cc, 1, Cc, 1, 0, 1, sp))) return st;
  // pos_conv: weight_norm(dim=2) -> w[o][i][k] = g[k] * v[o][i][k] / ||v[:, :, k]||; one GEMM per group
  GETP(pv, "hubert.encoder.pos_conv.0.weight_v", D, -1, -1);
  const int Cg = (int)pv->shape[1], kp = (int)pv->shape[2];
  GETP(pg, "hubert.encoder.pos_conv.0.weight_g", 1, 1, kp);
  GETP(pcb, "hubert.encoder.pos_conv.0.bias", D);
  SVC_REQUIRE(D % Cg == 0 && Cg % 8 == 0 && kp % 2 == 0, "hubert: pos_conv groups of %d, k=%d", Cg, kp);
  c->hPosK = kp;
  c->hPosG = D / Cg;
  std::vector<double> kscale(kp);
  for (int k = 0; k < kp; ++k) {
    double acc = 0;
    for (int64_t oi = 0; oi < (int64_t)D * Cg; ++oi) {
      const double v = pv->host[oi * kp + k];
      acc += v * v;
    }
    kscale[k] = (double)pg->host[k] / sqrt(acc);
  }
  c->hpos.assign(c->hPosG, PackedGemm());
  for (int gi = 0; gi < c->hPosG; ++gi) {
    auto pw_ = [&](int n, int ci, int t) {
      return (float)((double)pv->host[((int64_t)(gi * Cg + n) * Cg + ci) * kp + t] * kscale[t]);
    };
    auto pb_ = [&](int n) { return pcb->host[gi * Cg + n]; };
    st = sp ? pack_gemm_split3(c, c->hpos[gi], Cg, Cg, pw_, pb_, kp) : pack_gemm(c, c->hpos[gi], Cg, Cg, Cg, kp, pw_, pb_);
    if (st) return st;
    c->hpos[gi].tap_mul = 1;
    c->hpos[gi].tap_add = -kp / 2;  // padding k/2, SamePad drops the extra last frame
    c->hpos[gi].istride = 1;
  }
  GETP(elg, "hubert.encoder.layer_norm.weight", D);
  GETP(elb, "hubert.encoder.layer_norm.bias", D);
  if ((st = upload_param(c, elg, &c->henc_ln_g)) || (st = upload_param(c, elb, &c->henc_ln_b))) return st;
  c->hblocks.resize(c->hLayers);
  for (int i = 0; i < c->hLayers; ++i) {
    const std::string p = "hubert.encoder.layers." + std::to_string(i) + ".";
    HBlock& b = c->hblocks[i];
    GETP(qw, p + "self_attn.q_proj.weight", D, D);
    GETP(qb, p + "self_attn.q_proj.bias", D);
    GETP(kw, p + "self_attn.k_proj.weight", D, D);
    GETP(kb, p + "self_attn.k_proj.bias", D);
    GETP(vw, p + "self_attn.v_proj.weight", D, D);
    GETP(vb, p + "self_attn.v_proj.bias", D);
    GETP(ow, p + "self_attn.out_proj.weight", D, D);
    GETP(ob, p + "self_attn.out_proj.bias", D);
    GETP(l1g, p + "self_attn_layer_norm.weight", D);
    GETP(l1b, p + "self_attn_layer_norm.bias", D);
    GETP(l2g, p + "final_layer_norm.weight", D);
    GETP(l2b, p + "final_layer_norm.bias", D);
    GETP(f1w, p + "fc1.weight", -1, D);
    const int Fd = (int)f1w->shape[0];
    GETP(f1b, p + "fc1.bias", Fd);
    GETP(f2w, p + "fc2.weight", D, Fd);
    GETP(f2b, p + "fc2.bias", D);
    auto qkv_w = [&](int n, int ci, int) {
      const Param* w = n < D ? qw : (n < 2 * D ? kw : vw);
      return w->host[(int64_t)(n % D) * D + ci];
    };
    auto qkv_b = [&](int n) { return n < D ? qb->host[n] : (n < 2 * D ? kb->host[n - D] : vb->host[n - 2 * D]); };
    st = sp ? pack_gemm_split3(c, b.qkv, 3 * D, D, qkv_w, qkv_b) : pack_gemm(c, b.qkv, 3 * D, D, D, 1, qkv_w, qkv_b);
    if (st) return st;
    if ((st = pack_conv1d(c, b.out, ow->host, ob->host, D, D, 1, D, 1, 0, 1))) return st;  // A = attention output (fp16)
    SVC_REQUIRE(Fd % 8 == 0, "hubert: ffn width %d", Fd);
    if ((st = pack_conv1d_opt(c, b.fc1, f1w->host, f1b->host, Fd, D, 1, D, 1, 0, 1, sp))) return st;
    if ((st = pack_conv1d_opt(c, b.fc2, f2w->host, f2b->host, D, Fd, 1, Fd, 1, 0, 1, sp))) return st;
    if ((st = upload_param(c, l1g, &b.ln1_g)) || (st = upload_param(c, l1b, &b.ln1_b)) ||
        (st = upload_param(c, l2g, &b.ln2_g)) || (st = upload_param(c, l2b, &b.ln2_b)))
      return st;
  }
  GETP(fw, "hubert.final_proj.weight", -1, D);
  c->hFinal = (int)fw->shape[0];
  GETP(fb, "hubert.final_proj.bias", c->hFinal);
  if ((st = pack_conv1d_opt(c, c->hfinal, fw->host, fb->host, c->hFinal, D, 1, D, 1, 0, 1, sp))) return st;
  c->has_hubert = true;
  return SVC_OK;
}

// ---------------------------------------------------------------------------- finalize: mapper
int build_mapper(svc_ctx* c) {
  const int C = (int)cfgv(c, "mapper.residual_channels", 384);
  const int NL = (int)cfgv(c, "mapper.residual_layer_num", 20);
  const int nmel = (int)cfgv(c, "mapper.n_mel", 100);
  const int fc = (int)cfgv(c, "mapper.diffusion_fc_size", 128);
  c->C = C;
  c->n_layers = NL;
  c->n_mel = nmel;
  c->dil_cycle = (int)cfgv(c, "mapper.dilation_cycle_length", 4);
  const int ks = (int)cfgv(c, "mapper.residual_kernel_size", 3);
  if (ks != 3) {
    set_error("mapper: residual_kernel_size %d unsupported", ks);
    return SVC_ERR_INVALID;
  }
  const std::string p = "mapper.0.registered_modules_dict.";
  // One ContentEncoder Linear per content type (modules/encoder.py:144-148), summed with the other encoders:
  // packed as ONE GEMM over the content types' features concatenated along K in ascending name order
  // (the order of this map), with the biases summed.
  std::vector<const Param*> cws, cbs;
  {
    const std::string pre = p + "content_", suf = ".nn.weight";
    for (auto& kv : c->params) {
      const std::string& k = kv.first;
      if (k.rfind(pre, 0) == 0 && k.size() > pre.size() + suf.size() && k.compare(k.size() - suf.size(), suf.size(), suf) == 0) {
        const std::string ct = k.substr(pre.size(), k.size() - pre.size() - suf.size());
        GETP(w_, k, C, -1);
        GETP(b_, p + "content_" + ct + ".nn.bias", C);
        SVC_REQUIRE(w_->shape[1] % 8 == 0, "mapper: content_%s width %lld not a multiple of 8", ct.c_str(),
                    (long long)w_->shape[1]);
        cws.push_back(w_);
        cbs.push_back(b_);
      }
    }
  }
  SVC_REQUIRE(!cws.empty(), "missing parameter 'mapper.0.registered_modules_dict.content_<type>.nn.weight'");
  c->content_dim = 0;
  for (auto* w_ : cws) c->content_dim += (int)w_->shape[1];
  GETP(mb, p + "melody.melody_bins", -1);
  GETP(me, p + "melody.nn.weight", -1, C);
  GETP(eb, p + "loudness.energy_bins", mb->shape[0]);
  GETP(le, p + "loudness.nn.weight", me->shape[0], C);
  GETP(se, p + "singer.nn.weight", -1, C);
  c->n_bins = (int)me->shape[0];
  if (mb->shape[0] != c->n_bins - 1) {
    set_error("mapper: melody bins %lld vs embedding %d", (long long)mb->shape[0], c->n_bins);
    return SVC_ERR_INVALID;
  }
  int st;
  st = pack_gemm(
      c, c->content_lin, C, c->content_dim, c->content_dim, 1,
      [&](int n, int ci, int) {
        for (auto* w_ : cws) {
          const int d = (int)w_->shape[1];
          if (ci < d) return w_->host[(int64_t)n * d + ci];
          ci -= d;
        }
        return 0.0f;
      },
      [&](int n) {
        float b = 0.0f;
        for (auto* b_ : cbs) b += b_->host[n];
        return b;
      });
  if (st) return st;
  if ((st = upload_param(c, mb, &c->mbins)) || (st = upload_param(c, eb, &c->ebins)) ||
      (st = upload_param(c, me, &c->emb_m)) || (st = upload_param(c, le, &c->emb_l)) ||
      (st = upload_param(c, se, &c->emb_s)))
    return st;

  const std::string q = "mapper.1.";
  GETP(mpw, q + "mel_preprocess.projection.weight", C, nmel, 1);
  GETP(mpb, q + "mel_preprocess.projection.bias", C);
  if ((st = pack_conv1d(c, c->melpre, mpw->host, mpb->host, C, nmel, 1, (int)round_up(nmel, 8), 1, 0, 1))) return st;
  if (C == 384 && c->melpre.Kpad == 128 && c->melpre.K <= 128) {  // mel_proj's shape: W_mel in its fragment order
    void* wf = nullptr;
    SVC_HIP_CHECK(hipMalloc(&wf, mel_proj_pack_elems() * sizeof(f16)));
    c->allocs.push_back(wf);
    c->weight_bytes += (int64_t)(mel_proj_pack_elems() * sizeof(f16));
    c->melpre.Wfrag = reinterpret_cast<f16*>(wf);
    if ((st = mel_proj_pack(c->melpre.W, c->melpre.Kpad, c->melpre.Wfrag, 0))) return st;
    SVC_HIP_CHECK(hipStreamSynchronize(0));
  }
  GETP(p1w, q + "diffusion_embedding.projection1.weight", fc, 128);
  GETP(p1b, q + "diffusion_embedding.projection1.bias", fc);
  GETP(p2w, q + "diffusion_embedding.projection2.weight", fc, fc);
  GETP(p2b, q + "diffusion_embedding.projection2.bias", fc);
  GETP(table, "mapper.step_table", -1, 128);
  const int steps = (int)table->shape[0];
  c->steps = steps;
  std::vector<int> perm = pair_perm(C);
  c->dil.resize(NL);
  c->outres.resize(NL);
  std::vector<const Param*> opw_l(NL), opb_l(NL);
  std::vector<const Param*> cpw(NL), cpb(NL), dpw(NL), dpb(NL);
  for (int i = 0; i < NL; ++i) {
    std::string r = q + "residual_layers." + std::to_string(i) + ".";
    GETP(dw, r + "dilated_conv.weight", 2 * C, C, 3);
    GETP(db, r + "dilated_conv.bias", 2 * C);
    GETP(ow, r + "output_projection.weight", 2 * C, C, 1);
    GETP(ob, r + "output_projection.bias", 2 * C);
    GETP(cw2, r + "conditioner_projection.weight", 2 * C, -1, 1);
    GETP(cb2, r + "conditioner_projection.bias", 2 * C);
    GETP(pw, r + "diffusion_projection.weight", C, fc);
    GETP(pb, r + "diffusion_projection.bias", C);
    cpw[i] = cw2;
    cpb[i] = cb2;
    dpw[i] = pw;
    dpb[i] = pb;
    const int d = 1 << (i % c->dil_cycle);
    if ((st = pack_conv1d(c, c->dil[i], dw->host, db->host, 2 * C, C, 3, C, d, d, 1, &perm))) return st;
    if (C == 384 && c->dil[i].Kpad == 3 * C) {  // gate_ws's shape: its weights once more, in its fragment order
      void* wf = nullptr;
      SVC_HIP_CHECK(hipMalloc(&wf, gate_ws_pack_elems() * sizeof(f16)));
      c->allocs.push_back(wf);
      c->weight_bytes += (int64_t)(gate_ws_pack_elems() * sizeof(f16));
      c->dil[i].Wfrag = reinterpret_cast<f16*>(wf);
      if ((st = gate_ws_pack(c->dil[i].W, c->dil[i].Kpad, c->dil[i].Wfrag, 0))) return st;
      SVC_HIP_CHECK(hipStreamSynchronize(0));
    }
    // rows 0..C-1 of output_projection are the residual, C..2C-1 the skip (modules/diffsvc.py:229-231)
    if ((st = pack_conv1d(c, c->outres[i], ow->host, ob->host, C, C, 1, C, 1, 0, 1))) return st;
    if (C == 384) {  // res_proj's shape: its weights once more, in MFMA fragment order
      void* wf = nullptr;
      SVC_HIP_CHECK(hipMalloc(&wf, res_proj_pack_elems() * sizeof(f16)));
      c->allocs.push_back(wf);
      c->weight_bytes += (int64_t)(res_proj_pack_elems() * sizeof(f16));
      c->outres[i].Wfrag = reinterpret_cast<f16*>(wf);
      if ((st = res_proj_pack(c->outres[i].W, c->outres[i].Kpad, c->outres[i].Wfrag, 0))) return st;
      SVC_HIP_CHECK(hipStreamSynchronize(0));
    }
    opw_l[i] = ow;
    opb_l[i] = ob;
  }
  // sum over layers of skip_i = g_i @ Wskip_i + bskip_i is ONE GEMM over the concatenated gate outputs (pack_skip_all)
  std::vector<const float*> ow_h(NL), ob_h(NL), cpw_h(NL), cpb_h(NL);
  for (int i = 0; i < NL; ++i) {
    ow_h[i] = opw_l[i]->host + (size_t)C * C;
    ob_h[i] = opb_l[i]->host + C;
    cpw_h[i] = cpw[i]->host;
    cpb_h[i] = cpb[i]->host;
  }
  if ((st = pack_skip_all(c, c->skip_all, ow_h.data(), ob_h.data(), C, NL))) return st;
  const int cond_sz = (int)cpw[0]->shape[1];
  // all 20 conditioner projections as one GEMM (loop-invariant over diffusion steps: hoisted), in split-fp16
  // precision: it runs once per batch, and its rounding is the largest single denoiser-side term of the
  // mel-L1 error (precision sweep)
  if ((st = pack_cond_all(c, c->cp_all, cpw_h.data(), cpb_h.data(), C, NL, cond_sz))) return st;
  GETP(spw, q + "skip_projection.weight", C, C, 1);
  GETP(spb, q + "skip_projection.bias", C);
  GETP(opw, q + "output_projection.weight", nmel, C, 1);
  GETP(opb, q + "output_projection.bias", nmel);
  // The head (skip_projection + output_projection, modules/diffsvc.py:315-319) on split-fp16 operands by default
  // ("mapper.head_split"): its rounding feeds eps directly and is, after the conditioner projection, the largest
  // denoiser-side term of the mel-L1 error (precision); 3x the MFMA work of two small K = 384 GEMMs.
  c->head_split = cfgv(c, "mapper.head_split", 1) != 0;
  if ((st = pack_conv1d_opt(c, c->skipproj, spw->host, spb->host, C, C, 1, C, 1, 0, 1, c->head_split))) return st;
  if ((st = pack_conv1d_opt(c, c->outproj, opw->host, opb->host, nmel, C, 1, C, 1, 0, 1, c->head_split))) return st;

  // step MLP + per-layer diffusion projections for every step (input-independent: precomputed)
  std::vector<float> dp((size_t)steps * NL * C);
  std::vector<double> h1(fc), h2(fc);
  auto silu = [](double x) { return x / (1.0 + exp(-x)); };
  for (int t = 0; t < steps; ++t) {
    const float* e = table->host + (size_t)t * 128;
    for (int o = 0; o < fc; ++o) {
      double a = p1b->host[o];
      for (int i = 0; i < 128; ++i) a += (double)p1w->host[o * 128 + i] * e[i];
      h1[o] = (float)silu((float)a);
    }
    for (int o = 0; o < fc; ++o) {
      double a = p2b->host[o];
      for (int i = 0; i < fc; ++i) a += (double)p2w->host[o * fc + i] * h1[i];
      h2[o] = (float)silu((float)a);
    }
    for (int l = 0; l < NL; ++l)
      for (int o = 0; o < C; ++o) {
        double a = dpb[l]->host[o];
        for (int i = 0; i < fc; ++i) a += (double)dpw[l]->host[o * fc + i] * h2[i];
        dp[((size_t)t * NL + l) * C + o] = (float)a;
      }
  }
  if ((st = upload_vec(c, dp, &c->dproj))) return st;

  // noise schedule constants (modules/diffsvcrepo_inference.py:163-197: numpy f64 -> f32)
  const double b0 = cfgv(c, "mapper.noise_schedule_factors.0", 1e-4);
  const double b1 = cfgv(c, "mapper.noise_schedule_factors.1", 0.02);
  std::vector<double> betas(steps);
  const double stp = (b1 - b0) / (steps - 1);
  for (int i = 0; i < steps; ++i) betas[i] = (i == steps - 1) ? b1 : i * stp + b0;
  c->alphas_cumprod_f32.resize(steps);
  c->sra.resize(steps);
  c->srm1.resize(steps);
  c->pc1.resize(steps);
  c->pc2.resize(steps);
  c->plogvar.resize(steps);
  double ac = 1.0;
  for (int i = 0; i < steps; ++i) {
    const double alpha = 1.0 - betas[i];
    const double prev = ac;
    ac = ac * alpha;
    c->alphas_cumprod_f32[i] = (float)ac;
    c->sra[i] = (float)sqrt(1.0 / ac);
    c->srm1[i] = (float)sqrt(1.0 / ac - 1);
    c->pc1[i] = (float)(betas[i] * sqrt(prev) / (1.0 - ac));
    c->pc2[i] = (float)((1.0 - prev) * sqrt(alpha) / (1.0 - ac));
    const double pv = betas[i] * (1.0 - prev) / (1.0 - ac);
    c->plogvar[i] = (float)log(pv > 1e-20 ? pv : 1e-20);
  }
  if ((st = build_stats(c))) return st;
  c->has_mapper = true;
  return SVC_OK;
}

// the per-channel mel statistics: the de-normaliser in front of the vocoder and the normaliser (svc_mel_normalize,
// shallow diffusion) read them. A context without a mapper may carry them alone (copy-synthesis through the vocoder).
int build_stats(svc_ctx* c) {
  const int nmel = c->n_mel = (int)cfgv(c, "mapper.n_mel", 100);
  GETP(mn, "stats.mel_min", nmel);
  GETP(mx, "stats.mel_max", nmel);
  int st;
  if ((st = upload_param(c, mn, &c->mel_min)) || (st = upload_param(c, mx, &c->mel_max))) return st;
  return SVC_OK;
}

// ---------------------------------------------------------------------------- finalize: vocoder
// Activation1d parameters (modules/bigvgan.py:234-307). The kernels take log-scale SnakeBeta parameters: the
// magnitude term is 1 / (exp(beta) + 1e-9) and the frequency exp(alpha). Snake (:42-92) is SnakeBeta with beta = alpha;
// linear-scale parameters (snake_logscale = false) are passed as their logarithms, which needs them positive.
static int get_act(svc_ctx* c, const std::string& name, int ch, ActP& a) {
  const bool snake = cfgv(c, "vocoder.snake", 0) != 0;
  const bool logscale = cfgv(c, "vocoder.snake_logscale", 1) != 0;
  GETP(al, name + ".act.alpha", ch);
  const Param* be = al;
  if (!snake) {
    GETP(b, name + ".act.beta", ch);
    be = b;
  }
  GETP(fu, name + ".upsample.filter", 1, 1, 12);
  GETP(fd, name + ".downsample.lowpass.filter", 1, 1, 12);
  for (int i = 0; i < 12; ++i)
    if (fu->host[i] != fd->host[i]) {
      set_error("%s: up/down filters differ (unsupported)", name.c_str());
      return SVC_ERR_INVALID;
    }
  std::vector<float> av(al->host, al->host + ch), bv(be->host, be->host + ch);
  if (!logscale) {
    for (int i = 0; i < ch; ++i) {
      if (!(av[i] > 0.f) || !(bv[i] > 0.f)) {
        set_error("%s: snake_logscale=false needs positive alpha/beta (channel %d: %g, %g)", name.c_str(), i, av[i],
                  bv[i]);
        return SVC_ERR_INVALID;
      }
      av[i] = logf(av[i]);
      bv[i] = logf(bv[i]);
    }
  }
  int st;
  if ((st = upload_vec(c, av, &a.alpha)) || (st = upload_vec(c, bv, &a.beta)) || (st = upload_param(c, fu, &a.filt)))
    return st;
  return SVC_OK;
}

int build_vocoder(svc_ctx* c) {
  const int ns = (int)cfgv(c, "vocoder.n_stages", 6);
  const int nk = (int)cfgv(c, "vocoder.n_kernels", 3);
  const int C0 = (int)cfgv(c, "vocoder.upsample_initial_channel", 1536);
  const int vin = (int)cfgv(c, "vocoder.input_dim", 100);
  c->v_c0 = C0;
  c->v_in = vin;
  c->v_rb2 = cfgv(c, "vocoder.resblock", 1) == 2;
  int st;
  GETP(pv, "vocoder.conv_pre.weight_v", C0, vin, 7);
  GETP(pg, "vocoder.conv_pre.weight_g", C0, 1, 1);
  GETP(pb, "vocoder.conv_pre.bias", C0);
  if ((st = pack_conv1d(c, c->vpre, pv->host, pb->host, C0, vin, 7, (int)round_up(vin, 8), 1, 3, 1, nullptr, pg->host)))
    return st;
  c->vstages.resize(ns);
  int hop = 1;
  for (int i = 0; i < ns; ++i) {
    VStage& S = c->vstages[i];
    S.cin = C0 >> i;
    S.cout = C0 >> (i + 1);
    S.rate = (int)cfgv(c, ("vocoder.upsample_rates." + std::to_string(i)).c_str(), 2);
    S.k = (int)cfgv(c, ("vocoder.upsample_kernel_sizes." + std::to_string(i)).c_str(), 4);
    hop *= S.rate;
    std::string u = "vocoder.ups." + std::to_string(i) + ".0.";
    GETP(uv, u + "weight_v", S.cin, S.cout, S.k);
    GETP(ug, u + "weight_g", S.cin, 1, 1);
    GETP(ub, u + "bias", S.cout);
    if ((st = pack_conv_transpose(c, S.phases, uv->host, ug->host, ub->host, S.cin, S.cout, S.k, S.rate,
                                  (S.k - S.rate) / 2)))
      return st;
    if ((st = pack_conv_transpose_comb(c, S, uv->host, ug->host, ub->host))) return st;
    S.c1.resize(nk);
    S.c2.resize(nk);
    S.acts.resize(nk);
    S.rk.resize(nk);
    S.rd.resize(nk);
    const int ch = S.cout;
    for (int j = 0; j < nk; ++j) {
      const int kk = (int)cfgv(c, ("vocoder.resblock_kernel_sizes." + std::to_string(j)).c_str(), 3);
      S.rk[j] = kk;
      std::string rb = "vocoder.resblocks." + std::to_string(i * nk + j) + ".";
      const int nd = (int)cfgv(c, ("vocoder.resblock_dilation_sizes." + std::to_string(j) + ".n").c_str(), 3);
      S.c1[j].resize(nd);
      S.c2[j].resize(nd);
      S.acts[j].resize(2 * nd);
      S.rd[j].resize(nd);
      for (int l = 0; l < nd; ++l) {
        const int d =
            (int)cfgv(c, ("vocoder.resblock_dilation_sizes." + std::to_string(j) + "." + std::to_string(l)).c_str(), 1);
        S.rd[j][l] = d;
        if (c->v_rb2) {  // AMPBlock2 (modules/bigvgan.py:442-512): x = x + convs[l](activations[l](x)), dilation d
          std::string n = rb + "convs." + std::to_string(l) + ".";
          GETP(v, n + "weight_v", ch, ch, kk);
          GETP(g, n + "weight_g", ch, 1, 1);
          GETP(bb, n + "bias", ch);
          if ((st = pack_conv1d(c, S.c2[j][l], v->host, bb->host, ch, ch, kk, ch, d, (kk * d - d) / 2, 1, nullptr,
                                g->host)))
            return st;
          if ((st = get_act(c, rb + "activations." + std::to_string(l), ch, S.acts[j][2 * l + 1]))) return st;
          continue;
        }
        std::string n1 = rb + "convs1." + std::to_string(l) + ".", n2 = rb + "convs2." + std::to_string(l) + ".";
        GETP(v1, n1 + "weight_v", ch, ch, kk);
        GETP(g1, n1 + "weight_g", ch, 1, 1);
        GETP(b1, n1 + "bias", ch);
        GETP(v2, n2 + "weight_v", ch, ch, kk);
        GETP(g2, n2 + "weight_g", ch, 1, 1);
        GETP(b2, n2 + "bias", ch);
        if ((st = pack_conv1d(c, S.c1[j][l], v1->host, b1->host, ch, ch, kk, ch, d, (kk * d - d) / 2, 1, nullptr,
                              g1->host)))
          return st;
        if ((st = pack_conv1d(c, S.c2[j][l], v2->host, b2->host, ch, ch, kk, ch, 1, (kk - 1) / 2, 1, nullptr,
                              g2->host)))
          return st;
        if ((st = get_act(c, rb + "activations." + std::to_string(2 * l), ch, S.acts[j][2 * l]))) return st;
        if ((st = get_act(c, rb + "activations." + std::to_string(2 * l + 1), ch, S.acts[j][2 * l + 1]))) return st;
      }
    }
  }
  c->hop_out = hop;
  const int chl = C0 >> ns;
  if ((st = get_act(c, "vocoder.activation_post", chl, c->vact_post))) return st;
  GETP(qv, "vocoder.conv_post.weight_v", 1, chl, 7);
  GETP(qg, "vocoder.conv_post.weight_g", 1, 1, 1);
  GETP(qb, "vocoder.conv_post.bias", 1);
  {
    double s = 0;
    for (int i = 0; i < chl * 7; ++i) s += (double)qv->host[i] * qv->host[i];
    const double sc = qg->host[0] / sqrt(s);
    std::vector<float> w(chl * 7);
    for (int i = 0; i < chl * 7; ++i) w[i] = (float)(qv->host[i] * sc);
    if ((st = upload_vec(c, w, &c->vpost_w))) return st;
    c->vpost_b = qb->host[0];
  }
  GETP(fade, "vocoder.fade_out", -1);
  c->nfade = (int)fade->shape[0];
  if ((st = upload_param(c, fade, &c->fade))) return st;
  c->has_vocoder = true;
  return SVC_OK;
}

int build_features(svc_ctx* c) {
  c->fs = (int)cfgv(c, "fs", 24000);
  c->n_fft = (int)cfgv(c, "n_fft", 1024);
  c->hop = (int)cfgv(c, "hop_length", 256);
  c->n_mels = (int)cfgv(c, "n_mels", 100);
  c->fmin = cfgv(c, "fmin", 0);
  c->fmax = cfgv(c, "fmax", 12000);
  c->f0_min = cfgv(c, "f0_min", 65);
  c->f0_max = cfgv(c, "f0_max", 800);
  if ((int)cfgv(c, "win_length", 1024) != c->n_fft || !dft_mel_supported(c->n_fft)) {
    set_error("n_fft %d / win_length unsupported (n_fft 512, 1024 or 2048 and win_length == n_fft)", c->n_fft);
    return SVC_ERR_INVALID;
  }
  int st;
  const std::vector<float> fb24 = slaney_mel(c->fs, c->n_fft, c->n_mels, c->fmin, c->fmax);
  const std::vector<float> fb16 = slaney_mel(16000, 400, 80, 0.0, 8000.0);
  const FilterBands b24 = filter_bands(fb24, c->n_mels), b16 = filter_bands(fb16, 80);
  c->fb24_len = (int)b24.w.size();
  c->fb16_len = (int)b16.w.size();
  if ((st = upload_vec(c, b24.w, &c->fb24)) || (st = upload_vec(c, b16.w, &c->fb16))) return st;
  if ((st = upload_vec(c, b24.band, &c->band24)) || (st = upload_vec(c, b16.band, &c->band16))) return st;
  if ((st = upload_vec(c, fft_twiddles(c->n_fft), &c->tw24)) || (st = upload_vec(c, fft_twiddles(400), &c->tw16)))
    return st;
  if ((st = upload_vec(c, hann_periodic(c->n_fft), &c->win_mel))) return st;
  if ((st = upload_vec(c, hann_periodic(400), &c->win16))) return st;
  return SVC_OK;
}

}  // namespace svc

extern "C" {

svc_status svc_mel_filterbank(int sr, int n_fft, int n_mels, double fmin, double fmax, float* out) {
  SVC_REQUIRE(out && n_fft > 0 && n_mels > 0, "mel_filterbank: bad args");
  auto w = slaney_mel(sr, n_fft, n_mels, fmin, fmax);
  memcpy(out, w.data(), w.size() * sizeof(float));
  return SVC_OK;
}

}  // extern "C"
