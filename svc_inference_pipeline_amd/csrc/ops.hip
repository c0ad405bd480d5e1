// Test and tool surface: the op-level entry points (svc_op_*), which run single launchers with the arguments the
// stages give them, and the GEMM microbenchmark.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "engine.h"

// ---------------------------------------------------------------------------- op-level (tests)
namespace svc {

int op_ws(svc_ctx** tmp) {
  static svc_ctx* g = nullptr;
  if (!g) {
    g = new svc_ctx();
    g->tune.from_env();
    g->tune0 = g->tune;
    int dev = 0;
    (void)hipGetDevice(&dev);
    g->device = dev;
    g->finalized = true;
  }
  *tmp = g;
  return SVC_OK;
}

}  // namespace svc

extern "C" {

static int pack_from_device(const float* w_dev, size_t wn, const float* b_dev, int bn, std::vector<float>& wh,
                            std::vector<float>& bh) {
  wh.resize(wn);
  bh.assign(bn, 0.0f);
  SVC_HIP_CHECK(hipDeviceSynchronize());
  SVC_HIP_CHECK(hipMemcpy(wh.data(), w_dev, wn * 4, hipMemcpyDeviceToHost));
  if (b_dev) SVC_HIP_CHECK(hipMemcpy(bh.data(), b_dev, bn * 4, hipMemcpyDeviceToHost));
  return SVC_OK;
}

static void free_packed(svc_ctx* c, PackedGemm& g) {
  // op-level packs are temporary: release the two allocations made by pack_gemm
  for (void* p : {(void*)g.W, (void*)g.bias}) {
    for (auto it = c->allocs.begin(); it != c->allocs.end(); ++it)
      if (*it == p) {
        c->allocs.erase(it);
        break;
      }
    (void)hipFree(p);
  }
}

svc_status svc_op_conv1d(const float* x, int B, int T_in, int Cin, const float* w, const float* bias, int Cout, int k,
                         int stride, int dilation, int pad, int act, float* y, void* stream) {
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  const int T_out = (T_in + 2 * pad - dilation * (k - 1) - 1) / stride + 1;
  SVC_REQUIRE(T_out > 0, "op_conv1d: T_out=%d", T_out);
  std::vector<float> wh, bh;
  PackedGemm g;
  int st;
  if ((st = pack_from_device(w, (size_t)Cout * Cin * k, bias, Cout, wh, bh))) return st;
  const int Cp = (int)round_up(Cin, 8);
  if ((st = pack_conv1d(c, g, wh.data(), bh.data(), Cout, Cin, k, Cp, dilation, pad, stride))) return st;
  f16* x16;
  if ((st = c->ws.plan([&](Arena& ws) { x16 = ws.get<f16>((size_t)B * T_in * Cp); }))) return st;
  if ((st = f32_to_f16(x, Cin, x16, Cp, B * T_in, Cin, Cp, s, false))) return st;
  EpiArgs e = epi();
  e.act = act;
  e.out32 = y;
  e.ld32 = Cout;
  st = run_gemm(g, x16, Cp, Cin, B, T_in, T_out, e, s);
  (void)hipStreamSynchronize(s);
  free_packed(c, g);
  return st;
}

svc_status svc_op_amp_conv_ex(const float* x, const void* x16, int B, int L, int C, const float* alpha_log,
                              const float* beta_log, const float* filt, const float* w, const float* bias, int k, int d,
                              const int32_t* tv, int tv_mul, const float* add_row, const float* acc32, float acc_div,
                              float* out32, void* out16, void* stream) {
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  SVC_REQUIRE(amp_conv_supported(C, k, d) && d > 0, "op_amp_conv: C=%d k=%d d=%d unsupported", C, k, d);
  SVC_REQUIRE((x != nullptr) != (x16 != nullptr), "op_amp_conv: exactly one of x (f32) and x16 (f16)");
  SVC_REQUIRE(out32 || out16, "op_amp_conv: no output");
  std::vector<float> wh, bh;
  PackedGemm g;
  int st;
  if ((st = pack_from_device(w, (size_t)C * C * k, bias, C, wh, bh))) return st;
  if ((st = pack_conv1d(c, g, wh.data(), bh.data(), C, C, k, C, d, (k - 1) / 2 * d, 1))) return st;
  // the epilogue fields as svc_bigvgan sets them (c1: out16 only; c2: add_row + out32; resblock sum / mean: + acc32
  // (+ acc_div), out32 possibly acc32 itself)
  EpiArgs e = epi();
  e.out32 = out32;
  e.ld32 = C;
  e.out16 = (f16*)out16;
  e.ld16 = C;
  e.add_row = add_row;
  e.ld_add_row = C;
  e.acc32 = acc32;
  e.ld_acc = C;
  if (acc32) e.acc_div = acc_div;
  AmpConvArgs p{x, B, L, k, d, alpha_log, beta_log, filt, g.W, g.Kpad, g.bias};
  p.x16 = (const f16*)x16;
  p.tv = tv;
  p.tv_mul = tv_mul;
  st = amp_conv(p, C, e, s);
  (void)hipStreamSynchronize(s);
  free_packed(c, g);
  return st;
}

svc_status svc_op_amp_conv(const float* x, int B, int L, int C, const float* alpha_log, const float* beta_log,
                           const float* filt, const float* w, const float* bias, int k, int d, const float* add_row,
                           float* y, void* stream) {
  return svc_op_amp_conv_ex(x, nullptr, B, L, C, alpha_log, beta_log, filt, w, bias, k, d, nullptr, 1, add_row, nullptr,
                            1.0f, y, nullptr, stream);
}

svc_status svc_op_conv_transpose1d_comb(const void* x16, int B, int T_in, int Cin, const float* w, const float* bias,
                                        int Cout, int k, int stride, const int32_t* tv, int tv_mul, float* y,
                                        void* stream) {
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  SVC_REQUIRE(x16 && y && B > 0 && T_in > 0 && Cin > 0 && Cout > 0 && k > 0 && stride > 0, "op_conv_transpose1d_comb: bad args");
  std::vector<float> wh, bh;
  int st;
  VStage S;
  S.cin = Cin;
  S.cout = Cout;
  S.rate = stride;
  S.k = k;
  if ((st = pack_from_device(w, (size_t)Cout * Cin * k, bias, Cout, wh, bh))) return st;
  if ((st = pack_conv_transpose_comb(c, S, wh.data(), nullptr, bh.data()))) return st;
  // no other path: a shape the packer declines is an error here (svc_bigvgan runs the phase GEMMs for it)
  SVC_REQUIRE(S.up_comb, "op_conv_transpose1d_comb: cin=%d cout=%d k=%d stride=%d has no combined form", Cin, Cout, k,
              stride);
  // as svc_bigvgan's up-sampling: k = 3, d = -1, the f16 stage input, out32 rows [B*T_in][2 cout] = [B*2 T_in][cout]
  AmpConvArgs q{nullptr, B, T_in, 3, -1, nullptr, nullptr, nullptr, S.upc.W, S.upc.Kpad, S.upc.bias};
  q.x16 = (const f16*)x16;
  q.noact = true;
  q.tv = tv;
  q.tv_mul = tv_mul;
  EpiArgs u = epi();
  u.out32 = y;
  u.ld32 = S.cin;
  st = amp_conv(q, S.cin, u, s);
  (void)hipStreamSynchronize(s);
  free_packed(c, S.upc);
  return st;
}

svc_status svc_op_conv_transpose1d(const float* x, int B, int T_in, int Cin, const float* w, const float* bias,
                                   int Cout, int k, int stride, int pad, float* y, void* stream) {
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  const int T_out = (T_in - 1) * stride - 2 * pad + k;
  SVC_REQUIRE(T_out == T_in * stride, "op_conv_transpose1d: only T_out = T_in*stride supported (got %d)", T_out);
  SVC_REQUIRE(Cin % 8 == 0, "op_conv_transpose1d: Cin %% 8");
  std::vector<float> wh, bh;
  PackedGemm g;
  int st;
  if ((st = pack_from_device(w, (size_t)Cout * Cin * k, bias, Cout, wh, bh))) return st;
  std::vector<PackedGemm> ph;
  if ((st = pack_conv_transpose(c, ph, wh.data(), nullptr, bh.data(), Cin, Cout, k, stride, pad))) return st;
  f16* x16;
  if ((st = c->ws.plan([&](Arena& ws) { x16 = ws.get<f16>((size_t)B * T_in * Cin); }))) return st;
  if ((st = f32_to_f16(x, Cin, x16, Cin, B * T_in, Cin, Cin, s, false))) return st;
  for (int r = 0; r < stride && !st; ++r) {
    EpiArgs e = epi();
    e.T_ostore = T_out;
    e.ostride = stride;
    e.ophase = r;
    e.out32 = y;
    e.ld32 = Cout;
    st = run_gemm(ph[r], x16, Cin, Cin, B, T_in, T_in, e, s);
  }
  (void)hipStreamSynchronize(s);
  for (auto& p : ph) free_packed(c, p);
  return st;
}

svc_status svc_op_activation1d(const float* x, int B, int L, int C, const float* al, const float* be, const float* f,
                               float* y, void* stream) {
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  int st;
  f16* y16;
  if ((st = c->ws.plan([&](Arena& ws) { y16 = ws.get<f16>((size_t)B * L * C); }))) return st;
  if ((st = activation1d(x, y16, B, L, C, C, al, be, f, s))) return st;
  // widen for the caller (the product path feeds the f16 tensor straight into the next conv)
  return f16_to_f32(y16, y, (int64_t)B * L * C, s);
}

svc_status svc_op_activation1d_x16(const void* x16, int B, int L, int C, const float* al, const float* be,
                                   const float* f, float* y, void* stream) {
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  int st;
  f16* y16;
  if ((st = c->ws.plan([&](Arena& ws) { y16 = ws.get<f16>((size_t)B * L * C); }))) return st;
  if ((st = activation1d(nullptr, y16, B, L, C, C, al, be, f, s, nullptr, 1, (const f16*)x16))) return st;
  return f16_to_f32(y16, y, (int64_t)B * L * C, s);
}

svc_status svc_op_attention(const float* q, const float* k, const float* v, int B, int L, int D, float* out,
                            void* stream) {
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  int st;
  const size_t rows = (size_t)B * L;
  f16 *qkv, *o16;
  if ((st = c->ws.plan([&](Arena& ws) {
        qkv = ws.get<f16>(rows * 3 * D);
        o16 = ws.get<f16>(rows * D);
      })))
    return st;
  if ((st = pack_qkv(q, k, v, qkv, (int64_t)rows, D, powf(64.0f, -0.25f), s))) return st;
  if ((st = attention(qkv, o16, B, L, D, s, false))) return st;
  return f16_to_f32(o16, out, (int64_t)rows * D, s);
}

svc_status svc_op_attention_ragged(const float* q, const float* k, const float* v, int B, int L, int D,
                                   const int32_t* lens, float* out, void* stream) {
  SVC_REQUIRE(q && k && v && out, "op_attention_ragged: null tensor");
  SVC_REQUIRE(D > 0 && D % 64 == 0 && L > 0 && B > 0, "op_attention_ragged: bad shape B=%d L=%d D=%d", B, L, D);
  for (int b = 0; lens && b < B; ++b)
    SVC_REQUIRE(lens[b] >= 1 && lens[b] <= L, "op_attention_ragged: utterance %d: length %d outside 1..%d", b, lens[b],
                L);
  if (!lens) return svc_op_attention(q, k, v, B, L, D, out, stream);
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  int st;
  const size_t rows = (size_t)B * L;
  f16 *qkv, *o16;
  if ((st = c->ws.plan([&](Arena& ws) {
        qkv = ws.get<f16>(rows * 3 * D);
        o16 = ws.get<f16>(rows * D);
      })))
    return st;
  RingRetire retire_(c->lens_main, s);
  void* dev = nullptr;
  if ((st = c->lens_main.put(lens, (size_t)B * sizeof(int32_t), s, &dev))) return st;
  // (the padding rows are packed too: element-wise, whatever they hold)
  if ((st = pack_qkv(q, k, v, qkv, (int64_t)rows, D, powf(64.0f, -0.25f), s))) return st;
  if ((st = attention(qkv, o16, B, L, D, s, false, (const int*)dev))) return st;
  return f16_to_f32(o16, out, (int64_t)rows * D, s);
}

svc_status svc_op_layernorm(const float* x, const float* g, const float* b, int rows, int D, float* y, void* stream) {
  return layernorm_f32(x, g, b, y, rows, D, D, (hipStream_t)stream);
}

// the sampler's element-wise launchers with the arguments sample_impl gives them
svc_status svc_op_init_noise(uint64_t seed, const int32_t* utt_ids, int B, int T, int C, float std, float* x, void* x16,
                             int ld16, int bf16, void* stream) {
  SVC_REQUIRE(utt_ids && x && x16 && B > 0 && T > 0 && C > 0 && ld16 >= C, "op_init_noise: bad args");
  SVC_REQUIRE((int64_t)B * T * C <= INT32_MAX, "op_init_noise: B*T*C past 2^31");
  return init_noise(x, (f16*)x16, ld16, B, T, C, seed, utt_ids, std, (hipStream_t)stream, bf16 != 0);
}

svc_status svc_op_q_sample(const float* mel, const float* mel_min, const float* mel_max, int B, int T, int C,
                           float sqrt_ac, float sqrt_1mac, const float* z, uint64_t seed, const int32_t* utt_ids,
                           const int32_t* frames, float* x, void* x16, int ld16, int bf16, void* stream) {
  SVC_REQUIRE(mel && mel_min && mel_max && x && B > 0 && T > 0 && C > 0 && (!x16 || ld16 >= C),
              "op_q_sample: bad args");
  SVC_REQUIRE((int64_t)B * T * C <= INT32_MAX, "op_q_sample: B*T*C past 2^31");
  SVC_REQUIRE(z || utt_ids, "op_q_sample: device noise (z NULL) needs utt_ids");
  QSampleArgs q{};
  q.mel = mel;
  q.mn = mel_min;
  q.mx = mel_max;
  q.noised = 1;
  q.a = sqrt_ac;
  q.b = sqrt_1mac;
  q.z = z;
  q.seed = seed;
  q.utt_ids = utt_ids;
  q.tv = frames;
  q.x = x;
  q.x16 = (f16*)x16;
  q.ld16 = ld16;
  q.bf16 = bf16 != 0;
  return q_sample(q, B, T, C, (hipStream_t)stream);
}

svc_status svc_op_plms_update(const float* e0, const float* e1, const float* e2, const float* e3, float c0, float c1,
                              float c2, float c3, int ne, float div, float d, float A, float Bc, const float* xin,
                              float* xout, void* x16, int ld16, float* e_avg_out, int bf16, int rows, int C,
                              void* stream) {
  PlmsArgs p{};
  const float* e[4] = {e0, e1, e2, e3};
  const float cf[4] = {c0, c1, c2, c3};
  SVC_REQUIRE(ne >= 1 && ne <= 4 && xin && xout && rows > 0 && C > 0 && (!x16 || ld16 >= C), "op_plms_update: bad args");
  SVC_REQUIRE((int64_t)rows * C <= INT32_MAX, "op_plms_update: rows*C past 2^31");
  for (int k = 0; k < ne; ++k) {
    SVC_REQUIRE(e[k], "op_plms_update: e%d is NULL (ne = %d)", k, ne);
    p.e[k] = e[k];
    p.c[k] = cf[k];
  }
  p.ne = ne;
  p.div = div;
  p.d = d;
  p.A = A;
  p.Bc = Bc;
  p.xin = xin;
  p.xout = xout;
  p.x16 = (f16*)x16;
  p.ld16 = ld16;
  p.e_avg_out = e_avg_out;
  p.bf16 = bf16 != 0;
  return plms_update(p, rows, C, (hipStream_t)stream);
}

svc_status svc_op_dpm_update(float* x, const float* eps, const float* d_prev, float* d_out, int rows, int C, float sra,
                             float srm1, float w0, float w1, float a, float b, int final_step, uint16_t* x16, int ld16,
                             int bf16, void* stream) {
  SVC_REQUIRE(x && eps && rows > 0 && C > 0 && (!x16 || ld16 >= C), "op_dpm_update: bad args");
  SVC_REQUIRE((int64_t)rows * C <= INT32_MAX, "op_dpm_update: rows*C past 2^31");
  DpmArgs p{};
  p.x = x;
  p.eps = eps;
  p.d_prev = final_step ? nullptr : d_prev;
  p.d_out = d_out;
  p.sra = sra;
  p.srm1 = srm1;
  p.w0 = w0;
  p.w1 = w1;
  p.a = a;
  p.b = b;
  p.final_step = final_step != 0;
  p.x16 = (f16*)x16;
  p.ld16 = ld16;
  p.bf16 = bf16 != 0;
  return dpm_update(p, rows, C, (hipStream_t)stream);
}

svc_status svc_op_ddpm_update(float* x, const float* eps, int B, int T, int C, float sra, float srm1, float c1,
                              float c2, float sigma, const float* z, uint64_t seed, const int32_t* utt_ids, int step,
                              void* x16, int ld16, int bf16, void* stream) {
  SVC_REQUIRE(x && eps && x16 && B > 0 && T > 0 && C > 0 && ld16 >= C, "op_ddpm_update: bad args");
  SVC_REQUIRE((int64_t)B * T * C <= INT32_MAX, "op_ddpm_update: B*T*C past 2^31");
  SVC_REQUIRE(z || utt_ids, "op_ddpm_update: device noise (z NULL) needs utt_ids");
  DdpmArgs a{};
  a.sra = sra;
  a.srm1 = srm1;
  a.c1 = c1;
  a.c2 = c2;
  a.sigma = sigma;
  a.z = z;
  a.seed = seed;
  a.utt_ids = utt_ids;
  a.step = step;
  a.bf16 = bf16 != 0;
  return ddpm_update(x, eps, (f16*)x16, ld16, B, T, C, a, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------- the DiffSVC denoiser's steps
// Each entry packs its f32 weights as build_mapper does (finalize.hip), runs the step's helper of stage_diffsvc.hip
// (the launcher choice denoise / project_cond make, by the op-level context's kernel switches) and frees the packs.
// C = 384 residual channels, n_mel = 100 (rows of 104 halves), as the fragment-order kernels are built for.
constexpr int OPD_C = 384, OPD_NMEL = 100, OPD_LDX = 104;

namespace {
// the operand format of the packs made inside the scope (svc_ctx::pack_bf16)
struct PackFormat {
  svc_ctx* c;
  PackFormat(svc_ctx* ctx, int bf16) : c(ctx) { c->pack_bf16 = bf16 != 0; }
  ~PackFormat() { c->pack_bf16 = false; }
};
// a packed weight set, its fragment-order copy and a scratch buffer, released after a stream sync
struct OpPacks {
  svc_ctx* c;
  hipStream_t s;
  std::vector<PackedGemm> g;
  std::vector<void*> tmp;
  OpPacks(svc_ctx* ctx, hipStream_t stream, int n) : c(ctx), s(stream), g(n) {}
  int alloc(size_t bytes, void** out) {
    SVC_HIP_CHECK(hipMalloc(out, bytes));
    tmp.push_back(*out);
    return SVC_OK;
  }
  ~OpPacks() {
    (void)hipStreamSynchronize(s);
    for (auto& p : g)
      if (p.W) free_packed(c, p);
    for (void* p : tmp) (void)hipFree(p);
  }
};
// [rows][2C] 16-bit words between the reference's channel order and a gate GEMM's paired order (pair_perm): to_packed
// dst[n] = src[perm[n]], else dst[perm[n]] = src[n]
int permute_cp(const void* src, void* dst, size_t rows, int C, bool to_packed) {
  const std::vector<int> perm = pair_perm(C);
  std::vector<uint16_t> a(rows * 2 * C), b(rows * 2 * C);
  SVC_HIP_CHECK(hipDeviceSynchronize());
  SVC_HIP_CHECK(hipMemcpy(a.data(), src, a.size() * 2, hipMemcpyDeviceToHost));
  for (size_t r = 0; r < rows; ++r)
    for (int n = 0; n < 2 * C; ++n) {
      if (to_packed) b[r * 2 * C + n] = a[r * 2 * C + perm[n]];
      else b[r * 2 * C + perm[n]] = a[r * 2 * C + n];
    }
  SVC_HIP_CHECK(hipMemcpy(dst, b.data(), b.size() * 2, hipMemcpyHostToDevice));
  return SVC_OK;
}
}  // namespace

svc_status svc_op_diffsvc_gate(const void* x16, int B, int T, const float* w, const float* bias, const void* cp16,
                               int dil, const int32_t* tv, int bf16, void* y16, void* stream) {
  SVC_REQUIRE(x16 && w && bias && cp16 && y16 && B > 0 && T > 0, "op_diffsvc_gate: bad args");
  SVC_REQUIRE(dil == 1 || dil == 2 || dil == 4 || dil == 8, "op_diffsvc_gate: dilation %d (1, 2, 4 or 8)", dil);
  SVC_REQUIRE((int64_t)B * T * 2 * OPD_C * 2 < (1ll << 30), "op_diffsvc_gate: %d x %d rows", B, T);
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  const int C = OPD_C;
  PackFormat fmt(c, bf16);
  OpPacks pk(c, s, 1);
  PackedGemm& g = pk.g[0];
  std::vector<float> wh, bh;
  int st;
  if ((st = pack_from_device(w, (size_t)2 * C * C * 3, bias, 2 * C, wh, bh))) return st;
  const std::vector<int> perm = pair_perm(C);
  if ((st = pack_conv1d(c, g, wh.data(), bh.data(), 2 * C, C, 3, C, dil, dil, 1, &perm))) return st;
  void *wf, *cpp;
  if ((st = pk.alloc(gate_ws_pack_elems() * sizeof(f16), &wf))) return st;  // gate_ws's fragment order, as build_mapper
  g.Wfrag = reinterpret_cast<f16*>(wf);
  if ((st = gate_ws_pack(g.W, g.Kpad, g.Wfrag, 0))) return st;
  SVC_HIP_CHECK(hipStreamSynchronize(0));
  if ((st = pk.alloc((size_t)B * T * 2 * C * sizeof(f16), &cpp))) return st;
  if ((st = permute_cp(cp16, cpp, (size_t)B * T, C, true))) return st;
  return diffsvc_gate(g, (const f16*)x16, (const f16*)cpp, (f16*)y16, C, B, T, tv, s);
}

svc_status svc_op_diffsvc_res(const void* g16, int M, const float* w, const float* bias, const float* sub,
                              const float* add, int store_lo, int lanes_cap, int bf16, void* hi, void* lo,
                              void* stream) {
  SVC_REQUIRE(g16 && w && bias && sub && add && hi && lo && M > 0, "op_diffsvc_res: bad args");
  SVC_REQUIRE(lanes_cap >= -2 && lanes_cap <= 512, "op_diffsvc_res: lanes_cap %d (-1 tiled GEMM, -2, 0 or a lane count)",
              lanes_cap);
  SVC_REQUIRE((int64_t)M * OPD_C * 2 < (1ll << 30), "op_diffsvc_res: %d rows", M);
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  const int C = OPD_C;
  PackFormat fmt(c, bf16);
  OpPacks pk(c, s, 1);
  PackedGemm& g = pk.g[0];
  std::vector<float> wh, bh;
  int st;
  if ((st = pack_from_device(w, (size_t)C * C, bias, C, wh, bh))) return st;
  if ((st = pack_conv1d(c, g, wh.data(), bh.data(), C, C, 1, C, 1, 0, 1))) return st;
  void* wf;
  if ((st = pk.alloc(res_proj_pack_elems() * sizeof(f16), &wf))) return st;
  g.Wfrag = reinterpret_cast<f16*>(wf);
  if ((st = res_proj_pack(g.W, g.Kpad, g.Wfrag, 0))) return st;
  SVC_HIP_CHECK(hipStreamSynchronize(0));
  return diffsvc_residual(g, (const f16*)g16, sub, add, (f16*)hi, (f16*)lo, C, 1, M, lanes_cap, store_lo != 0, s);
}

svc_status svc_op_diffsvc_melpre(const void* x16, int M, const float* w, const float* bias, const float* add, int bf16,
                                 void* hi, void* lo, void* stream) {
  SVC_REQUIRE(x16 && w && bias && add && hi && lo && M > 0, "op_diffsvc_melpre: bad args");
  SVC_REQUIRE((int64_t)M * OPD_C * 2 < (1ll << 30), "op_diffsvc_melpre: %d rows", M);
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  const int C = OPD_C;
  PackFormat fmt(c, bf16);
  OpPacks pk(c, s, 1);
  PackedGemm& g = pk.g[0];
  std::vector<float> wh, bh;
  int st;
  if ((st = pack_from_device(w, (size_t)C * OPD_NMEL, bias, C, wh, bh))) return st;
  if ((st = pack_conv1d(c, g, wh.data(), bh.data(), C, OPD_NMEL, 1, OPD_LDX, 1, 0, 1))) return st;
  if (g.Kpad == 128 && g.K <= 128) {  // mel_proj's shape, as build_mapper
    void* wf;
    if ((st = pk.alloc(mel_proj_pack_elems() * sizeof(f16), &wf))) return st;
    g.Wfrag = reinterpret_cast<f16*>(wf);
    if ((st = mel_proj_pack(g.W, g.Kpad, g.Wfrag, 0))) return st;
    SVC_HIP_CHECK(hipStreamSynchronize(0));
  }
  return diffsvc_melpre(g, (const f16*)x16, OPD_LDX, OPD_NMEL, add, (f16*)hi, (f16*)lo, C, 1, M, s);
}

svc_status svc_op_diffsvc_skipsum(const void* g16, int NL, int rows_total, int row0, int rows, const float* w,
                                  const float* bias, int bf16, void* s16, void* stream) {
  SVC_REQUIRE(g16 && w && bias && s16 && NL >= 1 && NL <= 64, "op_diffsvc_skipsum: bad args");
  SVC_REQUIRE(rows_total > 0 && row0 >= 0 && rows > 0 && (int64_t)row0 + rows <= rows_total,
              "op_diffsvc_skipsum: rows [%d, %d + %d) of %d", row0, row0, rows, rows_total);
  SVC_REQUIRE((int64_t)NL * rows_total * OPD_C * 2 < (1ll << 30), "op_diffsvc_skipsum: %d x %d rows", NL, rows_total);
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  const int C = OPD_C;
  PackFormat fmt(c, bf16);
  OpPacks pk(c, s, 1);
  std::vector<float> wh, bh;
  int st;
  if ((st = pack_from_device(w, (size_t)NL * C * C, bias, NL * C, wh, bh))) return st;
  std::vector<const float*> ow(NL), ob(NL);
  for (int l = 0; l < NL; ++l) {
    ow[l] = wh.data() + (size_t)l * C * C;
    ob[l] = bh.data() + (size_t)l * C;
  }
  if ((st = pack_skip_all(c, pk.g[0], ow.data(), ob.data(), C, NL))) return st;
  // a sampler sub-batch: its rows of every layer's block, the layer stride that of the whole batch
  return diffsvc_skipsum(pk.g[0], (const f16*)g16 + (size_t)row0 * C, (size_t)rows_total * C, NL, (f16*)s16, C, true,
                         rows, s);
}

svc_status svc_op_diffsvc_head(const void* s16, int M, const float* wsp, const float* bsp, const float* wout,
                               const float* bout, int bf16, float* eps, void* stream) {
  SVC_REQUIRE(s16 && wsp && bsp && wout && bout && eps && M > 0, "op_diffsvc_head: bad args");
  SVC_REQUIRE((int64_t)M * 3 * OPD_C * 2 < (1ll << 30), "op_diffsvc_head: %d rows", M);
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  const int C = OPD_C;
  PackFormat fmt(c, bf16);
  OpPacks pk(c, s, 2);
  std::vector<float> wh, bh, wh2, bh2;
  int st;
  if ((st = pack_from_device(wsp, (size_t)C * C, bsp, C, wh, bh))) return st;
  if ((st = pack_from_device(wout, (size_t)OPD_NMEL * C, bout, OPD_NMEL, wh2, bh2))) return st;
  if ((st = pack_conv1d_opt(c, pk.g[0], wh.data(), bh.data(), C, C, 1, C, 1, 0, 1, true))) return st;
  if ((st = pack_conv1d_opt(c, pk.g[1], wh2.data(), bh2.data(), OPD_NMEL, C, 1, C, 1, 0, 1, true))) return st;
  f16* u16;
  if ((st = c->ws.plan([&](Arena& ws) { u16 = ws.get<f16>((size_t)M * 3 * C); }))) return st;
  return diffsvc_head(pk.g[0], pk.g[1], (const f16*)s16, u16, eps, C, OPD_NMEL, true, 1, M, s);
}

svc_status svc_op_diffsvc_condproj(const float* cond, int M, int NL, const float* w, const float* bias, int bf16,
                                   void* cp16, void* stream) {
  SVC_REQUIRE(cond && w && bias && cp16 && M > 0 && NL >= 1 && NL <= 64, "op_diffsvc_condproj: bad args");
  SVC_REQUIRE((int64_t)NL * M * 2 * OPD_C * 2 < (1ll << 30), "op_diffsvc_condproj: %d x %d rows", NL, M);
  svc_ctx* c;
  op_ws(&c);
  TuningScope tuning_scope_(&c->tune);
  hipStream_t s = (hipStream_t)stream;
  const int C = OPD_C;
  PackFormat fmt(c, bf16);
  OpPacks pk(c, s, 1);
  std::vector<float> wh, bh;
  int st;
  if ((st = pack_from_device(w, (size_t)NL * 2 * C * C, bias, NL * 2 * C, wh, bh))) return st;
  std::vector<const float*> cw(NL), cb(NL);
  for (int l = 0; l < NL; ++l) {
    cw[l] = wh.data() + (size_t)l * 2 * C * C;
    cb[l] = bh.data() + (size_t)l * 2 * C;
  }
  if ((st = pack_cond_all(c, pk.g[0], cw.data(), cb.data(), C, NL, C))) return st;
  f16* cond16;
  if ((st = c->ws.plan([&](Arena& ws) { cond16 = ws.get<f16>((size_t)M * 3 * C); }))) return st;
  void* cpp;  // the projections in the gate GEMMs' paired order, as project_cond leaves them
  if ((st = pk.alloc((size_t)NL * M * 2 * C * sizeof(f16), &cpp))) return st;
  if ((st = diffsvc_condproj(pk.g[0], cond, cond16, (f16*)cpp, (size_t)M * 2 * C, C, bf16 != 0, 1, M, s))) return st;
  SVC_HIP_CHECK(hipStreamSynchronize(s));
  return permute_cp(cpp, cp16, (size_t)NL * M, C, false);
}

}  // extern "C"

// ---------------------------------------------------------------------------- GEMM microbenchmark
// Times `iters` launches of one implicit-GEMM configuration on synthetic operands (tools/gemm_bench.py):
// M rows, N packed columns, K = taps*Cp, 1-tap or 3-tap conv, epilogue 0 = f16 store, 1 = paired gate.
__global__ void fill_f16_kernel(f16* p, int64_t n, uint32_t seed) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t h = (uint32_t)i * 2654435761u ^ seed;
  h ^= h >> 13;
  h *= 0x5bd1e995u;
  h ^= h >> 15;
  p[i] = (f16)(((h & 0xFFFF) / 65536.0f - 0.5f) * 0.5f);
}

extern "C" svc_status svc_gemm_bench(int M, int N, int Cin, int taps, int epi_kind, int variant, int iters, double* ms_out) {
  svc_ctx* oc;
  op_ws(&oc);
  TuningScope tuning_scope_(&oc->tune);
  SVC_REQUIRE(M > 0 && N > 0 && Cin % 8 == 0 && taps >= 1 && iters != 0, "gemm_bench: bad args");
  SVC_REQUIRE(epi_kind < 3 || epi_kind == 6 || variant == 24,
              "gemm_bench: the diagnostic gate epilogues (3-5) exist in variant 24 only");
  SVC_REQUIRE((variant >= 10 && variant <= 16) || variant == 20 || variant == 24 ||
                  (variant == 30 && epi_kind == 6 && N == 384 && Cin == 384 && taps == 1) ||
                  (variant == 40 && epi_kind == 1 && N == 768 && Cin == 384 && taps == 3),
              "gemm_bench: variant %d (30: res_proj, split residual epilogue, N = Cin = 384, 1 tap; 40: gate_ws, "
              "gate epilogue, N = 768, Cin = 384, 3 taps)", variant);
  const int K = taps * Cin, Kpad = (int)round_up(K, 64), Npad = (int)std::max(round_up(N, 256), round_up(N, 384));
  f16 *X, *W, *Y, *cp;
  float *bias, *R = nullptr;
  if (epi_kind == 2 || epi_kind == 6) {  // DiffSVC residual epilogue: x32 (6: split-fp16 lo half) read-modify-write
    SVC_HIP_CHECK(hipMalloc(&R, (size_t)M * N * 4));
    SVC_HIP_CHECK(hipMemset(R, 0, (size_t)M * N * 4));
  }
  SVC_HIP_CHECK(hipMalloc(&X, (size_t)M * Cin * 2));
  SVC_HIP_CHECK(hipMalloc(&W, (size_t)Npad * Kpad * 2));
  SVC_HIP_CHECK(hipMalloc(&Y, (size_t)M * N * 2));
  SVC_HIP_CHECK(hipMalloc(&cp, (size_t)M * N * 2));
  SVC_HIP_CHECK(hipMalloc(&bias, (size_t)Npad * 4));
  SVC_HIP_CHECK(hipMemset(bias, 0, (size_t)Npad * 4));
  hipLaunchKernelGGL(fill_f16_kernel, dim3(cdiv((int64_t)M * Cin, 256)), dim3(256), 0, 0, X, (int64_t)M * Cin, 1u);
  hipLaunchKernelGGL(fill_f16_kernel, dim3(cdiv((int64_t)Npad * Kpad, 256)), dim3(256), 0, 0, W, (int64_t)Npad * Kpad, 2u);
  hipLaunchKernelGGL(fill_f16_kernel, dim3(cdiv((int64_t)M * N, 256)), dim3(256), 0, 0, cp, (int64_t)M * N, 3u);
  // Y is also the residual hi half of the split epilogue (epi 6 / res_proj): defined values, no NaN / Inf patterns
  hipLaunchKernelGGL(fill_f16_kernel, dim3(cdiv((int64_t)M * N, 256)), dim3(256), 0, 0, Y, (int64_t)M * N, 4u);
  ConvGemmArgs a{};
  a.X = X; a.ldx = Cin; a.T_in = M; a.Cp = Cin; a.Cvalid = Cin; a.W = W; a.K = K; a.Kpad = Kpad;
  a.tap_mul = 1; a.tap_add = -(taps / 2); a.istride = 1; a.B = 1; a.T_out = M; a.N = N;
  if (const char* dv = getenv("SVC_BENCH_DIL")) {  // (bench tool only) the dilated conv's tap shift
    a.tap_mul = atoi(dv);
    a.tap_add = -(taps / 2) * a.tap_mul;
  }
  EpiArgs e = epi();
  e.bias = bias; e.T_ostore = M; e.ostride = 1;
  if (epi_kind == 1 || (epi_kind >= 3 && epi_kind <= 5)) {  // diagnostics: 3 = no cp read, no y store; 4 = no cp read; 5 = no y store
    e.kind = EPI_GATE; e.cp = (epi_kind == 3 || epi_kind == 4) ? nullptr : cp; e.ld_cp = N;
    e.y16 = (epi_kind == 3 || epi_kind == 5) ? nullptr : Y;
    e.ldy16 = N / 2;
  } else {
    e.out16 = Y; e.ld16 = N;
    if (epi_kind == 2) {
      e.acc32 = R; e.ld_acc = N; e.acc_div = 1.41421356237309515f; e.out32 = R; e.ld32 = N; e.add16 = bias;
    } else if (epi_kind == 6) {  // split residual in place, as diffsvc.outproj: (Y + lo) - sub -> Y / lo
      e.acc16_hi = Y; e.acc16_lo = reinterpret_cast<f16*>(R); e.acc_sub = bias; e.lo16 = reinterpret_cast<f16*>(R);
      e.ld_acc = N; e.acc_div = 1.41421356237309515f; e.add16 = bias;
    }
  }
  f16* Wf = nullptr;  // variant 30 / 40: res_proj's / gate_ws's fragment-order weights
  int st = SVC_OK;
  if (variant == 30) {
    SVC_HIP_CHECK(hipMalloc(&Wf, res_proj_pack_elems() * sizeof(f16)));
    st = res_proj_pack(W, Kpad, Wf, 0);  // (on failure: no launches below, the buffers are freed at the end)
  } else if (variant == 40) {
    SVC_HIP_CHECK(hipMalloc(&Wf, gate_ws_pack_elems() * sizeof(f16)));
    st = gate_ws_pack(W, Kpad, Wf, 0);
    a.Wfrag = Wf;
  }
  hipEvent_t e0, e1;
  SVC_HIP_CHECK(hipEventCreate(&e0));
  SVC_HIP_CHECK(hipEventCreate(&e1));
  // iters < 0: |iters| launches each after a 1 GiB (SVC_BENCH_FLUSH_MB) memset (operands evicted from L2 and the 256 MiB Infinity Cache,
  // as inside the sampler, where other layers' buffers stream between two launches of one GEMM), timed one by one
  const bool cold = iters < 0;
  if (cold) iters = -iters;
  void* flush = nullptr;
  size_t flush_bytes = (size_t)1 << 30;
  if (const char* fm = getenv("SVC_BENCH_FLUSH_MB")) flush_bytes = (size_t)atoi(fm) << 20;  // (bench tool only)
  if (cold) SVC_HIP_CHECK(hipMalloc(&flush, flush_bytes));
  // (bench tool only) res_proj's row lanes: -2 one workgroup per CU (the one-stream sampler's), 0 3/8 of the CUs
  const int rp_lanes = getenv("SVC_BENCH_RP_LANES") ? atoi(getenv("SVC_BENCH_RP_LANES")) : 0;
  const bool rp_lo = !getenv("SVC_BENCH_RP_NOLO");  // (bench tool only) the form without the lo store
  auto run = [&]() {
    if (variant == 30)
      return res_proj(X, Wf, bias, bias, bias, e.acc_div, Y, reinterpret_cast<f16*>(R), M, false, rp_lanes, rp_lo, 0);
    if (variant == 20 || variant == 24) return conv_gemm4(a, e, zero_page(), 0, variant == 24);
    if (variant == 40) return gate_ws(a, e, 0);
    return conv_gemm3(a, e, zero_page(), variant - 10, 0);
  };
  for (int w = 0; w < 2 && !st; ++w) st = run();
  if (const char* sp = variant == 40 ? getenv("SVC_GWS_STAMPS") : nullptr) {  // (bench tool only) step timeline
    unsigned long long* ds = nullptr;
    const size_t n = (size_t)256 * gate_ws_nstamp();
    SVC_HIP_CHECK(hipMalloc(&ds, n * 8));
    SVC_HIP_CHECK(hipMemset(ds, 0, n * 8));
    SVC_HIP_CHECK(hipDeviceSynchronize());
    gate_ws_stamps = ds;
    for (int w = 0; w < 3 && !st; ++w) st = run();  // the last launch's stamps remain
    gate_ws_stamps = nullptr;
    SVC_HIP_CHECK(hipDeviceSynchronize());
    std::vector<unsigned long long> hs(n);
    SVC_HIP_CHECK(hipMemcpy(hs.data(), ds, n * 8, hipMemcpyDeviceToHost));
    (void)hipFree(ds);
    if (FILE* f = fopen(sp, "wb")) {
      fwrite(hs.data(), 8, n, f);
      fclose(f);
    }
  }
  if (const char* sp = variant == 30 ? getenv("SVC_RP_STAMPS") : nullptr) {  // (bench tool only) ramp / steady / drain
    unsigned long long* ds = nullptr;
    const size_t n = (size_t)1024 * res_proj_nstamp();  // (at most 2 x 512 row lanes' workgroups)
    SVC_HIP_CHECK(hipMalloc(&ds, n * 8));
    SVC_HIP_CHECK(hipMemset(ds, 0, n * 8));
    SVC_HIP_CHECK(hipDeviceSynchronize());
    res_proj_stamps = ds;
    for (int w = 0; w < 3 && !st; ++w) {  // the last launch's stamps remain
      if (cold) SVC_HIP_CHECK(hipMemsetAsync(flush, w, flush_bytes, 0));  // (operands from HBM, as in the sampler)
      st = run();
    }
    res_proj_stamps = nullptr;
    SVC_HIP_CHECK(hipDeviceSynchronize());
    std::vector<unsigned long long> hs(n);
    SVC_HIP_CHECK(hipMemcpy(hs.data(), ds, n * 8, hipMemcpyDeviceToHost));
    (void)hipFree(ds);
    if (FILE* f = fopen(sp, "wb")) {
      fwrite(hs.data(), 8, n, f);
      fclose(f);
    }
  }
  if (const char* dump = getenv("SVC_BENCH_DUMP")) {  // (bench tool only) the gate output of the warm-up launches
    SVC_HIP_CHECK(hipDeviceSynchronize());
    std::vector<f16> hy((size_t)M * N / 2);
    SVC_HIP_CHECK(hipMemcpy(hy.data(), Y, hy.size() * sizeof(f16), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(dump, "wb")) {
      fwrite(hy.data(), sizeof(f16), hy.size(), f);
      fclose(f);
    }
  }
  float ms = 0;
  if (cold) {
    for (int i = 0; i < iters && !st; ++i) {
      SVC_HIP_CHECK(hipMemsetAsync(flush, i & 0xff, flush_bytes, 0));
      SVC_HIP_CHECK(hipEventRecord(e0, 0));
      st = run();
      SVC_HIP_CHECK(hipEventRecord(e1, 0));
      SVC_HIP_CHECK(hipEventSynchronize(e1));
      float one = 0;
      SVC_HIP_CHECK(hipEventElapsedTime(&one, e0, e1));
      ms += one;
    }
    (void)hipFree(flush);
  } else if (getenv("SVC_BENCH_PERLAUNCH")) {  // (bench tool only) each launch between its own event pair, as
    // bench.py's live profile brackets them: the event markers' own cost per launch
    std::vector<hipEvent_t> ev(2 * (size_t)iters);
    for (auto& x : ev) SVC_HIP_CHECK(hipEventCreate(&x));
    for (int i = 0; i < iters && !st; ++i) {  // back to back, no host synchronisation in between
      SVC_HIP_CHECK(hipEventRecord(ev[2 * i], 0));
      st = run();
      SVC_HIP_CHECK(hipEventRecord(ev[2 * i + 1], 0));
    }
    SVC_HIP_CHECK(hipEventSynchronize(ev.back()));
    for (int i = 0; i < iters; ++i) {
      float one = 0;
      SVC_HIP_CHECK(hipEventElapsedTime(&one, ev[2 * i], ev[2 * i + 1]));
      ms += one;
    }
    for (auto& x : ev) (void)hipEventDestroy(x);
  } else {
    SVC_HIP_CHECK(hipEventRecord(e0, 0));
    for (int i = 0; i < iters && !st; ++i)
      st = run();
    SVC_HIP_CHECK(hipEventRecord(e1, 0));
    SVC_HIP_CHECK(hipEventSynchronize(e1));
    SVC_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  }
  *ms_out = ms / iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  for (void* p : {(void*)X, (void*)W, (void*)Y, (void*)cp, (void*)bias, (void*)R, (void*)Wf}) if (p) (void)hipFree(p);
  return st;
}
