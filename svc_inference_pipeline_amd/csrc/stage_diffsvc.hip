// The DiffSVC denoiser and its samplers: DDPM, PLMS, and DPM-Solver++(2M) / DDIM over a list of timesteps.
#include <math.h>

#include "engine.h"

// ---------------------------------------------------------------------------- DiffSVC denoiser
struct DenoiseBufs {
  f16* cp16;     // [rows][NL*2C] conditioner projections of every layer (hoisted out of the sampler loop)
  f16* y16;      // [rows][C] next layer input x + diffusion_projection (the high half of the split residual stream)
  f16* g16;      // [rows][NL*C] gate outputs of every layer (A operand of the skip GEMM)
  f16* s16;      // [rows][3C] sum(skip) / sqrt(NL) ([hi | lo | hi] split-fp16 with head_split, else [rows][C])
  f16* u16;      // [rows][3C] relu(skip_projection), same layout
  f16* lo16;     // [rows][C] low half of the split residual stream: x + dproj = y16 + lo16
  size_t cp_ls;  // elements between layers of cp16, which is LAYER-major [NL][rows_total][2C]: each layer's gate
                 // epilogue reads one contiguous block (row-major over all layers put 30 KB between its rows)
  size_t g_ls;   // elements between layers of g16, also layer-major [NL][rows_total][C]: the gate GEMM writes and the
                 // residual GEMM reads one contiguous block; the skip GEMM reads the NL blocks as NL "taps" whose row
                 // shift is the layer stride (tap_mul = rows_total)
  f16* cond16;   // [rows][3C] the conditioner output as the [hi | lo | hi] operand of the projections (project_cond)
};


namespace svc {

// Residual stream x in split-fp16 storage (x + dproj_l = hi + lo, ~22 significand bits in 4 bytes): the layer's GEMM
// operand is its high half, so each residual update moves 10 instead of 12 bytes per element (an f32 residual stream
// measured 1.1 % slower end to end at the same mel-L1, round 1; removed in round 3).
int diffsvc_melpre(const PackedGemm& melpre, const f16* x16, int ldx16, int n_mel, const float* add, f16* hi, f16* lo,
                   int C, int B, int T, hipStream_t s) {
  if (tuning().res_proj && melpre.Wfrag && ldx16 <= 128) {
    // weight-stationary store stream (res_proj.hip mel_proj), bit-identical to the tiled GEMM
    prof_site("diffsvc.melpre");
    return mel_proj(x16, ldx16, melpre.Wfrag, melpre.bias, add, hi, lo, B * T, melpre.bf16, s);
  }
  EpiArgs e = epi();
  e.act = ACT_RELU;
  e.lo16 = lo;
  e.out16 = hi;
  e.ld16 = C;
  e.add16 = add;
  return run_gemm(melpre, x16, ldx16, n_mel, B, T, T, e, s, "diffsvc.melpre");
}

int diffsvc_gate(const PackedGemm& dil, const f16* x16, const f16* cp, f16* y16, int C, int B, int T, const int* tv,
                 hipStream_t s) {
  EpiArgs g = epi();
  g.kind = EPI_GATE;
  g.cp = cp;
  g.ld_cp = 2 * C;
  g.y16 = y16;
  g.ldy16 = C;
  return run_gemm(dil, x16, C, C, B, T, T, g, s, "diffsvc.dilated", tv, 1);
}

int diffsvc_res_lanes() {
  if (!tuning().res_proj) return -1;
  return tuning().res_proj > 1 ? tuning().res_proj : (tuning().sampler_streams == 1 ? -2 : 0);
}

// x = (x + residual) / sqrt(2); next input x + diffusion_projection_{i+1}(step):
// x_i = (hi + lo) - dproj_i (sub), and x_{i+1} + dproj_{i+1} (add) goes back split into hi / lo
int diffsvc_residual(const PackedGemm& outres, const f16* g16, const float* sub, const float* add, f16* hi, f16* lo,
                     int C, int B, int T, int lanes_cap, bool store_lo, hipStream_t s) {
  if (lanes_cap != -1 && C == 384 && outres.Wfrag && outres.N == C && outres.K == C) {
    // weight-stationary row stream (res_proj.hip), bit-identical to the tiled GEMM below
    prof_site("diffsvc.outproj");
    return res_proj(g16, outres.Wfrag, outres.bias, sub, add, 1.41421356237309515f, hi, lo, B * T, outres.bf16,
                    lanes_cap, store_lo, s);
  }
  EpiArgs r = epi();
  r.ld_acc = C;
  r.acc_div = 1.41421356237309515f;
  r.acc16_hi = hi;
  r.acc16_lo = lo;
  r.acc_sub = sub;
  r.lo16 = lo;
  r.out16 = hi;
  r.ld16 = C;
  r.add16 = add;
  return run_gemm(outres, g16, C, C, B, T, T, r, s, "diffsvc.outproj");
}

// skip = sum_i skip_i (modules/diffsvc.py:311); x = skip / sqrt(len(layers)) (:315)
int diffsvc_skipsum(const PackedGemm& skip_all, const f16* g16, size_t g_ls, int NL, f16* s16, int C, bool head_split,
                    int rows, hipStream_t s) {
  const int H3 = head_split ? 3 : 1;  // split-fp16 head operands are [hi | lo | hi] rows
  EpiArgs e = epi();
  e.scale_cols = C;
  e.col_scale = 1.0f / sqrtf((float)NL);
  e.out16 = s16;
  e.ld16 = C * H3;
  e.split16 = H3 == 3 ? C : 0;
  PackedGemm sk = skip_all;  // K index l * C + k = "tap" l * Cp + k with Cp = C: same packed weights
  sk.Cp = C;
  sk.taps = NL;
  sk.tap_mul = (int)(g_ls / C);
  sk.tap_add = 0;
  sk.istride = 1;
  return run_gemm(sk, g16, C, C, 1, NL * sk.tap_mul, rows, e, s, "diffsvc.skipsum");
}

int diffsvc_head(const PackedGemm& skipproj, const PackedGemm& outproj, const f16* s16, f16* u16, float* eps, int C,
                 int n_mel, bool head_split, int B, int T, hipStream_t s) {
  const int H3 = head_split ? 3 : 1;
  // relu(skip_projection) and output_projection in one launch: u never reaches HBM (diff_head.hip)
  if (tuning().diff_head && H3 == 3 && C == 384 && skipproj.N == C && skipproj.Npad >= C && skipproj.K == 3 * C &&
      skipproj.Kpad == 3 * C && outproj.K == 3 * C && outproj.Kpad == 3 * C && outproj.Npad >= 128 &&
      outproj.N <= 128 && n_mel % 4 == 0)
    return diff_head(s16, skipproj.W, skipproj.bias, C, 3 * C, outproj.W, outproj.bias, outproj.N, 3 * C, outproj.Npad,
                     eps, n_mel, B * T, zero_page(), s, skipproj.bf16);
  int st;
  EpiArgs e = epi();
  e.act = ACT_RELU;
  e.out16 = u16;
  e.ld16 = C * H3;
  e.split16 = H3 == 3 ? C : 0;
  if ((st = run_gemm(skipproj, s16, C * H3, C * H3, B, T, T, e, s, "diffsvc.skipproj"))) return st;
  e = epi();
  e.out32 = eps;
  e.ld32 = n_mel;
  return run_gemm(outproj, u16, C * H3, C * H3, B, T, T, e, s, "diffsvc.eps_out");
}

int diffsvc_condproj(const PackedGemm& cp_all, const float* cond, f16* cond16, f16* cp16, size_t cp_ls, int C,
                     bool bf16, int B, int T, hipStream_t s) {
  int st;
  if ((st = f32_to_f16x3(cond, C, cond16, B * T, C, s, bf16))) return st;  // [hi | lo | hi] split-fp16 operand
  // the projections of all layers as ONE GEMM over the packed weights (N = NL x 2C), each layer's 2C columns written
  // to its layer-major cp block (EpiArgs col_block): 20 launches of 470 tiles (1.8 rounds of workgroups each) became
  // one launch of 9 400 (round 5)
  EpiArgs e = epi();
  e.out16 = cp16;
  e.ld16 = 2 * C;
  e.col_block = 2 * C;
  e.col_block_stride = (int64_t)cp_ls;
  return run_gemm(cp_all, cond16, 3 * C, 3 * C, B, T, T, e, s, "diffsvc.condproj");
}

}  // namespace svc

// the sampler update that consumes a denoise's eps: none, the PLMS one or the DPM-Solver one
struct EpsUpdate {
  const PlmsArgs* plms = nullptr;
  const DpmArgs* dpm = nullptr;
  EpsUpdate() {}
  EpsUpdate(const PlmsArgs* p) : plms(p) {}
  EpsUpdate(const DpmArgs* d) : dpm(d) {}
};

// tv (device, optional): ragged batches, utterance b has tv[b] valid frames; only the dilated convs look across frames
// up (optional): the sampler update that consumes this eps, launched right after the head
static int denoise(svc_ctx* c, const DenoiseBufs& bb, const f16* x16, int B, int T, int t, float* eps, hipStream_t s,
                   const int* tv, EpsUpdate up = {}) {
  const int C = c->C, NL = c->n_layers, rows = B * T;
  const int ldx16 = (int)round_up(c->n_mel, 8);
  const float* dp = c->dproj + (size_t)t * NL * C;  // the step's diffusion projections, [NL][C]
  int st;
  if ((st = diffsvc_melpre(c->melpre, x16, ldx16, c->n_mel, dp, bb.y16, bb.lo16, C, B, T, s))) return st;
  // the split residual stream's high half, updated in place (y16) by gate + res_proj
  f16* hi = bb.y16;
  for (int i = 0; i < NL; ++i) {
    f16* g16 = bb.g16 + (size_t)i * bb.g_ls;
    if ((st = diffsvc_gate(c->dil[i], hi, bb.cp16 + (size_t)i * bb.cp_ls, g16, C, B, T, tv, s))) return st;
    if (i + 1 == NL) break;  // the last layer's residual output is unused (only skips feed the head)
    if ((st = diffsvc_residual(c->outres[i], g16, dp + (size_t)i * C, dp + (size_t)(i + 1) * C, hi, bb.lo16, C, B, T,
                               diffsvc_res_lanes(),
                               i + 2 < NL /* the last residual layer's low half is never read: layer NL - 1 has no update */,
                               s)))
      return st;
  }
  if ((st = diffsvc_skipsum(c->skip_all, bb.g16, bb.g_ls, NL, bb.s16, C, c->head_split, rows, s))) return st;
  if ((st = diffsvc_head(c->skipproj, c->outproj, bb.s16, bb.u16, eps, C, c->n_mel, c->head_split, B, T, s))) return st;
  if (up.plms) return plms_update(*up.plms, rows, c->n_mel, s);
  return up.dpm ? dpm_update(*up.dpm, rows, c->n_mel, s) : SVC_OK;
}

// the denoiser's part of a workspace layout (the sampler's, svc_diffsvc_eps's): gets only
static void layout_denoise(svc_ctx* c, Arena& ws, int B, int T, DenoiseBufs& bb) {
  const size_t rows = (size_t)B * T, C = c->C;
  bb.cp16 = ws.get<f16>(rows * c->n_layers * 2 * C);
  bb.y16 = ws.get<f16>(rows * C);
  bb.g16 = ws.get<f16>(rows * c->n_layers * C);
  bb.s16 = ws.get<f16>(rows * C * 3);  // [hi | lo | hi] when head_split
  bb.u16 = ws.get<f16>(rows * C * 3);
  bb.lo16 = ws.get<f16>(rows * C);
  bb.cp_ls = rows * 2 * C;
  bb.g_ls = rows * C;
  bb.cond16 = ws.get<f16>(rows * 3 * C);
}

static int project_cond(svc_ctx* c, const float* cond, int B, int T, const DenoiseBufs& bb, hipStream_t s) {
  return diffsvc_condproj(c->cp_all, cond, bb.cond16, bb.cp16, bb.cp_ls, c->C, c->bf16, B, T, s);
}

namespace svc {

// ragged batches: validate the per-utterance frame counts (host) and stage them to the device through `ring`
int stage_frames(StageRing& ring, const int32_t* frames, int B, int T, hipStream_t s, const int** dev_out) {
  *dev_out = nullptr;
  if (!frames) return SVC_OK;
  for (int b = 0; b < B; ++b)
    SVC_REQUIRE(frames[b] >= 1 && frames[b] <= T, "utterance %d: %d frames (batch length %d)", b, frames[b], T);
  void* dev = nullptr;
  int st = ring.put(frames, (size_t)B * sizeof(int32_t), s, &dev);
  *dev_out = reinterpret_cast<const int*>(dev);
  return st;
}

}  // namespace svc

// K (1..steps): the sampler starts at noise level K - 1, DDPM at step K - 1 and PLMS at ((K - 1) / interval) * interval
// with an empty history; K = steps is the whole schedule (svc_diffsvc_sample). The start state is x_T when given, else
// mel_src normalised and noised forward to level K - 1 (q_sample), else the x_T draw. noise (DDPM): [K][B*T][n_mel].
// sol (optional; svc_diffsvc_sample_steps, which validates it): the solver loop over sol->ts instead, K = ts[0] + 1;
// mode, interval and noise are not used then.
struct SolverSteps {
  const int32_t* ts;  // host, strictly decreasing, in [0, steps)
  int n, order;
};

// The DPM-Solver++(2M) coefficients of the step t -> s < t (DpmArgs a, b; w0, w1 with the previous step's h_prev), in
// f64 from the f32 alphas_cumprod table widened exactly, each rounded once: lambda = ln(ac / (1 - ac)) / 2,
// h = lambda_s - lambda_t, a = sigma_s / sigma_t, b = -alpha_s expm1(-h), w1 = -h / (2 h_prev), w0 = 1 - w1.
static double dpm_step_coeffs(const std::vector<float>& ac, int t, int s, double h_prev, DpmArgs& p) {
  const double at = ac[t], as = ac[s];
  const double h = 0.5 * log(as / (1.0 - as)) - 0.5 * log(at / (1.0 - at));
  p.a = (float)sqrt((1.0 - as) / (1.0 - at));
  p.b = (float)(-sqrt(as) * expm1(-h));
  const double w1 = h_prev > 0.0 ? -h / (2.0 * h_prev) : 0.0;
  p.w1 = (float)w1;
  p.w0 = (float)(1.0 - w1);
  return h;
}

static int sample_impl(svc_ctx* c, const float* cond, int B, int T, const int* tv, int mode, int interval, int K,
                       const float* x_T, const float* mel_src, const float* noise, uint64_t seed,
                       const int32_t* utt_ids, float* x0, hipStream_t stream, const SolverSteps* sol = nullptr) {
  SVC_REQUIRE(c->has_mapper, "mapper weights not loaded");
  SVC_REQUIRE(K >= 1 && K <= c->steps, "sample: k_step %d outside [1, %d]", K, c->steps);
  SVC_REQUIRE(sol || mode == SVC_MODE_DDPM || (mode == SVC_MODE_PLMS && interval >= 1), "sample: mode %d interval %d",
              mode, interval);
  SVC_REQUIRE(x_T || utt_ids, "sample: need x_T or utt_ids for device noise");
  // DDPM draws step noise on the device unless `noise` is given; that noise is keyed by utterance id
  SVC_REQUIRE(sol || mode != SVC_MODE_DDPM || noise || utt_ids, "sample: DDPM without `noise` needs utt_ids");
  hipStream_t s = (hipStream_t)stream;
  const int rows = B * T, nm = c->n_mel, ld16 = (int)round_up(nm, 8);
  DenoiseBufs bb;
  f16 *x16, *xp16;
  float *eps, *hist[5], *xp;
  int st = c->ws.plan([&](Arena& ws) {
    layout_denoise(c, ws, B, T, bb);
    x16 = ws.get<f16>((size_t)rows * ld16);
    eps = ws.get<float>((size_t)rows * nm);
    for (int k = 0; k < 5; ++k) hist[k] = ws.get<float>((size_t)rows * nm);
    xp = ws.get<float>((size_t)rows * nm);
    xp16 = ws.get<f16>((size_t)rows * ld16);
  });
  if (st || (st = project_cond(c, cond, B, T, bb, s))) return st;
  float* x = x0;  // the sampler state lives in the output buffer
  SVC_HIP_CHECK(hipMemsetAsync(x16, 0, (size_t)rows * ld16 * sizeof(f16), s));  // zero pad channels
  if (x_T) {
    SVC_HIP_CHECK(hipMemcpyAsync(x, x_T, (size_t)rows * nm * 4, hipMemcpyDeviceToDevice, s));
    if ((st = f32_to_f16(x, nm, x16, ld16, rows, nm, ld16, s, c->bf16))) return st;
  } else if (mel_src) {
    const float ac = c->alphas_cumprod_f32[K - 1];
    QSampleArgs q{};
    q.mel = mel_src;
    q.mn = c->mel_min;
    q.mx = c->mel_max;
    q.noised = 1;
    q.a = sqrtf(ac);
    q.b = sqrtf(1.0f - ac);
    q.seed = seed;
    q.utt_ids = utt_ids;
    q.tv = tv;
    q.x = x;
    q.x16 = x16;
    q.ld16 = ld16;
    q.bf16 = c->bf16;
    if ((st = q_sample(q, B, T, nm, s))) return st;
  } else {
    if ((st = init_noise(x, x16, ld16, B, T, nm, seed, utt_ids, 1.0f / 1.2f, s, c->bf16))) return st;
  }
  SVC_HIP_CHECK(hipMemsetAsync(xp16, 0, (size_t)rows * ld16 * sizeof(f16), s));

  // Utterance-aligned sub-batches on their own streams, issued kernel by kernel in alternation: their
  // launches overlap on the GPU, so one sub-batch's epilogue / prologue phases (HBM-bound, ~40 % of a
  // denoiser GEMM launch at this size) run beside the other's MFMA phases. Utterances are independent,
  // so results are identical to a single stream. Default 2 (round-2 final code, alternating A/B on two boxes:
  // +0.9 % over 3, 4: -15 %; profiles/r02zf_streams_ab.txt); sampler_streams = 1 disables the split.
  SubBatches sb;
  if ((st = sb.fork(c, tuning().sampler_streams, B, s))) return st;
  const int S = sb.n;
  struct Sub {
    int B, b0;
    size_t r0;
  } sub[kMaxSubStreams];
  for (int h = 0; h < S; ++h) {
    sub[h].b0 = sb.b0(h);
    sub[h].B = sb.b0(h + 1) - sub[h].b0;
    sub[h].r0 = (size_t)sub[h].b0 * T;
  }
  auto sub_bufs = [&](const Sub& u) {
    const size_t r = u.r0;
    const int C = c->C;
    return DenoiseBufs{bb.cp16 + r * 2 * C, bb.y16 + r * C, bb.g16 + r * C, bb.s16 + r * 3 * C, bb.u16 + r * 3 * C,
                       bb.lo16 + r * C, bb.cp_ls, bb.g_ls};
  };

  if (sol) {
    // Step j denoises at ts[j] and moves x to level ts[j + 1]: first order at j = 0 (no history yet), 2M from j = 1 when
    // order is 2; the last call returns its data prediction (sigma_next = 0), where the 2M extrapolation has no finite h.
    // One history buffer: D overwrites D_prev in place.
    double h_prev = 0.0;
    for (int j = 0; j < sol->n; ++j) {
      const int t = sol->ts[j];
      const bool last = j + 1 == sol->n;
      DpmArgs p{};
      p.sra = c->sra[t];
      p.srm1 = c->srm1[t];
      p.final_step = last;
      p.ld16 = ld16;
      p.bf16 = c->bf16;
      const bool second = !last && sol->order == 2 && j > 0;
      if (!last) h_prev = dpm_step_coeffs(c->alphas_cumprod_f32, t, sol->ts[j + 1], second ? h_prev : 0.0, p);
      for (int h = 0; h < S; ++h) {
        const Sub& u = sub[h];
        const size_t r = u.r0;
        DpmArgs q = p;
        q.x = x + r * nm;
        q.eps = eps + r * nm;
        q.d_prev = second ? hist[0] + r * nm : nullptr;
        q.d_out = sol->order == 2 && j + 2 < sol->n ? hist[0] + r * nm : nullptr;  // step j + 1 is a 2M step
        q.x16 = last ? nullptr : x16 + r * ld16;
        if ((st = denoise(c, sub_bufs(u), x16 + r * ld16, u.B, T, t, eps + r * nm, sb.stream(h),
                          tv ? tv + u.b0 : nullptr, &q)))
          return st;
      }
    }
    return sb.join();
  }
  if (mode == SVC_MODE_DDPM) {
    for (int i = K - 1; i >= 0; --i) {
      for (int h = 0; h < S; ++h) {
        const Sub& u = sub[h];
        const size_t r = u.r0;
        const hipStream_t us = sb.stream(h);
        if ((st = denoise(c, sub_bufs(u), x16 + r * ld16, u.B, T, i, eps + r * nm, us, tv ? tv + u.b0 : nullptr)))
          return st;
        DdpmArgs a{};
        a.sra = c->sra[i];
        a.srm1 = c->srm1[i];
        a.c1 = c->pc1[i];
        a.c2 = c->pc2[i];
        a.sigma = i > 0 ? expf(0.5f * c->plogvar[i]) : 0.0f;
        a.z = noise ? noise + (size_t)(K - 1 - i) * rows * nm + r * nm : nullptr;
        a.seed = seed;
        a.utt_ids = utt_ids ? utt_ids + u.b0 : nullptr;
        a.step = i;
        a.bf16 = c->bf16;
        if ((st = ddpm_update(x + r * nm, eps + r * nm, x16 + r * ld16, ld16, u.B, T, nm, a, us))) return st;
      }
    }
    return sb.join();
  }
  // PLMS: history ring of 4 epsilons + the first step's predictor buffers (the ring position is shared)
  int nh = 0, head = 0;  // hist slots: newest at hist[(head - 1) mod 5]
  const std::vector<float>& ac = c->alphas_cumprod_f32;
  for (int i = ((K - 1) / interval) * interval; i >= 0; i -= interval) {
    const int tp = i - interval > 0 ? i - interval : 0;
    // get_x_pred coefficients in f32 exactly as the reference's tensor ops (:96-113)
    const float a_t = ac[i], a_prev = ac[tp];
    const float a_t_sq = sqrtf(a_t), a_prev_sq = sqrtf(a_prev);
    const float A = 1.0f / (a_t_sq * (a_t_sq + a_prev_sq));
    const float Bc = 1.0f / (a_t_sq * (sqrtf((1.0f - a_prev) * a_t) + sqrtf((1.0f - a_t) * a_prev)));
    const float d = a_prev - a_t;
    for (int h = 0; h < S; ++h) {
      const Sub& u = sub[h];
      const size_t r = u.r0;
      const hipStream_t us = sb.stream(h);
      const DenoiseBufs ub = sub_bufs(u);
      float* ecur = hist[head] + r * nm;
      PlmsArgs p{};
      p.bf16 = c->bf16;
      p.d = d;
      p.A = A;
      p.Bc = Bc;
      p.xin = x + r * nm;
      p.xout = x + r * nm;
      p.x16 = x16 + r * ld16;
      p.ld16 = ld16;
      auto H = [&](int back) { return hist[((head - back) % 5 + 5) % 5] + r * nm; };
      // each update runs in (or right after) the denoise whose eps it consumes (denoise's plms argument)
      if (nh == 0) {
        PlmsArgs q = p;
        q.e[0] = ecur;
        q.c[0] = 1.0f;
        q.ne = 1;
        q.div = 1.0f;
        q.xout = xp + r * nm;
        q.x16 = xp16 + r * ld16;
        if ((st = denoise(c, ub, x16 + r * ld16, u.B, T, i, ecur, us, tv ? tv + u.b0 : nullptr, &q)))
          return st;
        float* eprev = hist[(head + 1) % 5] + r * nm;
        p.e[0] = ecur;
        p.e[1] = eprev;
        p.c[0] = 1.0f;
        p.c[1] = 1.0f;
        p.ne = 2;
        p.div = 2.0f;
        if ((st = denoise(c, ub, xp16 + r * ld16, u.B, T, tp, eprev, us, tv ? tv + u.b0 : nullptr, &p)))
          return st;
        continue;
      } else if (nh == 1) {
        p.e[0] = ecur;
        p.e[1] = H(1);
        p.c[0] = 3.0f;
        p.c[1] = -1.0f;
        p.ne = 2;
        p.div = 2.0f;
      } else if (nh == 2) {
        p.e[0] = ecur;
        p.e[1] = H(1);
        p.e[2] = H(2);
        p.c[0] = 23.0f;
        p.c[1] = -16.0f;
        p.c[2] = 5.0f;
        p.ne = 3;
        p.div = 12.0f;
      } else {
        p.e[0] = ecur;
        p.e[1] = H(1);
        p.e[2] = H(2);
        p.e[3] = H(3);
        p.c[0] = 55.0f;
        p.c[1] = -59.0f;
        p.c[2] = 37.0f;
        p.c[3] = -9.0f;
        p.ne = 4;
        p.div = 24.0f;
      }
      if ((st = denoise(c, ub, x16 + r * ld16, u.B, T, i, ecur, us, tv ? tv + u.b0 : nullptr, &p)))
        return st;
    }
    head = (head + 1) % 5;
    nh = nh < 4 ? nh + 1 : 4;
  }
  return sb.join();
}

extern "C" {

svc_status svc_diffsvc_eps(svc_ctx* c, const float* cond, const float* x, int B, int T, const int32_t* frames, int t,
                           float* eps, void* stream) {
  CTX_READY(c);
  SVC_REQUIRE(c->has_mapper, "mapper weights not loaded");
  SVC_REQUIRE(t >= 0 && t < c->steps, "eps: t=%d", t);
  hipStream_t s = (hipStream_t)stream;
  const int* tv;
  RingRetire retire_(c->lens_main, s);
  if (int st0 = stage_frames(c->lens_main, frames, B, T, s, &tv)) return st0;
  const int rows = B * T, ld16 = (int)round_up(c->n_mel, 8);
  DenoiseBufs bb;
  f16* x16;
  int st = c->ws.plan([&](Arena& ws) {
    layout_denoise(c, ws, B, T, bb);
    x16 = ws.get<f16>((size_t)rows * ld16);
  });
  if (st || (st = project_cond(c, cond, B, T, bb, s))) return st;
  if ((st = f32_to_f16(x, c->n_mel, x16, ld16, rows, c->n_mel, ld16, s, c->bf16))) return st;
  if ((st = denoise(c, bb, x16, B, T, t, eps, s, tv))) return st;
  return tv ? zero_tail_rows(eps, B, T, c->n_mel, tv, s) : SVC_OK;
}

svc_status svc_diffsvc_sample(svc_ctx* c, const float* cond, int B, int T, const int32_t* frames, int mode,
                              int interval, const float* x_T, const float* noise, uint64_t seed,
                              const int32_t* utt_ids, float* x0, void* stream) {
  CTX_READY(c);
  hipStream_t s = (hipStream_t)stream;
  const int* tv;
  RingRetire retire_(c->lens_main, s);
  int st = stage_frames(c->lens_main, frames, B, T, s, &tv);
  if (st ||
      (st = sample_impl(c, cond, B, T, tv, mode, interval, c->steps, x_T, nullptr, noise, seed, utt_ids, x0, s)))
    return st;
  // frames past an utterance's end hold no sample: zero them
  return tv ? zero_tail_rows(x0, B, T, c->n_mel, tv, s) : SVC_OK;
}

svc_status svc_diffsvc_sample_from(svc_ctx* c, const float* cond, int B, int T, const int32_t* frames, int mode,
                                   int interval, int k_step, const float* mel_src, const float* x_start,
                                   const float* noise, uint64_t seed, const int32_t* utt_ids, float* x0,
                                   void* stream) {
  CTX_READY(c);
  SVC_REQUIRE((mel_src != nullptr) != (x_start != nullptr), "sample_from: give exactly one of mel_src and x_start");
  SVC_REQUIRE(!mel_src || utt_ids, "sample_from: mel_src draws the forward noise on the device and needs utt_ids");
  hipStream_t s = (hipStream_t)stream;
  const int* tv;
  RingRetire retire_(c->lens_main, s);
  int st = stage_frames(c->lens_main, frames, B, T, s, &tv);
  if (st ||
      (st = sample_impl(c, cond, B, T, tv, mode, interval, k_step, x_start, mel_src, noise, seed, utt_ids, x0, s)))
    return st;
  return tv ? zero_tail_rows(x0, B, T, c->n_mel, tv, s) : SVC_OK;
}

svc_status svc_diffsvc_sample_steps(svc_ctx* c, const float* cond, int B, int T, const int32_t* frames,
                                    const int32_t* timesteps, int n_steps, int order, const float* mel_src,
                                    const float* x_start, uint64_t seed, const int32_t* utt_ids, float* x0,
                                    void* stream) {
  CTX_READY(c);
  SVC_REQUIRE(c->has_mapper, "mapper weights not loaded");
  SVC_REQUIRE(timesteps && n_steps >= 1, "sample_steps: empty timestep list");
  SVC_REQUIRE(order == 1 || order == 2, "sample_steps: order %d (1: DDIM, 2: DPM-Solver++(2M))", order);
  for (int j = 0; j < n_steps; ++j) {
    SVC_REQUIRE(timesteps[j] >= 0 && timesteps[j] < c->steps, "sample_steps: timesteps[%d] = %d outside [0, %d)", j,
                timesteps[j], c->steps);
    SVC_REQUIRE(j == 0 || timesteps[j] < timesteps[j - 1], "sample_steps: timesteps not strictly decreasing at %d", j);
  }
  SVC_REQUIRE(!(mel_src && x_start), "sample_steps: give at most one of mel_src and x_start");
  SVC_REQUIRE(x_start || utt_ids, "sample_steps: the device draw (x_start NULL) needs utt_ids");
  hipStream_t s = (hipStream_t)stream;
  const int* tv;
  RingRetire retire_(c->lens_main, s);
  const SolverSteps sol{timesteps, n_steps, order};
  int st = stage_frames(c->lens_main, frames, B, T, s, &tv);
  if (st || (st = sample_impl(c, cond, B, T, tv, SVC_MODE_PLMS, 1, timesteps[0] + 1, x_start, mel_src, nullptr, seed,
                              utt_ids, x0, s, &sol)))
    return st;
  return tv ? zero_tail_rows(x0, B, T, c->n_mel, tv, s) : SVC_OK;
}

// normalize_mel_channel (utils/acoustic_feature_extraction.py:75-80) with the context's statistics
svc_status svc_mel_normalize(svc_ctx* c, const float* mel, int B, int T, const int32_t* frames, float* x_norm,
                             void* stream) {
  CTX_READY(c);
  SVC_REQUIRE(c->mel_min && c->mel_max, "mel_normalize: mel statistics (stats.mel_min / stats.mel_max) not loaded");
  SVC_REQUIRE(mel && x_norm && B > 0 && T > 0 && (int64_t)B * T * c->n_mel <= INT32_MAX, "mel_normalize: bad args");
  hipStream_t s = (hipStream_t)stream;
  const int* tv;
  RingRetire retire_(c->lens_main, s);
  if (int st = stage_frames(c->lens_main, frames, B, T, s, &tv)) return st;
  QSampleArgs q{};
  q.mel = mel;
  q.mn = c->mel_min;
  q.mx = c->mel_max;
  q.tv = tv;
  q.x = x_norm;
  return q_sample(q, B, T, c->n_mel, s);
}

}  // extern "C"
