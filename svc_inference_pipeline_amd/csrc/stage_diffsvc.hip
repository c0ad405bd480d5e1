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

// The sampler update that denoise launches on its eps: the PLMS one (run_plms), the DPM-Solver one (run_solver), or
// none (svc_diffsvc_eps; run_ddpm, whose update also draws and is launched by the loop itself).
struct EpsUpdate {
  const PlmsArgs* plms = nullptr;
  const DpmArgs* dpm = nullptr;
  EpsUpdate(const PlmsArgs* p = nullptr) : plms(p) {}
  EpsUpdate(const DpmArgs* d) : dpm(d) {}
};

// eps = model(x16, t) for B utterances of T frames with the buffers bb, on s (the sampler: SamplerRun::denoise)
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

// An entry point's work on a ragged batch: stage `frames`, run body(tv), and zero out's rows past each utterance's end,
// which hold no result. The staged table is retired on every return path.
template <class Body>
static int with_frames(svc_ctx* c, const int32_t* frames, int B, int T, float* out, hipStream_t s, Body&& body) {
  const int* tv;
  RingRetire retire_(c->lens_main, s);
  int st = stage_frames(c->lens_main, frames, B, T, s, &tv);
  if (st || (st = body(tv))) return st;
  return tv ? zero_tail_rows(out, B, T, c->n_mel, tv, s) : SVC_OK;
}

// ---------------------------------------------------------------------------- samplers
// An entry point fills a SampleRequest; sample_impl validates it, plans the workspace and projects the conditioner
// (SamplerRun), sets the start state (set_start) and runs the request's step loop (run_ddpm, run_plms, run_solver).
enum SamplerKind { SAMPLER_DDPM, SAMPLER_PLMS, SAMPLER_SOLVER };
struct SampleRequest {
  // start: noise level K - 1, K in 1..steps (K = steps is the whole schedule, svc_diffsvc_sample). DDPM starts at step
  // K - 1, PLMS at ((K - 1) / interval) * interval with an empty history, the solver at ts[0] = K - 1. The state is
  // x_T when given, else mel_src normalised and noised forward to level K - 1 (q_sample), else the x_T draw.
  int K;
  const float *x_T, *mel_src;
  uint64_t seed;  // noise keys of whatever is drawn on the device
  const int32_t* utt_ids;
  SamplerKind kind;    // sampler: the kind, then each kind's own arguments
  int mode, interval;  // DDPM / PLMS: the caller's SVC_MODE_* word, which sample_impl validates, and PLMS's interval
  const float* noise;  // DDPM, optional: [K][B*T][n_mel], else drawn on the device
  const int32_t* ts;   // solver: n_ts host timesteps, strictly decreasing, in [0, steps); order 1 (DDIM) or 2 (2M)
  int n_ts, order;     // (svc_diffsvc_sample_steps validates them)
  // sample_impl rejects a mode that is neither
  static SamplerKind of_mode(int mode) { return mode == SVC_MODE_DDPM ? SAMPLER_DDPM : SAMPLER_PLMS; }
};

// What every step loop needs of one sampler call: the shapes, the workspace and the walk over the sub-batches.
struct SamplerRun {
  svc_ctx* c;
  int B, T;
  const int* tv;
  int rows, nm, ld16;  // B * T, n_mel, the row length of x16 / xp16 (n_mel rounded up to 8; the pad channels stay zero)
  float *x, *eps, *hist[5], *xp;  // x: the sampler state, which lives in the output buffer
  DenoiseBufs bb;
  f16 *x16, *xp16;
  SubBatches sb;  // sub-batch h: utterances sb.b0(h) .. sb.b0(h + 1) - 1 on sb.stream(h)

  // One layout for every sampler: DDPM uses no hist, xp or xp16 and the solver only hist[0], but these gets, their
  // sizes and their order are what svc_ctx_memory's workspace figure and the arena's sizing pass see. Shrinking the
  // layout per sampler is a behaviour change for another day.
  int plan() {
    return c->ws.plan([&](Arena& ws) {
      layout_denoise(c, ws, B, T, bb);
      x16 = ws.get<f16>((size_t)rows * ld16);
      eps = ws.get<float>((size_t)rows * nm);
      for (int k = 0; k < 5; ++k) hist[k] = ws.get<float>((size_t)rows * nm);
      xp = ws.get<float>((size_t)rows * nm);
      xp16 = ws.get<f16>((size_t)rows * ld16);
    });
  }
  // sub-batch h's rows of a whole-batch [rows][nm] f32 or [rows][ld16] 16-bit buffer
  template <class F>
  F* rowsf(F* p, int h) const { return p + (size_t)sb.b0(h) * T * nm; }
  f16* rows16(f16* p, int h) const { return p + (size_t)sb.b0(h) * T * ld16; }
  // the denoiser on sub-batch h and its stream: eps_out = model(x16_in, t), both whole-batch buffers, then the update
  int denoise(int h, f16* x16_in, int t, float* eps_out, EpsUpdate up = {}) {
    const size_t r = (size_t)sb.b0(h) * T, C = c->C;
    const DenoiseBufs ub{bb.cp16 + r * 2 * C, bb.y16 + r * C, bb.g16 + r * C, bb.s16 + r * 3 * C, bb.u16 + r * 3 * C,
                         bb.lo16 + r * C, bb.cp_ls, bb.g_ls};
    return ::denoise(c, ub, rows16(x16_in, h), sb.b0(h + 1) - sb.b0(h), T, t, rowsf(eps_out, h), sb.stream(h),
                     tv ? tv + sb.b0(h) : nullptr, up);
  }
};

// The start state into x and its 16-bit copy x16, with the pad channels of x16 and xp16 zeroed around it
static int set_start(SamplerRun& r, const SampleRequest& q, hipStream_t s) {
  SVC_HIP_CHECK(hipMemsetAsync(r.x16, 0, (size_t)r.rows * r.ld16 * sizeof(f16), s));  // zero pad channels
  if (q.x_T) {
    SVC_HIP_CHECK(hipMemcpyAsync(r.x, q.x_T, (size_t)r.rows * r.nm * 4, hipMemcpyDeviceToDevice, s));
    if (int st = f32_to_f16(r.x, r.nm, r.x16, r.ld16, r.rows, r.nm, r.ld16, s, r.c->bf16)) return st;
  } else if (q.mel_src) {
    const float ac = r.c->alphas_cumprod_f32[q.K - 1];
    QSampleArgs a{};
    a.mel = q.mel_src;
    a.mn = r.c->mel_min;
    a.mx = r.c->mel_max;
    a.noised = 1;
    a.a = sqrtf(ac);
    a.b = sqrtf(1.0f - ac);
    a.seed = q.seed;
    a.utt_ids = q.utt_ids;
    a.tv = r.tv;
    a.x = r.x;
    a.x16 = r.x16;
    a.ld16 = r.ld16;
    a.bf16 = r.c->bf16;
    if (int st = q_sample(a, r.B, r.T, r.nm, s)) return st;
  } else if (int st = init_noise(r.x, r.x16, r.ld16, r.B, r.T, r.nm, q.seed, q.utt_ids, 1.0f / 1.2f, s, r.c->bf16)) {
    return st;
  }
  SVC_HIP_CHECK(hipMemsetAsync(r.xp16, 0, (size_t)r.rows * r.ld16 * sizeof(f16), s));
  return SVC_OK;
}

// steps K - 1 .. 0; the update draws its z on the device, keyed by seed, utterance id and step, unless `noise` holds it
static int run_ddpm(SamplerRun& r, int K, const float* noise, uint64_t seed, const int32_t* utt_ids) {
  svc_ctx* c = r.c;
  for (int i = K - 1; i >= 0; --i) {
    DdpmArgs a{};
    a.sra = c->sra[i];
    a.srm1 = c->srm1[i];
    a.c1 = c->pc1[i];
    a.c2 = c->pc2[i];
    a.sigma = i > 0 ? expf(0.5f * c->plogvar[i]) : 0.0f;
    a.seed = seed;
    a.step = i;
    a.bf16 = c->bf16;
    for (int h = 0; h < r.sb.n; ++h) {
      if (int st = r.denoise(h, r.x16, i, r.eps)) return st;
      a.z = noise ? r.rowsf(noise + (size_t)(K - 1 - i) * r.rows * r.nm, h) : nullptr;
      a.utt_ids = utt_ids ? utt_ids + r.sb.b0(h) : nullptr;
      if (int st = ddpm_update(r.rowsf(r.x, h), r.rowsf(r.eps, h), r.rows16(r.x16, h), r.ld16,
                               r.sb.b0(h + 1) - r.sb.b0(h), r.T, r.nm, a, r.sb.stream(h)))
        return st;
    }
  }
  return SVC_OK;
}

// The five PLMS combinations e' = (sum_j c[j] e_j) / div (modules/diffsvcrepo_inference.py:117-147): the first step's
// predictor and corrector, then Adams-Bashforth of order 2, 3, 4 over the current eps and 1, 2, 3 earlier ones
struct PlmsCoeffs {
  int ne;
  float div, c[4];
};
static constexpr PlmsCoeffs kPlmsCoeffs[5] = {
    {1, 1.0f, {1.0f}}, {2, 2.0f, {1.0f, 1.0f}}, {2, 2.0f, {3.0f, -1.0f}}, {3, 12.0f, {23.0f, -16.0f, 5.0f}},
    {4, 24.0f, {55.0f, -59.0f, 37.0f, -9.0f}}};

// steps i = ((K - 1) / interval) * interval, ..., 0 from an empty history
static int run_plms(SamplerRun& r, int K, int interval) {
  const std::vector<float>& ac = r.c->alphas_cumprod_f32;
  // the ring of epsilons, shared by the sub-batches: slot 0 takes this step's, slot k holds the one k <= nh steps back
  int nh = 0, head = 0, st;
  auto slot = [&](int back) { return r.hist[((head - back) % 5 + 5) % 5]; };
  // sub-batch h's update of x, or with pred into xp / xp16, by a row of the table over the slots 0, dir, 2 dir, ...
  auto update = [&](PlmsArgs p, const PlmsCoeffs& k, int h, int dir, bool pred) {
    p.xin = r.rowsf(r.x, h);
    p.xout = r.rowsf(pred ? r.xp : r.x, h);
    p.x16 = r.rows16(pred ? r.xp16 : r.x16, h);
    p.ne = k.ne;
    p.div = k.div;
    for (int j = 0; j < k.ne; ++j) {
      p.e[j] = r.rowsf(slot(j * dir), h);
      p.c[j] = k.c[j];
    }
    return p;
  };
  for (int i = ((K - 1) / interval) * interval; i >= 0; i -= interval) {
    const int tp = i - interval > 0 ? i - interval : 0;
    // get_x_pred coefficients in f32 exactly as the reference's tensor ops (:96-113)
    const float a_t = ac[i], a_prev = ac[tp];
    const float a_t_sq = sqrtf(a_t), a_prev_sq = sqrtf(a_prev);
    PlmsArgs step{};
    step.A = 1.0f / (a_t_sq * (a_t_sq + a_prev_sq));
    step.Bc = 1.0f / (a_t_sq * (sqrtf((1.0f - a_prev) * a_t) + sqrtf((1.0f - a_t) * a_prev)));
    step.d = a_prev - a_t;
    step.ld16 = r.ld16;
    step.bf16 = r.c->bf16;
    for (int h = 0; h < r.sb.n; ++h) {
      if (nh == 0) {
        // No history: a predictor from eps(x, i) into xp / xp16, then x's update with the average of that eps and
        // eps(xp, tp), which borrows the next slot (-1). Both calls are enqueued before the next sub-batch's.
        const PlmsArgs q = update(step, kPlmsCoeffs[0], h, -1, true), p = update(step, kPlmsCoeffs[1], h, -1, false);
        if ((st = r.denoise(h, r.x16, i, slot(0), &q))) return st;
        st = r.denoise(h, r.xp16, tp, slot(-1), &p);
      } else {
        const PlmsArgs p = update(step, kPlmsCoeffs[1 + (nh < 3 ? nh : 3)], h, 1, false);
        st = r.denoise(h, r.x16, i, slot(0), &p);
      }
      if (st) return st;
    }
    head = (head + 1) % 5;
    nh = nh < 4 ? nh + 1 : 4;
  }
  return SVC_OK;
}

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

// Step j denoises at ts[j] and moves x to level ts[j + 1]: first order at j = 0 (no history yet), 2M from j = 1 when
// order is 2; the last call returns its data prediction (sigma_next = 0), where the 2M extrapolation has no finite h.
// One history buffer: D overwrites D_prev in place.
static int run_solver(SamplerRun& r, const int32_t* ts, int n, int order) {
  double h_prev = 0.0;
  for (int j = 0; j < n; ++j) {
    const int t = ts[j];
    const bool last = j + 1 == n;
    DpmArgs p{};
    p.sra = r.c->sra[t];
    p.srm1 = r.c->srm1[t];
    p.final_step = last;
    p.ld16 = r.ld16;
    p.bf16 = r.c->bf16;
    const bool second = !last && order == 2 && j > 0;
    if (!last) h_prev = dpm_step_coeffs(r.c->alphas_cumprod_f32, t, ts[j + 1], second ? h_prev : 0.0, p);
    for (int h = 0; h < r.sb.n; ++h) {
      p.x = r.rowsf(r.x, h);
      p.eps = r.rowsf(r.eps, h);
      p.d_prev = second ? r.rowsf(r.hist[0], h) : nullptr;
      p.d_out = order == 2 && j + 2 < n ? r.rowsf(r.hist[0], h) : nullptr;  // step j + 1 is a 2M step
      p.x16 = last ? nullptr : r.rows16(r.x16, h);
      if (int st = r.denoise(h, r.x16, t, r.eps, &p)) return st;
    }
  }
  return SVC_OK;
}

static int sample_impl(svc_ctx* c, const float* cond, int B, int T, const int* tv, const SampleRequest& q, float* x0,
                       hipStream_t s) {
  const bool sol = q.kind == SAMPLER_SOLVER;
  SVC_REQUIRE(c->has_mapper, "mapper weights not loaded");
  SVC_REQUIRE(q.K >= 1 && q.K <= c->steps, "sample: k_step %d outside [1, %d]", q.K, c->steps);
  SVC_REQUIRE(sol || q.mode == SVC_MODE_DDPM || (q.mode == SVC_MODE_PLMS && q.interval >= 1),
              "sample: mode %d interval %d", q.mode, q.interval);
  SVC_REQUIRE(q.x_T || q.utt_ids, "sample: need x_T or utt_ids for device noise");
  // DDPM draws step noise on the device unless `noise` is given; that noise is keyed by utterance id
  SVC_REQUIRE(sol || q.mode != SVC_MODE_DDPM || q.noise || q.utt_ids, "sample: DDPM without `noise` needs utt_ids");
  SamplerRun r{c, B, T, tv, B * T, c->n_mel, (int)round_up(c->n_mel, 8), x0};
  int st = r.plan();
  if (st || (st = project_cond(c, cond, B, T, r.bb, s)) || (st = set_start(r, q, s))) return st;
  // Utterance-aligned sub-batches on their own streams, issued kernel by kernel in alternation: their launches overlap
  // on the GPU, so one sub-batch's epilogue / prologue phases (HBM-bound, ~40 % of a denoiser GEMM launch at this size)
  // run beside the other's MFMA phases (profiles/r02zf_streams_ab.txt: 2 streams +0.9 % over 3, 4: -15 %). Utterances
  // are independent, so results are identical to a single stream; sampler_streams = 1 disables the split. Every loop
  // visits the sub-batches in order within a step: the enqueue order decides what runs beside what.
  if ((st = r.sb.fork(c, tuning().sampler_streams, B, s))) return st;
  switch (q.kind) {
    case SAMPLER_DDPM: st = run_ddpm(r, q.K, q.noise, q.seed, q.utt_ids); break;
    case SAMPLER_PLMS: st = run_plms(r, q.K, q.interval); break;
    case SAMPLER_SOLVER: st = run_solver(r, q.ts, q.n_ts, q.order); break;
  }
  return st ? st : r.sb.join();
}

static int sample_entry(svc_ctx* c, const float* cond, int B, int T, const int32_t* frames, const SampleRequest& q,
                        float* x0, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  return with_frames(c, frames, B, T, x0, s, [&](const int* tv) { return sample_impl(c, cond, B, T, tv, q, x0, s); });
}

extern "C" {

svc_status svc_diffsvc_eps(svc_ctx* c, const float* cond, const float* x, int B, int T, const int32_t* frames, int t,
                           float* eps, void* stream) {
  CTX_READY(c);
  SVC_REQUIRE(c->has_mapper, "mapper weights not loaded");
  SVC_REQUIRE(t >= 0 && t < c->steps, "eps: t=%d", t);
  hipStream_t s = (hipStream_t)stream;
  return with_frames(c, frames, B, T, eps, s, [&](const int* tv) {
    const int rows = B * T, ld16 = (int)round_up(c->n_mel, 8);
    DenoiseBufs bb;
    f16* x16;
    int st = c->ws.plan([&](Arena& ws) {
      layout_denoise(c, ws, B, T, bb);
      x16 = ws.get<f16>((size_t)rows * ld16);
    });
    if (st || (st = project_cond(c, cond, B, T, bb, s))) return st;
    if ((st = f32_to_f16(x, c->n_mel, x16, ld16, rows, c->n_mel, ld16, s, c->bf16))) return st;
    return denoise(c, bb, x16, B, T, t, eps, s, tv);
  });
}

svc_status svc_diffsvc_sample(svc_ctx* c, const float* cond, int B, int T, const int32_t* frames, int mode,
                              int interval, const float* x_T, const float* noise, uint64_t seed,
                              const int32_t* utt_ids, float* x0, void* stream) {
  CTX_READY(c);
  const SampleRequest q{c->steps, x_T, nullptr, seed, utt_ids, SampleRequest::of_mode(mode), mode, interval, noise};
  return sample_entry(c, cond, B, T, frames, q, x0, stream);
}

svc_status svc_diffsvc_sample_from(svc_ctx* c, const float* cond, int B, int T, const int32_t* frames, int mode,
                                   int interval, int k_step, const float* mel_src, const float* x_start,
                                   const float* noise, uint64_t seed, const int32_t* utt_ids, float* x0,
                                   void* stream) {
  CTX_READY(c);
  SVC_REQUIRE((mel_src != nullptr) != (x_start != nullptr), "sample_from: give exactly one of mel_src and x_start");
  SVC_REQUIRE(!mel_src || utt_ids, "sample_from: mel_src draws the forward noise on the device and needs utt_ids");
  const SampleRequest q{k_step, x_start, mel_src, seed, utt_ids, SampleRequest::of_mode(mode), mode, interval, noise};
  return sample_entry(c, cond, B, T, frames, q, x0, stream);
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
  const SampleRequest q{timesteps[0] + 1, x_start, mel_src, seed, utt_ids, SAMPLER_SOLVER,
                        /* no mode, interval, noise */ 0, 0, nullptr, timesteps, n_steps, order};
  return sample_entry(c, cond, B, T, frames, q, x0, stream);
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

