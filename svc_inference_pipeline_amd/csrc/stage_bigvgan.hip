// The BigVGAN vocoder stage.
#include "engine.h"

extern "C" {

// ---------------------------------------------------------------------------- BigVGAN
svc_status svc_bigvgan(svc_ctx* c, const float* x0, int B, int T, const int32_t* frames, float* wav, float* mel_out,
                       void* stream) {
  CTX_READY(c);
  SVC_REQUIRE(c->has_vocoder && c->mel_min && c->mel_max, "vocoder (and mapper stats) not loaded");
  hipStream_t s = (hipStream_t)stream;
  // ragged batches: utterance b has frames[b] mel frames; at a point where the signal is `mul` times the mel rate
  // its valid length is tv[b] * mul, and every conv / activation / the fade-out ends there
  const int* tv;
  RingRetire retire_(c->lens_main, s);
  if (int st0 = stage_frames(c->lens_main, frames, B, T, s, &tv)) return st0;
  for (int b = 0; frames && b < B; ++b)
    SVC_REQUIRE(frames[b] * c->hop_out >= c->nfade, "bigvgan: utterance %d (%d frames) shorter than the fade-out", b,
                frames[b]);
  const int nm = c->v_in, ldm = (int)round_up(nm, 8);
  int maxLC = 0, Lr = T;  // max over stages of L_i*C_i / T  (6144 for the reference config)
  for (auto& S : c->vstages) {
    Lr *= S.rate;
    maxLC = std::max(maxLC, (Lr / T) * S.cout);
  }
  // the activation kernels address one utterance's f32 stage buffer through 32-bit buffer offsets: T * maxLC * 4 bytes
  // must stay below 2 GiB (87 381 frames = 15.5 min of 24 kHz audio for the reference config); longer utterances are
  // rejected here rather than silently wrapped
  SVC_REQUIRE((int64_t)T * maxLC * 4 < ((int64_t)1 << 31),
              "bigvgan: T=%d frames per utterance exceeds the vocoder's limit of %lld frames (2 GiB stage span)", T,
              (long long)((((int64_t)1 << 31) - 1) / ((int64_t)maxLC * 4)));
  SVC_REQUIRE(T * c->hop_out >= c->nfade, "bigvgan: T=%d shorter than the fade-out", T);
  const size_t big = (size_t)B * T * maxLC;
  f16 *mel16, *pre16, *a16, *next16;
  float *X, *Xj, *tmp, *XS;
  int st = c->ws.plan([&](Arena& ws) {
    mel16 = ws.get<f16>((size_t)B * T * ldm);
    pre16 = ws.get<f16>((size_t)B * T * c->v_c0);
    X = ws.get<float>(big);
    Xj = ws.get<float>(big);
    tmp = ws.get<float>(big);
    XS = ws.get<float>(big);
    a16 = ws.get<f16>(big);
    next16 = ws.get<f16>(big);
  });
  if (st) return st;
  // amp_maxc: widest channel count that takes the fused kernel (0: activation1d + GEMM everywhere). C = 48 unfused is
  // 9 % slower (its N = 48 GEMMs are too narrow for the MFMA tiles); C = 96 fused is 1.0 ms per step faster than
  // activation1d + amp_conv's plain conv since both run on 256-row tiles of 2 x 2 waves (round 6; on the round-5 128-row
  // tiles, where every wave read all of W per k-loop, fused C = 96 had been 1 % slower end to end)
  const int amp_maxc = tuning().amp_maxc;
  const int ns = (int)c->vstages.size();

  // Utterance-aligned sub-batches on their own streams (as in svc_diffsvc_sample): every buffer is
  // time-major per utterance, so a sub-batch is a row offset into each; launches alternate between streams.
  // Default 1: its launches are long (0.3-2 ms) and measured no faster split (vocoder_streams = 2 / 3).
  SubBatches sb;
  if ((st = sb.fork(c, tuning().vocoder_streams, B, s))) return st;
  const int NS = sb.n;
  for (int h = 0; h < NS; ++h) {  // de-normalise + conv_pre
    const int Bh = sb.b0(h + 1) - sb.b0(h);
    const size_t r = (size_t)sb.b0(h) * T;
    if ((st = denorm_mel(x0 + r * nm, mel16 + r * ldm, mel_out ? mel_out + r * nm : nullptr, ldm, Bh * T, nm,
                         c->mel_min, c->mel_max, sb.stream(h))))
      return st;
    EpiArgs e = epi();
    e.out16 = pre16 + r * c->v_c0;
    e.ld16 = c->v_c0;
    if ((st = run_gemm(c->vpre, mel16 + r * ldm, ldm, nm, Bh, T, T, e, sb.stream(h), "bigvgan.conv_pre",
                       tv ? tv + sb.b0(h) : nullptr, 1)))
      return st;
  }
  int L = T;
  int mul = 1;  // samples of the current stage per mel frame
  for (int i = 0; i < ns; ++i) {
    VStage& S = c->vstages[i];
    const int Lin = L;
    const int mul_in = mul;
    L = Lin * S.rate;
    mul = mul_in * S.rate;
    const int ch = S.cout;
    for (int h = 0; h < NS; ++h) {
      const int Bh = sb.b0(h + 1) - sb.b0(h);
      const hipStream_t sh = sb.stream(h);
      const int* tvh = tv ? tv + sb.b0(h) : nullptr;
      // each sub-batch owns the fixed region [b0 * T * maxLC, b1 * T * maxLC) of every stage buffer for all
      // stages (offsets that moved with L * C would let a lagging stream's reads overlap another's writes)
      const size_t ro = (size_t)sb.b0(h) * T * maxLC;
      float *Xh = X + ro, *Xjh = Xj + ro, *tmph = tmp + ro, *XSh = XS + ro;
      f16* a16h = a16 + ro;
      const f16* in16 = i == 0 ? pre16 + (size_t)sb.b0(h) * T * c->v_c0 : next16 + ro;
      f16* next16h = next16 + ro;
      // ConvTranspose1d as `rate` phase GEMMs writing rows t*rate + r, or (rate 2, tune.amp_ups) as one conv
      if (S.up_comb && tuning().amp_ups) {
        AmpConvArgs q{nullptr, Bh, Lin, 3, -1, nullptr, nullptr, nullptr, S.upc.W, S.upc.Kpad, S.upc.bias};
        q.x16 = in16;
        q.noact = true;
        q.tv = tvh;
        q.tv_mul = mul_in;
        EpiArgs u = epi();
        u.out32 = Xh;
        u.ld32 = S.cin;
        prof_site("bigvgan.ups");
        if ((st = amp_conv(q, S.cin, u, sh))) return st;
      } else
      for (int r = 0; r < S.rate; ++r) {
        EpiArgs u = epi();
        u.T_ostore = L;
        u.ostride = S.rate;
        u.ophase = r;
        u.out32 = Xh;
        u.ld32 = ch;
        if ((st = run_gemm(S.phases[r], in16, S.cin, S.cin, Bh, Lin, Lin, u, sh, "bigvgan.ups", tvh, mul_in))) return st;
      }
      const int nk = (int)S.c1.size();
      for (int j = 0; j < nk; ++j) {
        const int nd = (int)S.c1[j].size();
        for (int l = 0; l < nd; ++l) {
          // AMPBlock2 reads its activation halo from the x it updates, so its x ping-pongs between Xj and tmp
          // (AMPBlock1 updates x in place: its second activation reads tmp)
          const float* src = (l == 0) ? Xh : ((c->v_rb2 && l % 2 == 0) ? tmph : Xjh);
          float* xnext = (c->v_rb2 && l % 2 == 1) ? tmph : Xjh;
          const ActP& a1 = S.acts[j][2 * l];
          const ActP& a2 = S.acts[j][2 * l + 1];
          // AMPBlock1: tmp = c1(a1(x)), x' = x + c2(a2(tmp)); AMPBlock2: x' = x + c(a(x)) with c = c2[l] (dilation d)
          const bool rb2 = c->v_rb2;
          const int d2 = rb2 ? S.rd[j][l] : 1;
          // AMPBlock1's intermediate c1(a1(x)) is stored f16 (tmp16, in tmp's memory): it is read once, by a2, whose
          // output is rounded to the f16 MFMA operand anyway; 4 B less per element read and written (round 3)
          f16* tmp16 = reinterpret_cast<f16*>(tmph);
          const float* act_in = rb2 ? src : nullptr;  // input of the activation before the second (or only) conv
          const f16* act_in16 = rb2 ? nullptr : tmp16;
          // small channel counts: SnakeBeta fused into the conv (amp_conv.hip); otherwise activation1d + GEMM
          const bool fuse = ch <= amp_maxc && amp_conv_supported(ch, S.rk[j], S.rd[j][l]);
          if (!rb2) {
            EpiArgs e1 = epi();
            e1.out16 = tmp16;
            e1.ld16 = ch;
            if (fuse) {
              const PackedGemm& g1 = S.c1[j][l];
              AmpConvArgs p1{src, Bh, L, S.rk[j], S.rd[j][l], a1.alpha, a1.beta, a1.filt, g1.W, g1.Kpad, g1.bias};
              p1.tv = tvh;
              p1.tv_mul = mul;
              prof_site("bigvgan.amp_c1");
              if ((st = amp_conv(p1, ch, e1, sh))) return st;
            } else {
              if ((st = activation1d(src, a16h, Bh, L, ch, ch, a1.alpha, a1.beta, a1.filt, sh, tvh, mul))) return st;
              if ((st = run_gemm(S.c1[j][l], a16h, ch, ch, Bh, L, L, e1, sh, "bigvgan.amp_c1", tvh, mul))) return st;
            }
          }
          if (!fuse &&
              (st = activation1d(act_in, a16h, Bh, L, ch, ch, a2.alpha, a2.beta, a2.filt, sh, tvh, mul, act_in16)))
            return st;
          EpiArgs e2 = epi();
          e2.add_row = src;
          e2.ld_add_row = ch;
          if (l + 1 < nd) {
            e2.out32 = xnext;
            e2.ld32 = ch;
          } else if (j == 0) {
            e2.out32 = XSh;
            e2.ld32 = ch;
          } else {
            e2.acc32 = XSh;
            e2.ld_acc = ch;
            if (j + 1 == nk) {
              e2.acc_div = (float)nk;
              if (i + 1 < ns) {
                e2.out16 = next16h;
                e2.ld16 = ch;
              } else {
                e2.out32 = XSh;
                e2.ld32 = ch;
              }
            } else {
              e2.out32 = XSh;
              e2.ld32 = ch;
            }
          }
          if (fuse) {
            const PackedGemm& g2 = S.c2[j][l];
            AmpConvArgs p2{act_in, Bh, L, S.rk[j], d2, a2.alpha, a2.beta, a2.filt, g2.W, g2.Kpad, g2.bias};
            p2.tv = tvh;
            p2.tv_mul = mul;
            p2.x16 = act_in16;
            prof_site("bigvgan.amp_c2");
            if ((st = amp_conv(p2, ch, e2, sh))) return st;
          } else if ((st = run_gemm(S.c2[j][l], a16h, ch, ch, Bh, L, L, e2, sh, "bigvgan.amp_c2", tvh, mul))) {
            return st;
          }
        }
      }
      // the stage output next16 feeds the next ConvTranspose; it is rewritten only after that ran (same stream)
    }
  }
  const int chl = c->vstages.back().cout;
  for (int h = 0; h < NS; ++h) {
    const int Bh = sb.b0(h + 1) - sb.b0(h);
    const size_t ro = (size_t)sb.b0(h) * T * maxLC;
    const int* tvh = tv ? tv + sb.b0(h) : nullptr;
    if ((st = activation1d(XS + ro, a16 + ro, Bh, L, chl, chl, c->vact_post.alpha, c->vact_post.beta,
                           c->vact_post.filt, sb.stream(h), tvh, mul)))
      return st;
    if ((st = conv_post(a16 + ro, chl, Bh, L, chl, c->vpost_w, c->vpost_b, c->fade, c->nfade,
                        wav + (size_t)sb.b0(h) * L, sb.stream(h), tvh, mul)))
      return st;
  }
  if ((st = sb.join())) return st;
  return (tv && mel_out) ? zero_tail_rows(mel_out, B, T, nm, tv, s) : SVC_OK;
}

}  // extern "C"
