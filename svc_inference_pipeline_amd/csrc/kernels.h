// The host launchers of the kernel files (and the few host helpers beside them) for their callers: engine.hip, the
// stage_*.hip files, finalize.hip and ops.hip. A launcher is declared here and nowhere else, and the file that
// defines it includes this header too: default arguments live here only, the argument structs exist once, and a
// definition that drifts from its declaration is a redefined default or an ambiguous call where it is compiled.
#pragma once
#include "common.h"
#include "amp_conv.h"
#include "arena.h"
#include "spectral.h"

namespace svc {

int attention(const f16* qkv, f16* out, int B, int L, int D, hipStream_t s, bool bf16, const int* lens = nullptr);
int layernorm_f16(const float* x, const float* g, const float* b, f16* y, int rows, int D, int ldy, hipStream_t s,
                  bool bf);
int layernorm_f32(const float* x, const float* g, const float* b, float* y, int rows, int D, int ldy, hipStream_t s);
int activation1d(const float* x, f16* y, int B, int L, int C, int ldy, const float* alpha_log, const float* beta_log,
                 const float* filt, hipStream_t s, const int* tv = nullptr, int tv_mul = 1, const f16* x16 = nullptr);
int f32_to_f16(const float* x, int ldx, f16* y, int ldy, int rows, int C, int Cpad, hipStream_t s, bool bf);
int denorm_mel(const float* x, f16* y, float* y32, int ldy, int rows, int C, const float* mn, const float* mx,
               hipStream_t s);
int content_map(const float* src, int B, int src_rows, int ld_src, int T, int D, f16* dst, int ld_dst, hipStream_t s,
                bool bf);
int bucketize(const double* f0, const float* en, const float* mbins, const float* ebins, int nb, int* im, int* ie,
              int n, hipStream_t s);
int plms_update(const PlmsArgs& p, int rows, int C, hipStream_t s);
int dpm_update(const DpmArgs& p, int rows, int C, hipStream_t s);
int ddpm_update(float* x, const float* eps, f16* x16, int ld16, int B, int T, int C, const DdpmArgs& a, hipStream_t s);
int init_noise(float* x, f16* x16, int ld16, int B, int T, int C, uint64_t seed, const int* utt_ids, float std,
               hipStream_t s, bool bf);
int q_sample(const QSampleArgs& q, int B, int T, int C, hipStream_t s);
int conv_post(const f16* a, int lda, int B, int L, int C, const float* w, float bias, const float* fade, int nfade,
              float* out, hipStream_t s, const int* tv = nullptr, int tv_mul = 1);
int zero_tail_rows(float* x, int B, int T, int C, const int* Tb, hipStream_t s);
int whisper_normalize(const float* logspec, float* mx_scratch, f16* out, int B, int64_t n_per_utt, hipStream_t s,
                      int split_c, bool bf, int ldo);
int layernorm_f16x3(const float* x, const float* g, const float* b, f16* y, int rows, int D, hipStream_t s, bool bf);
int f32_to_f16x3_grouped(const float* x, f16* y, int rows, int C, int Cg, hipStream_t s, bool bf);
int f16_to_f32(const f16* x, float* y, int64_t n, hipStream_t s);
int f32_to_f16x3(const float* x, int ldx, f16* y, int rows, int C, hipStream_t s, bool bf);
int conv_gemm3(const ConvGemmArgs& a, const EpiArgs& e, const f16* zpage, int variant, hipStream_t s);
int conv_gemm4(const ConvGemmArgs& a, const EpiArgs& e, const f16* zpage, hipStream_t s, bool direct_gate);
bool gate_ws_fits(const ConvGemmArgs& a, const EpiArgs& e);
extern unsigned long long* gate_ws_stamps;
int gate_ws_nstamp();
int gate_ws(const ConvGemmArgs& a, const EpiArgs& e, hipStream_t s);
int gate_ws_pack(const f16* W, int ldw, f16* Wf, hipStream_t s);
size_t gate_ws_pack_elems();
int res_proj(const f16* g, const f16* Wf, const float* bias, const float* sub, const float* add, float div, f16* hi,
             f16* lo, int M, bool bf16, int lanes_cap, bool store_lo, hipStream_t s);
extern unsigned long long* res_proj_stamps;
int res_proj_nstamp();
int res_proj_pack(const f16* W, int ldw, f16* Wf, hipStream_t s);
size_t res_proj_pack_elems();
int mel_proj(const f16* x, int ldx, const f16* Wf, const float* bias, const float* add, f16* hi, f16* lo, int M,
             bool bf16, hipStream_t s);
int mel_proj_pack(const f16* W, int ldw, f16* Wf, hipStream_t s);
size_t mel_proj_pack_elems();
int diff_head(const f16* s16, const f16* Wsp, const float* bsp, int Nsp, int Ksp, const f16* Wout, const float* bout,
              int Nout, int Kout, int Npad_out, float* eps, int ld_eps, int M, const f16* zpage, hipStream_t s,
              bool bf16);
int pitch_shift(double* f0, int B, int T, double target, hipStream_t s);
// target, scale: device f64 [B] (scale NULL: none)
int pitch_shift_ex(double* f0, int B, int T, const double* target, const double* scale, hipStream_t s);
// the factor pitch_shift_ex multiplies row b by, f0 only read. target, scale as above; factor: device f64 [B]
int pitch_factor(const double* f0, int B, int T, const double* target, const double* scale, double* factor,
                 hipStream_t s);
// the pooled voiced median (median.h). frames_dev: device int32 [B] or NULL; median: device f64 [1]; voiced: device
// int64 [1] or NULL
int f0_voiced_median(const double* f0, int B, int T, const int* frames_dev, double* median, long long* voiced,
                     Arena& ws, hipStream_t s);
int content_map_hubert(const float* src, int B, int src_rows, int ld_src, int T, int D, f16* dst, int ld_dst,
                       hipStream_t s, bool bf);
int content_map_ragged(const float* src, int B, int src_rows, int ld_src, int T, int D, f16* dst, int ld_dst,
                       const int* tab, hipStream_t s, bool bf);
int content_map_windows(const float* src, int B, int win_rows, int ld_src, int T, int D, f16* dst, int ld_dst,
                        const int* tab, hipStream_t s, bool bf);
int zero_tail_rows16(f16* x, int B, int T, int ld, const int* Tb, int max_tail, hipStream_t s);
int hubert_frames5(const float* wav, int B, int64_t n, f16* out, bool split, hipStream_t s, bool bf,
                   const int64_t* nb = nullptr);
int groupnorm_gelu(const float* x, int B, int T, int C, const float* gamma, const float* beta, double* part,
                   int max_chunks, float2* ss, f16* y, bool split, hipStream_t s, bool bf, const int* Tb = nullptr,
                   int nck_max = 0);
int layernorm_dual(const float* x, const float* g, const float* b, float* y32, f16* y16, int rows, int D, bool split,
                   hipStream_t s, bool bf);
int pack_qkv(const float* q, const float* k, const float* v, f16* qkv, int64_t rows, int D, float scale, hipStream_t s);
int f0_praat_ac(const float* wav, int B, int64_t n_samples, double fs, double time_step, double floor_hz,
                double ceiling_hz, double voicing, int T, double* f0_out, Arena& ws, const double* tables,
                hipStream_t s, const int64_t* n_b = nullptr, const int* T_b = nullptr, StageRing* ring = nullptr);
size_t f0_table_doubles(double fs, double floor_hz);
int f0_tables(double fs, double floor_hz, double* out);
size_t pyin_table_doubles(double sr, double fmin, double fmax, int frame_length, int win_length, int hop);
int pyin_tables(double sr, double fmin, double fmax, int frame_length, int win_length, int hop, double* out);
int f0_pyin(const float* wav, int B, int64_t ld, const int64_t* nvalid_dev, const int64_t* nvalid_host, double sr,
            double fmin, double fmax, int frame_length, int win_length, int hop, int F, double* f0, Arena& ws,
            const double* tables_dev, hipStream_t s);
size_t pcm16_table_bytes(int B);
int pcm16(const float* wav, int B, int64_t S, void* table, int64_t max_nb, int sil, int64_t L, int turn_up,
          double volume_peak, int16_t* pcm, float* peak_out, int need_peak, hipStream_t s);
size_t loudness_lens_bytes(int B);
size_t loudness_power_bytes(int B, int64_t K_max);
int loudness_match(const float* wav, const float* src, int B, int64_t S, int64_t S_src, void* table, int64_t K_max,
                   int window, int hop, double mix, double floor_rms, double max_gain, float* out, double* gain_out,
                   int64_t K_out, hipStream_t s);
// stitch.hip: the host half of svc_stitch (checks, the staged table, two launches)
int stitch(StageRing* ring, const int* device, const float* const* rows, int B, const int64_t* n, const int64_t* lead,
           const int64_t* body, const int32_t* joined, const int64_t* out_off, int xfade, int search, double eps,
           float* out, int64_t out_len, int32_t* shift_out, double* q_out, hipStream_t s);
// retrieve.hip: feature retrieval. table (device): int32 frames[B], then int32 sel[B]
int index_norms(const f16* x, int64_t N, int D, int ld, float* norms, hipStream_t s);
int retrieve_splits(int M, int64_t N);
int knn_topk(const f16* q, int M, int T, int D, int ld, const int* table, int B, const f16* x, const float* norms, int N,
             int ld_index, int n_splits, float* cand_s, int* cand_j, hipStream_t s);
int content_retrieve(const f16* q, int B, int T, int D, int ld, const int* table, const f16* x, const float* norms,
                     int N, int ld_index, int k, double rate, double dist_floor, f16* out, int ld_out, int* idx_out,
                     float* dist_out, Arena& ws, hipStream_t s);
// index_kmeans.hip: a retrieval index compacted by Lloyd's iteration (svc_index_assign / _update / _kmeans). Every
// function lays its scratch out on the arena it is given (one plan per call)
int index_assign(const f16* x, int64_t N, int D, int ld, const f16* cent, const float* cnorms, int K, int ld_cent,
                 int* labels, int* counts, double* inertia, Arena& ws, hipStream_t s);
int index_update(const f16* x, int64_t N, int D, int ld, const int* labels, int K, const f16* prev, int ld_prev, f16* out,
                 int ld_out, float* norms_out, int* counts, Arena& ws, hipStream_t s);
int index_kmeans(const f16* x, int64_t N, int D, int ld, int K, int iters, f16* cent, int ld_cent, float* cnorms,
                 int* labels, int* counts, double* inertia, Arena& ws, hipStream_t s);
int load_pcm(StageRing* ring, const int* device, const void* raw, int B, const int64_t* byte_off, const int64_t* n_frames,
             const int32_t* format, const int32_t* channels, const int32_t* sr_in, int sr_src, int64_t S_src,
             float* y_src, int sr_mono, int64_t S_mono, float* y_mono, float* y_mono_float, bool ex, int32_t* info,
             hipStream_t s);
// resample.hip: the cached plan of a rate pair (design_plan's integers) and its taps once more in phase-major order on
// the device, hpm[k0 * per_phase + r] = h[k0 + up * r] (per_phase = (taps - 1) / up + 1); 0, or -1 when the upload failed
int get_plan_pm(int sr_in, int sr_out, const double** hpm, int* up, int* down, int* pre_remove, int* taps,
                int* per_phase);

}  // namespace svc
