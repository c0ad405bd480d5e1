/*
 * svc_hip.h — C-ABI of libsvc_hip.so, the MI355X (gfx950) singing-voice-conversion hot path.
 *
 * The reference (WallaceRao/svc_inference_pipeline) has no FFI: its boundary is the set of Python
 * functions infer.py calls. Each entry point below replaces one of them (file:line in the reference):
 *
 *   svc_mel_energy      <- utils/mel.py:179-201 extract_mel_features (mel_spectrogram :130-174, energy :199)
 *   svc_f0_ac           <- utils/f0.py:120-161 get_f0_features_using_parselmouth (Praat to_pitch_ac + pad)
 *   svc_pitch_shift     <- utils/acoustic_feature_extraction.py:48-52 pitch_shift
 *   svc_pitch_shift_ex  <- the same with a target median (and an optional key scale) per utterance
 *   svc_pitch_factor    <- the factor svc_pitch_shift / svc_pitch_shift_ex multiply by, stored instead of applied
 *   svc_f0_voiced_median <- utils/acoustic_feature_extraction.py:21-30 get_target_f0_median (a singer's pooled contours)
 *   svc_mel_keyshift    <- Diff-SVC's key-shifted mel (utils/mel.py:43-117 get_mel(keyshift=), with the hop held): the
 *                          start mel of shallow diffusion moved by the pitch factor
 *   svc_whisper_encode  <- utils/whisper.py:13-28 whisper_encoder (log_mel_spectrogram + AudioEncoder)
 *   svc_map_content     <- utils/whisper.py:31-81 get_mapped_whisper_features
 *   svc_whisper_content_ragged <- utils/whisper.py:13-81, both of the above for a ragged batch: every 30 s window that
 *                          exists encoded once in one pass, one mapping launch (svc_whisper_windows: a clip's windows)
 *   svc_hubert_encode   <- utils/hubert.py:31-47 get_hubert_content (svc_hubert_encode_ragged: a ragged batch in one pass)
 *   svc_map_content_ragged <- utils/hubert.py:83-134 get_mapped_features / utils/whisper.py:31-81, per utterance
 *   svc_condition       <- modules/encoder.py:165-201 EncoderFramework.forward
 *   svc_diffsvc_sample  <- modules/diffsvcrepo_inference.py:154-240 svc_model_inference (DDPM or PLMS)
 *   svc_diffsvc_sample_from <- the same from noise level k_step - 1 (Diff-SVC's shallow diffusion)
 *   svc_diffsvc_sample_steps <- DPM-Solver++(2M) / DDIM over a list of timesteps (not in the reference)
 *   svc_mel_normalize   <- utils/acoustic_feature_extraction.py:75-80 normalize_mel_channel
 *   svc_bigvgan         <- utils/acoustic_feature_extraction.py:83-97 denormalize_mel_channel
 *                          + modules/bigvgan_inference.py:29-44 synthesis_audios (Generator + trim + fade)
 *   svc_load_pcm        <- utils/audio.py:10-55 load_audio_torch + utils/whisper_extractor/audio.py:22-49 load_audio
 *                          (sample decode, normalisation, mono mix and both resamplings of a ragged batch of wav
 *                          payloads; the RIFF header is parsed on the host)
 *   svc_load_pcm_ex     <- the same, plus utils/hubert.py:137-143 librosa.load(path, sr=16000): the float 16 kHz mono
 *                          rows HuBERT / ContentVec reads, from the launch that writes Whisper's rows
 *   svc_pcm16           <- utils/util.py:20-37 save_audio (peak normalisation, silence, 16-bit samples; the file
 *                          itself is written on the host)
 *   svc_loudness_match  <- no counterpart in the reference: so-vits-svc's loudness envelope adjustment, between
 *                          svc_bigvgan and svc_pcm16 (the output takes the source's slow RMS envelope)
 *   svc_stitch          <- no counterpart in the reference: so-vits-svc's --clip crossfade with RVC's SOLA alignment,
 *                          between svc_bigvgan and svc_loudness_match (overlapping chunks of a long clip, converted
 *                          as separate utterances, joined into one waveform)
 *   svc_content_retrieve <- no counterpart in the reference: RVC's feature index (index_rate), between the content
 *                          stage and svc_condition (each content frame blended with its k nearest frames of the
 *                          target singer's own recordings; svc_index_norms prepares an index)
 *   svc_index_kmeans    <- no counterpart in the reference: RVC's k-means compaction of a large feature index, at
 *                          enrolment (the searched rows become centroids of all of a singer's frames;
 *                          svc_index_assign and svc_index_update are its two steps)
 *
 * Conventions
 *   - Tensors are caller-owned DEVICE buffers, time-major: row = b*T + t, channels contiguous.
 *   - Every call is asynchronous and ordered on `stream` (a hipStream_t; NULL = default stream).
 *   - One context per device; a context is not thread-safe. Calls that share the context's workspace must be
 *     ordered on one stream; svc_mel_energy, svc_f0_ac and svc_pitch_shift are the exception (their own workspace /
 *     none) and may run, ordered among themselves, on a second stream beside the content encoders (the host
 *     pipeline overlaps them with Whisper that way, on svc_ctx_stream(ctx, 2)).
 *   - Parameters are given in the reference's own state_dict naming with a model prefix
 *     ("mapper.", "vocoder.", "whisper.") as host float32 arrays; they are folded (weight_norm),
 *     packed into MFMA layouts and uploaded by svc_ctx_finalize. Host arrays must stay valid until
 *     svc_ctx_finalize returns. A missing or mis-shaped parameter makes finalize fail (the reference
 *     silently keeps random init, utils/load_models.py:34-43).
 *   - Status codes instead of exceptions; svc_last_error() describes the last failure of this thread.
 *   - Ragged batches: a batch holds B utterances of different lengths padded to the longest (rows keep the batch
 *     stride). The per-utterance lengths are HOST arrays — n_samples (int64 [B], samples) for the 24 kHz feature
 *     stages, frames (int32 [B], mel frames) for the sampler and the vocoder; NULL means every utterance has the
 *     batch length. Each utterance is then computed exactly as a clip of its own length (its own reflect / zero /
 *     replicate padding, STFT frames, Praat frame grid, fade-out): outputs are bit-identical to converting it alone,
 *     and the rows past its end are written as zeros. svc_whisper_encode needs no lengths: pad its 16 kHz input with
 *     zeros (as pad_or_trim does). A ragged Whisper batch as a whole goes through svc_whisper_content_ragged, which
 *     takes utt_samples (int64 [B], 16 kHz samples) and frames (int32 [B], mel frames): clips of one 30 s window and
 *     clips of several windows share ONE encoder pass over exactly the windows that exist, each window framed in place
 *     from the padded batch (samples past an utterance's own count are never read), and one mapping launch writes
 *     every utterance's frames. HuBERT / ContentVec needs lengths too (its GroupNorm normalises over time, its positional
 *     convolution reads past the end and its attention looks at every key): svc_hubert_encode_ragged takes
 *     utt_samples (int64 [B], 16 kHz samples) and svc_map_content_ragged takes each utterance's source rows and mel
 *     frames (int32 [B] each), so a ragged ContentVec batch is one encoder pass and one mapping launch. The tables
 *     are staged to the device through a ring of 8 slots per stage group; a slot is reused only after every kernel of
 *     the call that read it has finished (its event is re-recorded on the call's stream after the call's last
 *     launch), so calls may use any streams.
 */
#ifndef SVC_HIP_H
#define SVC_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svc_ctx svc_ctx;
typedef int svc_status; /* 0 = ok, 1 = invalid argument, 2 = HIP error, 3 = bad state */

#define SVC_MODE_DDPM 0
#define SVC_MODE_PLMS 1

const char* svc_last_error(void);
int svc_abi_version(void);

svc_status svc_ctx_create(int device, svc_ctx** out);
svc_status svc_ctx_destroy(svc_ctx* ctx);
/* numeric configuration (config.json keys, flattened: "fs", "mapper.residual_layer_num", "vocoder.upsample_rates.0",
   ...; and the precision keys "content.split", "content.wsplit_attn" / _mlp / _qk / _v / _out, "mapper.head_split",
   "operands.bf16" (1: the content encoders, conditioner and DiffSVC GEMMs take bfloat16 operands on
   v_mfma_f32_16x16x32_bf16, and content features cross svc_map_content* / svc_condition as bfloat16; BigVGAN stays
   fp16), "hubert.output_layer"). An unknown key is SVC_ERR_INVALID (a misspelt key must not leave a default in place).
   "tune.<name>" keys set a kernel switch of this context at any time (gemm_variant, gemm3_direct, whisper_streams,
   sampler_streams, vocoder_streams, diff_head, amp_maxc, amp_ups, res_proj, gate_ws; "tune.reset" restores the creation-time values). Defaults
   are the measured production kernels; at creation an SVC_<NAME> environment variable overrides each. ctx may be
   NULL for "tune.*" keys: the switches of the op-level entry points (svc_op_*, svc_gemm_bench).
   "tune.retrieve_splits" is set the same way. It selects no kernel: it is the number of index splits of
   svc_content_retrieve's grid (0, the default: chosen from the call's shape), on which the result does not depend. */
svc_status svc_ctx_set_config(svc_ctx* ctx, const char* key, double value);
/* the value of a configuration key set on this context, or of a kernel switch ("tune.<name>"; ctx NULL: the
   op-level context's); a key that was never set is SVC_ERR_INVALID */
svc_status svc_ctx_get_config(svc_ctx* ctx, const char* key, double* value);
/* host-only: 1 when `key` is a configuration key svc_ctx_set_config accepts (not "tune.*"), else 0 */
int svc_config_key_known(const char* key);
svc_status svc_ctx_add_param(svc_ctx* ctx, const char* name, const float* host, int ndim, const int64_t* shape);
svc_status svc_ctx_finalize(svc_ctx* ctx);
/* bytes of device memory held by packed weights / by the workspace arena. The arena only grows, and each stage call
   sizes it by counting its own buffers: workspace_bytes is exactly what the largest stage call so far needed, with no
   slack (the feature stages' own workspace, svc_f0_ac / svc_f0_pyin, is not included). */
svc_status svc_ctx_memory(svc_ctx* ctx, int64_t* weight_bytes, int64_t* workspace_bytes);
/* the context's sub-stream `index` (< 8; created on first use, owned by the context): lets a caller overlap
   svc_f0_ac with the content encoder without creating a stream of its own */
svc_status svc_ctx_stream(svc_ctx* ctx, int index, void** stream);

/* A2/A3-energy: wav24k [B][n_samples] f32 -> mel [B*T][n_mels] f32 (log-mel, time-major), energy [B*T] f32.
   T = (n_samples + n_fft - hop - n_fft)/hop + 1 (bit-exact frame count, utils/mel.py:148-167).
   utt_samples (host int64 [B] or NULL): ragged batch, utterance b's samples (<= n_samples); its T_b frames as above. */
svc_status svc_mel_energy(svc_ctx* ctx, const float* wav24k, int B, int64_t n_samples, const int64_t* utt_samples,
                          float* mel, float* energy, void* stream);

/* A3-F0: Praat autocorrelation pitch (to_pitch_ac, voicing 0.6, floor f0_min, ceiling f0_max, time step hop/fs),
   padded to T frames as utils/f0.py:156-157; unvoiced = 0. f0 [B*T] float64. Uses the feature-stage workspace
   (shared with svc_mel_energy only): may run on another stream beside the content-encoder calls. */
svc_status svc_f0_ac(svc_ctx* ctx, const float* wav24k, int B, int64_t n_samples, const int64_t* utt_samples, int T,
                     double* f0, void* stream);

/* F4: pYIN F0, utils/f0.py:95-117 get_f0_features_using_pyin(audio, fs, win_length, hop_length,
   f0_min, f0_max) = librosa.pyin with its defaults (frame_length 2048, centred frames, 100 beta(2, 18) thresholds,
   0.1-semitone bins, Viterbi decoding) and the unvoiced frames set to 0. wav [B][n_samples] f32 -> f0 [B*T] float64,
   utterance b's frames 1 + utt_samples[b] / hop_length, the rest of its T rows 0 (T >= 1 + n_samples / hop_length
   when every utterance is full length). Uses the feature-stage workspace, like svc_f0_ac; the context need not be
   finalized. Parity is unpinned (librosa is absent here): tests/test_f0.py holds it to oracle/pyin.py, which restates
   librosa 0.10.1 (its parabolic-interpolation shift and pyin's pad_mode="constant" default; librosa 0.9 / 0.10.0
   compute the parabolic shift differently, and the reference pins no librosa version). The device tables are built
   once per (fs, f0_min, f0_max, win_length, hop_length) and kept in the context. */
svc_status svc_f0_pyin(svc_ctx* ctx, const float* wav, int B, int64_t n_samples, const int64_t* utt_samples, double fs,
                       int win_length, int hop_length, double f0_min, double f0_max, int T, double* f0, void* stream);

/* A4: in place, f0 [B*T] float64 *= target_median / median(voiced f0 of that utterance)
   (utils/acoustic_feature_extraction.py:33-52; np.median semantics, NaN when no frame is voiced). */
svc_status svc_pitch_shift(svc_ctx* ctx, double* f0, int B, int T, double target_median, void* stream);

/* A4 with a target per utterance. Row b: f0[b, :] *= target_median[b] / median(voiced f0[b, :]), then * scale[b] where
   scale is given: factor = target_median[b] / med; factor = factor * scale[b]; f0 *= factor, in that order (f64).
   target_median, scale: HOST f64 [B] (scale NULL = none); each must be finite and > 0 (checked before any device call,
   SVC_ERR_INVALID otherwise). With scale NULL and equal targets the result is bit-identical to svc_pitch_shift. The
   tables are staged through the feature stages' ring, like the ragged-batch lengths. */
svc_status svc_pitch_shift_ex(svc_ctx* ctx, double* f0, int B, int T, const double* target_median,
                              const double* scale, void* stream);

/* A4's factor without the shift: factor[b] = target_median[b] / median(voiced f0[b, :]), then * scale[b] where scale is
   given: svc_pitch_shift_ex's select and operations in its order (with scale NULL and equal targets svc_pitch_shift's),
   so f0 * factor in f64 is bit for bit what those calls write. f0 [B*T] f64 is only read; factor: DEVICE f64 [B],
   stream-ordered, NaN for a row with no voiced frame. target_median, scale: HOST f64 [B] (scale NULL = none), finite
   and > 0 (checked before any device call, SVC_ERR_INVALID otherwise), staged like svc_pitch_shift_ex's. One
   workgroup per row. */
svc_status svc_pitch_factor(svc_ctx* ctx, const double* f0, int B, int T, const double* target_median,
                            const double* scale, double* factor, void* stream);

/* The key-shifted log-mel: svc_mel_energy's mel of a voice whose pitch is moved by factor[b], from the unmoved audio.
   wav24k [B][n_samples] f32, factor DEVICE f64 [B] (svc_pitch_factor's) -> mel [B*T][n_mels] f32; T, utt_samples and
   each utterance's T_b as in svc_mel_energy; no energy. Utterance b, with n = n_fft:
     n_new   = rint(n * factor[b]) (f64 product, half to even), clamped to [n / 2, 2 n]; a factor that is not finite or
               <= 0 is taken as 1 (n_new = n). info (DEVICE int32 [B] or NULL): bit 0 such a factor, bit 1 the clamp
               acted, else 0. All on the device: nothing is read back, and a bad factor does not stop the batch.
     window  w[j] = (float)(0.5 - 0.5 cos(2 pi j / n_new)) (f64, periodic Hann), the multiply x * w[j] in f32.
     frame t reads samples t * hop + j - (n_new - hop) / 2, j < n_new: the hop is held, so the frame count is the
               unshifted one. One reflection at either end against the utterance's own length; samples at or past it
               are never read.
     X[k]    = sum_j xw[j] e^(-2 pi i k j / n_new), k = 0 .. min(n / 2, n_new / 2), in f64 (a direct DFT with exact
               integer phases); |X| = sqrtf(re^2 + im^2 + 1e-9f) on the f32 casts, then * (float)n / (float)n_new (two f32
               operations, in that order) where n_new != n. Bins k > n_new / 2 (a downward shift) are exactly 0.
     mel     = the context's slaney filterbank and logf(fmaxf(., 1e-5f)), svc_mel_energy's f32 sequence.
   Rows t >= T_b are zeros. SVC_ERR_INVALID before any device call: a null pointer, B < 1, n_fft other than 512 or 1024
   (or hop > n_fft / 2), a context without a mel filterbank, or an utterance of (2 n - hop + 1) / 2 samples or fewer
   (the widest window's reflection must stay inside the clip). Uses the feature stages' length ring and no workspace:
   may run beside the content encoder like svc_mel_energy. */
svc_status svc_mel_keyshift(svc_ctx* ctx, const float* wav24k, int B, int64_t n_samples, const int64_t* utt_samples,
                            const double* factor, float* mel, int32_t* info, void* stream);

/* A4, the target side: np.median of every f0[b, t] != 0 with t < frames[b] (frames: host int32 [B], NULL = all T),
   pooled over the batch: utils/acoustic_feature_extraction.py:21-30. median: device f64 [1] (NaN where nothing is
   voiced, as np.median of an empty selection); voiced: device int64 [1] or NULL, the pooled voiced count.
   Stream-ordered, no host sync: a radix select in 8-bit digits on one workgroup per 2048 cells, 10 stream operations
   per call whatever the size, integer atomics only (the same bits on every run). Requires B > 0, T > 0,
   B * T < 2^31 and 0 <= frames[b] <= T (checked before any device call). f0 is raw extractor output and is taken to
   be NaN-free: a NaN cell counts as voiced and sorts by its bit pattern (past +inf or before -inf), not as np.median
   would propagate it. Uses the feature-stage workspace, like svc_f0_ac; the context need not be finalized. */
svc_status svc_f0_voiced_median(svc_ctx* ctx, const double* f0, int B, int T, const int32_t* frames, double* median,
                                int64_t* voiced, void* stream);

/* A5+A6: wav16k [B][n_samples] f32 (int16-quantised, <= 480000 samples; zero-padded to 30 s)
   -> Whisper encoder output feats [B*n_ctx][n_state] f32.
   Non-finite input: the attention kernel is compiled with -fno-honor-nans (its softmax max tree skips NaN
   canonicalisation), so a NaN reaching q / k / v gives undefined feats (possibly finite) instead of a propagated
   NaN. The log-mel front end and LayerNorm keep finite audio finite; a NaN / inf sample in wav16k is the caller's
   error. The same holds for svc_hubert_encode and svc_op_attention. */
svc_status svc_whisper_encode(svc_ctx* ctx, const float* wav16k, int B, int64_t n_samples, float* feats, void* stream);

/* A7: feats [B*src_rows][D] f32 -> content [B*T][D] f16 (IEEE binary16 bits), 15:8 repeat/average. T <= 2812. */
svc_status svc_map_content(svc_ctx* ctx, const float* feats, int B, int src_rows, int T, int D, void* content_f16,
                           void* stream);

/* A7/A8 mapping with an output row stride: feats [B*src_rows][D] f32 -> out f16 [B*T] rows of ld_out halves
   (columns 0..D-1 written; pass a column-offset pointer to fill one content type of a concatenated buffer).
   mode 0: Whisper rule (utils/whisper.py:31-81, T <= 2812, source truncated to T*8/15+1 rows);
   mode 1: HuBERT rule (utils/hubert.py:83-134, all src_rows frames, <= 3 missing rows repeat the last mapped
   row; |T - src_rows*15/8| > 3 is SVC_ERR_INVALID where the reference calls exit()). */
svc_status svc_map_content_ex(svc_ctx* ctx, const float* feats, int B, int src_rows, int T, int D, int mode,
                              void* out_f16, int ld_out, void* stream);

/* svc_map_content_ex for a ragged batch: utterance b maps its first utt_src_rows[b] (1..src_rows) rows of feats to
   frames[b] (1..T) rows of out exactly as svc_map_content_ex maps a batch of that shape (mode 1: n_down =
   utt_src_rows[b] * 15 / 8, and |frames[b] - n_down| > 3 is SVC_ERR_INVALID naming the utterance); its rows
   frames[b] .. T-1 are zeros (columns 0..D-1; columns past D are not touched). Both tables are HOST int32 [B],
   checked before any HIP call; NULL = src_rows / T for every utterance (both NULL: svc_map_content_ex). */
svc_status svc_map_content_ragged(svc_ctx* ctx, const float* feats, int B, int src_rows, const int32_t* utt_src_rows,
                                  int T, const int32_t* frames, int D, int mode, void* out_f16, int ld_out,
                                  void* stream);

/* host-only: Whisper windows of a clip of `frames` mel frames: 1 for 1..2812 (the reference's single 30 s window,
   utils/whisper.py:52-56), else ceil(frames / 2805) windows of 478 720 samples (29.92 s = 1496 encoder rows =
   2805 mel frames); -1 for frames < 1 */
int svc_whisper_windows(int frames);

/* A5+A6+A7 for a ragged batch: wav16 f32 [B][n_samples] (int16-quantised 16 kHz), utterance b = its first
   utt_samples[b] samples -> out16 [B*T] rows of ld_out halves (columns 0..D-1; f16, or bf16 with operands.bf16).
   Utterance b has W_b = svc_whisper_windows(frames[b]) windows. A single window reads samples [0, min(utt_samples[b],
   480000)); window w of a longer clip reads [w * 478720, w * 478720 + clamp(utt_samples[b] - w * 478720, 0, 478720));
   the rest of each window's 30 s is zeros (pad_or_trim), a window may hold no samples at all, and samples at or past
   utt_samples[b] are never read. All W = sum W_b windows go through the encoder in ONE pass (log-mel with its
   per-window maximum, conv stem, blocks, ln_post; tune.whisper_streams sub-batches split over windows). One launch
   then maps: row t < frames[b] comes from window (W_b == 1 ? 0 : t / 2805), local row t' = t - 2805 * window, by
   svc_map_content's rule (source rows (8 t' + i) / 15, i = 0..7, summed in that order in f32, / 8); rows frames[b] ..
   T-1 are +0 in columns 0..D-1; columns at or past D of a wider buffer are not touched. Every utterance equals
   svc_whisper_encode + svc_map_content on its own windows bit for bit.
   feats_out: optional device f32 [W][n_ctx][n_state], the encoder output of every window, utterance-major (NULL: it
   stays in the workspace, which is sized for W windows as svc_whisper_encode sizes it for B).
   utt_samples: HOST int64 [B], each 0..n_samples, NULL = n_samples; frames: HOST int32 [B], each 1..T, NULL = T. Both
   are checked before any HIP call: a bad entry is SVC_ERR_INVALID naming the utterance, as are a null pointer, B < 1,
   ld_out < D, missing Whisper weights and a row count beyond int. The window table goes through the main length ring. */
svc_status svc_whisper_content_ragged(svc_ctx* ctx, const float* wav16, int B, int64_t n_samples,
                                      const int64_t* utt_samples, int T, const int32_t* frames,
                                      void* out16, int ld_out, float* feats_out, void* stream);

/* A8 (variant): HuBERT/ContentVec content encoder, replacing utils/hubert.py:31-47 get_hubert_content
   (fairseq HubertModel.extract_features(output_layer = config "hubert.output_layer", default 9) + final_proj).
   wav16k [B][n_samples] f32 (librosa-loaded 16 kHz float audio, utils/hubert.py:55) -> feats
   [B*svc_hubert_frames(n)][final_dim] f32. Parameters are added as "hubert." + fairseq state_dict keys.
   Every utterance has the batch length n: the GroupNorm normalises over all its rows and the attention sees every
   frame, so zero padding is NOT exact here (unlike Whisper); clips of different lengths go through
   svc_hubert_encode_ragged below. */
svc_status svc_hubert_encode(svc_ctx* ctx, const float* wav16k, int B, int64_t n_samples, float* feats, void* stream);
/* The same for a ragged batch (see "Ragged batches"): utterance b is wav16k[b][0 .. utt_samples[b]), the rest of its
   row is never read (it may hold anything). Its svc_hubert_frames(utt_samples[b]) rows of feats are bit-identical to
   svc_hubert_encode on that clip alone: the GroupNorm statistics run over its own conv_layers[0] rows in the chunk
   partition a clip of that length gets, the positional convolution sees zeros past its last frame, and the attention
   stops at its last frame (queries and keys). Its remaining rows of feats (the batch stride stays
   svc_hubert_frames(n_samples)) are zeros. utt_samples: HOST int64 [B], each 400 (one frame) .. n_samples, otherwise
   SVC_ERR_INVALID before any HIP call; NULL = svc_hubert_encode. */
svc_status svc_hubert_encode_ragged(svc_ctx* ctx, const float* wav16k, int B, int64_t n_samples,
                                    const int64_t* utt_samples, float* feats, void* stream);
/* frames of the conv feature extractor for n samples (499 for 160 000) */
int64_t svc_hubert_frames(int64_t n_samples);
svc_status svc_hubert_dims(svc_ctx* ctx, int* final_dim, int* embed_dim);

/* A10: content f16 [B*T][D], f0 f64 [B*T], energy f32 [B*T], singer int32 [B] -> cond f32 [B*T][384].
   With several content types (config mapper.content_feature) D is the sum of their widths and the
   content columns are concatenated in ascending type-name order (e.g. contentvec | whisper); the
   per-type Linear layers (modules/encoder.py:144-148) are summed as one GEMM. */
svc_status svc_condition(svc_ctx* ctx, const void* content_f16, const double* f0, const float* energy,
                         const int32_t* singer, int B, int T, float* cond, void* stream);

/* A10's integer half, exported for bit-exact testing: the melody / loudness embedding indices the conditioner uses,
   torch.bucketize(f0 f64, melody bins f32) and torch.bucketize(energy f32, loudness bins f32) with right=False and
   torch's NaN placement (past the last bin) — modules/encoder.py:47-57,70 and :93-102,115. Bins are the context's
   (checkpoint) bins. f0 [n] f64, energy [n] f32 -> melody_idx, loudness_idx [n] int32 in [0, n_bins - 1]. */
svc_status svc_condition_indices(svc_ctx* ctx, const double* f0, const float* energy, int n, int32_t* melody_idx,
                                 int32_t* loudness_idx, void* stream);

/* A11+A12: cond f32 [B*T][384] -> x_0 f32 [B*T][n_mel] (normalised mel, time-major). frames: see Ragged batches.
   mode SVC_MODE_DDPM: `interval` ignored, 1000 steps; SVC_MODE_PLMS: reference speedup (e.g. 10).
   x_T f32 [B*T][n_mel] or NULL (then drawn on device from `seed` and `utt_ids`).
   noise (DDPM only) f32 [steps][B*T][n_mel] (already in time-major order) or NULL (device Philox noise keyed by
   `seed` and `utt_ids`). utt_ids int32 [B] may be NULL only when nothing is drawn on the device: x_T given and,
   for DDPM, `noise` given; otherwise a NULL utt_ids is SVC_ERR_INVALID. */
svc_status svc_diffsvc_sample(svc_ctx* ctx, const float* cond, int B, int T, const int32_t* frames, int mode,
                              int interval, const float* x_T, const float* noise, uint64_t seed,
                              const int32_t* utt_ids, float* x0, void* stream);

/* single epsilon prediction (DiffSVC.forward, modules/diffsvc.py:284-321) for testing: x f32 [B*T][n_mel], step t */
svc_status svc_diffsvc_eps(svc_ctx* ctx, const float* cond, const float* x, int B, int T, const int32_t* frames, int t,
                           float* eps, void* stream);

/* normalize_mel_channel (utils/acoustic_feature_extraction.py:75-80) with the context's statistics, the inverse of the
   de-normaliser in svc_bigvgan: mel f32 [B*T][n_mel] as svc_mel_energy writes it -> x_norm f32 [B*T][n_mel],
   (mel - mel_min) / (mel_max - mel_min + 1e-12) * 2 - 1 per channel in f32, not clamped. frames: see Ragged batches;
   rows past an utterance's end are zeros. Needs stats.mel_min / stats.mel_max (a context without a mapper may carry
   them alone: svc_mel_normalize + svc_bigvgan is copy-synthesis through the vocoder). */
svc_status svc_mel_normalize(svc_ctx* ctx, const float* mel, int B, int T, const int32_t* frames, float* x_norm,
                             void* stream);

/* Shallow diffusion (Diff-SVC's k_step): svc_diffsvc_sample started at noise level k_step - 1 (1 <= k_step <= steps)
   instead of from pure noise. The start state is exactly one of
     mel_src  f32 [B*T][n_mel], the source clip's un-normalised mel (svc_mel_energy's): normalised as svc_mel_normalize
              does and noised forward, x = sqrt(ac[k-1]) y + sqrt(1 - ac[k-1]) z, z ~ N(0, 1) drawn on the device as
              svc_op_init_noise draws with counter word 1 = 0xFFFFFFFE (utt_ids required);
     x_start  f32 [B*T][n_mel], an already noised state.
   DDPM runs steps k_step - 1 .. 0 (noise, if given, is [k_step][B*T][n_mel], first row for step k_step - 1); PLMS runs
   i = ((k_step - 1) / interval) * interval, ... , 0 with an empty history at its first iteration. k_step = steps with
   x_start = x_T is svc_diffsvc_sample bit for bit. SVC_ERR_INVALID: k_step out of range, both or neither of mel_src /
   x_start, a NULL utt_ids when something is drawn on the device (mel_src; DDPM without noise). */
svc_status svc_diffsvc_sample_from(svc_ctx* ctx, const float* cond, int B, int T, const int32_t* frames, int mode,
                                   int interval, int k_step, const float* mel_src, const float* x_start,
                                   const float* noise, uint64_t seed, const int32_t* utt_ids, float* x0, void* stream);

/* A multistep ODE solver over a caller-given list of timesteps: DPM-Solver++(2M) in the data-prediction form (order 2)
   or its first-order case, DDIM at eta = 0 (order 1). timesteps: HOST int32 [n_steps], strictly decreasing, each in
   [0, steps); the denoiser runs once per entry, so the call costs n_steps denoiser calls. With lambda_t =
   ln(ac_t / (1 - ac_t)) / 2 over the context's f32 alphas_cumprod table and D_t = clip(sqrt(1 / ac_t) x -
   sqrt(1 / ac_t - 1) eps, -1, 1) (the DDPM path's clip_denoised prediction), the step t -> s is
     x_s = sqrt((1 - ac_s) / (1 - ac_t)) x_t - sqrt(ac_s) expm1(-h) Dbar,  h = lambda_s - lambda_t,
   Dbar = D_t at order 1 and at the first step, else (1 + h / (2 h_prev)) D_t - h / (2 h_prev) D_prev; the last entry
   returns x_0 = D_t (first order whatever `order` says). The start state at level timesteps[0] is x_start, or mel_src
   noised forward as in svc_diffsvc_sample_from, or with neither the x_T draw of svc_diffsvc_sample; the last two draw
   on the device and need utt_ids. Nothing is drawn per step. Which timesteps to take is the caller's policy (the
   Python package's config.solver_timesteps spaces them evenly in lambda). SVC_ERR_INVALID: an empty list, one that is
   not strictly decreasing, an entry outside [0, steps), an order other than 1 or 2, both start states, a device draw
   without utt_ids. The sampler stage at B = 32 x 937 frames: PLMS at interval 10 (101 denoiser calls) 198.6 ms; order 2
   over 50 / 20 / 10 log-SNR-spaced steps from noise 97.9 / 40.7 / 21.0 ms, over 20 / 10 from level 299 38.6 / 21.1 ms
   (profiles/dpm_bench.json): time follows the call count. Output quality at a given n_steps has been checked on an
   analytic Gaussian denoiser and on random weights only, no real checkpoint exists here. */
svc_status svc_diffsvc_sample_steps(svc_ctx* ctx, const float* cond, int B, int T, const int32_t* frames,
                                    const int32_t* timesteps, int n_steps, int order, const float* mel_src,
                                    const float* x_start, uint64_t seed, const int32_t* utt_ids, float* x0,
                                    void* stream);

/* A13+A14+A15: x0 f32 [B*T][n_mel] (normalised) -> wav [B][T*256] f32 (denorm, Generator, tanh, fade-out).
   frames (host int32 [B] or NULL): ragged batch, utterance b's waveform is frames[b]*256 samples (fade-out at its end,
   zeros after).
   mel_denorm_out (optional, f32 [B*T][n_mel]) receives the de-normalised mel. */
svc_status svc_bigvgan(svc_ctx* ctx, const float* x0, int B, int T, const int32_t* frames, float* wav,
                       float* mel_denorm_out, void* stream);

/* sample formats of a wav payload (little-endian, channels interleaved): PCM unsigned 8-bit, signed 16 / 24 / 32-bit,
   IEEE float 32 / 64-bit */
#define SVC_PCM_U8 0
#define SVC_PCM_S16 1
#define SVC_PCM_S24 2
#define SVC_PCM_S32 3
#define SVC_PCM_F32 4
#define SVC_PCM_F64 5

/* A1: the input end for a ragged batch of B wav files, replacing utils/audio.py:10-55 load_audio_torch (-> y_src) and
   utils/whisper_extractor/audio.py:22-49 load_audio (-> y_mono) for wav input: at most three launches whatever B is.
   raw: ONE device byte buffer holding the files' data-chunk payloads, utterance b's at raw + byte_off[b] (any byte
   alignment), n_frames[b] frames of channels[b] (1..8) interleaved samples of format[b] (SVC_PCM_*) at sr_in[b] Hz.
   The five tables are HOST arrays [B], staged through a ring of this entry point's own (any stream).
   y_src f32 [B][S_src] (or NULL): row b = channel 0 as float, divided by 1, 2^15 + 1 or 2^31 + 1 by its peak class
   (peak > 1.01, > 2^15; float formats only), resampled to sr_src (rows already at sr_src are not filtered): its first
   svc_resample_len(n_frames[b], sr_in[b], sr_src) samples, zeros after them to S_src.
   y_mono f32 [B][S_mono] (or NULL): row b = the mean over the channels (numpy's summation order, in f64) as float,
   resampled to sr_mono (always through the filter) and rounded to the int16 grid (svc_resample's quantize16), zeros
   after its svc_resample_len(n_frames[b], sr_in[b], sr_mono) samples.
   Each row is bit for bit what audio.load_audio / audio.load_whisper_audio give for that file alone (svc_resample's
   filter, index arithmetic and summation order). An empty utterance gives rows of zeros.
   info int32 [B] (device, or NULL): bits 0-1 the peak class (0, 1, 2), bit 2 set when the source row holds a
   non-finite sample (NaN, Inf, or a finite f64 beyond the f32 range; the mono row is not examined).
   SVC_ERR_INVALID before any HIP call: a null pointer (both outputs NULL included), B < 1, channels outside 1..8, an
   unknown format, a rate < 1, a negative length or offset, S_src / S_mono < 1 or shorter than the longest row, a rate
   ratio whose filter span exceeds the kernel's tile (down / up beyond ~400). The context need not be finalized. */
svc_status svc_load_pcm(svc_ctx* ctx, const void* raw, int B, const int64_t* byte_off, const int64_t* n_frames,
                        const int32_t* format, const int32_t* channels, const int32_t* sr_in, int sr_src,
                        int64_t S_src, float* y_src, int sr_mono, int64_t S_mono, float* y_mono, int32_t* info,
                        void* stream);

/* A1 with HuBERT / ContentVec's input: svc_load_pcm with a third output, the float mono rows that replace
   utils/hubert.py:137-143's librosa.load(path, sr=16000) for wav input. svc_load_pcm is the y_mono_float == NULL case
   (the same results bit for bit, the same launches).
   y_mono_float f32 [B][S_mono] (or NULL): row b = the mean over the channels exactly as y_mono takes it (f64, numpy's
   order) as float; where sr_in[b] != sr_mono, svc_resample's filter output (float)acc WITHOUT the int16 rounding (the
   value y_mono's sample is rounded from); where sr_in[b] == sr_mono, the float means themselves, unfiltered
   (librosa.load does not resample at the native rate; y_mono's row of the same utterance still goes through the
   up = down = 1 filter). Same length as y_mono's row, svc_resample_len(n_frames[b], sr_in[b], sr_mono), zeros after it
   to S_mono. Row b is bit for bit audio.load_contentvec_audio of that file alone. The row is not examined for
   non-finite samples; info is as svc_load_pcm writes it.
   Both mono rows come from ONE launch (one decode of the input into LDS, one pass over the taps, two stores), so a call
   stays at three launches at most (peak, source, mono) whichever rows are asked for. Any of the three outputs may be
   NULL, not all three; a row computed with the others present is bit-identical to the same row computed alone. With
   y_mono_float alone, rows already at sr_mono need no filter plan.
   SVC_ERR_INVALID before any HIP call as svc_load_pcm, with: all three outputs NULL; sr_mono / S_mono < 1 or S_mono
   shorter than the longest mono row when either mono output is given. */
svc_status svc_load_pcm_ex(svc_ctx* ctx, const void* raw, int B, const int64_t* byte_off, const int64_t* n_frames,
                           const int32_t* format, const int32_t* channels, const int32_t* sr_in, int sr_src,
                           int64_t S_src, float* y_src, int sr_mono, int64_t S_mono, float* y_mono,
                           float* y_mono_float, int32_t* info, void* stream);

/* host-only: samples per output row for a batch whose longest utterance has n_samples:
   n_samples + 2 * (add_silence ? fs / 20 : 0); -1 for n_samples < 0 or fs < 1 */
int64_t svc_pcm16_len(int64_t n_samples, int fs, int add_silence);

/* A16: utils/util.py:20-37 save_audio's sample conversion. wav f32 [B][S] -> pcm int16 [B][svc_pcm16_len(S, fs,
   add_silence)]: per utterance, peak = max |x|, x * (float)(volume_peak / peak) when turn_up, fs / 20 zeros before and
   after when add_silence, then clip(round_half_even(x * 32768), -32768, 32767): bit for bit the host path's samples
   (audio.to_pcm16, the project's pinned restatement of the reference function) for finite input.
   utt_samples (host int64 [B] or NULL = S each, 0 <= n_b <= S): ragged batch, see "Ragged batches"; utterance b's row
   is [silence | its n_b samples | silence | zeros to the row's end], and only its own n_b samples enter its peak.
   peak_out: optional device f32 [B], each utterance's max |x|.
   pcm must not alias wav; wav needs 4-byte and pcm 2-byte alignment only. The context need not be finalized. The
   length table goes through a ring of this entry point's own, so the call may run on any stream.
   Two differences from the reference function:
     - a silent or empty utterance (peak 0): the reference divides by zero (ZeroDivisionError); here its row is zeros
       and its peak_out is 0;
     - non-finite input is the caller's error and gives undefined samples (as for svc_whisper_encode). */
svc_status svc_pcm16(svc_ctx* ctx, const float* wav, int B, int64_t S, const int64_t* utt_samples, int fs,
                     int add_silence, int turn_up, double volume_peak, void* pcm, float* peak_out, void* stream);

/* host-only: 1 + n_out / hop; -1 for n_out < 0 or hop < 1 */
int64_t svc_loudness_frames(int64_t n_out, int hop);

/* Loudness envelope transfer (so-vits-svc's "loudness envelope adjustment"; opt-in, between svc_bigvgan and svc_pcm16).
   wav f32 [B][S] (the vocoder output), src f32 [B][S_src] (the source at the same rate and time origin: sample i of
   one lines up with sample i of the other) -> out f32 [B][S]. Per utterance, with n_out / n_src its own lengths,
   W = window, H = hop:
     K = svc_loudness_frames(n_out, H) frames for both signals; frame k covers samples [kH - W/2, kH - W/2 + W), a
     sample outside [0, n) of its signal counting as 0 (librosa's rms(center=True) with zero padding);
     P_k = (sum (double)s^2) / W, E_k = sqrt(P_k); g_k = pow(E_src_k / max(E_out_k, floor_rms), 1 - mix), then
     min(g_k, max_gain) when max_gain > 0 (a value <= 0 means no cap), all in f64;
     out[i] = (float)((double)wav[i] * (g_k0 + frac * (g_k1 - g_k0))), k0 = i / H, frac = (i - k0 H) / H,
     k1 = min(k0 + 1, K - 1), for i < n_out; zeros from n_out to S.
   This is audio.loudness_match, the project's host restatement: gains within (W + 16) * 2^-52 relative of it, samples
   within 1 f32 ulp. mix = 1 copies wav bit for bit; mix = 0 gives it the source's envelope. A silent source frame
   gives gain 0 (mix < 1); a silent output under a loud source is bounded by floor_rms, and by max_gain when given.
   utt_samples / src_samples (host int64 [B] or NULL = S / S_src each; 0 <= n_out <= S, 0 <= n_src <= S_src): ragged
   batch, see "Ragged batches"; each frame's sum runs in an order fixed by the utterance's own lengths, W and H, so an
   utterance's row is bit-identical to the same utterance converted alone.
   gain_out: optional device f64 [B][svc_loudness_frames(S, hop)], each utterance's g_k and 0 past its own K.
   out may be wav itself (the same pointer); any other overlap of out with wav, and any with src, is an error. All
   buffers need 4-byte alignment only (gain_out 8). The context need not be finalized. Two launches whatever B is; the
   length tables and the frame powers go through a ring of this entry point's own, so the call may run on any stream.
   SVC_ERR_INVALID before any HIP call: null wav, src or out; B < 1, S or S_src < 1; a length outside [0, S] /
   [0, S_src]; window or hop < 1; mix outside [0, 1] or NaN; floor_rms not > 0; out overlapping wav partially, or src;
   more than 64 MiB of frame powers (16 B * K * B: a hop far too small for the batch).
   Non-finite input is the caller's error and gives undefined samples. */
svc_status svc_loudness_match(svc_ctx* ctx, const float* wav, const float* src, int B, int64_t S, int64_t S_src,
                              const int64_t* utt_samples, const int64_t* src_samples, int window, int hop, double mix,
                              double floor_rms, double max_gain, float* out, double* gain_out, void* stream);

/* Long-form conversion's join (opt-in, after svc_bigvgan): B chunks, each the waveform of one utterance, are written
   into `out`; a chunk that continues its predecessor is aligned to it by SOLA and crossfaded over X = xfade samples,
   with candidates d in [-R, R), R = search (d = 0 alone when R = 0). All tables are host arrays of length B:
     rows[b]     device pointer of chunk b's waveform, n[b] usable samples (pointers into the vocoder's output as it
                 stands; nothing is copied)
     lead[b]     the row index of chunk b's first body sample; body[b] its body samples
     joined[b]   1: chunk b continues chunk b - 1 of the same song, else 0; joined[0] = 0
     out_off[b]  the index in out of chunk b's first body sample
   Every chunk has a displacement d_b, 0 for an unjoined chunk, and plays row sample lead[b] + d_b + j at
   out[out_off[b] + j], j < body[b]. For a joined chunk b:
     a_j = rows[b-1][lead[b-1] + d_{b-1} + body[b-1] + j], j < X: the predecessor as it was actually played, so the
     seams of a song form a chain; c_j(d) = rows[b][lead[b] + d + j];
     nom(d) = sum_j (double)a_j (double)c_j(d), den(d) = sum_j (double)c_j(d)^2, in f64 with j ascending from 0 (each
     product is exact in f64, so fused and unfused multiply-adds give the same sums);
     q(d) = nom |nom| / (den + eps), three IEEE f64 operations: it orders the candidates as SOLA's nom / sqrt(den + eps);
     d_b = the candidate first by greater q, then smaller |d|, then greater d (silence gives 0);
     out[out_off[b] + j] = (float)(a_j + w_j (c_j(d_b) - a_j)), w_j = (j + 0.5) / X in f64, for j < X; for
     X <= j < body[b], and for the whole body of an unjoined chunk, the row sample is copied bit for bit.
   This is audio.stitch, the project's host definition: displacements and q bit-equal, crossfade samples within 1 f32
   ulp. shift_out: optional device int32 [B], d_b. q_out: optional device f64 [B][max(2R, 1)], q(d) at index d + R, 0
   for an unjoined chunk. Exactly the intervals [out_off[b], out_off[b] + body[b]) of out are written.
   Two launches whatever B is: stitch_seams (one workgroup per song walks its seams in order: both windows in LDS, one
   candidate per thread, a workgroup arg-max) and stitch_write (chunks x blocks of output samples). Songs run in
   parallel. All buffers need 4-byte alignment only (q_out 8). The context need not be finalized; the tables go through
   a ring of this entry point's own, so the call may run on any stream.
   SVC_ERR_INVALID before any HIP call: null ctx, rows, a row pointer, a table or out; B < 1; xfade outside [1, 8192];
   search outside [0, 1024]; eps not > 0; out_len < 1; joined[0] != 0 or a joined[b] other than 0 / 1; for a joined b,
   out_off[b] != out_off[b-1] + body[b-1] or body[b] < xfade; a body[b] < 1 or n[b] < 1; an output interval outside
   [0, out_len); two output intervals that overlap; out overlapping a row; any row index that the definitions can
   read, for any admissible displacement of chunk b and of its predecessor, outside [0, n[b]): that is
   lead[b] - (joined[b] ? R : 0) < 0, or lead[b] + (joined[b] && R ? R - 1 : 0) + body[b] + (joined[b+1] ? X : 0) > n[b].
   Non-finite samples are the caller's error: they give undefined displacements and samples, never an access outside
   the buffers. */
svc_status svc_stitch(svc_ctx* ctx, const float* const* rows, int B, const int64_t* n, const int64_t* lead,
                      const int64_t* body, const int32_t* joined, const int64_t* out_off, int xfade, int search,
                      double eps, float* out, int64_t out_len, int32_t* shift_out, double* q_out, void* stream);

/* Feature retrieval, part 1: the squared norms of an index. index16: binary16 [N] rows of ld >= D halves (a singer's
   enrolled content frames). norms[j] = (float) sum_c (double)x[j][c]^2 over the row's D values in column order (every
   square is exact in f64), f32 [N]. One launch, one thread per row. The context need not be finalized.
   SVC_ERR_INVALID before any HIP call: null index16 or norms; N outside [1, 2^31); D not a multiple of 8 in [8, 2048];
   ld < D; rows that do not start on 16-byte boundaries (ld % 8 != 0 or a misaligned pointer); a context with
   "operands.bf16" (fp16 only). */
svc_status svc_index_norms(svc_ctx* ctx, const void* index16, int64_t N, int D, int ld, float* norms, void* stream);

/* Feature retrieval, part 2 (RVC's feature index, `index_rate`; opt-in, between the content stage and svc_condition):
   every content frame is blended with the distance-weighted mean of its k nearest frames of the index.
   content16: binary16 [B*T] rows of ld halves, of which the first D are the frame; index16 [N] rows of ld_index halves
   and norms f32 [N] (svc_index_norms of it); out16: binary16 [B*T] rows of ld_out halves.
   A row r = b*T + t takes part when t < frames[b] (host int32 [B], NULL: all T) and sel[b] != 0 (host int32 [B], NULL:
   all). For such a row, with q its D halves:
     s_j  = norms[j] - 2 * dot(q, x_j): the products of the f16 values accumulated in f32 on v_mfma_f32_16x16x32_f16 in
            ascending K, the same for every row and index row wherever they sit in a tile;
     the k_eff = min(k, N) smallest under the total order (s_j, j): s compared as f32, an equal s goes to the lower j.
            The order is total, so the selected set and its order are unique: they do not depend on the tiling or on
            the number of index splits ("tune.retrieve_splits": 0 chosen from B*T and N, else that many);
     d2_i = max((float)|q|^2 + s_i, (float)dist_floor), |q|^2 an f32 sum in an order fixed by D;
     w_i  = (1 / d2_i) / sum_i (1 / d2_i) in f32, the sum over ranks ascending;
     y    = sum_i w_i * x_i by f32 fma in rank order;
     out  = round16(rate * y + (1 - rate) * q), two f32 products and one add ((float)rate and (float)(1 - rate)).
   rate = 0 copies q bit for bit (the blend is not formed). rate = 1 replaces the frame by y.
   Rows that take no part: a row of a selected utterance past frames[b] is written as +0 in columns 0..D-1; the rows of
   an unselected utterance are copied when out16 != content16 and not touched when out16 == content16. Columns at or
   past D of out16 are never touched. A ragged batch's utterance is bit-identical to the same utterance alone.
   idx_out (optional, device int32 [B*T][k]): the selected j in rank order, -1 past k_eff and on rows that take no
   part. dist_out (optional, device f32 [B*T][k]): the clamped d2_i, 0 in the same places.
   out16 may be content16 itself (the same pointer and ld_out == ld: the wave that writes a row has finished reading
   it); any other overlap of out16 with content16, and any with index16 or norms, is an error.
   Two launches: knn_topk (the distance GEMM with the selection as its epilogue: the B*T x N scores are never stored;
   a grid of query tiles x index splits, each split leaving 8 candidates per row in the workspace) and retrieve_blend
   (merges the splits by the same order, weights, gathers, blends, 16-byte stores). The candidates come from the
   context's workspace arena (64 B x B*T x splits), so the call is ordered with the other stages that use it; frames and
   sel go through a ring of this entry point's own. The context need not be finalized.
   Measured on MI355X (tools/retrieve_bench.py, profiles/retrieve_bench.json; 32 x 937 rows, D = 1024, k = 8): 1.84 /
   6.58 / 24.6 ms per call against an index of 16,384 / 65,536 / 262,144 rows (knn_topk at 553 / 617 / 648 TFLOP/s),
   0.32 ms for one clip of 937 rows against 65,536; 2.0 / 2.0 / 1.7 / 2.5 times the f16 torch.matmul of the same
   product alone and 0.27 / 0.33 / 0.34 / 0.46 of the library composition (matmul, topk, gather, blend).
   SVC_ERR_INVALID before any HIP call: a null context, content16, index16, norms or out16; B or T < 1 (or B*T >=
   2^31 - 128); k outside [1, 8]; D not a multiple of 8 in [8, 2048]; N outside [1, 2^31); ld, ld_index or ld_out < D,
   or rows that do not start on 16-byte boundaries; rate outside [0, 1] or NaN; dist_floor not > 0 (as f32);
   frames[b] outside [0, T]; a partial overlap of the buffers; a context with "operands.bf16" (fp16 only: the message
   says so). Non-finite features are the caller's error and give undefined rows (never an access outside the buffers). */
svc_status svc_content_retrieve(svc_ctx* ctx, const void* content16, int B, int T, const int32_t* frames,
                                const int32_t* sel, int D, int ld, const void* index16, const float* norms, int64_t N,
                                int ld_index, int k, double rate, double dist_floor, void* out16, int ld_out,
                                int32_t* idx_out, float* dist_out, void* stream);

/* Index compaction (RVC fits k-means centres to a large feature index): Lloyd's iteration over a singer's content
   frames, so that the rows svc_content_retrieve searches are K centroids covering all N frames instead of a strided
   sample of them. fp16 rows only. Shared by the three entry points below: rows16 is binary16 [N] rows of ld >= D
   halves, N in [1, 2^22]; K in [1, min(N, 2^20)]; D a multiple of 8 in [8, 2048]; every set of rows (rows16, centroids)
   starts its rows on 16-byte boundaries (ld % 8 == 0, an aligned pointer). Scratch comes from the context's workspace
   arena through each call's own buffer list, so the calls are ordered with the other stages that use it. All work is
   enqueued on the stream: no host synchronisation, no random numbers. The context need not be finalized.
   SVC_ERR_INVALID before any HIP call: a null context or required pointer; N, K, D, iters outside the ranges above;
   ld < D or rows that do not start on 16-byte boundaries; an output that overlaps an input it is not allowed to be;
   a context with "operands.bf16" (fp16 only: the message says so).

   Part 1, the assignment. cent16: binary16 [K] rows of ld_cent halves, cent_norms f32 [K] (svc_index_norms of them).
     labels[r] (device int32 [N]) = the j smallest under the total order (s_j, j), s_j = cent_norms[j] - 2 * dot(x_r,
            c_j): svc_content_retrieve's score exactly (f16 products accumulated in f32 on v_mfma_f32_16x16x32_f16 in
            ascending K, the same for a row wherever it sits in a tile), compared as f32, an equal s going to the lower
            j. The labels therefore do not depend on the tiling, on "tune.retrieve_splits" or on the chunks of rows in
            which N is walked (2^18 rows per launch, fewer when the splits are forced high).
     counts[j] (optional, device int32 [K]) = the number of rows labelled j (integer atomics).
     inertia[0] (optional, device f64) = sum_r max((float)|x_r|^2 + s_label(r), 0): |x_r|^2 an f32 sum in
            svc_content_retrieve's order for |q|^2, each term f32, the terms added in f64 in an order fixed by N alone
            (4096 terms per workgroup, a fixed tree), so the value is bit-identical from run to run.
   Launches: index_prep, then per chunk knn_topk (svc_content_retrieve's kernel as it stands: rows as queries, centroids
   as the index) and index_label (rank 0 of the splits' candidates), then inertia_part / inertia_final where asked.
   Non-finite rows are the caller's error (such a row is labelled 0; never an access outside the buffers). */
svc_status svc_index_assign(svc_ctx* ctx, const void* rows16, int64_t N, int D, int ld, const void* cent16,
                            const float* cent_norms, int K, int ld_cent, int32_t* labels, int32_t* counts,
                            double* inertia, void* stream);

/* Part 2, the centroid update: the mean of every cluster, computed exactly and therefore independent of the order in
   which its rows are met. labels: device int32 [N]; prev16: the previous centroids, [K] rows of ld_prev halves.
     I(v)      = v * 2^24, an integer for every finite binary16 value, |I| < 2^40;
     S[j][c]   = sum of I(x_r[c]) over the rows with labels[r] == j: exact in int64 (N <= 2^22);
     out[j][c] = (half)(float)(((double)S[j][c] / (double)count_j) * 2^-24): the int64 -> f64 conversion, the f64
                 division and the f32 and f16 conversions each round to nearest even;
     a centroid with count_j == 0 keeps prev16's row bit for bit;
     norms_out[j] (f32 [K]) = svc_index_norms' arithmetic on the new row; counts[j] (optional, int32 [K]) = count_j.
   out16 ([K] rows of ld_out halves; columns at or past D are never touched) may be prev16 itself (the same pointer and
   ld_out == ld_prev); any other overlap with prev16, and any with rows16, is an error. A label outside [0, K) is the
   caller's error: its row joins no cluster, and nothing outside the buffers is touched.
   Launches: index_hist, index_scan and index_scatter group the row numbers by label (counts, an exclusive scan, an
   integer cursor per cluster); index_sum gives every cluster one workgroup per 1024 member rows, which streams whole
   rows in 16-byte pieces into int64 sums and writes the f16 row; index_combine (only when N > 1024) adds the int64
   partial rows of the clusters that had more than one workgroup; index_rownorms writes the new rows' norms. */
svc_status svc_index_update(svc_ctx* ctx, const void* rows16, int64_t N, int D, int ld, const int32_t* labels, int K,
                            const void* prev16, int ld_prev, void* out16, int ld_out, float* norms_out, int32_t* counts,
                            void* stream);

/* Part 3, the loop. cent16 ([K] rows of ld_cent halves) and cent_norms (f32 [K]) receive the result.
     centroid i starts as row floor(i * N / K) of rows16: the rule by which SVCPipeline.enroll(index_max_rows=K) thins
     an index, so iters = 0 returns that index (rows and svc_index_norms) bit for bit;
     iters times (0 <= iters <= 1000): svc_index_assign, then svc_index_update in place;
     one last svc_index_assign against the final centroids fills labels (optional, int32 [N]), counts (optional, int32
     [K]) and the last inertia. inertia (optional, device f64 [iters + 1]): entry i is the assignment's inertia against
     the centroids after i updates.
   There is no early stop: a converged state is a fixed point of assign + update, so further iterations change nothing.
   The result equals composing the two calls above by hand, bit for bit. cent16 must not overlap rows16.
   Measured on MI355X (tools/kmeans_bench.py, profiles/kmeans_bench.json). */
svc_status svc_index_kmeans(svc_ctx* ctx, const void* rows16, int64_t N, int D, int ld, int K, int iters, void* cent16,
                            int ld_cent, float* cent_norms, int32_t* labels, int32_t* counts, double* inertia,
                            void* stream);

/* ---------------- op-level entry points (used by the parity tests; weights are unpacked f32 device arrays) */
/* y[B*T_out][Cout] = conv1d(x[B*T_in][Cin]) ; w [Cout][Cin][k] ; act 0 none / 1 gelu / 2 relu */
svc_status svc_op_conv1d(const float* x, int B, int T_in, int Cin, const float* w, const float* bias, int Cout, int k,
                         int stride, int dilation, int pad, int act, float* y, void* stream);
/* ConvTranspose1d, w [Cin][Cout][k]; T_out = (T_in-1)*stride - 2*pad + k */
svc_status svc_op_conv_transpose1d(const float* x, int B, int T_in, int Cin, const float* w, const float* bias,
                                   int Cout, int k, int stride, int pad, float* y, void* stream);
/* Rational-ratio resampler (F1; replaces librosa.resample in utils/audio.py:49-53 and ffmpeg's 16 kHz decode in
 * utils/whisper_extractor/audio.py:41-49). x f32 [B][n_in] -> y f32 [B][svc_resample_len(n_in, sr_in, sr_out)],
 * scipy.signal.resample_poly's Kaiser(5) polyphase FIR; quantize16 = 1 rounds to int16 / 32768 (s16le decode). */
int64_t svc_resample_len(int64_t n_in, int sr_in, int sr_out);
svc_status svc_resample(const float* x, int B, int64_t n_in, int sr_in, int sr_out, int quantize16, float* y,
                        void* stream);
/* host-only: the designed taps (cap >= *n, or h = NULL to query *n) and the plan's up/down/pre_remove */
svc_status svc_resample_filter(int sr_in, int sr_out, double* h, int cap, int* n, int* up, int* down,
                               int* pre_remove);
/* BigVGAN AMP step for small channel counts: y = conv_k,d(Activation1d(x)) + bias (+ add_row), fused.
 * x, add_row, y f32 [B*L][C] time-major; w f32 [C][C][k] (effective weight); C in {24, 48, 96, 192}.
 * Replaces modules/bigvgan.py:427-431 (a1/c1, a2/c2 pairs) for the late generator stages. */
svc_status svc_op_amp_conv(const float* x, int B, int L, int C, const float* alpha_log, const float* beta_log,
                           const float* filt, const float* w, const float* bias, int k, int d, const float* add_row,
                           float* y, void* stream);
/* The same kernel with every operand svc_bigvgan gives it (the parity tests): input x (f32) or x16 (binary16), exactly
 * one of them; ragged lengths tv [B] (utterance b has min(L, tv[b] * tv_mul) rows, rows past that are left untouched;
 * NULL = all L); epilogue v = conv + bias (+ add_row), then v = (acc32 + v) / acc_div when acc32 is given; outputs out32
 * (f32, may be acc32 or add_row itself) and / or out16 (binary16, saturating). All tensors [B*L][C]; C in
 * {24, 48, 96, 192}. svc_op_amp_conv is this with x, add_row and out32 only. */
svc_status svc_op_amp_conv_ex(const float* x, const void* x16, int B, int L, int C, const float* alpha_log,
                              const float* beta_log, const float* filt, const float* w, const float* bias, int k, int d,
                              const int32_t* tv, int tv_mul, const float* add_row, const float* acc32, float acc_div,
                              float* out32, void* out16, void* stream);
/* The rate-2 ConvTranspose1d of BigVGAN's late stages as svc_bigvgan runs it (tune.amp_ups): one plain conv over the
 * input rows with the combined packing of both output phases. x16 binary16 [B*T_in][Cin], w f32 [Cin][Cout][k] (no
 * weight norm), pad = (k - stride) / 2, tv / tv_mul as above, y f32 [B*stride*T_in][Cout]. SVC_ERR_INVALID for a shape
 * without a combined form (anything but stride 2, k 4, Cin = 2 Cout in {48, 96, 192}): nothing else is run. */
svc_status svc_op_conv_transpose1d_comb(const void* x16, int B, int T_in, int Cin, const float* w, const float* bias,
                                        int Cout, int k, int stride, const int32_t* tv, int tv_mul, float* y,
                                        void* stream);
/* Activation1d(SnakeBeta, logscale): x f32 [B*L][C] -> y f32 [B*L][C] */
svc_status svc_op_activation1d(const float* x, int B, int L, int C, const float* alpha_log, const float* beta_log,
                               const float* filt12, float* y, void* stream);
/* the same on an f16 input x16 [B*L][C] (binary16; the AMPBlock1 convs1 outputs in the product path) */
svc_status svc_op_activation1d_x16(const void* x16, int B, int L, int C, const float* alpha_log, const float* beta_log,
                                   const float* filt12, float* y, void* stream);
/* attention on f32 q,k,v [B*L][D] (already projected; scaled inside by dh^-1/4 each) -> out f32 [B*L][D] */
svc_status svc_op_attention(const float* q, const float* k, const float* v, int B, int L, int D, float* out,
                            void* stream);
/* the same with per-utterance lengths, as svc_hubert_encode_ragged runs it: lens HOST int32 [B], each 1..L
   (otherwise SVC_ERR_INVALID before any HIP call; NULL = svc_op_attention). Utterance b attends over its first
   lens[b] rows only and equals svc_op_attention on those rows at L = lens[b] bit for bit; rows >= lens[b] of q / k / v
   are never read, and rows >= lens[b] of out are zeros. */
svc_status svc_op_attention_ragged(const float* q, const float* k, const float* v, int B, int L, int D,
                                   const int32_t* lens, float* out, void* stream);
svc_status svc_op_layernorm(const float* x, const float* g, const float* b, int rows, int D, float* y, void* stream);
/* The sampler's element-wise kernels exactly as svc_diffsvc_sample launches them (the parity tests; no copies, every
 * pointer a device pointer). x16 is the 16-bit copy for the next GEMM, rows of ld16 >= C halves of which columns
 * 0..C-1 are written: binary16, or bfloat16 bits with bf16 = 1.
 * svc_op_init_noise: x [B*T][C] = std * N(0, 1), the x_T draw: Philox4x32-10 with counter {t * C + c, 0xFFFFFFFF,
 * utt_ids[b], 0x5356434B} and key {seed low word, seed high word}, Box-Muller on its first two words. x16 is required. */
svc_status svc_op_init_noise(uint64_t seed, const int32_t* utt_ids, int B, int T, int C, float std, float* x, void* x16,
                             int ld16, int bf16, void* stream);
/* svc_diffsvc_sample_from's start state from mel_src, one launch: y = (mel - mel_min) / (mel_max - mel_min + 1e-12) * 2
 * - 1 per channel (mel_min, mel_max f32 [C]), x [B*T][C] = sqrt_ac y + sqrt_1mac z. z [B*T][C] given, or NULL: drawn as
 * in svc_op_init_noise with counter word 1 = 0xFFFFFFFE, which needs utt_ids (both NULL is SVC_ERR_INVALID). frames
 * (DEVICE int32 [B] or NULL): rows t >= frames[b] get 0 in x and x16. x16 is optional. Four channels per thread when
 * C % 4 == 0, ld16 % 4 == 0, the f32 pointers are 16-byte and x16 8-byte aligned, else one. */
svc_status svc_op_q_sample(const float* mel, const float* mel_min, const float* mel_max, int B, int T, int C,
                           float sqrt_ac, float sqrt_1mac, const float* z, uint64_t seed, const int32_t* utt_ids,
                           const int32_t* frames, float* x, void* x16, int ld16, int bf16, void* stream);
/* One PLMS update on [rows][C]: e' = (c0 e0 + c1 e1 + ...) / div over the first ne (1..4) histories (the others may
 * be NULL), xout = xin + d (A xin - Bc e'); xout may be xin. Optional outputs: x16 and e_avg_out (e'). Four channels
 * per thread when C % 4 == 0, ld16 % 4 == 0, the f32 pointers are 16-byte and x16 8-byte aligned, else one. */
svc_status svc_op_plms_update(const float* e0, const float* e1, const float* e2, const float* e3, float c0, float c1,
                              float c2, float c3, int ne, float div, float d, float A, float Bc, const float* xin,
                              float* xout, void* x16, int ld16, float* e_avg_out, int bf16, int rows, int C,
                              void* stream);
/* One DDPM p_sample step in place on x [B*T][C]: x0 = clip(sra x - srm1 eps, -1, 1), x = c1 x0 + c2 x + sigma z.
 * z [B*T][C] given, or NULL: drawn as in svc_op_init_noise with counter word 1 = step, which needs utt_ids (both NULL
 * is SVC_ERR_INVALID). x16 is required. */
svc_status svc_op_ddpm_update(float* x, const float* eps, int B, int T, int C, float sra, float srm1, float c1,
                              float c2, float sigma, const float* z, uint64_t seed, const int32_t* utt_ids, int step,
                              void* x16, int ld16, int bf16, void* stream);
/* One DPM-Solver++(2M) / DDIM update in place on x [rows][C] (svc_diffsvc_sample_steps launches it after each denoise):
 * D = clip(sra x - srm1 eps, -1, 1); Dbar = D, or with d_prev (NULL: no history) w0 D + w1 d_prev; x = a x + b Dbar, or
 * with final_step x = D (a, b, w0, w1 and d_prev are ignored). d_out (optional) receives D and may be d_prev. x16 is
 * optional. Four channels per thread when C % 4 == 0, ld16 % 4 == 0, the f32 pointers are 16-byte and x16 8-byte
 * aligned, else one; both forms return the same bits. */
svc_status svc_op_dpm_update(float* x, const float* eps, const float* d_prev, float* d_out, int rows, int C, float sra,
                             float srm1, float w0, float w1, float a, float b, int final_step, uint16_t* x16, int ld16,
                             int bf16, void* stream);
/* The DiffSVC denoiser's steps one at a time, each through the launcher choice svc_diffsvc_eps / svc_diffsvc_sample
 * make for it (stage_diffsvc.hip diffsvc_*), selected as there by the op-level context's kernel switches
 * (svc_ctx_set_config(NULL, "tune.gate_ws" | "tune.gemm_variant" | "tune.res_proj" | "tune.diff_head" |
 * "tune.sampler_streams")). C = 384 residual channels, n_mel = 100. Every pointer is a device pointer; 16-bit tensors
 * are binary16, or bfloat16 bits with bf16 = 1 (the weights are then packed as bfloat16 too). Weights are f32 in the
 * reference's layout and channel order and are packed per call as svc_ctx_finalize packs them. Arguments are checked
 * before any HIP call (SVC_ERR_INVALID).
 * gate: y16 [B*T][384] = sigmoid(g) * tanh(f), [g | f] = conv1d_k3(x16 [B*T][384]; w [768][384][3], bias [768],
 * dilation dil in {1, 2, 4, 8}, zero padding per utterance) + cp16 [B*T][768]. tv (DEVICE int32 [B] or NULL):
 * utterance b's input rows t >= tv[b] read as zero; every output row is written. */
svc_status svc_op_diffsvc_gate(const void* x16, int B, int T, const float* w, const float* bias, const void* cp16,
                               int dil, const int32_t* tv, int bf16, void* y16, void* stream);
/* res: the split residual stream hi + lo [M][384] updated in place, v = ((hi + lo) - sub + g16 [M][384] w^T + bias) /
 * sqrt(2) + add, hi = round16(v), lo = round16(v - hi); w [384][384] (the residual half of a layer's
 * output_projection), bias / sub / add [384]. lanes_cap: res_proj's row lanes as the stage computes them (-2, 0 or a
 * count), -1: the tiled GEMM. store_lo = 0 (res_proj only; the tiled GEMM always writes lo): lo is read, not written. */
svc_status svc_op_diffsvc_res(const void* g16, int M, const float* w, const float* bias, const float* sub,
                              const float* add, int store_lo, int lanes_cap, int bf16, void* hi, void* lo,
                              void* stream);
/* melpre: v = relu(x16 [M][104] (columns 100..103 zero) w^T + bias) + add into hi / lo [M][384]; w [384][100]. */
svc_status svc_op_diffsvc_melpre(const void* x16, int M, const float* w, const float* bias, const float* add, int bf16,
                                 void* hi, void* lo, void* stream);
/* skipsum: s = (sum_l g16[l][row0 + r] w[l]^T + sum_l bias[l]) / sqrt(NL) for r < rows, g16 layer-major
 * [NL][rows_total][384], w [NL][384][384] / bias [NL][384] the skip halves; s16 [rows][1152] = [hi | lo | hi]. */
svc_status svc_op_diffsvc_skipsum(const void* g16, int NL, int rows_total, int row0, int rows, const float* w,
                                  const float* bias, int bf16, void* s16, void* stream);
/* head: eps [M][100] = relu(s wsp^T + bsp) wout^T + bout on split operands, s16 [M][1152] = [hi | lo | hi],
 * wsp [384][384], wout [100][384]; one launch or two by "tune.diff_head". */
svc_status svc_op_diffsvc_head(const void* s16, int M, const float* wsp, const float* bsp, const float* wout,
                               const float* bout, int bf16, float* eps, void* stream);
/* condproj: cp16 [NL][M][768] (layer-major, reference channel order) = cond [M][384] (f32, split into 16-bit
 * hi + lo) w[l]^T + bias[l]; w [NL][768][384], bias [NL][768]. */
svc_status svc_op_diffsvc_condproj(const float* cond, int M, int NL, const float* w, const float* bias, int bf16,
                                   void* cp16, void* stream);
/* live per-kernel timing: enable(1) clears and starts recording (hipEvents around each launch),
   read(idx, ...) synchronises and returns kernel idx's name, total ms, launches, algorithmic FLOPs/bytes;
   n_kernels receives the number of distinct kernels. */
svc_status svc_profile_enable(int enable);
/* Restrict live profiling to kernels whose name starts with kernel_prefix ("" or NULL = all): bench.py times
 * only the dominant kernel in its timed region, so the other ~4 000 launches per step carry no events. */
svc_status svc_profile_filter(const char* kernel_prefix);
svc_status svc_profile_read(int idx, char* name, int name_len, double* total_ms, int64_t* launches, double* flops,
                            double* bytes, int* n_kernels);
/* GEMM microbenchmark on synthetic operands: average ms per launch of one implicit-GEMM configuration
   (10-14 = conv_gemm3 tiles, 15 = the production choice, 20 / 24 = conv_gemm4 with the LDS-staged / register
   gate epilogue; see run_gemm in engine.hip); epi 0 = f16 store, 1 = paired gate, 2 / 6 = f32 / split-fp16 residual
   read-modify-write, 3-5 = gate diagnostics (variant 24: 3 no cp read and no store, 4 no cp read, 5 no store);
   iters < 0: |iters| launches, each after a 1 GiB memset (operands evicted from the caches) */
svc_status svc_gemm_bench(int M, int N, int Cin, int taps, int epi, int variant, int iters, double* ms_out);
/* slaney mel filterbank (librosa.filters.mel, htk=False, norm='slaney') computed natively, host output */
svc_status svc_mel_filterbank(int sr, int n_fft, int n_mels, double fmin, double fmax, float* out_host);

#ifdef __cplusplus
}
#endif
#endif
