"""Batched counterpart of the reference's infer.py (infer.py:44-90), on one GPU.

    mel, energy = acoutic_feature_extractor(...)        infer.py:53   -> SVCEngine.mel_energy + f0
    f0 = pitch_shift(f0, cfg)                           infer.py:59   -> SVCEngine.pitch_shift (the target median per
                                                                         clip: its singer's, once enrolled with
                                                                         SVCPipeline.enroll; a key shift on request)
    whisper_feature = whisper_feature_extractor(...)    infer.py:64   -> whisper_encode + map_content
    contentVec_feature = contentVec_feature_extractor   infer.py:65   -> hubert_encode + map_content(rule="hubert")
    y_pred = svc_model_inference(...)                   infer.py:79   -> condition + diffsvc_sample
    y_pred = denormalize_mel_channel(y_pred, cfg)       infer.py:80   -> fused into bigvgan
    audio = synthesis_audios(...)                       infer.py:86   -> bigvgan (Generator, trim, fade)
    save_audio(save_path, audio, cfg.fs)                infer.py:90   -> pcm16 (with pcm16=True; the file: audio.py)

Inputs are device tensors of B equal-length utterances (24 kHz f32 and the 16 kHz int16-quantised
copy Whisper consumes); every stage runs in libsvc_hip.so on the current stream.

Long inputs (SURVEY.md §5 "Long-context", BASELINE config 4). The reference pads/trims Whisper's input
to one 30 s window and caps the mapped content at 2812 frames (utils/whisper.py:52-56), so for clips
longer than ~29.99 s its `torch.cat` in modules/encoder.py:197 raises. Here, when T > 2812, Whisper runs
on consecutive windows of 478 720 samples (29.92 s = 1496 encoder frames = exactly 2805 mel frames, so
the 15:8 map stays integral and every window starts on a mel frame). Each window is encoded in its own
zero-padded 30 s context and mapped with the reference's own 15:8 rule. Parity for such clips is per
window (tests/test_gpu_long.py). Mel, F0, the sampler and BigVGAN run over the whole length in one pass:
a 180 s song needs ~0.4 GB per vocoder stage buffer, far below 288 GB of HBM, so the vocoder needs no
overlap-add seams. Where memory must not grow with the song, or a song should share batches, convert_long cuts
it into overlapping chunks, converts them as a ragged batch under the song's own F0 and key, and joins them with
svc_stitch (DESIGN.md "Long-form conversion").
"""
from dataclasses import dataclass

import torch

from .audio import check_loudness_mix
from .config import check_solver, solver_timesteps
from .runtime import SVCEngine, check_k_step, check_k_step_mel, mel_frames
from .singers import check_index_compact, check_index_rate

WHISPER_WINDOW = 478720       # 16 kHz samples per long-input window (29.92 s)
WINDOW_MEL_FRAMES = 2805      # = 1496 encoder frames * 15 / 8
MAX_MAPPED = 2812             # utils/whisper.py:56 (1500 * 15 // 8)
HUBERT_CONTENT_TYPES = ("contentvec", "content_vector", "hubert")  # config/config.json:35 names it content_vector


def hubert_content_type(cfg):
    """The HuBERT / ContentVec content type cfg.mapper.content_feature names, or None."""
    types = getattr(getattr(cfg, "mapper", None), "content_feature", None) or ()
    return next((t for t in types if t in HUBERT_CONTENT_TYPES), None)


def wants_float16k(cfg):
    """The file entry points load the float 16 kHz rows (audio.load_batch(float16k=True)) exactly when the
    configuration names a HuBERT / ContentVec content type."""
    return hubert_content_type(cfg) is not None


@dataclass
class ConvertResult:
    wav: torch.Tensor        # f32 [B, T*hop] converted audio (before save_audio's peak normalisation)
    mel: torch.Tensor        # f32 [B, T, n_mels] source log-mel
    f0: torch.Tensor         # f64 [B, T] pitch-shifted F0
    x0: torch.Tensor         # f32 [B, T, n_mel] normalised mel from the sampler
    pcm: torch.Tensor = None  # int16 [B, T*hop + 2*(fs//20)] save_audio's samples of wav (convert(pcm16=True) only)


@dataclass
class LongChunks:
    """What convert_long(return_chunks=True) adds to its waveforms; every list has one entry per song."""
    plans: list    # audio.ChunkPlan
    chunks: list   # lists of f32 [T_k * hop] chunk waveforms (views into the vocoder outputs)
    shifts: list   # int32 [chunks] displacements the stitch chose (device)
    f0: list       # f64 [T_song] the song's pitch-shifted F0, which the chunks took their slices of
    stitched: list  # f32 [T_song * hop] the stitched song before the loudness stage and the sample conversion


class SVCPipeline:
    def __init__(self, engine: SVCEngine, f0_side=True, f0_method="parselmouth", hubert_ragged=None,
                 whisper_ragged=None):
        """whisper_ragged: a ragged batch's Whisper features come from ONE call (svc_whisper_content_ragged): every 30 s
        window that exists is encoded once, short and long clips in one encoder pass, and one mapping launch writes
        straight into the content buffer; False: the two-group form (clips of one window, then long clips padded to the
        longest one's window count, one copy per clip; the same values bit for bit; DESIGN.md "A5-A7 for ragged
        batches"). None (default): the one-call form with every engine that has it (SVCEngine does: its
        `ragged_whisper` is True), the two-group form with an engine object that lacks it. True with such an engine is
        a ValueError, never a quiet fall-back. The form in use is `self.whisper_ragged`.
        hubert_ragged: a ragged batch's HuBERT / ContentVec features come from ONE padded encoder pass with
        per-utterance lengths (svc_hubert_encode_ragged) and one ragged mapping launch; False: one encoder pass, one
        mapping and one copy per exact-length bucket (the same values bit for bit; DESIGN.md "A8 for ragged batches").
        None (default): the one-pass form with every engine that has the length-taking entry points (SVCEngine does:
        its `ragged_hubert` is True), the per-bucket form with an engine object that lacks them. True with such an
        engine is a ValueError, never a quiet fall-back. The form in use is `self.hubert_ragged`.
        f0_side: run the 24 kHz features (mel / energy, F0, pitch shift) on the context's sub-stream 2 beside the
        content encoder (default; measured +0.4 %) instead of on the caller's stream.
        f0_method: "parselmouth" (utils/f0.py:120-161, what utils/acoustic_feature_extraction.py:53 uses) or "pyin"
        (utils/f0.py:95-117 get_f0_features_using_pyin, svc_f0_pyin; its 1 + N // hop frames cut to the mel frames)."""
        if f0_method not in ("parselmouth", "pyin"):
            raise ValueError(f"f0_method {f0_method!r}: 'parselmouth' or 'pyin'")
        self.engine = engine
        self.f0_side = f0_side
        self.f0_method = f0_method
        able = bool(getattr(engine, "ragged_hubert", False))
        if hubert_ragged and not able:
            raise ValueError("hubert_ragged=True: the engine has no hubert_encode(n_samples=) / map_content(frames=, "
                             "src_rows=) (its ragged_hubert is not set)")
        self.hubert_ragged = able if hubert_ragged is None else bool(hubert_ragged)
        able = bool(getattr(engine, "ragged_whisper", False))
        if whisper_ragged and not able:
            raise ValueError("whisper_ragged=True: the engine has no whisper_content(wav16, n_samples, frames, T) (its "
                             "ragged_whisper is not set)")
        self.whisper_ragged = able if whisper_ragged is None else bool(whisper_ragged)

    def extract_f0(self, wav24, T, n_samples=None, T_b=None):
        """F0 by the configured method -> f64 [B, T] (rows past an utterance's T_b frames 0)."""
        e = self.engine
        if self.f0_method == "parselmouth":
            return e.f0(wav24, T, n_samples=n_samples)
        N = wav24.shape[1]
        f0 = e.f0_pyin(wav24, n_samples=n_samples, T=max(T, 1 + N // e.cfg.hop_length))[:, :T].contiguous()
        if T_b is not None:
            for b, tb in enumerate(T_b):
                f0[b, tb:] = 0
        return f0

    def shift_f0(self, f0, singers, key_shift=0.0):
        """A4 on f0 f64 [B, T], in place: clip b's voiced median moves onto its singer's (engine.singer_f0; the global
        target_f0_median for a singer that is not enrolled), then up by key_shift semitones (a scalar or one per clip;
        the factor 2 ** (k / 12) is computed here in f64). With an empty table and no shift this is the scalar call
        svc_pitch_shift as before, and `singers` (which may be a device tensor) is not looked at."""
        return self.engine.pitch_shift(f0, *self.shift_targets(f0.shape[0], singers, key_shift))

    def shift_targets(self, B, singers, key_shift=0.0):
        """The arguments after f0 with which shift_f0 calls engine.pitch_shift for a batch of B (engine.pitch_factor
        takes the same): none, the scalar route, with an empty singer table and no key shift; else (targets, scale), one
        target per clip and, with a key shift, one scale per clip (else None)."""
        e = self.engine
        table = getattr(e, "singer_f0", None)
        ks = key_shift.tolist() if hasattr(key_shift, "tolist") else key_shift
        ks = [float(k) for k in ks] if isinstance(ks, (list, tuple)) else [float(ks)] * B
        if len(ks) != B:
            raise ValueError(f"{len(ks)} key shifts for a batch of {B}")
        if not table and not any(ks):
            return ()
        ids = singers.reshape(-1).tolist() if hasattr(singers, "tolist") else list(singers)
        if len(ids) != B:
            raise ValueError(f"{len(ids)} singers for a batch of {B}")
        targets = [table.get(s, e.target_f0_median) if table else e.target_f0_median for s in ids]
        scale = [2.0 ** (k / 12.0) for k in ks] if any(ks) else None
        return targets, scale

    def _check_index_rate(self, index_rate):
        """index_rate validated (ValueError before any device work); None stays None. bf16 content has no retrieval."""
        index_rate = check_index_rate(index_rate)
        if index_rate is not None and getattr(self.engine, "operands", "fp16") == "bf16":
            raise ValueError("index_rate: feature retrieval takes fp16 content (this engine runs operands='bf16')")
        return index_rate

    def retrieve(self, content, singers, index_rate, frames=None):
        """Feature retrieval on content f16 [B, T, D] in place: one engine.content_retrieve call per distinct singer of
        the batch that has an index in engine.singer_index, `sel` marking that singer's clips; clips of singers
        without an index are left alone, and with no enrolled singer in the batch nothing is launched."""
        e = self.engine
        table = getattr(e, "singer_index", None)
        if index_rate is None or not table:
            return content
        ids = [int(s) for s in (singers.reshape(-1).tolist() if hasattr(singers, "tolist") else singers)]
        if len(ids) != content.shape[0]:
            raise ValueError(f"{len(ids)} singers for a batch of {content.shape[0]}")
        for s in sorted(set(ids)):
            entry = table.get(s)
            if entry is None:
                continue
            if entry["rows"].shape[1] != content.shape[2]:
                raise ValueError(f"singer {s}: index rows are {entry['rows'].shape[1]} wide, content is "
                                 f"{content.shape[2]}")
            sel = None if all(i == s for i in ids) else [1 if i == s else 0 for i in ids]
            e.content_retrieve(content, entry["rows"], entry["norms"], frames=frames, sel=sel, rate=index_rate,
                               out=content)
        return content

    def enroll(self, singer, sources=None, wavs24=None, max_batch=16, index=False, index_max_rows=None,
               wavs16=None, wavs16_float=None, index_compact="stride", index_iters=10):
        """Measure a singer's voiced F0 median from that singer's own recordings and record it as the singer's pitch
        target (utils/acoustic_feature_extraction.py:21-30 on the GPU): wav files (`sources`: paths, bytes or
        memoryviews, decoded by audio.load_batch) or 24 kHz f32 device tensors (`wavs24`), in ragged chunks of at most
        max_batch clips through the configured F0 extractor; each clip's own frames are gathered into one flat buffer
        and ONE svc_f0_voiced_median call takes the median of its voiced cells. -> the table entry {median, voiced,
        frames, n_utts} now in engine.singer_f0. A singer without a voiced frame is a ValueError; nothing is stored.
        index=True: the same recordings, in the same chunks, also go through the content stage (ragged_content), and
        each clip's own T_b content rows are concatenated into the singer's retrieval index in engine.singer_index
        (rows, their svc_index_norms, n_utts, frames, content types), which `index_rate=` on the conversion entry points
        searches. With `wavs24` the 16 kHz copies are needed too: `wavs16` (and `wavs16_float` for ContentVec), as
        convert_ragged takes them; `sources` are decoded to all of them. index_max_rows: an index of N > index_max_rows
        rows keeps rows floor(i * N / index_max_rows), i < index_max_rows (index_compact="stride", the default), or
        is replaced by the k-means centroids of all N rows (index_compact="kmeans": engine.index_kmeans with K =
        index_max_rows and index_iters rounds of Lloyd's iteration from those same strided rows; centroids that end
        without a row are dropped, and the entry records {"method", "iters", "inertia_first", "inertia_last",
        "dropped"} under "compact"). With N <= index_max_rows both modes keep every row. The F0 entry is what it is
        without index."""
        e = self.engine
        if (sources is None) == (wavs24 is None):
            raise ValueError("enroll: give either sources (wav files) or wavs24 (24 kHz tensors)")
        if max_batch < 1:
            raise ValueError("enroll: max_batch >= 1")
        if index_max_rows is not None and int(index_max_rows) < 1:
            raise ValueError("enroll: index_max_rows >= 1")
        index_compact, index_iters = check_index_compact(index_compact, index_iters)
        if index and getattr(e, "operands", "fp16") == "bf16":
            raise ValueError("enroll: index=True takes fp16 content (this engine runs operands='bf16')")
        if index and sources is None and wavs16 is None:
            raise ValueError("enroll: index=True with wavs24 needs the 16 kHz copies too (wavs16)")
        with e.lock:
            if sources is not None:
                from . import audio as A
                if index and wants_float16k(e.cfg):
                    wavs24, wavs16, wavs16_float = A.load_batch(list(sources), e.cfg.fs, e, float16k=True)
                else:
                    loaded = A.load_batch(list(sources), e.cfg.fs, e)
                    wavs24 = loaded[0]
                    wavs16 = loaded[1] if index else None
            wavs24 = [w.reshape(-1) for w in wavs24]
            if not wavs24:
                raise ValueError("enroll: no recordings")
            if index and (len(wavs16) != len(wavs24) or (wavs16_float is not None and len(wavs16_float) != len(wavs24))):
                raise ValueError("enroll: wavs16 (and wavs16_float) need one entry per recording")
            rows, crows = [], []
            for i in range(0, len(wavs24), int(max_batch)):
                w24, n24 = self._pad_stack(wavs24[i:i + int(max_batch)])
                T_b = [mel_frames(k, e.cfg.n_fft, e.cfg.hop_length) for k in n24]
                f0 = self.extract_f0(w24, max(T_b), n_samples=n24, T_b=T_b)
                rows += [f0[b, :tb] for b, tb in enumerate(T_b)]
                if index:
                    w16f = None if wavs16_float is None else list(wavs16_float[i:i + int(max_batch)])
                    c = self.ragged_content(list(wavs16[i:i + int(max_batch)]), T_b, max(T_b), w16f)
                    crows += [c[b, :tb] for b, tb in enumerate(T_b)]
            flat = torch.cat(rows).to(torch.float64).contiguous()
            med, cnt = e.f0_voiced_median(flat)
            voiced = int(cnt.item())
            if voiced == 0:
                raise ValueError(f"enroll: singer {singer}: no voiced frame in {len(wavs24)} recording(s)")
            entry = e.singer_f0.set(singer, float(med.item()), voiced=voiced, frames=int(flat.numel()),
                                    n_utts=len(wavs24))
            if index:
                x = torch.cat(crows).contiguous()
                N = x.shape[0]
                norms = compact = None
                if index_max_rows is not None and N > int(index_max_rows) and index_compact == "kmeans":
                    cent, cnorms, counts, inertia = e.index_kmeans(x, int(index_max_rows), index_iters)
                    live = counts > 0
                    x, norms = cent[live].contiguous(), cnorms[live].contiguous()
                    inertia = inertia.tolist()
                    compact = dict(method="kmeans", iters=index_iters, inertia_first=inertia[0],
                                   inertia_last=inertia[-1], dropped=int(index_max_rows) - int(x.shape[0]))
                elif index_max_rows is not None and N > int(index_max_rows):
                    keep = [i * N // int(index_max_rows) for i in range(int(index_max_rows))]
                    x = x[torch.tensor(keep, device=x.device)].contiguous()
                e.singer_index.set(singer, x, e.index_norms(x) if norms is None else norms, n_utts=len(wavs24),
                                   frames=N, content_types=sorted(e.cfg.mapper.content_feature),
                                   **({} if compact is None else dict(compact=compact)))
            return entry

    def content(self, wav16, T, wav16_float=None):
        """Content features of every type in cfg.mapper.content_feature mapped to T mel frames -> [B, T, sum of
        widths] in the engine's content_dtype (f16, or bf16 with operands="bf16"), the types' columns concatenated in ascending name order (the order in which the
        native conditioner packs their ContentEncoder Linears). "whisper" runs Whisper on the int16-quantised
        16 kHz audio (utils/whisper.py:96-103); "contentvec" runs HuBERT/ContentVec on float 16 kHz audio
        (utils/hubert.py:137-143; `wav16_float`, defaulting to wav16)."""
        e = self.engine
        m = e.cfg.mapper
        types = sorted(m.content_feature)
        if types == ["whisper"]:
            return self.whisper_content(wav16, T)
        widths = [int(m.input_content_dim[t]) for t in types]
        B = wav16.shape[0]
        out = torch.empty(B, T, sum(widths), device=wav16.device, dtype=e.content_dtype)
        col = 0
        for t, w in zip(types, widths):
            view = out[:, :, col:col + w]
            if t == "whisper":
                view.copy_(self.whisper_content(wav16, T))
            elif t in HUBERT_CONTENT_TYPES:
                feats = e.hubert_encode(wav16 if wav16_float is None else wav16_float)
                e.map_content(feats, T, rule="hubert", out=view)
            else:
                raise ValueError(f"content feature {t!r} is not supported (whisper, {', '.join(HUBERT_CONTENT_TYPES)})")
            col += w
        return out

    def whisper_content(self, wav16, T):
        """Whisper content features mapped to T mel frames -> f16 [B, T, D]."""
        e = self.engine
        B = wav16.shape[0]
        if T <= MAX_MAPPED:
            return e.map_content(e.whisper_encode(wav16), T)
        n_win = -(-T // WINDOW_MEL_FRAMES)
        need = n_win * WHISPER_WINDOW
        w = wav16
        if w.shape[1] < need:
            w = torch.nn.functional.pad(w, (0, need - w.shape[1]))
        wins = w[:, :need].reshape(B * n_win, WHISPER_WINDOW).contiguous()
        feats = e.whisper_encode(wins)                      # [B*n_win, 1500, D]
        D = feats.shape[-1]
        out = torch.empty(B, n_win * WINDOW_MEL_FRAMES, D, device=wav16.device, dtype=e.content_dtype)
        full = e.map_content(feats, WINDOW_MEL_FRAMES)     # every window mapped to 2805 frames
        out.copy_(full.view(B, n_win * WINDOW_MEL_FRAMES, D))
        return out[:, :T].contiguous()

    def _side_stream(self, device):
        if getattr(self, "_side", None) is None:
            self._side = self.engine.aux_stream(2)  # the context's own stream: no extra hardware-queue pressure
        return self._side

    def convert(self, wav24, wav16, singer, fast_inference=True, speedup=10, seed=0, utt_ids=None, x_T=None,
                noise=None, f0=None, wav16_float=None, pcm16=False, key_shift=0.0, k_step=None, k_step_mel="source",
                loudness_mix=None, solver=None, solver_steps=20, solver_spacing="logsnr", index_rate=None):
        """infer.py's sequence for B equal-length clips -> ConvertResult. `f0` (optional, f64 [B, T]) replaces the
        Praat extraction; it is pitch-shifted on a copy (the caller's tensor is not modified). pcm16: also run
        save_audio's sample conversion on the device (SVCEngine.pcm16, its defaults) and return it as `pcm`.
        key_shift: semitones on top of the shift to the singer's median, a scalar or one per clip (shift_f0).
        k_step (shallow diffusion; None: the full schedule from noise, the call as before): the sampler starts from the
        source's own mel noised to level k_step - 1 and denoises from there (SVCEngine.diffsvc_sample(k_step, mel_src));
        x_T is not used then.
        k_step_mel (with k_step): "source" (default) starts from the clip's own mel; "shifted" from its key-shifted mel
        (SVCEngine.mel_keyshift by the factor shift_f0 applies, SVCEngine.pitch_factor), so the start state's harmonics
        sit at the pitch the conditioner asks for. ConvertResult.mel stays the unshifted source mel.
        loudness_mix (None: the stage is not run, the call as before): loudness envelope transfer between the vocoder
        and the sample conversion (SVCEngine.loudness_match against wav24, in place): 0 gives the converted voice the
        source's slow RMS envelope, 1 leaves it as it is; `wav` and `pcm` are the adjusted ones.
        solver, solver_steps, solver_spacing (solver None: the DDPM / PLMS sampler, the call as before): "dpmpp2m" or
        "ddim" over solver_steps timesteps instead (SVCEngine.diffsvc_sample(solver=)), from noise or, with k_step, from
        the noised source mel; fast_inference and speedup are not used then, and `noise` is a ValueError.
        index_rate (None: the stage is not run, the call as before): feature retrieval between the content stage and
        the conditioner (retrieve(): SVCEngine.content_retrieve in place, once per enrolled singer of the batch): each
        content frame becomes index_rate * (the weighted mean of its nearest frames of its singer's enrolled index) +
        (1 - index_rate) * itself; clips of singers without an index (enroll(index=True)) are left alone."""
        k_step = self._check_k_step(k_step)
        check_k_step_mel(k_step_mel, k_step)
        loudness_mix = check_loudness_mix(loudness_mix)
        index_rate = self._check_index_rate(index_rate)
        solver_kw = self._solver_kw(solver, solver_steps, solver_spacing, k_step)
        with self.engine.lock:
            return self._convert(wav24, wav16, singer, fast_inference, speedup, seed, utt_ids, x_T, noise, f0,
                                 wav16_float, pcm16, key_shift, k_step, k_step_mel == "shifted", loudness_mix,
                                 solver_kw, index_rate)

    def _solver_kw(self, solver, solver_steps, solver_spacing, k_step):
        """The solver keywords validated (ValueError before any device work: the names, and the timestep list where the
        engine's configuration has a schedule) -> the keywords for the calls below, none when solver is None."""
        if check_solver(solver, solver_steps, solver_spacing) is None:
            return {}
        cfg = getattr(self.engine, "cfg", None)
        if getattr(cfg, "mapper", None) is not None:
            solver_timesteps(cfg, k_step, solver_steps, solver_spacing)
        return dict(solver=solver, solver_steps=solver_steps, solver_spacing=solver_spacing)

    def _check_k_step(self, k_step):
        """k_step validated against the engine's schedule (ValueError before any device work); None stays None."""
        return None if k_step is None else check_k_step(k_step, getattr(self.engine, "cfg", None))

    def _convert(self, wav24, wav16, singer, fast_inference, speedup, seed, utt_ids, x_T, noise, f0, wav16_float,
                 pcm16=False, key_shift=0.0, k_step=None, shifted=False, loudness_mix=None, solver_kw=None,
                 index_rate=None):
        e = self.engine
        T = mel_frames(wav24.shape[1], e.cfg.n_fft, e.cfg.hop_length)  # utils/mel.py:130-174 frame count
        # The 24 kHz features (mel / energy, and F0: Praat AC + pitch shift, latency-bound serial work on few CUs)
        # run on the context's sub-stream 2 beside the content encoder (they use their own workspace), joined before
        # the conditioner needs them
        main = torch.cuda.current_stream(wav24.device)
        side = self._side_stream(wav24.device) if self.f0_side else main
        side.wait_stream(main)
        with torch.cuda.stream(side):
            mel, energy = e.mel_energy(wav24)
            # a caller-supplied f0 is shifted on a copy (svc_pitch_shift works in place)
            f0 = self.extract_f0(wav24, T) if f0 is None else f0.to(torch.float64).contiguous().clone()
            mel_src, factor = mel, None
            if shifted:  # the factor shift_f0 is about to apply, from the unshifted f0
                factor = e.pitch_factor(f0, *self.shift_targets(f0.shape[0], singer, key_shift))
            self.shift_f0(f0, singer, key_shift)
            if shifted:
                mel_src, info = e.mel_keyshift(wav24, factor)
        assert mel.shape[1] == T
        content = self.content(wav16, T, wav16_float)
        if index_rate is not None:
            content = self.retrieve(content, singer, index_rate)
        main.wait_stream(side)
        for t in (mel, energy, f0) + ((mel_src, factor, info) if shifted else ()):
            t.record_stream(main)
        cond = e.condition(content, f0, energy, singer)
        if utt_ids is None and (x_T is None or k_step is not None):
            utt_ids = torch.arange(wav24.shape[0], device=wav24.device, dtype=torch.int32)
        if k_step is None:
            x0 = e.diffsvc_sample(cond, fast_inference=fast_inference, speedup=speedup, x_T=x_T, noise=noise,
                                  seed=seed, utt_ids=utt_ids, **(solver_kw or {}))
        else:  # the start mel was computed on the side stream: joined and recorded for this one above
            x0 = e.diffsvc_sample(cond, fast_inference=fast_inference, speedup=speedup, noise=noise, seed=seed,
                                  utt_ids=utt_ids, k_step=k_step, mel_src=mel_src, **(solver_kw or {}))
        wav = e.bigvgan(x0)
        if loudness_mix is not None:  # T * hop <= N: every clip's source covers its output
            e.loudness_match(wav, wav24, mix=loudness_mix, out=wav)
        return ConvertResult(wav=wav, mel=mel, f0=f0, x0=x0, pcm=e.pcm16(wav) if pcm16 else None)

    def convert_many(self, wavs24, wavs16, singers, wavs16_float=None, fast_inference=True, speedup=10, seed=0,
                     utt_ids=None, bucketed=False, pcm16=False, key_shift=0.0, k_step=None, k_step_mel="source",
                     loudness_mix=None, solver=None, solver_steps=20, solver_spacing="logsnr", index_rate=None):
        """Ragged requests: lists of per-utterance device tensors (24 kHz f32 [N_i],
        16 kHz [N16_i], optional float 16 kHz for ContentVec) and singer ids -> list of waveforms f32 [T_i*hop] in
        input order, each bit-identical to converting that clip alone with the same utterance id
        (tests/test_gpu_ragged.py). utt_ids (default: list positions) key the device noise, as in convert().

        Default: ONE padded batch with per-utterance lengths (convert_ragged): every kernel that looks across time
        (STFT, Praat frames, convolutions, anti-aliased activations, fade-out) stops at each utterance's own end.
        bucketed=True instead runs one batch per distinct length.
        pcm16=True: each waveform comes back as save_audio's samples instead, int16 [T_i*hop + 2*(fs//20)]
        (SVCEngine.pcm16 on the batch: each utterance scaled by its own peak).
        key_shift: semitones, a scalar or one per utterance (shift_f0).
        k_step, k_step_mel: shallow diffusion for the whole batch and its start mel, as in convert().
        loudness_mix: loudness envelope transfer for the whole batch, as in convert() (both routes).
        solver, solver_steps, solver_spacing: the sampler for the whole batch, as in convert() (both routes).
        index_rate: feature retrieval for the whole batch, as in convert() (both routes)."""
        k_step = self._check_k_step(k_step)
        shallow = {} if k_step is None else dict(k_step=k_step)  # and the other keywords that are left out when unset
        if check_k_step_mel(k_step_mel, k_step) != "source":
            shallow["k_step_mel"] = k_step_mel
        loudness_mix = check_loudness_mix(loudness_mix)
        if loudness_mix is not None:
            shallow["loudness_mix"] = loudness_mix
        index_rate = self._check_index_rate(index_rate)
        if index_rate is not None:
            shallow["index_rate"] = index_rate
        shallow.update(self._solver_kw(solver, solver_steps, solver_spacing, k_step))
        n = len(wavs24)
        if not (len(wavs16) == n == len(singers)) or (wavs16_float is not None and len(wavs16_float) != n):
            raise ValueError("convert_many: wavs24, wavs16, singers (and wavs16_float) must have one entry per utterance")
        ids = list(range(n)) if utt_ids is None else [int(u) for u in utt_ids]
        shifted = bool(torch.as_tensor(key_shift).any())
        if not bucketed:
            return self.convert_ragged(wavs24, wavs16, singers, wavs16_float=wavs16_float,
                                       fast_inference=fast_inference, speedup=speedup, seed=seed, utt_ids=ids,
                                       pcm16=pcm16, **(dict(key_shift=key_shift) if shifted else {}), **shallow)
        ks = key_shift.tolist() if hasattr(key_shift, "tolist") else key_shift
        ks = [float(k) for k in ks] if isinstance(ks, (list, tuple)) else [float(ks)] * n
        buckets = {}
        for i in range(n):
            key = (int(wavs24[i].shape[-1]), int(wavs16[i].shape[-1]),
                   int(wavs16_float[i].shape[-1]) if wavs16_float is not None else 0)
            buckets.setdefault(key, []).append(i)
        out = [None] * n
        dev = wavs24[0].device
        for key in sorted(buckets):
            idx = buckets[key]
            w24 = torch.stack([wavs24[i].reshape(-1) for i in idx]).contiguous()
            w16 = torch.stack([wavs16[i].reshape(-1) for i in idx]).contiguous()
            w16f = torch.stack([wavs16_float[i].reshape(-1) for i in idx]).contiguous() if wavs16_float is not None else None
            sing = torch.tensor([int(singers[i]) for i in idx], device=dev, dtype=torch.int32)
            uid = torch.tensor([ids[i] for i in idx], device=dev, dtype=torch.int32)
            res = self.convert(w24, w16, sing, fast_inference=fast_inference, speedup=speedup, seed=seed,
                               utt_ids=uid, wav16_float=w16f, pcm16=pcm16,
                               **(dict(key_shift=[ks[i] for i in idx]) if shifted else {}), **shallow)
            for j, i in enumerate(idx):
                out[i] = res.pcm[j] if pcm16 else res.wav[j]
        return out

    @staticmethod
    def _pad_stack(tensors):
        """list of 1-D device tensors -> zero-padded [B, max_len] and the host lengths"""
        lens = [int(t.shape[-1]) for t in tensors]
        out = torch.zeros(len(tensors), max(lens), dtype=tensors[0].dtype, device=tensors[0].device)
        for i, t in enumerate(tensors):
            out[i, :lens[i]] = t.reshape(-1)
        return out, lens

    def ragged_content(self, wavs16, T_b, T, wavs16_float=None):
        """Content features for a ragged batch -> f16 [B, T, D]; rows [b, :T_b[b]] equal convert()'s for that clip
        alone. Whisper runs on zero-padded 16 kHz audio (pad_or_trim pads with zeros, so the padding is exact): one
        whisper_content call that encodes each clip's own windows in one pass and maps them straight into the type's
        columns (whisper_ragged=False: two groups, clips the reference maps in one 30 s window (T_b <= 2812) and long
        clips, per-window as in whisper_content below, each copied into place clip by clip). HuBERT / ContentVec attends over every frame and normalises over time, so it takes the
        lengths: one padded encoder pass and one mapping launch straight into its columns of the result
        (hubert_ragged=False: one pass per exact-length bucket)."""
        e = self.engine
        m = e.cfg.mapper
        types = sorted(m.content_feature)
        widths = [int(m.input_content_dim[t]) for t in types]
        B = len(wavs16)
        dev = wavs16[0].device
        out = torch.zeros(B, T, sum(widths), device=dev, dtype=e.content_dtype)
        col = 0
        for t, w in zip(types, widths):
            if t == "whisper" and self.whisper_ragged:
                w16, n16 = self._pad_stack(wavs16)
                e.whisper_content(w16, n16, list(T_b), T, out=out[:, :, col:col + w])
            elif t == "whisper":
                for group in ([i for i in range(B) if T_b[i] <= MAX_MAPPED], [i for i in range(B) if T_b[i] > MAX_MAPPED]):
                    if not group:
                        continue
                    w16, _ = self._pad_stack([wavs16[i] for i in group])
                    Tg = max(T_b[i] for i in group)
                    c = self.whisper_content(w16, Tg)
                    for j, i in enumerate(group):
                        out[i, :T_b[i], col:col + w] = c[j, :T_b[i]]
            elif t in HUBERT_CONTENT_TYPES:
                src = wavs16 if wavs16_float is None else wavs16_float
                if self.hubert_ragged:
                    w16, n16 = self._pad_stack(src)
                    feats = e.hubert_encode(w16, n_samples=n16)
                    e.map_content(feats, T, rule="hubert", out=out[:, :, col:col + w], frames=T_b,
                                  src_rows=[e.hubert_frames(k) for k in n16])
                    col += w
                    continue
                buckets = {}
                for i in range(B):
                    buckets.setdefault((int(src[i].shape[-1]), T_b[i]), []).append(i)
                for (_, tb), idx in sorted(buckets.items()):
                    feats = e.hubert_encode(torch.stack([src[i].reshape(-1) for i in idx]).contiguous())
                    c = e.map_content(feats, tb, rule="hubert")
                    for j, i in enumerate(idx):
                        out[i, :tb, col:col + w] = c[j]
            else:
                raise ValueError(f"content feature {t!r} is not supported (whisper, {', '.join(HUBERT_CONTENT_TYPES)})")
            col += w
        return out

    def convert_ragged(self, wavs24, wavs16, singers, wavs16_float=None, fast_inference=True, speedup=10, seed=0,
                       utt_ids=None, pcm16=False, key_shift=0.0, k_step=None, k_step_mel="source", loudness_mix=None,
                       solver=None, solver_steps=20, solver_spacing="logsnr", index_rate=None, f0_shifted=None,
                       factor=None):
        """infer.py's sequence for B clips of different lengths as ONE padded batch: the C-ABI stages take the
        per-utterance lengths (include/svc_hip.h, "Ragged batches") and compute each clip exactly as alone.
        -> list of waveforms f32 [T_b * hop], or with pcm16=True of save_audio's samples int16
        [T_b * hop + 2 * (fs // 20)] (svc_pcm16 with the same lengths). Each clip's F0 moves onto its own singer's
        median (shift_f0), then up by key_shift semitones (a scalar or one per clip). k_step: shallow diffusion, as in
        convert(): each clip starts from its own mel (k_step_mel="shifted": its own key-shifted mel, by its own factor),
        noised with its own utterance id's draw. loudness_mix: loudness envelope transfer, as in convert(): each
        clip's T_b * hop output samples against its own 24 kHz source (svc_loudness_match with both length tables),
        before the sample conversion. solver, solver_steps, solver_spacing: the sampler, as in convert().
        index_rate: feature retrieval, as in convert(): each clip's own T_b content rows against its own singer's
        index (one svc_content_retrieve call per enrolled singer of the batch, `sel` marking that singer's clips).
        f0_shifted (None: the call as before): a list with, per clip, None or an f64 [T_b] device tensor of F0 that is
        already pitch-shifted (a chunk's slice of its song's contour, convert_long): such a clip skips the extraction
        and the shift, and when every clip has one no F0 kernel is launched. factor (f64 [B] on the device, needed with
        k_step_mel="shifted" once a clip has an f0_shifted): the factor those clips' start mel is shifted by."""
        k_step = self._check_k_step(k_step)
        check_k_step_mel(k_step_mel, k_step)
        loudness_mix = check_loudness_mix(loudness_mix)
        index_rate = self._check_index_rate(index_rate)
        solver_kw = self._solver_kw(solver, solver_steps, solver_spacing, k_step)
        with self.engine.lock:
            return self._convert_ragged(wavs24, wavs16, singers, wavs16_float, fast_inference, speedup, seed, utt_ids,
                                        pcm16, key_shift, k_step, k_step_mel == "shifted", loudness_mix, solver_kw,
                                        index_rate, f0_shifted, factor)

    def convert_long(self, wavs24, wavs16, singers, wavs16_float=None, clip_s=10.0, context_s=0.64, xfade=1024,
                     search=192, max_batch=32, return_chunks=False, fast_inference=True, speedup=10, seed=0,
                     utt_ids=None, pcm16=False, key_shift=0.0, k_step=None, k_step_mel="source", loudness_mix=None,
                     solver=None, solver_steps=20, solver_spacing="logsnr", index_rate=None):
        """convert_ragged for songs: each is cut into overlapping chunks of clip_s seconds (audio.chunk_plan), the chunks
        of all songs are converted as ragged batches of at most max_batch, and one svc_stitch call joins them (SOLA
        alignment over +-search samples, a crossfade of xfade samples; DESIGN.md "Long-form conversion") -> list of
        waveforms f32 [T_song * hop] (pcm16=True: save_audio's samples). Memory is bounded by max_batch chunks whatever
        a song's length. In order:
          1. the songs' F0 as a ragged batch (extract_f0, pitch_factor where k_step_mel="shifted", shift_f0): one key
             for the whole song, and the voicing path does not restart at a cut;
          2. the chunks through _convert_ragged, each with its slice of that F0 (f0_shifted=), its song's factor and the
             noise id (utterance id << 12) | chunk; no loudness stage and no sample conversion here;
          3. SVCEngine.stitch over all chunks of all songs, reading the vocoder outputs where they lie;
          4. loudness_match (against the songs' own 24 kHz sources) and pcm16 once, on the stitched songs as a ragged
             batch: an envelope and a peak are properties of the song.
        A song that needs no cut is one chunk, converted as convert_ragged converts it with utterance id u << 12. The last
        max(search - 1, 0) samples of a song of several chunks are zero (audio.chunk_plan). The other keywords are
        convert_ragged's; utt_ids must lie in [0, 2^19). return_chunks: -> (waveforms, LongChunks)."""
        from . import audio as A
        k_step = self._check_k_step(k_step)
        shifted = check_k_step_mel(k_step_mel, k_step) == "shifted"
        loudness_mix = check_loudness_mix(loudness_mix)
        index_rate = self._check_index_rate(index_rate)
        solver_kw = self._solver_kw(solver, solver_steps, solver_spacing, k_step)
        e = self.engine
        n = len(wavs24)
        if n < 1 or not (len(wavs16) == n == len(singers)) or (wavs16_float is not None and len(wavs16_float) != n):
            raise ValueError("convert_long: wavs24, wavs16, singers (and wavs16_float) need one entry per song, at least one")
        if int(max_batch) < 1:
            raise ValueError("convert_long: max_batch >= 1")
        ids = list(range(n)) if utt_ids is None else [int(u) for u in utt_ids]
        sids = [int(s) for s in singers]
        wavs24 = [w.reshape(-1) for w in wavs24]
        wavs16 = [w.reshape(-1) for w in wavs16]
        w16f = None if wavs16_float is None else [w.reshape(-1) for w in wavs16_float]
        hop = e.cfg.hop_length
        plans = [A.chunk_plan(int(wavs24[i].shape[0]), e.cfg.fs, hop, e.cfg.n_fft, clip_s, context_s, xfade, search,
                              utt_id=ids[i], n16=int(wavs16[i].shape[0]),
                              n16_float=None if w16f is None else int(w16f[i].shape[0])) for i in range(n)]
        with e.lock:
            w24, n24 = self._pad_stack(wavs24)
            T_s = [p.T_song for p in plans]
            f0 = self.extract_f0(w24, max(T_s), n_samples=n24, T_b=T_s)
            factor = e.pitch_factor(f0, *self.shift_targets(n, sids, key_shift)) if shifted else None
            self.shift_f0(f0, sids, key_shift)
            jobs = [(i, k) for i, p in enumerate(plans) for k in range(p.chunks)]
            rows = []
            for g in range(0, len(jobs), int(max_batch)):
                grp = jobs[g:g + int(max_batch)]
                cut = lambda ws, field: [ws[i][getattr(plans[i], field)[k][0]:getattr(plans[i], field)[k][1]] for i, k in grp]
                fac = None if factor is None else factor[torch.tensor([i for i, _ in grp], device=factor.device)]
                rows += self._convert_ragged(
                    cut(wavs24, "rows24"), cut(wavs16, "rows16"), [sids[i] for i, _ in grp],
                    None if w16f is None else cut(w16f, "rows16_float"), fast_inference, speedup, seed,
                    [plans[i].noise_ids[k] for i, k in grp], False, 0.0, k_step, shifted, None, solver_kw, index_rate,
                    [f0[i, plans[i].start[k]:plans[i].start[k] + plans[i].frames[k]] for i, k in grp], fac)
            S = max(T_s) * hop
            merged = A.merge_stitch_plans([p.stitch for p in plans], S)
            out = torch.zeros(n, S, device=w24.device, dtype=torch.float32)
            _, shifts = e.stitch(rows, merged, out=out, return_shifts=True)
            n_out = [t * hop for t in T_s]
            info = None
            if return_chunks:
                first = [sum(p.chunks for p in plans[:i]) for i in range(n + 1)]
                info = LongChunks(plans, [rows[first[i]:first[i + 1]] for i in range(n)],
                                  [shifts[first[i]:first[i + 1]] for i in range(n)], [f0[i, :T_s[i]] for i in range(n)],
                                  [out[i, :n_out[i]].clone() for i in range(n)]
                                  if loudness_mix is not None else [out[i, :n_out[i]] for i in range(n)])
            if loudness_mix is not None:
                e.loudness_match(out, w24, n_samples=n_out, src_samples=n24, mix=loudness_mix, out=out)
            if pcm16:
                pcm = e.pcm16(out, n_samples=n_out)
                sil2 = pcm.shape[1] - out.shape[1]
                wavs = [pcm[i, :n_out[i] + sil2] for i in range(n)]
            else:
                wavs = [out[i, :n_out[i]] for i in range(n)]
        return (wavs, info) if return_chunks else wavs

    def convert_files(self, sources, singers, fast_inference=True, speedup=10, seed=0, utt_ids=None, pcm16=False,
                      float16k=None, key_shift=0.0, k_step=None, k_step_mel="source", loudness_mix=None, solver=None,
                      solver_steps=20, solver_spacing="logsnr", index_rate=None, clip_s=None, context_s=0.64):
        """convert_ragged from wav files (paths, bytes or memoryviews): audio.load_batch decodes and resamples the whole
        batch in one device stage (svc_load_pcm), then the batch is converted as convert_ragged converts it.
        float16k: the load stage also writes the float 16 kHz rows (audio.load_contentvec_audio of each file) and
        HuBERT / ContentVec reads them as `wavs16_float`, what utils/hubert.py:137-143 feeds it; None (default): when
        the configuration names a HuBERT content type (wants_float16k); False: HuBERT is fed Whisper's int16-grid rows.
        Without a HuBERT type and with None or False, load_batch is called without the keyword.
        loudness_mix: as in convert_ragged(), against the 24 kHz rows the load stage wrote.
        solver, solver_steps, solver_spacing: the sampler, as in convert(). index_rate: as in convert_ragged().
        clip_s (None: every file is one utterance, the call as before): the files are converted as convert_long
        converts songs, in chunks of clip_s seconds with context_s seconds of context on each side."""
        from . import audio as A
        k_step = self._check_k_step(k_step)
        check_k_step_mel(k_step_mel, k_step)
        loudness_mix = check_loudness_mix(loudness_mix)
        index_rate = self._check_index_rate(index_rate)
        solver_kw = self._solver_kw(solver, solver_steps, solver_spacing, k_step)
        if wants_float16k(self.engine.cfg) if float16k is None else float16k:
            wavs24, wavs16, wavs16_float = A.load_batch(sources, self.engine.cfg.fs, self.engine, float16k=True)
        else:
            wavs24, wavs16 = A.load_batch(sources, self.engine.cfg.fs, self.engine)
            wavs16_float = None
        if clip_s is not None:
            return self.convert_long(wavs24, wavs16, singers, wavs16_float=wavs16_float, clip_s=clip_s,
                                     context_s=context_s, fast_inference=fast_inference, speedup=speedup, seed=seed,
                                     utt_ids=utt_ids, pcm16=pcm16, key_shift=key_shift, k_step=k_step,
                                     k_step_mel=k_step_mel, loudness_mix=loudness_mix, index_rate=index_rate,
                                     **solver_kw)
        return self.convert_ragged(wavs24, wavs16, singers, wavs16_float=wavs16_float, fast_inference=fast_inference,
                                   speedup=speedup, seed=seed, utt_ids=utt_ids, pcm16=pcm16, key_shift=key_shift,
                                   **({} if k_step is None else dict(k_step=k_step)),
                                   **({} if k_step_mel == "source" else dict(k_step_mel=k_step_mel)),
                                   **({} if loudness_mix is None else dict(loudness_mix=loudness_mix)),
                                   **({} if index_rate is None else dict(index_rate=index_rate)), **solver_kw)

    def _convert_ragged(self, wavs24, wavs16, singers, wavs16_float, fast_inference, speedup, seed, utt_ids,
                        pcm16=False, key_shift=0.0, k_step=None, shifted=False, loudness_mix=None, solver_kw=None,
                        index_rate=None, f0_shifted=None, factor=None):
        e = self.engine
        n = len(wavs24)
        ids = list(range(n)) if utt_ids is None else [int(u) for u in utt_ids]
        w24, n24 = self._pad_stack(wavs24)
        dev = w24.device
        T_b = [mel_frames(k, e.cfg.n_fft, e.cfg.hop_length) for k in n24]
        T = max(T_b)
        main = torch.cuda.current_stream(dev)
        side = self._side_stream(dev) if self.f0_side else main
        side.wait_stream(main)
        with torch.cuda.stream(side):
            mel, energy = e.mel_energy(w24, n_samples=n24)
            mel_src = mel
            if f0_shifted is None:
                f0 = self.extract_f0(w24, T, n_samples=n24, T_b=T_b)
                factor = None
                if shifted:  # as in _convert
                    factor = e.pitch_factor(f0, *self.shift_targets(n, [int(s) for s in singers], key_shift))
                self.shift_f0(f0, [int(s) for s in singers], key_shift)
            else:
                f0, factor = self._f0_supplied(w24, n24, T_b, [int(s) for s in singers], key_shift, f0_shifted, factor,
                                               shifted)
            if shifted:
                mel_src, info = e.mel_keyshift(w24, factor, n_samples=n24)
        content = self.ragged_content(list(wavs16), T_b, T, wavs16_float)
        if index_rate is not None:
            content = self.retrieve(content, [int(s) for s in singers], index_rate, frames=T_b)
        main.wait_stream(side)
        for t in (mel, energy, f0) + ((mel_src, factor, info) if shifted else ()):
            if t.is_cuda:
                t.record_stream(main)
        sing = torch.tensor([int(s) for s in singers], device=dev, dtype=torch.int32)
        cond = e.condition(content, f0, energy, sing)
        uid = torch.tensor(ids, device=dev, dtype=torch.int32)
        shallow = {} if k_step is None else dict(k_step=k_step, mel_src=mel_src)  # joined and recorded above
        x0 = e.diffsvc_sample(cond, fast_inference=fast_inference, speedup=speedup, seed=seed, utt_ids=uid, frames=T_b,
                              **shallow, **(solver_kw or {}))
        wav = e.bigvgan(x0, frames=T_b)
        hop = e.cfg.hop_length
        if loudness_mix is not None:
            e.loudness_match(wav, w24, n_samples=[t * hop for t in T_b], src_samples=n24, mix=loudness_mix, out=wav)
        if pcm16:
            pcm = e.pcm16(wav, n_samples=[t * hop for t in T_b])
            sil2 = pcm.shape[1] - wav.shape[1]  # both silences
            return [pcm[i, :T_b[i] * hop + sil2] for i in range(n)]
        return [wav[i, :T_b[i] * hop] for i in range(n)]

    def _f0_supplied(self, w24, n24, T_b, singers, key_shift, f0_shifted, factor, shifted):
        """_convert_ragged's F0 with f0_shifted given -> (f0 f64 [B, T], the factor f64 [B] or None): a clip with an
        entry takes it as it is (and its `factor`); the others, if any, go through extract_f0, pitch_factor and shift_f0
        as a ragged batch of their own (each clip is computed exactly as alone, so their values are the usual ones)."""
        e = self.engine
        n, T = len(T_b), max(T_b)
        if len(f0_shifted) != n:
            raise ValueError(f"{len(f0_shifted)} f0_shifted entries for a batch of {n}")
        have = [i for i in range(n) if f0_shifted[i] is not None]
        need = [i for i in range(n) if f0_shifted[i] is None]
        for i in have:
            if f0_shifted[i].dtype != torch.float64 or tuple(f0_shifted[i].shape) != (T_b[i],):
                raise ValueError(f"f0_shifted[{i}] must be f64 [{T_b[i]}]")
        if shifted and have and (factor is None or factor.dtype != torch.float64 or factor.numel() != n):
            raise ValueError(f"k_step_mel='shifted' with f0_shifted needs factor, f64 [{n}]")
        f0 = torch.zeros(n, T, device=w24.device, dtype=torch.float64)
        for i in have:
            f0[i, :T_b[i]] = f0_shifted[i]
        fac = factor.reshape(-1).clone() if shifted and have else None
        if need:
            ks = key_shift.tolist() if hasattr(key_shift, "tolist") else key_shift
            ks = [float(k) for k in ks] if isinstance(ks, (list, tuple)) else [float(ks)] * n
            Ts = max(T_b[i] for i in need)
            sub = w24[torch.tensor(need, device=w24.device)].contiguous()
            f0s = self.extract_f0(sub, Ts, n_samples=[n24[i] for i in need], T_b=[T_b[i] for i in need])
            targets = self.shift_targets(len(need), [singers[i] for i in need], [ks[i] for i in need])
            if shifted:
                fs_ = e.pitch_factor(f0s, *targets)
                if fac is None:
                    fac = fs_ if len(need) == n else None
                else:
                    fac[torch.tensor(need, device=w24.device)] = fs_
            e.pitch_shift(f0s, *targets)
            for j, i in enumerate(need):
                f0[i, :T_b[i]] = f0s[j, :T_b[i]]
        return f0, fac

    def resynthesize(self, wav24, n_samples=None):
        """Copy-synthesis through the vocoder alone (how a vocoder checkpoint is judged on its own): wav24 f32 [B, N]
        -> mel_energy -> mel_normalize -> bigvgan -> wav f32 [B, T * hop]; no content encoder, conditioner or sampler
        runs, and the engine needs only its vocoder. n_samples (ragged batch, host ints [B]): clip b is
        wav24[b, :n_samples[b]] and its waveform mel_frames(n_samples[b]) * hop samples, zeros after."""
        e = self.engine
        with e.lock:
            frames = None
            if n_samples is not None:
                frames = [mel_frames(int(k), e.cfg.n_fft, e.cfg.hop_length) for k in n_samples]
            mel, _ = e.mel_energy(wav24, n_samples=n_samples)
            return e.bigvgan(e.mel_normalize(mel, frames=frames), frames=frames)
