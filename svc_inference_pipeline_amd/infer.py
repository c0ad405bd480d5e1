"""Command-line counterpart of the reference's infer.py (infer.py:24-91): source wav + target singer ->
converted wav, on one MI355X through libsvc_hip.so.

    python -m svc_inference_pipeline_amd.infer --wav test_set/1100000814.wav --singer svcc_CDF1 \\
        --mapper-ckpt mapper.pt --vocoder-ckpt vocoder.pt --whisper-ckpt medium.pt [--fast] [--out gen/x.wav]
    python -m svc_inference_pipeline_amd.infer --wav a.wav b.wav c.wav ...   # several files: one ragged batch
    python -m svc_inference_pipeline_amd.infer --singer-f0 f0.json --singer svcc_CDF1 --enroll r1.wav r2.wav ...
        # measure the singer's voiced F0 median from the singer's own recordings and keep it in f0.json
    python -m svc_inference_pipeline_amd.infer --singer-f0 f0.json --key 2 --wav a.wav ...   # use it; 2 semitones up
    python -m svc_inference_pipeline_amd.infer --k-step 300 --fast --wav a.wav ...   # shallow diffusion from step 300
    python -m svc_inference_pipeline_amd.infer --clip 10 --fast --wav song.wav ...   # a long file in 10 s chunks
    python -m svc_inference_pipeline_amd.infer --resynth --vocoder-ckpt vocoder.pt --wav a.wav   # vocoder only

Same sequence as the reference: acoustic features (mel, energy, Praat F0) -> pitch shift to the target
singer -> Whisper (and / or ContentVec, --hubert-ckpt) content features -> DiffSVC sampler (DDPM-1000 by default, PLMS with --fast, as
svc_model_inference's fast_inference) -> de-normalisation -> BigVGAN -> fade -> 16-bit wav (peak 0.9, 50 ms of
silence each side). Checkpoint paths default to the config's svc_model_path / vocoder_model_path. Without
checkpoints the run needs --random-weights (seeded weights of the reference architectures: plumbing and
timing only, the audio is noise).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

from . import audio as A
from . import config as C
from . import weights as W
from .pipeline import SVCPipeline, hubert_content_type, wants_float16k
from .runtime import K_STEP_MELS, SVCEngine, check_k_step, check_k_step_mel, mel_frames
from .singers import INDEX_COMPACT, SingerF0Table, check_index_compact, check_index_rate


def build_engine(cfg, device=0, mapper_ckpt=None, vocoder_ckpt=None, whisper_ckpt=None, random_weights=None, seed=0,
                 hubert_ckpt=None):
    """Engine from the reference's checkpoints, or from seeded random weights when random_weights names a
    Whisper size ("medium" or "tiny-test"); checkpoints and random weights do not mix.
    When the config names a HuBERT / ContentVec content type the engine needs that model too: hubert_ckpt (fairseq's
    layout, weights.load_checkpoints), or with random_weights a seeded state of HUBERT_DIMS["tiny-test"] for
    "tiny-test" and of HUBERT_DIMS["contentvec"] otherwise (the type's input_content_dim is set to its width)."""
    types = list(cfg.mapper.content_feature)
    cv = hubert_content_type(cfg)
    if random_weights:
        kw = {}
        if "whisper" in types:
            dims = W.WHISPER_DIMS[random_weights]
            if dims["n_audio_state"] != cfg.mapper.input_content_dim["whisper"]:
                cfg.mapper.input_content_dim["whisper"] = dims["n_audio_state"]
            kw["whisper_state"] = W.make_whisper_state(dims, seed)
        if cv:
            hd = W.HUBERT_DIMS["tiny-test" if random_weights == "tiny-test" else "contentvec"]
            cfg.mapper.input_content_dim[cv] = hd["final_dim"]
            kw.update(hubert_state=W.make_hubert_state(hd, seed), hubert_output_layer=hd["output_layer"])
        return SVCEngine(cfg, device, mapper_state=W.make_mapper_state(cfg.mapper, seed),
                         vocoder_state=W.make_vocoder_state(cfg.vocoder, seed), **kw)
    if cv and not hubert_ckpt:
        raise SystemExit(f"the config names the content feature {cv!r}: need --hubert-ckpt (the ContentVec / HuBERT "
                         "checkpoint; default: the config's contentVec_model), or --random-weights")
    need_whisper = "whisper" in types
    if not (mapper_ckpt and vocoder_ckpt and (whisper_ckpt or not need_whisper)):
        raise SystemExit("need --mapper-ckpt, --vocoder-ckpt and --whisper-ckpt (or --random-weights)")
    st = W.load_checkpoints(mapper_ckpt, vocoder_ckpt, whisper_ckpt if need_whisper else None,
                            hubert_path=hubert_ckpt if cv else None)
    kw = {}
    if cv:  # utils/hubert.py:42 output_layer=9, or every layer of a shallower model
        kw.update(hubert_state=st["hubert"],
                  hubert_output_layer=W.hubert_dims_from_state(st["hubert"])["output_layer"])
    return SVCEngine(cfg, device, whisper_state=st.get("whisper"), mapper_state=st["mapper"],
                     vocoder_state=st["vocoder"], **kw)


def build_vocoder_engine(cfg, device=0, vocoder_ckpt=None, random_weights=None, seed=0):
    """--resynth's engine: the vocoder and the mel statistics, no mapper and no content encoder."""
    if random_weights:
        return SVCEngine(cfg, device, vocoder_state=W.make_vocoder_state(cfg.vocoder, seed))
    if not vocoder_ckpt:
        raise SystemExit("--resynth needs --vocoder-ckpt (or --random-weights)")
    return SVCEngine(cfg, device, vocoder_state=W.load_checkpoints(vocoder_path=vocoder_ckpt)["vocoder"])


def resynth_files(engine, cfg, wav_paths):
    """--resynth: every file's own mel through the vocoder alone (SVCPipeline.resynthesize, one ragged batch) ->
    list of (save_audio's int16 samples, T_i)."""
    w24 = A.load_batch(list(wav_paths), cfg.fs, engine)[0]
    w24 = [w.reshape(-1) for w in w24]
    pad, n24 = SVCPipeline._pad_stack(w24)
    wav = SVCPipeline(engine).resynthesize(pad, n_samples=n24)
    hop = cfg.hop_length
    T_b = [mel_frames(k, cfg.n_fft, hop) for k in n24]
    pcm = engine.pcm16(wav, n_samples=[t * hop for t in T_b])
    sil2 = pcm.shape[1] - wav.shape[1]
    return [(pcm[i, :t * hop + sil2].cpu().numpy(), t) for i, t in enumerate(T_b)]


def convert_file(engine, cfg, wav_path, singer_name, fast_inference=False, speedup=10, seed=0, device="cuda",
                 f0_method="parselmouth", pcm16=False, key_shift=0.0, k_step=None, k_step_mel="source",
                 loudness_mix=None, solver=None, solver_steps=20, index_rate=None):
    """One file through the GPU path -> (f32 waveform [T*hop] before save_audio's normalisation, T); with pcm16=True
    the waveform is save_audio's int16 samples instead (converted on the GPU, svc_pcm16). k_step, k_step_mel: shallow diffusion
    and its start mel; loudness_mix: loudness envelope transfer; solver, solver_steps: DPM-Solver++(2M) / DDIM instead of
    DDPM / PLMS; index_rate: feature retrieval against the singer's enrolled index (SVCPipeline.convert)."""
    # utils/audio.py:10-55 and whisper_extractor/audio.py:22-49 in one device stage (raises on non-finite samples)
    wav16f = None
    if wants_float16k(cfg):  # and utils/hubert.py:137-143's float 16 kHz copy from the same stage
        (wav24,), (wav16,), (wav16f,) = A.load_batch([wav_path], cfg.fs, engine, float16k=True)
    else:
        (wav24,), (wav16,) = A.load_batch([wav_path], cfg.fs, engine)
    singers = C.load_singers(cfg)
    if singer_name not in singers:
        raise KeyError(f"unknown singer {singer_name!r}; known: {sorted(singers)}")
    singer = torch.tensor([int(singers[singer_name])], dtype=torch.int32, device=device)  # utils/util.py:49-54
    utt = torch.zeros(1, dtype=torch.int32, device=device)
    res = SVCPipeline(engine, f0_method=f0_method).convert(wav24[None].contiguous(), wav16[None].contiguous(), singer,
                                      fast_inference=fast_inference, speedup=speedup, seed=seed, utt_ids=utt,
                                      wav16_float=None if wav16f is None else wav16f[None].contiguous(),
                                      pcm16=pcm16, key_shift=key_shift,
                                      **({} if k_step is None else dict(k_step=k_step)),
                                      **({} if k_step_mel == "source" else dict(k_step_mel=k_step_mel)),
                                      **({} if loudness_mix is None else dict(loudness_mix=loudness_mix)),
                                      **({} if index_rate is None else dict(index_rate=index_rate)),
                                      **({} if solver is None else dict(solver=solver, solver_steps=solver_steps)))
    return (res.pcm if pcm16 else res.wav)[0].cpu().numpy(), res.mel.shape[1]


def convert_files(engine, cfg, wav_paths, singer_name, fast_inference=False, speedup=10, seed=0, device="cuda",
                  f0_method="parselmouth", pcm16=False, key_shift=0.0, k_step=None, k_step_mel="source",
                  loudness_mix=None, solver=None, solver_steps=20, index_rate=None, clip_s=None, context_s=0.64):
    """Several files as ONE ragged batch (SVCPipeline.convert_many, per-utterance lengths through the C-ABI) ->
    list of (f32 waveform [T_i*hop], T_i); file i uses utterance id i, so file 0 equals convert_file's result.
    pcm16=True: save_audio's int16 samples [T_i*hop + 2*(fs//20)] instead of each f32 waveform.
    clip_s (--clip; None: each file is one utterance): the files are converted in overlapping chunks of clip_s seconds
    with context_s seconds of context and stitched (SVCPipeline.convert_long)."""
    singers = C.load_singers(cfg)
    if singer_name not in singers:
        raise KeyError(f"unknown singer {singer_name!r}; known: {sorted(singers)}")
    w16f = None  # all files decoded and resampled in one device stage
    if wants_float16k(cfg):
        w24, w16, w16f = A.load_batch(list(wav_paths), cfg.fs, engine, float16k=True)
    else:
        w24, w16 = A.load_batch(list(wav_paths), cfg.fs, engine)
    sid = int(singers[singer_name])
    pipe = SVCPipeline(engine, f0_method=f0_method)
    call = pipe.convert_many if clip_s is None else pipe.convert_long
    long_kw = {} if clip_s is None else dict(clip_s=clip_s, context_s=context_s)
    wavs = call(w24, w16, [sid] * len(w24), wavs16_float=w16f, **long_kw, fast_inference=fast_inference,
                speedup=speedup, seed=seed, pcm16=pcm16, key_shift=key_shift,
                **({} if k_step is None else dict(k_step=k_step)),
                **({} if k_step_mel == "source" else dict(k_step_mel=k_step_mel)),
                **({} if loudness_mix is None else dict(loudness_mix=loudness_mix)),
                **({} if index_rate is None else dict(index_rate=index_rate)),
                **({} if solver is None else dict(solver=solver, solver_steps=solver_steps)))
    hop = cfg.hop_length
    sil2 = 2 * (cfg.fs // 20) if pcm16 else 0
    return [(w.cpu().numpy(), (int(w.shape[0]) - sil2) // hop) for w in wavs]


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--wav", default=None, nargs="+",
                    help="one or more source files; several are converted as one ragged GPU batch (may be left out "
                         "with --enroll)")
    ap.add_argument("--singer-f0", default=None, metavar="FILE",
                    help="per-singer F0 medians (JSON, singers.SingerF0Table): loaded when the file exists, and saved "
                         "after an enrolment")
    ap.add_argument("--enroll", default=None, nargs="+", metavar="WAV",
                    help="recordings of --singer: their voiced F0 median becomes that singer's pitch target; exits "
                         "after the enrolment when no --wav is given")
    ap.add_argument("--key", type=float, default=0.0, metavar="SEMITONES",
                    help="key shift on top of the shift to the singer's median")
    ap.add_argument("--singer", default="svcc_CDF1")
    ap.add_argument("--out", default=None, help="default gen/<wav stem>_<singer>.wav (infer.py:28); one file only")
    ap.add_argument("--config", default=None, help="reference-format config.json (default: the packaged one)")
    ap.add_argument("--fast", action="store_true", help="PLMS (fast_inference=True) instead of DDPM-1000")
    ap.add_argument("--speedup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--k-step", type=int, default=None, metavar="K",
                    help="shallow diffusion (Diff-SVC's k_step): noise the source's own mel forward to step K and "
                         "denoise from there instead of from pure noise (1..1000; with and without --fast)")
    ap.add_argument("--k-step-mel", default="source", choices=K_STEP_MELS,
                    help="with --k-step, the mel the sampler starts from: the source's own, or 'shifted': its "
                         "key-shifted mel, moved by the same factor as the F0 (singer median and --key), so that its "
                         "harmonics sit where the conditioner's pitch asks for them")
    ap.add_argument("--solver", default=None, choices=sorted(C.SOLVERS),
                    help="a multistep ODE solver instead of DDPM / PLMS: DPM-Solver++(2M) (dpmpp2m) or its first-order "
                         "case DDIM (ddim), one denoiser call per step, from noise or with --k-step from the noised "
                         "source mel (--fast and --speedup are then not used). Output quality at a given step count "
                         "has been checked on an analytic denoiser and random weights only")
    ap.add_argument("--solver-steps", type=int, default=20, metavar="N",
                    help="with --solver, the number of timesteps, spaced evenly in log-SNR (default 20)")
    ap.add_argument("--loudness-mix", type=float, default=None, metavar="X",
                    help="loudness envelope transfer: the converted voice takes the source's slow RMS envelope; 0 "
                         "gives it the source's envelope, 1 leaves it unchanged (default: the step is not run)")
    ap.add_argument("--clip", type=float, default=None, metavar="SECONDS",
                    help="long-form conversion: each file is cut into overlapping chunks of this many seconds, the "
                         "chunks are converted as one ragged batch with the file's own F0 and key, then aligned (SOLA) "
                         "and crossfaded back together on the GPU; memory no longer grows with the file's length "
                         "(default: a file is one utterance)")
    ap.add_argument("--clip-context", type=float, default=None, metavar="SECONDS",
                    help="with --clip: the context converted on each side of a chunk (default 0.64)")
    ap.add_argument("--index", action="store_true",
                    help="with --enroll: also build the singer's retrieval index from the content frames of the "
                         "recordings (needs --singer-index to keep it)")
    ap.add_argument("--index-max-rows", type=int, default=None, metavar="N",
                    help="with --enroll --index: an index of more than N content frames is compacted to N rows "
                         "(default: every frame is kept)")
    ap.add_argument("--index-compact", default=None, choices=INDEX_COMPACT,
                    help="with --enroll --index: how a larger index is brought down to --index-max-rows: 'stride' "
                         "keeps rows floor(i * frames / N) (the default), 'kmeans' replaces the frames by the N k-means "
                         "centroids of all of them (on the GPU). Audible benefit is unverified")
    ap.add_argument("--index-iters", type=int, default=None, metavar="N",
                    help="with --index-compact kmeans: rounds of Lloyd's iteration, 0..1000 (default 10)")
    ap.add_argument("--singer-index", default=None, metavar="FILE",
                    help="per-singer retrieval indexes (.npz, singers.SingerIndexTable): loaded when the file exists, "
                         "and saved after --enroll --index")
    ap.add_argument("--index-rate", type=float, default=None, metavar="X",
                    help="feature retrieval (RVC's index_rate): each content frame becomes X * (the weighted mean of "
                         "its nearest frames of the singer's enrolled index) + (1 - X) * itself; 0..1 (default: the "
                         "step is not run). Audible benefit is unverified: no trained checkpoint has been run with it")
    ap.add_argument("--resynth", action="store_true",
                    help="copy-synthesis: each file's own mel through the vocoder alone (judges a vocoder checkpoint; "
                         "needs no mapper or content checkpoint); output gen/<wav stem>_resynth.wav")
    ap.add_argument("--mapper-ckpt", default=None)
    ap.add_argument("--vocoder-ckpt", default=None)
    ap.add_argument("--whisper-ckpt", default=None)
    ap.add_argument("--hubert-ckpt", default=None,
                    help="ContentVec / HuBERT checkpoint in fairseq's layout, for a config whose content features name "
                         "contentvec (default: the config's contentVec_model)")
    ap.add_argument("--random-weights", default=None, choices=sorted(W.WHISPER_DIMS))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--f0-method", default="parselmouth", choices=("parselmouth", "pyin"),
                    help="F0 extractor: Praat AC (the reference's infer.py) or pYIN (utils/f0.py:95-117; follows "
                         "librosa 0.10.1's pyin, parity-unpinned: librosa is not installed here)")
    return ap


def enroll_singer(engine, cfg, singer_name, wav_paths, f0_method="parselmouth", table_path=None, index=False,
                  index_path=None, index_max_rows=None, index_compact=None, index_iters=None):
    """--enroll: SVCPipeline.enroll of the named singer from wav files -> the table entry; the table is saved to
    table_path where given. index: also the singer's retrieval index (--index), saved to index_path where given;
    index_max_rows / index_compact / index_iters: SVCPipeline.enroll's, passed on where given."""
    singers = C.load_singers(cfg)
    if singer_name not in singers:
        raise KeyError(f"unknown singer {singer_name!r}; known: {sorted(singers)}")
    kw = dict(index=True) if index else {}
    kw.update({k: v for k, v in (("index_max_rows", index_max_rows), ("index_compact", index_compact),
                                 ("index_iters", index_iters)) if v is not None})
    entry = SVCPipeline(engine, f0_method=f0_method).enroll(int(singers[singer_name]), sources=list(wav_paths), **kw)
    if table_path:
        engine.singer_f0.save(table_path)
    if index and index_path:
        engine.singer_index.save(index_path)
    return entry


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.wav and not args.enroll:
        ap.error("need --wav (files to convert) or --enroll (recordings of --singer)")

    cfg = C.load_config(args.config) if args.config else C.load_config()
    mapper = args.mapper_ckpt or getattr(cfg, "svc_model_path", None)
    vocoder = args.vocoder_ckpt or getattr(cfg, "vocoder_model_path", None)
    if args.resynth:
        if not args.wav:
            ap.error("--resynth needs --wav")
        if args.out and len(args.wav) > 1:
            raise SystemExit("--out names one output file: omit it when converting several files")
        print("Loading vocoder...", flush=True)
        engine = build_vocoder_engine(cfg, args.device, vocoder, args.random_weights, args.seed)
        for path, (pcm, _) in zip(args.wav, resynth_files(engine, cfg, args.wav)):
            out = args.out or os.path.join("gen", f"{os.path.splitext(os.path.basename(path))[0]}_resynth.wav")
            A.write_wav_pcm16(out, pcm, cfg.fs)
            print("Saving", out, flush=True)
        engine.close()
        return 0
    try:
        check_k_step(args.k_step, cfg)
    except ValueError as exc:
        ap.error(f"--k-step: {exc}")
    try:
        check_k_step_mel(args.k_step_mel, args.k_step)
    except ValueError:
        ap.error("--k-step-mel shifted needs --k-step")
    try:
        A.check_loudness_mix(args.loudness_mix)
    except ValueError as exc:
        ap.error(f"--loudness-mix: {exc}")
    try:
        check_index_rate(args.index_rate)
    except ValueError as exc:
        ap.error(f"--index-rate: {exc}")
    if args.clip_context is not None and args.clip is None:
        ap.error("--clip-context needs --clip")
    if args.clip is not None:
        try:
            A.chunk_plan(cfg.fs, cfg.fs, cfg.hop_length, cfg.n_fft, args.clip,
                         0.64 if args.clip_context is None else args.clip_context)
        except ValueError as exc:
            ap.error(f"--clip / --clip-context: {exc}")
    if args.index and not args.enroll:
        ap.error("--index needs --enroll")
    for flag, val in (("--index-max-rows", args.index_max_rows), ("--index-compact", args.index_compact),
                      ("--index-iters", args.index_iters)):
        if val is not None and not (args.enroll and args.index):
            ap.error(f"{flag} needs --enroll --index")
    if args.index_max_rows is not None and args.index_max_rows < 1:
        ap.error("--index-max-rows: at least 1")
    try:
        check_index_compact(args.index_compact or "stride", 10 if args.index_iters is None else args.index_iters)
    except ValueError as exc:
        ap.error(f"--index-iters: {exc}")
    try:
        if C.check_solver(args.solver, args.solver_steps) is not None:
            C.solver_timesteps(cfg, args.k_step, args.solver_steps)
    except ValueError as exc:
        ap.error(f"--solver-steps: {exc}")
    print("Loading mapper and vocoder...", flush=True)
    hubert = args.hubert_ckpt or getattr(cfg, "contentVec_model", None)
    engine = build_engine(cfg, args.device, mapper, vocoder, args.whisper_ckpt, args.random_weights, args.seed,
                          hubert_ckpt=hubert)
    if args.singer_f0 and os.path.exists(args.singer_f0):
        engine.singer_f0 = SingerF0Table.load(args.singer_f0)
    if args.singer_index and os.path.exists(args.singer_index):
        engine.load_singer_index(args.singer_index)
    if args.enroll:
        ent = enroll_singer(engine, cfg, args.singer, args.enroll, args.f0_method, args.singer_f0, index=args.index,
                            index_path=args.singer_index, index_max_rows=args.index_max_rows,
                            index_compact=args.index_compact, index_iters=args.index_iters)
        print(f"Enrolled {args.singer}: voiced F0 median {ent['median']:.3f} Hz over {ent['voiced']} voiced of "
              f"{ent['frames']} frames, {ent['n_utts']} file(s)", flush=True)
        if not args.wav:
            engine.close()
            return 0
    if args.out and len(args.wav) > 1:
        raise SystemExit("--out names one output file: omit it when converting several files")
    t0 = time.time()
    print("Converting...", flush=True)
    dev = f"cuda:{args.device}"
    if len(args.wav) == 1 and args.clip is None:
        results = [convert_file(engine, cfg, args.wav[0], args.singer, args.fast, args.speedup, args.seed, device=dev,
                                f0_method=args.f0_method, pcm16=True, key_shift=args.key, k_step=args.k_step,
                                k_step_mel=args.k_step_mel, loudness_mix=args.loudness_mix, solver=args.solver,
                                solver_steps=args.solver_steps, index_rate=args.index_rate)]
    else:
        results = convert_files(engine, cfg, args.wav, args.singer, args.fast, args.speedup, args.seed, device=dev,
                                f0_method=args.f0_method, pcm16=True, key_shift=args.key, k_step=args.k_step,
                                k_step_mel=args.k_step_mel, loudness_mix=args.loudness_mix, solver=args.solver,
                                solver_steps=args.solver_steps, index_rate=args.index_rate,
                                **({} if args.clip is None else dict(
                                    clip_s=args.clip, context_s=0.64 if args.clip_context is None else args.clip_context)))
    print(f"Using time: {time.time() - t0:.3f}s ({sum(T for _, T in results)} frames, {len(results)} file(s))",
          flush=True)
    for path, (pcm, _) in zip(args.wav, results):  # save_audio's samples, already converted on the GPU
        out = args.out or os.path.join("gen", f"{os.path.splitext(os.path.basename(path))[0]}_{args.singer}.wav")
        A.write_wav_pcm16(out, pcm, cfg.fs)
        print("Saving", out, flush=True)
    engine.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
