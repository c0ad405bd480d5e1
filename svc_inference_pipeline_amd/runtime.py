"""Host-side engine: owns one libsvc_hip context per device and exposes each hot-path stage on
torch device tensors (PyTorch supplies device memory and the HIP stream; all compute is in
libsvc_hip.so). Layout of every tensor is time-major [B, T, C] (row = b*T + t).
"""
import ctypes
import os
import threading

import numpy as np
import torch

from . import _lib
from . import weights as W
from .config import SOLVERS, check_solver, load_stats, noise_schedule, solver_timesteps
from .singers import SingerF0Table, SingerIndexTable, check_index_rate, content_signature

MODE_DDPM, MODE_PLMS = 0, 1


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "libsvc_hip takes contiguous device tensors"
    return ctypes.c_void_p(t.data_ptr())


def _opt_ptr(t):
    """_ptr of an optional device tensor, made contiguous."""
    return _ptr(t.contiguous()) if t is not None else None


def _draw_keys(utt_ids, draws, B, device):
    """utt_ids as contiguous int32 (None stays None). What the device draws is keyed by utterance id: where it will
    draw (`draws`), missing ids default to the batch positions."""
    if utt_ids is None and draws:
        utt_ids = torch.arange(B, device=device, dtype=torch.int32)
    return utt_ids.to(torch.int32).contiguous() if utt_ids is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host_lengths(lengths, B, ctype):
    """Ragged-batch length table for the C-ABI: a host ctypes array of B entries, or None (uniform batch)."""
    if lengths is None:
        return None
    vals = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if len(vals) != B:
        raise ValueError(f"{len(vals)} lengths for a batch of {B}")
    return (ctype * B)(*vals)


def _host_f64(v):
    return v.detach().cpu().numpy().astype(np.float64) if isinstance(v, torch.Tensor) else np.asarray(v, np.float64)


def _host_table(values, B, what):
    """A host f64 table of B entries for the C-ABI from a scalar (repeated) or B values."""
    a = _host_f64(values).reshape(-1) if np.ndim(_host_f64(values)) else np.full(B, float(values))
    if a.shape[0] != B:
        raise ValueError(f"{a.shape[0]} {what} values for a batch of {B}")
    return (ctypes.c_double * B)(*a.tolist())


def mel_frames(n_samples, n_fft=1024, hop=256):
    """utils/mel.py:148-167 frame count (reflect pad (n_fft-hop)/2 each side, center=False)."""
    return (n_samples + (n_fft - hop) - n_fft) // hop + 1


def check_k_step(k_step, cfg=None):
    """Shallow diffusion's k_step as an int in [1, steps] (steps: the length of cfg.mapper's noise schedule; no upper
    bound where cfg has no mapper section), else ValueError before any device work; None (the full schedule) stays
    None."""
    if k_step is None:
        return None
    mapper = getattr(cfg, "mapper", None)
    steps = len(noise_schedule(mapper)) if mapper is not None else None
    ok = isinstance(k_step, (int, np.integer)) and not isinstance(k_step, bool)
    if not ok or k_step < 1 or (steps is not None and k_step > steps):
        raise ValueError(f"k_step {k_step!r}: an integer in [1, {steps if steps is not None else 'steps'}]")
    return int(k_step)


K_STEP_MELS = ("source", "shifted")


def check_k_step_mel(k_step_mel, k_step):
    """Shallow diffusion's start mel: "source" (the clip's own mel) or "shifted" (its key-shifted mel, mel_keyshift by
    the F0 factor), which needs a k_step; else ValueError before any device work."""
    if k_step_mel not in K_STEP_MELS:
        raise ValueError(f"k_step_mel {k_step_mel!r}: 'source' or 'shifted'")
    if k_step_mel == "shifted" and k_step is None:
        raise ValueError("k_step_mel='shifted' needs k_step (shallow diffusion)")
    return k_step_mel


def check_supported(cfg):
    """Reject configurations the native path does not implement, before any device work (raise ValueError)."""
    merge = getattr(cfg.mapper, "merge_mode", "add")
    if merge != "add":
        # modules/encoder.py:193-199: "add" sums the sub-encoder outputs, "concat" widens cond to their summed
        # widths. The native conditioner implements "add" only; anything else must not silently mis-condition.
        raise ValueError(f"mapper.merge_mode {merge!r}: only 'add' is supported (modules/encoder.py:195-199)")
    if cfg.vocoder.activation not in ("snake", "snakebeta"):
        raise ValueError(f"vocoder.activation {cfg.vocoder.activation!r}: snake or snakebeta "
                         "(modules/bigvgan.py:392-421)")


def engine_config_keys(c):
    """The reference config (utils/util.py JSON5 tree) flattened into the numeric keys svc_ctx_set_config takes."""
    kv = {k: getattr(c, k) for k in ("fs", "n_fft", "hop_length", "win_length", "n_mels", "fmin", "fmax", "f0_min",
                                     "f0_max")}
    m = c.mapper
    for k in ("residual_channels", "residual_layer_num", "n_mel", "diffusion_fc_size", "dilation_cycle_length",
              "residual_kernel_size"):
        kv["mapper." + k] = m[k]
    kv["mapper.noise_schedule_factors.0"] = m.noise_schedule_factors[0]
    kv["mapper.noise_schedule_factors.1"] = m.noise_schedule_factors[1]
    v = c.vocoder
    kv["vocoder.n_stages"] = len(v.upsample_rates)
    kv["vocoder.n_kernels"] = len(v.resblock_kernel_sizes)
    kv["vocoder.upsample_initial_channel"] = v.upsample_initial_channel
    kv["vocoder.input_dim"] = v.input_dim
    # modules/bigvgan.py:536 (AMPBlock1 if resblock == "1" else AMPBlock2), :392-421 snake / snakebeta
    kv["vocoder.resblock"] = 2 if str(v.resblock) == "2" else 1
    if v.activation not in ("snake", "snakebeta"):
        raise ValueError(f"vocoder.activation {v.activation!r}: snake or snakebeta (modules/bigvgan.py:392-421)")
    kv["vocoder.snake"] = 1 if v.activation == "snake" else 0
    kv["vocoder.snake_logscale"] = 1 if v.snake_logscale else 0
    for i, (u, k) in enumerate(zip(v.upsample_rates, v.upsample_kernel_sizes)):
        kv[f"vocoder.upsample_rates.{i}"] = u
        kv[f"vocoder.upsample_kernel_sizes.{i}"] = k
    for j, (k, ds) in enumerate(zip(v.resblock_kernel_sizes, v.resblock_dilation_sizes)):
        kv[f"vocoder.resblock_kernel_sizes.{j}"] = k
        kv[f"vocoder.resblock_dilation_sizes.{j}.n"] = len(ds)
        for l, d in enumerate(ds):
            kv[f"vocoder.resblock_dilation_sizes.{j}.{l}"] = d
    return kv


class SVCEngine:
    """Stages of infer.py on one GPU. `whisper_state`, `mapper_state`, `vocoder_state`, `hubert_state` are dicts
    in the reference's state_dict naming (svc_inference_pipeline_amd.weights; fairseq's for HuBERT); any subset
    may be given. `hubert_output_layer` is utils/hubert.py:42's output_layer (9). Precision modes (the defaults are
    the mode the north-star mel-L1 test and bench.py run; DESIGN.md, precision): `content_split` = 0 runs the content
    encoder on plain fp16 operands; 1 on split-fp16 operands ([hi | lo | hi] x [W_hi; W_hi; W_lo], ~19 significand
    bits, 3x the MFMA work); 2 (default) splits only the weights of Whisper's block linears ([x | x] x [W_hi; W_lo],
    2x, no extra activation bytes; the weight rounding is the larger share of their error) with the conv stem and
    HuBERT as in 1. `head_split` runs the DiffSVC head (skip_projection, output_projection) on split-fp16 operands,
    the largest denoiser-side term left. `operands`: "fp16" (default) or "bf16", the 16-bit format of the content
    encoder, conditioner and DiffSVC GEMM operands (v_mfma_f32_16x16x32_f16 or _bf16; the split modes apply to either;
    BigVGAN stays fp16) — BASELINE configs[4]'s fp16-vs-bf16 sweep (tools/precision_sweep.py --bf16).
    `config`: further numeric svc_ctx_set_config keys, set before finalize
    (e.g. {"content.wsplit_mlp": 0xffffff} to weight-split the MLP linears of all 24 Whisper blocks; an unknown key
    raises)."""

    ragged_hubert = True  # hubert_encode takes n_samples, map_content takes frames / src_rows (SVCPipeline)
    ragged_whisper = True  # whisper_content encodes a ragged batch window by window in one pass (SVCPipeline)

    def __init__(self, cfg, device=0, whisper_state=None, mapper_state=None, vocoder_state=None, hubert_state=None,
                 hubert_output_layer=9, content_split=2, head_split=True, config=None, operands="fp16"):
        check_supported(cfg)
        _lib.load()
        self.cfg = cfg
        # a libsvc_hip context is not thread-safe (its workspace and length-table rings are shared by its entry
        # points): SVCPipeline conversions and SVCServer's worker take this lock around a whole conversion
        self.lock = threading.RLock()
        self.device = device
        # per-singer F0 targets (SVCPipeline.enroll fills it); empty: every singer takes target_f0_median
        path = getattr(cfg, "singer_f0_file", None)
        self.singer_f0 = SingerF0Table.load(path) if path and os.path.exists(path) else SingerF0Table()
        # per-singer retrieval indexes (SVCPipeline.enroll(index=True) or load_singer_index fill it); empty: index_rate
        # finds no enrolled singer and launches nothing
        self.singer_index = SingerIndexTable()
        self._ctx = ctypes.c_void_p()
        torch.cuda.set_device(device)
        _lib.call("svc_ctx_create", device, ctypes.byref(self._ctx))
        self._keep = []
        self._set_config()
        # content_split: False / 0 = fp16, True / 1 = split-fp16 operands, 2 = weight-split Whisper linears
        _lib.call("svc_ctx_set_config", self._ctx, b"content.split", float(int(content_split)))
        _lib.call("svc_ctx_set_config", self._ctx, b"mapper.head_split", 1.0 if head_split else 0.0)
        if operands not in ("fp16", "bf16"):
            raise ValueError(f"operands {operands!r}: fp16 or bf16")
        self.operands = operands
        # the 16-bit format of content features (map_content's output, the conditioner's input)
        self.content_dtype = torch.bfloat16 if operands == "bf16" else torch.float16
        _lib.call("svc_ctx_set_config", self._ctx, b"operands.bf16", 1.0 if operands == "bf16" else 0.0)
        for k, v in (config or {}).items():  # further svc_ctx_set_config keys (e.g. "content.wsplit_mlp")
            _lib.call("svc_ctx_set_config", self._ctx, k.encode(), float(v))
        if whisper_state is not None:
            self._add_state("whisper.", whisper_state)
            self.whisper_dims = W.whisper_dims_from_state(whisper_state)
        if hubert_state is not None:
            _lib.call("svc_ctx_set_config", self._ctx, b"hubert.output_layer", float(hubert_output_layer))
            self._add_state("hubert.", hubert_state)
        if mapper_state is not None:
            self._add_state("mapper.", mapper_state)
            self._add("mapper.step_table", W.step_embedding_table(len(noise_schedule(cfg.mapper))).numpy())
            st = load_stats(cfg)
            self._add("stats.mel_min", st["mel_min"])
            self._add("stats.mel_max", st["mel_max"])
            self.target_f0_median = st["target_f0_median"]
        if vocoder_state is not None:
            if mapper_state is None:  # copy-synthesis (mel_normalize + bigvgan) needs the mel statistics alone
                st = load_stats(cfg)
                self._add("stats.mel_min", st["mel_min"])
                self._add("stats.mel_max", st["mel_max"])
            self._add_state("vocoder.", vocoder_state)
            self._add("vocoder.fade_out", W.fade_out_table(20 * cfg.hop_length).numpy())
        _lib.call("svc_ctx_finalize", self._ctx)
        self._keep = []

    # ------------------------------------------------------------------ setup
    def _set_config(self):
        for k, val in engine_config_keys(self.cfg).items():
            _lib.call("svc_ctx_set_config", self._ctx, k.encode(), float(val))

    def _add(self, name, arr):
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.float32))
        self._keep.append(a)
        shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
        _lib.call("svc_ctx_add_param", self._ctx, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.ndim, shape)

    def _add_state(self, prefix, sd):
        for k, v in sd.items():
            self._add(prefix + k, v.numpy() if isinstance(v, torch.Tensor) else v)

    def close(self):
        if self._ctx:
            _lib.call("svc_ctx_destroy", self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def aux_stream(self, index=2):
        """The context's sub-stream `index` as a torch stream (svc_ctx_stream); index 2 is idle while the Whisper
        encoder runs its two sub-batches on 0 and 1."""
        ptr = ctypes.c_void_p()
        _lib.call("svc_ctx_stream", self._ctx, index, ctypes.byref(ptr))
        return torch.cuda.ExternalStream(ptr.value, device=torch.device("cuda", self.device))

    def memory(self):
        wb, wsb = ctypes.c_int64(), ctypes.c_int64()
        _lib.call("svc_ctx_memory", self._ctx, ctypes.byref(wb), ctypes.byref(wsb))
        return wb.value, wsb.value

    def get_config(self, key):
        """A configuration key's value on this context, or a kernel switch's ("tune.<name>")."""
        return _lib.get_config(self._ctx, key)

    def tune(self, **switches):
        """Kernel switches of this context (csrc/common.h Tuning: A/B runs and parity tests), e.g.
        tune(sampler_streams=1); tune(reset=1) restores the values at creation (defaults, SVC_<NAME> environment)."""
        if not self._ctx:
            raise _lib.SVCError("tune: the engine is closed")
        _lib.tune(self._ctx, **switches)

    # ------------------------------------------------------------------ stages
    def mel_energy(self, wav24, n_samples=None):
        """wav24 f32 [B, N] -> (log-mel f32 [B, T, n_mels], energy f32 [B, T]) — utils/mel.py:179-201.
        n_samples (ragged batch, host ints [B]): utterance b is wav24[b, :n_samples[b]]; its frames past
        mel_frames(n_samples[b]) come back as zeros."""
        B, N = wav24.shape
        T = mel_frames(N, self.cfg.n_fft, self.cfg.hop_length)
        mel = torch.empty(B, T, self.cfg.n_mels, device=wav24.device, dtype=torch.float32)
        en = torch.empty(B, T, device=wav24.device, dtype=torch.float32)
        _lib.call("svc_mel_energy", self._ctx, _ptr(wav24), B, N, _host_lengths(n_samples, B, ctypes.c_int64),
                  _ptr(mel), _ptr(en), _stream())
        return mel, en

    def f0(self, wav24, T, n_samples=None):
        """Praat-AC F0 padded to T frames (utils/f0.py:120-161) -> f64 [B, T]; n_samples as in mel_energy."""
        B, N = wav24.shape
        f0 = torch.empty(B, T, device=wav24.device, dtype=torch.float64)
        _lib.call("svc_f0_ac", self._ctx, _ptr(wav24), B, N, _host_lengths(n_samples, B, ctypes.c_int64), T,
                  _ptr(f0), _stream())
        return f0

    def f0_pyin(self, wav24, n_samples=None, win_length=None, hop_length=None, f0_min=None, f0_max=None, T=None):
        """pYIN F0 (utils/f0.py:95-117 get_f0_features_using_pyin: librosa.pyin defaults, unvoiced frames 0) ->
        f64 [B, T], T = 1 + N // hop_length by default (librosa's centred frame count). Arguments default to the
        config's fs / win_length / hop_length / f0_min / f0_max, as the reference's callers pass them."""
        B, N = wav24.shape
        hop = self.cfg.hop_length if hop_length is None else int(hop_length)
        win = self.cfg.win_length if win_length is None else int(win_length)
        lo = self.cfg.f0_min if f0_min is None else float(f0_min)
        hi = self.cfg.f0_max if f0_max is None else float(f0_max)
        T = 1 + N // hop if T is None else int(T)
        f0 = torch.empty(B, T, device=wav24.device, dtype=torch.float64)
        _lib.call("svc_f0_pyin", self._ctx, _ptr(wav24), B, N, _host_lengths(n_samples, B, ctypes.c_int64),
                  float(self.cfg.fs), win, hop, float(lo), float(hi), T, _ptr(f0), _stream())
        return f0

    def pitch_shift(self, f0, target_median=None, scale=None):
        """In place: f0 *= target_median / median(voiced f0) per utterance
        (utils/acoustic_feature_extraction.py:33-52). f0 f64 [B, T]. target_median: None (the global one of
        config/stats.json) or a scalar: svc_pitch_shift; a sequence or tensor of B targets, or any `scale` (a scalar or
        B factors applied after the shift: row b *= (target[b] / med_b) * scale[b]): svc_pitch_shift_ex."""
        B, T = f0.shape
        tm = self.target_f0_median if target_median is None else target_median
        per_row = isinstance(tm, (list, tuple, np.ndarray, torch.Tensor)) and np.ndim(_host_f64(tm)) > 0
        if not per_row and scale is None:
            _lib.call("svc_pitch_shift", self._ctx, _ptr(f0), B, T, float(tm), _stream())
            return f0
        _lib.call("svc_pitch_shift_ex", self._ctx, _ptr(f0), B, T, _host_table(tm, B, "target_median"),
                  None if scale is None else _host_table(scale, B, "scale"), _stream())
        return f0

    def pitch_factor(self, f0, target_median=None, scale=None):
        """The factor pitch_shift(f0, target_median, scale) multiplies each row by, without applying it: f0 f64 [B, T]
        is only read -> f64 [B] on the device, stream-ordered (NaN for a row with no voiced frame). The arguments are
        pitch_shift's; f0 * factor is bit for bit what it writes (svc_pitch_factor)."""
        B, T = f0.shape
        tm = self.target_f0_median if target_median is None else target_median
        factor = torch.empty(B, device=f0.device, dtype=torch.float64)
        _lib.call("svc_pitch_factor", self._ctx, _ptr(f0), B, T, _host_table(tm, B, "target_median"),
                  None if scale is None else _host_table(scale, B, "scale"), _ptr(factor), _stream())
        return factor

    def mel_keyshift(self, wav24, factor, n_samples=None):
        """wav24 f32 [B, N], factor f64 [B] on the device (pitch_factor's) -> (the key-shifted log-mel f32
        [B, T, n_mels], info int32 [B]): mel_energy's mel of the same voice with its pitch moved by factor[b], from a
        window and transform of rint(n_fft * factor[b]) samples at the same hop (svc_mel_keyshift; Diff-SVC's start mel
        for shallow diffusion). info[b]: 1 the factor was not finite or <= 0 and was taken as 1, 2 the length was
        clamped to [n_fft / 2, 2 n_fft], else 0; nothing is read back. n_samples as in mel_energy."""
        B, N = wav24.shape
        T = mel_frames(N, self.cfg.n_fft, self.cfg.hop_length)
        if factor is not None and (factor.dtype != torch.float64 or factor.numel() != B):
            raise ValueError(f"mel_keyshift: factor must be f64 [{B}]")
        mel = torch.empty(B, max(T, 0), self.cfg.n_mels, device=wav24.device, dtype=torch.float32)
        info = torch.empty(B, device=wav24.device, dtype=torch.int32)
        _lib.call("svc_mel_keyshift", self._ctx, _ptr(wav24), B, N, _host_lengths(n_samples, B, ctypes.c_int64),
                  _ptr(factor), _ptr(mel), _ptr(info), _stream())
        return mel, info

    def f0_voiced_median(self, f0, frames=None):
        """np.median of the voiced (nonzero) cells of f0 f64 [B, T] (or [T]) with t < frames[b] (host ints [B]; None:
        all T), pooled over the batch (utils/acoustic_feature_extraction.py:21-30) -> (median f64 [1], voiced count
        int64 [1]) on the device, stream-ordered; the median is NaN where nothing is voiced."""
        if f0.dim() == 1:
            f0 = f0[None]
        if f0.dtype != torch.float64 or f0.dim() != 2:
            raise ValueError("f0_voiced_median: f0 must be f64 [B, T]")
        B, T = f0.shape
        med = torch.empty(1, device=f0.device, dtype=torch.float64)
        cnt = torch.empty(1, device=f0.device, dtype=torch.int64)
        _lib.call("svc_f0_voiced_median", self._ctx, _ptr(f0), B, T, _host_lengths(frames, B, ctypes.c_int32),
                  _ptr(med), _ptr(cnt), _stream())
        return med, cnt

    def whisper_encode(self, wav16):
        """wav16 f32 [B, N16] -> Whisper encoder output f32 [B, n_ctx, D] (utils/whisper.py:13-28)."""
        B, N = wav16.shape
        d = self.whisper_dims
        feats = torch.empty(B, d["n_audio_ctx"], d["n_audio_state"], device=wav16.device, dtype=torch.float32)
        _lib.call("svc_whisper_encode", self._ctx, _ptr(wav16), B, N, _ptr(feats), _stream())
        return feats

    def map_content(self, feats, T, rule="whisper", out=None, frames=None, src_rows=None):
        """15:8 repeat/average to mel frames -> [B, T, D] in content_dtype (f16; bf16 with operands="bf16").
        rule "whisper": utils/whisper.py:31-81 (T <= 2812); rule "hubert": utils/hubert.py:83-134 (no cap, <= 3
        missing frames repeat the last one, more is an error). `out` may be a column slice [B, T, D] of a wider
        buffer (concatenated content types).
        frames / src_rows (ragged batch, host ints [B]): utterance b maps its first src_rows[b] rows of feats to
        frames[b] frames as a batch of that shape would; its rows past frames[b] come back as zeros."""
        B, S, D = feats.shape
        if out is None:
            out = torch.empty(B, T, D, device=feats.device, dtype=self.content_dtype)
        assert out.shape == (B, T, D) and out.stride(2) == 1 and out.stride(0) == T * out.stride(1)
        assert out.dtype == self.content_dtype, f"map_content: out must be {self.content_dtype}"
        mode = {"whisper": 0, "hubert": 1}[rule]
        if frames is not None or src_rows is not None:
            _lib.call("svc_map_content_ragged", self._ctx, _ptr(feats.contiguous()), B, S,
                      _host_lengths(src_rows, B, ctypes.c_int32), T, _host_lengths(frames, B, ctypes.c_int32), D, mode,
                      ctypes.c_void_p(out.data_ptr()), out.stride(1), _stream())
            return out
        _lib.call("svc_map_content_ex", self._ctx, _ptr(feats.contiguous()), B, S, T, D, mode,
                  ctypes.c_void_p(out.data_ptr()), out.stride(1), _stream())
        return out

    def whisper_windows(self, frames):
        """30 s Whisper windows of a clip of `frames` mel frames (svc_whisper_windows: 1 up to 2812 frames, else
        ceil(frames / 2805))"""
        return int(_lib.load().svc_whisper_windows(int(frames)))

    def whisper_content(self, wav16, n_samples, frames, T, out=None, return_feats=False):
        """Whisper content features of a ragged batch (svc_whisper_content_ragged): wav16 f32 [B, N16] (int16-quantised
        16 kHz), utterance b = wav16[b, :n_samples[b]] (the rest of its row is not read) with frames[b] <= T mel frames
        (host ints [B] each; None = N16 / T for every utterance) -> [B, T, D] in content_dtype. Every window that
        exists is encoded once, all in one pass; rows [b, :frames[b]] equal whisper_encode + map_content on that
        clip's own windows bit for bit, rows past them are zeros. `out` may be a column slice [B, T, D] of a wider
        buffer, as in map_content. return_feats: also the encoder output of every window, f32 [sum of
        whisper_windows(frames[b]), n_ctx, D], utterance-major."""
        B, N = wav16.shape
        d = self.whisper_dims
        D = d["n_audio_state"]
        if out is None:
            out = torch.empty(B, T, D, device=wav16.device, dtype=self.content_dtype)
        assert out.shape == (B, T, D) and out.stride(2) == 1 and out.stride(0) == T * out.stride(1)
        assert out.dtype == self.content_dtype, f"whisper_content: out must be {self.content_dtype}"
        fr = _host_lengths(frames, B, ctypes.c_int32)
        feats = None
        if return_feats:
            n_win = sum(max(self.whisper_windows(t), 0) for t in (fr if fr is not None else [T] * B))
            feats = torch.empty(n_win, d["n_audio_ctx"], D, device=wav16.device, dtype=torch.float32)
        _lib.call("svc_whisper_content_ragged", self._ctx, _ptr(wav16), B, N,
                  _host_lengths(n_samples, B, ctypes.c_int64), T, fr, ctypes.c_void_p(out.data_ptr()), out.stride(1),
                  _ptr(feats), _stream())
        return (out, feats) if return_feats else out

    def hubert_frames(self, n_samples):
        """frames of the conv feature extractor for a clip of n_samples 16 kHz samples"""
        return int(_lib.load().svc_hubert_frames(int(n_samples)))

    def hubert_encode(self, wav16, n_samples=None):
        """get_hubert_content (utils/hubert.py:31-47): wav16 f32 [B, N] (16 kHz float audio) -> ContentVec
        features f32 [B, frames, final_dim] (time-major; the reference returns the transpose).
        n_samples (ragged batch, host ints [B], 400 <= n_b <= N): utterance b is wav16[b, :n_samples[b]] (the rest of
        its row is not read); its hubert_frames(n_samples[b]) rows equal encoding that clip alone bit for bit, and its
        rows past them come back as zeros."""
        B, N = wav16.shape
        fd, _ = ctypes.c_int(), ctypes.c_int()
        _lib.call("svc_hubert_dims", self._ctx, ctypes.byref(fd), None)
        F = int(_lib.load().svc_hubert_frames(N))
        feats = torch.empty(B, F, fd.value, device=wav16.device, dtype=torch.float32)
        if n_samples is not None:
            _lib.call("svc_hubert_encode_ragged", self._ctx, _ptr(wav16.contiguous()), B, N,
                      _host_lengths(n_samples, B, ctypes.c_int64), _ptr(feats), _stream())
            return feats
        _lib.call("svc_hubert_encode", self._ctx, _ptr(wav16.contiguous()), B, N, _ptr(feats), _stream())
        return feats

    def condition(self, content16, f0, energy, singer):
        """EncoderFramework.forward (modules/encoder.py:165-201) -> cond f32 [B, T, C]. content16 in
        content_dtype."""
        B, T, _ = content16.shape
        if content16.dtype != self.content_dtype:
            raise ValueError(f"condition: content must be {self.content_dtype}, got {content16.dtype}")
        cond = torch.empty(B, T, self.cfg.mapper.residual_channels, device=content16.device, dtype=torch.float32)
        singer = singer.to(torch.int32).contiguous()
        _lib.call("svc_condition", self._ctx, _ptr(content16), _ptr(f0.contiguous()), _ptr(energy.contiguous()),
                  _ptr(singer), B, T, _ptr(cond), _stream())
        return cond

    def condition_indices(self, f0, energy):
        """The conditioner's embedding indices (torch.bucketize semantics, modules/encoder.py:70,115):
        f0 f64 [...], energy f32 [...] -> (melody int32, loudness int32) of the same shape."""
        f0 = f0.to(torch.float64).contiguous()
        energy = energy.to(torch.float32).contiguous()
        assert f0.shape == energy.shape
        im = torch.empty(f0.shape, dtype=torch.int32, device=f0.device)
        ie = torch.empty_like(im)
        _lib.call("svc_condition_indices", self._ctx, _ptr(f0), _ptr(energy), f0.numel(), _ptr(im), _ptr(ie),
                  _stream())
        return im, ie

    def diffsvc_eps(self, cond, x, t, frames=None):
        B, T, _ = cond.shape
        eps = torch.empty_like(x)
        _lib.call("svc_diffsvc_eps", self._ctx, _ptr(cond), _ptr(x), B, T, _host_lengths(frames, B, ctypes.c_int32),
                  int(t), _ptr(eps), _stream())
        return eps

    def mel_normalize(self, mel, frames=None):
        """normalize_mel_channel (utils/acoustic_feature_extraction.py:75-80; not clamped): log-mel f32 [B, T, n_mel]
        as mel_energy returns it -> f32 [B, T, n_mel] in the sampler's and the vocoder's normalised range. frames
        (ragged batch, host ints [B]): rows past an utterance's frames come back as zeros."""
        B, T, _ = mel.shape
        out = torch.empty_like(mel, memory_format=torch.contiguous_format)
        _lib.call("svc_mel_normalize", self._ctx, _ptr(mel.contiguous()), B, T,
                  _host_lengths(frames, B, ctypes.c_int32), _ptr(out), _stream())
        return out

    def diffsvc_sample(self, cond, fast_inference=False, speedup=10, x_T=None, noise=None, seed=0, utt_ids=None,
                       frames=None, k_step=None, mel_src=None, x_start=None, solver=None, solver_steps=20,
                       solver_spacing="logsnr"):
        """svc_model_inference (modules/diffsvcrepo_inference.py:154-240) -> normalised mel x_0 f32 [B, T, n_mel].
        frames (ragged batch, host ints [B]): utterance b's mel frames; its rows past them come back as zeros.
        k_step (shallow diffusion, Diff-SVC's k_step; None: the whole schedule from x_T, the call as before): start
        at noise level k_step - 1 from exactly one of mel_src (the source's un-normalised log-mel [B, T, n_mel]:
        normalised and noised forward on the device, keyed by utt_ids) and x_start (an already noised state); DDPM
        `noise` is then [k_step, B*T*n_mel] (svc_diffsvc_sample_from).
        solver (None: the DDPM / PLMS call as before): "dpmpp2m" (DPM-Solver++(2M)) or "ddim" (its first-order case)
        over config.solver_timesteps(cfg, k_step, solver_steps, solver_spacing): one denoiser call per timestep
        (svc_diffsvc_sample_steps); fast_inference and speedup are not used. It composes with k_step / mel_src /
        x_start and frames; without k_step the start state is x_T when given, else the device draw. The solvers draw
        nothing per step: `noise` with a solver is a ValueError. Output quality at a given solver_steps has been checked
        on an analytic denoiser and random weights only."""
        B, T, _ = cond.shape
        k_step = check_k_step(k_step, self.cfg)
        solver = check_solver(solver, solver_steps, solver_spacing)
        if k_step is None and (mel_src is not None or x_start is not None):
            raise ValueError("diffsvc_sample: mel_src / x_start need k_step")
        if k_step is not None and (x_T is not None or (mel_src is None) == (x_start is None)):
            raise ValueError("diffsvc_sample: k_step takes exactly one of mel_src and x_start (and no x_T)")
        if solver is not None and noise is not None:
            raise ValueError("diffsvc_sample: `noise` with a solver (the solvers draw nothing per step)")
        x0 = torch.empty(B, T, self.cfg.mapper.n_mel, device=cond.device, dtype=torch.float32)
        if solver is not None:
            ts = solver_timesteps(self.cfg, k_step, solver_steps, solver_spacing)
            # the state at level ts[0]; without one, mel_src noised to it or the device draw
            start = x_T if k_step is None else x_start
            uid = _draw_keys(utt_ids, start is None, B, cond.device)
            _lib.call("svc_diffsvc_sample_steps", self._ctx, _ptr(cond), B, T, _host_lengths(frames, B, ctypes.c_int32),
                      (ctypes.c_int32 * len(ts))(*ts), len(ts), SOLVERS[solver], _opt_ptr(mel_src), _opt_ptr(start),
                      ctypes.c_uint64(seed), _ptr(uid), _ptr(x0), _stream())
            return x0
        # the device draws x_T, and DDPM's per-step z
        uid = _draw_keys(utt_ids, (x_T is None and x_start is None) or (noise is None and not fast_inference), B,
                         cond.device)
        mode = MODE_PLMS if fast_inference else MODE_DDPM
        if k_step is not None:
            _lib.call("svc_diffsvc_sample_from", self._ctx, _ptr(cond), B, T, _host_lengths(frames, B, ctypes.c_int32),
                      mode, int(speedup), k_step, _opt_ptr(mel_src), _opt_ptr(x_start), _opt_ptr(noise),
                      ctypes.c_uint64(seed), _ptr(uid), _ptr(x0), _stream())
        else:
            _lib.call("svc_diffsvc_sample", self._ctx, _ptr(cond), B, T, _host_lengths(frames, B, ctypes.c_int32), mode,
                      int(speedup), _opt_ptr(x_T), _opt_ptr(noise), ctypes.c_uint64(seed), _ptr(uid), _ptr(x0),
                      _stream())
        return x0

    def bigvgan(self, x0, return_mel=False, frames=None):
        """denormalize_mel_channel + synthesis_audios (Generator, trim, fade) -> wav f32 [B, T*hop]. frames (ragged
        batch, host ints [B]): utterance b's waveform is frames[b]*hop samples long (fade-out there, zeros after)."""
        B, T, _ = x0.shape
        wav = torch.empty(B, T * self.cfg.hop_length, device=x0.device, dtype=torch.float32)
        mel = torch.empty_like(x0) if return_mel else None
        _lib.call("svc_bigvgan", self._ctx, _ptr(x0.contiguous()), B, T, _host_lengths(frames, B, ctypes.c_int32),
                  _ptr(wav), _ptr(mel), _stream())
        return (wav, mel) if return_mel else wav

    def load_pcm(self, infos, fs=None, sr_mono=16000, float_mono=False):
        """The input end for a batch of parsed wavs (audio.WavInfo: format code, channels, rate, frames, payload view):
        one host concatenation of the payloads, one upload, one svc_load_pcm_ex call -> (y_src f32 [B, S_src] at `fs`
        (default: the config's), y_mono f32 [B, S_mono] at sr_mono on the int16 grid, n_src, n_mono (host ints [B]: each
        row's own samples, zeros after them), info int32 [B] on the device (bits 0-1 the normalisation class, bit 2
        non-finite source samples)). Row b is bit for bit audio.load_audio / audio.load_whisper_audio of that file.
        float_mono=True: a sixth value, y_mono_float f32 [B, S_mono], HuBERT / ContentVec's float copy at sr_mono from
        the same launch as y_mono (row b is audio.load_contentvec_audio of that file; n_mono is its length too)."""
        fs = int(self.cfg.fs if fs is None else fs)
        B = len(infos)
        if B < 1:
            raise ValueError("load_pcm: no utterances")
        lib = _lib.load()
        sizes = [len(i.payload) for i in infos]
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        host = np.empty(max(1, sum(sizes)), dtype=np.uint8)
        for o, n, i in zip(offs.tolist(), sizes, infos):
            host[o:o + n] = np.frombuffer(i.payload, dtype=np.uint8)
        with self.lock:
            dev = torch.device("cuda", self.device)
            raw = torch.from_numpy(host).to(dev)
            n_src = [int(lib.svc_resample_len(i.n_frames, i.sr, fs)) for i in infos]
            n_mono = [int(lib.svc_resample_len(i.n_frames, i.sr, sr_mono)) for i in infos]
            y_src = torch.empty(B, max(1, max(n_src)), device=dev, dtype=torch.float32)
            y_mono = torch.empty(B, max(1, max(n_mono)), device=dev, dtype=torch.float32)
            y_float = torch.empty_like(y_mono) if float_mono else None
            info = torch.empty(B, device=dev, dtype=torch.int32)
            i64, i32 = ctypes.c_int64 * B, ctypes.c_int32 * B
            _lib.call("svc_load_pcm_ex", self._ctx, _ptr(raw), B, i64(*offs.tolist()),
                      i64(*[i.n_frames for i in infos]), i32(*[i.format for i in infos]),
                      i32(*[i.channels for i in infos]), i32(*[i.sr for i in infos]), fs, y_src.shape[1], _ptr(y_src),
                      int(sr_mono), y_mono.shape[1], _ptr(y_mono), _ptr(y_float), _ptr(info),
                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if float_mono:
            return y_src, y_mono, n_src, n_mono, info, y_float
        return y_src, y_mono, n_src, n_mono, info

    def pcm16(self, wav, n_samples=None, add_silence=True, turn_up=True, volume_peak=0.9, return_peak=False):
        """save_audio's sample conversion (utils/util.py:20-37; audio.to_pcm16 per utterance, bit for bit) on the
        device: wav f32 [B, S] -> int16 [B, S + 2 * sil], sil = fs // 20 with add_silence else 0. n_samples (ragged
        batch, host ints [B], 0 <= n_b <= S): utterance b is wav[b, :n_samples[b]], normalised by its own peak; its
        row is [sil zeros | n_b samples | sil zeros | zeros]. A silent or empty utterance gives zeros and peak 0
        (to_pcm16 raises ZeroDivisionError). return_peak: also the f32 [B] peaks max |x|."""
        if wav.dim() != 2 or wav.dtype != torch.float32:
            raise ValueError("pcm16: wav must be f32 [B, S]")
        B, S = wav.shape
        L = int(_lib.load().svc_pcm16_len(S, int(self.cfg.fs), 1 if add_silence else 0))
        pcm = torch.empty(B, L, device=wav.device, dtype=torch.int16)
        peak = torch.empty(B, device=wav.device, dtype=torch.float32) if return_peak else None
        _lib.call("svc_pcm16", self._ctx, _ptr(wav), B, S, _host_lengths(n_samples, B, ctypes.c_int64),
                  int(self.cfg.fs), 1 if add_silence else 0, 1 if turn_up else 0, float(volume_peak), _ptr(pcm),
                  _ptr(peak), _stream())
        return (pcm, peak) if return_peak else pcm

    def loudness_match(self, wav, src, n_samples=None, src_samples=None, mix=0.0, window=None, hop=None,
                       floor_rms=1e-6, max_gain=None, out=None, return_gain=False):
        """Loudness envelope transfer on the device (svc_loudness_match; audio.loudness_match per utterance: gains
        within (window + 16) * 2^-52 relative, samples within 1 f32 ulp): wav f32 [B, S] (the vocoder output) takes the
        slow RMS envelope of src f32 [B, S_src] (the source at the same rate and time origin) -> f32 [B, S]. mix: 0
        gives the source's envelope, 1 leaves wav as it is. window / hop default to fs // 2 * 2 and fs // 2
        (so-vits-svc's). n_samples / src_samples (ragged batch, host ints [B]): utterance b is wav[b, :n_samples[b]]
        against src[b, :src_samples[b]]; its row is zeros from n_samples[b] on. max_gain: a cap on the per-frame gain
        (None: none). out: the result's tensor, which may be wav itself (in place). return_gain: also the f64
        [B, 1 + S // hop] per-frame gains (0 past an utterance's own frames)."""
        from .audio import check_loudness_mix, loudness_params
        if wav.dim() != 2 or wav.dtype != torch.float32 or src.dim() != 2 or src.dtype != torch.float32:
            raise ValueError("loudness_match: wav and src must be f32 [B, S] and [B, S_src]")
        if src.shape[0] != wav.shape[0]:
            raise ValueError(f"loudness_match: {src.shape[0]} source rows for a batch of {wav.shape[0]}")
        mix = check_loudness_mix(mix)
        if mix is None:
            raise ValueError("loudness_match: mix is None")
        window, hop = loudness_params(int(self.cfg.fs), window, hop)
        B, S = wav.shape
        if out is None:
            out = torch.empty_like(wav)
        elif out.shape != wav.shape or out.dtype != torch.float32:
            raise ValueError("loudness_match: out must be f32 with wav's shape")
        gain = None
        if return_gain:
            gain = torch.empty(B, int(_lib.load().svc_loudness_frames(S, hop)), device=wav.device, dtype=torch.float64)
        _lib.call("svc_loudness_match", self._ctx, _ptr(wav), _ptr(src), B, S, src.shape[1],
                  _host_lengths(n_samples, B, ctypes.c_int64), _host_lengths(src_samples, B, ctypes.c_int64), window,
                  hop, mix, float(floor_rms), 0.0 if max_gain is None else float(max_gain), _ptr(out), _ptr(gain),
                  _stream())
        return (out, gain) if return_gain else out

    def stitch(self, rows, plan, out=None, return_shifts=False, return_q=False):
        """Join converted chunks into their songs on the device (svc_stitch; audio.stitch is its definition:
        displacements and q bit-equal, crossfade samples within 1 f32 ulp, everything else copied bit for bit). rows: B
        f32 device tensors, chunk b's waveform with at least plan.n[b] samples (views into the vocoder's output; each
        contiguous along its samples; nothing is copied); plan: an audio.StitchPlan (host tables, in samples) -> out f32
        [plan.out_len]. `out`: the result's tensor (f32, contiguous, plan.out_len elements of any shape); only the
        chunks' body intervals are written, and without `out` the rest is zeros. return_shifts: also the
        displacements int32 [B]; return_q: also q f64 [B, max(2 search, 1)]. Two launches whatever B is, on the
        current stream; the tables are checked before any device work (SVCError)."""
        B = len(plan.n)
        if len(rows) != B or B < 1:
            raise ValueError(f"stitch: {len(rows)} rows for {B} chunks")
        for b, r in enumerate(rows):
            if not r.is_cuda or r.dtype != torch.float32 or r.dim() != 1 or (r.numel() > 1 and r.stride(0) != 1):
                raise ValueError(f"stitch: chunk {b}: a row must be a 1-D f32 device tensor with contiguous samples")
            if r.numel() < int(plan.n[b]):
                raise ValueError(f"stitch: chunk {b}: a row of {r.numel()} samples, n {int(plan.n[b])}")
        dev = rows[0].device
        if out is None:
            out = torch.zeros(int(plan.out_len), device=dev, dtype=torch.float32)
        elif out.dtype != torch.float32 or out.numel() != int(plan.out_len) or not out.is_contiguous():
            raise ValueError(f"stitch: out must be contiguous f32 with {int(plan.out_len)} elements")
        nc = max(2 * int(plan.search), 1)
        shifts = torch.empty(B, device=dev, dtype=torch.int32) if return_shifts else None
        q = torch.empty(B, nc, device=dev, dtype=torch.float64) if return_q else None
        i64 = lambda v: (ctypes.c_int64 * B)(*[int(x) for x in v])
        _lib.call("svc_stitch", self._ctx, (ctypes.c_void_p * B)(*[r.data_ptr() for r in rows]), B, i64(plan.n),
                  i64(plan.lead), i64(plan.body), (ctypes.c_int32 * B)(*[int(x) for x in plan.joined]),
                  i64(plan.out_off), int(plan.xfade), int(plan.search), float(plan.eps), _ptr(out),
                  int(plan.out_len), _ptr(shifts), _ptr(q), _stream())
        res = (out,) + ((shifts,) if return_shifts else ()) + ((q,) if return_q else ())
        return res if len(res) > 1 else out

    def index_norms(self, x16):
        """The squared norms of a retrieval index (svc_index_norms): x16 f16 [N, D] (rows may be a column slice of a
        wider buffer: stride(0) >= D, a multiple of 8) -> f32 [N], each row's f64 sum of squares rounded to f32."""
        if x16.dim() != 2 or x16.dtype != torch.float16 or x16.stride(1) != 1:
            raise ValueError("index_norms: the index must be f16 [N, D] with contiguous rows")
        N, D = x16.shape
        norms = torch.empty(N, device=x16.device, dtype=torch.float32)
        _lib.call("svc_index_norms", self._ctx, ctypes.c_void_p(x16.data_ptr()), N, D, x16.stride(0), _ptr(norms),
                  _stream())
        return norms

    def content_retrieve(self, content, index, norms, frames=None, sel=None, k=8, rate=1.0, dist_floor=None, out=None,
                         return_neighbours=False):
        """Feature retrieval (svc_content_retrieve; RVC's index_rate): every frame of content f16 [B, T, D] that takes
        part is replaced by rate * (the inverse-squared-distance weighted mean of its k nearest rows of index f16
        [N, D]) + (1 - rate) * itself. norms: index_norms(index). frames (host ints [B]): utterance b has frames[b]
        rows, the rows past them come back as zeros; sel (host 0 / 1 [B]): utterances with 0 take no part (copied, or
        left alone in place). dist_floor: the clamp on a squared distance, None: 1e-4 * D. out: the result's tensor,
        which may be content itself (in place); content, index and out may be column slices of wider buffers.
        return_neighbours: also (idx int32 [B, T, k], d2 f32 [B, T, k]): the selected index rows in rank order and
        their clamped squared distances, -1 / 0 past min(k, N) and on rows that take no part."""
        if self.operands != "fp16":
            raise ValueError("content_retrieve: fp16 content only (this engine runs operands='bf16')")
        if content.dim() != 3 or content.dtype != torch.float16 or content.stride(2) != 1:
            raise ValueError("content_retrieve: content must be f16 [B, T, D]")
        B, T, D = content.shape
        if content.stride(0) != T * content.stride(1):
            raise ValueError("content_retrieve: content rows must keep one stride over the batch")
        if index.dim() != 2 or index.dtype != torch.float16 or index.shape[1] != D or index.stride(1) != 1:
            raise ValueError(f"content_retrieve: the index must be f16 [N, {D}]")
        N = index.shape[0]
        if norms.dtype != torch.float32 or norms.numel() != N:
            raise ValueError(f"content_retrieve: norms must be f32 [{N}]")
        rate = check_index_rate(rate)
        if rate is None:
            raise ValueError("content_retrieve: rate is None")
        if out is None:
            out = torch.empty(B, T, D, device=content.device, dtype=torch.float16)
        elif (out.shape != content.shape or out.dtype != torch.float16 or out.stride(2) != 1
              or out.stride(0) != T * out.stride(1)):
            raise ValueError("content_retrieve: out must be f16 with content's shape")
        idx = d2 = None
        if return_neighbours:
            idx = torch.empty(B, T, int(k), device=content.device, dtype=torch.int32)
            d2 = torch.empty(B, T, int(k), device=content.device, dtype=torch.float32)
        _lib.call("svc_content_retrieve", self._ctx, ctypes.c_void_p(content.data_ptr()), B, T,
                  _host_lengths(frames, B, ctypes.c_int32), _host_lengths(sel, B, ctypes.c_int32), D,
                  content.stride(1), ctypes.c_void_p(index.data_ptr()), _ptr(norms), N, index.stride(0), int(k), rate,
                  1e-4 * D if dist_floor is None else float(dist_floor), ctypes.c_void_p(out.data_ptr()),
                  out.stride(1), _ptr(idx), _ptr(d2), _stream())
        return (out, idx, d2) if return_neighbours else out

    def _index_rows(self, name, what, x16, D=None):
        """f16 [n, D] with contiguous rows (a column slice of a wider buffer is fine), fp16 engines only"""
        if self.operands != "fp16":
            raise ValueError(f"{name}: fp16 rows only (this engine runs operands='bf16')")
        if x16.dim() != 2 or x16.dtype != torch.float16 or x16.stride(1) != 1 or (D is not None and x16.shape[1] != D):
            raise ValueError(f"{name}: {what} must be f16 [n, {'D' if D is None else D}] with contiguous rows")
        return x16.shape

    def index_assign(self, rows, centroids, norms, return_counts=False, return_inertia=False):
        """Lloyd's assignment (svc_index_assign): rows f16 [N, D] against centroids f16 [K, D] with norms =
        index_norms(centroids) -> labels int32 [N], each row's nearest centroid under content_retrieve's own score and
        order (an equal score goes to the lower j). Also, where asked, counts int32 [K] and inertia f64 [1] (the sum
        of the rows' clamped squared distances, bit-identical from run to run): (labels[, counts][, inertia])."""
        N, D = self._index_rows("index_assign", "rows", rows)
        K, _ = self._index_rows("index_assign", "centroids", centroids, D)
        if norms.dtype != torch.float32 or norms.numel() != K or not norms.is_contiguous():
            raise ValueError(f"index_assign: norms must be f32 [{K}]")
        labels = torch.empty(N, device=rows.device, dtype=torch.int32)
        counts = torch.empty(K, device=rows.device, dtype=torch.int32) if return_counts else None
        inertia = torch.empty(1, device=rows.device, dtype=torch.float64) if return_inertia else None
        _lib.call("svc_index_assign", self._ctx, ctypes.c_void_p(rows.data_ptr()), N, D, rows.stride(0),
                  ctypes.c_void_p(centroids.data_ptr()), _ptr(norms), K, centroids.stride(0), _ptr(labels),
                  _ptr(counts), _ptr(inertia), _stream())
        out = (labels,) + ((counts,) if return_counts else ()) + ((inertia,) if return_inertia else ())
        return out if len(out) > 1 else labels

    def index_update(self, rows, labels, prev, out=None, return_counts=False):
        """Lloyd's centroid update (svc_index_update): the exact mean of the rows f16 [N, D] of every label (int32 [N],
        values in [0, K)), rounded once to f16; a cluster without a row keeps prev's row (f16 [K, D]). out: the
        centroids' tensor, which may be prev itself. -> (centroids f16 [K, D], norms f32 [K][, counts int32 [K]])."""
        N, D = self._index_rows("index_update", "rows", rows)
        K, _ = self._index_rows("index_update", "prev", prev, D)
        if labels.dtype != torch.int32 or labels.numel() != N or not labels.is_contiguous():
            raise ValueError(f"index_update: labels must be int32 [{N}]")
        if out is None:
            out = torch.empty(K, D, device=rows.device, dtype=torch.float16)
        elif self._index_rows("index_update", "out", out, D)[0] != K:
            raise ValueError(f"index_update: out must be f16 [{K}, {D}]")
        norms = torch.empty(K, device=rows.device, dtype=torch.float32)
        counts = torch.empty(K, device=rows.device, dtype=torch.int32) if return_counts else None
        _lib.call("svc_index_update", self._ctx, ctypes.c_void_p(rows.data_ptr()), N, D, rows.stride(0), _ptr(labels),
                  K, ctypes.c_void_p(prev.data_ptr()), prev.stride(0), ctypes.c_void_p(out.data_ptr()), out.stride(0),
                  _ptr(norms), _ptr(counts), _stream())
        return (out, norms, counts) if return_counts else (out, norms)

    def index_kmeans(self, rows, K, iters=10, return_labels=False):
        """A retrieval index compacted to K centroids (svc_index_kmeans): the centroids start as rows floor(i N / K)
        (iters = 0 returns exactly that strided sample), then `iters` rounds of index_assign + index_update, and one
        last assignment. No early stop, no random numbers, no host synchronisation. -> (centroids f16 [K, D], norms
        f32 [K], counts int32 [K], inertia f64 [iters + 1][, labels int32 [N]])."""
        N, D = self._index_rows("index_kmeans", "rows", rows)
        K, iters = int(K), int(iters)
        if not 1 <= K <= N:
            raise ValueError(f"index_kmeans: K={K} (1 <= K <= N={N})")
        if not 0 <= iters <= 1000:
            raise ValueError(f"index_kmeans: iters={iters} (0 <= iters <= 1000)")
        cent = torch.empty(K, D, device=rows.device, dtype=torch.float16)
        norms = torch.empty(K, device=rows.device, dtype=torch.float32)
        counts = torch.empty(K, device=rows.device, dtype=torch.int32)
        inertia = torch.empty(iters + 1, device=rows.device, dtype=torch.float64)
        labels = torch.empty(N, device=rows.device, dtype=torch.int32) if return_labels else None
        _lib.call("svc_index_kmeans", self._ctx, ctypes.c_void_p(rows.data_ptr()), N, D, rows.stride(0), K, iters,
                  ctypes.c_void_p(cent.data_ptr()), cent.stride(0), _ptr(norms), _ptr(labels), _ptr(counts),
                  _ptr(inertia), _stream())
        return (cent, norms, counts, inertia, labels) if return_labels else (cent, norms, counts, inertia)

    def load_singer_index(self, path):
        """Replace engine.singer_index by the table saved at `path` (SingerIndexTable.save), on this engine's device;
        an index whose row width or content types differ from this configuration's content is a ValueError."""
        dim, types = content_signature(self.cfg)
        self.singer_index = SingerIndexTable.load(path, torch.device("cuda", self.device), dim=dim,
                                                  content_types=types)
        return self.singer_index
