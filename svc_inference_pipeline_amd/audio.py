"""Audio I/O for the conversion path, mirroring the reference's host functions.

    load_audio_torch(wave_file, fs)   utils/audio.py:10-55            -> load_audio (+ resample on the GPU)
    load_audio(file, sr=16000)        utils/whisper_extractor/audio.py:22-49 (ffmpeg s16le decode)
                                                                      -> load_whisper_audio
    librosa.load(path, sr=16000)      utils/hubert.py:137-143          -> load_contentvec_audio
    save_audio(path, waveform, fs)    utils/util.py:20-37              -> save_audio
    the loaders for a batch of files                                  -> load_batch (parse_wav on the host, one
                                                                         svc_load_pcm / svc_load_pcm_ex call on the GPU)

The reference reads wavs with soundfile, resamples with librosa (soxr) and decodes Whisper's 16 kHz input with
an ffmpeg subprocess; none of the three is in this image. Here a RIFF/WAVE reader gives soundfile's float
conversion (PCM int / 2^(bits-1), IEEE float as stored), and resampling runs in libsvc_hip.so
(`svc_resample`: scipy.signal.resample_poly's Kaiser(5) polyphase filter; parity pinned to scipy, unpinned
against soxr / ffmpeg's swresample). Only WAV input is supported (the reference's non-wav branch uses
librosa.load).
"""
import collections
import ctypes
import fractions
import math
import os
import struct

import numpy as np
import torch

from . import _lib

WHISPER_SR = 16000  # utils/whisper_extractor/audio.py:12


class AudioError(ValueError):
    pass


def read_wav(path):
    """RIFF/WAVE -> (float64 [n, channels], sample_rate), with soundfile.read's float scaling.
    PCM 8 (unsigned), 16, 24, 32-bit and IEEE float 32/64, WAVE_FORMAT_EXTENSIBLE included."""
    with open(path, "rb") as fh:
        data = fh.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise AudioError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, payload = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            tag, ch, sr, _, align, bits = struct.unpack("<HHIIHH", body[:16])
            if tag == 0xFFFE and len(body) >= 26:  # WAVE_FORMAT_EXTENSIBLE: sub-format GUID's first 2 bytes
                tag = struct.unpack("<H", body[24:26])[0]
            fmt = (tag, ch, sr, align, bits)
        elif cid == b"data":
            payload = body
        pos += 8 + size + (size & 1)
    if fmt is None or payload is None:
        raise AudioError(f"{path}: missing fmt or data chunk")
    tag, ch, sr, align, bits = fmt
    if ch < 1 or align != ch * bits // 8:
        raise AudioError(f"{path}: unsupported layout ({ch} channels, block align {align}, {bits} bits)")
    n = len(payload) // align
    raw = np.frombuffer(payload[:n * align], dtype=np.uint8)
    if tag == 1 and bits == 8:
        x = (raw.astype(np.float64) - 128.0) / 128.0
    elif tag == 1 and bits == 16:
        x = raw.view("<i2").astype(np.float64) / 32768.0
    elif tag == 1 and bits == 24:
        b3 = raw.reshape(-1, 3).astype(np.int32)
        v = b3[:, 0] | (b3[:, 1] << 8) | (b3[:, 2] << 16)
        x = (np.where(v >= 1 << 23, v - (1 << 24), v)).astype(np.float64) / float(1 << 23)
    elif tag == 1 and bits == 32:
        x = raw.view("<i4").astype(np.float64) / float(1 << 31)
    elif tag == 3 and bits == 32:
        x = raw.view("<f4").astype(np.float64)
    elif tag == 3 and bits == 64:
        x = raw.view("<f8").copy()
    else:
        raise AudioError(f"{path}: unsupported sample format (tag {tag}, {bits} bits)")
    return x.reshape(n, ch), sr


# sample-format codes of svc_load_pcm (include/svc_hip.h SVC_PCM_*) by (format tag, bits per sample)
PCM_FORMATS = {(1, 8): 0, (1, 16): 1, (1, 24): 2, (1, 32): 3, (3, 32): 4, (3, 64): 5}
PCM_DTYPES = ("u1", "<i2", None, "<i4", "<f4", "<f8")  # numpy dtype of a format code's samples (24-bit: none)

# a parsed wav: format code, channels, sample rate, frames, and a view of the data chunk's first frames * align bytes
WavInfo = collections.namedtuple("WavInfo", "format channels sr n_frames payload name")


def parse_wav(src, name=None):
    """RIFF/WAVE header of `src` (a path, bytes or a memoryview) -> WavInfo, without touching the samples: the payload
    is a zero-copy view into the file's bytes. Accepts and rejects exactly what read_wav does (the same chunk walk:
    odd-sized chunks padded, the last fmt / data chunk wins, WAVE_FORMAT_EXTENSIBLE by its sub-format)."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        data, path = memoryview(src).cast("B"), name if name is not None else "<bytes>"
    else:
        path = src if name is None else name
        with open(src, "rb") as fh:
            data = memoryview(fh.read())
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise AudioError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, payload = 12, None, None
    while pos + 8 <= len(data):
        cid, size = bytes(data[pos:pos + 4]), struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            tag, ch, sr, _, align, bits = struct.unpack("<HHIIHH", body[:16])
            if tag == 0xFFFE and len(body) >= 26:
                tag = struct.unpack("<H", body[24:26])[0]
            fmt = (tag, ch, sr, align, bits)
        elif cid == b"data":
            payload = body
        pos += 8 + size + (size & 1)
    if fmt is None or payload is None:
        raise AudioError(f"{path}: missing fmt or data chunk")
    tag, ch, sr, align, bits = fmt
    if ch < 1 or align != ch * bits // 8:
        raise AudioError(f"{path}: unsupported layout ({ch} channels, block align {align}, {bits} bits)")
    n = len(payload) // align
    if (tag, bits) not in PCM_FORMATS:
        raise AudioError(f"{path}: unsupported sample format (tag {tag}, {bits} bits)")
    return WavInfo(PCM_FORMATS[(tag, bits)], ch, sr, n, payload[:n * align], str(path))


def _normalise(audio):
    """utils/audio.py:31-45: float data scaled by 1, 2^15+1 or 2^31+1 by its peak, then float32."""
    mx = max(float(np.amax(audio)), float(-np.amin(audio))) if audio.size else 0.0
    max_mag = (2 ** 31) + 1 if mx > 2 ** 15 else ((2 ** 15) + 1 if mx > 1.01 else 1.0)
    return (torch.from_numpy(audio.astype(np.float32)) / max_mag).numpy()


def resample(x, sr_in, sr_out, device="cuda", quantize16=False):
    """f32 [B, n] or [n] (host or device) -> device f32 at sr_out, on the current stream (svc_resample)."""
    xt = torch.as_tensor(x, dtype=torch.float32, device=device)
    squeeze = xt.dim() == 1
    if squeeze:
        xt = xt[None]
    xt = xt.contiguous()
    B, n_in = xt.shape
    n_out = _lib.load().svc_resample_len(n_in, sr_in, sr_out)
    y = torch.empty(B, n_out, device=xt.device, dtype=torch.float32)
    _lib.call("svc_resample", ctypes.c_void_p(xt.data_ptr()), B, n_in, sr_in, sr_out, 1 if quantize16 else 0,
              ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(xt.device).cuda_stream))
    return y[0] if squeeze else y


def load_audio(path, fs, device="cuda"):
    """utils/audio.py:10-55 for a wav: channel 0, peak-class normalisation, resample to fs on the GPU.
    Returns a device f32 tensor, or None where the reference returns [] (NaN / Inf samples)."""
    audio, sr = read_wav(path)
    audio = audio[:, 0]
    if len(audio) <= 2:
        raise AudioError(f"{path}: {len(audio)} samples")
    x = _normalise(audio)
    if not np.isfinite(x).all():
        return None
    if sr == fs:
        return torch.as_tensor(x, device=device)
    return resample(x, sr, fs, device=device)


def load_whisper_audio(path, sr=WHISPER_SR, device="cuda"):
    """utils/whisper_extractor/audio.py:22-49: mono down-mix (ffmpeg ac=1 averages the channels), resample to
    16 kHz and quantise to int16 / 32768 (the s16le pipe)."""
    audio, sr_in = read_wav(path)
    mono = audio.mean(axis=1).astype(np.float32)
    return resample(mono, sr_in, sr, device=device, quantize16=True)


def load_contentvec_audio(path, sr=WHISPER_SR, device="cuda"):
    """utils/hubert.py:137-143 librosa.load(path, sr=16000) for a wav: mono down-mix as float32, resampled to `sr`
    without quantisation, and not resampled at all when the file already is at `sr` (librosa.load's rule).
    Unpinned against librosa in two places: librosa's to_mono takes the mean of the float32 samples (equal to the
    float64 mean taken here, then rounded, for 1 and 2 channels; for more than 2 channels it may differ in the last
    bit), and librosa resamples with soxr where this is svc_resample's Kaiser polyphase filter."""
    audio, sr_in = read_wav(path)
    mono = audio.mean(axis=1).astype(np.float32)
    if sr_in == sr:
        return torch.as_tensor(mono, device=device)
    return resample(mono, sr_in, sr, device=device, quantize16=False)


def load_batch(sources, fs, engine, on_error="raise", float16k=False):
    """load_audio and load_whisper_audio for a batch of wav files (paths, bytes or memoryviews; or WavInfo already
    parsed) in ONE device stage: headers on the host, then one upload and one svc_load_pcm call
    (SVCEngine.load_pcm) -> (wavs24, wavs16), lists of per-utterance row views of the two padded batches (what
    SVCPipeline.convert_ragged takes), each row bit for bit the per-file function's result.
    AudioError naming the source: a file of <= 2 frames (load_audio), or one with non-finite samples (where load_audio
    returns None and infer.py raises). on_error="return": nothing is raised for a bad file; the result is
    (wavs24, wavs16, errors) with None for it in both lists and its exception in errors (a dict by position); the other
    files are decoded as usual.
    float16k=True: load_contentvec_audio as well, from the same call (svc_load_pcm_ex) -> (wavs24, wavs16,
    wavs16_float), or (wavs24, wavs16, wavs16_float, errors); a failed file is None in the third list too."""
    infos, errors = [], {}
    for i, src in enumerate(sources):
        try:
            info = src if isinstance(src, WavInfo) else parse_wav(src, None if isinstance(src, (str, os.PathLike))
                                                                else f"<source {i}>")
            if info.n_frames <= 2:
                raise AudioError(f"{info.name}: {info.n_frames} samples")
            if info.channels > 8:
                raise AudioError(f"{info.name}: {info.channels} channels (at most 8)")
            infos.append((i, info))
        except (AudioError, struct.error, OSError) as exc:
            if on_error == "raise":
                raise
            errors[i] = exc
    w24, w16, w16f = [None] * len(sources), [None] * len(sources), [None] * len(sources)
    if infos:
        if float16k:
            y24, y16, n24, n16, flags, y16f = engine.load_pcm([info for _, info in infos], fs, float_mono=True)
        else:
            y24, y16, n24, n16, flags = engine.load_pcm([info for _, info in infos], fs)
        # integer samples cannot be non-finite: the flags are fetched only when some file holds floats
        bits = flags.cpu().tolist() if any(info.format >= 4 for _, info in infos) else [0] * len(infos)
        for j, (i, info) in enumerate(infos):
            if bits[j] & 4:
                errors[i] = AudioError(f"{info.name}: non-finite samples")
                continue
            w24[i], w16[i] = y24[j, :n24[j]], y16[j, :n16[j]]
            if float16k:
                w16f[i] = y16f[j, :n16[j]]
    out = (w24, w16, w16f) if float16k else (w24, w16)
    if on_error == "raise":
        if errors:
            raise errors[min(errors)]
        return out
    return out + (errors,)


def to_pcm16(waveform, fs, add_silence=True, turn_up=True, volume_peak=0.9):
    """utils/util.py:20-37 sample conversion: peak to volume_peak, fs//20 zeros both sides,
    PCM_S16 = clip(round(x * 32768)) (matches gen/1100000814_svcc_CDF1.wav: peak -29491)."""
    w = np.asarray(waveform, dtype=np.float32)
    if turn_up:
        w = w * (volume_peak / max(float(w.max()), abs(float(w.min()))))
    if add_silence:
        sil = np.zeros((fs // 20,), dtype=w.dtype)
        w = np.concatenate([sil, w, sil])
    return np.clip(np.round(w.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def loudness_params(fs=None, window=None, hop=None):
    """(window, hop) of the loudness envelope: so-vits-svc's defaults fs // 2 * 2 and fs // 2 (a one-second frame
    every half second) for whichever is None, which then needs fs."""
    if (window is None or hop is None) and fs is None:
        raise ValueError("loudness_match: give fs, or both window and hop")
    window = int(fs) // 2 * 2 if window is None else int(window)
    hop = int(fs) // 2 if hop is None else int(hop)
    if window < 1 or hop < 1:
        raise ValueError(f"loudness_match: window {window}, hop {hop}: both >= 1")
    return window, hop


def check_loudness_mix(mix):
    """loudness_mix as a float in [0, 1], else ValueError before any device work; None (the stage is not run) stays
    None."""
    if mix is None:
        return None
    ok = isinstance(mix, (int, float, np.integer, np.floating)) and not isinstance(mix, (bool, np.bool_))
    if not ok or not 0.0 <= float(mix) <= 1.0:  # NaN fails both comparisons
        raise ValueError(f"loudness_mix {mix!r}: a number in [0, 1] (0: the source's envelope, 1: unchanged)")
    return float(mix)


def _frame_rms(s, K, window, hop):
    """E_k, k < K: frame k covers samples [k hop - window // 2, .. + window) of s (f64), zero outside [0, len(s))."""
    E = np.zeros(K, dtype=np.float64)
    for k in range(K):
        lo = k * hop - window // 2
        seg = s[max(lo, 0):max(min(lo + window, len(s)), 0)]
        E[k] = np.sqrt(math.fsum(seg * seg) / window)
    return E


def loudness_gains(y, x, fs=None, window=None, hop=None, mix=0.0, floor_rms=1e-6, max_gain=None):
    """The per-frame gains g_k, f64 [1 + len(y) // hop], of loudness_match (its arguments)."""
    window, hop = loudness_params(fs, window, hop)
    mix = check_loudness_mix(mix)
    if mix is None or not floor_rms > 0:
        raise ValueError("loudness_match: mix in [0, 1] and floor_rms > 0")
    y = np.asarray(y, dtype=np.float32).reshape(-1).astype(np.float64)
    x = np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64)
    K = 1 + len(y) // hop
    E1, E2 = _frame_rms(x, K, window, hop), _frame_rms(y, K, window, hop)
    g = (E1 / np.maximum(E2, float(floor_rms))) ** (1.0 - mix)
    if max_gain is not None and max_gain > 0:
        g = np.minimum(g, float(max_gain))
    return g


def loudness_match(y, x, fs=None, window=None, hop=None, mix=0.0, floor_rms=1e-6, max_gain=None):
    """Loudness envelope transfer for one clip (so-vits-svc's "loudness envelope adjustment", per-frame form; DESIGN.md
    "Loudness envelope transfer"): the output y f32 [n_out] takes the slow RMS envelope of the source x f32 [n_src]
    (same rate and time origin) -> f32 [n_out]. The definition svc_loudness_match is tested against, f64 inside:
      K = 1 + n_out // hop frames for both signals; frame k covers samples [k hop - window // 2, .. + window), zero
      outside the signal (librosa's rms(center=True) with zero padding); E_k = sqrt(sum s^2 / window);
      g_k = (E_x_k / max(E_y_k, floor_rms)) ** (1 - mix), then min(g_k, max_gain) with a max_gain > 0;
      out[i] = f32(y[i] * (g_k0 + frac * (g_k1 - g_k0))), k0 = i // hop, frac = (i - k0 hop) / hop,
      k1 = min(k0 + 1, K - 1).
    mix = 1 returns y; mix = 0 gives y the source's envelope. window / hop default to fs // 2 * 2 and fs // 2."""
    window, hop = loudness_params(fs, window, hop)
    g = loudness_gains(y, x, None, window, hop, mix, floor_rms, max_gain)
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    i = np.arange(len(y), dtype=np.int64)
    k0 = i // hop
    frac = (i - k0 * hop).astype(np.float64) / float(hop)
    k1 = np.minimum(k0 + 1, len(g) - 1)
    return (y.astype(np.float64) * (g[k0] + frac * (g[k1] - g[k0]))).astype(np.float32)


CHUNK_GRID = 15          # mel frames: 3840 samples at 24 kHz = 2560 at 16 kHz = 8 Whisper or HuBERT frames
VOCODER_FADE_FRAMES = 20  # the vocoder fades out the last 20 * hop samples of every utterance (runtime: vocoder.fade_out)
MAX_CHUNKS = 1 << 12      # chunk k of utterance u draws its noise as utterance (u << 12) | k, an int32 id
STITCH_EPS = 1e-8         # RVC's SOLA: nom / sqrt(den + 1e-8)

# The join's tables (svc_stitch's arguments; all in samples): chunk b has n[b] usable samples, its body is
# row[lead[b] : lead[b] + body[b]] before displacement and lands at out[out_off[b] : out_off[b] + body[b]]
StitchPlan = collections.namedtuple("StitchPlan", "n lead body joined out_off out_len xfade search eps")

# One song cut into chunks (chunk_plan). Per chunk, lists of length `chunks`: start / frames (its first source frame and
# its own frame count T_k), body (frames [b0, b1) of the song it is responsible for), rows24 / rows16 / rows16_float
# (the sample intervals [lo, hi) of the source signals it is converted from), noise_ids; stitch: its StitchPlan, with
# out_off relative to the song's first sample and out_len = T_song * hop
ChunkPlan = collections.namedtuple("ChunkPlan", "T_song hop Cb Lc Rc chunks start frames body rows24 rows16 "
                                                "rows16_float noise_ids stitch")


def chunk_plan(n_samples, fs=24000, hop=256, n_fft=1024, clip_s=10.0, context_s=0.64, xfade=1024, search=192,
               utt_id=0, n16=None, n16_float=None, eps=STITCH_EPS):
    """The chunks of a song of n_samples 24 kHz samples for long-form conversion (DESIGN.md "Long-form conversion") ->
    ChunkPlan. In mel frames, all multiples of 15 (CHUNK_GRID: a whole sample at 24 and 16 kHz and a whole frame of both
    content encoders): the body length Cb = clip_s * fs / hop rounded down (at least 15), the contexts Lc = Rc =
    context_s * fs / hop rounded up. A cut lies at frame k Cb, k >= 1, while k Cb + Rc < T_song; chunk k is converted
    from source frames [max(0, k Cb - Lc), (k + 1) Cb + Rc) (the last chunk: to the song's last sample) and is
    responsible for frames [k Cb, (k + 1) Cb) (the last chunk: to T_song). Its 16 kHz rows are the same interval times
    2 / 3, clipped to that signal's length (n16, n16_float; default: n_samples * 2 // 3 and none).
    The stitch tables: a chunk with a successor has n = T_k hop - 20 hop usable samples (the vocoder fades out the
    rest), the last chunk T_k hop. A joined last chunk can be displaced by up to search - 1 samples towards its end,
    where there is nothing left to play: its stitched body is that much shorter, and the song's last
    max(search - 1, 0) samples, the silent end of the vocoder's fade-out, stay zero.
    ValueError: Rc hop < xfade + search + 20 hop, Lc hop < search, xfade > 15 hop, xfade or search outside
    svc_stitch's ranges, more than 4096 chunks, utt_id outside [0, 2^19), a song of less than one frame."""
    from .runtime import mel_frames
    n_samples, fs, hop, xfade, search, utt_id = int(n_samples), int(fs), int(hop), int(xfade), int(search), int(utt_id)
    G = CHUNK_GRID
    if not clip_s > 0 or not context_s >= 0:
        raise ValueError(f"chunk_plan: clip_s {clip_s!r} must be positive and context_s {context_s!r} not negative")
    # the seconds as the short decimals they were written as (0.64 is 16 / 25, not the binary fraction next to it)
    sec = lambda v: fractions.Fraction(v).limit_denominator(1000000)
    Cb = max(math.floor(sec(clip_s) * fs / hop) // G * G, G)
    Lc = Rc = -(-math.ceil(sec(context_s) * fs / hop) // G) * G
    if not 1 <= xfade <= 8192 or not 0 <= search <= 1024:
        raise ValueError(f"chunk_plan: xfade {xfade} (1..8192), search {search} (0..1024)")
    if Rc * hop < xfade + search + VOCODER_FADE_FRAMES * hop:
        raise ValueError(f"chunk_plan: right context of {Rc * hop} samples is shorter than xfade + search + the "
                         f"vocoder's fade-out ({xfade} + {search} + {VOCODER_FADE_FRAMES * hop})")
    if Lc * hop < search:
        raise ValueError(f"chunk_plan: left context of {Lc * hop} samples is shorter than search {search}")
    if xfade > G * hop:
        raise ValueError(f"chunk_plan: xfade {xfade} is longer than the shortest body ({G * hop} samples)")
    if not 0 <= utt_id < (1 << 19):
        raise ValueError(f"chunk_plan: utterance id {utt_id} outside [0, 2^19): chunk noise ids are (id << 12) | k")
    T_song = mel_frames(n_samples, n_fft, hop)
    if T_song < 1:
        raise ValueError(f"chunk_plan: {n_samples} samples are less than one frame")
    K = 1
    while K * Cb + Rc < T_song:
        K += 1
        if K > MAX_CHUNKS:
            raise ValueError(f"chunk_plan: more than {MAX_CHUNKS} chunks of {Cb} frames in {T_song} frames")
    n16 = n_samples * 2 // 3 if n16 is None else int(n16)
    start, frames, body, rows24, rows16, rows16f = [], [], [], [], [], []
    sn, lead, sbody, joined, out_off = [], [], [], [], []
    for k in range(K):
        last = k == K - 1
        s = max(0, k * Cb - Lc)
        e = T_song if last else (k + 1) * Cb + Rc
        b0, b1 = k * Cb, (T_song if last else (k + 1) * Cb)
        lo, hi = s * hop, (n_samples if last else e * hop)
        start.append(s), frames.append(e - s), body.append((b0, b1)), rows24.append((lo, hi))
        lo16, hi16 = lo * 2 // 3, hi * 2 // 3
        rows16.append((min(lo16, n16), n16 if last else min(hi16, n16)))
        if n16_float is not None:
            rows16f.append((min(lo16, int(n16_float)), int(n16_float) if last else min(hi16, int(n16_float))))
        sn.append((e - s) * hop - (0 if last else VOCODER_FADE_FRAMES * hop))
        lead.append((b0 - s) * hop)
        sbody.append((b1 - b0) * hop - (max(search - 1, 0) if last and k > 0 else 0))
        joined.append(1 if k > 0 else 0)
        out_off.append(b0 * hop)
    for k in range(K):  # svc_stitch's range rule, whatever the contexts were clipped to
        d_lo, d_hi = (-search, max(search - 1, 0)) if joined[k] else (0, 0)
        tail = xfade if k + 1 < K else 0
        if lead[k] + d_lo < 0 or lead[k] + d_hi + sbody[k] + tail > sn[k] or (joined[k] and sbody[k] < xfade):
            raise ValueError(f"chunk_plan: chunk {k} of {K}: rows [{lead[k] + d_lo}, {lead[k] + d_hi + sbody[k] + tail}) "
                             f"of {sn[k]} usable samples")
    st = StitchPlan(sn, lead, sbody, joined, out_off, T_song * hop, xfade, search, float(eps))
    return ChunkPlan(T_song, hop, Cb, Lc, Rc, K, start, frames, body, rows24, rows16,
                     rows16f if n16_float is not None else None, [(utt_id << 12) | k for k in range(K)], st)


def merge_stitch_plans(plans, out_stride):
    """The StitchPlans of several songs (equal xfade, search, eps) as one: song i's out_off moved by i * out_stride."""
    p0 = plans[0]
    if any((p.xfade, p.search, p.eps) != (p0.xfade, p0.search, p0.eps) for p in plans):
        raise ValueError("merge_stitch_plans: the songs' xfade, search and eps differ")
    if any(p.out_len > out_stride for p in plans):
        raise ValueError("merge_stitch_plans: a song is longer than out_stride")
    cat = lambda f: [v for p in plans for v in getattr(p, f)]
    off = [v + i * int(out_stride) for i, p in enumerate(plans) for v in p.out_off]
    return StitchPlan(cat("n"), cat("lead"), cat("body"), cat("joined"), off, len(plans) * int(out_stride), p0.xfade,
                      p0.search, p0.eps)


def check_stitch_plan(plan, rows_len=None):
    """svc_stitch's argument rules on a StitchPlan (ValueError); rows_len: the rows' allocated lengths, each >= n[b]."""
    B = len(plan.n)
    X, R = int(plan.xfade), int(plan.search)
    if B < 1 or any(len(t) != B for t in (plan.lead, plan.body, plan.joined, plan.out_off)):
        raise ValueError("stitch: the tables need one entry per chunk, at least one chunk")
    if not 1 <= X <= 8192 or not 0 <= R <= 1024 or not plan.eps > 0 or plan.out_len < 1:
        raise ValueError(f"stitch: xfade {X} (1..8192), search {R} (0..1024), eps {plan.eps} (> 0), out_len {plan.out_len}")
    if plan.joined[0]:
        raise ValueError("stitch: chunk 0 is joined to a predecessor it does not have")
    for b in range(B):
        n, lead, body, j, off = plan.n[b], plan.lead[b], plan.body[b], plan.joined[b], plan.out_off[b]
        if j not in (0, 1) or n < 1 or body < 1 or off < 0 or off + body > plan.out_len:
            raise ValueError(f"stitch: chunk {b}: joined {j}, n {n}, body {body}, output [{off}, {off + body}) of "
                             f"{plan.out_len}")
        if rows_len is not None and rows_len[b] < n:
            raise ValueError(f"stitch: chunk {b}: a row of {rows_len[b]} samples, n {n}")
        if j and (off != plan.out_off[b - 1] + plan.body[b - 1] or body < X):
            raise ValueError(f"stitch: chunk {b} is joined: its output must start where chunk {b - 1}'s ends, and its "
                             f"body {body} must hold xfade {X}")
        d_lo, d_hi = (-R, max(R - 1, 0)) if j else (0, 0)
        tail = X if b + 1 < B and plan.joined[b + 1] else 0
        if lead < 0 or lead + d_lo < 0 or lead + d_hi + body + tail > n:
            raise ValueError(f"stitch: chunk {b}: rows [{lead + d_lo}, {lead + d_hi + body + tail}) are read, the row "
                             f"has [0, {n})")
    order = sorted(range(B), key=lambda b: plan.out_off[b])
    for x, y in zip(order, order[1:]):
        if plan.out_off[x] + plan.body[x] > plan.out_off[y]:
            raise ValueError(f"stitch: the output intervals of chunks {x} and {y} overlap")


def stitch_q(a, row, lead, xfade, search, eps):
    """q(d) of every candidate d in [-search, search) (d = 0 alone for search 0), f64 [max(2 search, 1)]: a f32
    [xfade] is the predecessor's continuation, the candidates' windows are row[lead + d : lead + d + xfade]. The sums
    run in f64 with j ascending (np.cumsum adds in order; pairwise np.sum would not)."""
    X, R = int(xfade), int(search)
    nc = max(2 * R, 1)
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    seg = np.asarray(row[lead - R:lead - R + X + nc - 1], dtype=np.float32).astype(np.float64)
    win = np.lib.stride_tricks.sliding_window_view(seg, X)  # [nc, X]: row k is candidate d = k - R
    nom = np.cumsum(win * a[None, :], axis=1)[:, -1]
    den = np.cumsum(win * win, axis=1)[:, -1]
    return (nom * np.abs(nom)) / (den + np.float64(eps))


def stitch_pick(q, search):
    """The displacement among candidates d = k - search (k indexes q): greater q, then smaller |d|, then greater d."""
    best_q, best_d = None, 0
    for k, qk in enumerate(q.tolist()):
        d = k - int(search)
        if best_q is None or qk > best_q or (qk == best_q and (abs(d) < abs(best_d) or (abs(d) == abs(best_d) and d > best_d))):
            best_q, best_d = qk, d
    return best_d


def stitch(rows, plan, return_shifts=False, return_q=False, chain=True):
    """Join converted chunks into their songs (DESIGN.md "Long-form conversion"); the definition svc_stitch is tested
    against, f64 inside. rows: B f32 arrays, chunk b's waveform with at least plan.n[b] samples; plan: a StitchPlan
    -> out f32 [plan.out_len], zeros wherever no body lands. With X = xfade, R = search and d_b the displacement of
    chunk b (0 unless joined), chunk b plays row sample lead[b] + d_b + j at out[out_off[b] + j], j < body[b]. A
    joined chunk b: its predecessor, as it was actually played, continues as a_j = rows[b-1][lead[b-1] + d_{b-1} +
    body[b-1] + j], j < X (so a song's seams form a chain); d_b is the candidate in [-R, R) first by greater
    q(d) = nom |nom| / (den + eps), then smaller |d|, then greater d, where nom = sum a_j c_j(d), den = sum c_j(d)^2,
    c_j(d) = rows[b][lead[b] + d + j], summed in f64 in ascending j (SOLA's nom / sqrt(den + eps) ordering without the
    root); its first X samples are f32(a_j + w_j (c_j(d_b) - a_j)), w_j = (j + 0.5) / X; everything else is copied bit
    for bit. return_shifts: also the displacements int32 [B]; return_q: also q f64 [B, max(2R, 1)] (0 for unjoined
    chunks). chain=False takes d_{b-1} as 0 in a_j (what a stitch without the chain would do: tests only)."""
    B = len(plan.n)
    rows = [np.asarray(r, dtype=np.float32).reshape(-1) for r in rows]
    if len(rows) != B:
        raise ValueError(f"stitch: {len(rows)} rows for {B} chunks")
    check_stitch_plan(plan, [len(r) for r in rows])
    X, R = int(plan.xfade), int(plan.search)
    out = np.zeros(int(plan.out_len), dtype=np.float32)
    shifts = np.zeros(B, dtype=np.int32)
    qs = np.zeros((B, max(2 * R, 1)), dtype=np.float64)
    for b in range(B):
        lead, body, off = int(plan.lead[b]), int(plan.body[b]), int(plan.out_off[b])
        if not plan.joined[b]:
            out[off:off + body] = rows[b][lead:lead + body]
            continue
        pa = int(plan.lead[b - 1]) + (int(shifts[b - 1]) if chain else 0) + int(plan.body[b - 1])
        a = rows[b - 1][pa:pa + X]
        qs[b] = stitch_q(a, rows[b], lead, X, R, plan.eps)
        d = shifts[b] = stitch_pick(qs[b], R)
        c = rows[b][lead + d:lead + d + body]
        out[off:off + body] = c
        a64, c64 = a.astype(np.float64), c[:X].astype(np.float64)
        w = (np.arange(X, dtype=np.float64) + 0.5) / np.float64(X)
        out[off:off + X] = (a64 + w * (c64 - a64)).astype(np.float32)
    res = (out,) + ((shifts,) if return_shifts else ()) + ((qs,) if return_q else ())
    return res if len(res) > 1 else out


def write_wav_pcm16(path, pcm, fs):
    pcm = np.asarray(pcm, dtype="<i2")
    body = pcm.tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE"
    hdr += b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, fs, fs * 2, 2, 16)
    hdr += b"data" + struct.pack("<I", len(body))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(hdr + body)


def save_audio(path, waveform, fs, add_silence=True, turn_up=True, volume_peak=0.9):
    """utils/util.py:20-37: 16-bit PCM mono wav."""
    write_wav_pcm16(path, to_pcm16(waveform, fs, add_silence, turn_up, volume_peak), fs)
