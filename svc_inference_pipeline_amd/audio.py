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
