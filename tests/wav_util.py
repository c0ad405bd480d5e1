"""Synthetic RIFF/WAVE files for the input-end tests (test_load_pcm_host.py, test_gpu_load_pcm.py): every sample
format svc_load_pcm decodes, any channel count, optional WAVE_FORMAT_EXTENSIBLE header and extra chunks."""
import struct

import numpy as np

U8, S16, S24, S32, F32, F64 = range(6)               # include/svc_hip.h SVC_PCM_*
TAG_BITS = {U8: (1, 8), S16: (1, 16), S24: (1, 24), S32: (1, 32), F32: (3, 32), F64: (3, 64)}


def random_samples(rng, fmt, n, ch, amp=0.5):
    """[n, ch] samples in the format's own type: integers over the whole range (int32 array), floats within amp"""
    if fmt in (F32, F64):
        return (rng.uniform(-amp, amp, (n, ch))).astype(np.float32 if fmt == F32 else np.float64)
    bits = TAG_BITS[fmt][1]
    lo, hi = (0, 256) if fmt == U8 else (-(1 << (bits - 1)), 1 << (bits - 1))
    x = rng.integers(lo, hi, (n, ch), dtype=np.int64)
    x[0, 0], x[-1, -1] = lo, hi - 1  # the extremes are present
    return x


def payload_bytes(fmt, samples):
    """samples [n, ch] (random_samples' types) -> the data chunk's bytes, little-endian, interleaved"""
    x = np.asarray(samples)
    if fmt == U8:
        return x.astype(np.uint8).tobytes()
    if fmt == S16:
        return x.astype("<i2").tobytes()
    if fmt == S24:
        v = x.astype(np.int64).reshape(-1) & 0xFFFFFF
        return np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).tobytes()
    if fmt == S32:
        return x.astype("<i4").tobytes()
    return x.astype("<f4" if fmt == F32 else "<f8").tobytes()


def wav_bytes(fmt, samples, sr, extensible=False, before_data=(), after_data=()):
    """A whole file. before_data / after_data: extra (id, body) chunks around the data chunk (an odd-sized body is
    followed by its pad byte)."""
    x = np.asarray(samples)
    ch = x.shape[1]
    tag, bits = TAG_BITS[fmt]
    align = ch * bits // 8
    if extensible:
        guid = struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt_body = struct.pack("<HHIIHH", 0xFFFE, ch, sr, sr * align, align, bits) + struct.pack("<HHI", 22, bits, 0) + guid
    else:
        fmt_body = struct.pack("<HHIIHH", tag, ch, sr, sr * align, align, bits)

    def chunk(cid, body):
        return cid + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")

    body = b"WAVE" + chunk(b"fmt ", fmt_body)
    for cid, b in before_data:
        body += chunk(cid, b)
    body += chunk(b"data", payload_bytes(fmt, x))
    for cid, b in after_data:
        body += chunk(cid, b)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def decode_payload(fmt, ch, payload):
    """The documented decode (audio.read_wav's) of a payload view, in numpy: f64 [n, ch]"""
    raw = np.frombuffer(payload, dtype=np.uint8)
    if fmt == U8:
        x = (raw.astype(np.float64) - 128.0) / 128.0
    elif fmt == S16:
        x = raw.view("<i2").astype(np.float64) / 32768.0
    elif fmt == S24:
        b3 = raw.reshape(-1, 3).astype(np.int32)
        v = b3[:, 0] | (b3[:, 1] << 8) | (b3[:, 2] << 16)
        x = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.float64) / float(1 << 23)
    elif fmt == S32:
        x = raw.view("<i4").astype(np.float64) / float(1 << 31)
    elif fmt == F32:
        x = raw.view("<f4").astype(np.float64)
    else:
        x = raw.view("<f8").copy()
    return x.reshape(-1, ch)
