"""CPU: the host half of the input end (A1). audio.parse_wav takes read_wav's decisions without touching the samples;
svc_load_pcm is declared, bound, exported and checks its arguments before any HIP call (no GPU needed);
SVCServer.submit_file sizes a request from the header alone."""
import ctypes
import io
import os
import struct
import wave
from types import SimpleNamespace

import numpy as np
import pytest

from svc_inference_pipeline_amd import _lib
from svc_inference_pipeline_amd import audio as A
from svc_inference_pipeline_amd.runtime import mel_frames
from svc_inference_pipeline_amd.serving import SVCServer
from wav_util import F32, F64, S16, S24, S32, TAG_BITS, U8, decode_payload, random_samples, wav_bytes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = os.path.join(REPO, "tests", "golden", "test_set_1100000814.wav")


def test_header_declares_and_library_exports_load_pcm():
    txt = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    assert "svc_load_pcm        <- utils/audio.py:10-55 load_audio_torch + utils/whisper_extractor/audio.py:22-49" in txt
    for k, name in enumerate(("U8", "S16", "S24", "S32", "F32", "F64")):
        assert f"#define SVC_PCM_{name} {k}\n" in txt
    assert "svc_load_pcm" in _lib.PROTOTYPES and hasattr(_lib.load(), "svc_load_pcm")
    assert _lib.load().svc_abi_version() == 3  # additions only
    assert A.PCM_FORMATS == {TAG_BITS[f]: f for f in (U8, S16, S24, S32, F32, F64)}


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("fmt", [U8, S16, S24, S32, F32, F64])
def test_parse_wav_matches_read_wav(tmp_path, fmt, ch):
    """The header fields equal read_wav's (and the stdlib wave module's for the integer formats), and the payload
    view, reinterpreted in numpy, equals read_wav's samples exactly; a path, bytes and a memoryview give the same."""
    rng = np.random.default_rng(10 * fmt + ch)
    sr = [8000, 22050, 44100][ch - 1]
    data = wav_bytes(fmt, random_samples(rng, fmt, 257, ch), sr)
    path = str(tmp_path / "x.wav")
    open(path, "wb").write(data)
    ref, ref_sr = A.read_wav(path)
    for src in (path, data, memoryview(data)):
        info = A.parse_wav(src)
        assert (info.format, info.channels, info.sr, info.n_frames) == (fmt, ch, ref_sr, 257)
        assert isinstance(info.payload, memoryview) and len(info.payload) == 257 * ch * TAG_BITS[fmt][1] // 8
        assert np.array_equal(decode_payload(fmt, ch, info.payload), ref)
    assert info.payload.obj is data  # a view into the caller's bytes, not a copy
    assert A.parse_wav(path).name == path and A.parse_wav(data, name="req7").name == "req7"
    if fmt in (U8, S16, S24, S32):
        with wave.open(io.BytesIO(data), "rb") as f:
            assert (f.getnchannels(), f.getsampwidth() * 8, f.getframerate(), f.getnframes()) == \
                (info.channels, TAG_BITS[fmt][1], info.sr, info.n_frames)
            assert f.readframes(f.getnframes()) == bytes(info.payload)


def test_parse_wav_takes_read_wavs_decisions(tmp_path):
    """The test clip; a WAVE_FORMAT_EXTENSIBLE header; an odd-sized chunk before data (its pad byte skipped) and chunks
    after it; a data chunk cut short by the end of the file (whole frames only)."""
    ref, sr = A.read_wav(CLIP)
    info = A.parse_wav(CLIP)
    assert (info.format, info.channels, info.sr, info.n_frames) == (S16, ref.shape[1], sr, ref.shape[0])
    assert np.array_equal(decode_payload(info.format, info.channels, info.payload), ref)
    rng = np.random.default_rng(0)
    cases = {
        "extensible": wav_bytes(S24, random_samples(rng, S24, 33, 2), 48000, extensible=True),
        "extensible_float": wav_bytes(F32, random_samples(rng, F32, 33, 1), 16000, extensible=True),
        "odd_chunk": wav_bytes(S16, random_samples(rng, S16, 41, 1), 44100, before_data=[(b"LIST", b"abcde")],
                               after_data=[(b"id3 ", b"xyz")]),
        "cut_short": wav_bytes(S16, random_samples(rng, S16, 50, 2), 44100)[:-7],
    }
    for name, data in cases.items():
        path = str(tmp_path / (name + ".wav"))
        open(path, "wb").write(data)
        ref, sr = A.read_wav(path)
        info = A.parse_wav(data)
        assert (info.channels, info.sr, info.n_frames) == (ref.shape[1], sr, ref.shape[0]), name
        assert np.array_equal(decode_payload(info.format, info.channels, info.payload), ref), name
    assert A.parse_wav(cases["cut_short"]).n_frames == 48
    assert A.parse_wav(cases["odd_chunk"]).payload.obj is cases["odd_chunk"]


def test_parse_wav_raises_read_wavs_errors(tmp_path):
    good = wav_bytes(S16, np.zeros((8, 1), np.int64), 16000)
    fmt_chunk, data_chunk = good[12:36], good[36:]
    riff = lambda body: b"RIFF" + struct.pack("<I", len(body)) + body  # noqa: E731
    bad_align = bytearray(good)
    bad_align[32:34] = struct.pack("<H", 4)       # block align 4 for 1 x 16 bits
    adpcm = bytearray(good)
    adpcm[20:22] = struct.pack("<H", 2)           # format tag 2
    cases = {
        "not_riff": b"RIFX" + good[4:],
        "short": good[:10],
        "no_fmt": riff(b"WAVE" + data_chunk),
        "no_data": riff(b"WAVE" + fmt_chunk),
        "layout": bytes(bad_align),
        "format": bytes(adpcm),
        "zero_channels": good[:22] + struct.pack("<H", 0) + good[24:],
    }
    for name, data in cases.items():
        path = str(tmp_path / (name + ".wav"))
        open(path, "wb").write(data)
        with pytest.raises(A.AudioError) as want:
            A.read_wav(path)
        with pytest.raises(A.AudioError) as got:
            A.parse_wav(path)
        assert str(got.value) == str(want.value), name
        with pytest.raises(A.AudioError):
            A.parse_wav(data)


def _call(ctx=True, raw=True, B=1, byte_off=(0,), n_frames=(10,), fmt=(S16,), ch=(1,), sr=(44100,), sr_src=24000,
          S_src=16, y_src=True, sr_mono=16000, S_mono=16, y_mono=True, tables=True):
    """svc_load_pcm on host stand-ins: no argument below gets as far as a HIP call. ctx / raw / outputs are non-null
    pointers to host buffers that a failing call never reads."""
    keep = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(keep, ctypes.c_void_p)
    n = max(1, len(byte_off))
    i64 = lambda v: (ctypes.c_int64 * n)(*v) if tables else None  # noqa: E731
    i32 = lambda v: (ctypes.c_int32 * n)(*v) if tables else None  # noqa: E731
    lib = _lib.load()
    st = lib.svc_load_pcm(p if ctx else None, p if raw else None, B, i64(byte_off), i64(n_frames), i32(fmt), i32(ch),
                          i32(sr), sr_src, S_src, p if y_src else None, sr_mono, S_mono, p if y_mono else None, None,
                          None)
    return st, lib.svc_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(ctx=False), "null context"),
    (dict(raw=False), "null raw"),
    (dict(tables=False), "null byte_off table"),
    (dict(y_src=False, y_mono=False), "null y_src and y_mono"),
    (dict(B=0), "B=0"),
    (dict(B=-3), "B=-3"),
    (dict(ch=(0,)), "0 channels"),
    (dict(ch=(9,)), "9 channels"),
    (dict(fmt=(6,)), "unknown format 6"),
    (dict(fmt=(-1,)), "unknown format -1"),
    (dict(sr=(0,)), "rate 0"),
    (dict(sr_src=0), "sr_src=0"),
    (dict(sr_mono=-16000), "sr_mono=-16000"),
    (dict(n_frames=(-1,)), "negative length"),
    (dict(byte_off=(-2,)), "negative length or offset"),
    (dict(S_src=5), "6 source samples, S_src 5"),      # 10 frames at 44.1 kHz are 6 samples at 24 kHz
    (dict(S_mono=3), "4 mono samples, S_mono 3"),      # and 4 at 16 kHz
    (dict(S_src=0), "S_src=0"),
    (dict(sr=(16000000,), n_frames=(0,)), "too large for the filter tile"),
    (dict(B=2, byte_off=(0, 0), n_frames=(1, 1), fmt=(S16, S16), ch=(1, 12), sr=(8000, 8000)), "utterance 1: 12 channels"),
])
def test_load_pcm_rejects_bad_arguments_before_any_hip_call(kw, msg):
    st, err = _call(**kw)
    assert st == 1, (st, err)
    assert err.startswith("load_pcm:") and msg in err, err
    with pytest.raises(_lib.SVCError, match="load_pcm"):
        _lib.check(st)


def test_submit_file_sizes_the_request_from_the_header():
    """Nothing is decoded at submit time: the frame count the batcher sorts by is mel_frames(svc_resample_len(frames,
    rate, fs)), 379 for the test clip (the reference's 1200 + 379 * 256 + 1200 output samples); a file that cannot be
    queued fails its own future and nothing else."""
    cfg = SimpleNamespace(n_fft=1024, hop_length=256, fs=24000)
    srv = SVCServer(SimpleNamespace(engine=SimpleNamespace(cfg=cfg, device=None)), max_batch=4, max_wait_s=30.0)
    try:
        info = A.parse_wav(CLIP)
        want = mel_frames(int(_lib.load().svc_resample_len(info.n_frames, info.sr, 24000)), 1024, 256)
        data = open(CLIP, "rb").read()
        for src in (CLIP, data):
            req = srv._file_request(src, singer=3, utt_id=9)
            assert req.frames == want == 379 and req.file.n_frames == info.n_frames
            assert req.wav24 is None and req.wav16 is None and not req.future.done()
        for bad in (data[:40], wav_bytes(S16, np.zeros((2, 1), np.int64), 16000), b"junk"):
            fut = srv.submit_file(bad, singer=0)
            assert isinstance(fut.exception(timeout=1), (A.AudioError, struct.error))
        assert not srv._pending
    finally:
        srv.close()
