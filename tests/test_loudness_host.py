"""CPU: loudness envelope transfer's host side. audio.loudness_match (the definition svc_loudness_match is tested
against) on known answers and on one case framed by hand; the C-ABI symbols are declared, bound and exported with the ABI
version unchanged; every Python layer takes `loudness_mix`, runs the stage between the vocoder and the sample conversion
with the lengths it already holds, leaves it out for None and rejects a bad value before any device work; SVCServer
never puts two values in one batch; the CLI flag parses."""
import contextlib
import ctypes
import os
import re
import threading
import types

import numpy as np
import pytest
import torch

from svc_inference_pipeline_amd import _lib
from svc_inference_pipeline_amd import audio as A
from svc_inference_pipeline_amd import config as C
from svc_inference_pipeline_amd.pipeline import SVCPipeline
from svc_inference_pipeline_amd.serving import SVCServer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("W,H", [(512, 256), (511, 256), (100, 256), (4000, 256), (7, 1)])
@pytest.mark.parametrize("mix", [0.0, 0.25, 1.0])
def test_constant_signals_known_gain(W, H, mix):
    """Two constant signals of equal length: the zero padding cuts the same samples out of both frames, so every gain
    is (a1 / a2) ** (1 - mix) and every sample a2 times it. W odd, W < H and W > n are all here (n = 1000)."""
    n, a1, a2 = 1000, 0.5, 0.125
    y, x = np.full(n, a2, np.float32), np.full(n, a1, np.float32)
    g = A.loudness_gains(y, x, window=W, hop=H, mix=mix)
    assert g.shape == (1 + n // H,)
    want = (a1 / a2) ** (1.0 - mix)
    assert np.all(np.abs(g - want) <= 1e-12 * want)
    out = A.loudness_match(y, x, window=W, hop=H, mix=mix)
    assert out.dtype == np.float32 and out.shape == (n,)
    assert np.all(np.abs(out.astype(np.float64) - a2 * want) <= 2.0 ** -23 * a2 * want)  # one f32 rounding


def test_mix_one_returns_y_exactly():
    rng = np.random.default_rng(0)
    y = rng.standard_normal(777).astype(np.float32)
    x = np.zeros(500, np.float32)  # even under a silent source: pow(0, 0) = 1
    assert np.array_equal(A.loudness_match(y, x, window=100, hop=64, mix=1.0), y)
    assert np.array_equal(A.loudness_match(y, 3 * y, window=101, hop=64, mix=1), y)


def test_silent_source_gives_zeros_and_silent_output_is_bounded():
    rng = np.random.default_rng(1)
    y = rng.standard_normal(600).astype(np.float32)
    assert not A.loudness_match(y, np.zeros(600, np.float32), window=128, hop=64, mix=0.0).any()
    assert not A.loudness_match(y, np.zeros(600, np.float32), window=128, hop=64, mix=0.5).any()
    # a silent output under a loud source: the gain is E1 / floor_rms, finite, and the samples stay zero
    x = np.full(600, 0.5, np.float32)
    g = A.loudness_gains(np.zeros(600, np.float32), x, window=128, hop=64, floor_rms=1e-3)
    assert np.all(np.isfinite(g)) and g.max() <= 0.5 / 1e-3 * (1 + 1e-12)
    assert g[2] == pytest.approx(500.0, rel=1e-12)  # a frame inside the signal
    assert not A.loudness_match(np.zeros(600, np.float32), x, window=128, hop=64).any()
    # an almost silent output: bounded by floor_rms, and by max_gain when given
    tiny = np.full(600, 1e-9, np.float32)
    assert A.loudness_gains(tiny, x, window=128, hop=64, floor_rms=1e-3)[2] == pytest.approx(500.0, rel=1e-12)
    capped = A.loudness_gains(tiny, x, window=128, hop=64, floor_rms=1e-3, max_gain=4.0)
    assert np.array_equal(capped, np.full(10, 4.0))
    out = A.loudness_match(tiny, x, window=128, hop=64, floor_rms=1e-3, max_gain=4.0)
    assert np.array_equal(out, (tiny.astype(np.float64) * 4.0).astype(np.float32))
    for nocap in (None, 0.0, -1.0):
        assert A.loudness_gains(tiny, x, window=128, hop=64, floor_rms=1e-3, max_gain=nocap)[2] > 400


def test_single_frame_and_source_lengths():
    """K = 1 (n_out < hop): one gain for every sample. A source shorter or longer than the output changes only what its
    frames hold."""
    y = np.full(50, 0.25, np.float32)
    for n_src, inside in ((20, 20), (50, 32), (400, 32)):  # frame 0 covers samples [-32, 32)
        x = np.full(n_src, 0.5, np.float32)
        g = A.loudness_gains(y, x, window=64, hop=64)
        assert g.shape == (1,)
        want = np.sqrt(inside * 0.25 / 64) / np.sqrt(32 * 0.0625 / 64)
        assert g[0] == pytest.approx(want, rel=1e-12)
        out = A.loudness_match(y, x, window=64, hop=64)
        assert np.array_equal(out, np.full(50, np.float32(0.25 * g[0])))
    assert A.loudness_match(np.zeros(0, np.float32), np.ones(9, np.float32), window=4, hop=3).shape == (0,)
    assert A.loudness_gains(np.zeros(0, np.float32), np.ones(9, np.float32), window=4, hop=3).shape == (1,)


def test_framing_by_hand():
    """n = 10, W = 4, H = 3: K = 1 + 10 // 3 = 4 and frame k covers samples [3k - 2, 3k + 2):
         k = 0: (-2 -1) 0 1        k = 1: 1 2 3 4        k = 2: 4 5 6 7        k = 3: 7 8 9 (10)
    with y = 1 everywhere E2 = sqrt(count / 4) = sqrt(2/4), 1, 1, sqrt(3/4). Sample i uses k0 = i // 3, frac = (i % 3) / 3
    and k1 = min(k0 + 1, 3): sample 9 is the only one of the last, partial hop and takes g_3 alone."""
    x = np.arange(1, 11, dtype=np.float32)  # sample i holds i + 1
    y = np.ones(10, np.float32)
    sq = lambda idx: float(sum((i + 1) ** 2 for i in idx))
    E1 = np.sqrt(np.array([sq([0, 1]), sq([1, 2, 3, 4]), sq([4, 5, 6, 7]), sq([7, 8, 9])]) / 4.0)
    E2 = np.sqrt(np.array([2, 4, 4, 3]) / 4.0)
    g = A.loudness_gains(y, x, window=4, hop=3, mix=0.0)
    assert g.shape == (4,)
    assert np.all(np.abs(g - E1 / E2) <= 1e-14 * (E1 / E2))
    out = A.loudness_match(y, x, window=4, hop=3, mix=0.0)
    want = [g[0], g[0] + (g[1] - g[0]) / 3, g[0] + 2 * (g[1] - g[0]) / 3,
            g[1], g[1] + (g[2] - g[1]) / 3, g[1] + 2 * (g[2] - g[1]) / 3,
            g[2], g[2] + (g[3] - g[2]) / 3, g[2] + 2 * (g[3] - g[2]) / 3,
            g[3]]
    assert np.all(np.abs(out.astype(np.float64) - np.array(want)) <= 2.0 ** -23 * np.array(want))  # one f32 rounding
    assert out[9] == np.float32(g[3])
    # a shorter source: frame 3 holds sample 7 only, frame 2 samples 4..7
    g8 = A.loudness_gains(y, x[:8], window=4, hop=3)
    assert g8[3] == pytest.approx(np.sqrt(sq([7]) / 4.0) / E2[3], rel=1e-14) and g8[2] == pytest.approx(g[2], rel=1e-14)


def test_defaults_and_argument_errors():
    assert A.loudness_params(24000) == (24000, 12000) and A.loudness_params(22051) == (22050, 11025)
    assert A.loudness_params(None, 7, 3) == (7, 3) and A.loudness_params(24000, hop=5) == (24000, 5)
    y = np.ones(8, np.float32)
    with pytest.raises(ValueError, match="fs"):
        A.loudness_match(y, y)
    with pytest.raises(ValueError, match="window"):
        A.loudness_match(y, y, window=0, hop=3)
    for bad in (-0.1, 1.5, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="loudness_mix"):
            A.loudness_match(y, y, window=4, hop=3, mix=bad)
    with pytest.raises(ValueError, match="floor_rms"):
        A.loudness_match(y, y, window=4, hop=3, floor_rms=0.0)
    assert A.check_loudness_mix(None) is None and A.check_loudness_mix(1) == 1.0
    assert A.check_loudness_mix(np.float32(0.5)) == 0.5


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    lib = _lib.load()
    assert re.search(r"^svc_status\s+svc_loudness_match\s*\(", header, re.M)
    assert re.search(r"^int64_t\s+svc_loudness_frames\s*\(", header, re.M)
    assert "svc_loudness_match  <-" in header  # the opening list of entry points
    for name in ("svc_loudness_match", "svc_loudness_frames"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.svc_abi_version() == _lib.ABI_VERSION == 3  # additions only


def test_loudness_frames_edge_values():
    lib = _lib.load()
    assert lib.svc_loudness_frames(0, 1) == 1 and lib.svc_loudness_frames(0, 12000) == 1
    assert lib.svc_loudness_frames(10, 3) == 4 and lib.svc_loudness_frames(9, 3) == 4 and lib.svc_loudness_frames(8, 3) == 3
    assert lib.svc_loudness_frames(255, 256) == 1 and lib.svc_loudness_frames(256, 256) == 2
    assert lib.svc_loudness_frames(240000, 12000) == 21 and lib.svc_loudness_frames(4320000, 12000) == 361
    assert lib.svc_loudness_frames(2 ** 40, 1) == 2 ** 40 + 1
    assert lib.svc_loudness_frames(-1, 3) == -1 and lib.svc_loudness_frames(5, 0) == -1
    assert lib.svc_loudness_frames(5, -2) == -1


def test_null_context_is_an_error_with_a_message():
    lib = _lib.load()
    buf = ctypes.cast((ctypes.c_float * 4)(), ctypes.c_void_p)
    st = lib.svc_loudness_match(None, buf, buf, 1, 4, 4, None, None, 4, 2, 0.0, 1e-6, 0.0, buf, None, None)
    assert st == 1  # SVC_ERR_INVALID, before any HIP call
    with pytest.raises(_lib.SVCError, match="loudness_match"):
        _lib.call("svc_loudness_match", None, buf, buf, 1, 4, 4, None, None, 4, 2, 0.0, 1e-6, 0.0, buf, None, None)


# ------------------------------------------------------------------------------------------------ keyword plumbing
class _RecordingEngine:
    """CPU stand-in for SVCEngine: every stage returns zeros of the right shape and records its name; loudness_match
    and pcm16 record what they were given."""
    ragged_hubert = ragged_whisper = False

    def __init__(self):
        self.cfg = C.load_config()
        self.cfg.mapper.content_feature = ["whisper"]
        self.calls = []
        self.lock = threading.RLock()
        self.content_dtype = torch.float16
        self.singer_f0 = None
        self.target_f0_median = 0.0

    def mel_energy(self, w24, n_samples=None):
        self.calls.append(("mel",))
        B, N = w24.shape
        T = (N + 768 - 1024) // 256 + 1
        return torch.zeros(B, T, 100), torch.zeros(B, T)

    def f0(self, w24, T, n_samples=None):
        return torch.zeros(w24.shape[0], T, dtype=torch.float64)

    def pitch_shift(self, f0):
        return f0

    def whisper_encode(self, w16):
        return torch.zeros(w16.shape[0], 1500, 1024)

    def map_content(self, feats, T, rule="whisper", out=None):
        return feats[:, :1].expand(-1, T, -1).half()

    def condition(self, content, f0, energy, singer):
        return content[:, :, :384].float()

    def diffsvc_sample(self, cond, **kw):
        self.calls.append(("sample",))
        return cond[:, :, :100].clone()

    def bigvgan(self, x0, frames=None):
        self.calls.append(("bigvgan",))
        return torch.full((x0.shape[0], x0.shape[1] * 256), 0.5)

    def loudness_match(self, wav, src, n_samples=None, src_samples=None, mix=0.0, out=None, **kw):
        assert not kw, kw  # window, hop, floor_rms, max_gain stay at the engine's defaults
        self.calls.append(("loudness", tuple(wav.shape), tuple(src.shape), n_samples, src_samples, mix, out is wav))
        out.mul_(2.0)  # visible downstream: pcm16 and the caller get the adjusted tensor
        return out

    def pcm16(self, wav, n_samples=None):
        self.calls.append(("pcm16", float(wav[0, 0]), n_samples))
        return torch.zeros(wav.shape[0], wav.shape[1] + 2400, dtype=torch.int16)


@pytest.fixture
def cpu_streams(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(wait_stream=lambda s: None))
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None)  # convert() records its side-stream tensors


def test_convert_ragged_runs_the_stage_between_vocoder_and_pcm(cpu_streams):
    eng = _RecordingEngine()
    pipe = SVCPipeline(eng, f0_side=False)
    lens = [2400, 4800, 1000]
    T_b = [(n + 768 - 1024) // 256 + 1 for n in lens]
    w24 = [torch.zeros(n) for n in lens]
    w16 = [torch.zeros(n * 2 // 3) for n in lens]
    outs = pipe.convert_ragged(w24, w16, [0, 1, 2], loudness_mix=0.25, pcm16=True)
    kinds = [c[0] for c in eng.calls]
    assert kinds.count("loudness") == 1
    assert kinds.index("bigvgan") + 1 == kinds.index("loudness") == kinds.index("pcm16") - 1
    call = eng.calls[kinds.index("loudness")]
    # the padded vocoder output against the padded 24 kHz batch, each clip's own T_b * hop and source length, in place
    assert call[1:] == ((3, max(T_b) * 256), (3, 4800), [t * 256 for t in T_b], lens, 0.25, True)
    assert eng.calls[kinds.index("pcm16")][1:] == (1.0, [t * 256 for t in T_b])  # the adjusted waveform
    assert [o.shape[0] for o in outs] == [t * 256 + 2400 for t in T_b]
    # without pcm16 the adjusted f32 rows come back
    outs = pipe.convert_many(w24, w16, [0, 1, 2], loudness_mix=0)
    assert all(bool((o == 1.0).all()) and o.shape == (t * 256,) for o, t in zip(outs, T_b))
    assert eng.calls[-1][0] == "loudness" and eng.calls[-1][5] == 0.0


def test_convert_and_bucketed_route_run_the_stage(cpu_streams):
    eng = _RecordingEngine()
    pipe = SVCPipeline(eng, f0_side=False)
    res = pipe.convert(torch.zeros(2, 2500), torch.zeros(2, 1600), torch.zeros(2, dtype=torch.int32),
                       loudness_mix=1.0, pcm16=True)
    kinds = [c[0] for c in eng.calls]
    assert kinds.index("bigvgan") + 1 == kinds.index("loudness") == kinds.index("pcm16") - 1
    # equal lengths: no tables, the whole rows (T * hop = 2304 <= 2500 source samples)
    assert eng.calls[kinds.index("loudness")][1:] == ((2, 2304), (2, 2500), None, None, 1.0, True)
    assert bool((res.wav == 1.0).all()) and eng.calls[kinds.index("pcm16")][1] == 1.0
    eng.calls.clear()
    w24 = [torch.zeros(2400), torch.zeros(4800), torch.zeros(2400)]
    w16 = [torch.zeros(1600), torch.zeros(3200), torch.zeros(1600)]
    outs = pipe.convert_many(w24, w16, [0, 1, 2], bucketed=True, loudness_mix=0.5)
    loud = [c for c in eng.calls if c[0] == "loudness"]
    assert [c[1][0] for c in loud] == [2, 1] and all(c[5] == 0.5 for c in loud)  # one call per length bucket
    assert all(bool((o == 1.0).all()) for o in outs)


def test_none_leaves_the_stage_out(cpu_streams):
    eng = _RecordingEngine()
    pipe = SVCPipeline(eng, f0_side=False)
    w24, w16 = [torch.zeros(2400), torch.zeros(4800)], [torch.zeros(1600), torch.zeros(3200)]
    for kw in ({}, dict(loudness_mix=None)):
        outs = pipe.convert_ragged(w24, w16, [0, 1], **kw)
        assert all(bool((o == 0.5).all()) for o in outs)
        pipe.convert_many(w24, w16, [0, 1], bucketed=True, pcm16=True, **kw)
        res = pipe.convert(torch.zeros(1, 2500), torch.zeros(1, 1600), torch.zeros(1, dtype=torch.int32), **kw)
        assert bool((res.wav == 0.5).all())
    assert "loudness" not in [c[0] for c in eng.calls]
    assert all(c[1] == 0.5 for c in eng.calls if c[0] == "pcm16")


class _NoDeviceEngine:
    """An engine whose every stage fails the test: a bad loudness_mix must be rejected before any of them runs."""
    ragged_hubert = ragged_whisper = False

    def __init__(self):
        self.cfg = C.load_config()
        self.lock = threading.RLock()

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached with a bad loudness_mix")


@pytest.mark.parametrize("bad", [-0.01, 1.01, float("nan"), "0.5"])
def test_pipeline_rejects_bad_value_before_device_work(bad):
    pipe = SVCPipeline(_NoDeviceEngine())
    w24, w16 = torch.zeros(1, 2400), torch.zeros(1, 1600)
    with pytest.raises(ValueError, match="loudness_mix"):
        pipe.convert(w24, w16, torch.zeros(1, dtype=torch.int32), loudness_mix=bad)
    for bucketed in (False, True):
        with pytest.raises(ValueError, match="loudness_mix"):
            pipe.convert_many([w24[0]], [w16[0]], [0], bucketed=bucketed, loudness_mix=bad)
    with pytest.raises(ValueError, match="loudness_mix"):
        pipe.convert_ragged([w24[0]], [w16[0]], [0], loudness_mix=bad)
    with pytest.raises(ValueError, match="loudness_mix"):
        pipe.convert_files([b"not read"], [0], loudness_mix=bad)


def test_convert_files_passes_the_value_on(monkeypatch):
    pipe = SVCPipeline(_NoDeviceEngine())
    seen = []
    monkeypatch.setattr(A, "load_batch", lambda sources, fs, engine, **kw: (["w24"], ["w16"]) + ((["w16f"],) if kw else ()))
    monkeypatch.setattr(pipe, "convert_ragged", lambda *a, **kw: seen.append(kw) or ["out"])
    assert pipe.convert_files([b"x"], [0], loudness_mix=0.75) == ["out"]
    assert pipe.convert_files([b"x"], [0]) == ["out"]
    assert seen[0]["loudness_mix"] == 0.75 and "loudness_mix" not in seen[1]


class FakePipeline:
    """convert_ragged stand-in (as tests/test_serving.py's): records each batch's utterance ids and keywords."""

    def __init__(self):
        self.engine = types.SimpleNamespace(cfg=types.SimpleNamespace(n_fft=1024, hop_length=256), device=None)
        self.calls = []

    def convert_ragged(self, wavs24, wavs16, singers, wavs16_float=None, utt_ids=None, **kw):
        self.calls.append((list(utt_ids), kw))
        return [w * (s + 1) + u for w, s, u in zip(wavs24, singers, utt_ids)]


def test_server_never_mixes_loudness_values():
    p = FakePipeline()
    mixes = [None, 0.0, 0.0, None, 0.5, 0.0, 1]
    # nothing runs before close(): fewer requests than max_batch and a long max_wait_s; closing drains the queue
    with SVCServer(p, max_batch=8, max_wait_s=60.0, speedup=250, seed=3) as srv:
        futs = [srv.submit(torch.full((2000,), 0.5), torch.ones(1000), singer=0, loudness_mix=m) for m in mixes]
        for bad in (-1, 2.0, float("nan")):
            with pytest.raises(ValueError, match="loudness_mix"):
                srv.submit(torch.ones(2000), torch.ones(1000), singer=0, loudness_mix=bad)
        with pytest.raises(ValueError, match="loudness_mix"):
            srv.submit_file(b"RIFF", singer=0, loudness_mix=7)
        fut = srv.submit_file(b"not a wav file", singer=0, loudness_mix=0.5)
        assert fut.done() and fut.exception() is not None  # a bad file fails its own future, as before
    outs = [f.result(timeout=10) for f in futs]
    # equal lengths: only the value separates them (0.0 is not None); the oldest request's value forms each batch
    assert list(srv.batches) == [[0, 3], [1, 2, 5], [4], [6]]
    base = dict(fast_inference=True, speedup=250, seed=3)
    assert [kw for _, kw in p.calls] == [base, dict(base, loudness_mix=0.0), dict(base, loudness_mix=0.5),
                                         dict(base, loudness_mix=1.0)]
    for i, o in enumerate(outs):
        assert torch.equal(o, torch.full((2000,), 0.5) + i)


def test_cli_flag(capsys):
    from svc_inference_pipeline_amd import infer
    ap = infer.build_parser()
    assert ap.parse_args(["--wav", "a.wav"]).loudness_mix is None
    assert ap.parse_args(["--wav", "a.wav", "--loudness-mix", "0.25"]).loudness_mix == 0.25
    assert ap.parse_args(["--wav", "a.wav", "--loudness-mix", "0", "--fast"]).loudness_mix == 0.0
    for bad in ("1.5", "-0.1", "nan"):
        with pytest.raises(SystemExit) as exc:  # before any model is loaded
            infer.main(["--wav", "a.wav", "--loudness-mix", bad, "--random-weights", "tiny-test"])
        assert exc.value.code == 2 and "loudness_mix" in capsys.readouterr().err
