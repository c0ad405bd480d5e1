"""CPU: A4 per singer without a GPU. The two entry points (svc_f0_voiced_median, svc_pitch_shift_ex) are declared, bound
and exported, and check their arguments before any device call; SingerF0Table round-trips exactly; the pipeline picks
a target per utterance, keeps the scalar call when there is nothing per utterance to do, and carries key shifts to the
engine as 2 ** (k / 12); the server carries them per request; the CLI has the three options."""
import contextlib
import ctypes
import math
import os
import re
import threading
import types

import pytest
import torch

from svc_inference_pipeline_amd import _lib
from svc_inference_pipeline_amd.pipeline import SVCPipeline
from svc_inference_pipeline_amd.serving import SVCServer
from svc_inference_pipeline_amd.singers import SingerF0Table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLOBAL = 223.25784012425046


def test_header_declares_and_library_exports_both_entries():
    txt = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    assert re.search(r"^svc_status\s+svc_f0_voiced_median\s*\(", txt, re.M)
    assert re.search(r"^svc_status\s+svc_pitch_shift_ex\s*\(", txt, re.M)
    assert "NaN-free" in txt  # the header says what the median assumes of its input
    lib = _lib.load()
    for name in ("svc_f0_voiced_median", "svc_pitch_shift_ex"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.svc_abi_version() == 3  # additions only


# host stand-ins: no argument below gets as far as a HIP call, so the context and the tensors are never dereferenced
_P = ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)


def _f64(*v):
    return (ctypes.c_double * len(v))(*v)


@pytest.mark.parametrize("target,scale,what", [
    ((220.0, 0.0), None, "target median"),
    ((220.0, -1.0), None, "target median"),
    ((float("nan"), 220.0), None, "target median"),
    ((220.0, float("inf")), None, "target median"),
    ((220.0, 220.0), (1.0, 0.0), "scale"),
    ((220.0, 220.0), (-2.0, 1.0), "scale"),
    ((220.0, 220.0), (1.0, float("nan")), "scale"),
])
def test_pitch_shift_ex_rejects_bad_tables(target, scale, what):
    lib = _lib.load()
    st = lib.svc_pitch_shift_ex(_P, _P, 2, 4, _f64(*target), None if scale is None else _f64(*scale), None)
    assert st == 1  # SVC_ERR_INVALID
    msg = lib.svc_last_error().decode()
    assert "pitch_shift_ex" in msg and what in msg
    with pytest.raises(_lib.SVCError, match="pitch_shift_ex"):
        _lib.call("svc_pitch_shift_ex", _P, _P, 2, 4, _f64(*target), None if scale is None else _f64(*scale), None)


def test_pitch_shift_ex_null_context_and_shape():
    lib = _lib.load()
    assert lib.svc_pitch_shift_ex(None, _P, 1, 4, _f64(220.0), None, None) == 1
    assert b"null context" in lib.svc_last_error()
    assert lib.svc_pitch_shift_ex(_P, _P, 0, 4, _f64(220.0), None, None) == 1
    assert lib.svc_pitch_shift_ex(_P, _P, 1, 0, _f64(220.0), None, None) == 1


@pytest.mark.parametrize("B,T,frames,what", [
    (2, 4, (4, 5), "5 frames"),
    (2, 4, (-1, 4), "-1 frames"),
    (65536, 32768, None, "2^31"),
    (1 << 16, 1 << 16, None, "2^31"),
    (0, 4, None, "bad args"),
    (1, 0, None, "bad args"),
])
def test_voiced_median_rejects_bad_arguments(B, T, frames, what):
    lib = _lib.load()
    fr = None if frames is None else (ctypes.c_int32 * len(frames))(*frames)
    st = lib.svc_f0_voiced_median(_P, _P, B, T, fr, _P, None, None)
    assert st == 1  # SVC_ERR_INVALID
    msg = lib.svc_last_error().decode()
    assert "f0_voiced_median" in msg and what in msg
    assert lib.svc_f0_voiced_median(None, _P, 1, 4, None, _P, None, None) == 1
    assert b"null context" in lib.svc_last_error()


def test_singer_table_round_trips_exactly(tmp_path):
    t = SingerF0Table()
    assert not t and len(t) == 0 and t.get(3, GLOBAL) == GLOBAL and t.get(3) is None
    awkward = [174.73750413040062, 0.1 + 0.2, math.nextafter(220.0, 1e9), 5e-324, 1.7976931348623157e308, 1 / 3]
    for i, m in enumerate(awkward):
        t.set(i * 7, m, voiced=10 + i, frames=20 + i, n_utts=1 + i)
    path = str(tmp_path / "f0.json")
    t.save(path)
    back = SingerF0Table.load(path)
    assert back == t and len(back) == len(awkward) and list(back) == [i * 7 for i in range(len(awkward))]
    for i, m in enumerate(awkward):
        assert back.get(i * 7) == m and back.get(i * 7).hex() == m.hex()
        assert back.entry(i * 7) == dict(median=m, voiced=10 + i, frames=20 + i, n_utts=1 + i)
    assert 7 in back and 8 not in back
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            t.set(1, bad)


# ------------------------------------------------------------------ the pipeline's choice of call
class _NoReadback:
    """A singer 'device tensor' that must not be read back to the host"""

    def __init__(self, ids):
        self._ids = ids

    def _no(self, *a, **k):
        raise AssertionError("the singer tensor was read back")

    tolist = cpu = numpy = item = __iter__ = __getitem__ = reshape = _no


class _FakeEngine:
    """CPU stand-in for SVCEngine that records how the pitch shift is called"""

    def __init__(self, table=None):
        from svc_inference_pipeline_amd import config as C
        self.cfg = C.load_config()
        self.cfg.mapper.content_feature = ["whisper"]
        self.shifts = []
        self.lock = threading.RLock()
        self.content_dtype = torch.float16
        self.singer_f0 = table if table is not None else SingerF0Table()
        self.target_f0_median = GLOBAL

    def mel_energy(self, w24, n_samples=None):
        B, N = w24.shape
        T = (N + 768 - 1024) // 256 + 1
        return torch.zeros(B, T, 100), torch.zeros(B, T)

    def f0(self, w24, T, n_samples=None):
        return torch.ones(w24.shape[0], T, dtype=torch.float64)

    def pitch_shift(self, f0, *args):
        self.shifts.append(args)
        return f0

    def whisper_encode(self, w16):
        return torch.zeros(w16.shape[0], 1500, 1024)

    def map_content(self, feats, T, rule="whisper", out=None):
        return feats[:, :1].expand(-1, T, -1).half()

    def condition(self, content, f0, energy, singer):
        return content[:, :, :384].float()

    def diffsvc_sample(self, cond, **kw):
        return cond[:, :, :100].clone()

    def bigvgan(self, x0, frames=None):
        return x0[:, :, :1].repeat_interleave(256, dim=1)[:, :, 0]


@pytest.fixture
def no_streams(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(wait_stream=lambda s: None))
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None, raising=False)


def _pipe(table=None):
    eng = _FakeEngine(table)
    return eng, SVCPipeline(eng, f0_side=False, whisper_ragged=False)


def _ragged(pipe, singers, **kw):
    lens = [2400, 4800, 3000][:len(singers)]
    return pipe.convert_many([torch.zeros(n) for n in lens], [torch.zeros(n * 2 // 3) for n in lens], singers, **kw)


def test_pipeline_picks_a_target_per_utterance(no_streams):
    table = SingerF0Table()
    table.set(3, 174.73750413040062)
    table.set(9, 301.5)
    eng, pipe = _pipe(table)
    _ragged(pipe, [3, 5, 9])
    assert eng.shifts == [([174.73750413040062, GLOBAL, 301.5], None)]  # 5 is not enrolled: the global median
    # the uniform batch reads its singer tensor for the same choice
    eng.shifts.clear()
    pipe.convert(torch.zeros(2, 2400), torch.zeros(2, 1600), torch.tensor([9, 3], dtype=torch.int32))
    assert eng.shifts == [([301.5, 174.73750413040062], None)]


def test_empty_table_and_zero_shift_is_the_scalar_call(no_streams):
    eng, pipe = _pipe()
    _ragged(pipe, [3, 5, 9])
    _ragged(pipe, [3, 5, 9], key_shift=0.0)
    _ragged(pipe, [3, 5], key_shift=[0, 0.0])
    pipe.convert(torch.zeros(2, 2400), torch.zeros(2, 1600), _NoReadback([9, 3]))  # not read back
    pipe.convert(torch.zeros(2, 2400), torch.zeros(2, 1600), _NoReadback([9, 3]), key_shift=[0.0, 0.0])
    assert eng.shifts == [()] * 5  # engine.pitch_shift(f0) and nothing else, as before


def test_key_shift_reaches_the_engine_as_a_power_of_two(no_streams):
    eng, pipe = _pipe()
    _ragged(pipe, [3, 5, 9], key_shift=[12, 0, -7.5])
    _ragged(pipe, [3, 5], key_shift=2)
    pipe.convert(torch.zeros(2, 2400), torch.zeros(2, 1600), torch.tensor([9, 3]), key_shift=torch.tensor([1.0, -12.0]))
    assert eng.shifts == [
        ([GLOBAL] * 3, [2.0, 1.0, 2.0 ** (-7.5 / 12.0)]),
        ([GLOBAL] * 2, [2.0 ** (2 / 12.0)] * 2),
        ([GLOBAL] * 2, [2.0 ** (1 / 12.0), 0.5]),
    ]
    with pytest.raises(ValueError, match="key shifts"):
        _ragged(pipe, [3, 5, 9], key_shift=[1, 2])


def test_enroll_argument_checks():
    _, pipe = _pipe()
    with pytest.raises(ValueError, match="either"):
        pipe.enroll(3)
    with pytest.raises(ValueError, match="either"):
        pipe.enroll(3, sources=["a.wav"], wavs24=[torch.zeros(10)])


# ------------------------------------------------------------------ the server
class _FakePipeline:
    def __init__(self):
        self.engine = types.SimpleNamespace(cfg=types.SimpleNamespace(n_fft=1024, hop_length=256), device=None)
        self.calls = []
        self.enrolled = []

    def convert_ragged(self, wavs24, wavs16, singers, wavs16_float=None, utt_ids=None, **kw):
        self.calls.append((list(utt_ids), kw))
        return [w + u for w, u in zip(wavs24, utt_ids)]

    def enroll(self, singer, sources=None, wavs24=None, max_batch=16):
        self.enrolled.append((singer, sources, wavs24, max_batch))
        return dict(median=200.0, voiced=1, frames=1, n_utts=1)


def test_server_carries_key_shift_per_request():
    p = _FakePipeline()
    with SVCServer(p, max_batch=3, max_wait_s=5.0, speedup=250) as srv:
        futs = [srv.submit(torch.zeros(2000), torch.zeros(1000), singer=1, key_shift=k) for k in (0.0, 12, -3.5)]
        for f in futs:
            f.result(timeout=10)
        futs = [srv.submit(torch.zeros(2000), torch.zeros(1000), singer=1) for _ in range(3)]
        for f in futs:
            f.result(timeout=10)
        assert srv.enroll(4, wavs24=["x"], max_batch=2) == dict(median=200.0, voiced=1, frames=1, n_utts=1)
    base = dict(fast_inference=True, speedup=250, seed=0)
    assert p.calls == [([0, 1, 2], dict(base, key_shift=[0.0, 12.0, -3.5])), ([3, 4, 5], base)]
    assert p.enrolled == [(4, None, ["x"], 2)]


def test_submit_file_takes_a_key_shift():
    p = _FakePipeline()
    srv = SVCServer(p, max_batch=1, max_wait_s=0.0)
    try:
        req = srv._file_request(b"not a wav", 1)
        assert req.key_shift == 0.0 and req.future.done()
        fut = srv.submit_file(b"not a wav", 1, key_shift=3.0)  # a bad file fails its own future, as before
        with pytest.raises(Exception):
            fut.result(timeout=1)
    finally:
        srv.close()


# ------------------------------------------------------------------ the CLI
def test_cli_parses_the_new_options():
    from svc_inference_pipeline_amd.infer import build_parser
    ap = build_parser()
    a = ap.parse_args(["--singer", "svcc_CDF1", "--singer-f0", "f0.json", "--enroll", "r1.wav", "r2.wav"])
    assert a.singer_f0 == "f0.json" and a.enroll == ["r1.wav", "r2.wav"] and a.wav is None and a.key == 0.0
    a = ap.parse_args(["--wav", "a.wav", "b.wav", "--key", "-2.5", "--singer-f0", "f0.json"])
    assert a.wav == ["a.wav", "b.wav"] and a.key == -2.5 and a.enroll is None
    a = ap.parse_args(["--wav", "a.wav"])
    assert a.singer_f0 is None and a.enroll is None and a.key == 0.0
