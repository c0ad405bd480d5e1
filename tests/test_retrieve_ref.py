"""CPU: feature retrieval's host side. The numpy reference (tests/retrieve_ref.py, what the GPU tests compare against)
against a plain loop on tiny shapes, the tie rule, k > N, rate 0 and 1; SingerIndexTable's file round trip and its
mismatch errors; `index_rate` through every Python layer on stand-in engines (validated before any device work, the
stage between the content stage and the conditioner, one call per enrolled singer, None leaves it out, SVCServer never
mixes values, the CLI flags); the two C-ABI symbols declared, bound and exported with the ABI version unchanged; and
every SVC_ERR_INVALID case of svc_content_retrieve / svc_index_norms returning before any HIP call."""
import contextlib
import ctypes
import os
import re
import threading
import types

import numpy as np
import pytest
import torch

import retrieve_ref as R
from svc_inference_pipeline_amd import _lib
from svc_inference_pipeline_amd import config as C
from svc_inference_pipeline_amd.pipeline import SVCPipeline
from svc_inference_pipeline_amd.serving import SVCServer
from svc_inference_pipeline_amd.singers import SingerIndexTable, check_index_rate, content_signature

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference
def _draw(seed, M, N, D):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D)).astype(np.float16)
    q = (0.7 * x[rng.integers(0, N, M)].astype(np.float32) + 0.5 * rng.standard_normal((M, D))).astype(np.float16)
    return q, x


@pytest.mark.parametrize("M,N,D,k,rate", [(3, 5, 8, 2, 0.5), (4, 9, 16, 8, 1.0), (2, 1, 8, 1, 0.25), (5, 12, 24, 4, 0.75)])
def test_reference_matches_a_plain_loop(M, N, D, k, rate):
    q, x = _draw(M * 100 + N, M, N, D)
    ref = R.retrieve(q, x, k, rate, 1e-4 * D)
    brute = R.brute_force(q, x, k, rate, 1e-4 * D)
    assert ref["idx"].shape == (M, min(k, N))
    for r, (idx, out, d2) in enumerate(brute):
        assert list(ref["idx"][r]) == idx
        assert np.allclose(ref["d2"][r], d2, rtol=1e-12, atol=0)
        assert np.allclose(ref["out"][r], out, rtol=1e-12, atol=1e-14)
    assert np.all(np.diff(ref["sorted"], axis=1) >= 0) and np.all(ref["tau"] > 0)


def test_norms_are_the_rounded_f64_sums():
    _, x = _draw(7, 1, 6, 40)
    want = [np.float32(sum(float(v) * float(v) for v in row)) for row in x]
    assert np.array_equal(R.index_norms(x), np.array(want, np.float32))


def test_tie_rule_on_duplicated_rows():
    """Rows 1, 4 and 6 are one vector and the query is that vector: their scores are equal bit for bit, the selection
    takes them in ascending j, and a rank boundary inside the tie (k = 2) keeps the lower two."""
    q, x = _draw(11, 1, 8, 16)
    x[4] = x[1]
    x[6] = x[1]
    q[0] = x[1]
    s = R.scores(q, x)
    assert s[0, 1] == s[0, 4] == s[0, 6] == s[0].min()
    assert list(R.topk(s, 3)[0]) == [1, 4, 6]
    assert list(R.topk(s, 2)[0]) == [1, 4]
    assert list(R.topk(s, 4)[0][:3]) == [1, 4, 6]


def test_k_larger_than_the_index():
    q, x = _draw(12, 3, 3, 8)
    ref = R.retrieve(q, x, 8, 1.0, 1e-3)
    assert ref["idx"].shape == (3, 3) and ref["d2"].shape == (3, 3)
    for r in range(3):
        assert sorted(ref["idx"][r]) == [0, 1, 2]
        assert np.all(np.diff(ref["s"][r][ref["idx"][r]]) >= 0)


def test_rate_zero_and_one():
    q, x = _draw(13, 4, 10, 16)
    r0 = R.retrieve(q, x, 4, 0.0, 1e-3)
    assert np.array_equal(r0["out"], q.astype(np.float64))  # the query itself
    r1 = R.retrieve(q, x, 1, 1.0, 1e-3)
    for r in range(4):  # k = 1: the weight is 1 and the blend is the nearest row
        assert np.allclose(r1["out"][r], x[r1["idx"][r, 0]].astype(np.float64), rtol=1e-15, atol=0)


def test_an_exact_match_sits_at_the_floor_and_takes_the_weight():
    q, x = _draw(14, 2, 20, 32)
    q[0] = x[7]
    ref = R.retrieve(q, x, 4, 1.0, 1e-2)
    assert ref["idx"][0, 0] == 7 and ref["d2"][0, 0] == float(np.float32(1e-2))
    assert np.max(np.abs(ref["out"][0] - x[7].astype(np.float64))) < 1e-2  # the floor's weight dominates


def test_f16_ulp():
    assert R.f16_ulp(1.0) == 2.0 ** -10 and R.f16_ulp(1.999) == 2.0 ** -10 and R.f16_ulp(2.0) == 2.0 ** -9
    assert R.f16_ulp(0.0) == 2.0 ** -24 and R.f16_ulp(-3.0) == 2.0 ** -9


# ------------------------------------------------------------------------------------------------ the table
def _table():
    rng = np.random.default_rng(3)
    t = SingerIndexTable()
    for sid, n in ((3, 5), (11, 2)):
        rows = torch.from_numpy(rng.standard_normal((n, 16)).astype(np.float16))
        norms = torch.from_numpy(R.index_norms(rows.numpy()))
        t.set(sid, rows, norms, n_utts=2, frames=n + 4, content_types=["whisper"])
    return t


def test_index_table_round_trip(tmp_path):
    t = _table()
    path = str(tmp_path / "idx.npz")
    t.save(path)
    assert os.path.exists(path)  # written at the path given, no suffix appended
    u = SingerIndexTable.load(path, "cpu", dim=16, content_types=["whisper"])
    assert list(u) == [3, 11] and len(u) == 2 and 3 in u and 4 not in u and u.get(4) is None
    for sid in t:
        a, b = t.get(sid), u.get(sid)
        assert torch.equal(a["rows"].view(torch.int16), b["rows"].view(torch.int16))
        assert torch.equal(a["norms"], b["norms"]) and b["rows"].dtype == torch.float16
        assert (a["n_utts"], a["frames"], a["content_types"]) == (b["n_utts"], b["frames"], b["content_types"])
    with np.load(path) as doc:
        assert doc["rows_3"].dtype == np.uint16 and doc["rows_3"].shape == (5, 16)


def test_index_table_mismatch_errors(tmp_path):
    path = str(tmp_path / "idx.npz")
    _table().save(path)
    with pytest.raises(ValueError, match="16 wide"):
        SingerIndexTable.load(path, "cpu", dim=1024, content_types=["whisper"])
    with pytest.raises(ValueError, match="content types"):
        SingerIndexTable.load(path, "cpu", dim=16, content_types=["contentvec", "whisper"])
    t = SingerIndexTable()
    with pytest.raises(ValueError, match="f16"):
        t.set(0, torch.zeros(3, 8), torch.zeros(3))
    with pytest.raises(ValueError, match="norms"):
        t.set(0, torch.zeros(3, 8, dtype=torch.float16), torch.zeros(2))
    assert not t
    cfg = C.load_config()
    D, types = content_signature(cfg)
    assert types == sorted(cfg.mapper.content_feature) and D == sum(int(cfg.mapper.input_content_dim[k]) for k in types)


def test_check_index_rate():
    assert check_index_rate(None) is None and check_index_rate(0) == 0.0 and check_index_rate(1) == 1.0
    assert check_index_rate(np.float32(0.5)) == 0.5
    for bad in (-0.01, 1.01, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="index_rate"):
            check_index_rate(bad)


# ------------------------------------------------------------------------------------------------ keyword plumbing
class _RecordingEngine:
    """CPU stand-in for SVCEngine: every stage returns zeros of the right shape and records its name."""
    ragged_hubert = ragged_whisper = False
    operands = "fp16"

    def __init__(self):
        self.cfg = C.load_config()
        self.cfg.mapper.content_feature = ["whisper"]
        self.calls = []
        self.lock = threading.RLock()
        self.content_dtype = torch.float16
        self.singer_f0 = None
        self.singer_index = SingerIndexTable()
        self.target_f0_median = 0.0

    def enroll_index(self, singer, n=4):
        rows = torch.full((n, 1024), float(singer), dtype=torch.float16)
        self.singer_index.set(singer, rows, torch.zeros(n), n_utts=1, frames=n, content_types=["whisper"])

    def mel_energy(self, w24, n_samples=None):
        B, N = w24.shape
        T = (N + 768 - 1024) // 256 + 1
        return torch.zeros(B, T, 100), torch.zeros(B, T)

    def f0(self, w24, T, n_samples=None):
        return torch.zeros(w24.shape[0], T, dtype=torch.float64)

    def pitch_shift(self, f0):
        return f0

    def whisper_encode(self, w16):
        self.calls.append(("content",))
        return torch.zeros(w16.shape[0], 1500, 1024)

    def map_content(self, feats, T, rule="whisper", out=None):
        return feats[:, :1].expand(-1, T, -1).half().contiguous()

    def content_retrieve(self, content, index, norms, frames=None, sel=None, k=8, rate=1.0, dist_floor=None, out=None,
                         return_neighbours=False):
        self.calls.append(("retrieve", tuple(content.shape), float(index[0, 0]), frames, sel, k, rate, out is content))
        return out

    def condition(self, content, f0, energy, singer):
        self.calls.append(("condition",))
        return content[:, :, :384].float()

    def diffsvc_sample(self, cond, **kw):
        return cond[:, :, :100].clone()

    def bigvgan(self, x0, frames=None):
        return torch.full((x0.shape[0], x0.shape[1] * 256), 0.5)


@pytest.fixture
def cpu_streams(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(wait_stream=lambda s: None))
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None)


def test_convert_ragged_runs_one_call_per_enrolled_singer(cpu_streams):
    eng = _RecordingEngine()
    eng.enroll_index(5)
    eng.enroll_index(2)
    pipe = SVCPipeline(eng, f0_side=False)
    lens = [2400, 4800, 1000, 3000]
    T_b = [(n + 768 - 1024) // 256 + 1 for n in lens]
    w24 = [torch.zeros(n) for n in lens]
    w16 = [torch.zeros(n * 2 // 3) for n in lens]
    outs = pipe.convert_ragged(w24, w16, [5, 9, 2, 5], index_rate=0.5)
    assert len(outs) == 4
    kinds = [c[0] for c in eng.calls]
    # after the content stage, before the conditioner: singers in ascending order, singer 9 has no index
    assert kinds.index("content") < kinds.index("retrieve") and kinds[-1] == "condition"
    calls = [c for c in eng.calls if c[0] == "retrieve"]
    shape = (4, max(T_b), 1024)
    assert calls == [("retrieve", shape, 2.0, T_b, [0, 0, 1, 0], 8, 0.5, True),
                     ("retrieve", shape, 5.0, T_b, [1, 0, 0, 1], 8, 0.5, True)]
    eng.calls.clear()
    pipe.convert_many(w24[:2], w16[:2], [5, 5], index_rate=1)  # one singer in the whole batch: no sel table
    calls = [c for c in eng.calls if c[0] == "retrieve"]
    assert len(calls) == 1 and calls[0][4] is None and calls[0][6] == 1.0


def test_convert_and_bucketed_route_run_the_stage(cpu_streams):
    eng = _RecordingEngine()
    eng.enroll_index(1)
    pipe = SVCPipeline(eng, f0_side=False)
    pipe.convert(torch.zeros(2, 2500), torch.zeros(2, 1600), torch.tensor([1, 0], dtype=torch.int32), index_rate=0.25)
    calls = [c for c in eng.calls if c[0] == "retrieve"]
    assert calls == [("retrieve", (2, 9, 1024), 1.0, None, [1, 0], 8, 0.25, True)]
    eng.calls.clear()
    w24 = [torch.zeros(2400), torch.zeros(4800), torch.zeros(2400)]
    w16 = [torch.zeros(1600), torch.zeros(3200), torch.zeros(1600)]
    pipe.convert_many(w24, w16, [1, 1, 1], bucketed=True, index_rate=0.5)
    assert [c[1][0] for c in eng.calls if c[0] == "retrieve"] == [2, 1]  # one call per length bucket


def test_none_or_no_enrolled_singer_launches_nothing(cpu_streams):
    eng = _RecordingEngine()
    pipe = SVCPipeline(eng, f0_side=False)
    w24, w16 = [torch.zeros(2400), torch.zeros(4800)], [torch.zeros(1600), torch.zeros(3200)]
    pipe.convert_ragged(w24, w16, [0, 1], index_rate=0.5)  # an empty table
    eng.enroll_index(7)
    pipe.convert_ragged(w24, w16, [0, 1], index_rate=0.5)  # no clip of singer 7
    for kw in ({}, dict(index_rate=None)):
        pipe.convert_ragged(w24, w16, [7, 7], **kw)
        pipe.convert(torch.zeros(1, 2500), torch.zeros(1, 1600), torch.tensor([7], dtype=torch.int32), **kw)
    assert "retrieve" not in [c[0] for c in eng.calls]


class _NoDeviceEngine:
    """An engine whose every stage fails the test: a bad index_rate must be rejected before any of them runs."""
    ragged_hubert = ragged_whisper = False

    def __init__(self, operands="fp16"):
        self.cfg = C.load_config()
        self.lock = threading.RLock()
        self.operands = operands

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached with a bad index_rate")


def _all_entry_points(pipe, value):
    w24, w16 = torch.zeros(1, 2400), torch.zeros(1, 1600)
    with pytest.raises(ValueError, match="index_rate"):
        pipe.convert(w24, w16, torch.zeros(1, dtype=torch.int32), index_rate=value)
    for bucketed in (False, True):
        with pytest.raises(ValueError, match="index_rate"):
            pipe.convert_many([w24[0]], [w16[0]], [0], bucketed=bucketed, index_rate=value)
    with pytest.raises(ValueError, match="index_rate"):
        pipe.convert_ragged([w24[0]], [w16[0]], [0], index_rate=value)
    with pytest.raises(ValueError, match="index_rate"):
        pipe.convert_files([b"not read"], [0], index_rate=value)


@pytest.mark.parametrize("bad", [-0.01, 1.01, float("nan"), "0.5"])
def test_pipeline_rejects_bad_value_before_device_work(bad):
    _all_entry_points(SVCPipeline(_NoDeviceEngine()), bad)


def test_bf16_operands_with_index_rate_is_an_error():
    pipe = SVCPipeline(_NoDeviceEngine(operands="bf16"))
    _all_entry_points(pipe, 0.5)
    with pytest.raises(ValueError, match="bf16"):
        pipe.enroll(0, wavs24=[torch.zeros(2400)], wavs16=[torch.zeros(1600)], index=True)


def test_enroll_argument_errors():
    pipe = SVCPipeline(_NoDeviceEngine())
    with pytest.raises(ValueError, match="wavs16"):
        pipe.enroll(0, wavs24=[torch.zeros(2400)], index=True)
    with pytest.raises(ValueError, match="index_max_rows"):
        pipe.enroll(0, wavs24=[torch.zeros(2400)], wavs16=[torch.zeros(1600)], index=True, index_max_rows=0)


class FakePipeline:
    """convert_ragged stand-in (as tests/test_serving.py's): records each batch's utterance ids and keywords."""

    def __init__(self):
        self.engine = types.SimpleNamespace(cfg=types.SimpleNamespace(n_fft=1024, hop_length=256), device=None)
        self.calls = []

    def convert_ragged(self, wavs24, wavs16, singers, wavs16_float=None, utt_ids=None, **kw):
        self.calls.append((list(utt_ids), kw))
        return [w * (s + 1) + u for w, s, u in zip(wavs24, singers, utt_ids)]


def test_server_never_mixes_index_rates():
    p = FakePipeline()
    rates = [None, 0.0, 0.0, None, 0.5, 0.0, 1]
    with SVCServer(p, max_batch=8, max_wait_s=60.0, speedup=250, seed=3) as srv:
        futs = [srv.submit(torch.full((2000,), 0.5), torch.ones(1000), singer=0, index_rate=m) for m in rates]
        for bad in (-1, 2.0, float("nan")):
            with pytest.raises(ValueError, match="index_rate"):
                srv.submit(torch.ones(2000), torch.ones(1000), singer=0, index_rate=bad)
        with pytest.raises(ValueError, match="index_rate"):
            srv.submit_file(b"RIFF", singer=0, index_rate=7)
    outs = [f.result(timeout=10) for f in futs]
    assert list(srv.batches) == [[0, 3], [1, 2, 5], [4], [6]]
    base = dict(fast_inference=True, speedup=250, seed=3)
    assert [kw for _, kw in p.calls] == [base, dict(base, index_rate=0.0), dict(base, index_rate=0.5),
                                         dict(base, index_rate=1.0)]
    for i, o in enumerate(outs):
        assert torch.equal(o, torch.full((2000,), 0.5) + i)


def test_cli_flags(capsys):
    from svc_inference_pipeline_amd import infer
    ap = infer.build_parser()
    a = ap.parse_args(["--wav", "a.wav"])
    assert a.index_rate is None and a.index is False and a.singer_index is None
    a = ap.parse_args(["--enroll", "r.wav", "--index", "--singer-index", "s.npz", "--index-rate", "0.75"])
    assert a.index is True and a.singer_index == "s.npz" and a.index_rate == 0.75
    for bad in ("1.5", "-0.1", "nan"):
        with pytest.raises(SystemExit) as exc:  # before any model is loaded
            infer.main(["--wav", "a.wav", "--index-rate", bad, "--random-weights", "tiny-test"])
        assert exc.value.code == 2 and "index_rate" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        infer.main(["--wav", "a.wav", "--index", "--random-weights", "tiny-test"])
    assert exc.value.code == 2 and "--enroll" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ the C-ABI
_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


def _header_argtypes(name):
    header = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    m = re.search(r"^svc_status\s+" + name + r"\s*\(([^)]*)\);", header, re.M | re.S)
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        out.append(ctypes.c_void_p if "*" in arg else _CTYPES[arg.rsplit(" ", 1)[0]])
    return out


def test_symbols_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("svc_index_norms", "svc_content_retrieve"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and args == _header_argtypes(name), name
    assert len(_lib.PROTOTYPES["svc_content_retrieve"][1]) == 20 and len(_lib.PROTOTYPES["svc_index_norms"][1]) == 7
    header = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    assert "svc_content_retrieve <-" in header  # the opening list of entry points
    assert lib.svc_abi_version() == _lib.ABI_VERSION == 3  # additions only
    assert _lib.get_config(None, "tune.retrieve_splits") == 0.0  # op-level context, no GPU call
    _lib.tune(None, retrieve_splits=5)
    assert _lib.get_config(None, "tune.retrieve_splits") == 5.0
    _lib.tune(None, reset=1)


_KEEP = ctypes.create_string_buffer(1 << 16)  # 64-byte aligned below: host stand-ins a failing call never reads
_P = (ctypes.addressof(_KEEP) + 63) & ~63


def _retrieve(ctx=True, content=0, index=8192, norms=16384, out=24576, B=2, T=3, frames=None, sel=None, D=16, ld=16,
              N=4, ld_index=16, k=4, rate=0.5, dist_floor=1e-3, ld_out=16):
    """svc_content_retrieve on host stand-ins (offsets into one buffer; None: a null pointer): no argument below gets
    as far as a HIP call."""
    ptr = lambda off: None if off is None else ctypes.c_void_p(_P + off)  # noqa: E731
    i32 = lambda v: None if v is None else (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    lib = _lib.load()
    st = lib.svc_content_retrieve(ptr(0) if ctx else None, ptr(content), B, T, i32(frames), i32(sel), D, ld, ptr(index),
                                  ptr(norms), N, ld_index, k, rate, dist_floor, ptr(out), ld_out, None, None, None)
    return st, lib.svc_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(ctx=False), "null context"),
    (dict(content=None), "null content16"),
    (dict(index=None), "null index16"),
    (dict(norms=None), "null norms"),
    (dict(out=None), "null out16"),
    (dict(B=0), "B=0"),
    (dict(T=0), "T=0"),
    (dict(k=0), "k=0"),
    (dict(k=9), "k=9"),
    (dict(D=12, ld=24, ld_index=24, ld_out=24), "D=12"),
    (dict(D=0), "D=0"),
    (dict(D=2056, ld=2056, ld_index=2056, ld_out=2056), "D=2056"),
    (dict(N=0), "N=0"),
    (dict(N=2 ** 31), "N=2147483648"),
    (dict(ld=8), "ld=8"),
    (dict(ld_index=8), "ld_index=8"),
    (dict(ld_out=8), "ld_out=8"),
    (dict(ld=20), "16-byte"),
    (dict(content=2), "16-byte"),
    (dict(rate=-0.01), "rate"),
    (dict(rate=1.01), "rate"),
    (dict(rate=float("nan")), "rate"),
    (dict(dist_floor=0.0), "dist_floor"),
    (dict(dist_floor=-1.0), "dist_floor"),
    (dict(dist_floor=float("nan")), "dist_floor"),
    (dict(dist_floor=1e-60), "dist_floor"),  # positive as f64, zero as the f32 the kernel clamps with
    (dict(frames=[3, 4]), "utterance 1: 4 frames"),
    (dict(frames=[-1, 3]), "utterance 0: -1 frames"),
    (dict(out=32), "overlaps content16"),      # content is 6 rows x 32 B: a partial overlap
    (dict(out=0, ld_out=32), "overlaps content16"),  # the same pointer with another row stride
    (dict(out=8192 + 64), "overlaps index16"),
    (dict(out=16384), "overlaps norms"),
])
def test_content_retrieve_rejects_bad_arguments_before_any_hip_call(kw, msg):
    st, err = _retrieve(**kw)
    assert st == 1, (st, err)
    assert err.startswith("content_retrieve:") and msg in err, err
    with pytest.raises(_lib.SVCError, match="content_retrieve"):
        _lib.check(st)


@pytest.mark.parametrize("kw,msg", [
    (dict(ctx=False), "null context"),
    (dict(index=None), "null index16"),
    (dict(norms=None), "null norms"),
    (dict(N=0), "N=0"),
    (dict(N=2 ** 31), "N=2147483648"),
    (dict(D=20), "D=20"),
    (dict(ld=8), "ld=8"),
    (dict(ld=20), "16-byte"),
    (dict(index=4), "16-byte"),
])
def test_index_norms_rejects_bad_arguments_before_any_hip_call(kw, msg):
    a = dict(ctx=True, index=0, norms=8192, N=4, D=16, ld=16)
    a.update(kw)
    ptr = lambda off: None if off is None else ctypes.c_void_p(_P + off)  # noqa: E731
    lib = _lib.load()
    st = lib.svc_index_norms(ptr(0) if a["ctx"] else None, ptr(a["index"]), a["N"], a["D"], a["ld"], ptr(a["norms"]),
                             None)
    err = lib.svc_last_error().decode()
    assert st == 1 and err.startswith("index_norms:") and msg in err, (st, err)
