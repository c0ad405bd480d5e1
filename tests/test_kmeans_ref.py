"""Host checks of index compaction: the numpy reference (tests/kmeans_ref.py) against a plain Python-int loop, the
properties the contract states (exact mean, iters = 0, empty clusters), the argument validation of enroll, the server and
the CLI with stub engines, the table's optional metadata, and the C-ABI's refusals before any HIP call."""
import ctypes
import os
import re
import threading
import types

import numpy as np
import pytest
import torch

import kmeans_ref as KR
import retrieve_ref as R
from svc_inference_pipeline_amd import _lib
from svc_inference_pipeline_amd import config as C
from svc_inference_pipeline_amd.pipeline import SVCPipeline
from svc_inference_pipeline_amd.runtime import mel_frames
from svc_inference_pipeline_amd.serving import SVCServer
from svc_inference_pipeline_amd.singers import SingerIndexTable, check_index_compact

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(seed, N, D, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal((N, D))).astype(np.float16)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("N,D,K,iters", [(12, 8, 4, 0), (12, 8, 4, 2), (30, 16, 7, 3), (9, 8, 9, 1)])
def test_reference_matches_a_plain_loop(N, D, K, iters):
    x = _rows([3, N, D], N, D)
    ref = KR.kmeans(x, K, iters)
    bits, labels = KR.brute_force(x, K, iters)
    assert np.array_equal(np.array(bits, np.uint16), ref["centroids"].view(np.uint16))
    assert labels == ref["labels"].tolist()
    assert ref["inertia"].shape == (iters + 1,) and ref["counts"].sum() == N
    assert np.array_equal(ref["norms"], R.index_norms(ref["centroids"]))


def test_to_int_is_exact_over_all_finite_halves():
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    h = h[np.isfinite(h)]
    i = KR.to_int(h)
    assert np.abs(i).max() < 2 ** 40 and np.array_equal(i.astype(np.float64) * 2.0 ** -24, h.astype(np.float64))


def test_exact_mean_does_not_depend_on_the_order_of_the_members():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((200, 16)) * 10.0 ** rng.uniform(-6, 4, (200, 1))).astype(np.float16)  # 10 decades
    members = np.arange(0, 200, 3)
    want = KR.exact_mean(x, members).view(np.uint16)
    for _ in range(5):
        assert np.array_equal(KR.exact_mean(x, rng.permutation(members)).view(np.uint16), want)
    # and it is the correctly rounded mean: Python's exact rationals agree
    from fractions import Fraction
    col = [Fraction(float(v)) for v in x[members, 0]]
    exact = sum(col) / len(col)
    assert np.float16(np.float32(np.float64(float(exact)))).view(np.uint16) == want[0]


def test_iters_zero_is_the_index_max_rows_selection():
    x = _rows(7, 57, 8)
    for K in (1, 10, 56, 57):
        keep = [i * 57 // K for i in range(K)]  # SVCPipeline.enroll's rule
        assert KR.init_rows(57, K) == keep
        ref = KR.kmeans(x, K, 0)
        assert np.array_equal(ref["centroids"].view(np.uint16), x[keep].view(np.uint16))
        assert np.array_equal(ref["norms"], R.index_norms(x[keep]))


def test_an_empty_cluster_keeps_its_row_and_bad_labels_join_none():
    x = _rows(8, 20, 8)
    prev = _rows(9, 4, 8)
    labels = np.array([0, 2] * 10)
    labels[3] = -1
    labels[4] = 4
    out, norms, counts = KR.update(x, labels, prev)
    assert counts.tolist() == [9, 0, 9, 0]
    assert np.array_equal(out[[1, 3]].view(np.uint16), prev[[1, 3]].view(np.uint16))
    assert np.array_equal(out[0].view(np.uint16), KR.exact_mean(x, np.flatnonzero(labels == 0)).view(np.uint16))
    assert np.array_equal(norms, R.index_norms(out))


def test_ties_go_to_the_lower_centroid_and_near_ties_are_flagged():
    x = _rows(10, 6, 8)
    a = KR.assign(np.repeat(x, 2, axis=0), np.repeat(x, 2, axis=0))
    assert a["labels"].tolist() == [0, 0, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10]
    assert KR.near_ties(a).all() and a["counts"].tolist() == [2, 0] * 6
    b = KR.assign(x, x[:1])
    assert np.isinf(b["gap"]).all() and not KR.near_ties(b).any()


def test_lloyd_never_raises_the_reference_inertia():
    ref = KR.kmeans(_rows(1, 300, 72), 130, 6)
    assert np.all(np.diff(ref["inertia"]) <= 1e-6 * ref["inertia"][0]) and ref["inertia"][-1] < 0.7 * ref["inertia"][0]


# ------------------------------------------------------------------------------------------------ host layers
def test_check_index_compact():
    assert check_index_compact("stride") == ("stride", 10)
    assert check_index_compact("kmeans", 0) == ("kmeans", 0)
    assert check_index_compact("kmeans", np.int64(1000)) == ("kmeans", 1000)
    for mode in ("lloyd", None, 1, "KMEANS"):
        with pytest.raises(ValueError, match="index_compact"):
            check_index_compact(mode)
    for iters in (-1, 1001, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="index_iters"):
            check_index_compact("stride", iters)


class _NoDeviceEngine:
    """An engine whose every stage fails the test: bad arguments must be rejected before any of them runs."""
    ragged_hubert = ragged_whisper = False

    def __init__(self):
        self.cfg = C.load_config()
        self.lock = threading.RLock()
        self.operands = "fp16"

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached with bad arguments")


def test_enroll_rejects_bad_mode_or_iters_before_device_work():
    pipe = SVCPipeline(_NoDeviceEngine())
    kw = dict(wavs24=[torch.zeros(2400)], wavs16=[torch.zeros(1600)], index=True, index_max_rows=4)
    with pytest.raises(ValueError, match="index_compact"):
        pipe.enroll(0, index_compact="means", **kw)
    for bad in (-1, 1001, 1.5):
        with pytest.raises(ValueError, match="index_iters"):
            pipe.enroll(0, index_compact="kmeans", index_iters=bad, **kw)
    with pytest.raises(ValueError, match="index_iters"):  # checked in the default mode too
        pipe.enroll(0, index_iters=-3, **kw)


class _KmeansEngine:
    """Records enroll's calls; index_kmeans returns K = 4 centroids of which centroid 2 ended without a row."""
    operands = "fp16"
    ragged_hubert = ragged_whisper = False

    def __init__(self):
        self.cfg = C.load_config()
        self.lock = threading.RLock()
        self.singer_f0 = types.SimpleNamespace(set=lambda *a, **k: dict(median=200.0))
        self.singer_index = SingerIndexTable()
        self.calls = []

    def f0_voiced_median(self, flat):
        return torch.tensor(200.0), torch.tensor(3)

    def index_norms(self, x):
        self.calls.append(("index_norms", tuple(x.shape)))
        return (x.float() ** 2).sum(1)

    def index_kmeans(self, x, K, iters):
        self.calls.append(("index_kmeans", tuple(x.shape), K, iters))
        cent = x[:K].clone() + 1
        return cent, (cent.float() ** 2).sum(1), torch.tensor([3, 1, 0, 2][:K]), torch.tensor([9.0, 5.0, 4.0])


def _stub_pipe(frames=7):
    e = _KmeansEngine()
    pipe = SVCPipeline(e)
    content = torch.arange(frames * 8, dtype=torch.float16).reshape(1, frames, 8)
    pipe.extract_f0 = lambda w24, T, **kw: torch.full((1, T), 200.0, dtype=torch.float64)
    pipe.ragged_content = lambda w16, T_b, T, w16f=None: content[:, :T]
    return pipe, e, content[0]


def test_enroll_modes_with_a_stub_engine():
    wav = [torch.zeros(256 * 7)]
    kw = dict(wavs24=wav, wavs16=[torch.zeros(1600)], index=True)
    pipe, e, rows = _stub_pipe()
    assert mel_frames(256 * 7, e.cfg.n_fft, e.cfg.hop_length) == 7 == rows.shape[0]
    # the default and "stride": rows floor(i N / M), no k-means call, no metadata
    for extra in ({}, dict(index_compact="stride", index_iters=5)):
        e.calls.clear()
        pipe.enroll(3, index_max_rows=4, **kw, **extra)
        ent = e.singer_index.get(3)
        assert torch.equal(ent["rows"], rows[[0, 1, 3, 5]]) and "compact" not in ent and ent["frames"] == 7
        assert [c[0] for c in e.calls] == ["index_norms"]
    # "kmeans" with N > M: K = M, the empty centroid is dropped, the norms are index_kmeans' own
    e.calls.clear()
    pipe.enroll(3, index_max_rows=4, index_compact="kmeans", index_iters=2, **kw)
    ent = e.singer_index.get(3)
    assert e.calls == [("index_kmeans", (7, 8), 4, 2)]
    assert torch.equal(ent["rows"], (rows[:4] + 1)[[0, 1, 3]]) and ent["norms"].shape == (3,)
    assert ent["compact"] == dict(method="kmeans", iters=2, inertia_first=9.0, inertia_last=4.0, dropped=1)
    assert ent["frames"] == 7
    # N <= M: every row is kept in both modes
    for mode in ("stride", "kmeans"):
        e.calls.clear()
        pipe.enroll(3, index_max_rows=7, index_compact=mode, **kw)
        ent = e.singer_index.get(3)
        assert torch.equal(ent["rows"], rows) and "compact" not in ent and [c[0] for c in e.calls] == ["index_norms"]


def test_server_enroll_passes_the_arguments_through():
    seen = []
    p = types.SimpleNamespace(engine=types.SimpleNamespace(cfg=types.SimpleNamespace(n_fft=1024, hop_length=256),
                                                           device=None),
                              enroll=lambda singer, **kw: seen.append((singer, kw)) or "entry")
    with SVCServer(p, max_batch=2, max_wait_s=0.01) as srv:
        assert srv.enroll(4, wavs24=["w"]) == "entry"
        assert srv.enroll(5, sources=["a.wav"], index=True, index_max_rows=9, index_compact="kmeans",
                          index_iters=3) == "entry"
        with pytest.raises(TypeError, match="index_rows"):
            srv.enroll(5, sources=["a.wav"], index_rows=3)
    assert seen == [(4, dict(sources=None, wavs24=["w"], max_batch=16)),
                    (5, dict(sources=["a.wav"], wavs24=None, max_batch=16, index=True, index_max_rows=9,
                             index_compact="kmeans", index_iters=3))]


def test_cli_flags(capsys, monkeypatch):
    from svc_inference_pipeline_amd import infer
    ap = infer.build_parser()
    a = ap.parse_args(["--enroll", "r.wav", "--index"])
    assert a.index_max_rows is None and a.index_compact is None and a.index_iters is None
    a = ap.parse_args(["--enroll", "r.wav", "--index", "--index-max-rows", "8192", "--index-compact", "kmeans",
                       "--index-iters", "20"])
    assert (a.index_max_rows, a.index_compact, a.index_iters) == (8192, "kmeans", 20)
    with pytest.raises(SystemExit):
        ap.parse_args(["--enroll", "r.wav", "--index", "--index-compact", "lloyd"])
    capsys.readouterr()
    rw = ["--random-weights", "tiny-test"]
    for flag, val in (("--index-max-rows", "10"), ("--index-compact", "kmeans"), ("--index-iters", "3")):
        for argv in (["--wav", "a.wav", flag, val], ["--wav", "a.wav", "--enroll", "r.wav", flag, val]):
            with pytest.raises(SystemExit) as exc:  # before any model is loaded
                infer.main(argv + rw)
            assert exc.value.code == 2 and f"{flag} needs --enroll --index" in capsys.readouterr().err
    for argv, msg in ((["--index-max-rows", "0"], "--index-max-rows"), (["--index-iters", "1001"], "index_iters"),
                      (["--index-iters", "-1"], "index_iters")):
        with pytest.raises(SystemExit) as exc:
            infer.main(["--enroll", "r.wav", "--index"] + argv + rw)
        assert exc.value.code == 2 and msg in capsys.readouterr().err
    # enroll_singer hands the three on, and only where given
    seen = []

    class P:
        def __init__(self, engine, f0_method=None):
            pass

        def enroll(self, singer, **kw):
            seen.append(kw)
            return {}

    monkeypatch.setattr(infer, "SVCPipeline", P)
    cfg = C.load_config()
    name = sorted(C.load_singers(cfg))[0]
    infer.enroll_singer(None, cfg, name, ["r.wav"], index=True)
    infer.enroll_singer(None, cfg, name, ["r.wav"], index=True, index_max_rows=5, index_compact="kmeans", index_iters=2)
    assert seen == [dict(sources=["r.wav"], index=True),
                    dict(sources=["r.wav"], index=True, index_max_rows=5, index_compact="kmeans", index_iters=2)]


def test_index_table_round_trip_with_and_without_the_metadata(tmp_path):
    t = SingerIndexTable()
    rows = torch.from_numpy(_rows(2, 5, 8))
    norms = torch.from_numpy(R.index_norms(rows.numpy()))
    t.set(1, rows, norms, n_utts=2, frames=40, content_types=["whisper"])
    meta = dict(method="kmeans", iters=10, inertia_first=1234.5678901234567, inertia_last=0.1 + 0.2, dropped=3)
    t.set(2, rows[:3], norms[:3], n_utts=1, frames=90, content_types=["whisper"], compact=meta)
    assert "compact" not in t.get(1) and t.get(2)["compact"] == meta
    path = str(tmp_path / "index.npz")
    t.save(path)
    back = SingerIndexTable.load(path)
    assert "compact" not in back.get(1) and back.get(2)["compact"] == meta  # the inertias bit for bit
    for k in (1, 2):
        assert torch.equal(back.get(k)["rows"], t.get(k)["rows"]) and torch.equal(back.get(k)["norms"], t.get(k)["norms"])
        assert back.get(k)["frames"] == t.get(k)["frames"]
    # a table without k-means entries is written as before: no "compact" key anywhere in its metadata
    plain = SingerIndexTable()
    plain.set(1, rows, norms, n_utts=2, frames=40, content_types=["whisper"])
    ppath = str(tmp_path / "plain.npz")
    plain.save(ppath)
    with np.load(ppath) as doc:
        assert "compact" not in str(doc["meta"]) and sorted(doc.files) == ["meta", "norms_1", "rows_1"]
    assert "compact" not in SingerIndexTable.load(ppath).get(1)


# ------------------------------------------------------------------------------------------------ the C-ABI
_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
NAMES = ("svc_index_assign", "svc_index_update", "svc_index_kmeans")


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
    for name in NAMES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and args == _header_argtypes(name), name
    assert lib.svc_abi_version() == _lib.ABI_VERSION == 3  # additions only


_KEEP = ctypes.create_string_buffer(1 << 16)  # host stand-ins a failing call never reads
_P = (ctypes.addressof(_KEEP) + 63) & ~63


def _ptr(off):
    return None if off is None else ctypes.c_void_p(_P + off)


def _call(fn, **kw):
    """One of the three entry points on host stand-ins (offsets into one buffer; None: a null pointer)."""
    a = dict(ctx=True, rows=4096, N=64, D=16, ld=16, K=8, cent=8192, ldc=16, norms=12288, labels=16384, prev=20480,
             ldp=16, out=8192, ldo=16, iters=2)
    a.update(kw)
    lib = _lib.load()
    ctx = _ptr(0) if a["ctx"] else None
    if fn == "assign":
        st = lib.svc_index_assign(ctx, _ptr(a["rows"]), a["N"], a["D"], a["ld"], _ptr(a["cent"]), _ptr(a["norms"]),
                                  a["K"], a["ldc"], _ptr(a["labels"]), None, None, None)
    elif fn == "update":
        st = lib.svc_index_update(ctx, _ptr(a["rows"]), a["N"], a["D"], a["ld"], _ptr(a["labels"]), a["K"],
                                  _ptr(a["prev"]), a["ldp"], _ptr(a["out"]), a["ldo"], _ptr(a["norms"]), None, None)
    else:
        st = lib.svc_index_kmeans(ctx, _ptr(a["rows"]), a["N"], a["D"], a["ld"], a["K"], a["iters"], _ptr(a["cent"]),
                                  a["ldc"], _ptr(a["norms"]), None, None, None, None)
    return st, lib.svc_last_error().decode()


@pytest.mark.parametrize("fn,kw,msg", [
    ("assign", dict(ctx=False), "null context"),
    ("assign", dict(rows=None), "null rows16"),
    ("assign", dict(cent=None), "null cent16"),
    ("assign", dict(norms=None), "null cent_norms"),
    ("assign", dict(labels=None), "null labels"),
    ("assign", dict(N=0), "N=0"),
    ("assign", dict(N=2 ** 22 + 1), "N=4194305"),
    ("assign", dict(D=12, ld=24, ldc=24), "D=12"),
    ("assign", dict(D=0), "D=0"),
    ("assign", dict(D=2056, ld=2056, ldc=2056), "D=2056"),
    ("assign", dict(K=0), "K=0"),
    ("assign", dict(K=65), "K=65"),
    ("assign", dict(N=2 ** 22, K=2 ** 20 + 1), "K=1048577"),
    ("assign", dict(ld=8), "rows16 ld=8"),
    ("assign", dict(ldc=8), "cent16 ld=8"),
    ("assign", dict(ld=20), "16-byte"),
    ("assign", dict(rows=4098), "16-byte"),
    ("assign", dict(cent=8200), "16-byte"),
    ("update", dict(ctx=False), "null context"),
    ("update", dict(labels=None), "null labels"),
    ("update", dict(prev=None), "null prev16"),
    ("update", dict(out=None), "null out16"),
    ("update", dict(norms=None), "null norms_out"),
    ("update", dict(N=0), "N=0"),
    ("update", dict(K=65), "K=65"),
    ("update", dict(D=20), "D=20"),
    ("update", dict(ldp=8), "prev16 ld=8"),
    ("update", dict(ldo=8), "out16 ld=8"),
    ("update", dict(ldo=20), "16-byte"),
    ("update", dict(out=20480 + 32), "overlaps prev16"),            # prev is 8 rows x 32 B: a partial overlap
    ("update", dict(out=20480, ldo=32), "overlaps prev16"),         # the same pointer with another row stride
    ("update", dict(out=4096 + 64), "overlaps rows16"),
    ("kmeans", dict(ctx=False), "null context"),
    ("kmeans", dict(rows=None), "null rows16"),
    ("kmeans", dict(cent=None), "null cent16"),
    ("kmeans", dict(norms=None), "null cent_norms"),
    ("kmeans", dict(iters=-1), "iters=-1"),
    ("kmeans", dict(iters=1001), "iters=1001"),
    ("kmeans", dict(K=0), "K=0"),
    ("kmeans", dict(K=65), "K=65"),
    ("kmeans", dict(N=2 ** 23), "N=8388608"),
    ("kmeans", dict(D=24), "D=24"),
    ("kmeans", dict(ldc=20), "16-byte"),
    ("kmeans", dict(cent=4096 + 32), "overlaps rows16"),
])
def test_entry_points_reject_bad_arguments_before_any_hip_call(fn, kw, msg):
    st, err = _call(fn, **kw)
    assert st == 1, (st, err)
    assert err.startswith(f"index_{fn}:") and msg in err, err
