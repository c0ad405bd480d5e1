"""GPU: index compaction (svc_index_assign, svc_index_update, svc_index_kmeans) against tests/kmeans_ref.py.

Inputs are drawn on the CPU from fixed seeds. The assignment's shapes straddle knn_topk's 128-query and 128-index tiles
and its 64-half K stage: (N, D, K) = (300, 72, 130) and (520, 136, 257), and (1, 8, 1). The assignment is judged with
tau, the derived worst-case error of one device f32 score (retrieve_ref.tau); the update has no tolerance: given the
device's own labels its centroids and norms are the reference's bit for bit, since the mean is an exact integer sum
rounded once.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kmeans_ref as KR  # noqa: E402
import retrieve_ref as R  # noqa: E402
from gpu_util import dev  # noqa: E402
from oracle import noise as ON  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine, mel_frames  # noqa: E402

SENT = 0x5A5A  # the f16 bit pattern of every pad column


@pytest.fixture(scope="module")
def eng():
    e = SVCEngine(C.load_config(), 0)
    yield e
    e.close()


def rows_of(N, D, seed, scale=1.0):
    """f16 [N, D] standard normals times scale"""
    return (scale * np.random.default_rng(seed).standard_normal((N, D))).astype(np.float16)


@functools.lru_cache(maxsize=None)
def _assign_case(N, D, K, seed, scale):
    """(x, centroids = rows floor(i N / K), their norms, the reference assignment); shared, never modified"""
    x = rows_of(N, D, seed, scale)
    c = x[KR.init_rows(N, K)].copy()
    norms = R.index_norms(c)
    ref = KR.assign(x, c, norms)
    for a in (x, c, norms):
        a.setflags(write=False)
    return x, c, norms, ref


@functools.lru_cache(maxsize=None)
def _kmeans_case(N, D, K, seed, iters):
    x = rows_of(N, D, seed)
    x.setflags(write=False)
    return x, KR.kmeans(x, K, iters)


def _padded(a, ld):
    """f16 [R, D] -> device f16 [R, ld], the columns past D holding the sentinel"""
    a = np.ascontiguousarray(a, np.float16)
    buf = np.full((a.shape[0], ld), SENT, np.uint16)
    buf[:, :a.shape[1]] = a.view(np.uint16)
    return torch.from_numpy(buf.view(np.int16)).view(torch.float16).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _np_bits(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


def _assign(eng, x, c, pad=(8, 16)):
    """index_assign on padded buffers -> (labels, counts, inertia float, inertia bits)"""
    D = x.shape[1]
    xb, cb = _padded(x, D + pad[0]), _padded(c, D + pad[1])
    nd = eng.index_norms(cb[:, :D])
    labels, counts, inertia = eng.index_assign(xb[:, :D], cb[:, :D], nd, return_counts=True, return_inertia=True)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(xb), _bits(_padded(x, D + pad[0]))) and np.array_equal(_bits(cb), _bits(_padded(c, D + pad[1])))
    ine = inertia.cpu().numpy()
    return labels.cpu().numpy(), counts.cpu().numpy(), float(ine[0]), ine.view(np.uint64)[0]


# ------------------------------------------------------------------------------------------------------------- assign
@pytest.mark.parametrize("N,D,K,seed,scale", [(300, 72, 130, 1, 1.0), (520, 136, 257, 2, 0.5), (1, 8, 1, 4, 1.0)],
                         ids=lambda v: str(v))
def test_assign_against_the_reference(eng, N, D, K, seed, scale):
    """Measured on MI355X: no label differs from the reference's in any of the three cases; the inertia error is
    at most 0.0002 of its bound."""
    x, c, norms, ref = _assign_case(N, D, K, seed, scale)
    near = KR.near_ties(ref)
    gap_tau = float((ref["gap"] / ref["tau"]).min())
    print("N=%d D=%d K=%d: %d near-tie rows, least gap %.1f tau" % (N, D, K, int(near.sum()), gap_tau))
    assert near.sum() <= 0.01 * N  # a condition on the inputs, from the reference alone
    labels, counts, inertia, ibits = _assign(eng, x, c)
    assert labels.dtype == np.int32 and np.all((labels >= 0) & (labels < K))
    rows = np.arange(N)
    assert np.all(ref["s"][rows, labels] <= ref["best"] + 2.0 * ref["tau"])
    differ = labels != ref["labels"]
    print("labels that differ from the reference's: %d" % int(differ.sum()))
    assert not np.any(differ & ~near) and differ.sum() <= 0.01 * N
    assert np.array_equal(counts, np.bincount(labels, minlength=K))
    # inertia: each term is an f32 sum of |x|^2 (D additions) plus one f32 addition and the score's own error
    s_dev = ref["s"][rows, labels]
    want = float(np.maximum(ref["x2"] + s_dev, 0.0).sum())
    bound = float((ref["tau"] + 2.0 ** -22 * (ref["x2"] + np.abs(s_dev))).sum())
    print("inertia %.6f, reference %.6f, |error| / bound %.4f" % (inertia, want, abs(inertia - want) / bound))
    assert abs(inertia - want) <= bound
    # bit-identical from run to run, and for every number of index splits
    again = _assign(eng, x, c)
    assert np.array_equal(again[0], labels) and np.array_equal(again[1], counts) and again[3] == ibits
    try:
        for splits in (1, 3):
            eng.tune(retrieve_splits=splits)
            got = _assign(eng, x, c)
            assert np.array_equal(got[0], labels) and np.array_equal(got[1], counts) and got[3] == ibits, splits
    finally:
        eng.tune(reset=1)


def test_assign_exact_ties_go_to_the_lower_centroid(eng):
    """Every row twice, K = N: a row's two copies score alike bit for bit, so both take the lower j of the pair, and
    exactly half the counts are 0. 260 rows: the pairs (126, 127) and (128, 129) sit on either side of a tile edge."""
    base = rows_of(130, 72, 5)
    x = np.repeat(base, 2, axis=0)
    labels, counts, _, _ = _assign(eng, x, x)
    assert np.array_equal(labels, 2 * (np.arange(260) // 2))
    assert np.array_equal(counts, np.tile([2, 0], 130))


# ------------------------------------------------------------------------------------------------------------- update
def _update(eng, x, labels, prev, pad=(8, 16, 24), inplace=False):
    """index_update on padded buffers -> (centroid bits [K, ld_out], norms, counts)"""
    D = x.shape[1]
    xb, pb = _padded(x, D + pad[0]), _padded(prev, D + pad[1])
    ob = pb if inplace else _padded(np.zeros_like(prev), D + pad[2])
    if not inplace:
        ob.view(torch.int16).fill_(SENT)
    lab = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).cuda()
    out, norms, counts = eng.index_update(xb[:, :D], lab, pb[:, :D], out=ob[:, :D], return_counts=True)
    torch.cuda.synchronize()
    assert out.data_ptr() == ob.data_ptr() and np.array_equal(_bits(xb), _bits(_padded(x, D + pad[0])))
    if not inplace:
        assert np.array_equal(_bits(pb), _bits(_padded(prev, D + pad[1])))
    return _bits(ob), norms.cpu().numpy(), counts.cpu().numpy()


def _check_update(eng, x, labels, prev, **kw):
    want, wnorms, wcounts = KR.update(x, labels, prev)
    bits, norms, counts = _update(eng, x, labels, prev, **kw)
    D = x.shape[1]
    assert np.array_equal(counts, wcounts)
    assert np.array_equal(bits[:, :D], _np_bits(want))
    assert np.all(bits[:, D:] == SENT)
    assert np.array_equal(norms.view(np.uint32), wnorms.view(np.uint32))
    return wcounts


def _blobs(N, D, n_blobs, seed):
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((n_blobs, D))
    return (centres[rng.integers(0, n_blobs, N)] + 0.3 * rng.standard_normal((N, D))).astype(np.float16)


@pytest.mark.parametrize("N,D,K", [(1500, 72, 40), (600, 8, 33), (600, 2048, 33)], ids=lambda v: str(v))
def test_update_is_the_exact_mean_of_the_device_labels(eng, N, D, K):
    """24 Gaussian blobs; the previous centroids are rows floor(i N / K), except centroid 7, which is far from every row
    and so ends empty: it keeps its previous row. The labels are the device's own."""
    x = _blobs(N, D, 24, [7, N, D])
    prev = x[KR.init_rows(N, K)].copy()
    prev[7] = 40.0
    labels, counts, _, _ = _assign(eng, x, prev)
    assert counts[7] == 0 and counts.sum() == N
    got = _check_update(eng, x, labels, prev)
    assert np.array_equal(got, counts)
    _check_update(eng, x, labels, prev, inplace=True)


def test_update_one_cluster_of_4096_large_rows(eng):
    """All 4096 rows, of magnitude 60000, in cluster 1 of 3: column sums near 2^52 in units of 2^-24, four workgroups
    and the integer combine; clusters 0 and 2 are empty. Then 5000 rows over 3 clusters of more than 1024 rows each."""
    rng = np.random.default_rng(11)
    x = rng.uniform(55000.0, 65000.0, (4096, 72)).astype(np.float16)
    x[::7] = -x[::7] * np.float16(0.25)
    prev = rows_of(3, 72, 12)
    got = _check_update(eng, x, np.ones(4096, np.int32), prev)
    assert list(got) == [0, 4096, 0]
    x = rows_of(5000, 8, 13)
    labels = rng.integers(0, 3, 5000).astype(np.int32)
    got = _check_update(eng, x, labels, rows_of(3, 8, 14))
    assert got.min() > 1024


# ------------------------------------------------------------------------------------------------------------- k-means
def _dev_rows(x):
    return torch.from_numpy(np.array(x, np.float16).view(np.int16)).view(torch.float16).cuda()


@pytest.mark.parametrize("iters", [0, 1, 3])
def test_kmeans_is_assign_and_update_composed(eng, iters):
    N, D, K = 300, 72, 130
    x = rows_of(N, D, 1)
    xd = _dev_rows(x)
    cent, norms, counts, inertia, labels = eng.index_kmeans(xd, K, iters, return_labels=True)
    c = xd[torch.tensor(KR.init_rows(N, K), device="cuda")].contiguous()
    if iters == 0:
        assert torch.equal(cent, c)
    n = eng.index_norms(c)
    ine = []
    for _ in range(iters):
        lab, i1 = eng.index_assign(xd, c, n, return_inertia=True)
        ine.append(i1)
        c, n = eng.index_update(xd, lab, c)
    lab, cnt, i1 = eng.index_assign(xd, c, n, return_counts=True, return_inertia=True)
    ine.append(i1)
    assert torch.equal(cent, c) and torch.equal(norms.view(torch.int32), n.view(torch.int32))
    assert torch.equal(labels, lab) and torch.equal(counts, cnt)
    assert torch.equal(inertia.view(torch.int64), torch.cat(ine).view(torch.int64))
    assert torch.equal(norms, eng.index_norms(cent))


@pytest.mark.parametrize("N,D,K,seed,iters", [(300, 72, 130, 1, 3), (1000, 8, 16, 3, 4)], ids=lambda v: str(v))
def test_kmeans_equals_the_reference(eng, N, D, K, seed, iters):
    """No step of the reference has a near-tie row on these inputs (asserted), so the device's labels, and with them
    its centroids, are the reference's outright."""
    x, ref = _kmeans_case(N, D, K, seed, iters)
    for i, step in enumerate(ref["steps"]):
        assert not KR.near_ties(step).any(), i
    print("reference inertia %.1f -> %.1f" % (ref["inertia"][0], ref["inertia"][-1]))
    cent, norms, counts, inertia, labels = eng.index_kmeans(_dev_rows(x), K, iters, return_labels=True)
    assert np.array_equal(_bits(cent), _np_bits(ref["centroids"]))
    assert np.array_equal(labels.cpu().numpy(), ref["labels"]) and np.array_equal(counts.cpu().numpy(), ref["counts"])
    assert np.array_equal(norms.cpu().numpy().view(np.uint32), ref["norms"].view(np.uint32))
    ine = inertia.cpu().numpy()
    assert ine.shape == (iters + 1,) and ine[-1] <= ine[0] and ref["inertia"][-1] <= ref["inertia"][0]
    for i, step in enumerate(ref["steps"]):
        bound = float((step["tau"] + 2.0 ** -22 * (step["x2"] + np.abs(step["best"]))).sum())
        assert abs(ine[i] - step["inertia"]) <= bound, i


def test_kmeans_past_convergence_changes_nothing(eng):
    x = rows_of(300, 72, 1)
    xd = _dev_rows(x)
    a = eng.index_kmeans(xd, 130, 40, return_labels=True)
    b = eng.index_kmeans(xd, 130, 45, return_labels=True)
    ia, ib = a[3].cpu().numpy(), b[3].cpu().numpy()
    assert ia[-1] == ia[-2], "40 iterations did not reach a fixed point"
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[4], b[4])
    assert np.array_equal(ib[:41], ia) and np.all(ib[40:] == ia[-1])
    assert np.all(np.diff(ia) <= 1e-6 * ia[0])  # Lloyd's iteration never raises the inertia (beyond f16 rounding)


# ------------------------------------------------------------------------------------------------------------- invalid
def test_invalid_arguments_are_refused_before_any_launch(eng):
    x = torch.zeros(64, 16, dtype=torch.float16, device="cuda")
    c = torch.zeros(8, 16, dtype=torch.float16, device="cuda")
    n = torch.zeros(8, dtype=torch.float32, device="cuda")
    lab = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def assign(N=64, D=16, ld=16, K=8, ldc=16, rows=x, cent=c, norms=n, labels=lab):
        _lib.call("svc_index_assign", eng._ctx, rows is not None and p(rows) or None, N, D, ld,
                  cent is not None and p(cent) or None, norms is not None and p(norms) or None, K, ldc,
                  labels is not None and p(labels) or None, None, None, None)

    def update(N=64, D=16, ld=16, K=8, ldp=16, ldo=16, out=None, prev=c):
        out = torch.zeros(8, 16, dtype=torch.float16, device="cuda") if out is None else out
        _lib.call("svc_index_update", eng._ctx, p(x), N, D, ld, p(lab), K, p(prev), ldp, p(out), ldo, p(n), None, None)

    def kmeans(N=64, D=16, ld=16, K=8, iters=2, ldc=16, cent=c):
        _lib.call("svc_index_kmeans", eng._ctx, p(x), N, D, ld, K, iters, p(cent), ldc, p(n), None, None, None, None)

    assign(), update(), kmeans()  # the valid calls go through
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    try:
        bad = [lambda: assign(N=0), lambda: assign(N=(1 << 22) + 1), lambda: assign(D=12), lambda: assign(D=0),
               lambda: assign(D=2056), lambda: assign(K=0), lambda: assign(K=65), lambda: assign(ld=8),
               lambda: assign(ldc=12), lambda: assign(rows=None), lambda: assign(cent=None),
               lambda: assign(norms=None), lambda: assign(labels=None), lambda: assign(rows=x.view(-1)[1:]),
               lambda: update(N=0), lambda: update(K=65), lambda: update(D=4), lambda: update(ldo=8),
               lambda: update(ldp=20), lambda: update(out=x), lambda: update(out=c.view(-1)[16:], K=7),
               lambda: kmeans(iters=-1), lambda: kmeans(iters=1001), lambda: kmeans(K=0), lambda: kmeans(K=65),
               lambda: kmeans(D=24, ld=16), lambda: kmeans(cent=x), lambda: kmeans(N=1 << 23)]
        for i, f in enumerate(bad):
            with pytest.raises(_lib.SVCError) as ei:
                f()
            assert "status 1:" in str(ei.value), (i, str(ei.value))  # SVC_ERR_INVALID
        assert _lib.profile_read() == {}
    finally:
        _lib.profile_enable(False)
    with pytest.raises(ValueError):
        eng.index_kmeans(x, 65)
    with pytest.raises(ValueError):
        eng.index_kmeans(x, 8, iters=1001)
    with pytest.raises(ValueError):
        eng.index_assign(x.float(), c, n)


def test_bf16_context_is_refused_with_a_message():
    e = SVCEngine(C.load_config(), 0, operands="bf16")
    try:
        x = torch.zeros(64, 16, dtype=torch.float16, device="cuda")
        c = torch.zeros(8, 16, dtype=torch.float16, device="cuda")
        n = torch.zeros(8, dtype=torch.float32, device="cuda")
        lab = torch.zeros(64, dtype=torch.int32, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        with pytest.raises(_lib.SVCError, match="fp16 only"):
            _lib.call("svc_index_assign", e._ctx, p(x), 64, 16, 16, p(c), p(n), 8, 16, p(lab), None, None, None)
        with pytest.raises(_lib.SVCError, match="fp16 only"):
            _lib.call("svc_index_update", e._ctx, p(x), 64, 16, 16, p(lab), 8, p(c), 16, p(c), 16, p(n), None, None)
        with pytest.raises(_lib.SVCError, match="fp16 only"):
            _lib.call("svc_index_kmeans", e._ctx, p(x), 64, 16, 16, 8, 1, p(c), 16, p(n), None, None, None, None)
        with pytest.raises(ValueError, match="bf16"):
            e.index_kmeans(x, 8)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------ pipeline
TINY = W.WHISPER_DIMS["tiny-test"]


def _tone(f, secs, fs):
    t = np.arange(int(secs * fs)) / fs
    x = 0.3 * np.sin(2 * np.pi * f * t) + 0.15 * np.sin(4 * np.pi * f * t) + 0.08 * np.sin(6 * np.pi * f * t)
    x[int(0.35 * t.size):int(0.5 * t.size)] = 0.0
    return x.astype(np.float32)


def test_enroll_with_a_compacted_index_and_convert():
    """Tiny Whisper, full-size mapper and vocoder with random weights (as tests/test_gpu_retrieve.py builds them)."""
    cfg = C.load_config()
    cfg.mapper.input_content_dim["whisper"] = TINY["n_audio_state"]
    e = SVCEngine(cfg, 0, whisper_state=W.make_whisper_state(TINY, 0), mapper_state=W.make_mapper_state(cfg.mapper, 0),
                  vocoder_state=W.make_vocoder_state(cfg.vocoder, 0))
    try:
        pipe = SVCPipeline(e)
        r24 = [dev(_tone(f, s, 24000)) for f, s in ((140.0, 0.8), (330.0, 0.5))]
        r16 = [dev(np.round(_tone(f, s, 16000) * 32767.0).astype(np.float32) / 32768.0)
               for f, s in ((140.0, 0.8), (330.0, 0.5))]
        kw = dict(wavs24=r24, wavs16=r16, index=True)
        pipe.enroll(1, **kw)
        rows = e.singer_index.get(1)["rows"].clone()
        N = rows.shape[0]
        assert N > 10
        # the default mode is today's entry: rows floor(i N / 10) and their norms, no metadata
        pipe.enroll(1, index_max_rows=10, **kw)
        keep = torch.tensor([i * N // 10 for i in range(10)], device="cuda")
        ent = e.singer_index.get(1)
        assert torch.equal(ent["rows"], rows[keep]) and torch.equal(ent["norms"], e.index_norms(rows[keep]))
        assert "compact" not in ent and ent["frames"] == N
        pipe.enroll(1, index_max_rows=10, index_compact="stride", index_iters=3, **kw)
        assert torch.equal(e.singer_index.get(1)["rows"], rows[keep]) and "compact" not in e.singer_index.get(1)
        # k-means: the engine's own result less the empty centroids; the profile shows the new kernels
        _lib.profile_enable(True)
        try:
            pipe.enroll(1, index_max_rows=10, index_compact="kmeans", index_iters=4, **kw)
            names = {k.split("@")[0] for k in _lib.profile_read()}
        finally:
            _lib.profile_enable(False)
        assert {"index_init", "index_prep", "knn_topk", "index_label", "inertia_sum", "index_hist", "index_scan",
                "index_scatter", "index_sum"} <= names, names
        ent = e.singer_index.get(1)
        cent, norms, counts, inertia = e.index_kmeans(rows, 10, 4)
        live = counts > 0
        assert 1 <= ent["rows"].shape[0] <= 10 and ent["rows"].shape[0] == int(live.sum())
        assert torch.equal(ent["rows"], cent[live]) and torch.equal(ent["norms"], e.index_norms(ent["rows"]))
        assert ent["frames"] == N and ent["n_utts"] == 2
        assert ent["compact"] == dict(method="kmeans", iters=4, inertia_first=float(inertia[0]),
                                      inertia_last=float(inertia[-1]), dropped=10 - int(live.sum()))
        assert ent["compact"]["inertia_last"] <= ent["compact"]["inertia_first"]
        # N <= index_max_rows: both modes keep every row
        pipe.enroll(1, index_max_rows=N, index_compact="kmeans", **kw)
        assert torch.equal(e.singer_index.get(1)["rows"], rows) and "compact" not in e.singer_index.get(1)
        # a conversion against the compacted index
        pipe.enroll(1, index_max_rows=10, index_compact="kmeans", index_iters=4, **kw)
        w24 = [dev(ON.synth_clip(40, 0.6, 24000))]
        w16 = [dev(ON.synth_clip_16k_quantised(40, 0.6))]
        base = pipe.convert_ragged(w24, w16, [1], speedup=250, seed=5)
        outs = pipe.convert_ragged(w24, w16, [1], index_rate=0.5, speedup=250, seed=5)
        assert bool(torch.isfinite(outs[0]).all()) and not torch.equal(outs[0], base[0])
    finally:
        e.close()
