"""GPU: feature retrieval (svc_index_norms, svc_content_retrieve) against the f64 reference of tests/retrieve_ref.py.

Inputs are drawn on the CPU from a fixed seed: index rows are f16 normals, queries 0.7 * (a random index row) +
0.5 * normal. B = 3, T = 70, frames = [70, 33, 1]: 210 rows are no multiple of the 128-query tile and one clip has a
single row; N in {1, 7, 300, 2100} lies below k, inside one 128-row index tile, and across 3 and 17 tiles (which the
default grid splits 3 and 17 ways); D in {64, 256, 1024} is one, four and sixteen 64-half LDS stages; every row stride
is larger than D, and the columns past D hold a sentinel that must survive.

The selection is judged with tau, the derived worst-case error of a device f32 score (retrieve_ref.tau): no row is left
out, and wherever the reference's own gaps exceed tau the device's set and order must be the reference's exactly."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import retrieve_ref as R  # noqa: E402
from gpu_util import dev  # noqa: E402
from oracle import noise as ON  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine, mel_frames  # noqa: E402

B, T, FRAMES = 3, 70, [70, 33, 1]
SENT = 0x5A5A  # the f16 bit pattern of every pad column (203.25)
CASES = [(1, 64, 1), (1, 256, 8), (7, 64, 8), (7, 1024, 4), (300, 64, 1), (300, 64, 8), (300, 256, 4), (300, 1024, 8),
         (2100, 64, 4), (2100, 256, 8), (2100, 1024, 4), (2100, 1024, 8)]
LIVE = np.array([t < FRAMES[b] for b in range(B) for t in range(T)])


@pytest.fixture(scope="module")
def eng():
    e = SVCEngine(C.load_config(), 0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _data(N, D):
    """(q f16 [B*T, D], x f16 [N, D], norms f32 [N], s f64 [B*T, N], sorted s, tau [B*T]); computed once per (N, D),
    shared by the tests and never modified."""
    rng = np.random.default_rng([17, N, D])
    x = rng.standard_normal((N, D)).astype(np.float16)
    q = (0.7 * x[rng.integers(0, N, B * T)].astype(np.float32) + 0.5 * rng.standard_normal((B * T, D))).astype(np.float16)
    q[0, :4] = [-0.0, 0.0, -0.0, 1.0]  # signed zeros: rate = 0 must keep their bits
    norms = R.index_norms(x)
    s = R.scores(q, x, norms)
    out = (q, x, norms, s, np.sort(s, axis=1), R.tau(q, x, norms))
    for a in out:
        a.setflags(write=False)
    return out


def _padded(a, ld):
    """f16 [R, D] -> device f16 [R, ld], the columns past D holding the sentinel"""
    a = np.ascontiguousarray(a, np.float16)
    buf = np.full((a.shape[0], ld), SENT, np.uint16)
    buf[:, :a.shape[1]] = a.view(np.uint16)
    return torch.from_numpy(buf.view(np.int16)).view(torch.float16).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _run(eng, q, x, norms=None, frames=FRAMES, sel=None, k=8, rate=0.5, floor=None, shape=(B, T), pads=(8, 16, 24),
         inplace=False):
    """content_retrieve on padded buffers -> (out bits uint16 [B*T, ld_out], idx [B*T, k], d2 [B*T, k], device norms).
    Checked here: the index, the norms and (unless in place) the content come back unchanged."""
    b, t = shape
    D = q.shape[1]
    ld, ldx, ldo = D + pads[0], D + pads[1], D + pads[2]
    qb, xb = _padded(q, ld), _padded(x, ldx)
    nd = eng.index_norms(xb[:, :D])
    if norms is not None:
        assert np.array_equal(nd.cpu().numpy(), norms)  # the f64 sums rounded once: exact
    content = qb.view(b, t, ld)[:, :, :D]
    if inplace:
        ob = qb
    else:
        ob = _padded(np.zeros((b * t, D), np.float16), ldo)
        ob.view(torch.int16).fill_(SENT)  # every column: a row the call must write shows if it does not
    out = ob.view(b, t, ob.shape[1])[:, :, :D]
    res, idx, d2 = eng.content_retrieve(content, xb[:, :D], nd, frames=frames, sel=sel, k=k, rate=rate,
                                        dist_floor=floor, out=out, return_neighbours=True)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    assert np.array_equal(_bits(xb), _bits(_padded(x, ldx)))
    if not inplace:
        assert np.array_equal(_bits(qb), _bits(_padded(q, ld)))
    return _bits(ob), idx.cpu().numpy().reshape(b * t, k), d2.cpu().numpy().reshape(b * t, k), nd


def _f16(bits):
    return np.ascontiguousarray(bits).view(np.float16)


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("N,D,k", CASES, ids=lambda v: str(v))
def test_against_the_reference(eng, N, D, k):
    """Selection, distances and output of every live row (figures printed before they are asserted).
    The bounds are derived, not fitted. Largest observed on MI355X over the twelve cases: d2 error / tau 0.010
    (N = 7 and 2100, D = 64), output error / bound 0.43 (N = 1, D = 64, where the bound is little more than the one f16
    ulp); at D = 1024 they are 0.002 and 0.11. Rows whose k-th gap is clear of tau (set and order then exact): all 104
    live rows at D = 64, 90 of 104 at (2100, 1024, 8), the least."""
    q, x, norms, s, srt, tau = _data(N, D)
    rate, floor = 0.75, 1e-4 * D
    k_eff = min(k, N)
    out, idx, d2, _ = _run(eng, q, x, norms, k=k, rate=rate)
    assert np.all(out[:, D:] == SENT)
    # a condition on the inputs, from the reference alone: most rows have a clear k-th gap
    if k_eff < N:
        clear = (srt[:, k_eff] - srt[:, k_eff - 1]) > tau
        print("rows with a gap above tau: %.1f %%" % (100.0 * clear[LIVE].mean()))
        assert clear[LIVE].mean() >= 0.8
    xmax = float(np.abs(x.astype(np.float64)).max())
    worst_out = worst_d = 0.0
    exact_rows = 0
    for r in np.flatnonzero(LIVE):
        got = idx[r]
        assert np.all(got[k_eff:] == -1) and np.all(d2[r, k_eff:] == 0.0), r
        sel_j = got[:k_eff]
        assert np.all((sel_j >= 0) & (sel_j < N)) and len(set(sel_j.tolist())) == k_eff, (r, sel_j)
        sk = srt[r, k_eff - 1]
        assert np.all(s[r, sel_j] <= sk + tau[r]), (r, sel_j)
        must = np.flatnonzero(s[r] < sk - tau[r])
        assert set(must.tolist()) <= set(sel_j.tolist()), r
        ref_order = R.order(s[r])[:k_eff]
        if k_eff == N or srt[r, k_eff] - sk > tau[r]:
            assert set(sel_j.tolist()) == set(ref_order.tolist()), r
            exact_rows += 1
            for i in range(k_eff - 1):  # the reference's order wherever its adjacent gap is clear
                if srt[r, i + 1] - srt[r, i] > tau[r]:
                    assert set(sel_j[:i + 1].tolist()) == set(ref_order[:i + 1].tolist()), (r, i)
        want, d2_ref = R.blend_row(q[r], x, s[r], sel_j, rate, floor)
        f32floor = float(np.float32(floor))
        at_floor = (d2[r, :k_eff] == np.float32(floor)) & (d2_ref == f32floor)
        derr = np.abs(d2[r, :k_eff].astype(np.float64) - d2_ref)
        assert np.all(at_floor | (derr <= tau[r])), (r, derr, tau[r])
        worst_d = max(worst_d, float((derr / tau[r]).max()))
        bound = R.f16_ulp(want) + 2.0 * xmax * tau[r] / d2_ref.min()
        err = np.abs(_f16(out[r, :D]).astype(np.float64) - want)
        worst_out = max(worst_out, float((err / bound).max()))
        assert np.all(err <= bound), (r, float((err / bound).max()))
    print("N=%d D=%d k=%d: %d of %d rows exact; worst d2 err / tau %.3f, worst out err / bound %.3f"
          % (N, D, k, exact_rows, int(LIVE.sum()), worst_d, worst_out))
    # the rows that take no part
    dead = ~LIVE
    assert np.all(idx[dead] == -1) and np.all(d2[dead] == 0.0)
    assert np.all(out[dead, :D] == 0)  # +0


@pytest.mark.parametrize("N,D,k", [(300, 64, 8), (2100, 256, 4), (300, 1024, 4)], ids=lambda v: str(v))
def test_exact_matches(eng, N, D, k):
    """Every query is a copy of an index row and dist_floor = 4 tau: the match ranks first, its d2 is the floor on the
    device and in the reference, and the output obeys the reference test's bound."""
    _, x, norms, _, _, _ = _data(N, D)
    rng = np.random.default_rng([23, N, D])
    src = rng.integers(0, N, B * T)
    q = x[src].copy()
    s = R.scores(q, x, norms)
    tau = R.tau(q, x, norms)
    floor = float(np.float32(4.0 * tau.max()))
    out, idx, d2, _ = _run(eng, q, x, norms, k=k, rate=1.0, floor=floor)
    xmax = float(np.abs(x.astype(np.float64)).max())
    for r in np.flatnonzero(LIVE):
        assert idx[r, 0] == src[r], (r, idx[r], src[r])
        want, d2_ref = R.blend_row(q[r], x, s[r], idx[r], 1.0, floor)
        assert d2[r, 0] == np.float32(floor) and d2_ref[0] == floor
        err = np.abs(_f16(out[r, :D]).astype(np.float64) - want)
        assert np.all(err <= R.f16_ulp(want) + 2.0 * xmax * tau[r] / d2_ref.min()), r


def test_exact_ties_go_to_the_lower_index(eng):
    """Rows 127, 128 and 129 are one vector (a 128-row tile boundary runs through them; 128 and 129 meet in one lane's
    list) and so are 100 and 256 (different tiles, and different splits when the index is split): equal scores bit for
    bit, so the lower j wins, also where the rank boundary cuts the tie (k = 2), for every number of splits."""
    N, D = 300, 64
    q, x, _, _, _, _ = _data(N, D)
    x = x.copy()
    x[128] = x[127]
    x[129] = x[127]
    x[256] = x[100]
    q = q.copy()
    q[1] = x[127]
    q[2] = (x[127].astype(np.float32) + 0.01).astype(np.float16)
    q[3] = x[100]
    try:
        for splits in (0, 1, 2, 5):
            eng.tune(retrieve_splits=splits)
            for k in (2, 8):
                _, idx, d2, _ = _run(eng, q, x, k=k)
                assert list(idx[1, :2]) == [127, 128] and list(idx[2, :2]) == [127, 128], (splits, k, idx[1], idx[2])
                assert list(idx[3, :2]) == [100, 256], (splits, k, idx[3])
                if k == 8:
                    assert list(idx[1, :3]) == [127, 128, 129] and list(idx[2, :3]) == [127, 128, 129]
                    assert d2[2, 0] == d2[2, 1] == d2[2, 2]
    finally:
        eng.tune(reset=1)


# ------------------------------------------------------------------------------------------------ bit identity
def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))


@pytest.mark.parametrize("N,D,k", [(300, 256, 4), (2100, 64, 8)], ids=lambda v: str(v))
def test_each_clip_alone_and_every_split_count(eng, N, D, k):
    q, x, norms, _, _, _ = _data(N, D)
    full = _run(eng, q, x, norms, k=k)
    for b in range(B):
        rows = slice(b * T, b * T + FRAMES[b])
        one = _run(eng, q[rows], x, norms, frames=None, k=k, shape=(1, FRAMES[b]))
        for u, v in zip(full[:3], one[:3]):
            assert np.array_equal(u[rows], v), b
    try:
        for splits in (1, 2, 5):
            eng.tune(retrieve_splits=splits)
            assert _same(_run(eng, q, x, norms, k=k), full), splits
    finally:
        eng.tune(reset=1)
    assert eng.get_config("tune.retrieve_splits") == 0.0


def test_in_place_rate_zero_and_sel(eng):
    N, D, k = 300, 256, 4
    q, x, norms, _, _, _ = _data(N, D)
    ld = D + 8
    full = _run(eng, q, x, norms, k=k)
    inpl = _run(eng, q, x, norms, k=k, inplace=True)
    assert np.array_equal(inpl[0][:, :D], full[0][:, :D]) and np.all(inpl[0][:, D:] == SENT)
    assert np.array_equal(inpl[1], full[1]) and np.array_equal(inpl[2], full[2])
    # rate = 0: the live rows are the input's bits (signed zeros included), the neighbours are still reported
    zero = _run(eng, q, x, norms, k=k, rate=0.0)
    qbits = np.ascontiguousarray(q).view(np.uint16)
    assert np.array_equal(zero[0][LIVE, :D], qbits[LIVE]) and np.all(zero[0][~LIVE, :D] == 0)
    assert qbits[0, 0] == 0x8000 and zero[0][0, 0] == 0x8000
    assert np.array_equal(zero[1], full[1]) and np.array_equal(zero[2], full[2])
    # sel = [1, 0, 1]: clip 1 takes no part. A separate output receives a copy of its rows (all T of them); in place
    # they are not touched; the selected clips are as in the full call; pad columns keep the sentinel
    clip1 = np.zeros(B * T, bool)
    clip1[T:2 * T] = True
    part = _run(eng, q, x, norms, k=k, sel=[1, 0, 1])
    assert np.array_equal(part[0][clip1, :D], qbits[clip1]) and np.all(part[0][:, D:] == SENT)
    assert np.array_equal(part[0][~clip1], full[0][~clip1])
    assert np.all(part[1][clip1] == -1) and np.all(part[2][clip1] == 0.0)
    assert np.array_equal(part[1][~clip1], full[1][~clip1]) and np.array_equal(part[2][~clip1], full[2][~clip1])
    pin = _run(eng, q, x, norms, k=k, sel=[1, 0, 1], inplace=True)
    assert np.array_equal(pin[0][clip1, :D], qbits[clip1]) and np.all(pin[0][:, D:] == SENT)
    assert np.array_equal(pin[0][~clip1, :D], full[0][~clip1, :D])
    assert pin[0].shape[1] == ld


def test_second_call_does_not_grow_the_workspace(eng):
    q, x, norms, _, _, _ = _data(2100, 64)
    first = _run(eng, q, x, norms, k=8)
    mem = eng.memory()[1]
    assert mem > 0
    again = _run(eng, q, x, norms, k=8)
    assert eng.memory()[1] == mem and _same(first, again)
    small = _run(eng, q[:T], x[:7], k=8, frames=None, shape=(1, T))  # a smaller call leaves the arena alone
    assert eng.memory()[1] == mem and small[1].shape == (T, 8)


def test_bf16_context_is_refused_with_a_message():
    e = SVCEngine(C.load_config(), 0, operands="bf16")
    try:
        buf = torch.zeros(64, 16, dtype=torch.float16, device="cuda")
        nrm = torch.zeros(64, dtype=torch.float32, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        with pytest.raises(_lib.SVCError, match="fp16 only"):
            _lib.call("svc_index_norms", e._ctx, p(buf), 64, 16, 16, p(nrm), None)
        out = torch.zeros(8, 16, dtype=torch.float16, device="cuda")
        with pytest.raises(_lib.SVCError, match="fp16 only"):
            _lib.call("svc_content_retrieve", e._ctx, p(buf), 2, 4, None, None, 16, 16, p(buf), p(nrm), 64, 16, 4, 0.5,
                      1e-3, p(out), 16, None, None, None)
        with pytest.raises(ValueError, match="bf16"):
            e.content_retrieve(buf[:8].view(2, 4, 16), buf, nrm)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ end to end
TINY = W.WHISPER_DIMS["tiny-test"]
SECS = [0.6, 1.0, 0.6]


def _tone(f, secs, fs):
    """A harmonic tone at f Hz with a silent stretch, f32 [secs * fs]"""
    t = np.arange(int(secs * fs)) / fs
    x = 0.3 * np.sin(2 * np.pi * f * t) + 0.15 * np.sin(4 * np.pi * f * t) + 0.08 * np.sin(6 * np.pi * f * t)
    x[int(0.35 * t.size):int(0.5 * t.size)] = 0.0
    return x.astype(np.float32)


def test_enroll_and_convert_end_to_end():
    """Tiny Whisper, full-size mapper and vocoder with random weights (as tests/test_gpu_shallow.py builds them)."""
    cfg = C.load_config()
    cfg.mapper.input_content_dim["whisper"] = TINY["n_audio_state"]
    e = SVCEngine(cfg, 0, whisper_state=W.make_whisper_state(TINY, 0), mapper_state=W.make_mapper_state(cfg.mapper, 0),
                  vocoder_state=W.make_vocoder_state(cfg.vocoder, 0))
    try:
        pipe = SVCPipeline(e)
        w24 = [dev(ON.synth_clip(40 + i, s, 24000)) for i, s in enumerate(SECS)]
        w16 = [dev(ON.synth_clip_16k_quantised(40 + i, s)) for i, s in enumerate(SECS)]
        r24 = [dev(_tone(f, s, 24000)) for f, s in ((140.0, 0.8), (330.0, 0.5))]  # voiced: the F0 enrolment needs it
        r16 = [dev(np.round(_tone(f, s, 16000) * 32767.0).astype(np.float32) / 32768.0)
               for f, s in ((140.0, 0.8), (330.0, 0.5))]
        singers = [1, 3, 1]
        kw = dict(speedup=250, seed=5)
        # F0 enrolment alone, then the conversions every later comparison starts from
        ent = pipe.enroll(1, wavs24=r24)
        base = pipe.convert_ragged(w24, w16, singers, **kw)
        assert not e.singer_index
        assert all(torch.equal(a, b) for a, b in zip(pipe.convert_ragged(w24, w16, singers, index_rate=0.5, **kw), base))
        # with the index: the F0 entry is the same, the index holds each recording's own content rows
        assert pipe.enroll(1, wavs24=r24, wavs16=r16, index=True) == ent
        T_r = [mel_frames(int(w.shape[0]), cfg.n_fft, cfg.hop_length) for w in r24]
        entry = e.singer_index.get(1)
        c = pipe.ragged_content(r16, T_r, max(T_r))
        rows = torch.cat([c[b, :t] for b, t in enumerate(T_r)])
        assert torch.equal(entry["rows"], rows) and entry["frames"] == sum(T_r) and entry["n_utts"] == 2
        assert entry["content_types"] == ["whisper"] and torch.equal(entry["norms"], e.index_norms(rows))
        assert np.array_equal(entry["norms"].cpu().numpy(), R.index_norms(rows.cpu().numpy()))
        assert pipe.enroll(1, wavs24=r24, wavs16=r16, index=True, max_batch=1) == ent  # chunked: the same rows
        assert torch.equal(e.singer_index.get(1)["rows"], rows)
        pipe.enroll(1, wavs24=r24, wavs16=r16, index=True, index_max_rows=10)
        keep = [i * rows.shape[0] // 10 for i in range(10)]
        assert torch.equal(e.singer_index.get(1)["rows"], rows[keep]) and e.singer_index.get(1)["frames"] == sum(T_r)
        pipe.enroll(1, wavs24=r24, wavs16=r16, index=True)
        # index_rate = None: as a pipeline that never enrolled an index
        assert all(torch.equal(a, b) for a, b in zip(pipe.convert_ragged(w24, w16, singers, **kw), base))
        assert all(torch.equal(a, b) for a, b in zip(pipe.convert_ragged(w24, w16, singers, index_rate=None, **kw), base))
        # index_rate = 0.5: the conditioner receives content_retrieve's result, called by hand
        T_b = [mel_frames(int(w.shape[0]), cfg.n_fft, cfg.hop_length) for w in w24]
        plain = pipe.ragged_content(w16, T_b, max(T_b))
        hand = e.content_retrieve(plain, rows, entry["norms"], frames=T_b, sel=[1, 0, 1], rate=0.5)
        seen = []
        cond = e.condition
        e.condition = lambda content, *a: seen.append(content.clone()) or cond(content, *a)
        try:
            outs = pipe.convert_ragged(w24, w16, singers, index_rate=0.5, **kw)
        finally:
            del e.condition
        assert len(seen) == 1 and torch.equal(seen[0], hand)
        assert torch.equal(hand[1], plain[1]) and not torch.equal(hand[0], plain[0])  # singer 3 has no index
        assert all(bool(torch.isfinite(o).all()) for o in outs)
        # the mixed batch changes only the enrolled singer's clips
        assert torch.equal(outs[1], base[1]) and not torch.equal(outs[0], base[0]) and not torch.equal(outs[2], base[2])
        many = pipe.convert_many(w24, w16, singers, index_rate=0.5, **kw)
        assert all(torch.equal(a, b) for a, b in zip(many, outs))
    finally:
        e.close()
