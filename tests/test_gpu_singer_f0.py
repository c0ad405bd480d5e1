"""GPU, A4 per singer: svc_f0_voiced_median (the pooled voiced median of a ragged batch, a multi-workgroup radix
select) against np.median, exactly; the same on the reference's own recorded target contours
(tests/golden/target_f0_contours.npz); svc_pitch_shift_ex (a target and an optional scale per row) against numpy's
restatement, exactly; and SVCPipeline.enroll followed by conversions whose clips shift to their own singers' medians.

Every device buffer of the op-level tests lies between guard zones pre-filled with a nonzero sentinel: a write outside
the payload breaks a guard, and a read outside it changes the voiced count."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import dev, ptr, stream  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine, mel_frames  # noqa: E402

G = 128  # guard elements before and after a payload
SENT = {torch.float64: -7777.25, torch.int64: 0x5A5A5A5A5A5A}
TARGET = 223.25784012425046


class Buf:
    """A flat device payload of n elements between two guard zones, all pre-filled with the dtype's sentinel."""

    def __init__(self, n, dtype=torch.float64, init=None):
        self.sent, self.lo, self.n = SENT[dtype], G, n
        self.full = torch.full((G + n + G,), self.sent, dtype=dtype, device="cuda")
        self.t = self.full[self.lo:self.lo + n]
        assert self.full.data_ptr() % 256 == 0
        if init is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init)).reshape(-1))

    def host(self, *shape):
        a = self.t.cpu().numpy()
        return a.reshape(shape) if shape else a

    def guards_ok(self):
        return bool((self.full[:self.lo] == self.sent).all() and (self.full[self.lo + self.n:] == self.sent).all())


@pytest.fixture(scope="module")
def tiny_engine():
    cfg = C.load_config()
    dims = W.WHISPER_DIMS["tiny-test"]
    cfg.mapper.input_content_dim["whisper"] = dims["n_audio_state"]
    e = SVCEngine(cfg, 0, mapper_state=W.make_mapper_state(cfg.mapper, 0))
    yield e
    e.close()


def _np_median(v):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return np.float64(np.median(v))


def _voiced_median(e, x, frames):
    """One svc_f0_voiced_median call on x f64 [B, T] (frames: host ints [B] or None) -> (median bits uint64, count);
    input and both outputs between guard zones, which must survive."""
    B, T = x.shape
    xin = Buf(B * T, init=x)
    med, cnt = Buf(1), Buf(1, torch.int64)
    fr = None if frames is None else (ctypes.c_int32 * B)(*[int(f) for f in frames])
    _lib.call("svc_f0_voiced_median", e._ctx, ptr(xin.t), B, T, fr, ptr(med.t), ptr(cnt.t), stream())
    torch.cuda.synchronize()
    assert xin.guards_ok() and med.guards_ok() and cnt.guards_ok()
    assert np.array_equal(xin.host(B, T), x, equal_nan=True)  # the input is read only
    return med.host().view(np.uint64)[0], int(cnt.host()[0])


def _median_cases(B, T, frames, rng):
    """(name, x [B, T]) for one shape and length table: the cells at t >= frames[b] hold a nonzero sentinel that must
    not count; the valid cells hold pooled voiced counts 0, 1, 2, an odd and an even one (as far as they fit), one
    repeated value (ties through every pass), two values one ulp apart split about evenly, and mixed signs."""
    valid = np.arange(T)[None, :] < np.asarray([T] * B if frames is None else frames)[:, None]
    nv = int(valid.sum())
    idx = np.flatnonzero(valid.reshape(-1))

    def lay(values):  # values for the valid cells, in order
        x = np.full(B * T, 991.5)
        x[idx] = values
        return x.reshape(B, T)

    odd, even = (nv // 2) | 1, max(2, (nv * 3 // 4) & ~1)
    for n in sorted({0, 1, 2, odd, even, nv}):
        if n <= nv:
            v = np.zeros(nv)
            v[rng.permutation(nv)[:n]] = rng.uniform(65.0, 800.0, n)
            yield f"voiced{n}", lay(v)
    if nv:
        yield "one_value", lay(np.full(nv, 220.0))
        tie = np.zeros(nv)
        tie[rng.permutation(nv)[:max(1, nv // 2)]] = 311.127
        yield "ties_and_unvoiced", lay(tie)
        lo = 233.08188075904496
        yield "one_ulp", lay(np.where(np.arange(nv) % 2 == 0, lo, np.nextafter(lo, 1e9))[rng.permutation(nv)])
        mixed = rng.standard_normal(nv) * 100.0
        mixed[rng.random(nv) < 0.2] = 0.0
        mixed[0] = -57.3
        yield "mixed_signs", lay(mixed)
        yield "negative", lay(-rng.uniform(65.0, 800.0, nv))


def _frame_tables(B, T, rng):
    """None (every row whole) and ragged tables that include 0 and T"""
    tabs = [None]
    if B == 1:
        tabs += [[T], [T - T // 3], [0]]
    else:
        fr = rng.integers(0, T + 1, B)
        fr[0], fr[-1], fr[B // 2] = 0, T, T
        tabs.append(fr.tolist())
        fr2 = rng.integers(0, T + 1, B)
        fr2[0], fr2[-1] = T, 0
        tabs.append(fr2.tolist())
    return tabs


@pytest.mark.parametrize("B,T", [(1, 1), (1, 2), (3, 65), (4, 257), (7, 937), (33, 2123), (1, 70001)])
def test_voiced_median_vs_np(tiny_engine, B, T):
    """svc_f0_voiced_median == np.median(x[x != 0]) over the concatenated valid cells, bit for bit, with the exact
    count: one cell up to 35 workgroups with a partial last one, ragged lengths with 0 and T, every small voiced count,
    ties, neighbours one ulp apart, signed values; NaN where nothing is voiced; two calls give the same bits."""
    rng = np.random.default_rng(1000 * B + T)
    n_cases = 0
    for frames in _frame_tables(B, T, rng):
        valid = np.arange(T)[None, :] < np.asarray([T] * B if frames is None else frames)[:, None]
        for name, x in _median_cases(B, T, frames, rng):
            pooled = x[valid]
            v = pooled[pooled != 0]
            exp = _np_median(v) if v.size else np.float64("nan")
            bits, cnt = _voiced_median(tiny_engine, x, frames)
            got = np.uint64(bits).view(np.float64)
            print(f"B={B} T={T} frames={'all' if frames is None else 'ragged'} {name}: voiced {cnt} median {got!r}")
            assert cnt == v.size, (name, frames)
            if v.size == 0:
                assert np.isnan(got), (name, frames)
            else:
                assert bits == exp.view(np.uint64), (name, frames, got, exp)
            bits2, cnt2 = _voiced_median(tiny_engine, x, frames)
            assert (bits2, cnt2) == (bits, cnt), (name, frames)
            n_cases += 1
    assert n_cases >= 4


def test_voiced_median_reference_contours(tiny_engine, golden):
    """The reference's own target contours (the leading 321 of config/f0.pkl): as a ragged [321, 1282] batch with a
    sentinel in the padding, as its first 320 rows, and as one flat row, each the recorded numpy median and count."""
    g = golden("target_f0_contours")
    f0, lens = g["f0"], g["lengths"].astype(np.int64)
    assert f0.shape == (65437,) and lens.shape == (321,) and int(lens.sum()) == 65437 and int(lens.max()) <= 1282
    T = 1282
    x = np.full((321, T), 991.5)
    off = np.concatenate([[0], np.cumsum(lens)])
    for b in range(321):
        x[b, :lens[b]] = f0[off[b]:off[b + 1]]
    m321, v321 = np.float64(g["median_321"]), int(g["voiced_321"])
    m320, v320 = np.float64(g["median_320"]), int(g["voiced_320"])
    assert (float(m321), v321, float(m320), v320) == (174.73750413040062, 44844, 174.49461696631786, 44671)
    assert _np_median(f0[f0 != 0]) == m321  # the fixture states what numpy gives
    bits, cnt = _voiced_median(tiny_engine, x, lens.tolist())
    assert (bits, cnt) == (m321.view(np.uint64), v321)
    bits, cnt = _voiced_median(tiny_engine, x[:320], lens[:320].tolist())
    assert (bits, cnt) == (m320.view(np.uint64), v320)
    bits, cnt = _voiced_median(tiny_engine, f0[None, :], None)
    assert (bits, cnt) == (m321.view(np.uint64), v321)
    # through the engine method too
    med, n = tiny_engine.f0_voiced_median(torch.from_numpy(x).cuda(), frames=lens.tolist())
    assert med.dtype == torch.float64 and n.dtype == torch.int64
    assert float(med.item()) == float(m321) and int(n.item()) == v321


# ------------------------------------------------------------------ pitch shift with a target per row
def _pitch_rows(T, rng):
    """Rows of f0 [T] float64 for one launch: voiced counts 0, 1, 2, 3, an even and an odd one, all T; one repeated
    value; two values one ulp apart; mixed signs (the recipe of test_gpu_sampler_ops.py, restated)."""
    rows = []
    for n in sorted({0, 1, 2, 3, (T // 2) & ~1, (T // 2) | 1, T - 1, T}):
        if 0 <= n <= T:
            f = np.zeros(T)
            f[rng.permutation(T)[:n]] = rng.uniform(80.0, 600.0, n)
            rows.append(f)
    rows.append(np.full(T, 220.0))
    tie = np.zeros(T)
    tie[rng.permutation(T)[:max(1, T // 2)]] = 311.127
    rows.append(tie)
    rows.append(np.where(rng.random(T) < 0.5, 233.08188075904496, np.nextafter(233.08188075904496, 1e9)))
    mixed = rng.standard_normal(T) * 100.0
    mixed[rng.random(T) < 0.2] = 0.0
    mixed[0] = -57.3  # (never an unvoiced row)
    rows.append(mixed)
    rows.append(-rng.uniform(80.0, 600.0, T))
    return np.stack(rows)


@pytest.mark.parametrize("T", [1, 64, 65, 257, 937])
def test_pitch_shift_ex_vs_np(tiny_engine, T):
    """svc_pitch_shift_ex: row b = f0[b] * (target[b] / np.median(voiced f0[b])), with a scale
    f0[b] * ((target[b] / med) * scale[b]), exactly (a NaN row where nothing is voiced); with equal targets and no
    scale, the bits of svc_pitch_shift."""
    rng = np.random.default_rng(T)
    f0 = _pitch_rows(T, rng)
    B = f0.shape[0]
    targets = rng.uniform(90.0, 500.0, B)
    scales = 2.0 ** (rng.integers(-12, 13, B) / 12.0)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        med = np.array([np.median(r[r != 0]) for r in f0])
    for scale in (None, scales):
        buf = Buf(B * T, init=f0)
        tiny_engine.pitch_shift(buf.t.view(B, T), targets, scale)
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            factor = targets / med
            if scale is not None:
                factor = factor * scale
            exp = f0 * factor[:, None]
        assert np.isnan(exp[0]).all() and np.isfinite(exp[1:]).all()
        np.testing.assert_array_equal(buf.host(B, T), exp)
        assert buf.guards_ok()
    # a tensor of targets takes the same path; equal targets without a scale are the scalar entry's bits
    a, b = Buf(B * T, init=f0), Buf(B * T, init=f0)
    tiny_engine.pitch_shift(a.t.view(B, T), torch.full((B,), TARGET, dtype=torch.float64))
    tiny_engine.pitch_shift(b.t.view(B, T), TARGET)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a.host(B, T), b.host(B, T))
    assert a.guards_ok() and b.guards_ok()


# ------------------------------------------------------------------ enrol, then convert
def _tone(f, secs, fs, pause=(0.35, 0.5)):
    """A harmonic tone at f Hz with a silent stretch (fractions of the clip), f32 [secs * fs]"""
    t = np.arange(int(secs * fs)) / fs
    x = 0.3 * np.sin(2 * np.pi * f * t) + 0.15 * np.sin(4 * np.pi * f * t) + 0.08 * np.sin(6 * np.pi * f * t)
    x[int(pause[0] * t.size):int(pause[1] * t.size)] = 0.0
    return x.astype(np.float32)


def _clip(f, secs):
    """(24 kHz f32, 16 kHz f32 on the int16 grid) device tensors of one tone"""
    return dev(_tone(f, secs, 24000)), dev(np.round(_tone(f, secs, 16000) * 32767.0).astype(np.float32) / 32768.0)


def _full_engines(n):
    """n engines on the same seeded weights (generated once)"""
    cfg = C.load_config()
    dims = W.WHISPER_DIMS["tiny-test"]
    cfg.mapper.input_content_dim["whisper"] = dims["n_audio_state"]
    states = dict(whisper_state=W.make_whisper_state(dims, 0), mapper_state=W.make_mapper_state(cfg.mapper, 0),
                  vocoder_state=W.make_vocoder_state(cfg.vocoder, 0))
    return [SVCEngine(cfg, 0, **states) for _ in range(n)]


class _ScalarPipeline(SVCPipeline):
    """The pitch shift as it was before there were per-singer targets: one scalar call"""

    def shift_f0(self, f0, singers, key_shift=0.0):
        return self.engine.pitch_shift(f0)


def _voiced(x):
    x = np.asarray(x).reshape(-1)
    return x[x != 0]


def test_enroll_then_convert_two_singers():
    e, e2 = _full_engines(2)
    try:
        pipe = SVCPipeline(e)
        (a, a16), (b, b16) = _clip(140.0, 0.45), _clip(330.0, 0.6)
        kw = dict(speedup=250, seed=5)
        ids = lambda *v: dev(np.array(v), torch.int32)  # noqa: E731
        # an empty table and no shift: the scalar path, bit for bit what an engine without any of this computes
        assert len(e.singer_f0) == 0
        before = pipe.convert_ragged([a, b], [a16, b16], [3, 5], **kw)
        plain = _ScalarPipeline(e2).convert_ragged([a, b], [a16, b16], [3, 5], **kw)
        for x, y in zip(before, plain):
            assert torch.equal(x, y)

        # enrolment: the median of the voiced cells of the same clips' F0 rows
        hop, n_fft = e.cfg.hop_length, e.cfg.n_fft
        T_b = [mel_frames(int(w.shape[0]), n_fft, hop) for w in (a, b)]
        raw = [e.f0(w[None].contiguous(), t)[0].cpu().numpy() for w, t in zip((a, b), T_b)]
        assert all(_voiced(r).size > 4 for r in raw), "the test clips must be voiced"
        pooled = _voiced(np.concatenate(raw))
        ent = pipe.enroll(3, wavs24=[a, b])
        assert ent == dict(median=float(np.median(pooled)), voiced=pooled.size, frames=sum(T_b), n_utts=2)
        assert e.singer_f0.get(3) == ent["median"] and e.singer_f0.get(5, TARGET) == TARGET
        m3 = np.float64(ent["median"])
        assert pipe.enroll(3, wavs24=[a, b], max_batch=1) == ent  # chunked: the same rows, the same bits
        with pytest.raises(ValueError, match="voiced"):
            pipe.enroll(7, wavs24=[torch.zeros(12000, device="cuda")])
        assert 7 not in e.singer_f0 and len(e.singer_f0) == 1

        # a ragged batch to an enrolled and an unenrolled singer == each clip alone
        outs = pipe.convert_ragged([a, b], [a16, b16], [3, 5], **kw)
        one = [pipe.convert(w[None].contiguous(), w16[None].contiguous(), ids(s), utt_ids=ids(i), **kw)
               for i, (w, w16, s) in enumerate(((a, a16, 3), (b, b16, 5)))]
        for i in range(2):
            assert torch.equal(outs[i], one[i].wav[0]), i
        assert not torch.equal(outs[0], before[0]) and torch.equal(outs[1], before[1])
        med = [np.float64(np.median(_voiced(r))) for r in raw]
        np.testing.assert_array_equal(one[0].f0[0].cpu().numpy(), raw[0] * (m3 / med[0]))
        np.testing.assert_array_equal(one[1].f0[0].cpu().numpy(), raw[1] * (np.float64(e.target_f0_median) / med[1]))

        # an octave up on clip 0 only: its factor doubles exactly
        up = pipe.convert(a[None].contiguous(), a16[None].contiguous(), ids(3), utt_ids=ids(0), key_shift=[12], **kw)
        np.testing.assert_array_equal(up.f0[0].cpu().numpy(), raw[0] * ((m3 / med[0]) * 2.0))
        np.testing.assert_array_equal(up.f0[0].cpu().numpy(), 2.0 * one[0].f0[0].cpu().numpy())
        shifted = pipe.convert_ragged([a, b], [a16, b16], [3, 5], key_shift=[12, 0], **kw)
        assert torch.equal(shifted[0], up.wav[0]) and torch.equal(shifted[1], one[1].wav[0])
    finally:
        e.close()
        e2.close()
