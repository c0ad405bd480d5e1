"""A1 on the GPU: svc_load_pcm (wav payloads of a ragged batch -> the 24 kHz source rows and the 16 kHz mono rows)
against the per-file host path.

The yardstick everywhere is the path the project had before, on the same bytes written to a file of their own:
audio.load_audio / audio.load_whisper_audio for that file alone, compared exactly (np.array_equal): the kernels restate
that path's arithmetic, so there is no tolerance to choose. In addition the source rows are held to
read_wav + _normalise + scipy.signal.resample_poly in f64 within test_gpu_audio.py's bound,
2e-7 * max(max |ref|, 1e-3) + 1e-9, and the mono rows to that test's int16 criterion (within one step of the rounded f64
result). Every op-level call pre-fills its outputs with a sentinel, some floats before the first row and one guard row
after the last included, and checks them, the zero tails and the sentinels around the rows.

Sizes: the row kernels give a workgroup 1024 output samples and the peak pass 4096 frames (load_pcm.hip kChunk,
kPeakChunk); rows here cross those counts with remainders, and one case uses rate ratios (384 kHz input) at which a
workgroup walks its samples in several LDS tiles."""
import ctypes
import functools
import os
import tempfile
import wave

import numpy as np
import pytest
import scipy.signal as ss
import torch

pytestmark = pytest.mark.gpu

from gpu_util import ptr, stream  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import audio as A  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import infer as I  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402
from svc_inference_pipeline_amd.serving import SVCServer  # noqa: E402
from wav_util import F32, F64, S16, S24, S32, U8, random_samples, wav_bytes  # noqa: E402

SENTINEL = 7.5
PRE = 5  # sentinel floats in front of the first row (the rows then start off any 16-byte boundary)
FS, SR16 = 24000, 16000
CLIP = os.path.join(os.path.dirname(__file__), "golden", "test_set_1100000814.wav")


@pytest.fixture(scope="module")
def engine():
    """A context without weights: svc_load_pcm needs none."""
    e = SVCEngine(C.load_config(), 0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def host_path(data, fs=FS):
    """The per-file path on these bytes alone -> (load_audio's row or None, load_whisper_audio's row, read_wav's f64
    samples, rate); computed once per file and shared."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.wav")
        with open(path, "wb") as fh:
            fh.write(data)
        with np.errstate(all="ignore"):
            src = A.load_audio(path, fs)
            mono = A.load_whisper_audio(path)
            x, sr = A.read_wav(path)
    return (None if src is None else src.cpu().numpy()), mono.cpu().numpy(), x, sr


def expected_info(x64):
    """info of a file from read_wav's samples by _normalise's rule: the class of channel 0's peak, bit 2 when the
    normalised float samples are not all finite"""
    with np.errstate(all="ignore"):
        c0 = x64[:, 0]
        mx = max(float(np.amax(c0)), float(-np.amin(c0)))
        cls = 2 if mx > 2 ** 15 else (1 if mx > 1.01 else 0)
        return cls | (0 if np.isfinite(A._normalise(c0)).all() else 4)


def launch(e, files, offsets=None, sr_src=FS, sr_mono=SR16, want_src=True, want_mono=True):
    """One svc_load_pcm call on whole wav files (bytes): their payloads go into one device buffer at `offsets`
    (default: packed behind 1 filler byte each, so most starts are odd) between 0xA5 filler bytes."""
    infos = [A.parse_wav(f) for f in files]
    B = len(infos)
    if offsets is None:
        offsets, pos = [], 1
        for i in infos:
            offsets.append(pos)
            pos += len(i.payload) + 1
            pos += 1 - pos % 2  # keep the next start odd
    total = max(o + len(i.payload) for o, i in zip(offsets, infos)) + 3
    host = np.full(total, 0xA5, dtype=np.uint8)
    for o, i in zip(offsets, infos):
        host[o:o + len(i.payload)] = np.frombuffer(i.payload, dtype=np.uint8)
    raw = torch.from_numpy(host).cuda()
    lib = _lib.load()
    n_src = [int(lib.svc_resample_len(i.n_frames, i.sr, sr_src)) for i in infos]
    n_mono = [int(lib.svc_resample_len(i.n_frames, i.sr, sr_mono)) for i in infos]
    S_src, S_mono = max(1, max(n_src)) + 3, max(1, max(n_mono)) + 2  # rows longer than the longest utterance
    ysrc = torch.full((PRE + (B + 1) * S_src,), SENTINEL, device="cuda") if want_src else None
    ymono = torch.full((PRE + (B + 1) * S_mono,), SENTINEL, device="cuda") if want_mono else None
    info = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
    i64, i32 = ctypes.c_int64 * B, ctypes.c_int32 * B
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * PRE) if t is not None else None  # noqa: E731
    _lib.call("svc_load_pcm", e._ctx, ptr(raw), B, i64(*offsets), i64(*[i.n_frames for i in infos]),
              i32(*[i.format for i in infos]), i32(*[i.channels for i in infos]), i32(*[i.sr for i in infos]),
              sr_src, S_src, off(ysrc), sr_mono, S_mono, off(ymono), ptr(info), stream())
    torch.cuda.synchronize()

    def rows(buf, S, n):
        if buf is None:
            return None
        flat = buf.cpu().numpy()
        assert np.all(flat[:PRE] == SENTINEL), "floats before the first row were written"
        assert np.all(flat[PRE + B * S:] == SENTINEL), "the guard row after the last row was written"
        y = flat[PRE:PRE + B * S].reshape(B, S)
        for b in range(B):
            assert not y[b, n[b]:].any(), f"row {b}: the tail past its {n[b]} samples is not zero"
        return [y[b, :n[b]] for b in range(B)]

    flags = info.cpu().numpy()
    assert flags[B] == -1
    return rows(ysrc, S_src, n_src), rows(ymono, S_mono, n_mono), flags[:B]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def check_against_host(files, src_rows, mono_rows, flags, fs=FS):
    """Every row against the per-file path (exact), the f64 scipy bound on the source rows and the int16 criterion on
    the mono rows, info against _normalise's rule."""
    for b, data in enumerate(files):
        ref_src, ref_mono, x, sr = host_path(data, fs)
        assert flags[b] == expected_info(x), (b, flags[b])
        if mono_rows is not None:
            assert same(mono_rows[b], ref_mono), (b, "mono")
        if flags[b] & 4:
            assert ref_src is None  # load_audio refuses the file; its rows are unspecified
            continue
        if src_rows is not None:
            assert same(src_rows[b], ref_src), (b, "source", int(np.argmax(src_rows[b] != ref_src)))
            norm = A._normalise(x[:, 0]).astype(np.float64)
            ref = norm if sr == fs else ss.resample_poly(norm, fs, sr)
            assert np.max(np.abs(src_rows[b] - ref)) <= 2e-7 * max(np.max(np.abs(ref)), 1e-3) + 1e-9, (b, "scipy")
        if mono_rows is not None and np.isfinite(x).all():
            m = x.mean(axis=1).astype(np.float32).astype(np.float64)
            q = np.clip(np.round(ss.resample_poly(m, SR16, sr) * 32768.0), -32768, 32767)
            got = mono_rows[b].astype(np.float64) * 32768.0
            assert np.array_equal(got, np.round(got)) and np.max(np.abs(got - q)) <= 1.0, (b, "int16 grid")


FORMAT_CASES = [(f, c) for f in (U8, S16, S24, S32, F32, F64) for c in (1, 2, 3)] + [(F64, 7), (F64, 8), (S16, 8)]


@pytest.mark.parametrize("fmt,ch", FORMAT_CASES)
def test_formats_and_channel_counts(engine, fmt, ch):
    """257 frames already at 24 kHz: the source row is the decoded, normalised channel 0 itself (a pure decode check,
    integer formats over their whole range), the mono row the channel mean through the 24 -> 16 kHz filter; 7 and 8
    channels pin numpy's summation order (sequential below 8, pairwise at 8)."""
    data = wav_bytes(fmt, random_samples(np.random.default_rng(100 * fmt + ch), fmt, 257, ch), FS)
    src, mono, flags = launch(engine, [data])
    _, _, x, _ = host_path(data)
    assert same(src[0], A._normalise(x[:, 0]))
    assert flags[0] == 0
    check_against_host([data], src, mono, flags)


@pytest.fixture(scope="module")
def ragged_files():
    rng = np.random.default_rng(7)
    spec = [(S16, 2, 44100, 4099), (S24, 1, 48000, 1001), (F32, 3, 22050, 300), (S32, 2, 16000, 7), (F64, 1, 24000, 3)]
    return [wav_bytes(f, random_samples(rng, f, n, ch), sr) for f, ch, sr, n in spec]


def test_ragged_mixed_rates_in_one_call(engine, ragged_files):
    """B = 5, rates 44100 / 48000 / 22050 / 16000 / 24000 (five plans; the 24 kHz source row is unfiltered, the 16 kHz
    mono row goes through the up = down = 1 filter), mixed formats and channel counts, 3 to 4099 frames (2231 source
    samples: two whole workgroups and a remainder), every payload at an odd byte offset. Each row is exact against the
    per-file path, and each utterance run alone (B = 1) gives the same bits."""
    offsets, pos = [], 3
    for f in ragged_files:
        offsets.append(pos)
        pos += len(A.parse_wav(f).payload) + 2
        pos += 1 - pos % 2
    assert all(o % 2 == 1 for o in offsets)
    src, mono, flags = launch(engine, ragged_files, offsets)
    assert [len(r) for r in src] == [2231, 501, 327, 11, 3] and [len(r) for r in mono] == [1488, 334, 218, 7, 2]
    check_against_host(ragged_files, src, mono, flags)
    for b, data in enumerate(ragged_files):
        s1, m1, f1 = launch(engine, [data], [b])  # another offset, too
        assert same(s1[0], src[b]) and same(m1[0], mono[b]) and f1[0] == flags[b], b
    only_src, none, f2 = launch(engine, ragged_files, offsets, want_mono=False)
    none2, only_mono, f3 = launch(engine, ragged_files, offsets, want_src=False)
    assert none is None and none2 is None and np.array_equal(f2, flags) and np.array_equal(f3, flags)
    assert all(same(a, b) for a, b in zip(only_src, src)) and all(same(a, b) for a, b in zip(only_mono, mono))


def test_large_rate_ratio_walks_several_tiles(engine):
    """384 kHz input: down / up is 16 for the source row and 24 for the mono row, so a workgroup's 1024 samples need more
    input than its LDS buffer holds and are walked in tiles of 491 and 321 samples; 40000 and 1500 frames in one call."""
    rng = np.random.default_rng(21)
    files = [wav_bytes(S16, random_samples(rng, S16, 40000, 1), 384000),
             wav_bytes(F32, random_samples(rng, F32, 1500, 2), 384000)]
    src, mono, flags = launch(engine, files)
    assert [len(r) for r in src] == [2500, 94] and [len(r) for r in mono] == [1667, 63]
    check_against_host(files, src, mono, flags)


@pytest.mark.parametrize("where,sr", [("first", FS), ("last", 44100), ("boundary", FS)])
def test_normalisation_classes(engine, where, sr):
    """F32 with a channel-0 peak of 300 (class 1: / 32769), F64 with -70000 (class 2: / 2^31), stereo F32 whose
    channel 1 reaches 70000 while channel 0 stays within 0.5 (class 0: only channel 0 counts); 5000 frames, the peak in
    the first sample, in the last, or on either side of the peak pass's 4096-frame block boundary. At 24 kHz the source
    row is _normalise's output itself; at 44.1 kHz the normalised samples go through the filter."""
    rng = np.random.default_rng(3)
    n = 5000
    at = {"first": (0, 0), "last": (n - 1, n - 1), "boundary": (4096, 4095)}[where]
    a = random_samples(rng, F32, n, 1)
    a[at[0], 0] = 300.0
    b = random_samples(rng, F64, n, 2)
    b[at[1], 0] = -70000.0
    c = random_samples(rng, F32, n, 2)
    c[at[0], 1] = 70000.0
    files = [wav_bytes(F32, a, sr), wav_bytes(F64, b, sr), wav_bytes(F32, c, sr)]
    src, mono, flags = launch(engine, files)
    assert flags.tolist() == [1, 2, 0]
    check_against_host(files, src, mono, flags)
    if sr == FS:
        for k, x in enumerate((a, b, c)):
            assert same(src[k], A._normalise(np.asarray(x[:, 0], dtype=np.float64))), k
        assert float(np.abs(src[0]).max()) == np.float32(300.0) / np.float32(32769.0) and np.abs(src[2]).max() <= 0.5


@pytest.fixture(scope="module")
def nonfinite_files():
    rng = np.random.default_rng(9)
    n = 600
    nan32 = random_samples(rng, F32, n, 1)
    nan32[123, 0] = np.nan
    inf64 = random_samples(rng, F64, n, 2)
    inf64[n - 1, 0] = -np.inf
    big64 = random_samples(rng, F64, n, 1)
    big64[0, 0] = 1e39  # finite, beyond the f32 range
    nan_ch1 = random_samples(rng, F32, n, 2)
    nan_ch1[7, 1] = np.nan
    fine = random_samples(rng, S16, n, 1)
    return [wav_bytes(F32, nan32, 44100), wav_bytes(F64, inf64, 44100), wav_bytes(F64, big64, 48000),
            wav_bytes(F32, nan_ch1, 44100), wav_bytes(S16, fine, 44100)]


def test_non_finite_samples_set_bit_2(engine, nonfinite_files):
    """A NaN in F32 channel 0, an Inf in F64 channel 0 and a finite F64 value of 1e39 set bit 2; a NaN in channel 1
    alone does not (the mono row is not examined; it carries the NaN as load_whisper_audio's does). The class bits are
    _normalise's: NaN makes the peak NaN (class 0), Inf and 1e39 exceed 2^15 (class 2)."""
    src, mono, flags = launch(engine, nonfinite_files)
    assert flags.tolist() == [4, 6, 6, 0, 0]
    check_against_host(nonfinite_files, src, mono, flags)
    assert np.isnan(mono[3]).any() and np.isfinite(src[3]).all()


def test_load_batch_raises_for_the_bad_file_only(engine, nonfinite_files, tmp_path):
    paths = []
    for k, data in enumerate(nonfinite_files):
        paths.append(str(tmp_path / f"file{k}.wav"))
        open(paths[-1], "wb").write(data)
    with pytest.raises(A.AudioError, match="file0.wav: non-finite samples"):
        A.load_batch(paths, FS, engine)
    with pytest.raises(A.AudioError, match="file2.wav: non-finite samples"):
        A.load_batch(paths[2:], FS, engine)
    short = str(tmp_path / "short.wav")
    open(short, "wb").write(wav_bytes(S16, np.zeros((2, 1), np.int64), 44100))
    with pytest.raises(A.AudioError, match="short.wav: 2 samples"):
        A.load_batch([paths[4], short], FS, engine)
    w24, w16, errors = A.load_batch(paths + [short], FS, engine, on_error="return")
    assert sorted(errors) == [0, 1, 2, 5] and all(isinstance(v, A.AudioError) for v in errors.values())
    good24, good16 = A.load_batch(paths[3:5], FS, engine)  # the others alone: the same results
    for k, j in ((3, 0), (4, 1)):
        ref_src, ref_mono, _, _ = host_path(nonfinite_files[k])
        assert same(w24[k].cpu().numpy(), ref_src) and same(w16[k].cpu().numpy(), ref_mono), k
        assert torch.equal(w24[k], good24[j]) and same(w16[k].cpu().numpy(), good16[j].cpu().numpy()), k
    assert all(w24[k] is None and w16[k] is None for k in errors)
    (b24,), (b16,) = A.load_batch([nonfinite_files[4]], FS, engine)  # bytes in place of a path
    assert torch.equal(b24, good24[1]) and torch.equal(b16, good16[1])


def test_mono_rows_are_quantised_also_at_16k(engine):
    """F32 samples off the int16 grid, one file already at 16 kHz: its mono row equals load_whisper_audio's, lies on
    the grid and so is not a copy of the decoded samples (it went through the up = down = 1 filter and the rounding);
    its 24 kHz source row is filtered, its 16 kHz 'source' row with sr_src = 16000 is the samples themselves."""
    rng = np.random.default_rng(4)
    x = random_samples(rng, F32, 1200, 1)
    files = [wav_bytes(F32, x, SR16), wav_bytes(F32, random_samples(rng, F32, 900, 2), 44100)]
    src, mono, flags = launch(engine, files)
    check_against_host(files, src, mono, flags)
    for row in mono:
        assert np.array_equal(row * 32768.0, np.round(row * 32768.0))
    assert len(mono[0]) == 1200 and not np.array_equal(mono[0], x[:, 0])
    assert np.max(np.abs(mono[0] - x[:, 0])) <= 0.5 / 32768.0 + 1e-7
    copy, _, _ = launch(engine, files[:1], sr_src=SR16, want_mono=False)
    assert same(copy[0], x[:, 0])


def count_launches(fn):
    _lib.profile_filter("load_pcm")
    _lib.profile_enable(True)
    try:
        fn()
        stats = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
        _lib.profile_filter("")
    assert stats and all(k.startswith("load_pcm") for k in stats), stats
    return {k: v["launches"] for k, v in stats.items()}


def test_launch_count_does_not_grow_with_the_batch(engine, ragged_files):
    """At most three launches per call (peak, source, mono) for B = 5 as for B = 1; two when no utterance holds floats."""
    five = count_launches(lambda: launch(engine, ragged_files))
    one = count_launches(lambda: launch(engine, ragged_files[2:3]))
    ints = count_launches(lambda: launch(engine, [ragged_files[0], ragged_files[1], ragged_files[3]]))
    assert sum(five.values()) == sum(one.values()) == 3 and five == one, (five, one)
    assert sum(ints.values()) == 2 and not any("peak" in k for k in ints), ints


@pytest.fixture(scope="module")
def tiny():
    cfg = C.load_config()
    e = I.build_engine(cfg, 0, random_weights="tiny-test", seed=0)
    yield cfg, e
    e.close()


def test_through_the_layers(tiny, tmp_path):
    """The golden clip and a shortened copy: SVCPipeline.convert_files equals infer.convert_files, and both equal the
    per-file loaders followed by convert_many (what the CLI did before); SVCServer.submit_file on the file's bytes
    equals convert_file for the same utterance id, and a bad file in the same queue fails its own future only."""
    cfg, e = tiny
    with wave.open(CLIP, "rb") as f:
        params, pcm = f.getparams(), f.readframes(f.getnframes())
    short = str(tmp_path / "short.wav")
    with wave.open(short, "wb") as f:
        f.setparams(params)
        f.writeframes(pcm[:len(pcm) * 3 // 5 // 2 * 2])
    kw = dict(fast_inference=True, speedup=250, seed=0)
    sid = int(C.load_singers(cfg)["svcc_CDF1"])
    pipe = SVCPipeline(e)
    got = pipe.convert_files([CLIP, short], [sid, sid], pcm16=True, **kw)
    cli = I.convert_files(e, cfg, [CLIP, short], "svcc_CDF1", pcm16=True, **kw)
    w24 = [A.load_audio(p, cfg.fs) for p in (CLIP, short)]
    w16 = [A.load_whisper_audio(p) for p in (CLIP, short)]
    before = pipe.convert_many(w24, w16, [sid, sid], pcm16=True, **kw)
    for k in range(2):
        assert got[k].dtype == torch.int16 and cli[k][0].dtype == np.int16
        assert np.array_equal(got[k].cpu().numpy(), cli[k][0]), k
        assert np.array_equal(cli[k][0], before[k].cpu().numpy()), k
    assert cli[0][1] == 379
    one, T = I.convert_file(e, cfg, CLIP, "svcc_CDF1", pcm16=True, **kw)
    nan = np.zeros((500, 1), np.float32)
    nan[3] = np.nan
    with SVCServer(pipe, max_batch=4, max_wait_s=0.0, pcm16=True, **kw) as server:
        bad = server.submit_file(wav_bytes(F32, nan, 44100), sid)
        fut = server.submit_file(open(CLIP, "rb").read(), sid, utt_id=0)
        served = fut.result(timeout=120)
        assert isinstance(bad.exception(timeout=120), A.AudioError)
    assert T == 379 and served.dtype == torch.int16 and np.array_equal(served.cpu().numpy(), one)
