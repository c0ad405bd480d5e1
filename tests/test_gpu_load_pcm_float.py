"""A1 on the GPU with HuBERT / ContentVec's input: svc_load_pcm_ex (wav payloads of a ragged batch -> the source rows, the
16 kHz int16-grid mono rows and the 16 kHz FLOAT mono rows) against the per-file host path.

The yardstick is the per-file path on the same bytes written to a file of their own: audio.load_audio,
audio.load_whisper_audio and audio.load_contentvec_audio for that file alone, compared exactly (np.array_equal): the
kernel restates that path's arithmetic, so there is no tolerance to choose. In addition the float rows are held to
read_wav, the f64 channel mean and scipy.signal.resample_poly in f64 within test_gpu_audio.py's bound,
2e-7 * max(max |ref|, 1e-3) + 1e-9 (the same filter and f32 output as the source rows it governs in
test_gpu_load_pcm.py). Every op-level call pre-fills its outputs with a sentinel, some floats before the first row and
one guard row after the last included, and checks them, the zero tails and the sentinels around the rows; payloads sit
at odd byte offsets.

Sizes: a workgroup owns 1024 output samples of a row (load_pcm.hip kChunk); rows here end one short of, on and one past
that count, and one case uses 384 kHz input, at which a workgroup walks its samples in several LDS tiles."""
import ctypes
import functools
import itertools
import os
import tempfile

import numpy as np
import pytest
import scipy.signal as ss
import torch

pytestmark = pytest.mark.gpu

from gpu_util import ptr, stream  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import audio as A  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402
from wav_util import F32, F64, S16, S24, S32, U8, random_samples, wav_bytes  # noqa: E402

SENTINEL = 7.5
PRE = 5  # sentinel floats in front of the first row (the rows then start off any 16-byte boundary)
FS, SR16 = 24000, 16000
ALL = ("src", "mono", "float")


@pytest.fixture(scope="module")
def engine():
    """A context without weights: the load stage needs none."""
    e = SVCEngine(C.load_config(), 0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def host_path(data):
    """The per-file path on these bytes alone -> (load_audio's row or None, load_whisper_audio's row,
    load_contentvec_audio's row, read_wav's f64 samples, rate); computed once per file and shared."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.wav")
        with open(path, "wb") as fh:
            fh.write(data)
        with np.errstate(all="ignore"):
            src = A.load_audio(path, FS)
            mono = A.load_whisper_audio(path)
            flt = A.load_contentvec_audio(path)
            x, sr = A.read_wav(path)
    return (None if src is None else src.cpu().numpy()), mono.cpu().numpy(), flt.cpu().numpy(), x, sr


def odd_offsets(infos, first=1):
    offsets, pos = [], first
    for i in infos:
        offsets.append(pos)
        pos += len(i.payload) + 1
        pos += 1 - pos % 2  # keep the next start odd
    assert all(o % 2 == 1 for o in offsets)
    return offsets


def launch(e, files, want=ALL, offsets=None):
    """One svc_load_pcm_ex call on whole wav files (bytes): their payloads go into one device buffer at odd byte
    offsets between 0xA5 filler bytes. -> ({"src" | "mono" | "float": the rows asked for}, info)"""
    infos = [A.parse_wav(f) for f in files]
    B = len(infos)
    offsets = odd_offsets(infos) if offsets is None else offsets
    total = max(o + len(i.payload) for o, i in zip(offsets, infos)) + 3
    host = np.full(total, 0xA5, dtype=np.uint8)
    for o, i in zip(offsets, infos):
        host[o:o + len(i.payload)] = np.frombuffer(i.payload, dtype=np.uint8)
    raw = torch.from_numpy(host).cuda()
    lib = _lib.load()
    n = {"src": [int(lib.svc_resample_len(i.n_frames, i.sr, FS)) for i in infos],
         "mono": [int(lib.svc_resample_len(i.n_frames, i.sr, SR16)) for i in infos]}
    n["float"] = n["mono"]
    S = {"src": max(1, max(n["src"])) + 3, "mono": max(1, max(n["mono"])) + 2}  # longer than the longest utterance
    S["float"] = S["mono"]
    bufs = {k: torch.full((PRE + (B + 1) * S[k],), SENTINEL, device="cuda") if k in want else None for k in ALL}
    info = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
    i64, i32 = ctypes.c_int64 * B, ctypes.c_int32 * B
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * PRE) if t is not None else None  # noqa: E731
    _lib.call("svc_load_pcm_ex", e._ctx, ptr(raw), B, i64(*offsets), i64(*[i.n_frames for i in infos]),
              i32(*[i.format for i in infos]), i32(*[i.channels for i in infos]), i32(*[i.sr for i in infos]),
              FS, S["src"], off(bufs["src"]), SR16, S["mono"], off(bufs["mono"]), off(bufs["float"]), ptr(info),
              stream())
    torch.cuda.synchronize()
    rows = {}
    for k in want:
        flat = bufs[k].cpu().numpy()
        assert np.all(flat[:PRE] == SENTINEL), (k, "floats before the first row were written")
        assert np.all(flat[PRE + B * S[k]:] == SENTINEL), (k, "the guard row after the last row was written")
        y = flat[PRE:PRE + B * S[k]].reshape(B, S[k])
        for b in range(B):
            assert not y[b, n[k][b]:].any(), f"{k} row {b}: the tail past its {n[k][b]} samples is not zero"
        rows[k] = [y[b, :n[k][b]] for b in range(B)]
    flags = info.cpu().numpy()
    assert flags[B] == -1
    return rows, flags[:B]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def check_against_host(files, rows):
    """Every row that was asked for against the per-file path (exact); the float rows also against f64 scipy."""
    for b, data in enumerate(files):
        ref_src, ref_mono, ref_float, x, sr = host_path(data)
        if "src" in rows and ref_src is not None:
            assert same(rows["src"][b], ref_src), (b, "source")
        if "mono" in rows:
            assert same(rows["mono"][b], ref_mono), (b, "mono")
        if "float" in rows:
            got = rows["float"][b]
            assert same(got, ref_float), (b, "float", int(np.argmax(got != ref_float)))
            if np.isfinite(x).all():
                m = x.mean(axis=1)
                ref = m if sr == SR16 else ss.resample_poly(m, SR16, sr)
                err, bound = np.max(np.abs(got - ref)), 2e-7 * max(np.max(np.abs(ref)), 1e-3) + 1e-9
                print(f"file {b}: float row max |err| {err:.3e} against f64 scipy, bound {bound:.3e}")
                assert err <= bound, (b, "scipy", err, bound)


FORMAT_CASES = [(f, c) for f in (U8, S16, S24, S32, F32, F64) for c in (1, 2, 3)] + [(F64, 7), (F64, 8), (S16, 8)]


@pytest.mark.parametrize("fmt,ch", FORMAT_CASES)
def test_formats_and_channel_counts(engine, fmt, ch):
    """257 frames at 24 kHz: the float row is the channel mean through the 24 -> 16 kHz filter, unrounded; 7 and 8
    channels pin numpy's summation order. The other two rows are what they were."""
    data = wav_bytes(fmt, random_samples(np.random.default_rng(100 * fmt + ch), fmt, 257, ch), FS)
    rows, flags = launch(engine, [data])
    assert flags[0] == 0 and len(rows["float"][0]) == len(rows["mono"][0]) == 172
    check_against_host([data], rows)


SPEC = [(S16, 2, 44100, 4099), (S24, 1, 48000, 1001), (F32, 3, 22050, 300), (S32, 2, 16000, 7), (F64, 1, 24000, 3)]


@pytest.fixture(scope="module")
def ragged_files():
    rng = np.random.default_rng(7)
    return [wav_bytes(f, random_samples(rng, f, n, ch), sr) for f, ch, sr, n in SPEC]


def test_ragged_mixed_rates_in_one_call(engine, ragged_files):
    """B = 5, five rates, mixed formats and channel counts, 3 to 4099 frames, every payload at an odd byte offset: every
    row is exact against the per-file path. The 16 kHz utterance takes both branches in the one kernel: its float row
    is its decoded channel mean, unfiltered, while its quantised row went through the up = down = 1 filter and lies on
    the int16 grid. Each utterance alone (B = 1) gives the same bits, and so does each of the seven non-empty subsets
    of the three outputs, with the same info."""
    infos = [A.parse_wav(f) for f in ragged_files]
    offsets = odd_offsets(infos, first=3)
    rows, flags = launch(engine, ragged_files, offsets=offsets)
    assert [len(r) for r in rows["src"]] == [2231, 501, 327, 11, 3]
    assert [len(r) for r in rows["mono"]] == [len(r) for r in rows["float"]] == [1488, 334, 218, 7, 2]
    check_against_host(ragged_files, rows)
    x, sr = host_path(ragged_files[3])[3:]
    assert sr == SR16
    assert same(rows["float"][3], x.mean(axis=1).astype(np.float32))
    q = rows["mono"][3] * 32768.0
    assert np.array_equal(q, np.round(q)) and not np.array_equal(rows["mono"][3], rows["float"][3])
    for b, data in enumerate(ragged_files):
        one, f1 = launch(engine, [data], offsets=[2 * b + 1])  # another offset, too
        assert all(same(one[k][0], rows[k][b]) for k in ALL) and f1[0] == flags[b], b
    subsets = [c for r in (1, 2, 3) for c in itertools.combinations(ALL, r)]
    assert len(subsets) == 7
    for want in subsets:
        part, f2 = launch(engine, ragged_files, want=want, offsets=offsets)
        assert sorted(part) == sorted(want) and np.array_equal(f2, flags), want
        for k in want:
            assert all(same(a, b) for a, b in zip(part[k], rows[k])), (want, k)


def frames_for(n16, sr=44100):
    """the fewest frames at `sr` whose 16 kHz row has n16 samples"""
    lib = _lib.load()
    n = n16 * sr // SR16 - 4
    while int(lib.svc_resample_len(n, sr, SR16)) < n16:
        n += 1
    assert int(lib.svc_resample_len(n, sr, SR16)) == n16
    return n


def test_rows_across_workgroup_boundaries(engine):
    """Mono S16 at 44.1 kHz whose 16 kHz rows have 1023, 1024, 1025 and 2049 samples (one short of a workgroup's 1024,
    exactly one, one past, two and one), and an F32 file already at 16 kHz with 1025 frames: an unfiltered float row
    that crosses a chunk, copied from two workgroups' tiles."""
    rng = np.random.default_rng(31)
    files = [wav_bytes(S16, random_samples(rng, S16, frames_for(n), 1), 44100) for n in (1023, 1024, 1025, 2049)]
    x = random_samples(rng, F32, 1025, 1)
    files.append(wav_bytes(F32, x, SR16))
    rows, flags = launch(engine, files)
    assert [len(r) for r in rows["float"]] == [1023, 1024, 1025, 2049, 1025] and not flags.any()
    check_against_host(files, rows)
    assert same(rows["float"][4], x[:, 0])
    only, _ = launch(engine, files, want=("float",))  # the rows at 16 kHz need no plan here: the direct copy
    assert all(same(a, b) for a, b in zip(only["float"], rows["float"]))


def test_large_rate_ratio_walks_several_tiles(engine):
    """384 kHz input: down / up is 24 for the mono rows, so a workgroup's 1024 samples are walked in tiles of 321;
    40000 and 1500 frames in one call."""
    rng = np.random.default_rng(21)
    files = [wav_bytes(S16, random_samples(rng, S16, 40000, 1), 384000),
             wav_bytes(F32, random_samples(rng, F32, 1500, 2), 384000)]
    rows, flags = launch(engine, files)
    assert [len(r) for r in rows["float"]] == [1667, 63]
    check_against_host(files, rows)


def test_empty_utterance_gives_rows_of_zeros(engine):
    """0 frames through the C entry point (load_batch refuses such a file) beside a normal utterance: its three rows
    are zeros (launch checks every sample past a row's own length), the other's rows are what they are alone."""
    rng = np.random.default_rng(5)
    empty = wav_bytes(S16, np.zeros((0, 2), np.int64), 44100)
    normal = wav_bytes(S24, random_samples(rng, S24, 1300, 2), 32000)
    assert A.parse_wav(empty).n_frames == 0
    for files, k in (([empty, normal], 1), ([normal, empty], 0)):
        rows, flags = launch(engine, files)
        assert all(len(rows[name][1 - k]) == 0 for name in ALL) and flags[1 - k] == 0
        alone, f1 = launch(engine, [normal])
        assert all(same(rows[name][k], alone[name][0]) for name in ALL) and flags[k] == f1[0]
    check_against_host([normal], alone)


def test_nan_in_channel_1_only(engine):
    """F32 stereo with a NaN in channel 1: the float row carries it (as load_contentvec_audio's does), info stays 0
    (only the source row is examined) and the source row, channel 0, is finite."""
    rng = np.random.default_rng(9)
    x = random_samples(rng, F32, 600, 2)
    x[7, 1] = np.nan
    files = [wav_bytes(F32, x, 44100), wav_bytes(F32, x, SR16)]
    rows, flags = launch(engine, files)
    assert flags.tolist() == [0, 0]
    check_against_host(files, rows)
    for b in range(2):
        assert np.isnan(rows["float"][b]).any() and np.isfinite(rows["src"][b]).all(), b
    assert np.isnan(rows["float"][1][7]) and np.isnan(rows["float"][1]).sum() == 1


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
    # (a name may carry the site label "@..." an earlier GEMM of the process left behind: it is no part of the name)
    names = [k.split("@")[0] for k in stats]
    assert len(set(names)) == len(names), stats
    return {k.split("@")[0]: v["launches"] for k, v in stats.items()}


def test_three_launches_whatever_is_asked_for(engine, ragged_files):
    """The full call makes three launches (peak, source, mono) for B = 5 as for B = 1, with the same names, and two
    when no utterance holds floats; exactly one launch writes both mono rows."""
    five = count_launches(lambda: launch(engine, ragged_files))
    one = count_launches(lambda: launch(engine, ragged_files[2:3]))
    ints = count_launches(lambda: launch(engine, [ragged_files[0], ragged_files[1], ragged_files[3]]))
    assert five == one == {"load_pcm_peak": 1, "load_pcm_src": 1, "load_pcm_mono": 1}, (five, one)
    assert ints == {"load_pcm_src": 1, "load_pcm_mono": 1}, ints
    both = count_launches(lambda: launch(engine, ragged_files, want=("mono", "float")))
    assert {k: v for k, v in both.items() if "peak" not in k} == {"load_pcm_mono": 1}, both
    flt = count_launches(lambda: launch(engine, ragged_files, want=("float",)))
    assert {k: v for k, v in flt.items() if "peak" not in k} == {"load_pcm_mono": 1}, flt
