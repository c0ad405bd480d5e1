"""A16 on the GPU: svc_pcm16 (save_audio's sample conversion, utils/util.py:20-37) against the host path.

The expected value everywhere is audio.to_pcm16 applied on the host to each utterance's own samples, and every
comparison is exact (np.array_equal): the kernels restate its arithmetic (f64 division rounded to f32, f32 product,
round half to even, clip), so there is no tolerance to choose. Every op-level case pre-fills the output with a sentinel,
one guard row after the last row included, and checks whole rows [silence | samples | silence | zeros] and the guard.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import dev, ptr, stream  # noqa: E402
from oracle import noise as ON  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import audio as A  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import infer as I  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402
from svc_inference_pipeline_amd.serving import SVCServer  # noqa: E402

SENTINEL = 0x5A5A
CLIP = os.path.join(os.path.dirname(__file__), "golden", "test_set_1100000814.wav")


@pytest.fixture(scope="module")
def engine():
    """A context without weights: svc_pcm16 needs none."""
    e = SVCEngine(C.load_config(), 0)
    yield e
    e.close()


def launch(e, x, lens, fs, add_silence, turn_up, volume_peak=0.9, wav_off=0, pcm_off=0):
    """Enqueue one svc_pcm16 call on x f32 [B, S] (host) with its own sentinel-filled buffers; wav_off / pcm_off shift
    the base pointers by that many elements (misaligned views). Returns the handles collect() reads."""
    B, S = x.shape
    L = int(_lib.load().svc_pcm16_len(S, fs, 1 if add_silence else 0))
    wbuf = torch.full((wav_off + B * S,), 7.0, dtype=torch.float32)
    wbuf[wav_off:] = torch.from_numpy(np.ascontiguousarray(x)).reshape(-1)
    wbuf = wbuf.cuda()
    pbuf = torch.full((pcm_off + (B + 1) * L,), SENTINEL, dtype=torch.int16, device="cuda")
    peak = torch.full((B,), -1.0, dtype=torch.float32, device="cuda")
    table = None if lens is None else (ctypes.c_int64 * B)(*[int(v) for v in lens])
    _lib.call("svc_pcm16", e._ctx, ctypes.c_void_p(wbuf.data_ptr() + 4 * wav_off), B, S, table, fs,
              1 if add_silence else 0, 1 if turn_up else 0, float(volume_peak),
              ctypes.c_void_p(pbuf.data_ptr() + 2 * pcm_off), ptr(peak), stream())
    return wbuf, pbuf, peak, (B, L, pcm_off)


def collect(handles):
    """-> (pcm int16 [B, L], peaks f32 [B]) once the stream has drained; the sentinels around the rows are asserted."""
    _, pbuf, peak, (B, L, pcm_off) = handles
    torch.cuda.synchronize()
    flat = pbuf.cpu().numpy()
    assert np.all(flat[:pcm_off] == SENTINEL), "samples before the first row were written"
    assert np.all(flat[pcm_off + B * L:] == SENTINEL), "the guard row after the last row was written"
    return flat[pcm_off:pcm_off + B * L].reshape(B, L), peak.cpu().numpy()


def expected(x, lens, fs, add_silence, turn_up, volume_peak=0.9):
    """Rows [sil zeros | to_pcm16(x[b, :n_b], add_silence=False) | zeros] and the peaks; a silent or empty utterance
    (where to_pcm16 raises) is a row of zeros with peak 0."""
    B, S = x.shape
    lens = [S] * B if lens is None else lens
    sil = fs // 20 if add_silence else 0
    rows = np.zeros((B, S + 2 * sil), dtype=np.int16)
    peaks = np.zeros(B, dtype=np.float32)
    for b, n in enumerate(lens):
        xb = x[b, :n]
        if n:
            peaks[b] = np.max(np.abs(xb))
        if n and (peaks[b] > 0 or not turn_up):
            rows[b, sil:sil + n] = A.to_pcm16(xb, fs, add_silence=False, turn_up=turn_up, volume_peak=volume_peak)
    return rows, peaks


def check(e, x, lens, fs, add_silence, turn_up, volume_peak=0.9, **off):
    pcm, peaks = collect(launch(e, x, lens, fs, add_silence, turn_up, volume_peak, **off))
    rows, ref_peaks = expected(x, lens, fs, add_silence, turn_up, volume_peak)
    assert pcm.shape == rows.shape
    for b in range(x.shape[0]):
        assert np.array_equal(pcm[b], rows[b]), (b, int(np.argmax(pcm[b] != rows[b])))
    assert np.array_equal(peaks, ref_peaks)
    return pcm, peaks


@pytest.mark.parametrize("fs", [100, 24000])
@pytest.mark.parametrize("add_silence,turn_up", [(a, t) for a in (False, True) for t in (False, True)])
def test_ragged_odd_strides(engine, fs, add_silence, turn_up):
    """B = 3, S = 1031, lengths [1031, 257, 1]: odd row strides on both sides (sil = 5 at fs = 100), rows past n_b
    hold 100.0, which a peak pass that read the padding would pick up."""
    S, lens = 1031, [1031, 257, 1]
    x = (np.random.default_rng(11).standard_normal((3, S)) * 0.2).astype(np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = 100.0
    check(engine, x, lens, fs, add_silence, turn_up)


def test_rounding_and_clipping(engine):
    """turn_up=False: the ties (k + 0.5) / 32768 go to the even neighbour, +-1.0, +-1.5 and the two values half a step
    inside / outside the int16 range clip."""
    ties = [(k + 0.5) / 32768.0 for k in range(-40, 41)]
    edge = [1.0, -1.0, 1.5, -1.5, 32767.5 / 32768.0, -32768.5 / 32768.0]
    x = np.array([ties + edge], dtype=np.float32)
    assert np.array_equal(x.astype(np.float64), np.array([ties + edge]))  # all exact in f32
    pcm, _ = check(engine, x, None, 24000, False, False)
    got = dict(zip(ties + edge, pcm[0].tolist()))
    assert got[0.5 / 32768.0] == 0 and got[1.5 / 32768.0] == 2 and got[2.5 / 32768.0] == 2
    assert got[-0.5 / 32768.0] == 0 and got[-1.5 / 32768.0] == -2 and got[-39.5 / 32768.0] == -40
    assert got[1.0] == 32767 and got[-1.0] == -32768 and got[1.5] == 32767 and got[-1.5] == -32768
    assert got[32767.5 / 32768.0] == 32767 and got[-32768.5 / 32768.0] == -32768
    check(engine, x, None, 100, True, False)  # the same samples behind 5 zeros: another store alignment


@pytest.mark.parametrize("where", ["first", "last", "negative"])
def test_peak_placement_and_misaligned_bases(engine, where):
    """B = 2, S = 70001, lengths [70001, 65537]: several peak blocks per row, the peak in the first sample, in the
    last sample of the utterance, or negative; wav offset by one float and pcm by one int16, so neither base is
    16-byte aligned (and the rows' strides are odd)."""
    S, lens = 70001, [70001, 65537]
    x = (np.random.default_rng(5).uniform(-0.3, 0.3, (2, S))).astype(np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = 100.0
        if where == "first":
            x[b, 0] = 0.71 + 0.01 * b
        elif where == "last":
            x[b, n - 1] = 0.66 + 0.01 * b
        else:
            x[b, n // 2 + 3] = -0.83 - 0.01 * b
    _, peaks = check(engine, x, lens, 24000, True, True, wav_off=1, pcm_off=1)
    assert np.all(peaks > 0.6)


def test_no_state_between_calls(engine):
    """Two calls back to back on one stream and one context, loud then quiet: the second call's peaks start from
    zero again (its own staged scratch), so it equals its own host result."""
    rng = np.random.default_rng(3)
    loud = (rng.uniform(-0.9, 0.9, (2, 5000))).astype(np.float32)
    quiet = (rng.uniform(-0.01, 0.01, (2, 5000))).astype(np.float32)
    h1 = launch(engine, loud, [5000, 4097], 24000, True, True)
    h2 = launch(engine, quiet, [4999, 5000], 24000, True, True)
    for h, x, lens in ((h1, loud, [5000, 4097]), (h2, quiet, [4999, 5000])):
        pcm, peaks = collect(h)
        rows, ref_peaks = expected(x, lens, 24000, True, True)
        assert np.array_equal(pcm, rows) and np.array_equal(peaks, ref_peaks)
    assert peaks.max() <= 0.01


def test_silent_and_empty_utterances(engine):
    """An all-zero utterance and one of zero samples beside a normal one: their rows are zeros and their peaks 0 (the
    host function divides by zero there), the normal row is unaffected."""
    S = 3001
    x = np.zeros((3, S), dtype=np.float32)
    x[1] = 100.0  # n_b = 0: nothing of this row may be read
    x[2] = (np.random.default_rng(2).standard_normal(S) * 0.1).astype(np.float32)
    lens = [S, 0, 2900]
    x[2, 2900:] = 100.0
    for turn_up in (True, False):
        pcm, peaks = check(engine, x, lens, 24000, True, turn_up)
        assert not pcm[0].any() and not pcm[1].any() and pcm[2].any()
        assert peaks[0] == 0 and peaks[1] == 0 and peaks[2] > 0
    pcm, _ = check(engine, x, lens, 24000, True, True)
    alone = A.to_pcm16(x[2, :2900], 24000)  # silence included: the row's first 1200 + 2900 + 1200 samples
    assert np.array_equal(pcm[2, :len(alone)], alone) and not pcm[2, len(alone):].any()


def test_argument_errors(engine):
    x = dev(np.random.default_rng(0).uniform(-0.5, 0.5, (2, 640)).astype(np.float32))
    with pytest.raises(_lib.SVCError, match="utterance 1"):
        engine.pcm16(x, n_samples=[640, 641])
    with pytest.raises(_lib.SVCError, match="utterance 0"):
        engine.pcm16(x, n_samples=[-1, 640])
    with pytest.raises(_lib.SVCError, match="volume_peak"):
        engine.pcm16(x, volume_peak=0.0)
    pcm, peak = engine.pcm16(x, n_samples=[640, 300], return_peak=True)  # the engine still works
    assert pcm.dtype == torch.int16 and pcm.shape == (2, 640 + 2400)
    xs = x.cpu().numpy()
    assert np.array_equal(pcm[0].cpu().numpy(), A.to_pcm16(xs[0], 24000))
    assert np.array_equal(pcm[1, :300 + 2400].cpu().numpy(), A.to_pcm16(xs[1, :300], 24000))
    assert not pcm[1, 300 + 2400:].any()
    assert np.array_equal(peak.cpu().numpy(), np.array([np.abs(xs[0]).max(), np.abs(xs[1, :300]).max()], np.float32))
    quiet = engine.pcm16(x, volume_peak=0.0, turn_up=False, add_silence=False)  # volume_peak is unused without turn_up
    assert np.array_equal(quiet[0].cpu().numpy(), A.to_pcm16(xs[0], 24000, add_silence=False, turn_up=False))


@pytest.fixture(scope="module")
def tiny():
    cfg = C.load_config()
    e = I.build_engine(cfg, 0, random_weights="tiny-test", seed=0)  # the CLI's --random-weights tiny-test engine
    yield cfg, e
    e.close()


def test_pipeline_pcm16(tiny):
    """convert / convert_ragged / SVCServer with pcm16=True return to_pcm16 of their own f32 result; with the default
    they return what they returned before (no pcm, the f32 views)."""
    cfg, e = tiny
    pipe = SVCPipeline(e)
    secs = [1.0, 0.6]
    w24 = [dev(ON.synth_clip(80 + i, s, 24000)) for i, s in enumerate(secs)]
    w16 = [dev(ON.synth_clip_16k_quantised(80 + i, s)) for i, s in enumerate(secs)]
    kw = dict(fast_inference=True, speedup=250, seed=4)
    for i in range(2):
        one = dict(utt_ids=dev(np.array([i]), torch.int32), **kw)
        res = pipe.convert(w24[i][None], w16[i][None], dev(np.array([i]), torch.int32), pcm16=True, **one)
        assert res.pcm.dtype == torch.int16 and res.pcm.shape == (1, res.wav.shape[1] + 2 * (cfg.fs // 20))
        assert np.array_equal(res.pcm[0].cpu().numpy(), A.to_pcm16(res.wav[0].cpu().numpy(), cfg.fs))
        plain = pipe.convert(w24[i][None], w16[i][None], dev(np.array([i]), torch.int32), **one)
        assert plain.pcm is None and torch.equal(plain.wav, res.wav)
    f32 = pipe.convert_ragged(w24, w16, [0, 1], **kw)
    pcm = pipe.convert_ragged(w24, w16, [0, 1], pcm16=True, **kw)
    hop = cfg.hop_length
    for i in range(2):
        T = (len(w24[i]) + 768 - 1024) // 256 + 1
        assert f32[i].dtype == torch.float32 and f32[i].shape == (T * hop,)
        assert pcm[i].dtype == torch.int16 and pcm[i].shape == (T * hop + 2 * (cfg.fs // 20),)
        assert np.array_equal(pcm[i].cpu().numpy(), A.to_pcm16(f32[i].cpu().numpy(), cfg.fs)), i
    many = pipe.convert_many(w24, w16, [0, 1], bucketed=True, pcm16=True, **kw)
    for i in range(2):
        assert torch.equal(many[i], pcm[i]), i
    for flag, want in ((True, pcm), (False, f32)):
        with SVCServer(pipe, max_batch=2, max_wait_s=0.0, **(dict(pcm16=True) if flag else {}), **kw) as server:
            futs = [server.submit(w24[i], w16[i], i) for i in range(2)]
            got = [f.result(timeout=120) for f in futs]
        for i in range(2):
            assert got[i].dtype == want[i].dtype and torch.equal(got[i], want[i]), (flag, i)


def test_cli_writes_the_same_file(tiny, tmp_path):
    """The CLI converts on the GPU and writes the samples itself: the file is byte-identical to audio.save_audio of
    convert_file's f32 waveform for the same arguments."""
    cfg, e = tiny
    out = str(tmp_path / "gen" / "cli.wav")
    assert I.main(["--wav", CLIP, "--singer", "svcc_CDF1", "--out", out, "--random-weights", "tiny-test", "--fast",
                   "--speedup", "250"]) == 0
    wav, _ = I.convert_file(e, cfg, CLIP, "svcc_CDF1", fast_inference=True, speedup=250, seed=0)
    assert wav.dtype == np.float32
    ref = str(tmp_path / "ref.wav")
    A.save_audio(ref, wav, cfg.fs)
    assert open(out, "rb").read() == open(ref, "rb").read()
