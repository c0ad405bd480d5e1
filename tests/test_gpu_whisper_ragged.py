"""GPU: ragged Whisper batches window by window in one pass (svc_whisper_content_ragged; include/svc_hip.h "Ragged
batches", DESIGN.md "A5-A7 for ragged batches"). Every utterance of a padded batch is compared with torch.equal against
the two-group path (SVCPipeline(whisper_ragged=False).whisper_content: svc_whisper_encode + svc_map_content) run on
that clip alone; the rows past its frames are zeros, the columns beside its own are untouched, and the padding the
caller leaves in the batch (NaN here) is never read. The clips sit on the window rule's edges: one short clip, the last
single-window length (trimmed at 30 s), the first two-window length, a last window exactly full, one sample in a third
window, and a window that holds no samples at all. tiny-test Whisper dims (n_ctx 1500, D 128, 2 layers)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import dev, ptr, rel_l2, stream  # noqa: E402
from oracle import noise as ON  # noqa: E402
from oracle import pipeline as OP  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline, WHISPER_WINDOW, WINDOW_MEL_FRAMES  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine, mel_frames  # noqa: E402

TINY = W.WHISPER_DIMS["tiny-test"]
D = TINY["n_audio_state"]
NAN = float("nan")
# (frames, 16 kHz samples)
EDGES = [(20, 3414), (2812, 480085), (2813, 480086), (5610, 957440), (5611, 957441), (2900, 400000)]
EDGE_WINDOWS = [1, 1, 2, 2, 3, 2]


@pytest.fixture(scope="module")
def cfg():
    c = C.load_config()
    c.mapper.input_content_dim["whisper"] = D
    return c


@pytest.fixture(scope="module")
def wstate():
    return W.make_whisper_state(TINY, 0)


@pytest.fixture(scope="module")
def engine(cfg, wstate):
    e = SVCEngine(cfg, 0, whisper_state=wstate)
    yield e
    e.close()


_CLIPS = {}


def _clip(i, n):
    """int16-quantised 16 kHz clip of exactly n samples, made once per (seed, length) and shared"""
    if (i, n) not in _CLIPS:
        w = ON.synth_clip_16k_quantised(40 + i, n / 16000.0 + 0.01)[:n]
        assert w.shape == (n,)
        _CLIPS[(i, n)] = w
    return _CLIPS[(i, n)]


def _windows(wav, frames):
    """the zero-padded windows the two-group path encodes for one clip (host arrays)"""
    n_win = 1 if frames <= 2812 else -(-frames // WINDOW_MEL_FRAMES)
    if n_win == 1:
        return [wav[:480000]]
    out = []
    for w in range(n_win):
        buf = np.zeros(WHISPER_WINDOW, np.float32)
        part = wav[w * WHISPER_WINDOW:(w + 1) * WHISPER_WINDOW]
        buf[:len(part)] = part
        out.append(buf)
    return out


def _check_edges(e, cases, windows, feats_too):
    clips = [_clip(i, n) for i, (_, n) in enumerate(cases)]
    frames = [t for t, _ in cases]
    ns = [n for _, n in cases]
    B, T = len(cases), max(frames)
    assert [e.whisper_windows(t) for t in frames] == windows
    big = torch.full((B, max(ns)), NAN)
    for i, w in enumerate(clips):
        big[i, :ns[i]] = torch.from_numpy(w)
    buf = torch.full((B, T, D + 16), 7.0, device="cuda", dtype=e.content_dtype)
    res = e.whisper_content(big.cuda(), ns, frames, T, out=buf[:, :, 8:8 + D], return_feats=feats_too)
    torch.cuda.synchronize()
    o = buf.cpu()
    assert bool(torch.isfinite(o.float()).all())
    assert bool((o[:, :, :8] == 7.0).all()) and bool((o[:, :, 8 + D:] == 7.0).all())
    old = SVCPipeline(e, whisper_ragged=False)
    assert not old.whisper_ragged
    for i, (t, n) in enumerate(cases):
        one = old.whisper_content(dev(clips[i][None]), t)[0].cpu()
        assert one.shape == (t, D)
        assert torch.equal(o[i, :t, 8:8 + D], one), (i, t, n)
        assert not o[i, t:, 8:8 + D].float().any(), (i, t, n)
    if feats_too:
        feats = res[1].cpu()
        assert feats.shape == (sum(windows), TINY["n_audio_ctx"], D) and bool(torch.isfinite(feats).all())
        k = 0
        for i, (t, n) in enumerate(cases):
            for w, win in enumerate(_windows(clips[i], t)):
                assert torch.equal(feats[k], e.whisper_encode(dev(win[None]))[0].cpu()), (i, w)
                k += 1
        assert k == sum(windows)


def test_edges_bit_for_bit(engine):
    assert sum(EDGE_WINDOWS) == 11
    _check_edges(engine, EDGES, EDGE_WINDOWS, feats_too=True)


def test_edges_bf16_operands(cfg, wstate):
    e = SVCEngine(cfg, 0, whisper_state=wstate, operands="bf16")
    try:
        assert e.content_dtype == torch.bfloat16
        _check_edges(e, [EDGES[0], EDGES[2], EDGES[5]], [1, 2, 2], feats_too=False)
    finally:
        e.close()


def test_two_windows_against_the_oracle(engine, wstate):
    """the bound tests/test_gpu_long.py holds this encoder to, per window"""
    t, n = EDGES[2]
    wav = _clip(2, n)
    got = engine.whisper_content(dev(wav[None]), [n], [t], t)[0].float().cpu().numpy()
    ref = OP.whisper_content(wstate, wav, t)
    assert got.shape == ref.shape == (t, D)
    for c in range(2):
        sl = slice(c * WINDOW_MEL_FRAMES, min(t, (c + 1) * WINDOW_MEL_FRAMES))
        err = rel_l2(got[sl], ref[sl])
        print(f"window {c}: rel-L2 {err:.2e}")
        assert err < 5e-3, (c, err)


def test_bad_tables_are_rejected_before_any_launch(engine):
    w = torch.zeros(3, 16000, device="cuda")
    with pytest.raises(_lib.SVCError, match="utterance 1"):
        engine.whisper_content(w, [16000] * 3, [94, 0, 94], 94)
    with pytest.raises(_lib.SVCError, match="utterance 2"):
        engine.whisper_content(w, [16000] * 3, [94, 94, 95], 94)
    with pytest.raises(_lib.SVCError, match="utterance 0"):
        engine.whisper_content(w, [16001, 16000, 16000], [94] * 3, 94)
    out = torch.empty(3, 94, D, device="cuda", dtype=torch.float16)
    with pytest.raises(_lib.SVCError, match="ld_out"):
        _lib.call("svc_whisper_content_ragged", engine._ctx, ptr(w), 3, 16000, None, 94, None, ptr(out), D - 1, None,
                  stream())
    torch.cuda.synchronize()


def test_null_tables_are_the_uniform_batch(engine):
    T, n = 94, 16000
    w = dev(np.stack([_clip(10 + b, n) for b in range(2)]))
    feats = engine.whisper_encode(w)
    plain = engine.map_content(feats, T)
    a, fa = engine.whisper_content(w, None, None, T, return_feats=True)
    b = engine.whisper_content(w, [n, n], [T, T], T)
    assert torch.equal(a, b) and torch.equal(a, plain)
    # svc_whisper_encode on a clip is still one window of the ragged call
    assert torch.equal(fa, feats)
    assert torch.equal(fa[1], engine.whisper_encode(w[1:2].contiguous())[0])
    raw = torch.empty(2, T, D, device="cuda", dtype=torch.float16)
    _lib.call("svc_whisper_content_ragged", engine._ctx, ptr(w), 2, n, None, T, None, ptr(raw), D, None, stream())
    assert torch.equal(raw, plain)


class _Recording:
    """an engine that counts the content-encoder calls it passes on"""

    def __init__(self, engine):
        self._e = engine
        self.counts = {"whisper_content": 0, "whisper_encode": 0}

    def __getattr__(self, name):
        v = getattr(self._e, name)
        if name in self.counts:
            def counted(*a, **k):
                self.counts[name] += 1
                return v(*a, **k)
            return counted
        return v


def test_pipeline_ragged_one_call(cfg, wstate):
    """a one-window clip beside a two-window clip: the same waveforms from both forms"""
    e = SVCEngine(cfg, 0, whisper_state=wstate, mapper_state=W.make_mapper_state(cfg.mapper, 0),
                  vocoder_state=W.make_vocoder_state(cfg.vocoder, 0))
    try:
        secs = [1.0, 2.0, 30.2]
        w24 = [dev(ON.synth_clip(70 + i, s, 24000)) for i, s in enumerate(secs)]
        w16 = [dev(ON.synth_clip_16k_quantised(70 + i, s)) for i, s in enumerate(secs)]
        assert [e.whisper_windows(mel_frames(int(w.shape[0]))) for w in w24] == [1, 1, 2]
        rec = _Recording(e)
        new = SVCPipeline(rec)
        assert new.whisper_ragged
        a = new.convert_ragged(w24, w16, [1, 0, 2], speedup=250, seed=3)
        assert rec.counts == {"whisper_content": 1, "whisper_encode": 0}
        b = SVCPipeline(e, whisper_ragged=False).convert_ragged(w24, w16, [1, 0, 2], speedup=250, seed=3)
        for i in range(3):
            assert a[i].shape[0] == mel_frames(int(w24[i].shape[0])) * cfg.hop_length
            assert torch.equal(a[i], b[i]), i
    finally:
        e.close()
