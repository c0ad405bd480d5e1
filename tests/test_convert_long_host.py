"""CPU: the host logic of SVCPipeline.convert_long with a stand-in engine: one song-level F0 pass, the chunks of all
songs in groups of max_batch with their F0 slices and noise ids, one stitch over everything, the song-level tail."""
import contextlib
import types

import pytest
import torch

from svc_inference_pipeline_amd import audio as A
from svc_inference_pipeline_amd.pipeline import SVCPipeline
from test_pipeline_host import _FakeEngine

HOP = 256
CLIP = dict(clip_s=0.8, context_s=0.32)


class _LongEngine(_FakeEngine):
    """F0 = the frame index + 1000 * (row's first sample), shifted by +0.5; the vocoder output = the chunk's noise id."""

    def f0(self, w24, T, n_samples=None):
        self.calls.append(("f0", T, list(n_samples)))
        base = torch.arange(T, dtype=torch.float64)[None] + 1000.0 * w24[:, :1].double()
        return base.repeat(1, 1).contiguous()

    def pitch_shift(self, f0, *targets):
        self.calls.append(("shift", tuple(f0.shape)))
        f0 += 0.5
        return f0

    def condition(self, content, f0, energy, singer):
        self.calls.append(("condition", f0.clone(), singer.tolist()))
        return content[:, :, :384].float()

    def diffsvc_sample(self, cond, fast_inference=True, speedup=10, seed=0, utt_ids=None, frames=None, **kw):
        self.calls.append(("sample", tuple(cond.shape), list(frames), utt_ids.tolist()))
        x0 = torch.zeros(cond.shape[0], cond.shape[1], 100)
        x0[:, :, 0] = utt_ids.float()[:, None]
        return x0

    def stitch(self, rows, plan, out=None, return_shifts=False):
        self.calls.append(("stitch", [tuple(r.shape) for r in rows], plan))
        res, shifts = A.stitch([r.numpy() for r in rows], plan, return_shifts=True)
        out.reshape(-1).copy_(torch.from_numpy(res))
        return out, torch.from_numpy(shifts)

    def loudness_match(self, wav, src, n_samples=None, src_samples=None, mix=0.0, out=None):
        self.calls.append(("loudness", tuple(wav.shape), tuple(src.shape), list(n_samples), list(src_samples), mix))
        return out

    def pcm16(self, wav, n_samples=None):
        self.calls.append(("pcm16", tuple(wav.shape), list(n_samples)))
        return torch.zeros(wav.shape[0], wav.shape[1] + 2400, dtype=torch.int16)


@pytest.fixture
def pipe(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(wait_stream=lambda s: None))
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    return SVCPipeline(_LongEngine(), f0_side=False)


def songs(lens):
    w24 = [torch.full((n,), float(i + 1)) for i, n in enumerate(lens)]
    w16 = [torch.full((n * 2 // 3,), float(i + 1)) for i, n in enumerate(lens)]
    return w24, w16


def test_chunks_groups_f0_slices_and_noise_ids(pipe):
    eng = pipe.engine
    lens = [72000, 36000 + 77]  # 281 frames: 4 chunks; 140 frames: 2 chunks
    w24, w16 = songs(lens)
    wavs, info = pipe.convert_long(w24, w16, [3, 4], utt_ids=[5, 9], max_batch=4, return_chunks=True, **CLIP)
    kinds = [c[0] for c in eng.calls]
    assert kinds.count("f0") == 1 and kinds.count("shift") == 1 and kinds.count("stitch") == 1
    assert kinds.index("shift") < kinds.index("sample")  # the songs' F0 comes first
    assert next(c for c in eng.calls if c[0] == "f0")[1:] == (281, lens)
    plans = info.plans
    assert [p.chunks for p in plans] == [4, 2]
    samples = [c for c in eng.calls if c[0] == "sample"]
    assert [len(c[3]) for c in samples] == [4, 2]  # six chunks in groups of at most four, in song order
    assert samples[0][3] == [(5 << 12) | k for k in range(4)] and samples[1][3] == [(9 << 12) | k for k in range(2)]
    assert samples[0][2] == plans[0].frames and samples[1][2] == plans[1].frames
    conds = [c for c in eng.calls if c[0] == "condition"]
    assert conds[0][2] == [3, 3, 3, 3] and conds[1][2] == [4, 4]
    # each chunk was conditioned on its slice of the song's shifted F0, zeros past its own frames
    jobs = [(0, k) for k in range(4)] + [(1, k) for k in range(2)]
    rows = torch.cat([conds[0][1], torch.nn.functional.pad(conds[1][1], (0, conds[0][1].shape[1] - conds[1][1].shape[1]))])
    for r, (i, k) in enumerate(jobs):
        s, t = plans[i].start[k], plans[i].frames[k]
        want = torch.arange(s, s + t, dtype=torch.float64) + 1000.0 * (i + 1) + 0.5
        assert torch.equal(rows[r, :t], want) and not rows[r, t:].any()
        assert torch.equal(info.f0[i][s:s + t], want)
    # one stitch over all six chunks, rows as long as the chunks' own frames, out_off moved to each song's row
    st = next(c for c in eng.calls if c[0] == "stitch")
    assert st[1] == [(t * HOP,) for p in plans for t in p.frames]
    S = 281 * HOP
    assert st[2].out_len == 2 * S and st[2].joined == [0, 1, 1, 1, 0, 1]
    assert st[2].out_off == plans[0].stitch.out_off + [S + v for v in plans[1].stitch.out_off]
    # the songs: chunk k's noise id where chunk k's body landed (constant rows: any displacement gives the same)
    for i, (u, p) in enumerate(zip((5, 9), plans)):
        assert wavs[i].shape == (p.T_song * HOP,)
        tail = p.stitch.search - 1
        for k in range(p.chunks):
            lo = p.stitch.out_off[k] + (p.stitch.xfade if k else 0)
            assert bool((wavs[i][lo:p.stitch.out_off[k] + p.stitch.body[k]] == float((u << 12) | k)).all())
        assert not wavs[i][-tail:].any()
        assert [c.shape[0] for c in info.chunks[i]] == [t * HOP for t in p.frames]
    assert "loudness" not in kinds and "pcm16" not in kinds


def test_tail_runs_once_on_the_songs(pipe):
    eng = pipe.engine
    lens = [72000, 36077]
    w24, w16 = songs(lens)
    out = pipe.convert_long(w24, w16, [3, 4], loudness_mix=0.25, pcm16=True, max_batch=1, **CLIP)
    kinds = [c[0] for c in eng.calls]
    assert kinds.count("sample") == 6 and kinds.count("stitch") == 1
    assert kinds.count("loudness") == 1 and kinds.count("pcm16") == 1
    assert kinds.index("stitch") < kinds.index("loudness") < kinds.index("pcm16")
    loud = next(c for c in eng.calls if c[0] == "loudness")
    assert loud[1:] == ((2, 281 * HOP), (2, 72000), [281 * HOP, 140 * HOP], lens, 0.25)
    assert next(c for c in eng.calls if c[0] == "pcm16")[1:] == ((2, 281 * HOP), [281 * HOP, 140 * HOP])
    assert [o.shape[0] for o in out] == [281 * HOP + 2400, 140 * HOP + 2400] and out[0].dtype == torch.int16


def test_single_chunk_song_and_errors(pipe):
    eng = pipe.engine
    w24, w16 = songs([24000])
    wavs, info = pipe.convert_long(w24, w16, [1], utt_ids=[7], return_chunks=True, **CLIP)
    assert info.plans[0].chunks == 1
    sample = next(c for c in eng.calls if c[0] == "sample")
    assert sample[3] == [7 << 12] and wavs[0].shape == (93 * HOP,) and bool((wavs[0] == float(7 << 12)).all())
    with pytest.raises(ValueError, match="utterance id"):
        pipe.convert_long(w24, w16, [1], utt_ids=[1 << 19], **CLIP)
    with pytest.raises(ValueError, match="one entry per song"):
        pipe.convert_long(w24, [], [1], **CLIP)
    with pytest.raises(ValueError, match="max_batch"):
        pipe.convert_long(w24, w16, [1], max_batch=0, **CLIP)
    with pytest.raises(ValueError, match="right context"):
        pipe.convert_long(w24, w16, [1], clip_s=0.8, context_s=0.1)


def test_convert_files_routes_by_clip_s(pipe, monkeypatch):
    w24, w16 = songs([72000])
    monkeypatch.setattr(A, "load_batch", lambda sources, fs, engine, **kw: (w24, w16))
    seen = []
    monkeypatch.setattr(pipe, "convert_long", lambda *a, **kw: seen.append(("long", kw)) or ["L"])
    monkeypatch.setattr(pipe, "convert_ragged", lambda *a, **kw: seen.append(("ragged", kw)) or ["R"])
    assert pipe.convert_files(["a.wav"], [1]) == ["R"] and "clip_s" not in seen[-1][1] and "f0_shifted" not in seen[-1][1]
    assert pipe.convert_files(["a.wav"], [1], clip_s=None) == ["R"]
    assert pipe.convert_files(["a.wav"], [1], clip_s=0.8, context_s=0.32, pcm16=True) == ["L"]
    assert seen[-1][0] == "long" and seen[-1][1]["clip_s"] == 0.8 and seen[-1][1]["context_s"] == 0.32
    assert seen[-1][1]["pcm16"] is True
