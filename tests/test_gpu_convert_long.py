"""Long-form conversion end to end on the GPU: SVCPipeline.convert_long (chunk plan, song-level F0, chunk conversion,
svc_stitch, song-level loudness and sample conversion), convert_files(clip_s=) and the CLI's --clip.

The engine is the CLI's --random-weights tiny-test one (plumbing, not audio quality); PLMS at speedup 250. The song is a
3.0 s synthetic clip cut by clip_s = 0.8, context_s = 0.32 into 4 chunks of 75-frame bodies. One conversion of it is
shared by the tests that only look at it."""
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import dev  # noqa: E402
from oracle import noise as ON  # noqa: E402
from stitch_util import ulps  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import audio as A  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import infer as I  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402

KW = dict(fast_inference=True, speedup=250, seed=4)
CLIP = dict(clip_s=0.8, context_s=0.32)
SEED, UTT, SINGER = 31, 5, 1


@pytest.fixture(scope="module")
def tiny():
    cfg = C.load_config()
    e = I.build_engine(cfg, 0, random_weights="tiny-test", seed=0)
    yield cfg, e, SVCPipeline(e)
    e.close()


def clip(seed, seconds):
    return dev(ON.synth_clip(seed, seconds, 24000)), dev(ON.synth_clip_16k_quantised(seed, seconds))


@pytest.fixture(scope="module")
def song(tiny):
    """The 3.0 s song, its conversion with return_chunks, and the plan."""
    cfg, e, pipe = tiny
    w24, w16 = clip(SEED, 3.0)
    wavs, info = pipe.convert_long([w24], [w16], [SINGER], utt_ids=[UTT], return_chunks=True, **CLIP, **KW)
    torch.cuda.synchronize()
    return w24, w16, wavs[0], info


def stitch_launches(fn):
    _lib.profile_enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    return res, sum(v["launches"] for k, v in prof.items() if k.startswith("stitch"))


def test_plan_and_shapes(tiny, song):
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    p = info.plans[0]
    assert p.chunks == 4 and [b1 - b0 for b0, b1 in p.body] == [75, 75, 75, 56] and p.T_song == 281
    assert p.noise_ids == [(UTT << 12) | k for k in range(4)]
    assert wav.dtype == torch.float32 and wav.shape == (p.T_song * cfg.hop_length,)
    assert [tuple(c.shape) for c in info.chunks[0]] == [(t * cfg.hop_length,) for t in p.frames]
    assert bool(torch.isfinite(wav).all())
    tail = max(p.stitch.search - 1, 0)
    assert not wav[-tail:].any() and wav[:-tail].abs().max() > 0  # the end no displaced last chunk could fill


def test_chunk_waveforms_are_convert_ragged_of_the_slices(tiny, song):
    """Each chunk is bit for bit convert_ragged of the plan's slices with the chunk noise ids and f0_shifted = the
    slices of the song-level shifted F0 (one group here, two groups of two there)."""
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    p = info.plans[0]
    s24 = [w24[lo:hi] for lo, hi in p.rows24]
    s16 = [w16[lo:hi] for lo, hi in p.rows16]
    f0s = [info.f0[0][s:s + t] for s, t in zip(p.start, p.frames)]
    ref = pipe.convert_ragged(s24, s16, [SINGER] * 4, utt_ids=p.noise_ids, f0_shifted=f0s, **KW)
    for k in range(4):
        assert torch.equal(info.chunks[0][k], ref[k]), k
    # without the supplied F0 the chunks come out different: it is used
    own = pipe.convert_ragged(s24, s16, [SINGER] * 4, utt_ids=p.noise_ids, **KW)
    assert any(not torch.equal(own[k], ref[k]) for k in range(4))
    # a mixed list: the clips without an entry are extracted and shifted as usual
    mixed = pipe.convert_ragged(s24, s16, [SINGER] * 4, utt_ids=p.noise_ids, f0_shifted=[f0s[0], None, f0s[2], None], **KW)
    for k in range(4):
        assert torch.equal(mixed[k], (ref if k % 2 == 0 else own)[k]), k


def test_stitched_result_is_the_host_stitch_of_the_chunks(tiny, song):
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    p = info.plans[0]
    rows = [c.cpu().numpy() for c in info.chunks[0]]
    want, shifts = A.stitch(rows, p.stitch, return_shifts=True)
    got = info.stitched[0].cpu().numpy()
    assert info.shifts[0].cpu().tolist() == shifts.tolist()
    print("displacements", shifts.tolist(), "max ulp", int(ulps(got, want).max()))
    assert ulps(got, want).max() <= 1
    assert torch.equal(wav, info.stitched[0])  # no loudness stage, no sample conversion: the stitched song itself
    st = p.stitch
    for k in range(4):  # past each crossfade the chunk's own samples, bit for bit
        lo = st.lead[k] + int(shifts[k])
        x = st.xfade if k else 0
        assert np.array_equal(got[st.out_off[k] + x:st.out_off[k] + st.body[k]], rows[k][lo + x:lo + st.body[k]])


def test_f0_is_the_songs_own(tiny, song):
    """The returned F0 is shift_f0(extract_f0(song)), bit for bit, not what the chunks alone would give: the chunk-wise
    factors differ from the song's for this input."""
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    p = info.plans[0]
    f0 = pipe.extract_f0(w24[None].contiguous(), p.T_song)
    song_factor = e.pitch_factor(f0, *pipe.shift_targets(1, [SINGER]))
    pipe.shift_f0(f0, [SINGER])
    assert torch.equal(info.f0[0], f0[0]) and info.f0[0].dtype == torch.float64
    factors = []
    for (lo, hi), t in zip(p.rows24, p.frames):
        fk = pipe.extract_f0(w24[lo:hi][None].contiguous(), t)
        factors.append(float(e.pitch_factor(fk, *pipe.shift_targets(1, [SINGER]))[0]))
    print("song factor", float(song_factor[0]), "chunk factors", factors)
    assert all(np.isfinite(factors)) and any(f != float(song_factor[0]) for f in factors)


def test_single_chunk_is_convert_ragged(tiny):
    cfg, e, pipe = tiny
    w24, w16 = clip(SEED + 1, 1.0)
    (got, info), n = stitch_launches(lambda: pipe.convert_long([w24], [w16], [SINGER], utt_ids=[7], return_chunks=True,
                                                               **CLIP, **KW))
    assert info.plans[0].chunks == 1 and n == 2 and not info.shifts[0].any()
    ref = pipe.convert_ragged([w24], [w16], [SINGER], utt_ids=[7 << 12], **KW)
    assert torch.equal(got[0], ref[0])


def test_group_size_does_not_matter(tiny, song):
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    two = pipe.convert_long([w24], [w16], [SINGER], utt_ids=[UTT], max_batch=2, **CLIP, **KW)
    assert torch.equal(two[0], wav)
    one = pipe.convert_long([w24], [w16], [SINGER], utt_ids=[UTT], max_batch=1, **CLIP, **KW)
    assert torch.equal(one[0], wav)


def test_two_songs_in_one_call_equal_each_alone(tiny, song):
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    v24, v16 = clip(SEED + 2, 1.7)
    (both, binfo), n = stitch_launches(lambda: pipe.convert_long([v24, w24], [v16, w16], [2, SINGER], utt_ids=[9, UTT],
                                                                 max_batch=3, return_chunks=True, **CLIP, **KW))
    assert n == 2 and [p.chunks for p in binfo.plans] == [2, 4]
    alone = pipe.convert_long([v24], [v16], [2], utt_ids=[9], **CLIP, **KW)
    assert both[0].shape == alone[0].shape and torch.equal(both[0], alone[0])
    assert torch.equal(both[1], wav)


def test_loudness_mix(tiny, song):
    """loudness_mix = 0: audio.loudness_match of the stitched song against the song's own source, within 1 ulp (the
    envelope is the song's, not a chunk's)."""
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    got, ginfo = pipe.convert_long([w24], [w16], [SINGER], utt_ids=[UTT], loudness_mix=0.0, return_chunks=True, **CLIP,
                                   **KW)
    assert torch.equal(ginfo.stitched[0], wav)
    want = A.loudness_match(wav.cpu().numpy(), w24.cpu().numpy(), fs=cfg.fs, mix=0.0)
    d = ulps(got[0].cpu().numpy(), want)
    assert d.max() <= 1, int(d.max())
    assert not np.array_equal(want, wav.cpu().numpy())  # the stage did something


def test_pcm16(tiny, song):
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    got = pipe.convert_long([w24], [w16], [SINGER], utt_ids=[UTT], pcm16=True, **CLIP, **KW)
    ref = e.pcm16(wav[None].contiguous())
    assert got[0].dtype == torch.int16 and torch.equal(got[0], ref[0])
    assert got[0].shape[0] == wav.shape[0] + 2 * (cfg.fs // 20)


def test_shallow_diffusion_uses_the_songs_factor(tiny, song):
    """k_step with k_step_mel="shifted": every chunk's start mel is shifted by the SONG's factor. The chunks equal
    convert_ragged of the slices with that factor given, and differ with another factor."""
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    p = info.plans[0]
    kw = dict(k_step=500, k_step_mel="shifted", key_shift=3.0, **KW)
    got, ginfo = pipe.convert_long([w24], [w16], [SINGER], utt_ids=[UTT], return_chunks=True, **CLIP, **kw)
    assert bool(torch.isfinite(got[0]).all())
    f0 = pipe.extract_f0(w24[None].contiguous(), p.T_song)
    factor = e.pitch_factor(f0, *pipe.shift_targets(1, [SINGER], 3.0))
    pipe.shift_f0(f0, [SINGER], 3.0)
    assert torch.equal(ginfo.f0[0], f0[0])
    s24 = [w24[lo:hi] for lo, hi in p.rows24]
    s16 = [w16[lo:hi] for lo, hi in p.rows16]
    f0s = [f0[0, s:s + t] for s, t in zip(p.start, p.frames)]
    args = (s24, s16, [SINGER] * 4)
    ckw = dict(utt_ids=p.noise_ids, f0_shifted=f0s, k_step=500, k_step_mel="shifted", **KW)
    ref = pipe.convert_ragged(*args, factor=factor.repeat(4), **ckw)
    other = pipe.convert_ragged(*args, factor=factor.repeat(4) * 1.25, **ckw)
    for k in range(4):
        assert torch.equal(ginfo.chunks[0][k], ref[k]), k
    assert any(not torch.equal(other[k], ref[k]) for k in range(4))
    with pytest.raises(ValueError, match="factor"):
        pipe.convert_ragged(*args, **ckw)


def write_song(path, seconds=3.0):
    pcm = np.clip(np.round(ON.synth_clip(SEED, seconds, 24000).astype(np.float64) * 32768.0), -32768, 32767)
    A.write_wav_pcm16(str(path), pcm.astype(np.int16), 24000)


def test_cli_and_convert_files(tiny, tmp_path):
    """--clip 0.8 --clip-context 0.32 writes the samples convert_files(clip_s=0.8, context_s=0.32, pcm16=True) returns
    (utterance id 0, the CLI's seed-0 engine, which is this module's)."""
    cfg, e, pipe = tiny
    src, out = tmp_path / "song.wav", tmp_path / "gen" / "song_out.wav"
    write_song(src)
    sid = int(C.load_singers(cfg)["svcc_CDF1"])
    want = pipe.convert_files([str(src)], [sid], pcm16=True, fast_inference=True, speedup=250, seed=0, **CLIP)
    w24, w16 = A.load_batch([str(src)], cfg.fs, e)
    long_ = pipe.convert_long(w24, w16, [sid], pcm16=True, fast_inference=True, speedup=250, seed=0, **CLIP)
    assert torch.equal(want[0], long_[0])
    assert I.main(["--wav", str(src), "--singer", "svcc_CDF1", "--out", str(out), "--random-weights", "tiny-test",
                   "--fast", "--speedup", "250", "--clip", "0.8", "--clip-context", "0.32"]) == 0
    with wave.open(str(out), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, 24000)
        pcm = np.frombuffer(f.readframes(f.getnframes()), "<i2")
    assert np.array_equal(pcm, want[0].cpu().numpy())
    plain = pipe.convert_files([str(src)], [sid], pcm16=True, fast_inference=True, speedup=250, seed=0)
    assert plain[0].shape == want[0].shape and not torch.equal(plain[0], want[0])  # the whole file as one utterance


def test_without_clip_nothing_changes(tiny, song, tmp_path):
    """convert_files(clip_s=None) and convert_ragged without the new keywords launch no stitch kernel, and the new
    keywords passed as None are the call without them, bit for bit."""
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    v24, v16 = clip(SEED + 2, 1.7)
    src = tmp_path / "song.wav"
    write_song(src, 1.0)
    _, n_files = stitch_launches(lambda: pipe.convert_files([str(src)], [SINGER], clip_s=None, **KW))
    plain, n_plain = stitch_launches(lambda: pipe.convert_ragged([w24, v24], [w16, v16], [SINGER, 2], **KW))
    none, n_none = stitch_launches(lambda: pipe.convert_ragged([w24, v24], [w16, v16], [SINGER, 2], f0_shifted=None,
                                                               factor=None, **KW))
    assert n_files == 0 and n_plain == 0 and n_none == 0
    for a, b in zip(plain, none):
        assert a.dtype == b.dtype and torch.equal(a, b)
    _, n_long = stitch_launches(lambda: pipe.convert_long([w24, v24], [w16, v16], [SINGER, 2], **CLIP, **KW))
    assert n_long == 2  # two launches for six chunks of two songs


def test_argument_errors(tiny, song):
    cfg, e, pipe = tiny
    w24, w16, wav, info = song
    with pytest.raises(ValueError, match="utterance id"):
        pipe.convert_long([w24], [w16], [SINGER], utt_ids=[1 << 19], **CLIP, **KW)
    with pytest.raises(ValueError, match="right context"):
        pipe.convert_long([w24], [w16], [SINGER], clip_s=0.8, context_s=0.1, **KW)
    with pytest.raises(ValueError, match="max_batch"):
        pipe.convert_long([w24], [w16], [SINGER], max_batch=0, **CLIP, **KW)
    with pytest.raises(ValueError, match="one entry per song"):
        pipe.convert_long([w24], [w16, w16], [SINGER], **CLIP, **KW)
    with pytest.raises(ValueError, match="f0_shifted"):
        pipe.convert_ragged([w24], [w16], [SINGER], f0_shifted=[info.f0[0][:-1]], **KW)
    with pytest.raises(ValueError, match="f0_shifted"):
        pipe.convert_ragged([w24], [w16], [SINGER], f0_shifted=[], **KW)
