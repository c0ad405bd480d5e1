"""GPU: svc_pitch_factor and svc_mel_keyshift (the key-shifted start mel of shallow diffusion) at op level against
tests/keyshift_ref.py, ragged batches, bad factors and invalid arguments, and k_step_mel="shifted" through SVCPipeline
and SVCServer against the hand-composed stage sequence."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import keyshift_ref as KR  # noqa: E402
from gpu_util import dev, ptr, stream  # noqa: E402
from oracle import noise as ON  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine, mel_frames  # noqa: E402
from svc_inference_pipeline_amd.serving import SVCServer  # noqa: E402

LENS = (6000, 7200, 24000)  # T = 23, 28, 93
FACTORS = (0.5, 2.0 ** (-5 / 12), 1.0, 2.0 ** (3 / 12), 2.0)  # n_new = 512, 767, 1024, 1218, 2048
# both sides transform in f64 and take the magnitude in f32; what differs is the f32 filterbank sum of at most about 60
# positive terms (about 4e-6 relative) and logf: 1e-4 is more than 10 x that
TOL = 1e-4


@pytest.fixture(scope="module")
def feat():
    """A features-only engine (no weights)."""
    e = SVCEngine(C.load_config(), 0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def clip(i):
    return ON.synth_clip(20 + i, LENS[i] / 24000.0, 24000)


@functools.lru_cache(maxsize=None)
def ref(i, factor):
    """The reference of clip i, computed once."""
    mel, info = KR.mel_keyshift(clip(i), factor, C.load_config())
    mel.setflags(write=False)
    return mel, info


def factors(vals):
    return torch.tensor(list(vals), dtype=torch.float64).cuda()


def alone(e, i, factor):
    mel, info = e.mel_keyshift(dev(clip(i))[None], factors([factor]))
    torch.cuda.synchronize()
    return mel[0], int(info[0])


# ------------------------------------------------------------------ 1. pitch_factor
def test_pitch_factor_is_the_factor_pitch_shift_applies(feat):
    B, T = 3, 93
    rng = np.random.default_rng(7)
    f0 = rng.uniform(80.0, 700.0, (B, T))
    f0[0, 10:31] = 0.0
    f0[0, 60:62] = 0.0
    f0[2, :5] = 0.0
    f0[2, 40:77] = 0.0  # an even and an odd voiced count between rows 0 and 2
    f0[1] = 0.0
    d = dev(f0, torch.float64)
    keep = d.clone()
    targets, scale = [174.7375, 301.5, 233.08], [2.0 ** (4 / 12), 1.0, 2.0 ** (-7 / 12)]
    for args in ((220.5,), (targets,), (targets, scale)):
        factor = feat.pitch_factor(d, *args)
        assert factor.shape == (B,) and factor.dtype == torch.float64
        assert torch.equal(d, keep)  # only read
        want = feat.pitch_shift(keep.clone(), *args)
        got = d * factor[:, None]
        torch.cuda.synchronize()
        assert bool(torch.isnan(factor[1])) and bool(torch.isfinite(factor[[0, 2]]).all())
        assert torch.equal(got[[0, 2]], want[[0, 2]])  # bit for bit
        assert bool(torch.isnan(got[1]).all()) and bool(torch.isnan(want[1]).all())
    # the value itself, against numpy
    factor = feat.pitch_factor(d, targets, scale).cpu().numpy()
    for b in (0, 2):
        med = np.median(f0[b][f0[b] != 0])
        assert factor[b] == targets[b] / med * scale[b]
    with pytest.raises(_lib.SVCError, match="target median"):
        feat.pitch_factor(d, [200.0, -1.0, 200.0])
    with pytest.raises(_lib.SVCError, match="scale"):
        feat.pitch_factor(d, targets, [1.0, float("nan"), 1.0])


# ------------------------------------------------------------------ 2. mel_keyshift against the reference
@pytest.mark.parametrize("factor", FACTORS, ids=lambda f: "%.4f" % f)
def test_mel_keyshift_vs_reference(feat, factor):
    for i in range(len(LENS)):
        want, winfo = ref(i, factor)
        got, info = alone(feat, i, factor)
        assert got.shape == (mel_frames(LENS[i]), 100) and info == winfo == 0
        d = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print(f"factor {factor:.4f} n={LENS[i]}: max |d| {d.max():.3e} mean |d| {d.mean():.3e}")
        assert d.max() <= TOL


def test_factor_one_is_mel_energy(feat):
    for i in range(len(LENS)):
        mel, _ = feat.mel_energy(dev(clip(i))[None])
        got, info = alone(feat, i, 1.0)
        d = (got - mel[0]).abs().max().item()
        print(f"n={LENS[i]}: max |d| {d:.3e}")
        assert info == 0 and d <= TOL


def test_shortest_valid_clip(feat):
    """897 samples: the widest window's reflection reaches sample 896 at the start and sample 0 at the end."""
    wav = ON.synth_clip(31, 897 / 24000.0, 24000)
    assert wav.shape == (897,)
    for factor in (2.0, 0.5):
        mel, info = feat.mel_keyshift(dev(wav)[None], factors([factor]))
        want, _ = KR.mel_keyshift(wav, factor, feat.cfg)
        assert mel.shape == (1, 3, 100) and int(info[0]) == 0
        assert np.abs(mel[0].cpu().numpy().astype(np.float64) - want).max() <= TOL


# ------------------------------------------------------------------ 3. ragged
def test_ragged_batch_is_each_clip_alone(feat):
    fs = [2.0 ** (3 / 12), 0.5, 2.0]
    N = max(LENS)
    w = torch.full((3, N), float("nan"), dtype=torch.float32).cuda()  # the padding must never be read
    for i, n in enumerate(LENS):
        w[i, :n] = dev(clip(i))
    mel, info = feat.mel_keyshift(w, factors(fs), n_samples=list(LENS))
    torch.cuda.synchronize()
    assert mel.shape == (3, mel_frames(N), 100) and info.tolist() == [0, 0, 0]
    assert bool(torch.isfinite(mel).all())
    for i, n in enumerate(LENS):
        one, _ = alone(feat, i, fs[i])
        Tb = mel_frames(n)
        assert torch.equal(mel[i, :Tb], one), i  # bit for bit
        assert bool((mel[i, Tb:] == 0).all()), i


# ------------------------------------------------------------------ 4. bad factors
@pytest.mark.parametrize("bad,as_factor,flag", [(float("nan"), 1.0, 1), (float("inf"), 1.0, 1), (0.0, 1.0, 1),
                                                (-1.0, 1.0, 1), (0.3, 0.5, 2), (3.0, 2.0, 2)])
def test_bad_factors_do_not_stop_a_batch(feat, bad, as_factor, flag):
    want, winfo = alone(feat, 1, as_factor)
    got, info = alone(feat, 1, bad)
    assert winfo == 0 and info == flag == KR.n_new_of(bad, 1024)[1]
    assert torch.equal(got, want)
    # and beside a good one in the same call
    w = dev(np.stack([clip(1), clip(1)]))
    mel, info = feat.mel_keyshift(w, factors([bad, 2.0 ** (3 / 12)]))
    assert info.tolist() == [flag, 0]
    assert torch.equal(mel[0], want) and torch.equal(mel[1], alone(feat, 1, 2.0 ** (3 / 12))[0])


# ------------------------------------------------------------------ 5. invalid arguments
def _raw(e, wav, B, N, factor, mel, lens=None):
    _lib.call("svc_mel_keyshift", e._ctx, ptr(wav), B, N, lens, ptr(factor), ptr(mel), None, stream())


def test_invalid_arguments(feat):
    w = dev(clip(1))[None]
    N = w.shape[1]
    f = factors([1.0])
    mel = torch.full((1, mel_frames(N), 100), 7.0, dtype=torch.float32).cuda()
    with pytest.raises(_lib.SVCError, match="status 1.*null factor"):
        _raw(feat, w, 1, N, None, mel)
    with pytest.raises(_lib.SVCError, match="status 1"):
        feat.mel_keyshift(w, None)
    with pytest.raises(_lib.SVCError, match="status 1.*null wav"):
        _raw(feat, None, 1, N, f, mel)
    with pytest.raises(_lib.SVCError, match="status 1.*null mel"):
        _raw(feat, w, 1, N, f, None)
    with pytest.raises(_lib.SVCError, match="status 1.*B=0"):
        _raw(feat, w, 0, N, f, mel)
    with pytest.raises(_lib.SVCError, match="status 1.*896"):
        _raw(feat, w, 1, 896, f, mel)
    with pytest.raises(_lib.SVCError, match="status 1.*utterance 0: 896"):
        _raw(feat, w, 1, N, f, mel, (ctypes.c_int64 * 1)(896))
    with pytest.raises(_lib.SVCError, match="status 1.*utterance 0"):
        _raw(feat, w, 1, N, f, mel, (ctypes.c_int64 * 1)(N + 1))
    torch.cuda.synchronize()
    assert bool((mel == 7.0).all())  # nothing was launched
    cfg = C.load_config()
    cfg.n_fft = cfg.win_length = 2048
    e = SVCEngine(cfg, 0)
    try:
        with pytest.raises(_lib.SVCError, match="status 1.*n_fft 2048"):
            e.mel_keyshift(dev(clip(2))[None], f)
    finally:
        e.close()


# ------------------------------------------------------------------ 6. / 7. pipeline and server
TINY = W.WHISPER_DIMS["tiny-test"]
K = 50
SECS = (0.6, 1.0)
KW = dict(fast_inference=True, speedup=10, seed=5)  # PLMS: 5 steps from K = 50


@pytest.fixture(scope="module")
def engine():
    """Full-size mapper and vocoder, tiny Whisper (as tests/test_gpu_shallow.py builds it)."""
    cfg = C.load_config()
    cfg.mapper.input_content_dim["whisper"] = TINY["n_audio_state"]
    e = SVCEngine(cfg, 0, whisper_state=W.make_whisper_state(TINY, 0), mapper_state=W.make_mapper_state(cfg.mapper, 0),
                  vocoder_state=W.make_vocoder_state(cfg.vocoder, 0))
    yield e
    e.close()


@pytest.fixture(scope="module")
def clips():
    w24 = [dev(ON.synth_clip(40 + i, s, 24000)) for i, s in enumerate(SECS)]
    w16 = [dev(ON.synth_clip_16k_quantised(40 + i, s)) for i, s in enumerate(SECS)]
    return w24, w16, [1, 3]


def _one(pipe, clips, i, **kw):
    w24, w16, singers = clips
    return pipe.convert(w24[i][None], w16[i][None], dev(np.array([singers[i]]), torch.int32),
                        utt_ids=dev(np.array([i]), torch.int32), **KW, **kw)


def _by_hand(engine, pipe, clips, i, shift_args):
    """f0, pitch_factor, pitch_shift, mel_keyshift, condition, diffsvc_sample(k_step, mel_src=shifted), bigvgan"""
    w24, w16, singers = clips
    w = w24[i][None]
    T = mel_frames(w.shape[1])
    f0 = engine.f0(w, T)
    factor = engine.pitch_factor(f0, *shift_args)
    engine.pitch_shift(f0, *shift_args)
    shifted, info = engine.mel_keyshift(w, factor)
    mel, energy = engine.mel_energy(w)
    content = pipe.content(w16[i][None], T)
    cond = engine.condition(content, f0, energy, dev(np.array([singers[i]]), torch.int32))
    x0 = engine.diffsvc_sample(cond, utt_ids=dev(np.array([i]), torch.int32), k_step=K, mel_src=shifted, **KW)
    return engine.bigvgan(x0), x0, mel, shifted, int(info[0]), float(factor[0])


def test_pipeline_shifted_is_the_hand_composed_sequence(engine, clips):
    pipe = SVCPipeline(engine)
    tm = engine.target_f0_median
    res = _one(pipe, clips, 1, k_step=K, k_step_mel="shifted", key_shift=4)
    wav, x0, mel, shifted, info, factor = _by_hand(engine, pipe, clips, 1, ([tm], [2.0 ** (4 / 12)]))
    assert info == 0 and np.isfinite(factor) and KR.n_new_of(factor, 1024)[0] != 1024  # the start mel does move
    assert torch.equal(res.x0, x0) and torch.equal(res.wav, wav) and bool(torch.isfinite(wav).all())
    assert torch.equal(res.mel, mel) and not torch.equal(mel, shifted)  # ConvertResult.mel stays the source mel
    # shift_f0's scalar route (no singer table, no key shift)
    res0 = _one(pipe, clips, 1, k_step=K, k_step_mel="shifted")
    wav0, x00 = _by_hand(engine, pipe, clips, 1, ())[:2]
    assert torch.equal(res0.x0, x00) and torch.equal(res0.wav, wav0)
    # "source" is the call without the keyword, and not the shifted one
    src = _one(pipe, clips, 1, k_step=K, k_step_mel="source", key_shift=4)
    plain = _one(pipe, clips, 1, k_step=K, key_shift=4)
    assert torch.equal(src.x0, plain.x0) and torch.equal(src.wav, plain.wav) and torch.equal(src.f0, res.f0)
    assert not torch.equal(src.x0, res.x0)


def test_ragged_and_server_shifted_match_single_clips(engine, clips):
    pipe = SVCPipeline(engine)
    w24, w16, singers = clips
    keys = [4.0, -3.0]
    ones = [_one(pipe, clips, i, k_step=K, k_step_mel="shifted", key_shift=keys[i]).wav[0] for i in range(2)]
    rag = pipe.convert_ragged(w24, w16, singers, utt_ids=[0, 1], key_shift=keys, k_step=K, k_step_mel="shifted", **KW)
    many = pipe.convert_many(w24, w16, singers, key_shift=keys, k_step=K, k_step_mel="shifted", bucketed=True, **KW)
    with SVCServer(pipe, max_batch=4, max_wait_s=60.0, **KW) as srv:
        futs = [srv.submit(w24[i], w16[i], singers[i], utt_id=i, key_shift=keys[i], k_step=K, k_step_mel="shifted")
                for i in range(2)]
    outs = [f.result(timeout=60) for f in futs]
    assert list(map(sorted, srv.batches)) == [[0, 1]]
    for i in range(2):
        assert torch.equal(rag[i], ones[i]) and torch.equal(many[i], ones[i]) and torch.equal(outs[i], ones[i]), i
