"""CPU: the key-shifted mel's numpy reference (tests/keyshift_ref.py) and the host side of k_step_mel. The reference
agrees with the torch form of the same definition (torch.stft with a window and transform of n_new samples at the held
hop); the key-shifted mel of a tone at f0 is the plain mel of the tone at factor * f0, which the unshifted mel is far
from; every Python layer rejects a bad k_step_mel before any device work, and SVCServer keeps one value per batch."""
import os
import re
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import keyshift_ref as KR
from oracle import features as OF
from oracle import noise as ON
from svc_inference_pipeline_amd import _lib
from svc_inference_pipeline_amd import config as C
from svc_inference_pipeline_amd.pipeline import SVCPipeline
from svc_inference_pipeline_amd.runtime import check_k_step_mel
from svc_inference_pipeline_amd.serving import SVCServer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = [0.5, 0.75, 2.0 ** (-5 / 12), 1.0, 2.0 ** (3 / 12), 2.0 ** (7 / 12), 2.0]
MEAN_BOUND, MAX_BOUND = 3e-5, 4e-3  # the f64 transform against torch's f32 FFT; the max sits at cells near the clamp


@pytest.fixture(scope="module")
def cfg():
    return C.load_config()


def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    lib = _lib.load()
    for name in ("svc_pitch_factor", "svc_mel_keyshift"):
        assert re.search(r"^svc_status\s+%s\s*\(" % name, header, re.M), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.svc_abi_version() == _lib.ABI_VERSION == 3  # additions only


def test_n_new_rule():
    assert KR.n_new_of(2.0 ** (-5 / 12), 1024) == (767, 0) and KR.n_new_of(2.0 ** (3 / 12), 1024) == (1218, 0)
    assert KR.n_new_of(0.5, 1024) == (512, 0) and KR.n_new_of(2.0, 1024) == (2048, 0)
    assert KR.n_new_of(0.3, 1024) == (512, 2) and KR.n_new_of(3.0, 1024) == (2048, 2)
    assert KR.n_new_of(1e300, 1024) == (2048, 2)
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        assert KR.n_new_of(bad, 1024) == (1024, 1)
    assert KR.n_new_of(1022.5 / 1024, 1024) == (1022, 0) and KR.n_new_of(1023.5 / 1024, 1024) == (1024, 0)  # half to even


def torch_form(wav, factor, cfg, fb):
    """The same definition with torch: reflect-pad by (n_new - hop) // 2 and (n_new - hop + 1) // 2, torch.stft with
    n_new points and a periodic Hann window of n_new at the held hop, sqrt(. + 1e-9), crop or zero-fill to
    n_fft / 2 + 1 bins, * n_fft / n_new, filterbank, log(clamp 1e-5). -> f32 [T, n_mels]"""
    n, hop = cfg.n_fft, cfg.hop_length
    n_new = KR.n_new_of(factor, n)[0]
    y = torch.from_numpy(np.asarray(wav, np.float32))[None]
    pl, pr = (n_new - hop) // 2, (n_new - hop + 1) // 2
    y = torch.nn.functional.pad(y.unsqueeze(1), (pl, pr), mode="reflect").squeeze(1)
    spec = torch.stft(y, n_new, hop_length=hop, win_length=n_new, window=torch.hann_window(n_new), center=False,
                      normalized=False, onesided=True, return_complex=True)
    spec = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + 1e-9)[0]  # [n_new // 2 + 1, T]
    nb = n // 2 + 1
    if spec.shape[0] < nb:
        spec = torch.nn.functional.pad(spec, (0, 0, 0, nb - spec.shape[0]))
    spec = spec[:nb] * n / n_new
    mel = torch.matmul(torch.from_numpy(fb).float(), spec)
    return torch.log(torch.clamp(mel, min=1e-5)).T.numpy()


@pytest.fixture(scope="module")
def ref_clips(cfg):
    return [ON.synth_clip(3, s, 24000) for s in (0.3, 2.0)]


@pytest.mark.parametrize("factor", FACTORS, ids=lambda f: "%.4f" % f)
def test_reference_vs_torch_form(cfg, ref_clips, factor):
    fb = KR.filterbank(cfg)
    for wav in ref_clips:
        ref, info = KR.mel_keyshift(wav, factor, cfg, fb)
        tf = torch_form(wav, factor, cfg, fb)
        assert info == 0 and ref.shape == tf.shape == (OF.mel_frames(len(wav)), cfg.n_mels)
        d = np.abs(ref - tf)
        print(f"factor {factor:.4f} n={len(wav)}: mean |d| {d.mean():.3e} max |d| {d.max():.3e}")
        assert d.mean() < MEAN_BOUND and d.max() < MAX_BOUND


def test_reference_at_factor_one_is_the_mel(cfg, ref_clips):
    for wav in ref_clips:
        ref, _ = KR.mel_keyshift(wav, 1.0, cfg)
        mel = OF.mel_spectrogram(torch.from_numpy(wav)[None], cfg)[0].numpy().T
        d = np.abs(ref - mel)
        print(f"n={len(wav)}: mean |d| {d.mean():.3e} max |d| {d.max():.3e}")
        assert d.mean() < MEAN_BOUND and d.max() < MAX_BOUND


def tone(f0, seconds=1.0, fs=24000):
    t = np.arange(int(round(seconds * fs)), dtype=np.float64) / fs
    return (0.3 / 1.7 * sum(np.sin(2 * np.pi * h * f0 * t) / h for h in range(1, 9))).astype(np.float32)


@pytest.mark.parametrize("f0,factor", [(220.0, 2.0 ** (4 / 12)), (330.0, 2.0 ** (-7 / 12)), (150.0, 2.0), (400.0, 0.5)])
def test_shifted_mel_of_a_tone_is_the_mel_of_the_shifted_tone(cfg, f0, factor):
    fb = KR.filterbank(cfg)
    shifted = KR.mel_keyshift(tone(f0), factor, cfg, fb)[0][4:-4]
    plain = KR.mel_keyshift(tone(f0), 1.0, cfg, fb)[0][4:-4]
    target = KR.mel_keyshift(tone(factor * f0), 1.0, cfg, fb)[0][4:-4]
    d_shift, d_plain = np.abs(shifted - target).mean(), np.abs(plain - target).mean()
    print(f"f0 {f0} x {factor:.4f}: shifted {d_shift:.3f} nat, unshifted {d_plain:.3f} nat")
    assert d_shift < 0.15
    assert d_plain > 1.5


# ------------------------------------------------------------------ host validation
def test_check_k_step_mel():
    assert check_k_step_mel("source", None) == "source" and check_k_step_mel("source", 300) == "source"
    assert check_k_step_mel("shifted", 300) == "shifted"
    for bad in ("Shifted", "", None, 1, "target"):
        with pytest.raises(ValueError, match="k_step_mel"):
            check_k_step_mel(bad, 300)
    with pytest.raises(ValueError, match="needs k_step"):
        check_k_step_mel("shifted", None)


class _NoDeviceEngine:
    """An engine whose every stage fails the test: a bad k_step_mel must be rejected before any of them runs."""
    ragged_hubert = ragged_whisper = False

    def __init__(self):
        self.cfg = C.load_config()
        self.lock = threading.RLock()

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached with a bad k_step_mel")


@pytest.mark.parametrize("kw,match", [(dict(k_step=300, k_step_mel="both"), "k_step_mel"),
                                      (dict(k_step_mel="shifted"), "needs k_step"),
                                      (dict(k_step=None, k_step_mel="shifted"), "needs k_step")])
def test_pipeline_rejects_bad_k_step_mel_before_device_work(kw, match):
    pipe = SVCPipeline(_NoDeviceEngine())
    w24, w16 = torch.zeros(1, 2400), torch.zeros(1, 1600)
    with pytest.raises(ValueError, match=match):
        pipe.convert(w24, w16, torch.zeros(1, dtype=torch.int32), **kw)
    for bucketed in (False, True):
        with pytest.raises(ValueError, match=match):
            pipe.convert_many([w24[0]], [w16[0]], [0], bucketed=bucketed, **kw)
    with pytest.raises(ValueError, match=match):
        pipe.convert_ragged([w24[0]], [w16[0]], [0], **kw)
    with pytest.raises(ValueError, match=match):
        pipe.convert_files([b"not read"], [0], **kw)


def test_cli_k_step_mel(capsys):
    from svc_inference_pipeline_amd import infer
    ap = infer.build_parser()
    assert ap.parse_args(["--wav", "a.wav"]).k_step_mel == "source"
    args = ap.parse_args(["--wav", "a.wav", "--k-step", "300", "--k-step-mel", "shifted"])
    assert args.k_step == 300 and args.k_step_mel == "shifted"
    with pytest.raises(SystemExit) as exc:  # before any model is loaded
        infer.main(["--wav", "a.wav", "--k-step-mel", "shifted", "--random-weights", "tiny-test"])
    assert exc.value.code == 2 and "--k-step-mel shifted needs --k-step" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        ap.parse_args(["--wav", "a.wav", "--k-step", "300", "--k-step-mel", "target"])
    assert exc.value.code == 2


class FakePipeline:
    """convert_ragged stand-in (as tests/test_serving.py's): records each batch's utterance ids and keywords."""

    def __init__(self):
        self.engine = SimpleNamespace(cfg=SimpleNamespace(n_fft=1024, hop_length=256), device=None)
        self.calls = []

    def convert_ragged(self, wavs24, wavs16, singers, wavs16_float=None, utt_ids=None, **kw):
        self.calls.append((list(utt_ids), kw))
        return [w * (s + 1) + u for w, s, u in zip(wavs24, singers, utt_ids)]


def test_server_never_mixes_k_step_mels():
    p = FakePipeline()
    reqs = [(300, "source"), (300, "shifted"), (300, "source"), (300, "shifted"), (None, "source"), (100, "shifted")]
    # nothing runs before close(): fewer requests than max_batch and a long max_wait_s; closing drains the queue
    with SVCServer(p, max_batch=8, max_wait_s=60.0, speedup=250, seed=3) as srv:
        futs = [srv.submit(torch.full((2000,), 0.5), torch.ones(1000), singer=0, k_step=k, k_step_mel=m)
                for k, m in reqs]
        with pytest.raises(ValueError, match="needs k_step"):
            srv.submit(torch.ones(2000), torch.ones(1000), singer=0, k_step_mel="shifted")
        with pytest.raises(ValueError, match="k_step_mel"):
            srv.submit(torch.ones(2000), torch.ones(1000), singer=0, k_step=300, k_step_mel="both")
        with pytest.raises(ValueError, match="needs k_step"):
            srv.submit_file(b"RIFF", singer=0, k_step_mel="shifted")
    outs = [f.result(timeout=10) for f in futs]
    # equal lengths: only (k_step, k_step_mel) separates them; the oldest request's pair forms each batch
    assert list(srv.batches) == [[0, 2], [1, 3], [4], [5]]
    base = dict(fast_inference=True, speedup=250, seed=3)
    assert [kw for _, kw in p.calls] == [dict(base, k_step=300), dict(base, k_step=300, k_step_mel="shifted"), base,
                                         dict(base, k_step=100, k_step_mel="shifted")]
    for i, o in enumerate(outs):
        assert torch.equal(o, torch.full((2000,), 0.5) + i)
