"""CPU: shallow diffusion's host side. The three new C-ABI symbols are declared, bound and exported with the ABI version
unchanged; the float64 normaliser of tests/shallow_ref.py inverts the oracle's de-normaliser on the packaged statistics;
every Python layer rejects a bad k_step before any device work; SVCServer never puts two k_step values in one batch."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import shallow_ref as S
from oracle import features as OF
from svc_inference_pipeline_amd import _lib
from svc_inference_pipeline_amd import config as C
from svc_inference_pipeline_amd.pipeline import SVCPipeline
from svc_inference_pipeline_amd.runtime import SVCEngine, check_k_step
from svc_inference_pipeline_amd.serving import SVCServer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svc_mel_normalize", "svc_diffsvc_sample_from", "svc_op_q_sample")


def test_new_symbols_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"^svc_status\s+%s\s*\(" % name, header, re.M), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.svc_abi_version() == _lib.ABI_VERSION == 3  # additions only


def test_normalize_inverts_denormalize_on_packaged_stats():
    """normalize(denormalize(x)) = x to float64 rounding: with d = max - min + 1e-12 the round trip is
    ((x + 1) / 2 d + min - min) / d * 2 - 1, whose only error that is not a relative rounding of an O(1) value is the
    cancellation against min (|min| <= 11.6 against a result scaled by 2 / d). Bound: 16 * 2^-53 * (1 + |x| + 2 |min| / d)
    per element."""
    st = C.load_stats(C.load_config())
    mn, mx = st["mel_min"].astype(np.float64), st["mel_max"].astype(np.float64)
    assert mn.shape == mx.shape == (100,)
    assert np.all(mx > mn)  # every channel has a range: the normaliser never divides by the 1e-12 guard alone
    x = np.random.default_rng(0).uniform(-1.3, 1.3, (100, 257))  # [n_mel, T], out-of-range frames included
    den = OF.denormalize_mel_channel(x, mn, mx)
    back = S.normalize_mel_channel(den.T, mn, mx).T
    d = (mx - mn + 1e-12)[:, None]
    bound = 16 * 2.0 ** -53 * (1 + np.abs(x) + 2 * np.abs(mn)[:, None] / d)
    assert np.all(np.abs(back - x) <= bound)
    # and it is the reference's own formula on the reference's own layout ([n_mel, T], statistics expanded on axis -1)
    ref = (den - mn[:, None]) / (mx[:, None] - mn[:, None] + 1e-12) * 2 - 1
    assert np.array_equal(back, ref)
    # not clamped
    assert back.min() < -1.2 and back.max() > 1.2


def test_q_sample_reference_limits():
    """a^2 + b^2 = 1 to float32 rounding at every K; K = 1 is almost the clean mel and K = 1000 almost pure noise."""
    import sampler_ref as R
    sch = R.schedule()
    for K in (1, 2, 300, 1000):
        a, b = S.q_coeffs(sch, K)
        assert abs(float(a) ** 2 + float(b) ** 2 - 1.0) < 4 * 2.0 ** -24
    assert S.q_coeffs(sch, 1)[0] > 0.999 and S.q_coeffs(sch, 1000)[0] < 0.01
    z = S.q_noise(9, [7, 0], 5, 100)
    assert z.shape == (2, 5, 100) and not np.array_equal(z, R.noise_block(9, [7, 0], R.XT_STEP, 5, 100))
    y = np.full((2, 5, 100), 0.25)
    assert np.array_equal(S.q_sample(y, np.float32(1.0), np.float32(0.0), z), y)


@pytest.mark.parametrize("bad", [0, -3, 1001, 2.5, "300", True])
def test_check_k_step_rejects(bad):
    cfg = C.load_config()
    with pytest.raises(ValueError, match="k_step"):
        check_k_step(bad, cfg)


def test_check_k_step_accepts():
    cfg = C.load_config()
    assert check_k_step(None, cfg) is None
    assert check_k_step(1, cfg) == 1 and check_k_step(np.int64(1000), cfg) == 1000


class _NoDeviceEngine:
    """An engine whose every stage fails the test: a bad k_step must be rejected before any of them runs."""
    ragged_hubert = ragged_whisper = False

    def __init__(self):
        import threading
        self.cfg = C.load_config()
        self.lock = threading.RLock()

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached with a bad k_step")


@pytest.mark.parametrize("bad", [0, 1001, 2.5])
def test_pipeline_rejects_bad_k_step_before_device_work(bad):
    pipe = SVCPipeline(_NoDeviceEngine())
    w24, w16 = torch.zeros(1, 2400), torch.zeros(1, 1600)
    with pytest.raises(ValueError, match="k_step"):
        pipe.convert(w24, w16, torch.zeros(1, dtype=torch.int32), k_step=bad)
    for bucketed in (False, True):
        with pytest.raises(ValueError, match="k_step"):
            pipe.convert_many([w24[0]], [w16[0]], [0], bucketed=bucketed, k_step=bad)
    with pytest.raises(ValueError, match="k_step"):
        pipe.convert_ragged([w24[0]], [w16[0]], [0], k_step=bad)
    with pytest.raises(ValueError, match="k_step"):
        pipe.convert_files([b"not read"], [0], k_step=bad)


def test_engine_rejects_bad_k_step_arguments():
    """SVCEngine.diffsvc_sample checks k_step and its start-state arguments before it touches the library."""
    e = SVCEngine.__new__(SVCEngine)  # no context: the checks come first
    e.cfg = C.load_config()
    cond = torch.zeros(1, 4, 384)
    mel = torch.zeros(1, 4, 100)
    for bad in (0, 1001, 2.5):
        with pytest.raises(ValueError, match="k_step"):
            e.diffsvc_sample(cond, k_step=bad, mel_src=mel)
    with pytest.raises(ValueError, match="exactly one"):
        e.diffsvc_sample(cond, k_step=300)
    with pytest.raises(ValueError, match="exactly one"):
        e.diffsvc_sample(cond, k_step=300, mel_src=mel, x_start=mel)
    with pytest.raises(ValueError, match="exactly one"):
        e.diffsvc_sample(cond, k_step=300, x_start=mel, x_T=mel)
    with pytest.raises(ValueError, match="need k_step"):
        e.diffsvc_sample(cond, mel_src=mel)


def test_cli_k_step_and_resynth_arguments(capsys):
    """--k-step parses with and without --fast and a bad value ends the run before any model is loaded; --resynth
    needs only a vocoder checkpoint (its absence is the one thing it reports)."""
    from svc_inference_pipeline_amd import infer
    ap = infer.build_parser()
    assert ap.parse_args(["--wav", "a.wav"]).k_step is None and not ap.parse_args(["--wav", "a.wav"]).resynth
    assert ap.parse_args(["--wav", "a.wav", "--k-step", "300"]).k_step == 300
    assert ap.parse_args(["--wav", "a.wav", "--k-step", "300", "--fast"]).fast
    for bad in ("0", "1001"):
        with pytest.raises(SystemExit) as exc:
            infer.main(["--wav", "a.wav", "--k-step", bad, "--random-weights", "tiny-test"])
        assert exc.value.code == 2 and "k_step" in capsys.readouterr().err
    cfg = C.load_config()
    cfg.vocoder_model_path = None
    with pytest.raises(SystemExit, match="--resynth needs --vocoder-ckpt"):
        infer.build_vocoder_engine(cfg, 0, None, None)


class FakePipeline:
    """convert_ragged stand-in (as tests/test_serving.py's): records each batch's utterance ids and keywords."""

    def __init__(self):
        self.engine = SimpleNamespace(cfg=SimpleNamespace(n_fft=1024, hop_length=256), device=None)
        self.calls = []

    def convert_ragged(self, wavs24, wavs16, singers, wavs16_float=None, utt_ids=None, **kw):
        self.calls.append((list(utt_ids), kw))
        return [w * (s + 1) + u for w, s, u in zip(wavs24, singers, utt_ids)]


def test_server_never_mixes_k_steps():
    p = FakePipeline()
    ks = [None, 300, 300, None, 100, 300]
    # nothing runs before close(): fewer requests than max_batch and a long max_wait_s; closing drains the queue
    with SVCServer(p, max_batch=8, max_wait_s=60.0, speedup=250, seed=3) as srv:
        futs = [srv.submit(torch.full((2000,), 0.5), torch.ones(1000), singer=0, k_step=k) for k in ks]
        with pytest.raises(ValueError, match="k_step"):
            srv.submit(torch.ones(2000), torch.ones(1000), singer=0, k_step=0)
    outs = [f.result(timeout=10) for f in futs]
    # equal lengths: only k_step separates them; the oldest request's k_step forms each batch
    assert list(srv.batches) == [[0, 3], [1, 2, 5], [4]]
    base = dict(fast_inference=True, speedup=250, seed=3)
    assert [kw for _, kw in p.calls] == [base, dict(base, k_step=300), dict(base, k_step=100)]
    for i, o in enumerate(outs):
        assert torch.equal(o, torch.full((2000,), 0.5) + i)


def test_server_file_requests_carry_k_step():
    """submit_file validates k_step on the caller's thread and keeps it on the request (a bad file fails its own future
    as before)."""
    p = FakePipeline()
    with SVCServer(p, max_batch=2, max_wait_s=0.05) as srv:
        with pytest.raises(ValueError, match="k_step"):
            srv.submit_file(b"RIFF", singer=0, k_step=-1)
        fut = srv.submit_file(b"not a wav file", singer=0, k_step=300)
        assert fut.done() and fut.exception() is not None
