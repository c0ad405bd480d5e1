"""CPU: the host half of feeding HuBERT / ContentVec from wav files. svc_load_pcm_ex is declared, bound, exported and
checks its arguments before any HIP call; SVCPipeline.convert_files asks the load stage for the float 16 kHz rows
exactly when the configuration names a HuBERT type and hands them to hubert_encode (recording stand-in engine);
SVCServer batches a file request by what it will hold after decoding; the HuBERT checkpoint reader and writer are each
other's inverse; the CLI names --hubert-ckpt when the weights are missing."""
import copy
import ctypes
import json
import os
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from svc_inference_pipeline_amd import _lib
from svc_inference_pipeline_amd import audio as A
from svc_inference_pipeline_amd import config as C
from svc_inference_pipeline_amd import infer as I
from svc_inference_pipeline_amd import weights as W
from svc_inference_pipeline_amd.pipeline import HUBERT_CONTENT_TYPES, SVCPipeline
from svc_inference_pipeline_amd.serving import SVCServer, _Request
from wav_util import F32, S16, random_samples, wav_bytes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HT = W.HUBERT_DIMS["tiny-test"]


# ---------------------------------------------------------------------------- symbols and argument checks
def test_header_declares_and_library_exports_load_pcm_ex():
    txt = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    assert "svc_status svc_load_pcm_ex(svc_ctx* ctx, const void* raw, int B," in txt
    assert "float* y_mono_float, int32_t* info, void* stream);" in txt
    assert "svc_load_pcm_ex" in _lib.PROTOTYPES and hasattr(_lib.load(), "svc_load_pcm_ex")
    assert len(_lib.PROTOTYPES["svc_load_pcm_ex"][1]) == len(_lib.PROTOTYPES["svc_load_pcm"][1]) + 1
    assert _lib.load().svc_abi_version() == 3 == _lib.ABI_VERSION  # additions only


def _call_ex(ctx=True, B=1, byte_off=(0,), n_frames=(10,), fmt=(S16,), ch=(1,), sr=(44100,), sr_src=24000, S_src=16,
             y_src=True, sr_mono=16000, S_mono=16, y_mono=True, y_float=True):
    """svc_load_pcm_ex on host stand-ins: no argument below gets as far as a HIP call. ctx / raw / outputs are non-null
    pointers to host buffers that a failing call never reads."""
    keep = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(keep, ctypes.c_void_p)
    n = max(1, len(byte_off))
    i64 = lambda v: (ctypes.c_int64 * n)(*v)  # noqa: E731
    i32 = lambda v: (ctypes.c_int32 * n)(*v)  # noqa: E731
    lib = _lib.load()
    st = lib.svc_load_pcm_ex(p if ctx else None, p, B, i64(byte_off), i64(n_frames), i32(fmt), i32(ch), i32(sr), sr_src,
                             S_src, p if y_src else None, sr_mono, S_mono, p if y_mono else None,
                             p if y_float else None, None, None)
    return st, lib.svc_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(ctx=False), "null context"),
    (dict(y_src=False, y_mono=False, y_float=False), "null y_src and y_mono and y_mono_float (nothing to compute)"),
    (dict(y_src=False, y_mono=False, S_mono=0), "S_mono=0"),                      # a float row alone, S_mono < 1
    (dict(y_mono=False, S_mono=-4), "S_mono=-4"),
    (dict(y_src=False, y_mono=False, sr_mono=0), "sr_mono=0"),
    (dict(y_src=False, y_mono=False, S_mono=3), "4 mono samples, S_mono 3"),      # 10 frames at 44.1 kHz: 4 at 16 kHz
    (dict(B=2, byte_off=(0, 0), n_frames=(10, 100), fmt=(S16, S16), ch=(1, 1), sr=(16000, 16000), y_src=False,
          y_mono=False, S_mono=99), "utterance 1: 100 mono samples, S_mono 99"),  # rows that need no filter plan
    (dict(y_mono=False, S_src=5), "6 source samples, S_src 5"),
    (dict(y_src=False, y_mono=False, ch=(9,)), "9 channels"),
    (dict(y_src=False, y_mono=False, sr=(16000000,), n_frames=(0,)), "too large for the filter tile"),
])
def test_load_pcm_ex_rejects_bad_arguments_before_any_hip_call(kw, msg):
    st, err = _call_ex(**kw)
    assert st == 1, (st, err)
    assert err.startswith("load_pcm:") and msg in err, err
    with pytest.raises(_lib.SVCError, match="load_pcm"):
        _lib.check(st)


# ---------------------------------------------------------------------------- plumbing, with a recording engine
QUANT, FLOAT = 16.0, 0.25  # what the stand-in's quantised and float rows hold


class RecordingEngine:
    """Stands in for SVCEngine below convert_files: load_pcm fills the two mono batches with QUANT and FLOAT, and the
    content entry points record the audio they are handed."""
    ragged_hubert = ragged_whisper = True
    content_dtype = torch.float16

    def __init__(self, cfg):
        self.cfg, self.lock, self.calls = cfg, threading.RLock(), []

    def load_pcm(self, *args, **kwargs):
        self.calls.append(("load_pcm", args, kwargs))
        infos = args[0]
        B = len(infos)
        n24 = [i.n_frames * 3 // 2 for i in infos]
        n16 = [i.n_frames for i in infos]
        out = (torch.zeros(B, max(n24)), torch.full((B, max(n16)), QUANT), n24, n16, torch.zeros(B, dtype=torch.int32))
        return out + (torch.full((B, max(n16)), FLOAT),) if kwargs.get("float_mono") else out

    def whisper_content(self, w16, n16, T_b, T, out=None):
        self.calls.append(("whisper_content", w16.clone(), list(n16)))

    def hubert_encode(self, w16, n_samples=None):
        self.calls.append(("hubert_encode", w16.clone(), list(n_samples)))
        return torch.zeros(w16.shape[0], 3, 4)

    def hubert_frames(self, n):
        return 3

    def map_content(self, feats, T, rule="whisper", out=None, frames=None, src_rows=None):
        self.calls.append(("map_content", rule))


def _config(types):
    cfg = C.load_config()
    cfg.mapper.content_feature = list(types)
    for t in types:
        cfg.mapper.input_content_dim[t] = 8
    return cfg


def _run_convert_files(monkeypatch, types, **kw):
    """convert_files on two 16 kHz files through the real load_batch and ragged_content; the stages after the content
    features are cut off. -> (the engine's record, load_batch's recorded calls)"""
    e = RecordingEngine(_config(types))
    pipe = SVCPipeline(e)
    assert pipe.hubert_ragged and pipe.whisper_ragged
    batch_calls, real = [], A.load_batch

    def load_batch(*args, **kwargs):
        batch_calls.append((args, kwargs))
        return real(*args, **kwargs)

    def after_loading(wavs24, wavs16, singers, wavs16_float, *rest):
        pipe.ragged_content(list(wavs16), [4] * len(wavs16), 4, wavs16_float)
        return "converted"

    monkeypatch.setattr(A, "load_batch", load_batch)
    pipe._convert_ragged = after_loading
    rng = np.random.default_rng(0)
    files = [wav_bytes(S16, random_samples(rng, S16, n, 1), 16000) for n in (40, 25)]
    assert pipe.convert_files(files, [0, 1], **kw) == "converted"
    return e, files, batch_calls


def _audio_of(e, name):
    got = [c for c in e.calls if c[0] == name]
    assert len(got) == 1, (name, [c[0] for c in e.calls])
    return got[0][1], got[0][2]


@pytest.mark.parametrize("cv", HUBERT_CONTENT_TYPES)
def test_convert_files_feeds_hubert_the_float_rows(monkeypatch, cv):
    e, files, batch_calls = _run_convert_files(monkeypatch, [cv, "whisper"])
    (args, kwargs), = batch_calls
    assert kwargs == {"float16k": True} and args[1:] == (e.cfg.fs, e)
    name, largs, lkw = e.calls[0]
    assert name == "load_pcm" and lkw == {"float_mono": True} and len(largs) == 2 and largs[1] == e.cfg.fs
    w, n = _audio_of(e, "hubert_encode")
    assert n == [40, 25] and bool((w[0] == FLOAT).all()) and bool((w[1, :25] == FLOAT).all())
    w, n = _audio_of(e, "whisper_content")
    assert n == [40, 25] and bool((w[0] == QUANT).all()) and bool((w[1, :25] == QUANT).all())


def test_convert_files_float16k_false_keeps_the_old_feed(monkeypatch):
    e, files, batch_calls = _run_convert_files(monkeypatch, ["contentvec"], float16k=False)
    (args, kwargs), = batch_calls
    assert kwargs == {} and len(args) == 3
    assert e.calls[0][0] == "load_pcm" and e.calls[0][2] == {} and len(e.calls[0][1]) == 2
    w, n = _audio_of(e, "hubert_encode")
    assert n == [40, 25] and bool((w[0] == QUANT).all())
    e, _, _ = _run_convert_files(monkeypatch, ["contentvec"], float16k=True)
    assert bool((_audio_of(e, "hubert_encode")[0][0] == FLOAT).all())


def test_convert_files_on_the_packaged_config_loads_as_before(monkeypatch):
    """Whisper only: load_batch(sources, fs, engine) and load_pcm(infos, fs), no keyword, so an engine stand-in whose
    load_pcm does not know float_mono keeps working."""
    assert C.load_config().mapper.content_feature == ["whisper"]
    e, files, batch_calls = _run_convert_files(monkeypatch, ["whisper"])
    (args, kwargs), = batch_calls
    assert kwargs == {} and len(args) == 3 and args[0] == files and args[1:] == (e.cfg.fs, e)
    name, largs, lkw = e.calls[0]
    assert name == "load_pcm" and lkw == {} and len(largs) == 2 and largs[1] == e.cfg.fs
    assert [i.n_frames for i in largs[0]] == [40, 25]
    assert not [c for c in e.calls if c[0] == "hubert_encode"]
    assert bool((_audio_of(e, "whisper_content")[0][0] == QUANT).all())


def test_load_batch_returns_the_float_rows_before_the_errors():
    e = RecordingEngine(_config(["contentvec"]))
    rng = np.random.default_rng(1)
    good = wav_bytes(F32, random_samples(rng, F32, 30, 2), 16000)
    short = wav_bytes(S16, np.zeros((2, 1), np.int64), 16000)
    w24, w16, w16f, errors = A.load_batch([good, short, b"junk"], 24000, e, on_error="return", float16k=True)
    assert sorted(errors) == [1, 2] and isinstance(errors[1], A.AudioError)
    assert [x is None for x in w16f] == [False, True, True] == [x is None for x in w16] == [x is None for x in w24]
    assert w16f[0].shape == w16[0].shape == (30,) and bool((w16f[0] == FLOAT).all()) and bool((w16[0] == QUANT).all())
    w24, w16, w16f = A.load_batch([good], 24000, e, float16k=True)
    assert len(w16f) == 1 and bool((w16f[0] == FLOAT).all())
    assert len(A.load_batch([good], 24000, e)) == 2 and len(A.load_batch([good], 24000, e, on_error="return")) == 3
    with pytest.raises(A.AudioError, match="2 samples"):
        A.load_batch([good, short], 24000, e, float16k=True)


# ---------------------------------------------------------------------------- server batching
def _server(types):
    cfg = SimpleNamespace(n_fft=1024, hop_length=256, fs=24000, mapper=SimpleNamespace(content_feature=list(types)))
    return SVCServer(SimpleNamespace(engine=SimpleNamespace(cfg=cfg, device=None)), max_batch=8, max_wait_s=30.0)


def _take(srv, pending):
    """_take_batch on a queue of our own, with the worker kept out (it sleeps until a submit notifies it)"""
    with srv._cv:
        srv._pending = list(pending)
        batch = srv._take_batch()
        left, srv._pending = srv._pending, []
    return batch, left


def test_file_requests_batch_by_what_they_will_hold():
    data = wav_bytes(S16, random_samples(np.random.default_rng(2), S16, 4410, 1), 44100)
    x = torch.zeros(2400)
    for types, with_float in ((["contentvec"], True), (["whisper", "content_vector"], True), (["whisper"], False)):
        srv = _server(types)
        try:
            file_a, file_b = srv._file_request(data, 0, utt_id=1), srv._file_request(data, 0, utt_id=2)
            assert file_a.float16k is with_float and file_a.wav16_float is None and file_a.frames > 0
            plain = _Request(wav24=x, wav16=x, singer=0, utt_id=3, frames=file_a.frames)
            floats = _Request(wav24=x, wav16=x, singer=0, utt_id=4, wav16_float=x, frames=file_a.frames)
            mate, other = (floats, plain) if with_float else (plain, floats)
            batch, left = _take(srv, [file_a, plain, floats, file_b])
            assert [r.utt_id for r in batch] == [1, mate.utt_id, 2] and left == [other], types
            batch, left = _take(srv, [other, file_a, mate, file_b])
            assert batch == [other] and left == [file_a, mate, file_b], types
            batch, left = _take(srv, [mate, other, file_a])
            assert batch == [mate, file_a] and left == [other], types
        finally:
            srv.close()


# ---------------------------------------------------------------------------- checkpoints
def test_hubert_checkpoint_round_trip(tmp_path):
    sd = W.make_hubert_state(HT, 3)
    assert sorted(sd) == sorted(W.hubert_param_names(HT["n_layer"]))
    paths = W.save_checkpoints(str(tmp_path), hubert_state=sd)
    assert sorted(paths) == ["hubert"]
    ckpt = torch.load(paths["hubert"], map_location="cpu", weights_only=True)
    assert sorted(ckpt) == ["model"] and sorted(ckpt["model"]) == sorted(sd)  # fairseq's layout, fairseq's key names
    got = W.load_checkpoints(hubert_path=paths["hubert"])
    assert sorted(got) == ["hubert"] and sorted(got["hubert"]) == sorted(sd)
    for k, v in sd.items():
        assert got["hubert"][k].dtype == np.float32 and np.array_equal(got["hubert"][k], v), k
    dims = W.hubert_dims_from_state(got["hubert"], output_layer=HT["output_layer"])
    assert {k: dims[k] for k in HT} == HT


def test_hubert_checkpoint_with_legacy_args_and_missing_keys(tmp_path):
    import argparse
    sd = {k: torch.from_numpy(v) for k, v in W.make_hubert_state(HT, 0).items()}
    legacy = str(tmp_path / "legacy.pt")
    torch.save({"args": argparse.Namespace(arch="hubert", label_rate=50), "model": sd}, legacy)
    assert sorted(W.load_checkpoints(hubert_path=legacy)["hubert"]) == sorted(sd)
    for gone in ("encoder.layers.1.fc2.bias", "final_proj.weight", "encoder.pos_conv.0.weight_g"):
        path = str(tmp_path / "missing.pt")
        torch.save({"model": {k: v for k, v in sd.items() if k != gone}}, path)
        with pytest.raises(ValueError, match=gone.replace(".", r"\.")):
            W.load_checkpoints(hubert_path=path)
    path = str(tmp_path / "no_model.pt")
    torch.save({"state_dict": sd}, path)
    with pytest.raises(ValueError, match="model"):
        W.load_checkpoints(hubert_path=path)
    path = str(tmp_path / "pickle.pt")
    torch.save({"args": SimpleNamespace(arch="hubert"), "model": sd}, path)  # a class that is not allow-listed
    with pytest.raises(Exception, match="(?i)weights_only|unsupported global|allowlist"):
        W.load_checkpoints(hubert_path=path)  # never a full unpickle


# ---------------------------------------------------------------------------- CLI
def _hubert_config(tmp_path, **top):
    cfg = copy.deepcopy(C.load_config().to_dict())
    cfg.pop("config_dir")
    cfg["mapper"]["content_feature"] = ["contentvec"]
    cfg["mapper"]["input_content_dim"] = {"contentvec": 256}
    for name in ("singer_file", "stats_file"):
        cfg[name] = os.path.join(C.CONFIG_DIR, cfg[name])
    cfg.update(top)
    path = str(tmp_path / "config.json")
    with open(path, "w") as fh:
        json.dump(cfg, fh)
    return path


def test_cli_names_hubert_ckpt_when_the_weights_are_missing(tmp_path):
    """A HuBERT configuration without --hubert-ckpt (and no contentVec_model in the config) and without
    --random-weights ends before any engine is built, also when the other three checkpoints are named."""
    cfg = _hubert_config(tmp_path)
    for extra in ([], ["--mapper-ckpt", "m.pt", "--vocoder-ckpt", "v.pt", "--whisper-ckpt", "w.pt"]):
        with pytest.raises(SystemExit) as exc:
            I.main(["--wav", "a.wav", "--config", cfg] + extra)
        assert "--hubert-ckpt" in str(exc.value.code) and "contentvec" in str(exc.value.code)
    assert "--hubert-ckpt" in I.main.__globals__["__doc__"]
