"""CPU: the host half of the ragged Whisper stage. svc_whisper_windows and svc_whisper_content_ragged are declared,
bound and exported; the window count is the pipeline's own rule; a NULL context is rejected before any HIP call (no GPU
needed, as in test_hubert_ragged_host.py); and SVCPipeline.ragged_content's Whisper branch is one whisper_content call
on an engine that has it, the two-group form otherwise."""
import ctypes
import os
import re

import pytest

from svc_inference_pipeline_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry_points():
    txt = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    lib = _lib.load()
    assert re.search(r"int svc_whisper_windows\(", txt)
    assert re.search(r"svc_status svc_whisper_content_ragged\(", txt)
    for name in ("svc_whisper_windows", "svc_whisper_content_ragged"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    flat = " ".join(txt.split())
    assert "int svc_whisper_windows(int frames);" in flat
    assert ("svc_status svc_whisper_content_ragged(svc_ctx* ctx, const float* wav16, int B, int64_t n_samples, "
            "const int64_t* utt_samples, int T, const int32_t* frames, void* out16, int ld_out, float* feats_out, "
            "void* stream);") in flat
    # svc_whisper_encode keeps its prototype; additions only
    assert ("svc_status svc_whisper_encode(svc_ctx* ctx, const float* wav16k, int B, int64_t n_samples, float* feats, "
            "void* stream);") in flat
    res, args = _lib.PROTOTYPES["svc_whisper_content_ragged"]
    assert res is ctypes.c_int and len(args) == 11
    assert _lib.PROTOTYPES["svc_whisper_windows"] == (ctypes.c_int, [ctypes.c_int])
    assert lib.svc_abi_version() == 3


def test_whisper_windows_known_answers_and_pipeline_rule():
    from svc_inference_pipeline_amd.pipeline import MAX_MAPPED, WINDOW_MEL_FRAMES
    win = _lib.load().svc_whisper_windows
    for frames, n in ((0, -1), (1, 1), (2812, 1), (2813, 2), (5610, 2), (5611, 3), (16875, 7)):
        assert win(frames) == n, frames
    assert win(-5) == -1
    for T in range(1, 20001):
        assert win(T) == (1 if T <= MAX_MAPPED else -(-T // WINDOW_MEL_FRAMES)), T


def test_null_context_is_rejected_before_any_hip_call():
    keep = ctypes.create_string_buffer(1 << 12)  # a host stand-in: a failing call never reads it
    p = ctypes.cast(keep, ctypes.c_void_p)
    lib = _lib.load()
    st = lib.svc_whisper_content_ragged(None, p, 1, 1000, (ctypes.c_int64 * 1)(1000), 5, (ctypes.c_int32 * 1)(5), p, 8,
                                        None, None)
    err = lib.svc_last_error().decode()
    assert st == 1, (st, err)
    assert "null context" in err, err
    with pytest.raises(_lib.SVCError):
        _lib.check(st)


def test_ragged_content_is_one_whisper_content_call():
    """SVCPipeline.ragged_content's Whisper branch on a recording stand-in engine: one whisper_content call with the
    padded batch, its sample counts and frames == T_b, straight into the content buffer, and no whisper_encode /
    map_content call; whisper_ragged=False (and an engine without the entry point) keeps the two-group form."""
    import threading
    from types import SimpleNamespace

    import torch

    from svc_inference_pipeline_amd import config as C
    from svc_inference_pipeline_amd.pipeline import SVCPipeline

    calls = []
    cfg = C.load_config()
    cfg.mapper.content_feature = ["whisper"]
    cfg.mapper.input_content_dim["whisper"] = 8
    seen = {}

    def whisper_content(w16, n_samples, frames, T, out=None, return_feats=False):
        calls.append(("content", tuple(w16.shape), list(n_samples), list(frames), T))
        seen["w16"] = w16.clone()
        assert out is not None and tuple(out.shape) == (w16.shape[0], T, 8)
        for b, t in enumerate(frames):
            out[b, :t] = w16[b, 0].half()
            out[b, t:] = 0
        return out

    def whisper_encode(w16):
        calls.append(("encode", tuple(w16.shape)))
        return w16[:, :1, None].expand(-1, 1500, 8).float().contiguous()

    def map_content(feats, T, rule="whisper", out=None, frames=None, src_rows=None):
        calls.append(("map", T, rule))
        assert out is None and frames is None and src_rows is None
        return feats[:, :1].expand(-1, T, -1).half().clone()

    eng = SimpleNamespace(cfg=cfg, lock=threading.RLock(), content_dtype=torch.float16, ragged_whisper=True,
                          whisper_content=whisper_content, whisper_encode=whisper_encode, map_content=map_content)
    T_b = [94, 2900, 188]
    lens16 = [16000, 494934, 32000]
    w16 = [torch.full((n,), float(i + 1)) for i, n in enumerate(lens16)]
    T = max(T_b)
    pipe = SVCPipeline(eng)
    assert pipe.whisper_ragged and SVCPipeline(eng, whisper_ragged=True).whisper_ragged
    out = pipe.ragged_content(w16, T_b, T)
    assert calls == [("content", (3, 494934), lens16, T_b, T)]
    for i, n in enumerate(lens16):  # the padded batch: each clip's samples, zeros after them
        assert bool((seen["w16"][i, :n] == float(i + 1)).all()) and not seen["w16"][i, n:].any()
    assert out.shape == (3, T, 8) and out.dtype == torch.float16
    for i in range(3):
        assert bool((out[i, :T_b[i]] == float(i + 1)).all()) and not out[i, T_b[i]:].any()

    plain = SimpleNamespace(**{k: v for k, v in vars(eng).items() if k not in ("ragged_whisper", "whisper_content")})
    with pytest.raises(ValueError, match="whisper_ragged=True"):  # asked for explicitly: an error, no quiet fall-back
        SVCPipeline(plain, whisper_ragged=True)
    for old in (SVCPipeline(eng, whisper_ragged=False), SVCPipeline(plain)):
        assert not old.whisper_ragged
        del calls[:]
        out2 = old.ragged_content(w16, T_b, T)
        assert not any(c[0] == "content" for c in calls)
        # two groups: the one-window clips as one batch, the long clip as two windows of 478 720 samples
        assert [c[1] for c in calls if c[0] == "encode"] == [(2, 32000), (2, 478720)]
        assert [c[1] for c in calls if c[0] == "map"] == [188, 2805]
        assert torch.equal(out2, out)
