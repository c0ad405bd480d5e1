"""CPU: the host half of the ragged HuBERT / ContentVec stage. svc_hubert_encode_ragged, svc_map_content_ragged and
svc_op_attention_ragged are declared, bound and exported, and reject a bad length table or argument with a message
before any HIP call (no GPU needed, as in test_load_pcm_host.py)."""
import ctypes
import os
import re

import pytest

from svc_inference_pipeline_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("svc_hubert_encode_ragged", "svc_map_content_ragged", "svc_op_attention_ragged")


def test_header_declares_and_library_exports_the_entry_points():
    txt = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"svc_status " + name + r"\(", txt), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    flat = " ".join(txt.split())
    assert ("svc_status svc_hubert_encode_ragged(svc_ctx* ctx, const float* wav16k, int B, int64_t n_samples, "
            "const int64_t* utt_samples, float* feats, void* stream);") in flat
    assert ("svc_status svc_map_content_ragged(svc_ctx* ctx, const float* feats, int B, int src_rows, "
            "const int32_t* utt_src_rows, int T, const int32_t* frames, int D, int mode, void* out_f16, int ld_out, "
            "void* stream);") in flat
    assert ("svc_status svc_op_attention_ragged(const float* q, const float* k, const float* v, int B, int L, int D, "
            "const int32_t* lens, float* out, void* stream);") in flat
    # svc_hubert_encode keeps its prototype; additions only
    assert ("svc_status svc_hubert_encode(svc_ctx* ctx, const float* wav16k, int B, int64_t n_samples, float* feats, "
            "void* stream);") in flat
    assert lib.svc_abi_version() == 3


def _buf():
    keep = ctypes.create_string_buffer(1 << 16)  # a host stand-in: a failing call never reads it
    return keep, ctypes.cast(keep, ctypes.c_void_p)


def _encode(ctx=True, B=2, n=1000, utt=(1000, 400)):
    keep, p = _buf()
    table = (ctypes.c_int64 * len(utt))(*utt)
    lib = _lib.load()
    st = lib.svc_hubert_encode_ragged(p if ctx else None, p, B, n, table, p, None)
    return st, lib.svc_last_error().decode()


def _map(ctx=True, B=2, src_rows=10, utt_src=(10, 5), T=18, frames=(18, 9), D=8, mode=1, ld_out=8):
    keep, p = _buf()
    lib = _lib.load()
    st = lib.svc_map_content_ragged(p if ctx else None, p, B, src_rows, (ctypes.c_int32 * len(utt_src))(*utt_src), T,
                                    (ctypes.c_int32 * len(frames))(*frames), D, mode, p, ld_out, None)
    return st, lib.svc_last_error().decode()


def _attention(B=2, L=10, D=64, lens=(10, 3)):
    keep, p = _buf()
    lib = _lib.load()
    st = lib.svc_op_attention_ragged(p, p, p, B, L, D, (ctypes.c_int32 * len(lens))(*lens), p, None)
    return st, lib.svc_last_error().decode()


@pytest.mark.parametrize("fn,kw,msg", [
    (_encode, dict(ctx=False), "null context"),
    (_encode, dict(utt=(1000, 399)), "utterance 1: 399 samples"),
    (_encode, dict(utt=(1001, 400)), "utterance 0: 1001 samples"),
    (_encode, dict(utt=(-1, 400)), "utterance 0: -1 samples"),
    (_encode, dict(B=0), "B=0"),
    (_map, dict(ctx=False), "null context"),
    (_map, dict(mode=2), "mode 2"),
    (_map, dict(utt_src=(11, 5)), "utterance 0: 11 of 10 source rows"),
    (_map, dict(utt_src=(10, 0)), "utterance 1: 0 of 10 source rows"),
    (_map, dict(frames=(19, 9)), "utterance 0: 10 of 10 source rows, 19 of 18 frames"),
    (_map, dict(frames=(18, 0)), "utterance 1: 5 of 10 source rows, 0 of 18 frames"),
    (_map, dict(frames=(18, 13)), "utterance 1: 5 content frames map to 9 rows but T=13"),
    (_map, dict(mode=0, frames=(18, 9), utt_src=(10, 4)), "utterance 1: T=9 src_rows=4"),
    (_map, dict(ld_out=4), "ld_out=4"),
    (_attention, dict(D=96), "D=96"),
    (_attention, dict(D=0), "D=0"),
    (_attention, dict(lens=(10, 0)), "utterance 1: length 0 outside 1..10"),
    (_attention, dict(lens=(11, 3)), "utterance 0: length 11 outside 1..10"),
    (_attention, dict(B=0, lens=(1,)), "B=0"),
])
def test_bad_arguments_are_rejected_before_any_hip_call(fn, kw, msg):
    st, err = fn(**kw)
    assert st == 1, (st, err)
    assert msg in err, err
    with pytest.raises(_lib.SVCError):
        _lib.check(st)


def test_ragged_content_is_one_encode_and_one_map():
    """SVCPipeline.ragged_content's HuBERT branch on a recording stand-in engine: one padded encode with the sample
    counts and one map with the frame tables, straight into the type's column slice; hubert_ragged=False (and an engine
    without the length-taking entry points) keeps one encode per exact length."""
    import threading
    from types import SimpleNamespace

    import torch

    from svc_inference_pipeline_amd import config as C
    from svc_inference_pipeline_amd.pipeline import SVCPipeline

    calls = []
    cfg = C.load_config()
    cfg.mapper.content_feature = ["contentvec"]
    cfg.mapper.input_content_dim["contentvec"] = 8
    frames_of = lambda n: (n - 400) // 320 + 1  # noqa: E731

    def encode(w16, n_samples=None):
        calls.append(("encode", tuple(w16.shape), None if n_samples is None else list(n_samples)))
        return w16[:, :1, None].expand(-1, frames_of(w16.shape[1]), 8).float().contiguous()

    def map_content(feats, T, rule="whisper", out=None, frames=None, src_rows=None):
        calls.append(("map", T, rule, None if frames is None else list(frames),
                      None if src_rows is None else list(src_rows)))
        res = feats[:, :1].expand(-1, T, -1).half().clone()
        for b, t in enumerate(frames or []):
            res[b, t:] = 0
        if out is None:
            return res
        out.copy_(res)
        return out

    eng = SimpleNamespace(cfg=cfg, lock=threading.RLock(), content_dtype=torch.float16, ragged_hubert=True,
                          hubert_encode=encode, map_content=map_content, hubert_frames=frames_of)
    lens16 = [16000, 32000, 16001]
    w16 = [torch.full((n,), float(i + 1)) for i, n in enumerate(lens16)]
    T_b = [94, 188, 94]
    out = SVCPipeline(eng).ragged_content(w16, T_b, 188)
    assert calls == [("encode", (3, 32000), lens16), ("map", 188, "hubert", T_b, [49, 99, 49])]
    for i in range(3):
        assert bool((out[i, :T_b[i]] == float(i + 1)).all()) and not out[i, T_b[i]:].any()
    assert SVCPipeline(eng).hubert_ragged and SVCPipeline(eng, hubert_ragged=True).hubert_ragged
    plain = SimpleNamespace(**{**vars(eng), "ragged_hubert": False})
    with pytest.raises(ValueError, match="hubert_ragged=True"):  # asked for explicitly: an error, no quiet fall-back
        SVCPipeline(plain, hubert_ragged=True)
    for pipe in (SVCPipeline(eng, hubert_ragged=False), SVCPipeline(plain)):
        assert not pipe.hubert_ragged
        del calls[:]
        out2 = pipe.ragged_content(w16, T_b, 188)
        assert sorted(c[1] for c in calls if c[0] == "encode") == [(1, 16000), (1, 16001), (1, 32000)]
        assert all(c[2] is None for c in calls if c[0] == "encode")
        assert torch.equal(out2, out)


def test_hubert_mismatch_message_is_the_non_ragged_one():
    """the > 3 frame mismatch names utils/hubert.py as svc_map_content_ex does, plus the utterance"""
    st, err = _map(frames=(18, 13))
    assert st == 1 and err.startswith("content_map_hubert:") and "utils/hubert.py:114-120" in err
