"""GPU: ragged HuBERT / ContentVec batches in one padded pass (include/svc_hip.h
"Ragged batches"). svc_op_attention_ragged, svc_hubert_encode_ragged and svc_map_content_ragged compute every utterance
of a padded batch exactly as a clip of its own length: outputs are compared with torch.equal / np.array_equal against
the same entry points run on the clip alone, the rows past an utterance's end are zeros, and the padding the caller
leaves in the batch (NaN here) is never read. Against the CPU oracle the tolerances are those of test_gpu_hubert.py
(5e-3) and test_gpu_ops.py's attention tests (3e-3). Shapes cross the kernels' boundaries: 128-query blocks, 64-key
tiles, one frame."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import call, dev, ptr, rel_l2, stream  # noqa: E402
from oracle import models as OM  # noqa: E402
from oracle import noise as ON  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine, mel_frames  # noqa: E402

HT = W.HUBERT_DIMS["tiny-test"]
NAN = float("nan")

# ---------------------------------------------------------------------------- attention, op level
ATT_B, ATT_L, ATT_D = 5, 200, 128
ATT_LENS = [200, 129, 128, 64, 1]


def _i32(v):
    import ctypes
    return (ctypes.c_int32 * len(v))(*v)


def _att_ref(q, k, v):
    """f32 torch softmax attention of one clip [L, D] (head dim 64)"""
    L, D = q.shape
    H = D // 64
    sc = 64 ** -0.25
    qh = q.view(L, H, 64).permute(1, 0, 2) * sc
    kh = k.view(L, H, 64).permute(1, 2, 0) * sc
    vh = v.view(L, H, 64).permute(1, 0, 2)
    return (F.softmax(qh @ kh, dim=-1) @ vh).permute(1, 0, 2).reshape(L, D)


def _att_single(q, k, v):
    """svc_op_attention on one clip's own rows [Lb, D] (host tensors)"""
    Lb, D = q.shape
    out = torch.empty(Lb, D, device="cuda")
    qd, kd, vd = dev(q.contiguous()), dev(k.contiguous()), dev(v.contiguous())
    call("svc_op_attention", ptr(qd), ptr(kd), ptr(vd), 1, Lb, D, ptr(out), stream())
    return out.cpu()


def _check_ragged_attention(q, k, v, lens):
    """q, k, v host [B, L, D] (valid rows finite); the batch is run with NaN in every padding row"""
    B, L, D = q.shape
    qn, kn, vn = q.clone(), k.clone(), v.clone()
    for b, lb in enumerate(lens):
        for t in (qn, kn, vn):
            t[b, lb:] = NAN
    out = torch.empty(B * L, D, device="cuda")
    qd, kd, vd = (dev(t.reshape(B * L, D)) for t in (qn, kn, vn))
    call("svc_op_attention_ragged", ptr(qd), ptr(kd), ptr(vd), B, L, D, _i32(lens), ptr(out), stream())
    o = out.cpu().view(B, L, D)
    assert bool(torch.isfinite(o).all())
    for b, lb in enumerate(lens):
        one = _att_single(q[b, :lb], k[b, :lb], v[b, :lb])
        err = rel_l2(o[b, :lb].numpy(), _att_ref(q[b, :lb], k[b, :lb], v[b, :lb]).numpy())
        print(f"utterance {b} (L={lb}): rel-L2 {err:.2e}")
        assert torch.equal(o[b, :lb], one), b
        assert err < 3e-3, (b, err)
        assert not o[b, lb:].any(), b
    return o


def test_attention_ragged_matches_single_clips():
    g = torch.Generator().manual_seed(21)
    q, k, v = (torch.randn(ATT_B, ATT_L, ATT_D, generator=g) for _ in range(3))
    _check_ragged_attention(q, k, v, ATT_LENS)
    # lens = NULL is svc_op_attention
    n = ATT_B * ATT_L
    qd, kd, vd = (dev(t.reshape(n, ATT_D)) for t in (q, k, v))
    a, b = torch.empty(n, ATT_D, device="cuda"), torch.empty(n, ATT_D, device="cuda")
    call("svc_op_attention_ragged", ptr(qd), ptr(kd), ptr(vd), ATT_B, ATT_L, ATT_D, None, ptr(a), stream())
    call("svc_op_attention", ptr(qd), ptr(kd), ptr(vd), ATT_B, ATT_L, ATT_D, ptr(b), stream())
    assert torch.equal(a, b)


def test_attention_ragged_rescale_in_tail():
    """The Lb = 129 utterance's last key is an outlier every query leans towards: the deferred rescale fires in its
    third tile, a tail tile holding that one valid key (63 masked).
    That it fires is checked here, not assumed: the kernel makes P = 2^(s - m) against the running max m of the first
    128 keys and rounds it to f16, and moves the max only when a tile's P column sum passes 2^14. With k_last = 12 k and
    q = q0 + 6 k, s_last - m is about 12 * 6 * |k|^2 / 8 * log2(e) ~ 800 in exp2 units for |k|^2 ~ 64 (asserted below
    to exceed 16 for every query and head, i.e. P > 2^16 > 2^14), so every query column of that tile takes the
    rescale path; without it P overflows f16 and the finite / rel-L2 assertions fail."""
    g = torch.Generator().manual_seed(22)
    q, k, v = (torch.randn(ATT_B, ATT_L, ATT_D, generator=g) for _ in range(3))
    b, lb = 1, ATT_LENS[1]
    assert lb == 129
    k[b, lb - 1] *= 12.0
    q[b] = q[b] + 0.5 * k[b, lb - 1:lb]
    H = ATT_D // 64
    s2 = torch.einsum("qhd,khd->hqk", q[b, :lb].view(lb, H, 64), k[b, :lb].view(lb, H, 64)) / 8.0 * 1.4426950408889634
    gap = (s2[:, :, lb - 1] - s2[:, :, :lb - 1].max(dim=-1).values).min().item()
    print(f"score of the last key above the running max of the first 128, exp2 units, min over queries: {gap:.1f}")
    assert gap > 16.0
    _check_ragged_attention(q, k, v, ATT_LENS)


# ---------------------------------------------------------------------------- encoder
_ORACLE = {}


def _clip(seed, n):
    w = ON.synth_clip(seed, n / 16000.0 + 0.01, 16000)[:n].astype(np.float32)
    assert w.shape == (n,)
    return w


def _oracle_feats(tag, sd, wav, layer):
    """CPU oracle features of one clip, computed once per (weights, clip) and shared"""
    key = (tag, wav.shape[0], float(wav[:16].sum()))
    if key not in _ORACLE:
        with torch.no_grad():
            _ORACLE[key] = OM.hubert_content(sd, torch.from_numpy(wav)[None], layer)[0].numpy()
    return _ORACLE[key]


def _check_ragged_encoder(e, tag, sd, layer, ns, oracle=True):
    clips = [_clip(50 + i, n) for i, n in enumerate(ns)]
    frames = [W.hubert_frames(n) for n in ns]
    big = torch.full((len(ns), max(ns)), NAN)
    for i, w in enumerate(clips):
        big[i, :ns[i]] = torch.from_numpy(w)
    feats = e.hubert_encode(big.cuda(), n_samples=ns).cpu()
    assert feats.shape[:2] == (len(ns), max(frames))
    for i, n in enumerate(ns):
        one = e.hubert_encode(dev(clips[i][None])).cpu()[0]
        assert one.shape[0] == frames[i]
        assert torch.equal(feats[i, :frames[i]], one), (i, n)
        assert not feats[i, frames[i]:].any(), (i, n)
        if oracle:
            err = rel_l2(feats[i, :frames[i]].numpy(), _oracle_feats(tag, sd, clips[i], layer))
            print(f"{tag} clip {i} ({n} samples, {frames[i]} frames): rel-L2 {err:.2e}")
            assert err < 5e-3, (i, n, err)
    return frames


TINY_NS = [64080, 41360, 41040, 20560, 720, 400]


@pytest.fixture(scope="module")
def hsd():
    return W.make_hubert_state(HT, 0)


@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_encoder_ragged_tiny(hsd, split):
    assert [W.hubert_frames(n) for n in TINY_NS] == [200, 129, 128, 64, 2, 1]
    e = SVCEngine(C.load_config(), 0, hubert_state=hsd, hubert_output_layer=HT["output_layer"], content_split=split)
    try:
        _check_ragged_encoder(e, "tiny", hsd, HT["output_layer"], TINY_NS)
        w = dev(np.stack([_clip(60 + b, 20560) for b in range(2)]))
        assert torch.equal(e.hubert_encode(w, n_samples=None), e.hubert_encode(w))
        a = torch.empty(2, 64, HT["final_dim"], device="cuda")
        _lib.call("svc_hubert_encode_ragged", e._ctx, ptr(w), 2, 20560, None, ptr(a), stream())
        assert torch.equal(a, e.hubert_encode(w))
    finally:
        e.close()


def test_encoder_ragged_bf16_operands(hsd):
    """operands="bf16" runs the ragged attention's bfloat16 instance (and bf16 zero rows / operands everywhere else):
    the same exact assertions against the clip alone. No oracle bound here: what bfloat16 operands cost in accuracy
    is pinned by test_gpu_configs.py for the non-ragged encoder, which each clip equals bit for bit."""
    e = SVCEngine(C.load_config(), 0, hubert_state=hsd, hubert_output_layer=HT["output_layer"], operands="bf16")
    try:
        _check_ragged_encoder(e, "tiny-bf16", hsd, HT["output_layer"], TINY_NS, oracle=False)
    finally:
        e.close()


def test_encoder_ragged_contentvec_dims():
    """768 wide, 12 heads, 16 positional-conv groups of 48, 512-channel extractor"""
    d = W.HUBERT_DIMS["contentvec"]
    sd = W.make_hubert_state(d, 1)
    e = SVCEngine(C.load_config(), 0, hubert_state=sd, hubert_output_layer=d["output_layer"])
    try:
        assert _check_ragged_encoder(e, "contentvec", sd, d["output_layer"], [41360, 20880, 720]) == [129, 65, 2]
    finally:
        e.close()


# ---------------------------------------------------------------------------- mapping
@pytest.fixture(scope="module")
def engine(hsd):
    e = SVCEngine(C.load_config(), 0, hubert_state=hsd, hubert_output_layer=HT["output_layer"])
    yield e
    e.close()


def test_map_ragged_exact(engine, golden):
    g = golden("hubert_map")
    cases = [(int(s), int(t)) for s, t in g["cases"]]
    B, S, T, D = len(cases), max(s for s, _ in cases), max(t for _, t in cases), 24
    feats = torch.full((B, S, D), NAN)
    for b, (s, t) in enumerate(cases):
        feats[b, :s] = torch.from_numpy(g[f"raw_{s}_{t}"])
    buf = torch.full((B, T, 40), 7.0, device="cuda", dtype=torch.float16)
    engine.map_content(feats.cuda(), T, rule="hubert", out=buf[:, :, 8:32], frames=[t for _, t in cases],
                       src_rows=[s for s, _ in cases])
    o = buf.cpu().numpy()
    for b, (s, t) in enumerate(cases):
        exp = g[f"out_{s}_{t}"].astype(np.float32).astype(np.float16)
        assert np.array_equal(o[b, :t, 8:32], exp), (s, t)
        assert not o[b, t:, 8:32].any(), (s, t)
    assert np.all(o[:, :, :8] == 7.0) and np.all(o[:, :, 32:] == 7.0)
    # one utterance the reference would exit() on fails the batch, naming it
    for s, t, _ in g["exits"]:
        bad = cases[:2] + [(int(s), int(t))]
        with pytest.raises(_lib.SVCError, match=r"utterance 2.*utils/hubert\.py"):
            engine.map_content(torch.zeros(3, 499, 4, device="cuda"), max(t for _, t in bad), rule="hubert",
                               frames=[t for _, t in bad], src_rows=[s for s, _ in bad])


def test_map_ragged_whisper_rule(engine):
    """mode 0: each utterance's rows equal map_content at the batch length (the Whisper rule is row-wise)"""
    g = torch.Generator().manual_seed(31)
    T_b = [935, 400, 93, 1]
    S_b = [499, 215, 50, 1]   # T * 8 // 15 + 1 source rows at least
    feats = torch.randn(4, 499, 24, generator=g)
    full = engine.map_content(feats.cuda(), max(T_b)).cpu()
    for b, s in enumerate(S_b):
        feats[b, s:] = NAN
    rag = engine.map_content(feats.cuda(), max(T_b), frames=T_b, src_rows=S_b).cpu()
    for b, t in enumerate(T_b):
        assert torch.equal(rag[b, :t], full[b, :t]), b
        assert not rag[b, t:].any(), b
    with pytest.raises(_lib.SVCError, match="utterance 1"):
        engine.map_content(feats.cuda(), max(T_b), frames=T_b, src_rows=[499, 213, 50, 1])


# ---------------------------------------------------------------------------- pipeline and server
PIPE_N16 = [64080, 41360, 20560]


@pytest.fixture(scope="module")
def cv_pipeline(hsd):
    """the ContentVec configuration of test_gpu_hubert.py's test_contentvec_pipeline_plms, its three clips and each
    clip's single conversion (the reference the ragged paths are compared with)"""
    cfg = C.load_config()
    cfg.mapper.content_feature = ["contentvec"]
    cfg.mapper.input_content_dim["contentvec"] = HT["final_dim"]
    e = SVCEngine(cfg, 0, mapper_state=W.make_mapper_state(cfg.mapper, 0),
                  vocoder_state=W.make_vocoder_state(cfg.vocoder, 0), hubert_state=hsd,
                  hubert_output_layer=HT["output_layer"])
    w16 = [dev(_clip(80 + i, n)) for i, n in enumerate(PIPE_N16)]
    w24 = [dev(ON.synth_clip(80 + i, n * 1.5 / 24000.0 + 0.01, 24000)[:n * 3 // 2].astype(np.float32))
           for i, n in enumerate(PIPE_N16)]
    pipe = SVCPipeline(e)
    singers = [2, 0, 3]
    single = [pipe.convert(w24[i][None], w16[i][None], dev(np.array([singers[i]]), torch.int32), speedup=250, seed=7,
                           utt_ids=dev(np.array([30 + i]), torch.int32), wav16_float=w16[i][None]).wav[0].clone()
              for i in range(3)]
    yield e, w24, w16, singers, single
    e.close()


def test_pipeline_ragged_one_pass(cv_pipeline):
    e, w24, w16, singers, single = cv_pipeline
    pipe = SVCPipeline(e)
    assert pipe.hubert_ragged
    ids = [30, 31, 32]
    _lib.profile_enable(True)
    outs = pipe.convert_ragged(w24, w16, singers, wavs16_float=w16, speedup=250, seed=7, utt_ids=ids)
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    # (the site label stays on the launches that follow the GEMM: the GroupNorm is counted apart)
    conv0 = sum(v["launches"] for k, v in prof.items()
                if k.endswith("@hubert.conv0") and not k.startswith("groupnorm_gelu"))
    assert sum(v["launches"] for k, v in prof.items() if k.startswith("groupnorm_gelu")) == 1
    att = sum(v["launches"] for k, v in prof.items() if k.startswith("attention"))
    print(f"hubert.conv0 launches {conv0}, attention launches {att}")
    for i in range(3):
        assert outs[i].shape[0] == mel_frames(int(w24[i].shape[0])) * 256
        assert torch.equal(outs[i], single[i]), i
    assert conv0 == 1 and att == HT["output_layer"]
    # the per-bucket form gives the same waveforms
    old = SVCPipeline(e, hubert_ragged=False).convert_ragged(w24, w16, singers, wavs16_float=w16, speedup=250, seed=7,
                                                             utt_ids=ids)
    for i in range(3):
        assert torch.equal(old[i], single[i]), i


def test_server_ragged_contentvec(cv_pipeline):
    from svc_inference_pipeline_amd.serving import SVCServer
    e, w24, w16, singers, single = cv_pipeline
    with SVCServer(SVCPipeline(e), max_batch=4, max_wait_s=0.2, speedup=250, seed=7) as srv:
        futs = [srv.submit(w24[i], w16[i], singer=singers[i], utt_id=30 + i, wav16_float=w16[i]) for i in range(3)]
        outs = [f.result(timeout=120) for f in futs]
    assert sorted(u for b in srv.batches for u in b) == [30, 31, 32]
    for i in range(3):
        assert torch.equal(outs[i], single[i]), i
