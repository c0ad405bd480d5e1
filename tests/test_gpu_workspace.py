"""GPU: every stage sizes its workspace by laying its own buffers out twice (csrc/arena.h Arena::plan), so a fresh
context runs its first call at exactly the counted capacity, with no slack behind the last buffer.

Each stage runs on engine A at a small shape, at a shape that needs a larger workspace, and at the small shape again;
a fresh engine B runs the large shape only, so its arena is exactly as large as that call counts. The first and third
outputs on A are bit-identical (a call's result does not depend on the arena having grown in between), A's large output
is bit-identical to B's (nor on what the arena held before), and memory()[1] never decreases. Small and large: B = 1
then 3, about 0.3 s then 1 s of audio, 20 then 40 frames (20 frames is the vocoder fade-out's minimum), and at least 400
samples for HuBERT. The op-level entry points share one process-wide context, so they have no fresh engine B: their
large shape runs before and after the small one instead. The feature stages (f0, f0_pyin) have a workspace of their own,
which memory() does not report."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import call, dev, ptr, stream  # noqa: E402
from oracle import noise as ON  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine, mel_frames  # noqa: E402

TINY = W.WHISPER_DIMS["tiny-test"]
HT = W.HUBERT_DIMS["tiny-test"]
SMALL = dict(B=1, sec=0.3, T=20)
LARGE = dict(B=3, sec=1.0, T=40)


@pytest.fixture(scope="module")
def cfg():
    c = C.load_config()
    c.mapper.input_content_dim["whisper"] = TINY["n_audio_state"]
    return c


@pytest.fixture(scope="module")
def states(cfg):
    return dict(whisper_state=W.make_whisper_state(TINY, 0), hubert_state=W.make_hubert_state(HT, 0),
                mapper_state=W.make_mapper_state(cfg.mapper, 0), vocoder_state=W.make_vocoder_state(cfg.vocoder, 0))


def _wav(shape, fs, seed):
    n = int(shape["sec"] * fs)
    return dev(np.stack([ON.synth_clip(seed + b, shape["sec"], fs)[:n] for b in range(shape["B"])]).astype(np.float32))


def _randn(seed, *size, dtype=torch.float32):
    return torch.randn(*size, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def _bits(out):
    torch.cuda.synchronize()
    return [t.cpu() for t in (out if isinstance(out, tuple) else (out,))]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and
                                    bool((x.view(torch.uint8) == y.view(torch.uint8)).all()) for x, y in zip(a, b))


def _check(cfg, states, needs, run):
    """run(engine, shape) -> the stage's output tensor(s); engines are built from the states named in `needs`"""
    kw = {k: states[k] for k in needs}
    if "hubert_state" in kw:
        kw["hubert_output_layer"] = HT["output_layer"]
    a, b = SVCEngine(cfg, 0, **kw), SVCEngine(cfg, 0, **kw)
    try:
        mem = [a.memory()[1]]
        outs = []
        for shape in (SMALL, LARGE, SMALL):
            outs.append(_bits(run(a, shape)))
            mem.append(a.memory()[1])
        only_large = _bits(run(b, LARGE))
        print("workspace bytes on A:", mem, "on B:", b.memory()[1])
        assert all(x <= y for x, y in zip(mem, mem[1:])), mem
        assert mem[3] == mem[2] == b.memory()[1]  # the small call left the arena alone; B holds what the large call counts
        assert _same(outs[0], outs[2]), "small shape: first and third call differ"
        assert _same(outs[1], only_large), "large shape differs between a grown and a fresh arena"
    finally:
        a.close()
        b.close()


def test_whisper_encode(cfg, states):
    _check(cfg, states, ["whisper_state"], lambda e, s: e.whisper_encode(_wav(s, 16000, 10)))


@pytest.mark.parametrize("ragged", [False, True])
def test_hubert_encode(cfg, states, ragged):
    def run(e, s):
        wav = _wav(s, 16000, 20)
        n = wav.shape[1]
        return e.hubert_encode(wav, n_samples=[n, n * 9 // 16, 400][:s["B"]] if ragged else None)
    _check(cfg, states, ["hubert_state"], run)


def _cond_inputs(e, s, D):
    B, T = s["B"], s["T"]
    content = _randn(30, B, T, D, dtype=e.content_dtype)
    f0 = dev(np.stack([ON.synth_f0(1 + b, T) for b in range(B)]), torch.float64)
    energy = _randn(31, B, T).abs()
    singer = torch.ones(B, dtype=torch.int32).cuda()
    return content, f0, energy, singer


def test_condition(cfg, states):
    D = sum(v.shape[1] for k, v in states["mapper_state"].items() if ".content_" in k and k.endswith(".nn.weight"))
    _check(cfg, states, ["mapper_state"], lambda e, s: e.condition(*_cond_inputs(e, s, D)))


def test_diffsvc_eps(cfg, states):
    C_, nm = cfg.mapper.residual_channels, cfg.mapper.n_mel
    _check(cfg, states, ["mapper_state"],
           lambda e, s: e.diffsvc_eps(_randn(40, s["B"], s["T"], C_), _randn(41, s["B"], s["T"], nm), 500))


def test_diffsvc_sample_plms(cfg, states):
    C_, nm = cfg.mapper.residual_channels, cfg.mapper.n_mel
    _check(cfg, states, ["mapper_state"],
           lambda e, s: e.diffsvc_sample(_randn(50, s["B"], s["T"], C_), fast_inference=True, speedup=250,
                                         x_T=_randn(51, s["B"], s["T"], nm)))


@pytest.mark.parametrize("ragged", [False, True])
def test_bigvgan(cfg, states, ragged):
    nm = cfg.mapper.n_mel

    def run(e, s):
        x0 = _randn(60, s["B"], s["T"], nm).clamp(-1, 1)
        return e.bigvgan(x0, return_mel=True, frames=[s["T"], s["T"] - 7, 20][:s["B"]] if ragged else None)
    _check(cfg, states, ["mapper_state", "vocoder_state"], run)


def test_f0(cfg, states):
    def run(e, s):
        wav = _wav(s, cfg.fs, 70)
        return e.f0(wav, mel_frames(wav.shape[1], cfg.n_fft, cfg.hop_length))
    _check(cfg, states, [], run)


def test_f0_pyin(cfg, states):
    _check(cfg, states, [], lambda e, s: e.f0_pyin(_wav(s, cfg.fs, 80)))


def _op_sequence(run):
    """large, small, large, small on the op-level context: equal shapes give equal bits whatever ran in between"""
    outs = [_bits(run(s)) for s in (LARGE, SMALL, LARGE, SMALL)]
    assert _same(outs[0], outs[2]) and _same(outs[1], outs[3])


def test_op_attention():
    def run(s):
        B, L, D = s["B"], 5 * s["T"], 64 * s["B"]
        q, k, v = (_randn(90 + i, B * L, D) for i in range(3))
        out = torch.empty(B * L, D, device="cuda")
        call("svc_op_attention", ptr(q), ptr(k), ptr(v), B, L, D, ptr(out), stream())
        return out
    _op_sequence(run)


def test_op_conv1d():
    def run(s):
        B, T, Cin, Cout, k = s["B"], s["T"], 24 * s["B"], 40, 3
        x, w, b = _randn(95, B * T, Cin), _randn(96, Cout, Cin, k) / np.sqrt(Cin * k), _randn(97, Cout)
        y = torch.empty(B * T, Cout, device="cuda")
        call("svc_op_conv1d", ptr(x), B, T, Cin, ptr(w), ptr(b), Cout, k, 1, 1, 1, 0, ptr(y), stream())
        return y
    _op_sequence(run)
