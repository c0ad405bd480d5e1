"""GPU parity: shallow diffusion (Diff-SVC's k_step). The fused normalise + q_sample launch (csrc/elementwise.hip
q_sample) at op level against the float64 references of tests/shallow_ref.py, between guard zones as in
tests/test_gpu_sampler_ops.py; svc_mel_normalize; svc_diffsvc_sample_from against the oracle's samplers run with
steps = K; that k_step = steps is the existing sampler bit for bit; sub-streams; and the pipeline, copy-synthesis and
server on top."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sampler_ref as R  # noqa: E402
import shallow_ref as S  # noqa: E402
from gpu_util import call, dev, ptr, rel_l2, stream  # noqa: E402
from oracle import models as OM  # noqa: E402
from oracle import noise as ON  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.pipeline import SVCPipeline  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402
from svc_inference_pipeline_amd.serving import SVCServer  # noqa: E402
from test_gpu_sampler_ops import SEEDS, Buf, _check16, _ids, _init_noise, _step_noise  # noqa: E402

STEPS = 1000
KS = (1, 300, 1000)
SHAPES = [([3], 1, 100, 104), ([7, 0, 2 ** 31 - 1], 50, 100, 104), ([1, 4], 700, 100, 104), ([6, 2], 37, 80, 88)]
SHAPE_IDS = ["1x1x100", "3x50x100", "2x700x100", "2x37x80"]


@functools.lru_cache(maxsize=None)
def _stats(Cc=100):
    st = C.load_stats(C.load_config())
    return st["mel_min"][:Cc].copy(), st["mel_max"][:Cc].copy()


@functools.lru_cache(maxsize=None)
def _z_ref(seed, ids, T, Cc):
    """The float64 forward draw, computed once per (seed, shape) and shared by the K cases; never modified."""
    z = S.q_noise(seed, list(ids), T, Cc)
    z.setflags(write=False)
    return z


def _mel(ids, T, Cc, seed=0):
    """One float32 mel [T, C] per utterance id (so a batch can be reordered), normalised range about [-1.2, 1.2]."""
    mn, mx = _stats(Cc)
    return np.stack([S.mel_for_range(np.random.default_rng([seed, u % 9973, T, Cc]), (T, Cc), mn, mx) for u in ids])


def _q(mel, ids, coef, seed, ld16, z=None, frames=None, bf16=0, off=0):
    """svc_op_q_sample on guarded buffers -> float32 [B, T, C]. Checked here: guards of every buffer, inputs unchanged,
    the 16-bit copy the exact operand rounding of the float32 output with its pad columns untouched. off = 1 moves the
    float32 payloads (mel, z, x) one element off 16-byte alignment, which selects the one-channel kernel."""
    B, T, Cc = mel.shape
    mn, mx = _stats(Cc)
    m, x, h = Buf(mel.size, off=off, init=mel), Buf(mel.size, off=off), Buf(B * T * ld16, torch.int16)
    mnb, mxb = Buf(Cc, init=mn), Buf(Cc, init=mx)
    zb = Buf(mel.size, off=off, init=z) if z is not None else None
    idd = _ids(ids) if ids is not None else None
    fr = _ids(frames) if frames is not None else None
    assert m.t.data_ptr() % 16 == 4 * off and x.t.data_ptr() % 16 == 4 * off
    call("svc_op_q_sample", ptr(m.t), ptr(mnb.t), ptr(mxb.t), B, T, Cc, float(coef[0]), float(coef[1]),
         ptr(zb.t) if zb else None, seed, ptr(idd), ptr(fr), ptr(x.t), ptr(h.t), ld16, bf16, stream())
    out = x.host(B, T, Cc)
    assert x.guards_ok() and m.guards_ok() and mnb.guards_ok() and mxb.guards_ok()
    assert np.array_equal(m.host(B, T, Cc), mel) and np.array_equal(mnb.host(), mn) and np.array_equal(mxb.host(), mx)
    if zb:
        assert zb.guards_ok() and np.array_equal(zb.host(B, T, Cc), z)
    _check16(h, out.reshape(B * T, Cc), ld16, bf16)
    return out


def _q_draw(seed, ids, T, Cc, ld16):
    """The forward draw itself: coefficients (0, 1) make the output fma(0, y, 1 z) = z exactly."""
    return _q(_mel(ids, T, Cc), ids, (0.0, 1.0), seed, ld16)


# ------------------------------------------------------------------ 1. q_sample vs float64
@pytest.mark.parametrize("seed", SEEDS, ids=lambda s: "seed%x" % s)
@pytest.mark.parametrize("ids,T,Cc,ld16", SHAPES, ids=SHAPE_IDS)
def test_q_sample_vs_f64(ids, T, Cc, ld16, seed):
    """x_K = sqrt(ac) y + sqrt(1 - ac) z at K = 1, 300, 1000 with the device draw, element by element within
    sqrt(1 - ac) NOISE_ATOL + 8 u (1 + |y| + |sqrt(1 - ac) z|) of float64 (shallow_ref.q_sample_bound: the draw's own
    bound scaled, plus eight float32 roundings); with a given z the first term drops. The mel spans about [-1.2, 1.2]
    normalised (nothing is clamped). bfloat16 mode returns the same float32 bits; a payload one float off alignment (the
    one-channel kernel) returns the same bits as the aligned one (the four-channel kernel; C = 80 and 100 both qualify).
    Largest observed on MI355X: err / bound 0.35 with the device draw (B = 2, T = 700, seed 0x123456789ABCDEF0, K = 1)
    and 0.23 with a given z; largest |x_gpu - x_ref| 6.4e-7 (B = 2, T = 700, seed 0, K = 1000)."""
    sch = R.schedule()
    mel = _mel(ids, T, Cc)
    mn, mx = _stats(Cc)
    y = S.normalize_mel_channel(mel, mn, mx)
    if y.size > 1000:
        assert y.min() < -1.1 and y.max() > 1.1
    zr = _z_ref(seed, tuple(ids), T, Cc)
    worst = worst_abs = 0.0
    for K in KS:
        a, b = S.q_coeffs(sch, K)
        got = _q(mel, ids, (a, b), seed, ld16)
        assert np.isfinite(got).all()
        err = np.abs(got - S.q_sample(y, a, b, zr))
        ratio = float(np.max(err / S.q_sample_bound(y, a, b, zr, drawn=True)))
        print("q_sample B=%d T=%d C=%d seed=%x K=%d: max |d| %.3e, err/bound %.4f"
              % (len(ids), T, Cc, seed, K, float(err.max()), ratio))
        worst, worst_abs = max(worst, ratio), max(worst_abs, float(err.max()))
        assert ratio <= 1.0
        assert np.array_equal(_q(mel, ids, (a, b), seed, ld16, bf16=1), got)
        assert np.array_equal(_q(mel, ids, (a, b), seed, ld16, off=1, bf16=K & 1), got)
    # a given z: only the arithmetic term is left; no utt_ids needed
    a, b = S.q_coeffs(sch, 300)
    zg = np.random.default_rng([seed & 0xFFFF, T, Cc]).standard_normal(mel.shape).astype(np.float32)
    got = _q(mel, None, (a, b), seed, ld16, z=zg)
    err = np.abs(got - S.q_sample(y, a, b, zg))
    ratio = float(np.max(err / S.q_sample_bound(y, a, b, zg, drawn=False)))
    print("q_sample given z B=%d T=%d C=%d: max |d| %.3e, err/bound %.4f" % (len(ids), T, Cc, float(err.max()), ratio))
    assert ratio <= 1.0
    assert np.array_equal(_q(mel, None, (a, b), seed, ld16, z=zg, off=1), got)


def test_q_sample_needs_a_noise_source():
    """z NULL and utt_ids NULL: SVC_ERR_INVALID, nothing written."""
    mel = _mel([3], 2, 100)
    mn, mx = _stats(100)
    m, x, h = Buf(200, init=mel), Buf(200), Buf(208, torch.int16)
    mnb, mxb = Buf(100, init=mn), Buf(100, init=mx)
    with pytest.raises(_lib.SVCError, match="status 1:.*needs utt_ids"):
        call("svc_op_q_sample", ptr(m.t), ptr(mnb.t), ptr(mxb.t), 1, 2, 100, 0.5, 0.5, None, 0, None, None, ptr(x.t),
             ptr(h.t), 104, 0, stream())
    assert bool((x.full == x.sent).all()) and bool((h.full == h.sent).all())


# ------------------------------------------------------------------ 2. keying
def test_q_noise_keying():
    """Row b depends on utt_ids[b] alone; an element's draw not on T; and the forward draw (step word 0xFFFFFFFE) is
    none of the sampler's other draws: against x_T's and DDPM steps 0 and K - 1 fewer than 1e-3 of the elements are
    equal. The draw itself meets the x_T draw's bound against normal_f64."""
    seed, ids, K = 9, [7, 0, 2 ** 31 - 1], 300
    coef = S.q_coeffs(R.schedule(), K)
    mel = _mel(ids, 50, 100)
    a = _q(mel, ids, coef, seed, 104)
    b = _q(mel[[2, 0]], [ids[2], ids[0]], coef, seed, 104)
    assert np.array_equal(b[0], a[2]) and np.array_equal(b[1], a[0])
    assert np.array_equal(_q(mel[1:2], [0], coef, seed, 104)[0], a[1])
    mel64 = _mel(ids, 64, 100, seed=1)
    mel64[:, :50] = mel
    assert np.array_equal(_q(mel64, ids, coef, seed, 104)[:, :50], a)
    z = _q_draw(seed, ids, 50, 100, 104)
    assert float(np.max(np.abs(z - _z_ref(seed, tuple(ids), 50, 100)))) <= R.NOISE_ATOL
    assert not np.array_equal(z[0], z[1]) and not np.array_equal(z[0], z[2])
    others = {"xT": _init_noise(seed, ids, 50, 100, 104, std=1.0), "step0": _step_noise(seed, ids, 0, 50, 100, 104),
              "stepK-1": _step_noise(seed, ids, K - 1, 50, 100, 104)}
    for name, o in others.items():
        assert np.mean(z == o) < 1e-3, name


# ------------------------------------------------------------------ engine-level tests
TINY = W.WHISPER_DIMS["tiny-test"]


@pytest.fixture(scope="module")
def cfg():
    c = C.load_config()
    c.mapper.input_content_dim["whisper"] = TINY["n_audio_state"]
    return c


@pytest.fixture(scope="module")
def states(cfg):
    return dict(whisper=W.make_whisper_state(TINY, 0), mapper=W.make_mapper_state(cfg.mapper, 0),
                vocoder=W.make_vocoder_state(cfg.vocoder, 0))


@pytest.fixture(scope="module")
def engine(cfg, states):
    """Full-size mapper and vocoder, tiny Whisper (as tests/test_gpu_ragged.py builds it)."""
    e = SVCEngine(cfg, 0, whisper_state=states["whisper"], mapper_state=states["mapper"], vocoder_state=states["vocoder"])
    yield e
    e.close()


def _x_start(mel, ids, K, seed):
    """The noised start state of mel [B, T, 100] from svc_op_q_sample with the engine's statistics and coefficients."""
    return torch.from_numpy(_q(mel, ids, S.q_coeffs(R.schedule(), K), seed, 104)).cuda()


# ------------------------------------------------------------------ 3. ragged
def test_ragged_q_sample_and_mel_normalize(engine):
    """frames = [50, 37] in a T = 50 batch: each utterance's rows equal the utterance alone bit for bit, rows past 37 of
    the second are exactly 0 in the float32 output and in the 16-bit copy (_q checks the copy against the output); the
    same for svc_mel_normalize, which equals the float64 normaliser within 4 u (1 + |y|): the difference, the range and
    the quotient round (y + 1) / 2 three times, 3 u (1 + |y|) after the doubling, and the final - 1 rounds y once.
    Largest err / bound observed on MI355X: 0.62."""
    seed, ids, K = 5, [11, 4], 300
    coef = S.q_coeffs(R.schedule(), K)
    mel = _mel(ids, 50, 100)
    for bf16 in (0, 1):
        for off in (0, 1):
            rag = _q(mel, ids, coef, seed, 104, frames=[50, 37], bf16=bf16, off=off)
            assert np.array_equal(rag[0], _q(mel[:1], ids[:1], coef, seed, 104)[0])
            assert np.array_equal(rag[1, :37], _q(mel[1:, :37].copy(), ids[1:], coef, seed, 104)[0])
            assert np.all(rag[1, 37:] == 0) and not np.signbit(rag[1, 37:]).any()
    md = dev(mel)
    full = engine.mel_normalize(md).cpu().numpy()
    y = S.normalize_mel_channel(mel, *_stats(100))
    err = np.abs(full - y) / (4 * R.F32_U * (1 + np.abs(y)))
    print("mel_normalize: max err/bound %.4f" % float(err.max()))
    assert float(err.max()) <= 1.0
    assert full.min() < -1.1 and full.max() > 1.1  # not clamped
    rag = engine.mel_normalize(md, frames=[50, 37]).cpu().numpy()
    assert np.array_equal(rag[0], full[0]) and np.array_equal(rag[1, :37], full[1, :37])
    assert np.array_equal(rag[1, :37], engine.mel_normalize(md[1:, :37].contiguous()).cpu().numpy()[0])
    assert np.all(rag[1, 37:] == 0)
    # the normaliser is the noised kernel's y: coefficients (1, 0) with a zero z return it exactly
    assert np.array_equal(_q(mel, None, (1.0, 0.0), 0, 104, z=np.zeros_like(mel)), full)


# ------------------------------------------------------------------ 4. mel_normalize round trip
def test_mel_normalize_round_trip_through_bigvgan(engine, golden):
    """The de-normaliser in svc_bigvgan returns the mel that svc_mel_normalize was given, within test_bigvgan's 1e-4.
    Measured on MI355X: max |d| 4.8e-7."""
    mel = golden("bigvgan")["mel"]  # de-normalised [100, T]
    x = engine.mel_normalize(dev(mel.T[None].astype(np.float32)))
    wav, mel_d = engine.bigvgan(x, return_mel=True)
    err = float(np.max(np.abs(mel_d[0].cpu().numpy().T - mel)))
    print("mel_normalize -> bigvgan de-normaliser: max |d| %.3e" % err)
    assert err < 1e-4
    assert wav.shape == (1, mel.shape[1] * 256) and bool(torch.isfinite(wav).all())


# ------------------------------------------------------------------ 5. sampler vs oracle
@pytest.fixture(scope="module")
def oracle_den(cfg, states, golden):
    cond = torch.from_numpy(golden("conditioner_diffsvc")["cond"])
    table = W.step_embedding_table(STEPS)
    cache = {}
    den = lambda x, t: OM.diffsvc_forward(states["mapper"], cfg.mapper, x, cond, t, table, cp_cache=cache)  # noqa: E731
    return cond, den, OM.schedule_constants(C.noise_schedule(cfg.mapper))


def test_shallow_plms_vs_oracle(engine, oracle_den):
    """PLMS from K = 101 at interval 50 (i = 100, 50, 0: three iterations, four denoiser calls) against
    oracle.models.sample_plms(steps=101, interval=50) from the same start state (svc_op_q_sample's, so the draw
    tolerance does not enter), rel-L2 under test_plms_and_ddpm's 1e-3.
    Measured on MI355X: 5.9e-5."""
    cond, den, consts = oracle_den
    T = cond.shape[1]
    xs = _x_start(_mel([5], T, 100), [5], 101, seed=7)
    got = engine.diffsvc_sample(cond.cuda(), fast_inference=True, speedup=50, k_step=101, x_start=xs)
    ref = OM.sample_plms(den, xs.cpu(), 1, T, 101, 50, consts)
    r = rel_l2(got.cpu().numpy(), ref.numpy())
    print("shallow PLMS K=101 interval=50: rel_l2 %.3e" % r)
    assert bool(torch.isfinite(got).all()) and r < 1e-3


def test_shallow_ddpm_vs_oracle(engine, oracle_den, golden):
    """DDPM from K = 30 with injected oracle.noise.step_noise for steps 29 ... 0 against
    oracle.models.sample_ddpm(steps=30), rel-L2 under test_plms_and_ddpm's 1.5e-3.
    Measured on MI355X: 2.9e-5."""
    cond, den, consts = oracle_den
    T, K = cond.shape[1], 30
    seed = int(golden("samplers")["seed"])
    xs = _x_start(_mel([6], T, 100), [6], K, seed=7)
    noise = np.stack([ON.step_noise(seed, i, 1, T) for i in reversed(range(K))])
    got = engine.diffsvc_sample(cond.cuda(), fast_inference=False, k_step=K, x_start=xs, noise=dev(noise))
    ref = OM.sample_ddpm(den, xs.cpu(), 1, T, K, consts, lambda i: torch.from_numpy(ON.step_noise(seed, i, 1, T)))
    r = rel_l2(got.cpu().numpy(), ref.numpy())
    print("shallow DDPM K=30: rel_l2 %.3e" % r)
    assert bool(torch.isfinite(got).all()) and r < 1.5e-3


# ------------------------------------------------------------------ 6. the same loop
@pytest.fixture(scope="module")
def cond3(golden):
    g = golden("conditioner_diffsvc")
    return dev(np.concatenate([g["cond"], g["cond"][:, ::-1], 0.5 * g["cond"]], 0))


UTT3 = [5, 2 ** 31 - 1, 7]


def test_k_step_full_is_the_existing_sampler(engine, cond3):
    """k_step = steps with x_start = x_T is svc_diffsvc_sample bit for bit: PLMS (speedup 250) and DDPM with device
    noise, B = 3 with utterance ids."""
    B, T, _ = cond3.shape
    utt = dev(np.array(UTT3), torch.int32)
    xT = torch.from_numpy(_init_noise(9, UTT3, T, 100, 104)).cuda()
    for fast in (True, False):
        old = engine.diffsvc_sample(cond3, fast_inference=fast, speedup=250, x_T=xT, seed=9, utt_ids=utt)
        new = engine.diffsvc_sample(cond3, fast_inference=fast, speedup=250, k_step=STEPS, x_start=xT, seed=9,
                                    utt_ids=utt)
        assert bool(torch.isfinite(old).all()) and torch.equal(old, new), fast


def test_mel_src_path_equals_x_start_path(engine, cond3):
    """svc_diffsvc_sample_from(mel_src) = svc_diffsvc_sample_from(x_start = svc_op_q_sample(mel_src)) bit for bit, PLMS
    and DDPM with device noise, uniform and ragged: the op entry is what the sampler launches."""
    B, T, _ = cond3.shape
    utt = dev(np.array(UTT3), torch.int32)
    mel = _mel(UTT3, T, 100)
    for fast, K, sp in ((True, 300, 100), (False, 20, 10)):
        xs = _x_start(mel, UTT3, K, seed=9)
        for frames in (None, [T, T - 20, 40]):
            a = engine.diffsvc_sample(cond3, fast_inference=fast, speedup=sp, k_step=K, mel_src=dev(mel), seed=9,
                                      utt_ids=utt, frames=frames)
            b = engine.diffsvc_sample(cond3, fast_inference=fast, speedup=sp, k_step=K, x_start=xs, seed=9,
                                      utt_ids=utt, frames=frames)
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (fast, frames)
            if frames:
                assert bool((a[1, T - 20:] == 0).all()) and bool((a[2, 40:] == 0).all())
    # another K is another result
    at = [engine.diffsvc_sample(cond3, fast_inference=True, speedup=100, k_step=K, mel_src=dev(mel), seed=9, utt_ids=utt)
          for K in (300, 301)]
    assert not torch.equal(at[0], at[1])


def test_sample_from_rejects_bad_arguments(engine, cond3):
    """SVC_ERR_INVALID with a message: k_step outside [1, steps], both or neither start state, NULL utt_ids with
    mel_src."""
    B, T, _ = cond3.shape
    mel = dev(_mel(UTT3, T, 100))
    utt = dev(np.array(UTT3), torch.int32)
    x0 = torch.full((B, T, 100), -7.0, device="cuda")

    def run(K, mel_src, x_start, ids):
        _lib.call("svc_diffsvc_sample_from", engine._ctx, ptr(cond3), B, T, None, 1, 100, K, ptr(mel_src), ptr(x_start),
                  None, 0, ptr(ids), ptr(x0), stream())

    for K in (0, -1, STEPS + 1):
        with pytest.raises(_lib.SVCError, match="status 1:.*k_step"):
            run(K, mel, None, utt)
    for ms, xs in ((mel, mel), (None, None)):
        with pytest.raises(_lib.SVCError, match="status 1:.*exactly one"):
            run(300, ms, xs, utt)
    with pytest.raises(_lib.SVCError, match="status 1:.*utt_ids"):
        run(300, mel, None, None)
    torch.cuda.synchronize()
    assert bool((x0 == -7.0).all())


# ------------------------------------------------------------------ 7. sub-streams
def test_shallow_sub_streams_bit_identical(engine, cond3, tune):
    """sampler_streams 1 / 2 / 3 give identical bits for a k_step call at B = 3 (an uneven split), PLMS and DDPM."""
    B, T, _ = cond3.shape
    utt = dev(np.array(UTT3), torch.int32)
    mel = dev(_mel(UTT3, T, 100))
    outs = {}
    for ns in ("1", "2", "3"):
        tune(engine, sampler_streams=ns)
        outs[ns] = [engine.diffsvc_sample(cond3, fast_inference=fast, speedup=100, k_step=K, mel_src=mel, seed=9,
                                          utt_ids=utt, frames=[T, T - 20, 40]).cpu().numpy()
                    for fast, K in ((True, 300), (False, 20))]
    for ns in ("2", "3"):
        assert np.array_equal(outs[ns][0], outs["1"][0]) and np.array_equal(outs[ns][1], outs["1"][1]), ns


# ------------------------------------------------------------------ 8. pipeline, copy-synthesis, server
SECS = [0.6, 1.0, 0.6]


@pytest.fixture(scope="module")
def clips():
    w24 = [dev(ON.synth_clip(40 + i, s, 24000)) for i, s in enumerate(SECS)]
    w16 = [dev(ON.synth_clip_16k_quantised(40 + i, s)) for i, s in enumerate(SECS)]
    return w24, w16, [1, 3, 0]


def _alone(pipe, clips, i, **kw):
    w24, w16, singers = clips
    return pipe.convert(w24[i][None], w16[i][None], dev(np.array([singers[i]]), torch.int32), speedup=100, seed=5,
                        utt_ids=dev(np.array([i]), torch.int32), **kw)


def test_pipeline_k_step(engine, clips):
    """convert_many(k_step=K) on clips of two lengths (ragged, and bucketed) equals each clip converted alone with its
    utterance id, bit for bit; k_step changes the result; convert(k_step=None) is the call without the argument."""
    pipe = SVCPipeline(engine)
    w24, w16, singers = clips
    K = 300
    outs = pipe.convert_many(w24, w16, singers, speedup=100, seed=5, k_step=K)
    buck = pipe.convert_many(w24, w16, singers, speedup=100, seed=5, k_step=K, bucketed=True)
    for i in range(len(SECS)):
        one = _alone(pipe, clips, i, k_step=K)
        assert bool(torch.isfinite(one.wav).all())
        assert torch.equal(outs[i], one.wav[0]) and torch.equal(buck[i], one.wav[0]), i
    full = _alone(pipe, clips, 0)
    none = _alone(pipe, clips, 0, k_step=None)
    assert torch.equal(full.wav, none.wav) and torch.equal(full.x0, none.x0)
    assert not torch.equal(full.x0, _alone(pipe, clips, 0, k_step=K).x0)


def test_resynthesize(engine, cfg, states, clips):
    """Copy-synthesis: T * hop samples per clip, equal to bigvgan(mel_normalize(mel_energy(wav))); a ragged batch gives
    each clip as alone; an engine with the vocoder alone (no mapper, no content encoder) gives the same bits."""
    pipe = SVCPipeline(engine)
    w24 = clips[0]
    hop = cfg.hop_length
    alone = []
    for w in w24:
        out = pipe.resynthesize(w[None])
        mel, _ = engine.mel_energy(w[None])
        assert out.shape == (1, mel.shape[1] * hop) and bool(torch.isfinite(out).all())
        assert torch.equal(out, engine.bigvgan(engine.mel_normalize(mel)))
        alone.append(out[0])
    pad, n24 = SVCPipeline._pad_stack(w24)
    rag = pipe.resynthesize(pad, n_samples=n24)
    for i, a in enumerate(alone):
        assert torch.equal(rag[i, :a.shape[0]], a) and bool((rag[i, a.shape[0]:] == 0).all()), i
    voc = SVCEngine(cfg, 0, vocoder_state=states["vocoder"])
    try:
        assert torch.equal(SVCPipeline(voc).resynthesize(w24[1][None])[0], alone[1])
    finally:
        voc.close()


def test_server_k_step_matches_single_clips(engine, clips):
    """Requests with and without k_step through SVCServer: each result is that clip converted alone with its id."""
    pipe = SVCPipeline(engine)
    w24, w16, singers = clips
    ks = [300, None, 300]
    with SVCServer(pipe, max_batch=4, max_wait_s=60.0, speedup=100, seed=5) as srv:
        futs = [srv.submit(w24[i], w16[i], singers[i], utt_id=i, k_step=ks[i]) for i in range(3)]
    outs = [f.result(timeout=60) for f in futs]
    assert sorted(map(sorted, srv.batches)) == [[0, 2], [1]]
    for i in range(3):
        assert torch.equal(outs[i], _alone(pipe, clips, i, **({} if ks[i] is None else dict(k_step=ks[i]))).wav[0]), i
