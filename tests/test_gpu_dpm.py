"""GPU parity: the DPM-Solver++(2M) / DDIM sampler. The fused update launch (csrc/elementwise.hip dpm_update) at op
level through svc_op_dpm_update against the float64 reference of tests/dpm_ref.py, between guard zones as in
tests/test_gpu_sampler_ops.py; svc_diffsvc_sample_steps against the reference loop run over the oracle's denoiser;
sub-streams, ragged batches, the start states, the one-entry list; that solver=None leaves the existing calls alone;
and the pipeline and server on top."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dpm_ref as D  # noqa: E402
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
from test_gpu_sampler_ops import Buf, _check16, _init_noise  # noqa: E402

STEPS = 1000
SHAPES = [(1, 100, 104), (150, 100, 104), (74, 80, 88)]
# the coefficient sets: three real steps (h_prev: a plausible previous step's, dpm_ref-side only) and the final form
CASES = {"999to949": (999, 949, None), "300to120": (300, 120, 500), "12to0": (12, 0, 40), "final0": (0, None, None)}


def _coeffs(sch, case, history):
    t, s, tp = CASES[case]
    if s is None:
        return D.final_coeffs(sch, t), True
    h_prev = None
    if history:
        h_prev = D.step_coeffs(sch["ac"], tp, t)["h"] if tp is not None else D.step_coeffs(sch["ac"], t, s)["h"]
    return D.kernel_coeffs(sch, t, s, h_prev), False


def _dpm(x, eps, d_prev, co, final, Cc, ld16, bf16=0, alias=False, off=0, want_d=True):
    """One svc_op_dpm_update launch on guarded buffers -> (x', D or None), float32 [rows, C]. Checked here: the guards
    of every buffer, eps (and an un-aliased d_prev) unchanged, the 16-bit copy the exact operand rounding of x' with its
    pad columns untouched. alias: d_out is d_prev. off = 1 moves every float32 payload one element off 16-byte
    alignment, which selects the one-channel kernel."""
    rows = x.shape[0]
    n = rows * Cc
    xb, eb = Buf(n, off=off, init=x), Buf(n, off=off, init=eps)
    pb = Buf(n, off=off, init=d_prev) if d_prev is not None else None
    ob = pb if alias else (Buf(n, off=off) if want_d else None)
    h = Buf(rows * ld16, torch.int16)
    assert xb.t.data_ptr() % 16 == 4 * off and eb.t.data_ptr() % 16 == 4 * off
    call("svc_op_dpm_update", ptr(xb.t), ptr(eb.t), ptr(pb.t) if pb else None, ptr(ob.t) if ob else None, rows, Cc,
         *[float(v) for v in co], int(final), ptr(h.t), ld16, bf16, stream())
    out = xb.host(rows, Cc).copy()
    assert xb.guards_ok() and eb.guards_ok() and np.array_equal(eb.host(rows, Cc), eps)
    if pb is not None:
        assert pb.guards_ok()
        if not alias:
            assert np.array_equal(pb.host(rows, Cc), d_prev)
    if ob is not None:
        assert ob.guards_ok()
    _check16(h, out, ld16, bf16)
    return out, (ob.host(rows, Cc).copy() if ob is not None else None)


# ------------------------------------------------------------------ 1. the update vs float64
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("rows,Cc,ld16", SHAPES, ids=["1x100", "150x100", "74x80"])
def test_dpm_update_vs_f64(rows, Cc, ld16, case):
    """x' and D of the real steps 999 -> 949, 300 -> 120, 12 -> 0 and of the final form at t = 0, with and without a
    history, element by element within 16 u times the summed magnitudes of their terms of float64 (dpm_ref.dpm_ref); an
    element whose pre-clip value lies within its bound of -1 / +1 is compared against both sides of the clip. Inputs as
    sampler_ref.ddpm_inputs scales them: a third of the elements on each side of the clip. d_out aliased to d_prev
    and separate, a bfloat16 copy instead of a binary16 one, and a payload one float off alignment (the one-channel
    kernel; C = 100 and 80 both take the four-channel one when aligned) all return the same bits.
    Largest err / bound observed on MI355X: x' 0.15 (12 -> 0, 74 x 80, with a history), D 0.094."""
    sch = R.schedule()
    worst = [0.0, 0.0]
    for history in (False, True):
        co, final = _coeffs(sch, case, history)
        x, eps, dp = D.dpm_inputs(rows, Cc, co[0], co[1])
        d_prev = dp if history else None
        out, d = _dpm(x, eps, d_prev, co, final, Cc, ld16, want_d=not final)
        assert np.isfinite(out).all()
        wx, wd, pre = D.err_over_bound(out, d, x, eps, d_prev, co, final)
        print("dpm %s rows=%d C=%d history=%d: err/bound x %.4f D %.4f" % (case, rows, Cc, history, wx, wd))
        worst = [max(worst[0], wx), max(worst[1], wd)]
        assert wx <= 1.0 and wd <= 1.0
        if rows > 1:
            for part in (pre < -1, np.abs(pre) < 1, pre > 1):
                assert part.mean() > 0.25
        # the other forms of the same launch: the same bits
        variants = [dict(bf16=1), dict(off=1), dict(off=1, bf16=1), dict(want_d=False)]
        if history and not final:
            variants += [dict(alias=True), dict(alias=True, off=1, bf16=1)]
        for kw in variants:
            o2, d2 = _dpm(x, eps, d_prev, co, final, Cc, ld16, **dict(dict(want_d=not final), **kw))
            assert np.array_equal(o2, out), kw
            if d2 is not None and d is not None:
                assert np.array_equal(d2, d), kw
        if final:  # a, b, w0, w1 and d_prev are ignored; D, when asked for, is x'
            junk = (co[0], co[1], 3.0, -2.0, 0.5, 7.0)
            o3, d3 = _dpm(x, eps, dp, junk, True, Cc, ld16)
            assert np.array_equal(o3, out) and np.array_equal(d3, out)
    print("dpm %s rows=%d C=%d: worst err/bound x %.4f D %.4f" % (case, rows, Cc, *worst))


def test_dpm_update_detects_swapped_coefficients():
    """x, eps and d_prev are independent draws, so the kernel's output is far outside the bound of a reference whose
    w0 / w1, a / b or sra / srm1 are exchanged: the comparison above would show any such slip."""
    sch = R.schedule()
    co, _ = _coeffs(sch, "300to120", True)
    x, eps, dp = D.dpm_inputs(150, 100, co[0], co[1])
    out, d = _dpm(x, eps, dp, co, False, 100, 104)
    assert D.err_over_bound(out, d, x, eps, dp, co, False)[0] <= 1.0
    for sw in ((co[0], co[1], co[3], co[2], co[4], co[5]), (co[0], co[1], co[2], co[3], co[5], co[4]),
               (co[1], co[0], co[2], co[3], co[4], co[5])):
        assert D.err_over_bound(out, None, x, eps, dp, sw, False)[0] > 1e3
    # and a history that is not read shows too
    no_hist, _ = _dpm(x, eps, None, co, False, 100, 104)
    assert D.err_over_bound(no_hist, None, x, eps, dp, co, False)[0] > 1e3


def test_dpm_update_rejects_bad_args():
    """x or eps NULL, no rows, no channels, rows of the 16-bit copy shorter than C: SVC_ERR_INVALID, nothing written."""
    xb, eb, h = Buf(300, init=np.ones(300, np.float32)), Buf(300, init=np.ones(300, np.float32)), Buf(312, torch.int16)
    ob = Buf(300)
    for a in ((None, ptr(eb.t), 3, 100, 104), (ptr(xb.t), None, 3, 100, 104), (ptr(xb.t), ptr(eb.t), 0, 100, 104),
              (ptr(xb.t), ptr(eb.t), 3, 0, 104), (ptr(xb.t), ptr(eb.t), 3, 100, 96)):
        with pytest.raises(_lib.SVCError, match="status 1:.*op_dpm_update"):
            call("svc_op_dpm_update", a[0], a[1], None, ptr(ob.t), a[2], a[3], 1.0, 0.5, 1.0, 0.0, 0.9, 0.1, 0,
                 ptr(h.t), a[4], 0, stream())
    assert bool((xb.t == 1.0).all()) and bool((h.full == h.sent).all()) and bool((ob.full == ob.sent).all())


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
    """Full-size mapper and vocoder, tiny Whisper (as tests/test_gpu_shallow.py builds it)."""
    e = SVCEngine(cfg, 0, whisper_state=states["whisper"], mapper_state=states["mapper"], vocoder_state=states["vocoder"])
    yield e
    e.close()


def _mel(ids, T, seed=0):
    st = C.load_stats(C.load_config())
    return np.stack([S.mel_for_range(np.random.default_rng([seed, u % 9973, T, 100]), (T, 100), st["mel_min"],
                                     st["mel_max"]) for u in ids])


def _x_start(engine, mel, ids, level, seed):
    """mel [B, T, 100] noised forward to `level` by svc_op_q_sample with the packaged statistics -> device f32."""
    st = C.load_stats(C.load_config())
    B, T, Cc = mel.shape
    a, b = S.q_coeffs(R.schedule(), level + 1)
    m, x, h = dev(mel), torch.empty(B, T, Cc, device="cuda"), torch.zeros(B * T * 104, dtype=torch.int16, device="cuda")
    mn, mx, idd = dev(st["mel_min"]), dev(st["mel_max"]), dev(np.array(ids), torch.int32)  # alive across the launch
    call("svc_op_q_sample", ptr(m), ptr(mn), ptr(mx), B, T, Cc, float(a), float(b), None, seed, ptr(idd), None, ptr(x),
         ptr(h), 104, 0, stream())
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) < 8.0
    return x


# ------------------------------------------------------------------ 2. sampler vs the reference loop
@pytest.fixture(scope="module")
def oracle_den(cfg, states, golden):
    cond = torch.from_numpy(golden("conditioner_diffsvc")["cond"])
    table = W.step_embedding_table(STEPS)
    cache = {}

    def den(x, t):
        return OM.diffsvc_forward(states["mapper"], cfg.mapper, x, cond, torch.full((x.shape[0],), t, dtype=torch.long),
                                  table, cp_cache=cache)
    return cond, den


def _ref_loop(den, x, ts, order):
    sch = R.schedule()
    return D.sample_steps(den, x, ts, order, sch["ac"], sra=sch["sra"], srm1=sch["srm1"])


def _inside(x0):
    """The share of elements of a sampler output that the final clip left alone."""
    return float((x0.abs() < 1.0).float().mean())


def test_dpmpp2m_vs_reference_loop(engine, cfg, oracle_den):
    """dpmpp2m over 8 logsnr steps from K = 1000 (x_T given, so no draw tolerance enters) against
    dpm_ref.sample_steps with oracle.models.diffsvc_forward as the denoiser: rel-L2 under the 1.5e-3 that
    test_plms_and_ddpm and test_shallow_ddpm_vs_oracle hold this denoiser to over more calls.
    Measured on MI355X: 1.03e-3 (7 % of the reference's elements end inside the clip)."""
    cond, den = oracle_den
    T = cond.shape[1]
    ts = C.solver_timesteps(cfg, None, 8)
    assert len(ts) == 8 and ts[0] == 999 and ts[-1] == 0
    xT = torch.from_numpy(_init_noise(3, [5], T, 100, 104)).cuda()
    got = engine.diffsvc_sample(cond.cuda(), x_T=xT, solver="dpmpp2m", solver_steps=8)
    ref = _ref_loop(den, xT.cpu(), ts, 2)
    r = rel_l2(got.cpu().numpy(), ref.numpy())
    print("dpmpp2m 8 steps from K=1000: rel_l2 %.3e, inside the clip %.3f" % (r, _inside(ref)))
    assert bool(torch.isfinite(got).all()) and r < 1.5e-3
    assert _inside(ref) > 0.02  # not a comparison of two saturated fields
    # the second order is in it: the first-order loop over the same list ends elsewhere
    assert rel_l2(got.cpu().numpy(), _ref_loop(den, xT.cpu(), ts, 1).numpy()) > 10 * max(r, 1e-5)


def test_ddim_vs_reference_loop(engine, cfg, oracle_den):
    """ddim over 4 logsnr steps from K = 300 via x_start (svc_op_q_sample's state) against the first-order reference
    loop, the same bound.
    Measured on MI355X: 1.5e-4 (53 % of the reference's elements end inside the clip)."""
    cond, den = oracle_den
    T = cond.shape[1]
    ts = C.solver_timesteps(cfg, 300, 4)
    assert len(ts) == 4 and ts[0] == 299 and ts[-1] == 0
    xs = _x_start(engine, _mel([6], T), [6], 299, seed=7)
    got = engine.diffsvc_sample(cond.cuda(), k_step=300, x_start=xs, solver="ddim", solver_steps=4)
    ref = _ref_loop(den, xs.cpu(), ts, 1)
    r = rel_l2(got.cpu().numpy(), ref.numpy())
    print("ddim 4 steps from K=300: rel_l2 %.3e, inside the clip %.3f" % (r, _inside(ref)))
    assert bool(torch.isfinite(got).all()) and r < 1.5e-3
    assert _inside(ref) > 0.02


# ------------------------------------------------------------------ 3. structure
@pytest.fixture(scope="module")
def cond3(golden):
    g = golden("conditioner_diffsvc")
    return dev(np.concatenate([g["cond"], g["cond"][:, ::-1], 0.5 * g["cond"]], 0))


UTT3 = [5, 2 ** 31 - 1, 7]


def test_solver_sub_streams_bit_identical(engine, cond3, tune):
    """sampler_streams 1 against 2 (and 3): identical bits at B = 3 (an uneven split), ragged, both solvers, from
    noise and from a source mel."""
    B, T, _ = cond3.shape
    utt = dev(np.array(UTT3), torch.int32)
    mel = dev(_mel(UTT3, T))
    outs = {}
    for ns in ("1", "2", "3"):
        tune(engine, sampler_streams=ns)
        outs[ns] = [engine.diffsvc_sample(cond3, solver=sol, solver_steps=5, seed=9, utt_ids=utt,
                                          frames=[T, T - 20, 40], **kw).cpu().numpy()
                    for sol, kw in (("dpmpp2m", {}), ("ddim", dict(k_step=300, mel_src=mel)))]
        assert all(np.isfinite(o).all() for o in outs[ns])
    for ns in ("2", "3"):
        assert np.array_equal(outs[ns][0], outs["1"][0]) and np.array_equal(outs[ns][1], outs["1"][1]), ns


def test_solver_ragged_equals_each_utterance_alone(engine, cond3):
    """frames = [93, 37]: each utterance equals itself converted alone with its utterance id, bit for bit, and the tail
    rows of the short one are +0; from the device draw and from a source mel."""
    T = cond3.shape[1]
    assert T == 93
    cond, ids = cond3[:2].contiguous(), UTT3[:2]
    utt = dev(np.array(ids), torch.int32)
    mel = dev(_mel(ids, T))
    for kw, src in ((dict(solver="dpmpp2m", solver_steps=6), False),
                    (dict(solver="dpmpp2m", solver_steps=5, k_step=300), True)):
        rag = engine.diffsvc_sample(cond, seed=9, utt_ids=utt, frames=[93, 37], **kw,
                                    **(dict(mel_src=mel) if src else {}))
        assert bool(torch.isfinite(rag).all())
        for b, n in ((0, 93), (1, 37)):
            one = engine.diffsvc_sample(cond[b:b + 1, :n].contiguous(), seed=9, utt_ids=utt[b:b + 1], **kw,
                                        **(dict(mel_src=mel[b:b + 1, :n].contiguous()) if src else {}))
            assert torch.equal(rag[b, :n], one[0]), (kw, b)
        tail = rag[1, 37:].cpu().numpy()
        assert np.all(tail == 0) and not np.signbit(tail).any()


def test_solver_mel_src_path_equals_x_start_path(engine, cfg, cond3):
    """svc_diffsvc_sample_steps(mel_src) = the same call with x_start = svc_op_q_sample(mel_src) at level ts[0], bit
    for bit; and without k_step the device draw equals x_T = svc_op_init_noise's draw."""
    B, T, _ = cond3.shape
    utt = dev(np.array(UTT3), torch.int32)
    mel = _mel(UTT3, T)
    kw = dict(solver="dpmpp2m", solver_steps=5, seed=9, utt_ids=utt)
    assert C.solver_timesteps(cfg, 300, 5)[0] == 299
    xs = _x_start(engine, mel, UTT3, 299, seed=9)
    a = engine.diffsvc_sample(cond3, k_step=300, mel_src=dev(mel), **kw)
    b = engine.diffsvc_sample(cond3, k_step=300, x_start=xs, **kw)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    xT = torch.from_numpy(_init_noise(9, UTT3, T, 100, 104)).cuda()
    assert torch.equal(engine.diffsvc_sample(cond3, **kw), engine.diffsvc_sample(cond3, x_T=xT, **kw))
    assert not torch.equal(a, engine.diffsvc_sample(cond3, k_step=301, mel_src=dev(mel), **kw))


def test_one_entry_list_is_the_clipped_data_prediction(engine, cond3):
    """solver_steps = 1 is the final form alone: x0 = clamp(sra x - srm1 eps) with eps of svc_diffsvc_eps at that
    level, within the update's bound (16 u (|sra x| + |srm1 eps|), both sides of the clip where it is that close).
    Measured on MI355X: err / bound 0.094, half of the elements clipped."""
    sch = R.schedule()
    T = cond3.shape[1]
    xs = _x_start(engine, _mel(UTT3, T), UTT3, 299, seed=4)
    for solver in ("ddim", "dpmpp2m"):
        got = engine.diffsvc_sample(cond3, k_step=300, x_start=xs, solver=solver, solver_steps=1)
        eps = engine.diffsvc_eps(cond3, xs, 299)
        wx, _, pre = D.err_over_bound(got.cpu().numpy(), None, xs.cpu().numpy(), eps.cpu().numpy(), None,
                                      D.final_coeffs(sch, 299), True)
        print("one-entry list (%s): err/bound %.4f, clipped %.2f" % (solver, wx, float(np.mean(np.abs(pre) > 1))))
        assert wx <= 1.0 and float(got.abs().max()) <= 1.0


def test_solver_none_is_the_existing_call(engine, cond3):
    """solver=None (and the other two keywords at any value) returns the bits of the call without the keywords: PLMS,
    DDPM, and a k_step call."""
    utt = dev(np.array(UTT3), torch.int32)
    mel = dev(_mel(UTT3, cond3.shape[1]))
    for kw in (dict(fast_inference=True, speedup=100), dict(fast_inference=False, k_step=20, mel_src=mel),
               dict(fast_inference=True, speedup=50, k_step=300, mel_src=mel)):
        old = engine.diffsvc_sample(cond3, seed=9, utt_ids=utt, **kw)
        new = engine.diffsvc_sample(cond3, seed=9, utt_ids=utt, solver=None, solver_steps=7, solver_spacing="uniform",
                                    **kw)
        assert bool(torch.isfinite(old).all()) and torch.equal(old, new), kw
    sol = engine.diffsvc_sample(cond3, seed=9, utt_ids=utt, solver="ddim", solver_steps=7, fast_inference=True,
                                speedup=100)
    assert not torch.equal(sol, engine.diffsvc_sample(cond3, seed=9, utt_ids=utt, fast_inference=True, speedup=100))


def test_sample_steps_rejects_bad_arguments(engine, cond3):
    """SVC_ERR_INVALID with a message, x0 untouched: an empty list, one not strictly decreasing, an entry outside
    [0, steps), an order other than 1 or 2, both start states, a device draw without utt_ids; `noise` with a solver is a
    ValueError in Python. svc_diffsvc_sample keeps rejecting any mode but 0 and 1."""
    B, T, _ = cond3.shape
    mel = dev(_mel(UTT3, T))
    utt = dev(np.array(UTT3), torch.int32)
    x0 = torch.full((B, T, 100), -7.0, device="cuda")

    def run(ts, order=2, mel_src=None, x_start=None, ids=utt):
        arr = (ctypes.c_int32 * max(len(ts), 1))(*ts)
        _lib.call("svc_diffsvc_sample_steps", engine._ctx, ptr(cond3), B, T, None, arr, len(ts), order, ptr(mel_src),
                  ptr(x_start), 0, ptr(ids), ptr(x0), stream())

    with pytest.raises(_lib.SVCError, match="status 1:.*empty"):
        run([])
    for ts in ([5, 5], [3, 7], [999, 500, 500, 0]):
        with pytest.raises(_lib.SVCError, match="status 1:.*strictly decreasing"):
            run(ts)
    for ts in ([STEPS], [-1], [999, -2]):
        with pytest.raises(_lib.SVCError, match="status 1:.*outside"):
            run(ts)
    for order in (0, 3):
        with pytest.raises(_lib.SVCError, match="status 1:.*order"):
            run([999, 0], order=order)
    with pytest.raises(_lib.SVCError, match="status 1:.*at most one"):
        run([299, 0], mel_src=mel, x_start=mel)
    for ms in (None, mel):
        with pytest.raises(_lib.SVCError, match="status 1:.*utt_ids"):
            run([299, 0], mel_src=ms, ids=None)
    with pytest.raises(_lib.SVCError, match="status 1:.*mode 2"):
        _lib.call("svc_diffsvc_sample", engine._ctx, ptr(cond3), B, T, None, 2, 10, None, None, 0, ptr(utt), ptr(x0),
                  stream())
    with pytest.raises(ValueError, match="noise"):
        engine.diffsvc_sample(cond3, solver="dpmpp2m", noise=torch.zeros(STEPS, B * T * 100, device="cuda"))
    torch.cuda.synchronize()
    assert bool((x0 == -7.0).all())


# ------------------------------------------------------------------ 4. pipeline and server
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


def test_pipeline_solver_equals_the_engine_calls(engine, clips):
    """convert(solver="dpmpp2m", solver_steps=6) equals the engine's stages composed by hand; convert_many (ragged and
    bucketed) returns each clip as converted alone; solver=None is the call without the keyword."""
    pipe = SVCPipeline(engine)
    w24, w16, singers = clips
    kw = dict(solver="dpmpp2m", solver_steps=6)
    res = _alone(pipe, clips, 1, **kw)
    e = engine
    wav24, sing, utt = w24[1][None], dev(np.array([singers[1]]), torch.int32), dev(np.array([1]), torch.int32)
    mel, energy = e.mel_energy(wav24)
    T = mel.shape[1]
    f0 = pipe.extract_f0(wav24, T)
    pipe.shift_f0(f0, sing, 0.0)
    cond = e.condition(pipe.content(w16[1][None], T, None), f0, energy, sing)
    x0 = e.diffsvc_sample(cond, seed=5, utt_ids=utt, **kw)
    assert bool(torch.isfinite(res.wav).all())
    assert torch.equal(res.x0, x0) and torch.equal(res.wav, e.bigvgan(x0))
    outs = pipe.convert_many(w24, w16, singers, speedup=100, seed=5, **kw)
    buck = pipe.convert_many(w24, w16, singers, speedup=100, seed=5, bucketed=True, **kw)
    for i in range(len(SECS)):
        one = res if i == 1 else _alone(pipe, clips, i, **kw)
        assert torch.equal(outs[i], one.wav[0]) and torch.equal(buck[i], one.wav[0]), i
    full, none = _alone(pipe, clips, 0), _alone(pipe, clips, 0, solver=None)
    assert torch.equal(full.wav, none.wav) and torch.equal(full.x0, none.x0)
    assert not torch.equal(full.x0, _alone(pipe, clips, 0, **kw).x0)
    # with shallow diffusion: the start mel is the clip's own
    ks = _alone(pipe, clips, 0, k_step=300, **kw)
    assert torch.equal(ks.x0, e.diffsvc_sample(
        e.condition(pipe.content(w16[0][None], ks.mel.shape[1], None), ks.f0, e.mel_energy(w24[0][None])[1],
                    dev(np.array([singers[0]]), torch.int32)),
        seed=5, utt_ids=dev(np.array([0]), torch.int32), k_step=300, mel_src=ks.mel, **kw))


def test_server_solver_matches_single_clips(engine, clips):
    """An SVCServer with the solver set, one request overriding the step count and one going back to PLMS: each result
    is that clip converted alone with its id, and the settings never share a batch."""
    pipe = SVCPipeline(engine)
    w24, w16, singers = clips
    over = [{}, dict(solver_steps=4), dict(solver="none")]
    with SVCServer(pipe, max_batch=4, max_wait_s=60.0, speedup=100, seed=5, solver="dpmpp2m", solver_steps=6) as srv:
        futs = [srv.submit(w24[i], w16[i], singers[i], utt_id=i, **over[i]) for i in range(3)]
    outs = [f.result(timeout=60) for f in futs]
    assert sorted(map(sorted, srv.batches)) == [[0], [1], [2]]
    alone = [dict(solver="dpmpp2m", solver_steps=6), dict(solver="dpmpp2m", solver_steps=4), {}]
    for i in range(3):
        assert torch.equal(outs[i], _alone(pipe, clips, i, **alone[i]).wav[0]), i
    with SVCServer(pipe, max_batch=4, max_wait_s=60.0, speedup=100, seed=5, solver="ddim", solver_steps=5) as srv:
        futs = [srv.submit(w24[i], w16[i], singers[i], utt_id=i) for i in range(3)]
    outs = [f.result(timeout=60) for f in futs]
    assert sorted(map(sorted, srv.batches)) == [[0, 1, 2]]
    for i in range(3):
        assert torch.equal(outs[i], _alone(pipe, clips, i, solver="ddim", solver_steps=5).wav[0]), i
