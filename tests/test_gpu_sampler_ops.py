"""GPU parity, op level: the element-wise half of the DiffSVC sampler (csrc/elementwise.hip) against the float64
references of tests/sampler_ref.py. The device noise production draws (x_T and the DDPM z: Philox4x32-10 + Box-Muller),
the PLMS update in both kernel forms, the DDPM p_sample step and its clip, each through the svc_op_* entry that calls the
production launcher; that those entries are what svc_diffsvc_sample runs; and svc_pitch_shift's radix-select median
against np.median.

Every output lies between guard zones, and its 16-bit copy has pad columns (ld16 > C), pre-filled with a sentinel that
must survive the launch."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sampler_ref as R  # noqa: E402
from gpu_util import call, ptr, stream  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd import weights as W  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402

G = 128  # guard elements before and after a payload: more than a row, and the payload keeps its 16-byte alignment
SENT = {torch.float32: -7777.25, torch.int16: 0x5A5A, torch.float64: -7777.25}
STD_XT = float(np.float32(1.0) / np.float32(1.2))  # sample_impl's 1.0f / 1.2f
SEEDS = [0, 9, 0x123456789ABCDEF0]


class Buf:
    """A flat device payload of n elements between two guard zones, all pre-filled with the dtype's sentinel; `off`
    shifts the payload by that many elements (off = 1 misaligns a float32 payload)."""

    def __init__(self, n, dtype=torch.float32, off=0, init=None):
        self.sent, self.lo, self.n = SENT[dtype], G + off, n
        self.full = torch.full((G + off + n + G,), self.sent, dtype=dtype, device="cuda")
        self.t = self.full[self.lo:self.lo + n]
        assert self.full.data_ptr() % 256 == 0
        if init is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init)).reshape(-1))

    def host(self, *shape):
        a = self.t.cpu().numpy()
        a = a.view(np.uint16) if a.dtype == np.int16 else a
        return a.reshape(shape) if shape else a

    def guards_ok(self):
        return bool((self.full[:self.lo] == self.sent).all() and (self.full[self.lo + self.n:] == self.sent).all())


def _check16(h, x32, ld16, bf16):
    """h: Buf of [rows][ld16] 16-bit words; columns < C hold the operand rounding of x32 [rows, C], the rest and the
    guards the sentinel."""
    rows, Cc = x32.shape
    got = h.host(rows, ld16)
    assert np.array_equal(got[:, :Cc], R.op16_bits(x32, bf16))
    assert np.all(got[:, Cc:] == SENT[torch.int16]) and h.guards_ok()


def _ids(ids):
    return torch.tensor(ids, dtype=torch.int32, device="cuda")


def _init_noise(seed, ids, T, Cc, ld16, bf16=0, std=STD_XT):
    """svc_op_init_noise -> float32 [B, T, C]; guards, pad columns and the 16-bit copy are checked here."""
    B = len(ids)
    idd, x, h = _ids(ids), Buf(B * T * Cc), Buf(B * T * ld16, torch.int16)
    call("svc_op_init_noise", seed, ptr(idd), B, T, Cc, std, ptr(x.t), ptr(h.t), ld16, bf16, stream())
    out = x.host(B, T, Cc)
    assert x.guards_ok()
    _check16(h, out.reshape(B * T, Cc), ld16, bf16)
    return out


def _step_noise(seed, ids, step, T, Cc, ld16, bf16=0):
    """The DDPM step draw through svc_op_ddpm_update: all coefficients 0 and sigma 1 make the output z exactly."""
    B = len(ids)
    idd, x, h = _ids(ids), Buf(B * T * Cc, init=np.zeros(B * T * Cc, np.float32)), Buf(B * T * ld16, torch.int16)
    eps = torch.zeros(B * T * Cc, device="cuda")
    call("svc_op_ddpm_update", ptr(x.t), ptr(eps), B, T, Cc, 0.0, 0.0, 0.0, 0.0, 1.0, None, seed, ptr(idd), step,
         ptr(h.t), ld16, bf16, stream())
    out = x.host(B, T, Cc)
    assert x.guards_ok()
    _check16(h, out.reshape(B * T, Cc), ld16, bf16)
    return out


# ------------------------------------------------------------------ device noise
@pytest.mark.parametrize("seed", SEEDS, ids=lambda s: "seed%x" % s)
@pytest.mark.parametrize("ids,T,Cc,ld16", [([3], 1, 100, 104), ([7, 0, 2 ** 31 - 1], 50, 100, 104),
                                           ([1, 4], 700, 100, 104), ([6, 2], 37, 80, 88)],
                         ids=["1x1x100", "3x50x100", "2x700x100", "2x37x80"])
def test_init_noise_vs_reference(ids, T, Cc, ld16, seed):
    """x_T as production draws it, element by element against normal_f64 (|z_gpu - std z_ref| <= 1e-5: a wrong bit
    anywhere in Philox, a dropped key word or a colliding element key moves draws by O(1)); binary16 and bfloat16
    copies are the roundings of the float32 values, bit for bit.
    Largest |z_gpu - std z_ref| observed on MI355X: 4.9e-7 (B = 2, T = 700, seed 9), 5 % of the bound."""
    got = _init_noise(seed, ids, T, Cc, ld16)
    ref = STD_XT * R.noise_block(seed, ids, R.XT_STEP, T, Cc)
    err = float(np.max(np.abs(got - ref)))
    print("init_noise B=%d T=%d C=%d seed=%x: max |d| %.3e" % (len(ids), T, Cc, seed, err))
    assert np.isfinite(got).all()
    assert err <= R.NOISE_ATOL
    assert np.array_equal(_init_noise(seed, ids, T, Cc, ld16, bf16=1), got)
    # std scales the same draws
    unit = _init_noise(seed, ids, T, Cc, ld16, std=1.0)
    assert float(np.max(np.abs(unit - R.noise_block(seed, ids, R.XT_STEP, T, Cc)))) <= R.NOISE_ATOL


def test_noise_keyed_by_utterance_and_frame():
    """Row b depends on utt_ids[b] alone (same bits at another batch position and in another batch size), and an
    element's draw not on T (keys are t * C + c): the first 50 frames of a T = 64 batch are the T = 50 batch."""
    a = _init_noise(9, [7, 0, 2 ** 31 - 1], 50, 100, 104)
    b = _init_noise(9, [2 ** 31 - 1, 7], 50, 100, 104)
    assert np.array_equal(b[0], a[2]) and np.array_equal(b[1], a[0])
    assert np.array_equal(_init_noise(9, [0], 50, 100, 104)[0], a[1])
    c = _init_noise(9, [7, 0, 2 ** 31 - 1], 64, 100, 104)
    assert np.array_equal(c[:, :50], a)
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], a[2])
    # the DDPM step draw is keyed the same way
    za = _step_noise(9, [7, 0, 2 ** 31 - 1], 5, 50, 100, 104)
    zb = _step_noise(9, [2 ** 31 - 1, 7], 5, 64, 100, 104)
    assert np.array_equal(zb[0, :50], za[2]) and np.array_equal(zb[1, :50], za[0])


@pytest.mark.parametrize("seed", SEEDS, ids=lambda s: "seed%x" % s)
def test_ddpm_step_noise_vs_reference(seed):
    """The z ddpm_kernel draws when none is given (svc_op_ddpm_update with zero coefficients and sigma = 1 returns it
    exactly) at steps 0, 1 and 999 against normal_f64 under the x_T bound; consecutive steps and the x_T draw (step
    word 0xFFFFFFFF) all differ.
    Largest |z_gpu - z_ref| observed on MI355X: 5.0e-7 (seed 0, step 0)."""
    ids, T, Cc = [7, 0, 2 ** 31 - 1], 50, 100
    z = {}
    for step in (0, 1, 2, 999):
        z[step] = _step_noise(seed, ids, step, T, Cc, 104, bf16=step & 1)
        if step != 2:
            err = float(np.max(np.abs(z[step] - R.noise_block(seed, ids, step, T, Cc))))
            print("ddpm z seed=%x step=%d: max |d| %.3e" % (seed, step, err))
            assert err <= R.NOISE_ATOL
    z["xT"] = _init_noise(seed, ids, T, Cc, 104, std=1.0)
    for a, b in [(0, 1), (1, 2), (0, "xT"), (999, "xT")]:
        assert np.mean(z[a] == z[b]) < 1e-3, (a, b)


# ------------------------------------------------------------------ PLMS update
def _plms(e, coef, div, co, xin, xout, x16, ld16, eavg, bf16, rows, Cc):
    ep = [ptr(t) for t in e] + [None] * (4 - len(e))
    cf = [float(c) for c in coef] + [0.0] * (4 - len(coef))
    d, A, Bc = (float(v) for v in co)
    call("svc_op_plms_update", *ep, *cf, len(e), float(div), d, A, Bc, ptr(xin), ptr(xout), ptr(x16), ld16,
         ptr(eavg), bf16, rows, Cc, stream())


def _plms_run(x, e, coef, div, co, Cc, ld16, bf16, alias, off_xin=0, with_eavg=True):
    """One launch on guarded buffers -> (xout, e_avg or None), float32 [rows, C]; the 16-bit copy, pad columns and
    guards are checked here. alias: xout is xin (production's corrector steps), else a buffer of its own (the first
    step's predictor). off_xin = 1 moves xin off 16-byte alignment, which selects the one-channel kernel."""
    rows = x.shape[0]
    n = rows * Cc
    eb = [Buf(n, init=ek) for ek in e]
    xi = Buf(n, off=off_xin, init=x)
    xo = xi if alias else Buf(n, off=off_xin)
    h = Buf(rows * ld16, torch.int16)
    ea = Buf(n) if with_eavg else None
    assert xi.t.data_ptr() % 16 == 4 * off_xin and all(b.t.data_ptr() % 16 == 0 for b in eb)
    _plms([b.t for b in eb], coef, div, co, xi.t, xo.t, h.t, ld16, ea.t if ea else None, bf16, rows, Cc)
    out = xo.host(rows, Cc)
    assert xo.guards_ok() and xi.guards_ok() and all(b.guards_ok() for b in eb)
    if not alias:
        assert np.array_equal(xi.host(rows, Cc), x)
    for b, ek in zip(eb, e):
        assert np.array_equal(b.host(rows, Cc), ek)
    _check16(h, out, ld16, bf16)
    if ea:
        assert ea.guards_ok()
    return out, (ea.host(rows, Cc) if ea else None)


@pytest.mark.parametrize("i", [990, 10], ids=["t990", "t10"])
@pytest.mark.parametrize("coef,div", R.PLMS_COEFFS, ids=["pred", "first", "ab2", "ab3", "ab4"])
def test_plms_update_vs_f64(coef, div, i):
    """The five production coefficient sets at a large and a small t (interval 10), independent random histories.
    Four-channel form (C = 100, ld16 = 104, rows 1 / 3 / 257) and one-channel form (C = 99; C = 100 with xin one float
    off alignment) against float64 within 16 u (|x| + |d| (|A x| + |Bc| sum |c_k e_k| / div)), e_avg_out within
    16 u sum |c_k e_k| / div; the two forms bit-identical on the same data; xout aliasing xin and not; binary16 and
    bfloat16 copies the exact roundings of xout.
    Largest err / bound observed on MI355X: x 0.20, e_avg_out 0.18 (both at AB4)."""
    co = R.plms_step_coeffs(R.schedule(), i, 10)
    ne = len(coef)
    worst_x = worst_e = 0.0
    for rows in (1, 3, 257):
        x, e = R.plms_inputs(rows, 100, ne)
        e_ref, be, x_ref, bx = R.plms_ref(x, e, coef, div, *co)
        v_out, v_e = _plms_run(x, e, coef, div, co, 100, 104, 0, alias=False)           # plms4_kernel
        worst_x = max(worst_x, float(np.max(np.abs(v_out - x_ref) / bx)))
        worst_e = max(worst_e, float(np.max(np.abs(v_e - e_ref) / np.maximum(be, 1e-300))))
        assert np.all(np.abs(v_out - x_ref) <= bx) and np.all(np.abs(v_e - e_ref) <= be)
        s_out, s_e = _plms_run(x, e, coef, div, co, 100, 104, 0, alias=False, off_xin=1)  # plms_kernel, same data
        assert np.array_equal(s_out, v_out) and np.array_equal(s_e, v_e)
        # in place, bfloat16 copy, no e_avg_out: both forms
        a_out, _ = _plms_run(x, e, coef, div, co, 100, 104, 1, alias=True, with_eavg=False)
        assert np.array_equal(a_out, v_out)
        a_out, _ = _plms_run(x, e, coef, div, co, 100, 104, 1, alias=True, off_xin=1, with_eavg=False)
        assert np.array_equal(a_out, v_out)
        # C = 99: no four-channel form
        x9, e9 = R.plms_inputs(rows, 99, ne)
        e_ref, be, x_ref, bx = R.plms_ref(x9, e9, coef, div, *co)
        o9, ea9 = _plms_run(x9, e9, coef, div, co, 99, 104, rows & 1, alias=False)
        assert np.all(np.abs(o9 - x_ref) <= bx) and np.all(np.abs(ea9 - e_ref) <= be)
        worst_x = max(worst_x, float(np.max(np.abs(o9 - x_ref) / bx)))
    print("plms ne=%d t=%d: err/bound x %.4f e_avg %.4f" % (ne, i, worst_x, worst_e))


def test_plms_update_rejects_bad_args():
    """A missing history (ne = 2 with e1 NULL) or ne outside 1..4 is SVC_ERR_INVALID and nothing is written."""
    x, e = R.plms_inputs(3, 100, 1)
    xi, xo, eb = Buf(300, init=x), Buf(300), Buf(300, init=e[0])
    for ne in (2, 0, 5):
        with pytest.raises(_lib.SVCError, match="status 1:.*op_plms_update"):
            call("svc_op_plms_update", ptr(eb.t), None, None, None, 1.0, 1.0, 0.0, 0.0, ne, 2.0, 0.1, 1.0, 1.0,
                 ptr(xi.t), ptr(xo.t), None, 104, None, 0, 3, 100, stream())
    assert bool((xo.full == xo.sent).all())


# ------------------------------------------------------------------ DDPM p_sample
@pytest.mark.parametrize("i", [999, 500, 1, 0], ids=lambda i: "t%d" % i)
@pytest.mark.parametrize("B,T", [(1, 1), (3, 50)])
def test_ddpm_update_vs_f64(B, T, i):
    """p_sample with z given and the schedule's coefficients at t = 999, 500, 1, 0 (sigma = 0 at 0), inputs scaled so
    that sra x - srm1 eps falls below -1, inside and above +1 in about equal thirds. Every element within 16 u of the
    sum of its terms' magnitudes of the float64 result; elements whose pre-clip value lies within its own bound of
    -1 / +1 may have gone to either side of the clip. In place, 16-bit copies exact roundings.
    Largest err / bound observed on MI355X: 0.16 (B = 3, T = 50, t = 1)."""
    Cc, ld16 = 100, 104
    co = R.ddpm_step_coeffs(R.schedule(), i)
    x, eps, z = R.ddpm_inputs(B * T, Cc, co[0], co[1])
    outs = []
    for bf16 in (0, 1):
        xb, eb, zb, h = Buf(x.size, init=x), Buf(x.size, init=eps), Buf(x.size, init=z), Buf(B * T * ld16, torch.int16)
        call("svc_op_ddpm_update", ptr(xb.t), ptr(eb.t), B, T, Cc, *[float(v) for v in co], ptr(zb.t), 0, None, i,
             ptr(h.t), ld16, bf16, stream())
        out = xb.host(B * T, Cc)
        assert xb.guards_ok() and np.array_equal(eb.host(B * T, Cc), eps) and np.array_equal(zb.host(B * T, Cc), z)
        _check16(h, out, ld16, bf16)
        outs.append(out)
    assert np.array_equal(outs[0], outs[1])
    worst, pre = R.ddpm_err_over_bound(outs[0], x, eps, z, co)
    print("ddpm B=%d T=%d t=%d: err/bound %.4f" % (B, T, i, worst))
    for part in (pre < -1, np.abs(pre) < 1, pre > 1):
        assert part.any() and (B * T == 1 or part.mean() > 0.25)
    assert worst <= 1.0


def test_ddpm_update_needs_a_noise_source():
    """z NULL and utt_ids NULL: no key for the device draw, SVC_ERR_INVALID, x untouched."""
    xb, eb, h = Buf(100, init=np.ones(100, np.float32)), Buf(100, init=np.ones(100, np.float32)), Buf(104, torch.int16)
    with pytest.raises(_lib.SVCError, match="status 1:.*needs utt_ids"):
        call("svc_op_ddpm_update", ptr(xb.t), ptr(eb.t), 1, 1, 100, 1.0, 0.0, 1.0, 0.0, 1.0, None, 0, None, 3,
             ptr(h.t), 104, 0, stream())
    assert bool((xb.t == 1.0).all()) and bool((h.full == h.sent).all())


# ------------------------------------------------------------------ the op entries are the production path
@pytest.fixture(scope="module")
def tiny_engine():
    cfg = C.load_config()
    dims = W.WHISPER_DIMS["tiny-test"]
    cfg.mapper.input_content_dim["whisper"] = dims["n_audio_state"]
    e = SVCEngine(cfg, 0, mapper_state=W.make_mapper_state(cfg.mapper, 0))
    yield e
    e.close()


def test_op_noise_is_what_the_sampler_draws(tiny_engine):
    """svc_diffsvc_sample with device noise (seed, utt_ids: how the pipeline, the server and the benchmark run it)
    equals, bit for bit, the same sampler fed x_T = svc_op_init_noise(std = 1 / 1.2) and, for DDPM, noise[j] =
    the svc_op_ddpm_update draw of step 999 - j: what the tests above check is what production consumes."""
    e = tiny_engine
    B, T, Cc, seed, ids = 2, 16, 100, 0x9E3779B97F4A7C15, [5, 2 ** 31 - 1]
    cond = (torch.randn(B, T, 384, generator=torch.Generator().manual_seed(3)) * 0.5).cuda()
    idd = _ids(ids)
    xT = torch.from_numpy(_init_noise(seed, ids, T, Cc, 104)).cuda()
    dev_plms = e.diffsvc_sample(cond, fast_inference=True, speedup=250, seed=seed, utt_ids=idd)
    giv_plms = e.diffsvc_sample(cond, fast_inference=True, speedup=250, x_T=xT)
    assert torch.isfinite(dev_plms).all() and torch.equal(dev_plms, giv_plms)
    noise = torch.zeros(1000, B * T * Cc, device="cuda")
    zeros, h16 = torch.zeros(B * T * Cc, device="cuda"), torch.zeros(B * T * 104, dtype=torch.int16, device="cuda")
    for j in range(1000):
        _lib.call("svc_op_ddpm_update", ptr(noise[j]), ptr(zeros), B, T, Cc, 0.0, 0.0, 0.0, 0.0, 1.0, None, seed,
                  ptr(idd), 999 - j, ptr(h16), 104, 0, stream())
    torch.cuda.synchronize()
    dev_ddpm = e.diffsvc_sample(cond, fast_inference=False, seed=seed, utt_ids=idd)
    giv_ddpm = e.diffsvc_sample(cond, fast_inference=False, x_T=xT, noise=noise)
    assert torch.isfinite(dev_ddpm).all() and torch.equal(dev_ddpm, giv_ddpm)
    assert not torch.equal(dev_ddpm, dev_plms)


# ------------------------------------------------------------------ pitch shift
def _pitch_rows(T, rng):
    """Rows of f0 [T] float64 for one launch: voiced counts 0, 1, 2, 3, an even and an odd one, all T; one repeated
    value (ties through all 64 radix passes); two values one ulp apart; mixed signs."""
    rows = []
    for n in sorted({0, 1, 2, 3, (T // 2) & ~1, (T // 2) | 1, T - 1, T}):
        if 0 <= n <= T:
            f = np.zeros(T)
            f[rng.permutation(T)[:n]] = rng.uniform(80.0, 600.0, n)
            rows.append(f)
    rows.append(np.full(T, 220.0))
    tie = np.zeros(T)
    tie[rng.permutation(T)[:max(1, T // 2)]] = 311.127
    rows.append(tie)
    rows.append(np.where(rng.random(T) < 0.5, 233.08188075904496, np.nextafter(233.08188075904496, 1e9)))
    mixed = rng.standard_normal(T) * 100.0
    mixed[rng.random(T) < 0.2] = 0.0
    mixed[0] = -57.3  # (never an unvoiced row)
    rows.append(mixed)
    rows.append(-rng.uniform(80.0, 600.0, T))
    return np.stack(rows)


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 255, 256, 257, 937])
def test_pitch_shift_vs_np_median(tiny_engine, T):
    """svc_pitch_shift = f0 * (target / np.median(f0[f0 != 0])) per row, exactly (NaN row where nothing is voiced):
    T below, at and above the wave and the block size, every small voiced count, ties, neighbours one ulp apart and
    signed values (the select's keys are order-preserving), all rows of a T in one launch."""
    target = 223.25784012425046
    f0 = _pitch_rows(T, np.random.default_rng(T))
    B = f0.shape[0]
    buf = Buf(B * T, torch.float64, init=f0)
    tiny_engine.pitch_shift(buf.t.view(B, T), target)
    torch.cuda.synchronize()
    got = buf.host(B, T)
    exp = np.empty_like(f0)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for b in range(B):
            exp[b] = f0[b] * (target / np.median(f0[b][f0[b] != 0]))
    assert np.isnan(exp[0]).all() and np.isfinite(exp[1:]).all()
    np.testing.assert_array_equal(got, exp)
    assert buf.guards_ok()
