"""CPU: the sampler references of tests/sampler_ref.py checked on their own. The Philox restatement reproduces the
published Random123 known answers, the restated draw is a sound N(0, 1) (moments and correlations within 4 standard
errors), and a plain float32 evaluation of the PLMS and DDPM formulas meets the bounds the GPU kernels are held to
(tests/test_gpu_sampler_ops.py), on the same inputs."""
import numpy as np
import pytest

import sampler_ref as R

N_DRAWS = 2_000_000


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("ctr,key,expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, expect):
    """Random123's kat_vectors for philox4x32-10."""
    assert _hex(R.philox4x32_10(ctr, key)) == expect


def test_philox_is_elementwise():
    """Array counters give what the scalars give, word by word."""
    elem = np.array([0, 1, 99, 2 ** 32 - 1], dtype=np.uint64)
    out = R.philox4x32_10([elem, 7, 3, 0x5356434B], [9, 1])
    for j, e in enumerate(elem):
        one = R.philox4x32_10([int(e), 7, 3, 0x5356434B], [9, 1])
        assert [int(w[j]) for w in out] == [int(w) for w in one]


@pytest.fixture(scope="module")
def draws():
    elem = np.arange(N_DRAWS, dtype=np.uint64)
    return R.normal_f64(9, 5, R.XT_STEP, elem), R.normal_f64(9, 6, R.XT_STEP, elem)


def test_draw_is_standard_normal(draws):
    """Mean, variance and kurtosis of 2e6 draws of one (seed, utterance, step) within 4 standard errors."""
    z, n = draws[0], N_DRAWS
    mean, var = z.mean(), z.var()
    kurt = np.mean((z - mean) ** 4) / var ** 2
    print("mean %.2e var-1 %.2e kurt-3 %.2e" % (mean, var - 1, kurt - 3))
    assert abs(mean) < 4 / np.sqrt(n)
    assert abs(var - 1) < 4 * np.sqrt(2 / n)
    assert abs(kurt - 3) < 4 * np.sqrt(24 / n)


def test_draws_are_uncorrelated(draws):
    """Lag-1 autocorrelation along the element index, and the correlation between two utterance ids."""
    za, zb = draws
    n = N_DRAWS
    c = lambda a, b: float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))
    lag1, across = c(za[:-1], za[1:]), c(za, zb)
    print("lag-1 %.2e across utterances %.2e" % (lag1, across))
    assert abs(lag1) < 4 / np.sqrt(n)
    assert abs(across) < 4 / np.sqrt(n)


def test_draws_are_finite_and_u1_positive(draws):
    elem = np.arange(N_DRAWS, dtype=np.uint64)
    u1, u2 = R.uniforms(9, 5, R.XT_STEP, elem)
    assert u1.min() >= 2.0 ** -24 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    assert np.isfinite(draws[0]).all() and np.isfinite(draws[1]).all()
    # the extremes of the 24-bit uniforms: u1 = 2^-24 is the largest magnitude, u1 = 1 gives 0
    assert np.abs(draws[0]).max() <= np.sqrt(2 * np.log(2.0 ** 24))
    # float32 evaluation of the same formula (what the device does, with another libm) within the GPU test's bound
    ang = np.float32(6.283185307179586) * u2.astype(np.float32)
    z32 = np.sqrt(np.float32(-2.0) * np.log(u1.astype(np.float32))) * np.cos(ang)
    assert z32.dtype == np.float32
    assert np.max(np.abs(z32.astype(np.float64) - draws[0])) <= R.NOISE_ATOL


def test_key_words_all_matter():
    """Each of seed low / high word, utterance, step and element changes the draw (a dropped word would not)."""
    elem = np.arange(64, dtype=np.uint64)
    base = R.normal_f64(0x123456789ABCDEF0, 7, 3, elem)
    for other in (R.normal_f64(0x123456789ABCDEF1, 7, 3, elem), R.normal_f64(0x023456789ABCDEF0, 7, 3, elem),
                  R.normal_f64(0x123456789ABCDEF0, 8, 3, elem), R.normal_f64(0x123456789ABCDEF0, 7, 4, elem),
                  R.normal_f64(0x123456789ABCDEF0, 7, 3, elem + np.uint64(1))):
        assert not np.any(other == base)


@pytest.mark.parametrize("i", [990, 10])
@pytest.mark.parametrize("coef,div", R.PLMS_COEFFS)
@pytest.mark.parametrize("rows,C", [(1, 100), (3, 100), (257, 100), (257, 99)])
def test_plms_f32_meets_bound(rows, C, coef, div, i):
    """A float32 evaluation of the PLMS update stays within the bound the GPU test uses, on that test's inputs."""
    d, A, Bc = R.plms_step_coeffs(R.schedule(), i, 10)
    x, e = R.plms_inputs(rows, C, len(coef))
    e32, x32 = R.plms_f32(x, e, coef, div, d, A, Bc)
    assert e32.dtype == np.float32 and x32.dtype == np.float32
    e_ref, be, x_ref, bx = R.plms_ref(x, e, coef, div, d, A, Bc)
    assert np.all(np.abs(e32 - e_ref) <= be)
    assert np.all(np.abs(x32 - x_ref) <= bx)
    # and the bound is not slack enough to hide a swapped or sign-flipped coefficient
    if len(coef) > 1:
        sw = list(coef)
        sw[0], sw[1] = sw[1], sw[0]
        if sw != list(coef):
            _, xs = R.plms_f32(x, e, sw, div, d, A, Bc)
            assert np.mean(np.abs(xs - x_ref) > bx) > 0.9


def test_plms_coeffs_match_oracle():
    """(d, A, Bc) give the oracle's plms_x_pred (torch float32) to float32 rounding."""
    import torch
    from oracle import models as OM
    sch = R.schedule()
    x, e = R.plms_inputs(5, 100, 1)
    for i, itv in [(990, 10), (10, 10), (750, 250), (0, 10)]:
        d, A, Bc = R.plms_step_coeffs(sch, i, itv)
        ref = OM.plms_x_pred(torch.from_numpy(x)[None], torch.from_numpy(e[0])[None], torch.tensor([i]), itv,
                             torch.from_numpy(sch["ac"]))[0].numpy()
        _, _, x_ref, bx = R.plms_ref(x, e, (1.0,), 1.0, d, A, Bc)
        assert np.all(np.abs(ref - x_ref) <= bx)


@pytest.mark.parametrize("i", [999, 500, 1, 0])
@pytest.mark.parametrize("rows", [1, 150])
def test_ddpm_f32_meets_bound(rows, i):
    """A float32 evaluation of p_sample stays within the GPU test's bound on that test's inputs, the oracle's ddpm_step
    (torch float32) too, and the inputs exercise both sides of the clip and its inside."""
    import torch
    from oracle import models as OM
    from svc_inference_pipeline_amd import config as C
    sch = R.schedule()
    co = R.ddpm_step_coeffs(sch, i)
    assert (co[4] == 0) == (i == 0)
    x, eps, z = R.ddpm_inputs(rows, 100, co[0], co[1])
    worst, pre = R.ddpm_err_over_bound(R.ddpm_f32(x, eps, z, *co), x, eps, z, co)
    assert worst <= 1.0
    if rows > 1:
        for part in (pre < -1, np.abs(pre) < 1, pre > 1):
            assert 0.25 < part.mean() < 0.42
    consts = OM.schedule_constants(C.noise_schedule(C.load_config().mapper))
    t = lambda a: torch.from_numpy(a)[None]
    ref = OM.ddpm_step(t(x), t(eps), i, t(z), consts)[0].numpy()
    assert R.ddpm_err_over_bound(ref, x, eps, z, co)[0] <= 1.0
    # a clip at 0.99 instead of 1 is outside the bound wherever the clip acts from above (c1 = 1 at step 0)
    if i == 0 and rows > 1:
        f = np.float32
        bad = f(co[2]) * np.minimum(np.maximum(f(co[0]) * x - f(co[1]) * eps, f(-1.0)), f(0.99)) + f(co[3]) * x
        assert R.ddpm_err_over_bound(bad, x, eps, z, co)[0] > 1.0


def test_op16_bits():
    """The 16-bit roundings used to check the x16 copies agree with torch's."""
    import torch
    v = np.concatenate([np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 3,
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 5.77, -5.77, 1e-8], np.float32)])
    t = torch.from_numpy(v)
    assert np.array_equal(R.op16_bits(v, False), t.to(torch.float16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.op16_bits(v, True), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
