"""numpy references of the sampler's element-wise kernels (csrc/elementwise.hip): the counter-based normal draw
(Philox4x32-10 + Box-Muller) behind x_T and the DDPM step noise, the PLMS update and the DDPM p_sample step, all in
float64, with the element-wise error bounds the GPU tests (tests/test_gpu_sampler_ops.py) hold the kernels to.
tests/test_sampler_ref.py checks this file itself on the CPU (known answers, moments, and that a plain float32
evaluation of each formula meets its bound).

Bounds. u = 2^-24 is float32's unit roundoff. An update is about a dozen float32 roundings (FMA contraction allowed), so
each output is held to 16 u times the sum of the magnitudes of its terms: measured against the magnitudes, not the
result, so that the cancellation of the Adams-Bashforth combinations is covered."""
import numpy as np

U32 = np.uint64(0xFFFFFFFF)
F32_U = 2.0 ** -24
XT_STEP = 0xFFFFFFFF  # the counter word "step" of the x_T draw
NOISE_ATOL = 1e-5     # |z_gpu - std z_ref|: device libm error on values <= sqrt(2 ln 2^24) = 5.77 (8 ulp = 3.8e-6)

# the five PLMS combinations (modules/diffsvcrepo_inference.py:117-147): the first step's predictor and corrector,
# then Adams-Bashforth of order 2, 3, 4
PLMS_COEFFS = [((1.0,), 1.0), ((1.0, 1.0), 2.0), ((3.0, -1.0), 2.0), ((23.0, -16.0, 5.0), 12.0),
               ((55.0, -59.0, 37.0, -9.0), 24.0)]


# ------------------------------------------------------------------ Philox4x32-10 + Box-Muller
def philox4x32_10(counter, key):
    """Random123 philox4x32-10: counter [4], key [2] (each word an integer or an array of them) -> 4 words, uint64
    arrays holding 32-bit values."""
    c = [np.asarray(w, dtype=np.uint64) & U32 for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & U32 for w in key]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c[0]  # 32 x 32 -> 64 bits: exact in uint64
        p1 = m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & U32, (p0 >> s32) ^ c[3] ^ k[1], p0 & U32]
        k = [(k[0] + w0) & U32, (k[1] + w1) & U32]
    return c


def uniforms(seed, utt, step, elem):
    """The two Box-Muller uniforms of one draw, float64 (both exact in float32): u1 in (0, 1], u2 in [0, 1)."""
    seed = int(seed)
    c = philox4x32_10([elem, int(step) & 0xFFFFFFFF, int(utt) & 0xFFFFFFFF, 0x5356434B],
                      [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    s8 = np.uint64(8)
    u1 = ((c[0] >> s8) + np.uint64(1)).astype(np.float64) / 16777216.0
    u2 = (c[1] >> s8).astype(np.float64) / 16777216.0
    return u1, u2


def normal_f64(seed, utt, step, elem):
    """The N(0, 1) draw keyed by (seed u64, utterance id, step, element index t * C + c), float64. The angle is the
    float32 product float32(2 pi) * float32(u2), as the kernel forms it: that input rounding (up to 2.4e-7 rad) is part
    of the definition, what is left to the device is libm's logf / sqrtf / cosf."""
    u1, u2 = uniforms(seed, utt, step, elem)
    angle = (np.float32(6.283185307179586) * u2.astype(np.float32)).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(angle)


def noise_block(seed, utt_ids, step, T, C):
    """[B, T, C] float64: utterance b's draws at elements t * C + c."""
    elem = np.arange(T * C, dtype=np.uint64)
    return np.stack([normal_f64(seed, int(u), step, elem).reshape(T, C) for u in utt_ids])


# ------------------------------------------------------------------ schedule coefficients
def schedule():
    """float64 betas of the committed configuration -> dict of the float32 tables the engine keeps (finalize.hip build_mapper, run by
    svc_ctx_finalize; modules/diffsvcrepo_inference.py:163-197)."""
    from svc_inference_pipeline_amd import config as C
    betas = C.noise_schedule(C.load_config().mapper)
    alphas = 1.0 - betas
    ac = np.cumprod(alphas)
    prev = np.append(1.0, ac[:-1])
    pv = betas * (1.0 - prev) / (1.0 - ac)
    f = lambda a: np.asarray(a, np.float32)
    return dict(ac=f(ac), sra=f(np.sqrt(1.0 / ac)), srm1=f(np.sqrt(1.0 / ac - 1)),
                c1=f(betas * np.sqrt(prev) / (1.0 - ac)), c2=f((1.0 - prev) * np.sqrt(alphas) / (1.0 - ac)),
                logvar=f(np.log(np.maximum(pv, 1e-20))))


def plms_step_coeffs(sch, i, interval):
    """(d, A, Bc) of the PLMS step t = i -> max(i - interval, 0), in float32 operation by operation as sample_impl
    (and the reference's tensor ops, :96-113) compute them."""
    f = np.float32
    a_t, a_prev = sch["ac"][i], sch["ac"][max(i - interval, 0)]
    a_t_sq, a_prev_sq = np.sqrt(a_t), np.sqrt(a_prev)
    A = f(1.0) / (a_t_sq * (a_t_sq + a_prev_sq))
    Bc = f(1.0) / (a_t_sq * (np.sqrt((f(1.0) - a_prev) * a_t) + np.sqrt((f(1.0) - a_t) * a_prev)))
    d = a_prev - a_t
    assert all(isinstance(v, np.float32) for v in (d, A, Bc))
    return d, A, Bc


def ddpm_step_coeffs(sch, i):
    """(sra, srm1, c1, c2, sigma) of DDPM step i as float32; sigma = exp(0.5 logvar) for i > 0, else 0."""
    sigma = np.exp(np.float32(0.5) * sch["logvar"][i]) if i > 0 else np.float32(0.0)
    return sch["sra"][i], sch["srm1"][i], sch["c1"][i], sch["c2"][i], np.float32(sigma)


# ------------------------------------------------------------------ PLMS update
def plms_inputs(rows, C, ne, seed=0):
    """x and ne independent histories, float32 [rows, C], N(0, 1): independent so that a swapped coefficient shows."""
    rng = np.random.default_rng([seed, rows, C, ne])
    x = rng.standard_normal((rows, C)).astype(np.float32)
    e = [rng.standard_normal((rows, C)).astype(np.float32) for _ in range(ne)]
    return x, e


def plms_ref(x, e, coef, div, d, A, Bc):
    """float64 e' = sum_k c_k e_k / div and x' = x + d (A x - Bc e') of float32 inputs, with their bounds:
    -> (e_avg, bound_e, x_out, bound_x)."""
    x = np.asarray(x, np.float64)
    d, A, Bc, div = float(d), float(A), float(Bc), float(div)
    terms = [float(c) * np.asarray(ek, np.float64) for c, ek in zip(coef, e)]
    e_avg = sum(terms) / div
    mag_e = sum(np.abs(t) for t in terms) / abs(div)
    x_out = x + d * (A * x - Bc * e_avg)
    bound_e = 16 * F32_U * mag_e
    bound_x = 16 * F32_U * (np.abs(x) + abs(d) * (np.abs(A * x) + abs(Bc) * mag_e))
    return e_avg, bound_e, x_out, bound_x


def plms_f32(x, e, coef, div, d, A, Bc):
    """The same formula evaluated in plain float32, in the kernel's order -> (e_avg, x_out)."""
    f = np.float32
    acc = f(coef[0]) * e[0]
    for c, ek in zip(coef[1:], e[1:]):
        acc = acc + f(c) * ek
    acc = acc / f(div)
    return acc, x + f(d) * (f(A) * x - f(Bc) * acc)


# ------------------------------------------------------------------ DDPM p_sample
def ddpm_inputs(rows, C, sra, srm1, seed=0):
    """x, eps, z float32 [rows, C], scaled so that sra x - srm1 eps ~ N(0, 2.32^2): a third below -1, a third inside,
    a third above +1 (P(|N(0, s^2)| < 1) = 1/3 at s = 2.32)."""
    rng = np.random.default_rng([seed, rows, C])
    s = 2.32 / np.sqrt(2.0)
    x = (rng.standard_normal((rows, C)) * (s / float(sra))).astype(np.float32)
    eps = (rng.standard_normal((rows, C)) * (s / float(srm1))).astype(np.float32)
    z = rng.standard_normal((rows, C)).astype(np.float32)
    return x, eps, z


def ddpm_ref(x, eps, z, sra, srm1, c1, c2, sigma):
    """float64 p_sample (clip_denoised) of float32 inputs -> (pre, out, out_unclipped, bound_pre, bound): pre the value
    before the clip, out_unclipped the result had the clip not acted; bound_pre = 16 u (|sra x| + |srm1 eps|),
    bound = 16 u (|c1| (|sra x| + |srm1 eps|) + |c2 x| + |sigma z|)."""
    x, eps, z = (np.asarray(a, np.float64) for a in (x, eps, z))
    sra, srm1, c1, c2, sigma = (float(v) for v in (sra, srm1, c1, c2, sigma))
    pre = sra * x - srm1 * eps
    mag_pre = np.abs(sra * x) + np.abs(srm1 * eps)
    tail = c2 * x + sigma * z
    out = c1 * np.clip(pre, -1.0, 1.0) + tail
    bound = 16 * F32_U * (abs(c1) * mag_pre + np.abs(c2 * x) + np.abs(sigma * z))
    return pre, out, c1 * pre + tail, 16 * F32_U * mag_pre, bound


def ddpm_f32(x, eps, z, sra, srm1, c1, c2, sigma):
    f = np.float32
    x0 = np.minimum(np.maximum(f(sra) * x - f(srm1) * eps, f(-1.0)), f(1.0))
    return f(c1) * x0 + f(c2) * x + f(sigma) * z


def ddpm_err_over_bound(got, x, eps, z, coeffs):
    """max of |got - ref| / bound over the elements; an element whose float64 pre-clip value lies within bound_pre of
    -1 or +1 may have gone to either side of the clip and is compared against both."""
    pre, out, out_un, bound_pre, bound = ddpm_ref(x, eps, z, *coeffs)
    got = np.asarray(got, np.float64)
    err = np.abs(got - out)
    near = np.abs(np.abs(pre) - 1.0) <= bound_pre
    err = np.where(near, np.minimum(err, np.abs(got - out_un)), err)
    return float(np.max(err / np.maximum(bound, 1e-300))), pre


# ------------------------------------------------------------------ 16-bit operand copies
def bf16_bits(x32):
    """bfloat16 bits (round to nearest even) of finite float32 values, uint16."""
    b = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def op16_bits(x32, bf16):
    """The 16-bit GEMM-operand copy of float32 values |v| <= 65504: binary16 bits, or bfloat16 bits."""
    return bf16_bits(x32) if bf16 else np.ascontiguousarray(x32, np.float32).astype(np.float16).view(np.uint16)
