"""numpy references of shallow diffusion's start state (csrc/elementwise.hip q_sample), float64: the reference's
normalize_mel_channel (utils/acoustic_feature_extraction.py:75-80, no clamp) and Diff-SVC's q_sample at noise level
K - 1, x_K = sqrt(ac[K - 1]) y + sqrt(1 - ac[K - 1]) z, with the forward draw z keyed like the sampler's other device
noise (sampler_ref.normal_f64) under a step word of its own."""
import numpy as np

import sampler_ref as R

Q_STEP = 0xFFFFFFFE  # the counter word "step" of the forward draw (x_T: 0xFFFFFFFF, DDPM step i: i)


def normalize_mel_channel(mel, mel_min, mel_max):
    """mel [..., C], mel_min / mel_max [C] -> (mel - mel_min) / (mel_max - mel_min + 1e-12) * 2 - 1 in float64."""
    mel, mn, mx = (np.asarray(a, np.float64) for a in (mel, mel_min, mel_max))
    return (mel - mn) / (mx - mn + 1e-12) * 2 - 1


def q_coeffs(sch, K):
    """(sqrt(ac[K - 1]), sqrt(1 - ac[K - 1])) in float32, operation by operation as sample_impl forms them from the
    float32 alphas_cumprod table (sampler_ref.schedule())."""
    ac = sch["ac"][K - 1]
    a, b = np.sqrt(ac), np.sqrt(np.float32(1.0) - ac)
    assert isinstance(a, np.float32) and isinstance(b, np.float32)
    return a, b


def q_noise(seed, utt_ids, T, C):
    """The forward draw z [B, T, C] float64 of utterances utt_ids."""
    return R.noise_block(seed, utt_ids, Q_STEP, T, C)


def q_sample(y, a, b, z):
    """x_K = a y + b z in float64 (a, b the float32 coefficients, taken exactly)."""
    return float(a) * np.asarray(y, np.float64) + float(b) * np.asarray(z, np.float64)


def q_sample_bound(y, a, b, z, drawn):
    """The element-wise bound the GPU test holds svc_op_q_sample to. With z drawn on the device its libm error enters
    scaled by b: b * NOISE_ATOL (sampler_ref: the draw's own bound). The float32 arithmetic is at most eight roundings
    (mel - mn, mx - mn, + 1e-12, the quotient, * 2 - 1 as one or two, b z, the multiply-add) on intermediates no larger
    than 1 + |y| or |b z|: 8 u (1 + |y| + |b z|), u = 2^-24."""
    y, z = np.asarray(y, np.float64), np.asarray(z, np.float64)
    arith = 8 * R.F32_U * (1 + np.abs(y) + np.abs(float(b) * z))
    return (float(b) * R.NOISE_ATOL if drawn else 0.0) + arith


def mel_for_range(rng, shape, mel_min, mel_max, lo=-1.2, hi=1.2):
    """float32 mel [..., C] whose normalised value is uniform over about [lo, hi]: out-of-range frames on both sides."""
    y = rng.uniform(lo, hi, shape)
    mn, mx = np.asarray(mel_min, np.float64), np.asarray(mel_max, np.float64)
    return ((y + 1) / 2 * (mx - mn + 1e-12) + mn).astype(np.float32)
