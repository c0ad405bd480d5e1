"""numpy reference of the DPM-Solver++(2M) / DDIM sampler (csrc/elementwise.hip dpm_update, csrc/stage_diffsvc.hip
svc_diffsvc_sample_steps): the timestep lists, written independently of svc_inference_pipeline_amd/config.py; the step
coefficients; the element-wise update in float64 with its bound and in plain float32; the sampler loop; and an analytic
Gaussian denoiser whose probability-flow ODE has a closed-form end point, on which convergence is checked (the seeded
random mapper saturates the clip on ~91 % of the elements, so "converges to the fine-step limit" means nothing there).
tests/test_dpm_ref.py checks this file on the CPU, tests/test_gpu_dpm.py holds the kernels to it.

Bounds. As in sampler_ref.py: u = 2^-24, an update is under a dozen float32 roundings, each output is held to 16 u times
the sum of the magnitudes of its terms."""
import numpy as np

from sampler_ref import F32_U


# ------------------------------------------------------------------ timesteps
def log_snr(ac, K=None):
    """lambda_t = ln(ac_t / (1 - ac_t)) / 2 in float64 of the float32 alphas_cumprod table (levels 0..K-1)."""
    a = np.asarray(ac, np.float32).astype(np.float64)[:K]
    return 0.5 * np.log(a / (1.0 - a))


def timesteps(ac, K, n, spacing="logsnr"):
    """The n-step list from level K - 1: strictly decreasing ints in [0, K - 1] starting at K - 1. "logsnr": for each of
    the n targets evenly spaced from lambda_{K-1} to lambda_0 the nearest grid level (the first of equals), kept when
    strictly below the previous one; "uniform": floor((K - 1)(n - 1 - j) / (n - 1))."""
    if n < 1 or n > K or spacing not in ("logsnr", "uniform"):
        raise ValueError("timesteps: n in [1, K], spacing logsnr | uniform")
    if n == 1:
        return [K - 1]
    if spacing == "uniform":
        return [(K - 1) * (n - 1 - j) // (n - 1) for j in range(n)]
    lam = log_snr(ac, K)
    hi, lo = float(lam[0]), float(lam[K - 1])
    out = []
    for j in range(n):
        target = lo + (hi - lo) * j / (n - 1)
        best, best_d = 0, abs(float(lam[0]) - target)
        for t in range(1, K):  # a plain scan: the first minimum wins
            d = abs(float(lam[t]) - target)
            if d < best_d:
                best, best_d = t, d
        if not out or best < out[-1]:
            out.append(best)
    return out


# ------------------------------------------------------------------ coefficients
def step_coeffs(ac, t, s, h_prev=None):
    """The step t -> s < t in float64 from the float32 table: -> dict(h, a, b, w0, w1). a = sigma_s / sigma_t,
    b = -alpha_s expm1(-h), h = lambda_s - lambda_t; with h_prev (the previous step's h) w1 = -h / (2 h_prev) and
    w0 = 1 - w1 (the 2M extrapolation), else w0 = 1, w1 = 0."""
    a64 = np.asarray(ac, np.float32).astype(np.float64)
    at, as_ = float(a64[t]), float(a64[s])
    lam = lambda v: 0.5 * np.log(v / (1.0 - v))  # noqa: E731
    h = lam(as_) - lam(at)
    w1 = -h / (2.0 * h_prev) if h_prev else 0.0
    return dict(h=float(h), a=float(np.sqrt((1.0 - as_) / (1.0 - at))), b=float(-np.sqrt(as_) * np.expm1(-h)),
                w0=float(1.0 - w1), w1=float(w1))


def kernel_coeffs(sch, t, s, h_prev=None):
    """(sra, srm1, w0, w1, a, b) as float32, each rounded once: what the sampler hands dpm_update for the step t -> s."""
    c = step_coeffs(sch["ac"], t, s, h_prev)
    f = np.float32
    return sch["sra"][t], sch["srm1"][t], f(c["w0"]), f(c["w1"]), f(c["a"]), f(c["b"])


def final_coeffs(sch, t):
    """The final form at level t: only sra and srm1 are read."""
    z = np.float32(0.0)
    return sch["sra"][t], sch["srm1"][t], z, z, z, z


# ------------------------------------------------------------------ the update
def dpm_inputs(rows, C, sra, srm1, seed=0):
    """x, eps as sampler_ref.ddpm_inputs scales them (a third of sra x - srm1 eps below -1, inside, above +1) and an
    independent d_prev uniform in [-1, 1], float32 [rows, C]: independent so that a swapped coefficient shows."""
    from sampler_ref import ddpm_inputs
    x, eps, _ = ddpm_inputs(rows, C, sra, srm1, seed)
    d_prev = np.random.default_rng([seed, rows, C, 77]).uniform(-1.0, 1.0, (rows, C)).astype(np.float32)
    return x, eps, d_prev


def dpm_ref(x, eps, d_prev, coeffs, final):
    """float64 update of float32 inputs; coeffs = (sra, srm1, w0, w1, a, b), d_prev None: no history.
    -> dict(pre, d, d_un, x, x_un, bound_pre, bound_x): pre the value before the clip, *_un the results had the clip
    not acted, bound_pre = 16 u (|sra x| + |srm1 eps|) (also D's bound), bound_x = 16 u (|a x| + |b| (|w0| (|sra x| +
    |srm1 eps|) + |w1 d_prev|)), or bound_pre at the final step."""
    x, eps = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    sra, srm1, w0, w1, a, b = (float(v) for v in coeffs)
    pre = sra * x - srm1 * eps
    mag_pre = np.abs(sra * x) + np.abs(srm1 * eps)
    d = np.clip(pre, -1.0, 1.0)
    if final:
        return dict(pre=pre, d=d, d_un=pre, x=d, x_un=pre, bound_pre=16 * F32_U * mag_pre, bound_x=16 * F32_U * mag_pre)
    if d_prev is None:
        bar = lambda v: v  # noqa: E731
        mag_bar = mag_pre
    else:
        dp = np.asarray(d_prev, np.float64)
        bar = lambda v: w0 * v + w1 * dp  # noqa: E731
        mag_bar = abs(w0) * mag_pre + np.abs(w1 * dp)
    return dict(pre=pre, d=d, d_un=pre, x=a * x + b * bar(d), x_un=a * x + b * bar(pre),
                bound_pre=16 * F32_U * mag_pre, bound_x=16 * F32_U * (np.abs(a * x) + abs(b) * mag_bar))


def dpm_f32(x, eps, d_prev, coeffs, final):
    """The same formula in plain float32 (no fused multiply-add) -> (d, x_out)."""
    f = np.float32
    sra, srm1, w0, w1, a, b = (f(v) for v in coeffs)
    d = np.minimum(np.maximum(sra * x - srm1 * eps, f(-1.0)), f(1.0))
    if final:
        return d, d
    bar = d if d_prev is None else w0 * d + w1 * d_prev
    return d, a * x + b * bar


def err_over_bound(got_x, got_d, x, eps, d_prev, coeffs, final):
    """(max |x' - ref| / bound_x, max |D - ref| / bound_pre, pre); an element whose float64 pre-clip value lies within
    bound_pre of -1 or +1 may have gone to either side of the clip and is compared against both, as
    sampler_ref.ddpm_err_over_bound does. got_d None: only x'."""
    r = dpm_ref(x, eps, d_prev, coeffs, final)
    near = np.abs(np.abs(r["pre"]) - 1.0) <= r["bound_pre"]

    def worst(got, ref, ref_un, bound):
        got = np.asarray(got, np.float64)
        err = np.abs(got - ref)
        err = np.where(near, np.minimum(err, np.abs(got - ref_un)), err)
        return float(np.max(err / np.maximum(bound, 1e-300)))

    wx = worst(got_x, r["x"], r["x_un"], r["bound_x"])
    wd = worst(got_d, r["d"], r["d_un"], r["bound_pre"]) if got_d is not None else 0.0
    return wx, wd, r["pre"]


# ------------------------------------------------------------------ the loop
def sample_steps(denoise, x, ts, order, ac, sra=None, srm1=None, stats=None):
    """The sampler loop of svc_diffsvc_sample_steps: denoise(x, t) -> eps at each ts[j]; first order at j = 0, 2M from
    j = 1 when order is 2, the last entry returns D (first order). Works on numpy arrays or torch tensors (only
    arithmetic and clip / clamp are used). sra / srm1: the engine's float32 tables (default: float64 from ac).
    stats (a dict, optional) receives `clipped`, the number of elements the clip acted on."""
    a64 = np.asarray(ac, np.float32).astype(np.float64)
    clip = (lambda v: v.clamp(-1.0, 1.0)) if hasattr(x, "clamp") else (lambda v: np.clip(v, -1.0, 1.0))
    d_prev, h_prev, clipped = None, None, 0
    for j, t in enumerate(ts):
        eps = denoise(x, t)
        r = float(sra[t]) if sra is not None else float(np.sqrt(1.0 / a64[t]))
        rm1 = float(srm1[t]) if srm1 is not None else float(np.sqrt(1.0 / a64[t] - 1.0))
        pre = r * x - rm1 * eps
        d = clip(pre)
        clipped += int((d != pre).sum())
        if j + 1 == len(ts):
            x = d
            break
        second = order == 2 and j > 0
        c = step_coeffs(ac, t, ts[j + 1], h_prev if second else None)
        bar = c["w0"] * d + c["w1"] * d_prev if second else d
        x = c["a"] * x + c["b"] * bar
        d_prev, h_prev = d, c["h"]
    if stats is not None:
        stats["clipped"] = clipped
    return x


def ddim_eta0(denoise, x, ts, ac):
    """DDIM at eta = 0 as Song et al. write it, independent of the solver's form: x0 = (x - sqrt(1 - ac_t) eps) /
    sqrt(ac_t) clipped, eps re-derived from the clipped x0, x_s = sqrt(ac_s) x0 + sqrt(1 - ac_s) eps'; after the last
    entry x = x0."""
    a64 = np.asarray(ac, np.float32).astype(np.float64)
    for j, t in enumerate(ts):
        eps = denoise(x, t)
        x0 = np.clip((x - np.sqrt(1.0 - a64[t]) * eps) / np.sqrt(a64[t]), -1.0, 1.0)
        if j + 1 == len(ts):
            return x0
        e2 = (x - np.sqrt(a64[t]) * x0) / np.sqrt(1.0 - a64[t])
        s = ts[j + 1]
        x = np.sqrt(a64[s]) * x0 + np.sqrt(1.0 - a64[s]) * e2
    return x


# ------------------------------------------------------------------ the analytic case
class GaussianCase:
    """Data ~ N(mu_c, s^2) per channel: the exact eps is sigma_t (x - alpha_t mu) / (alpha_t^2 s^2 + sigma_t^2), the
    probability-flow ODE keeps (x - alpha_t mu) / sqrt(alpha_t^2 s^2 + sigma_t^2) constant, so from a state x at level
    K - 1 the exact end point is mu + s (x - alpha mu) / sqrt(alpha^2 s^2 + sigma^2)."""

    def __init__(self, ac, K, rows=50, C=100, s=0.1, seed=0):
        rng = np.random.default_rng(seed)
        self.ac = np.asarray(ac, np.float32).astype(np.float64)
        self.mu = rng.uniform(-0.4, 0.4, C)[None, :]
        self.s = s
        al, sg = np.sqrt(self.ac[K - 1]), np.sqrt(1.0 - self.ac[K - 1])
        # a start state of the forward marginal at level K - 1
        self.x_start = al * (self.mu + s * rng.standard_normal((rows, C))) + sg * rng.standard_normal((rows, C))
        self.exact = self.mu + s * (self.x_start - al * self.mu) / np.sqrt(al * al * s * s + sg * sg)

    def denoise(self, x, t):
        al2, sg2 = self.ac[t], 1.0 - self.ac[t]
        return np.sqrt(sg2) * (x - np.sqrt(al2) * self.mu) / (al2 * self.s ** 2 + sg2)
