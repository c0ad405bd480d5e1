"""Reference arithmetic and the assertions of the amp_conv op-level parity tests (csrc/amp_conv.hip: BigVGAN's fused
SnakeBeta Activation1d + dilated conv + epilogue, and its plain-conv form that runs the rate-2 up-sampling).

The assertions live here, written against a small backend interface, so that the same code checks the GPU library
(tests/test_gpu_ops.py) and a torch-CPU emulation of the kernel's arithmetic with deliberate defects
(tests/test_amp_ref.py): the CPU suite proves that every check can fail.

A backend provides
  amp_conv(x, x16, al, be, f, w, bias, k, d, tv, tv_mul, add_row, acc32, acc_div, out32, out16) -> (out32, out16)
      x [B, L, C] f32 (f16-valued when x16), w [C, C, k], tv a list of B ints or None; out32 / out16 are the arrays the
      outputs start from (None: not requested; out32 the string "acc32": the f32 output IS the acc32 operand)
  ups_comb(x, w, bias, k, s, tv, tv_mul, out) -> out [B, s*T, cout]      x [B, T, cin] f16-valued, w [cin, cout, k]
  ups_phase(x, w, bias, k, s) -> [B, s*T, cout] or None                  the phase-GEMM ConvTranspose1d, if there is one

Accumulation bound (fp32 sums of exact f16 x f16 products): |out - ref| <= 2 K 2^-24 S + 2^-23 |ref| with K the number
of products per output and S = sum |a||w| + |bias| + |add_row| + |acc32|. (K - 1) u S is the standard bound for any
fp32 summation order; the factor 2 covers the MFMA's internal grouping, the bias / operand adds and the acc_div
division. An f16 output adds half an f16 ulp, 2^-11 |ref|, with the reference clamped to +-65504.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import models as OM

SENT32 = np.float32(-7777.25)  # outputs start from these: rows a kernel must not write are compared bit for bit
SENT16 = np.float16(-1234.0)
F16_MAX = 65504.0


def tile_rows(C):
    """Output rows per workgroup (AmpCfg::BT)."""
    return 512 if C <= 48 else 256


def f16r(a):
    """Round to binary16, returned as f64."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def row_counts(B, L, tv, tv_mul):
    return [L] * B if tv is None else [min(L, int(t) * tv_mul) for t in tv]


def length_cases(C):
    """(name, B, L, tv, tv_mul): lengths one row either side of a tile and of two tiles, a ragged batch whose utterances
    end on, one past and far before a tile edge, the same with a frame multiplier (one product clamps at L), and
    lengths shorter than the activation's 6-row edge zone or than the conv padding."""
    BT = tile_rows(C)
    L = 2 * BT + 40
    cases = [("L%d" % n, 2, n, None, 1) for n in (BT - 1, BT, BT + 1, 2 * BT + 1)]
    cases.append(("ragged", 4, L, [L, BT, BT + 1, 7], 1))
    cases.append(("ragged_mul8", 4, L, [L // 8 + 3, BT // 8, BT // 8 + 1, 1], 8))
    cases += [("L%d" % n, 2, n, None, 1) for n in (1, 2, 5, 13)]
    return cases


def ups_cases(cin):
    BT = tile_rows(cin)
    T = BT + 24
    cases = [("T%d" % n, 2 if n < BT else 1, n, None, 1) for n in (1, 2, 40, BT - 1, BT, BT + 1)]
    cases.append(("ragged", 3, T, [T, BT, 1], 1))
    cases.append(("ragged_mul4", 3, T, [T // 4 + 2, BT // 4, 1], 4))
    return cases


def make_inputs(C, x16, B, L, seed=5):
    from svc_inference_pipeline_amd import weights as W
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, C, generator=g) * 2
    if x16:
        x = x.half().float()
    al = torch.randn(C, generator=g) * 0.3
    be = torch.randn(C, generator=g) * 0.3
    f = W.kaiser_sinc_filter1d(0.25, 0.3, 12).view(-1)
    return x.numpy(), al.numpy(), be.numpy(), f.numpy()


def act_ref(x, Lbs, al, be, f):
    """Activation1d (oracle.models.activation1d, in f64) of every utterance truncated to its own length: the
    up-sampler's replicate padding happens at Lb, not at L. x [B, L, C] -> f64 [B, L, C], rows past Lb zero."""
    out = np.zeros(x.shape, np.float64)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    for b, Lb in enumerate(Lbs):
        y = OM.activation1d(t(x[b, :Lb].T[None]), t(al), t(be), t(f))
        out[b, :Lb] = y[0].numpy().T
    return out


def conv_ref64(a_taps, w, bias, add_row=None, acc32=None, acc_div=1.0):
    """f64 sum over taps and channels of the given f16-valued A operands (a_taps[j] [..., C]: what tap j reads for each
    output row) times f16-rounded weights w [Cout, C, k], through the epilogue v = conv + bias (+ add_row),
    v = (acc32 + v) / acc_div. Returns (ref, S) with S = sum |a||w| + |bias| + |add_row| + |acc32|."""
    w16 = f16r(w)
    ref = np.zeros(a_taps[0].shape[:-1] + (w.shape[0],), np.float64) + np.asarray(bias, np.float64)
    S = np.zeros_like(ref) + np.abs(np.asarray(bias, np.float64))
    for j, a in enumerate(a_taps):
        a = np.asarray(a, np.float64)
        ref += a @ w16[:, :, j].T
        S += np.abs(a) @ np.abs(w16[:, :, j]).T
    if add_row is not None:
        ref += np.asarray(add_row, np.float64)
        S += np.abs(np.asarray(add_row, np.float64))
    if acc32 is not None:
        ref = (np.asarray(acc32, np.float64) + ref) / acc_div
        S += np.abs(np.asarray(acc32, np.float64))
    return ref, S


def acc_bound(ref, S, K, out16=False):
    """The accumulation bound of the module docstring; returns (reference, bound), the reference clamped for f16."""
    if out16:
        ref = np.clip(ref, -F16_MAX, F16_MAX)
    bound = 2.0 * K * 2.0 ** -24 * S + 2.0 ** -23 * np.abs(ref)
    if out16:
        bound = bound + 2.0 ** -11 * np.abs(ref)
    return ref, bound


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_untouched(out, init, Lbs, what, rate=1):
    for b, Lb in enumerate(Lbs):
        assert np.array_equal(_bits(out[b, rate * Lb:]), _bits(init[b, rate * Lb:])), \
            "%s: utterance %d has rows past its end (%d) written" % (what, b, rate * Lb)


def assert_within(out, ref, bound, Lbs, what, rate=1):
    """Every element of the rows below each utterance's end within its bound; returns the largest err / bound."""
    worst = 0.0
    for b, Lb in enumerate(Lbs):
        n = rate * Lb
        o = np.asarray(out[b, :n], np.float64)
        assert np.isfinite(o).all(), "%s: utterance %d not finite" % (what, b)
        ratio = np.abs(o - ref[b, :n]) / bound[b, :n]
        if ratio.size:
            i = np.unravel_index(np.argmax(ratio), ratio.shape)
            assert ratio[i] <= 1.0, "%s: utterance %d row %d channel %d: |%.9g - %.9g| = %.3e, %.2f x the bound" % (
                what, b, i[0], i[1], o[i], ref[b, :n][i], abs(o[i] - ref[b, :n][i]), ratio[i])
            worst = max(worst, float(ratio[i]))
    return worst


def probe_weight(C, k, j):
    """w[co, ci, j] = delta(co, ci), zero elsewhere: the conv output IS the image row tap j reads (products with 1 and 0
    and sums with 0 are exact)."""
    w = np.zeros((C, C, k), np.float32)
    w[np.arange(C), np.arange(C), j] = 1.0
    return w


def run_probe(backend, inp, x16, k, d, j, tv, tv_mul, sl=slice(None)):
    x, al, be, f = inp
    xs = x[sl]
    init = np.full(xs.shape, SENT32, np.float32)
    tvs = None if tv is None else list(tv[sl])
    out, _ = backend.amp_conv(xs, x16, al, be, f, probe_weight(x.shape[2], k, j), np.zeros(x.shape[2], np.float32), k,
                              d, tvs, tv_mul, None, None, 1.0, init.copy(), None)
    return out, init


def check_tap_probes(backend, C, x16, B, L, tv, tv_mul, kds, taps=None, alone=True, seed=5):
    """(a) The activation image element by element. For each (k, d) and tap j, output row t reads image row
    t + (j - (k-1)/2) d of the tile that owns t: inside [0, Lb) it must match act_ref rounded to f16 within
    test_activation1d's two bounds (rel-L2 < 1e-3, max |d| / (|ref| + 1e-2) < 5e-3), outside it must be exactly 0, and
    output rows >= Lb must keep their bits. Every utterance of a batch must equal itself run alone, bit for bit.
    Returns (largest rel-L2, largest element ratio)."""
    inp = make_inputs(C, x16, B, L, seed)
    Lbs = row_counts(B, L, tv, tv_mul)
    ref16 = f16r(act_ref(inp[0], Lbs, *inp[1:]))
    worst_l2 = worst_el = 0.0
    for k, d in kds:
        for j in (taps(k) if taps else (0, (k - 1) // 2, k - 1)):
            what = "C=%d x16=%d k=%d d=%d tap %d" % (C, x16, k, d, j)
            out, init = run_probe(backend, inp, x16, k, d, j, tv, tv_mul)
            assert_untouched(out, init, Lbs, what)
            shift = (j - (k - 1) // 2) * d
            num = den = 0.0
            for b, Lb in enumerate(Lbs):
                o = out[b, :Lb].astype(np.float64)
                assert np.array_equal(f16r(o), o), what + ": not f16 values (the probe does not read the image)"
                src = np.arange(Lb) + shift
                inside = (src >= 0) & (src < Lb)
                assert np.all(o[~inside] == 0.0), "%s: utterance %d reads non-zero rows outside [0, %d)" % (what, b, Lb)
                got, exp = o[inside], ref16[b, src[inside]]
                if got.size:
                    el = np.abs(got - exp) / (np.abs(exp) + 1e-2)
                    i = np.unravel_index(np.argmax(el), el.shape)
                    assert el[i] < 5e-3, "%s: utterance %d row %d channel %d: %.7g against %.7g" % (
                        what, b, np.arange(Lb)[inside][i[0]], i[1], got[i], exp[i])
                    worst_el = max(worst_el, float(el[i]))
                    num += float(np.sum((got - exp) ** 2))
                    den += float(np.sum(exp ** 2))
            if den > 0:
                l2 = (num / den) ** 0.5
                assert l2 < 1e-3, "%s: rel-L2 %.3e" % (what, l2)
                worst_l2 = max(worst_l2, l2)
            if alone and B > 1:
                for u in range(B):
                    o1, _ = run_probe(backend, inp, x16, k, d, j, tv, tv_mul, slice(u, u + 1))
                    assert np.array_equal(_bits(o1[0]), _bits(out[u])), \
                        "%s: utterance %d differs from itself run alone" % (what, u)
    return worst_l2, worst_el


EPILOGUES = ("c1", "c2", "c2_inplace", "mean16", "mean32")


def check_epilogues(backend, C, x16, B, L, tv, tv_mul, k, d, seed=5):
    """(b) Conv + every production epilogue against conv_ref64 of the kernel's own A operands (the k tap probes of the
    same case: same padding, tiles and runs), under the accumulation bound with K = k C; rows past Lb keep their bits
    in every output. Returns the largest err / bound of the f32 outputs and of the f16 outputs (an f16 output's bound
    is mostly its own half ulp, which a rounding reaches: that ratio lies near 1 by construction)."""
    inp = make_inputs(C, x16, B, L, seed)
    x, al, be, f = inp
    Lbs = row_counts(B, L, tv, tv_mul)
    a_taps = []
    for j in range(k):
        o, _ = run_probe(backend, inp, x16, k, d, j, tv, tv_mul)
        for b, Lb in enumerate(Lbs):
            o[b, Lb:] = 0.0
        a_taps.append(o.astype(np.float64))
    g = torch.Generator().manual_seed(seed + 100)
    w = (torch.randn(C, C, k, generator=g) / np.sqrt(C * k)).numpy()
    bias = (torch.randn(C, generator=g) * 0.1).numpy()
    add = torch.randn(B, L, C, generator=g).numpy()
    acc = torch.randn(B, L, C, generator=g).numpy()
    i32 = np.full(x.shape, SENT32, np.float32)
    i16 = np.full(x.shape, SENT16, np.float16)
    worst = {False: 0.0, True: 0.0}
    for name in EPILOGUES:
        what = "C=%d x16=%d k=%d d=%d %s" % (C, x16, k, d, name)
        use_add = name != "c1"
        use_acc = name in ("c2_inplace", "mean16", "mean32")
        div = 3.0 if name in ("mean16", "mean32") else 1.0
        o16 = name in ("c1", "mean16")
        ref, S = conv_ref64(a_taps, w, bias, add if use_add else None, acc if use_acc else None, div)
        ref, bound = acc_bound(ref, S, k * C, o16)
        if o16:
            _, out = backend.amp_conv(x, x16, al, be, f, w, bias, k, d, tv, tv_mul, add if use_add else None,
                                      acc.copy() if use_acc else None, div, None, i16.copy())
            init = i16
        else:
            alias = name in ("c2_inplace", "mean32")  # as svc_bigvgan: the resblock sum is updated in place
            out, _ = backend.amp_conv(x, x16, al, be, f, w, bias, k, d, tv, tv_mul, add,
                                      acc.copy() if use_acc else None, div, "acc32" if alias else i32.copy(), None)
            init = acc if alias else i32
        assert_untouched(out, init, Lbs, what)
        worst[o16] = max(worst[o16], assert_within(out, ref, bound, Lbs, what))
    return worst[False], worst[True]


def check_saturation(backend, C, x16, B, L, tv, tv_mul, k, d, seed=5):
    """A bias of 1e5 in two channels: the f16 output reads 65504 there and is finite everywhere."""
    x, al, be, f = make_inputs(C, x16, B, L, seed)
    Lbs = row_counts(B, L, tv, tv_mul)
    g = torch.Generator().manual_seed(seed + 200)
    w = (torch.randn(C, C, k, generator=g) / np.sqrt(C * k)).numpy()
    bias = (torch.randn(C, generator=g) * 0.1).numpy()
    hot = [1, C - 3]
    bias[hot] = 1e5
    init = np.full(x.shape, SENT16, np.float16)
    _, out = backend.amp_conv(x, x16, al, be, f, w, bias, k, d, tv, tv_mul, None, None, 1.0, None, init.copy())
    assert_untouched(out, init, Lbs, "saturation")
    for b, Lb in enumerate(Lbs):
        assert np.isfinite(out[b, :Lb].astype(np.float32)).all()
        assert np.all(out[b, :Lb][:, hot].astype(np.float32) == F16_MAX)
        cold = np.delete(out[b, :Lb].astype(np.float32), hot, axis=1)
        assert np.all(np.abs(cold) < 100.0)


def check_ups(backend, cin, B, T, tv, tv_mul, seed=9, k=4, s=2):
    """(c) The combined rate-2 up-sampling against an f64 conv_transpose1d of the f16-rounded input and weights
    (K = 2 cin live products per output); rows >= 2 Lb keep their bits; at cin 96 / 192 bit-identical to the phase
    GEMMs on the same input (every utterance against itself alone at its own length). Returns the largest
    err / bound."""
    cout = cin // 2
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, T, cin, generator=g)).half().float().numpy()
    w = (torch.randn(cin, cout, k, generator=g) / np.sqrt(cin * k / s)).numpy()
    bias = (torch.randn(cout, generator=g) * 0.1).numpy()
    Lbs = row_counts(B, T, tv, tv_mul)
    init = np.full((B, s * T, cout), SENT32, np.float32)
    out = backend.ups_comb(x, w, bias, k, s, tv, tv_mul, init.copy())
    what = "ups cin=%d T=%d tv=%r x%d" % (cin, T, tv, tv_mul)
    assert_untouched(out, init, Lbs, what, rate=s)
    w64 = torch.from_numpy(f16r(w))
    b64 = torch.from_numpy(bias.astype(np.float64))
    ref = np.zeros(out.shape, np.float64)
    S = np.ones(out.shape, np.float64)
    for b, Lb in enumerate(Lbs):
        xb = torch.from_numpy(x[b, :Lb].astype(np.float64).T[None])
        ref[b, :s * Lb] = F.conv_transpose1d(xb, w64, b64, stride=s, padding=(k - s) // 2)[0].numpy().T
        S[b, :s * Lb] = F.conv_transpose1d(xb.abs(), w64.abs(), b64.abs(), stride=s, padding=(k - s) // 2)[0].numpy().T
    ref, bound = acc_bound(ref, S, 2 * cin)
    worst = assert_within(out, ref, bound, Lbs, what, rate=s)
    if cin in (96, 192):
        for b, Lb in enumerate(Lbs):
            ph = backend.ups_phase(x[b:b + 1, :Lb], w, bias, k, s)
            if ph is not None:
                assert np.array_equal(_bits(ph[0]), _bits(out[b, :s * Lb])), \
                    "%s: utterance %d differs from the phase GEMMs" % (what, b)
    return worst
