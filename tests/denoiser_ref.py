"""Reference arithmetic, bounds and assertions of the DiffSVC denoiser's op-level parity tests: the six steps of
stage_diffsvc.hip (input projection, dilated conv + gate, residual projection, skip sum, head, conditioner projection)
behind svc_op_diffsvc_*.

As tests/amp_ref.py: the assertions live here, written against a backend, so that the same code checks the GPU library
(tests/test_gpu_denoiser_ops.py) and a torch-CPU emulation of each kernel's arithmetic with planted defects
(tests/test_denoiser_ref.py). All arithmetic is torch float64 on the backend's device.

A backend provides `device` and, on torch tensors of that device (16-bit tensors are float16, or bfloat16 with bf):
  gate(x: Guarded, B, T, w, bias, cp16, dil, tv, bf, y16)        x.t [B*T, 384]; tv an int32 tensor [B] or None
  res(g16, w, bias, sub, add, store_lo, lanes_cap, bf, hi, lo)   hi / lo [M, 384] updated in place
  melpre(x16, w, bias, add, bf, hi, lo)                          x16 [M, 104]
  skipsum(g16, NL, rows_total, row0, rows, w, bias, bf, s16)     g16 [NL * rows_total, 384], s16 [rows, 1152]
  head(s16, wsp, bsp, wout, bout, bf, eps)                       s16 [M, 1152], eps f32 [M, 100]
  condproj(cond, NL, w, bias, bf, cp16)                          cond f32 [M, 384], cp16 [NL * M, 768]
Outputs are views into Guarded buffers: sentinel guard rows before and after, which must keep their bits.

References. Each op's f64 reference is built from the 16-bit operand VALUES the kernel reads: activations as given,
weights rounded to the operand format as the packers round them (finalize.hip: enc16_host; split weights
w_hi = round16(w), w_lo = round16(w - w_hi), value w_hi + w_lo), f32 biases and vectors as given.

Bounds (per element, derived; u = 2^-24, u16 = 2^-11 for binary16 and 2^-8 for bfloat16).
  accumulation   2 K u S + 2 u |ref| (amp_ref.acc_bound) with S = sum |a||w| + |bias| + ... and K the number of
                 NON-ZERO products of that output (a zero product adds nothing to an fp32 sum, so (K - 1) u S holds
                 with K counted so; for dense operands it is the full K). Sparse probe rows / columns therefore have
                 bounds near u S, which a result carrying one 16-bit half only cannot meet.
  split operand  the three products hi w_hi + lo w_hi + hi w_lo leave out lo w_lo: sum |a_lo||w_lo| is added.
  split store    v -> hi = round16(v), lo = round16(v - hi): |hi + lo - v| <= u16^2 |v| (+ 2^-25 for binary16, whose
                 lo is a subnormal below 2^-14): 2^-22 |v| for binary16, 2^-16 |v| for bfloat16. Exact checks beside
                 it: hi is a 16-bit value nearest to hi + lo (|lo| at most half an ulp of hi; NOT round16(hi + lo) ==
                 hi: when v - hi lies within 2^-11 of half an ulp, lo rounds up to exactly half an ulp and hi + lo is
                 a tie whose even neighbour need not be hi; a correct split store reaches this about once per 6000
                 elements), and the third segment of a [hi | lo | hi] row repeats the first bit for bit.
  16-bit output  u16 |ref| (+ 2^-25 for binary16).
  epilogue       every f32 operation of the kernel's epilogue expression adds u times the magnitude of its result,
                 listed in each reference function.
  gate           pre-activation bounds dg, df propagate as 0.25 dg + df (|d sigmoid| <= 1/4, |d tanh| <= 1,
                 |sigmoid|, |tanh| <= 1), plus gate_allow(a, b) for gate_act's own arithmetic (common.h):
                   t1 = c1 a, t2 = c2 |b|: constant and product rounding, |dt| <= 2 u |t|
                   E1 = exp2(t1), E2 = exp2(t2): v_exp_f32, 1 ulp = 2^-23 relative, plus the argument error through
                     the exponential: rho_i = 2^-23 + 2 ln2 u |t_i|  (t1 clamped to 64)
                   d1 = 1 + E1 (u), den = fma(d1, E2, d1) (u), v_rcp_f32 (2^-23), num = 1 - E2 (u |num| and, the
                     cancellation at small |b|, the absolute rho_2 E2), the product (u)
                 => |r - sigmoid(a) tanh(b)| <= |r| (4 u + 2^-23 + rho_1 (1 - sigmoid(a)) + rho_2 E2 / (1 + E2))
                                                 + sigmoid(a) rho_2 E2 / (1 + E2) + 2^-63
                 (first order; 2^-63 covers the clamp at a < -44.4, where the result is at most 2^-64 against a true
                 value below 2^-64). tests/test_denoiser_ref.py confirms it with an f32 evaluation of gate_act
                 against f64 over a dense (a, b) grid, the clamp region and b = 0 included.

Rows past an utterance's end (gate, with tv): every form (gate_ws, conv_gemm4 LDS-staged and register epilogue) writes
every output row; a row at or past tv[b] holds the gate of the masked-input conv (its taps that reach back below tv[b]
read real rows, the others zero) plus its own cp row. That is pinned here for all forms: those rows are compared under
the same bound. Input rows at or past tv[b], and the guard rows around x, hold 3e4: a tap that reads one lands far
outside any bound.
"""
import math

import torch

C = 384
NMEL = 100
LDX = 104
U = 2.0 ** -24
POISON = 3e4
GUARD_ROWS = 16
F64 = torch.float64


def dt16(bf):
    return torch.bfloat16 if bf else torch.float16


def u16(bf):
    return 2.0 ** -8 if bf else 2.0 ** -11


def floor16(bf):
    return 0.0 if bf else 2.0 ** -25


def enc16(v, bf):
    """f32 tensor -> the operand format, as Op16::enc (binary16 saturates) / enc16_host."""
    v = v.to(torch.float32)
    return v.to(torch.bfloat16) if bf else v.clamp(-65504.0, 65504.0).to(torch.float16)


def r16(v, bf):
    return enc16(v, bf).to(F64)


def wsplit(w, bf):
    """pack_gemm_split3's weight halves as f64 values: (w_hi, w_lo)."""
    w = w.to(torch.float32)
    hi = enc16(w, bf)
    lo = enc16(w - hi.to(torch.float32), bf)
    return hi.to(F64), lo.to(F64)


def bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def rng(seed):
    return torch.Generator().manual_seed(seed)


class Guarded:
    """[rows, cols] tensor between GUARD_ROWS guard rows on each side, all pre-filled with `fill`."""

    def __init__(self, rows, cols, dtype, device, fill, init=None):
        self.fill = fill
        self.full = torch.full((rows + 2 * GUARD_ROWS, cols), fill, dtype=dtype, device=device)
        self.t = self.full[GUARD_ROWS:GUARD_ROWS + rows]
        if init is not None:
            self.t.copy_(init.to(dtype))
        self.init_bits = bits(self.full).clone()

    def assert_guards(self, what):
        b = bits(self.full)
        assert torch.equal(b[:GUARD_ROWS], self.init_bits[:GUARD_ROWS]), what + ": guard rows before the buffer written"
        assert torch.equal(b[-GUARD_ROWS:], self.init_bits[-GUARD_ROWS:]), what + ": guard rows after the buffer written"

    def assert_untouched(self, what):
        assert torch.equal(bits(self.full), self.init_bits), what + ": buffer written"


SENT16 = -1234.0
SENT32 = -7777.25


def nz_count(a, w):
    """[M, N] number of non-zero products of a [M, K] @ w [N, K]^T."""
    return (a != 0).to(torch.float32) @ (w != 0).to(torch.float32).T


def acc_bound(ref, S, K):
    return 2.0 * K.to(F64) * U * S + 2.0 * U * ref.abs()


def gemm64(a, w):
    """(a w^T, |a||w|^T, non-zero product count) for a [M, K], w [N, K] f64."""
    return a @ w.T, a.abs() @ w.abs().T, nz_count(a, w)


def split_gemm64(a_hi, a_lo, w_hi, w_lo):
    """The split-operand product of values a_hi + a_lo and w_hi + w_lo: (ref, S, K, omitted) with ref the full product,
    S / K over the kernel's three products and omitted = sum |a_lo||w_lo| (the product it leaves out)."""
    ref = (a_hi + a_lo) @ (w_hi + w_lo).T
    S = (a_hi.abs() + a_lo.abs()) @ w_hi.abs().T + a_hi.abs() @ w_lo.abs().T
    K = nz_count(a_hi, w_hi) + nz_count(a_lo, w_hi) + nz_count(a_hi, w_lo)
    return ref, S, K, a_lo.abs() @ w_lo.abs().T


def assert_within(out, ref, bound, what):
    """Every element within its bound; returns the largest err / bound."""
    out = out.to(F64)
    assert bool(torch.isfinite(out).all()), what + ": not finite"
    ratio = (out - ref).abs() / bound
    i = int(torch.argmax(ratio))
    r, c = divmod(i, ratio.shape[1])
    worst = float(ratio[r, c])
    assert worst <= 1.0, "%s: row %d column %d: |%.9g - %.9g| = %.3e, %.2f x the bound" % (
        what, r, c, float(out[r, c]), float(ref[r, c]), abs(float(out[r, c]) - float(ref[r, c])), worst)
    return worst


def assert_split(hi, lo, ref, bound, bf, what):
    """The split store: hi a nearest 16-bit value of hi + lo, hi + lo within bound + the split term of ref. Returns the
    largest err / bound."""
    h, v = hi.to(F64), hi.to(F64) + lo.to(F64)
    assert bool(torch.isfinite(v).all()), what + ": not finite"
    mag = bits(hi).to(torch.int32) & 0x7fff
    sgn = torch.where((bits(hi).to(torch.int32) & 0x8000) != 0, -1.0, 1.0).to(F64)
    dec = lambda m: m.to(torch.int16).view(dt16(bf)).to(F64)
    up, dn = dec(mag + 1), torch.where(mag > 0, dec((mag - 1).clamp(min=0)), -dec(torch.ones_like(mag)))
    va, ha = v * sgn, h * sgn
    near = ((va - ha).abs() <= (va - up).abs()) & ((va - ha).abs() <= (va - dn).abs())
    assert bool(near.all()), "%s: hi is not a nearest 16-bit value of hi + lo in %d elements" % (what, int((~near).sum()))
    return assert_within(v, ref, bound + u16(bf) ** 2 * ref.abs() + floor16(bf), what)


# ---------------------------------------------------------------------------------------------- gate arithmetic
def gate_allow(a, b):
    """Bound of gate_act's own f32 arithmetic at pre-activations (a, b) (module docstring)."""
    L2E = 1.4426950408889634
    t1 = (L2E * a.abs()).clamp(max=64.0)
    t2 = 2.0 * L2E * b.abs()
    rho1 = 2.0 ** -23 + 2.0 * math.log(2.0) * U * t1
    rho2 = 2.0 ** -23 + 2.0 * math.log(2.0) * U * t2
    sig = torch.sigmoid(a)
    e2 = torch.exp(-2.0 * b.abs())
    q = rho2 * e2 / (1.0 + e2)
    r = (sig * torch.tanh(b)).abs()
    return r * (4.0 * U + 2.0 ** -23 + rho1 * (1.0 - sig) + q) + sig * q + 2.0 ** -63


def gate_act_f32(a, b):
    """gate_act (common.h) evaluated in float32, operation by operation."""
    f = torch.float32
    a, b = a.to(f), b.to(f)
    t1 = (torch.tensor(-1.4426950408889634, dtype=f) * a).clamp(max=64.0)
    e1 = torch.exp2(t1)
    e2 = torch.exp2(torch.tensor(-2.8853900817779268, dtype=f) * b.abs())
    d1 = 1.0 + e1
    den = (d1.to(F64) * e2.to(F64) + d1.to(F64)).to(f)  # fmaf: one rounding
    r = (1.0 - e2) * (1.0 / den)
    return torch.copysign(r, b)


# ---------------------------------------------------------------------------------------------- references
def melpre_ref(x, w, bias, add, bf):
    """v = relu(x w16^T + bias) + add -> (ref, bound of hi + lo before the split term). f32 operations after the sum:
    + bias (in the accumulation's factor 2), + add: u |v|."""
    w16 = r16(w, bf)
    acc, S, K = gemm64(x[:, :NMEL].to(F64), w16)
    pre = acc + bias.to(F64)
    S = S + bias.to(F64).abs()
    v = pre.clamp(min=0.0) + add.to(F64)
    return v, acc_bound(pre, S, K) + U * v.abs()


def res_ref(g, hi0, lo0, w, bias, sub, add, bf, div=math.sqrt(2.0)):
    """v = ((hi0 + lo0) - sub + g w16^T + bias) / sqrt(2) + add. f32 operations: hi0 + lo0 exact (at most 23 bits
    apart), - sub: u |x - sub|, + (acc + bias): u |t|, the division (its f32 divisor is within 2^-25 of sqrt(2)): 2 u |q|,
    + add: u |v|."""
    w16 = r16(w, bf)
    acc, S, K = gemm64(g.to(F64), w16)
    x = hi0.to(F64) + lo0.to(F64)
    pre = acc + bias.to(F64)
    xs = x - sub.to(F64)
    t = xs + pre
    q = t / div
    v = q + add.to(F64)
    S = S + bias.to(F64).abs()
    bound = (acc_bound(pre, S, K) + U * xs.abs() + U * t.abs()) / div + 2.0 * U * q.abs() + U * v.abs()
    return v, bound


def gate_ref(x, B, T, w, bias, cp, dil, tv, bf):
    """y = sigmoid(g) tanh(f), [g | f] = conv1d_k3,dil(x masked at tv, zero padded per utterance) + bias + cp.
    x [B*T, C], cp [B*T, 2C] values -> (ref, bound) [B*T, C], every row (module docstring)."""
    w16 = r16(w, bf)  # [2C, C, 3]
    x = x.to(F64).reshape(B, T, C).clone()
    if tv is not None:
        for b in range(B):
            x[b, int(tv[b]):] = 0.0
    pre = torch.zeros(B, T, 2 * C, dtype=F64, device=x.device) + bias.to(F64)
    S = torch.zeros_like(pre) + bias.to(F64).abs()
    K = torch.zeros(B, T, 2 * C, dtype=torch.float32, device=x.device)
    for j in range(3):
        sh = (j - 1) * dil
        a = torch.zeros_like(x)
        lo, hi = max(0, -sh), min(T, T - sh)
        if hi > lo:
            a[:, lo:hi] = x[:, lo + sh:hi + sh]
        a2 = a.reshape(B * T, C)
        r, s, k = gemm64(a2, w16[:, :, j])
        pre += r.reshape(B, T, -1)
        S += s.reshape(B, T, -1)
        K += k.reshape(B, T, -1)
    cpv = cp.to(F64).reshape(B, T, 2 * C)
    pre = (pre + cpv).reshape(B * T, 2 * C)
    S = (S + cpv.abs()).reshape(B * T, 2 * C)
    d = acc_bound(pre, S, K.reshape(B * T, 2 * C)) + U * pre.abs()  # (the cp add: one more f32 rounding)
    a, b = pre[:, :C], pre[:, C:]
    ref = torch.sigmoid(a) * torch.tanh(b)
    bound = 0.25 * d[:, :C] + d[:, C:] + gate_allow(a, b) + u16(bf) * ref.abs() + floor16(bf)
    return ref, bound


def skipsum_ref(g, NL, rows_total, row0, rows, w, bias, bf):
    """s = (sum_l g[l][row0 + r] w16[l]^T + f32(sum_l bias[l])) / sqrt(NL). f32 operations: the bias sum's rounding
    u |bsum|, the scale 1 / sqrtf(NL) (sqrtf, the division and the product: 3 u |s|)."""
    w16 = r16(w, bf).reshape(NL, C, C)
    gg = g.to(F64).reshape(NL, rows_total, C)[:, row0:row0 + rows]
    a = gg.permute(1, 0, 2).reshape(rows, NL * C)
    wk = w16.permute(1, 0, 2).reshape(C, NL * C)
    acc, S, K = gemm64(a, wk)
    bsum = bias.to(F64).reshape(NL, C).sum(0)
    pre = acc + bsum
    S = S + bsum.abs()
    sc = 1.0 / math.sqrt(NL)
    ref = pre * sc
    return ref, (acc_bound(pre, S, K) + U * bsum.abs()) * sc + 3.0 * U * ref.abs()


def head_ref(s_hi, s_lo, wsp, bsp, wout, bout, bf):
    """eps = relu(s wsp^T + bsp) wout^T + bout on split operands -> (ref, bound) [M, NMEL]. u's bound (split-operand
    accumulation + its split store) propagates through |wout|; the second product's non-zero count takes every u that
    can be positive within its bound."""
    sp_hi, sp_lo = wsplit(wsp, bf)
    wo_hi, wo_lo = wsplit(wout, bf)
    upre, S, K, om = split_gemm64(s_hi.to(F64), s_lo.to(F64), sp_hi, sp_lo)
    upre = upre + bsp.to(F64)
    S = S + bsp.to(F64).abs()
    du = acc_bound(upre, S, K) + om
    u = upre.clamp(min=0.0)
    du = du + u16(bf) ** 2 * u + floor16(bf) * (upre + du > 0)
    ua = torch.where(upre + du > 0, (u + du), torch.zeros_like(u))  # |u| the kernel can hold
    wo = wo_hi + wo_lo
    ref = u @ wo.T + bout.to(F64)
    S2 = ua @ (wo_hi.abs() + wo_lo.abs()).T * (1.0 + u16(bf)) + bout.to(F64).abs()
    K2 = 3.0 * nz_count(ua, wo)
    om2 = (u16(bf) * ua) @ wo_lo.abs().T
    return ref, du @ wo.abs().T + acc_bound(ref, S2, K2) + om2


def cond_split(cond, bf):
    """f32_to_f16x3: (hi, lo) of the f32 conditioner rows."""
    cond = cond.to(torch.float32)
    hi = enc16(cond, bf)
    lo = enc16(cond - hi.to(torch.float32), bf)
    return hi, lo


def condproj_ref(cond, NL, w, bias, bf):
    """cp[l] = (c_hi + c_lo) (w_hi + w_lo)[l]^T + bias[l] -> (ref, bound) [NL * M, 2C], reference channel order."""
    c_hi, c_lo = cond_split(cond, bf)
    w_hi, w_lo = wsplit(w.reshape(NL * 2 * C, C), bf)
    ref, S, K, om = split_gemm64(c_hi.to(F64), c_lo.to(F64), w_hi, w_lo)
    b = bias.to(F64).reshape(1, NL * 2 * C)
    ref = ref + b
    bound = acc_bound(ref, S + b.abs(), K) + om + u16(bf) * ref.abs() + floor16(bf)
    M = cond.shape[0]
    lm = lambda t: t.reshape(M, NL, 2 * C).permute(1, 0, 2).reshape(NL * M, 2 * C)
    return lm(ref), lm(bound)


# ---------------------------------------------------------------------------------------------- inputs
def _sparse_rows(t, every, keep, g):
    """Rows m % every == every // 2 keep `keep` random columns only: probe rows with few non-zero products."""
    for m in range(every // 2, t.shape[0], every):
        idx = torch.randperm(t.shape[1], generator=g)[:keep]
        row = torch.zeros_like(t[m])
        row[idx] = t[m, idx]
        t[m] = row
    return t


def split_values(v, bf):
    """hi / lo 16-bit tensors of f32 values, as a split store leaves them."""
    hi = enc16(v, bf)
    return hi, enc16(v.to(torch.float32) - hi.to(torch.float32), bf)


def gate_inputs(B, T, tv, bf, seed=3):
    g = rng(seed)
    x = enc16(torch.randn(B * T, C, generator=g) * 1.5, bf)
    if tv is not None:
        xv = x.reshape(B, T, C)
        for b in range(B):
            xv[b, int(tv[b]):] = POISON
    w = torch.randn(2 * C, C, 3, generator=g) / math.sqrt(3 * C)
    bias = torch.randn(2 * C, generator=g) * 0.1
    cp = enc16(torch.randn(B * T, 2 * C, generator=g), bf)
    return x, w, bias, cp


def res_inputs(M, bf, seed=4):
    g = rng(seed)
    gate = _sparse_rows(torch.rand(M, C, generator=g) * 2 - 1, 7, 2, g)
    g16 = enc16(gate, bf)
    hi, lo = split_values(torch.randn(M, C, generator=g) * 4, bf)
    w = torch.randn(C, C, generator=g) / math.sqrt(C)
    bias, sub, add = (torch.randn(C, generator=g) * s for s in (0.1, 1.0, 1.0))
    return g16, hi, lo, w, bias, sub, add


def melpre_inputs(M, bf, seed=5):
    g = rng(seed)
    x = torch.zeros(M, LDX)
    x[:, :NMEL] = _sparse_rows(torch.randn(M, NMEL, generator=g), 5, 2, g)
    w = torch.randn(C, NMEL, generator=g) / math.sqrt(NMEL)
    bias, add = torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g)
    return enc16(x, bf), w, bias, add


def skipsum_inputs(NL, rows_total, bf, seed=6):
    """Rows r % 3 == 1 of every layer's block keep one channel: those output rows sum NL products (bound ~ 2 NL u S)."""
    g = rng(seed)
    gate = torch.rand(NL, rows_total, C, generator=g) * 2 - 1
    keep = torch.randint(0, C, (NL, rows_total), generator=g)
    probe = torch.zeros_like(gate).scatter_(2, keep[:, :, None], gate.gather(2, keep[:, :, None]))
    gate[:, 1::3] = probe[:, 1::3]
    gate = gate.reshape(NL * rows_total, C)
    w = torch.randn(NL, C, C, generator=g) / math.sqrt(C)
    bias = torch.randn(NL, C, generator=g) * 0.1
    return enc16(gate, bf), w, bias


HEAD_PROBE_U = (7, 200, 383)  # skip_projection rows with 2 non-zero weights and a positive bias
HEAD_PROBE_EPS = (3, 98)      # output_projection rows that read only those


def head_inputs(M, bf, seed=7):
    """Dense random weights, except: skip_projection rows HEAD_PROBE_U read two channels only (u there has a bound near
    u S), and output_projection rows HEAD_PROBE_EPS read only those u: eps there is exact to ~1e-6 relative with both
    halves of u and to 2^-12 with its high half alone."""
    g = rng(seed)
    s_hi, s_lo = split_values(torch.randn(M, C, generator=g), bf)
    wsp = torch.randn(C, C, generator=g) / math.sqrt(C)
    bsp = torch.randn(C, generator=g) * 0.3
    wout = torch.randn(NMEL, C, generator=g) / math.sqrt(C)
    bout = torch.randn(NMEL, generator=g) * 0.1
    for k in HEAD_PROBE_U:
        row = torch.zeros(C)
        row[[k // 2, (k * 5 + 1) % C]] = torch.tensor([0.37, -0.21])
        wsp[k] = row
        bsp[k] = 2.5
    for n in HEAD_PROBE_EPS:
        row = torch.zeros(C)
        row[list(HEAD_PROBE_U)] = torch.tensor([0.61, 0.43, 0.83])
        wout[n] = row
    return torch.cat([s_hi, s_lo, s_hi], 1).contiguous(), wsp, bsp, wout, bout


COND_PROBE_K = 11           # conditioner channel whose values lie in [1, 1.002)
COND_PROBE_O = (5, C + 70)  # output channels (reference order) of every layer that read it alone, bias = -weight


def condproj_inputs(M, NL, bf, seed=8):
    """Dense random weights, except output channels COND_PROBE_O of every layer: one weight w0 on conditioner channel
    COND_PROBE_K, whose values are 1 + d with d in [0, 2e-3), and bias -w0: the output w0 d (+ the weight split's
    residue) is 1e-3 of its terms, so its 16-bit rounding is far below the 2^-12 w0 that the low half of the
    conditioner (or of the weight) carries."""
    g = rng(seed)
    cond = torch.randn(M, C, generator=g)
    cond[:, COND_PROBE_K] = 1.0 + torch.rand(M, generator=g) * 2e-3
    w = torch.randn(NL, 2 * C, C, generator=g) / math.sqrt(C)
    bias = torch.randn(NL, 2 * C, generator=g) * 0.1
    for l in range(NL):
        for o in COND_PROBE_O:
            w0 = float(torch.rand(1, generator=g)) * 0.5 + 0.3
            w[l, o] = 0.0
            w[l, o, COND_PROBE_K] = w0
            bias[l, o] = -w[l, o, COND_PROBE_K]
    return cond, w, bias


# ---------------------------------------------------------------------------------------------- checks
def _dev(backend, *ts):
    return [None if t is None else t.to(backend.device) for t in ts]


def check_gate(backend, B, T, tv, dil, bf, seed=3, ref_cache=None):
    """The gate of one batch against gate_ref on every row; x between poison guard rows, y between sentinel guard
    rows. Returns the largest err / bound."""
    what = "gate B=%d T=%d dil=%d tv=%s bf16=%d" % (B, T, dil, "yes" if tv is not None else "no", bf)
    x, w, bias, cp = _dev(backend, *gate_inputs(B, T, tv, bf, seed))
    xg = Guarded(B * T, C, dt16(bf), backend.device, POISON, x)
    y = Guarded(B * T, C, dt16(bf), backend.device, SENT16)
    tvd = None if tv is None else torch.tensor([int(t) for t in tv], dtype=torch.int32, device=backend.device)
    backend.gate(xg, B, T, w, bias, cp, dil, tvd, bf, y.t)
    y.assert_guards(what)
    xg.assert_untouched(what + " input")
    key = (B, T, None if tv is None else tuple(int(t) for t in tv), dil, bf, seed)
    if ref_cache is not None and key in ref_cache:
        ref, bound = ref_cache[key]
    else:
        ref, bound = gate_ref(x, B, T, w, bias, cp, dil, tv, bf)
        if ref_cache is not None:
            ref_cache[key] = (ref, bound)
    return assert_within(y.t, ref, bound, what), y.t.clone()


def check_res(backend, M, lanes_cap, bf, seed=4):
    """The residual update in place with store_lo = 1 (reference, split checks, guards), then with store_lo = 0: hi bit
    equal; lo bit-untouched for res_proj (lanes_cap != -1), and, pinned, written as with store_lo = 1 by the tiled GEMM,
    which has no such form. Returns (largest err / bound, hi, lo)."""
    what = "res M=%d lanes_cap=%d bf16=%d" % (M, lanes_cap, bf)
    g16, hi0, lo0, w, bias, sub, add = _dev(backend, *res_inputs(M, bf, seed))
    ref, bound = res_ref(g16, hi0, lo0, w, bias, sub, add, bf)
    out = {}
    for store_lo in (1, 0):
        hi = Guarded(M, C, dt16(bf), backend.device, SENT16, hi0)
        lo = Guarded(M, C, dt16(bf), backend.device, SENT16, lo0)
        backend.res(g16, w, bias, sub, add, store_lo, lanes_cap, bf, hi.t, lo.t)
        hi.assert_guards(what + " hi")
        lo.assert_guards(what + " lo")
        out[store_lo] = (hi, lo)
    hi, lo = out[1]
    worst = assert_split(hi.t, lo.t, ref, bound, bf, what)
    assert torch.equal(bits(out[0][0].t), bits(hi.t)), what + ": hi differs between store_lo = 0 and 1"
    if lanes_cap != -1:
        out[0][1].assert_untouched(what + " store_lo = 0: lo")
    else:
        assert torch.equal(bits(out[0][1].t), bits(lo.t)), what + ": the tiled GEMM's lo differs between store_lo values"
    return worst, hi.t.clone(), lo.t.clone()


def check_melpre(backend, M, bf, seed=5):
    what = "melpre M=%d bf16=%d" % (M, bf)
    x16, w, bias, add = _dev(backend, *melpre_inputs(M, bf, seed))
    ref, bound = melpre_ref(x16, w, bias, add, bf)
    hi = Guarded(M, C, dt16(bf), backend.device, SENT16)
    lo = Guarded(M, C, dt16(bf), backend.device, SENT16)
    backend.melpre(x16, w, bias, add, bf, hi.t, lo.t)
    hi.assert_guards(what + " hi")
    lo.assert_guards(what + " lo")
    return assert_split(hi.t, lo.t, ref, bound, bf, what), hi.t.clone(), lo.t.clone()


def check_skipsum(backend, NL, rows_total, row0, rows, bf, seed=6):
    what = "skipsum NL=%d rows %d+%d of %d bf16=%d" % (NL, row0, rows, rows_total, bf)
    g16, w, bias = _dev(backend, *skipsum_inputs(NL, rows_total, bf, seed))
    ref, bound = skipsum_ref(g16, NL, rows_total, row0, rows, w, bias, bf)
    s = Guarded(rows, 3 * C, dt16(bf), backend.device, SENT16)
    backend.skipsum(g16, NL, rows_total, row0, rows, w, bias, bf, s.t)
    s.assert_guards(what)
    hi, lo, hi2 = s.t[:, :C], s.t[:, C:2 * C], s.t[:, 2 * C:]
    assert torch.equal(bits(hi2), bits(hi)), what + ": the third segment is not the first"
    return assert_split(hi, lo, ref, bound, bf, what)


def check_head(backend, M, bf, seed=7):
    what = "head M=%d bf16=%d" % (M, bf)
    s16, wsp, bsp, wout, bout = _dev(backend, *head_inputs(M, bf, seed))
    ref, bound = head_ref(s16[:, :C], s16[:, C:2 * C], wsp, bsp, wout, bout, bf)
    eps = Guarded(M, NMEL, torch.float32, backend.device, SENT32)
    backend.head(s16, wsp, bsp, wout, bout, bf, eps.t)
    eps.assert_guards(what)
    return assert_within(eps.t, ref, bound, what), eps.t.clone()


def check_condproj(backend, M, NL, bf, seed=8):
    what = "condproj M=%d NL=%d bf16=%d" % (M, NL, bf)
    cond, w, bias = _dev(backend, *condproj_inputs(M, NL, bf, seed))
    ref, bound = condproj_ref(cond, NL, w, bias, bf)
    cp = Guarded(NL * M, 2 * C, dt16(bf), backend.device, SENT16)
    backend.condproj(cond, NL, w, bias, bf, cp.t)
    cp.assert_guards(what)
    return assert_within(cp.t, ref, bound, what)


# ---------------------------------------------------------------------------------------------- shapes
# (B, T, tv): the smallest shapes that reach gate_ws's edges: one and one-and-a-bit 16-row blocks, utterance ends
# inside blocks, past the 160-row ring, every row part populated, ragged batches, a full LDS length table; and the
# shapes gate_ws declines (more than 1024 utterances, T < 16), which must run conv_gemm4
GATE_SHAPES = {
    "1x16": (1, 16, None), "1x17": (1, 17, None), "3x37": (3, 37, None), "2x161": (2, 161, None),
    "2x700": (2, 700, None), "ragged4x301": (4, 301, [301, 17, 160, 299]), "ragged3x40": (3, 40, [9, 40, 1]),
    "1024x16tv": (1024, 16, [(7 * b) % 16 + 1 for b in range(1024)]),
    "1025x16": (1025, 16, None), "1x5": (1, 5, None), "3x15": (3, 15, None),
}
GATE_WS_DECLINES = ("1025x16", "1x5", "3x15")
RES_M = (1, 15, 16, 17, 83, 16 * 24 + 1)
RES_LANES = (-1, 0, -2, 1, 8, 24)
MELPRE_M = (1, 15, 16, 17, 300)
SKIPSUM_CASES = ((50, 0, 50), (150, 50, 100), (129, 1, 127))  # (rows_total, row0, rows), NL = 20
HEAD_M = (1, 127, 128, 129, 257, 1025, 11 * 128 + 5)
CONDPROJ_CASES = ((1, 3), (127, 3), (129, 3), (33, 20))  # (M, NL)
