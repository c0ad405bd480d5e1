"""The denoiser op-level parity checks (tests/denoiser_ref.py, run on the GPU by tests/test_gpu_denoiser_ops.py) on a
torch-CPU emulation of each kernel's arithmetic: 16-bit operands, f32 accumulation, the kernel's epilogue expression. A
correct f32 implementation meets every bound at every shape the GPU tests use, the references compose to the oracle's
denoiser, and each planted defect fails an assertion at every one of those shapes.

Planted defect -> the assertion that catches it (the message each test matches):
  res: lo not read ("lo_dropped")                     res hi + lo outside the bound (sparse g rows: bound ~ u S)
  res: divisor 1.40 ("div_140")                        res hi + lo outside the bound
  res: add = dproj_i, not dproj_{i+1} ("dproj_same")   res hi + lo outside the bound
  gate: a tap crosses an utterance end ("cross_end")   gate outside the bound (the neighbour's row, or a poison guard row)
  gate: a tap reads past tv[b] ("past_tv")             gate outside the bound (poison rows), shapes with tv
  head: u_lo dropped ("u_lo_dropped")                  head outside the bound at the probe columns HEAD_PROBE_EPS
  condproj: cond lo dropped ("cond_lo_dropped")        condproj outside the bound at the probe channels COND_PROBE_O
  skipsum: layer stride rows, not rows_total           skipsum outside the bound; at (50, 0, 50) rows == rows_total and
    ("stride_rows")                                    the two strides are the same computation: asserted to be clean
  every op: one 16-column block of 16 rows zeroed      that op outside the bound ("zero_block")
  every op: one row zeroed ("zero_row")                that op outside the bound
"""
import math
from types import SimpleNamespace

import pytest
import torch

import denoiser_ref as R
from oracle import models as OM

C, NMEL = R.C, R.NMEL
f32 = torch.float32


def _damage(out, mutant):
    """zero_block: rows [r0, r0 + 16) x columns 32..47 with r0 the middle 16-row block; zero_row: the middle row."""
    rows = out.shape[0]
    if mutant == "zero_block":
        r0 = (rows // 2) // 16 * 16
        out[r0:r0 + 16, 32:48] = 0
    elif mutant == "zero_row":
        out[rows // 2] = 0


class Emu:
    """denoiser_ref backend: the kernels' arithmetic in float32 on the CPU. `mutant` plants one defect."""
    device = "cpu"

    def __init__(self, mutant=None):
        self.mutant = mutant

    def gate(self, x, B, T, w, bias, cp16, dil, tv, bf, y16):
        w16 = R.enc16(w, bf).to(f32)
        full = x.full.to(f32)  # guard rows included: what a tap that leaves the batch finds there
        G = R.GUARD_ROWS
        if self.mutant != "past_tv" and tv is not None:
            full = full.clone()
            for b in range(B):
                full[G + b * T + int(tv[b]):G + (b + 1) * T] = 0.0
        acc = torch.zeros(B * T, 2 * C)
        t = torch.arange(B * T) % T
        for j in range(3):
            sh = (j - 1) * dil
            a = full[G + sh:G + sh + B * T].clone()
            if self.mutant != "cross_end":
                a[(t + sh < 0) | (t + sh >= T)] = 0.0
            acc += a @ w16[:, :, j].T
        pre = (acc + bias) + cp16.to(f32)
        y = R.gate_act_f32(pre[:, :C], pre[:, C:])
        _damage(y, self.mutant)
        y16.copy_(y.to(R.dt16(bf)))

    def res(self, g16, w, bias, sub, add, store_lo, lanes_cap, bf, hi, lo):
        w16 = R.enc16(w, bf).to(f32)
        v = g16.to(f32) @ w16.T + bias
        x = hi.to(f32) if self.mutant == "lo_dropped" else hi.to(f32) + lo.to(f32)
        div = torch.tensor(1.40 if self.mutant == "div_140" else 1.41421356237309515, dtype=f32)
        wv = ((x - sub) + v) / div + (sub if self.mutant == "dproj_same" else add)
        _damage(wv, self.mutant)
        h = R.enc16(wv, bf)
        if store_lo or lanes_cap == -1:
            lo.copy_(R.enc16(wv - h.to(f32), bf))
        hi.copy_(h)

    def melpre(self, x16, w, bias, add, bf, hi, lo):
        w16 = R.enc16(w, bf).to(f32)
        wv = (x16[:, :NMEL].to(f32) @ w16.T + bias).clamp(min=0.0) + add
        _damage(wv, self.mutant)
        h = R.enc16(wv, bf)
        hi.copy_(h)
        lo.copy_(R.enc16(wv - h.to(f32), bf))

    def skipsum(self, g16, NL, rows_total, row0, rows, w, bias, bf, s16):
        w16 = R.enc16(w, bf).to(f32).reshape(NL, C, C)
        stride = rows if self.mutant == "stride_rows" else rows_total
        acc = torch.zeros(rows, C)
        for l in range(NL):
            acc += g16[l * stride + row0:l * stride + row0 + rows].to(f32) @ w16[l].T
        bsum = bias.to(torch.float64).reshape(NL, C).sum(0).to(f32)
        v = (acc + bsum) * (torch.tensor(1.0, dtype=f32) / torch.sqrt(torch.tensor(float(NL), dtype=f32)))
        _damage(v, self.mutant)
        h = R.enc16(v, bf)
        s16.copy_(torch.cat([h, R.enc16(v - h.to(f32), bf), h], 1))

    @staticmethod
    def _split3(a_hi, a_lo, w, bf):
        w_hi = R.enc16(w, bf)
        w_lo = R.enc16(w.to(f32) - w_hi.to(f32), bf)
        return (a_hi.to(f32) @ w_hi.to(f32).T + a_lo.to(f32) @ w_hi.to(f32).T) + a_hi.to(f32) @ w_lo.to(f32).T

    def head(self, s16, wsp, bsp, wout, bout, bf, eps):
        u = (self._split3(s16[:, :C], s16[:, C:2 * C], wsp, bf) + bsp).clamp(min=0.0)
        u_hi = R.enc16(u, bf)
        u_lo = R.enc16(u - u_hi.to(f32), bf)
        if self.mutant == "u_lo_dropped":
            u_lo = torch.zeros_like(u_lo)
        e = self._split3(u_hi, u_lo, wout, bf) + bout
        _damage(e, self.mutant)
        eps.copy_(e)

    def condproj(self, cond, NL, w, bias, bf, cp16):
        c_hi, c_lo = R.cond_split(cond, bf)
        if self.mutant == "cond_lo_dropped":
            c_lo = torch.zeros_like(c_lo)
        v = self._split3(c_hi, c_lo, w.reshape(NL * 2 * C, C), bf) + bias.reshape(-1)
        M = cond.shape[0]
        v = v.reshape(M, NL, 2 * C).permute(1, 0, 2).reshape(NL * M, 2 * C).contiguous()
        _damage(v, self.mutant)
        cp16.copy_(R.enc16(v, bf))


_GATE_REFS = {}


def _gate(mutant, name, bf=0):
    B, T, tv = R.GATE_SHAPES[name]
    dil = (1, 2, 4, 8)[sorted(R.GATE_SHAPES).index(name) % 4]
    return R.check_gate(Emu(mutant), B, T, tv, dil, bf, ref_cache=_GATE_REFS)[0]


# ------------------------------------------------------------------ gate_act's arithmetic allowance
def test_gate_act_allowance():
    """gate_act in float32 against f64 sigmoid * tanh over a dense grid: the clamp region a < -44.4, saturated and
    tiny |b| and b = 0 included; every point within gate_allow, and the allowance is no blanket: at moderate arguments it
    stays below 16 f32 ulps of the result."""
    a = torch.cat([torch.linspace(-70.0, 40.0, 1101, dtype=R.F64), torch.tensor([-44.0, -44.36, -44.4, -45.0, 0.0], dtype=R.F64)])
    b = torch.cat([torch.linspace(-20.0, 20.0, 801, dtype=R.F64),
                   torch.tensor([0.0, 1e-30, -1e-30, 1e-7, -1e-7, 1e-4, 3e-3, -3e-3], dtype=R.F64)])
    A, Bv = torch.meshgrid(a.to(f32).to(R.F64), b.to(f32).to(R.F64), indexing="ij")
    got = R.gate_act_f32(A, Bv).to(R.F64)
    ref = torch.sigmoid(A) * torch.tanh(Bv)
    ratio = (got - ref).abs() / R.gate_allow(A, Bv)
    print("gate_act f32 emulation: largest err / allowance %.3f" % float(ratio.max()))
    assert bool(torch.isfinite(got).all()) and float(ratio.max()) <= 1.0
    assert bool((got[:, b == 0] == 0).all())
    mod = (A.abs() <= 8) & (Bv.abs() >= 0.25) & (Bv.abs() <= 8)
    assert float((R.gate_allow(A, Bv) / ref.abs())[mod].max()) < 16 * 2.0 ** -23


# ------------------------------------------------------------------ the clean emulation meets every bound
@pytest.mark.parametrize("name", sorted(R.GATE_SHAPES))
def test_emulation_passes_gate(name):
    for bf in (0, 1):
        if bf and R.GATE_SHAPES[name][0] > 1000:
            continue  # (the same arithmetic; the two large batches once)
        assert 0 < _gate(None, name, bf) <= 1.0


@pytest.mark.parametrize("bf", [0, 1])
def test_emulation_passes_the_other_ops(bf):
    worst = {}
    for M in R.RES_M:
        for lanes in (-1, 0):
            worst["res"] = max(worst.get("res", 0), R.check_res(Emu(), M, lanes, bf)[0])
    for M in R.MELPRE_M:
        worst["melpre"] = max(worst.get("melpre", 0), R.check_melpre(Emu(), M, bf)[0])
    for rt, r0, rows in R.SKIPSUM_CASES:
        worst["skipsum"] = max(worst.get("skipsum", 0), R.check_skipsum(Emu(), 20, rt, r0, rows, bf))
    for M in R.HEAD_M:
        worst["head"] = max(worst.get("head", 0), R.check_head(Emu(), M, bf)[0])
    for M, NL in R.CONDPROJ_CASES:
        worst["condproj"] = max(worst.get("condproj", 0), R.check_condproj(Emu(), M, NL, bf))
    print("emulation bf16=%d: largest err / bound %s" % (bf, {k: round(v, 3) for k, v in worst.items()}))
    assert all(0 < v <= 1.0 for v in worst.values())


def test_split_store_ties_exist():
    """The reason assert_split asks for "a nearest value", not round16(hi + lo) == hi: the correct split store reaches
    exact ties (lo rounded up to half an ulp of hi) whose even neighbour is not hi."""
    v = torch.randn(1000, 400, generator=R.rng(1)) * 4
    hi, lo = R.split_values(v, 0)
    s = hi.to(R.F64) + lo.to(R.F64)
    odd = int((s.to(torch.float16) != hi).sum())  # (a tie is exact in float64 and rounds to even here)
    print("split store: %d of %d elements re-round to the other neighbour" % (odd, v.numel()))
    assert 0 < odd < v.numel() // 1000
    R.assert_split(hi, lo, v.to(R.F64), torch.zeros_like(s) + 1e-30, 0, "ties")


# ------------------------------------------------------------------ the references compose to the oracle
def test_references_compose_to_the_oracle():
    """Two residual layers (melpre, gate, res, gate, skip sum, head, with both conditioner projections) composed from the
    reference functions on 16-bit-exact weights equal oracle.models.diffsvc_forward in float64 to rounding."""
    g = R.rng(21)
    B, T, NL, fc = 2, 9, 2, 16
    M = B * T
    rn = lambda *s: torch.randn(*s, generator=g).to(R.F64)
    # binary16 values, scaled before the rounding: the references' weight rounding is then the identity
    q16 = lambda *s, d=1: (torch.randn(*s, generator=g) / d).half().to(R.F64)
    sd = {}

    def put(name, w, b):
        sd[name + ".weight"], sd[name + ".bias"] = w, b

    put("1.mel_preprocess.projection", q16(C, NMEL, 1, d=8), q16(C, d=4))
    put("1.diffusion_embedding.projection1", rn(fc, 128) / 11, rn(fc))
    put("1.diffusion_embedding.projection2", rn(fc, fc) / 4, rn(fc))
    put("1.skip_projection", q16(C, C, 1, d=16), q16(C, d=4))
    put("1.output_projection", q16(NMEL, C, 1, d=16), q16(NMEL, d=4))
    L = ["1.residual_layers.%d." % i for i in range(NL)]
    for r in L:
        put(r + "dilated_conv", q16(2 * C, C, 3, d=32), q16(2 * C, d=4))
        put(r + "output_projection", q16(2 * C, C, 1, d=16), q16(2 * C, d=4))
        put(r + "conditioner_projection", q16(2 * C, C, 1, d=16), q16(2 * C, d=4))
        put(r + "diffusion_projection", rn(C, fc) / 4, rn(C))
    x, cond, table = q16(B, T, NMEL), q16(B, T, C), rn(5, 128)
    mcfg = SimpleNamespace(residual_layer_num=NL, dilation_cycle_length=4)
    want = OM.diffsvc_forward(sd, mcfg, x, cond, torch.tensor([3, 3]), table)
    # the step MLP and the layers' diffusion projections (finalize.hip precomputes them per step)
    lin = lambda name, v: sd[name + ".weight"] @ v + sd[name + ".bias"]
    e = torch.nn.functional.silu(lin("1.diffusion_embedding.projection1", table[3]))
    e = torch.nn.functional.silu(lin("1.diffusion_embedding.projection2", e))
    dp = [lin(r + "diffusion_projection", e) for r in L]
    w1 = lambda name: sd[name + ".weight"][:, :, 0]
    cw = torch.stack([w1(r + "conditioner_projection") for r in L])
    cb = torch.stack([sd[r + "conditioner_projection.bias"] for r in L])
    cp, _ = R.condproj_ref(cond.reshape(M, C), NL, cw, cb, 0)
    x104 = torch.zeros(M, R.LDX, dtype=R.F64)
    x104[:, :NMEL] = x.reshape(M, NMEL)
    h, _ = R.melpre_ref(x104, w1("1.mel_preprocess.projection"), sd["1.mel_preprocess.projection.bias"], dp[0], 0)
    gates = []
    for i, r in enumerate(L):
        y, _ = R.gate_ref(h, B, T, sd[r + "dilated_conv.weight"], sd[r + "dilated_conv.bias"], cp[i * M:(i + 1) * M],
                          2 ** i, None, 0)
        gates.append(y)
        if i + 1 < NL:
            ow, ob = w1(r + "output_projection")[:C], sd[r + "output_projection.bias"][:C]
            h, _ = R.res_ref(y, h, torch.zeros_like(h), ow, ob, dp[i], dp[i + 1], 0)
    sw = torch.stack([w1(r + "output_projection")[C:] for r in L])
    sb = torch.stack([sd[r + "output_projection.bias"][C:] for r in L])
    s, _ = R.skipsum_ref(torch.cat(gates), NL, M, 0, M, sw, sb, 0)
    eps, _ = R.head_ref(s, torch.zeros_like(s), w1("1.skip_projection"), sd["1.skip_projection.bias"],
                        w1("1.output_projection"), sd["1.output_projection.bias"], 0)
    err = float((eps.reshape(B, T, NMEL) - want).abs().max())
    print("references composed against the oracle: max |d| %.3e (eps up to %.2f)" % (err, float(want.abs().max())))
    assert err <= 1e-12 * float(want.abs().max())  # float64 on both sides (observed 4e-15)


# ------------------------------------------------------------------ planted defects
@pytest.mark.parametrize("name", sorted(R.GATE_SHAPES))
@pytest.mark.parametrize("mutant", ["cross_end", "past_tv", "zero_block", "zero_row"])
def test_gate_checks_catch(mutant, name):
    if mutant == "past_tv" and R.GATE_SHAPES[name][2] is None:
        assert _gate(mutant, name) <= 1.0  # no length table: nothing to read past
        return
    with pytest.raises(AssertionError, match="gate .*x the bound"):
        _gate(mutant, name)


@pytest.mark.parametrize("mutant", ["lo_dropped", "div_140", "dproj_same", "zero_block", "zero_row"])
def test_res_checks_catch(mutant):
    for M in R.RES_M:
        for bf in (0, 1):
            with pytest.raises(AssertionError, match="res M=%d .*x the bound" % M):
                R.check_res(Emu(mutant), M, 0, bf)


@pytest.mark.parametrize("mutant", ["zero_block", "zero_row"])
def test_melpre_checks_catch(mutant):
    for M in R.MELPRE_M:
        with pytest.raises(AssertionError, match="melpre .*x the bound"):
            R.check_melpre(Emu(mutant), M, 0)


@pytest.mark.parametrize("mutant", ["stride_rows", "zero_block", "zero_row"])
def test_skipsum_checks_catch(mutant):
    for rt, r0, rows in R.SKIPSUM_CASES:
        if mutant == "stride_rows" and rows == rt:
            assert R.check_skipsum(Emu(mutant), 20, rt, r0, rows, 0) <= 1.0  # the same computation
            continue
        with pytest.raises(AssertionError, match="skipsum .*x the bound"):
            R.check_skipsum(Emu(mutant), 20, rt, r0, rows, 0)


@pytest.mark.parametrize("mutant", ["u_lo_dropped", "zero_block", "zero_row"])
def test_head_checks_catch(mutant):
    for M in R.HEAD_M:
        for bf in (0, 1):
            with pytest.raises(AssertionError, match="head M=%d .*x the bound" % M):
                R.check_head(Emu(mutant), M, bf)


@pytest.mark.parametrize("mutant", ["cond_lo_dropped", "zero_block", "zero_row"])
def test_condproj_checks_catch(mutant):
    for M, NL in R.CONDPROJ_CASES:
        for bf in (0, 1):
            with pytest.raises(AssertionError, match="condproj M=%d .*x the bound" % M):
                R.check_condproj(Emu(mutant), M, NL, bf)
