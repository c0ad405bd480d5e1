"""GPU parity, op level: the DiffSVC denoiser's six steps (svc_op_diffsvc_*, which run the launcher choices of
stage_diffsvc.hip's denoise / project_cond) element by element against the float64 references and derived bounds of
tests/denoiser_ref.py, in binary16 and bfloat16, in every kernel form, at the smallest shapes that reach each kernel's
edges. tests/test_denoiser_ref.py proves on the CPU that each of these checks fails for the defects it exists for.

Every output lies between sentinel guard rows that must keep their bits; the gate's input lies between poison rows and
holds poison past each utterance's end. The profiler tag asserts which kernel ran. Each test prints its largest
err / bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import denoiser_ref as R  # noqa: E402
from gpu_util import call, ptr, stream  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402


class _Gpu:
    device = "cuda"

    def gate(self, x, B, T, w, bias, cp16, dil, tv, bf, y16):
        call("svc_op_diffsvc_gate", ptr(x.t), B, T, ptr(w), ptr(bias), ptr(cp16), dil, ptr(tv), bf, ptr(y16), stream())

    def res(self, g16, w, bias, sub, add, store_lo, lanes_cap, bf, hi, lo):
        call("svc_op_diffsvc_res", ptr(g16), g16.shape[0], ptr(w), ptr(bias), ptr(sub), ptr(add), store_lo, lanes_cap,
             bf, ptr(hi), ptr(lo), stream())

    def melpre(self, x16, w, bias, add, bf, hi, lo):
        call("svc_op_diffsvc_melpre", ptr(x16), x16.shape[0], ptr(w), ptr(bias), ptr(add), bf, ptr(hi), ptr(lo),
             stream())

    def skipsum(self, g16, NL, rows_total, row0, rows, w, bias, bf, s16):
        call("svc_op_diffsvc_skipsum", ptr(g16), NL, rows_total, row0, rows, ptr(w), ptr(bias), bf, ptr(s16), stream())

    def head(self, s16, wsp, bsp, wout, bout, bf, eps):
        call("svc_op_diffsvc_head", ptr(s16), s16.shape[0], ptr(wsp), ptr(bsp), ptr(wout), ptr(bout), bf, ptr(eps),
             stream())

    def condproj(self, cond, NL, w, bias, bf, cp16):
        call("svc_op_diffsvc_condproj", ptr(cond), cond.shape[0], NL, ptr(w), ptr(bias), bf, ptr(cp16), stream())


class _Launched:
    """The kernels launched inside the block, by profiler tag (the part before "@site")."""

    def __enter__(self):
        _lib.profile_enable(True)
        self.tags = None
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.tags = {n.split("@")[0] for n, v in _lib.profile_read().items() if v["launches"] > 0}
        finally:
            _lib.profile_enable(False)


FMT = pytest.mark.parametrize("bf", [0, 1], ids=["f16", "bf16"])
GATE_FORMS = {"gate_ws": dict(gate_ws=1, gemm_variant=15), "gemm20": dict(gemm_variant=20),
              "gemm24": dict(gemm_variant=24)}
GATE_TAGS = {"gate_ws": "gate_ws<16x128>", "gemm20": "conv_gemm4<128,128,pair>", "gemm24": "conv_gemm4<128,128,gate>"}


@FMT
@pytest.mark.parametrize("name", list(R.GATE_SHAPES))
def test_gate(name, bf, tune):
    """Dilated conv + conditioner projection + gate: gate_ws, conv_gemm4 with the LDS-staged (gemm_variant 20) and the
    register (24) gate epilogue, each at dilations 1, 2, 4 and 8, every output row (rows past an utterance's end
    included: all forms write the masked-input result) within 0.25 dg + df + gate_allow + the 16-bit output rounding
    of the f64 reference (denoiser_ref.gate_ref). The shapes gate_ws declines (B > 1024, T < 16) must run conv_gemm4's
    register-epilogue kernel. One reference per dilation, shared by the forms.
    Largest observed err / bound on MI355X: dense batches 0.09 - 0.10 (binary16) and 0.43 - 0.46 (bfloat16): there the
    K = 1152 accumulation term outweighs the output's half ulp; T < 16 (conv_gemm4) 0.28 / 0.74; the batches with a
    length table 0.987 - 0.997 in both formats: rows far past an utterance's end have no non-zero product, so their
    bound is the 16-bit output's own half ulp (+ gate_allow), which a rounding among 10^5 such elements reaches."""
    B, T, tv = R.GATE_SHAPES[name]
    refs, worst = {}, 0.0
    for form, switches in GATE_FORMS.items():
        tune(None, reset=1)
        tune(None, **switches)
        for dil in (1, 2, 4, 8):
            with _Launched() as ran:
                w, _ = R.check_gate(_Gpu(), B, T, tv, dil, bf, ref_cache=refs)
            want = GATE_TAGS["gemm24" if form == "gate_ws" and name in R.GATE_WS_DECLINES else form]
            assert ran.tags == {want}, (form, dil, ran.tags)
            worst = max(worst, w)
    print("gate %s %s: largest err / bound %.4f" % (name, "bf16" if bf else "f16", worst))


@FMT
@pytest.mark.parametrize("M", R.RES_M)
def test_res(M, bf):
    """The residual update in place, res_proj at lanes_cap 0 (the first form), -2, 1, 8, 24 (the loader-wave form) and
    the tiled GEMM (-1), both store_lo values: hi + lo within the derived bound (+ the split term) of the f64
    reference, hi a nearest 16-bit value of hi + lo, store_lo = 0 leaves lo bit-untouched (res_proj) and hi bit-equal;
    all forms bit-equal to one another.
    Largest observed err / bound on MI355X: 0.005 (M = 1) to 0.58 (M = 385) binary16, 0.10 to 0.49 bfloat16. The largest
    ratios are in the probe rows (two non-zero products): their bound is mostly the split store's own rounding
    u16^2 |v|, which lo's rounding reaches; the CPU emulation gives the same 0.58."""
    outs, worst = [], 0.0
    for lanes in R.RES_LANES:
        with _Launched() as ran:
            w, hi, lo = R.check_res(_Gpu(), M, lanes, bf)
        if lanes == -1:
            assert len(ran.tags) == 1 and next(iter(ran.tags)).startswith("conv_gemm3<"), ran.tags
        else:
            assert ran.tags == {"res_proj<16x192>"}, ran.tags
        outs.append((hi, lo))
        worst = max(worst, w)
    for hi, lo in outs[1:]:
        assert torch.equal(R.bits(hi), R.bits(outs[0][0])) and torch.equal(R.bits(lo), R.bits(outs[0][1])), \
            "res M=%d: the forms differ" % M
    print("res M=%d %s: largest err / bound %.4f" % (M, "bf16" if bf else "f16", worst))


@FMT
@pytest.mark.parametrize("M", R.MELPRE_M)
def test_melpre(M, bf, tune):
    """The input projection + ReLU + layer-0 diffusion projection into the split stream: mel_proj and the tiled GEMM
    (tune.res_proj = 0) against the f64 reference, bit-equal to each other.
    Largest observed err / bound on MI355X: 0.005 (M = 1) to 0.55 (M = 300) binary16, 0.12 to 0.49 bfloat16; as for the
    residual, the probe rows' bound is mostly the split store's own rounding."""
    outs, worst = [], 0.0
    for rp in (1, 0):
        tune(None, res_proj=rp)
        with _Launched() as ran:
            w, hi, lo = R.check_melpre(_Gpu(), M, bf)
        if rp:
            assert ran.tags == {"mel_proj<16x384>"}, ran.tags
        else:
            assert len(ran.tags) == 1 and next(iter(ran.tags)).startswith("conv_gemm3<"), ran.tags
        outs.append((hi, lo))
        worst = max(worst, w)
    assert torch.equal(R.bits(outs[0][0]), R.bits(outs[1][0])) and torch.equal(R.bits(outs[0][1]), R.bits(outs[1][1]))
    print("melpre M=%d %s: largest err / bound %.4f" % (M, "bf16" if bf else "f16", worst))


@FMT
@pytest.mark.parametrize("rows_total,row0,rows", R.SKIPSUM_CASES)
def test_skipsum(rows_total, row0, rows, bf):
    """The skip sum over 20 layer-major gate blocks as one K = 7680 GEMM, a whole batch and two sub-batches whose layer
    stride (rows_total) differs from their row count: [hi | lo | hi] against the f64 reference (every third row of g is
    a one-channel probe row with a bound near u S).
    Largest observed err / bound on MI355X: 0.18 - 0.20 binary16, 0.39 bfloat16 (in the probe rows, whose bound is
    mostly the split store's own rounding; the dense rows stay below 0.001 of their K = 7680 bound)."""
    w = R.check_skipsum(_Gpu(), 20, rows_total, row0, rows, bf)
    print("skipsum %d+%d of %d %s: largest err / bound %.4f" % (row0, rows, rows_total, "bf16" if bf else "f16", w))


@FMT
@pytest.mark.parametrize("M", R.HEAD_M)
def test_head(M, bf, tune):
    """relu(skip_projection) + output_projection on split operands, fused (diff_head) and as two GEMMs, against the f64
    reference under the split operands' bound: the probe columns (denoiser_ref.HEAD_PROBE_EPS) hold eps to ~1e-6
    relative, which a head that keeps one 16-bit half of u cannot meet. M to 1025 and 11 * 128 + 5: 9 and 12 tiles.
    Largest observed err / bound on MI355X: 0.04 (M = 1) to 0.14 (M = 1413) binary16, 0.05 to 0.33 bfloat16 (an f32
    output)."""
    worst = 0.0
    for fused in (1, 0):
        tune(None, diff_head=fused)
        with _Launched() as ran:
            w, _ = R.check_head(_Gpu(), M, bf)
        if fused:
            assert ran.tags == {"diff_head<128>"}, ran.tags
        else:
            assert ran.tags and all(t.startswith("conv_gemm3<") for t in ran.tags), ran.tags
        worst = max(worst, w)
    print("head M=%d %s: largest err / bound %.4f" % (M, "bf16" if bf else "f16", worst))


@FMT
@pytest.mark.parametrize("M,NL", R.CONDPROJ_CASES)
def test_condproj(M, NL, bf):
    """The conditioner projections of all layers as one split-operand GEMM, layer-major, given back in reference
    channel order: against the f64 reference; the probe channels (denoiser_ref.COND_PROBE_O) cancel to 1e-3 of their
    terms, so a projection that drops the conditioner's (or the weight's) low half lands far outside.
    Largest observed err / bound on MI355X: 0.35 - 0.54 binary16, 0.73 - 0.88 bfloat16: a 16-bit output, whose bound
    is mostly its own half ulp."""
    w = R.check_condproj(_Gpu(), M, NL, bf)
    print("condproj M=%d NL=%d %s: largest err / bound %.4f" % (M, NL, "bf16" if bf else "f16", w))


def test_bad_arguments_launch_nothing():
    """One bad argument per op: SVC_ERR_INVALID, no kernel launched, the output untouched."""
    d = "cuda"
    h = lambda *s: torch.zeros(*s, dtype=torch.float16, device=d)
    f = lambda *s: torch.zeros(*s, device=d)
    out16 = R.Guarded(16, 3 * R.C, torch.float16, d, R.SENT16)
    out32 = R.Guarded(16, R.NMEL, torch.float32, d, R.SENT32)
    o, s = ptr(out16.t), stream()
    cases = [
        ("svc_op_diffsvc_gate", (ptr(h(16, 384)), 1, 16, ptr(f(768, 384, 3)), ptr(f(768)), ptr(h(16, 768)), 3, None, 0, o, s)),
        ("svc_op_diffsvc_res", (ptr(h(16, 384)), 16, ptr(f(384, 384)), ptr(f(384)), ptr(f(384)), ptr(f(384)), 1, -3, 0, o, o, s)),
        ("svc_op_diffsvc_melpre", (ptr(h(16, 104)), 0, ptr(f(384, 100)), ptr(f(384)), ptr(f(384)), 0, o, o, s)),
        ("svc_op_diffsvc_skipsum", (ptr(h(32, 384)), 2, 16, 8, 9, ptr(f(2, 384, 384)), ptr(f(2, 384)), 0, o, s)),
        ("svc_op_diffsvc_head", (ptr(h(16, 1152)), 16, ptr(f(384, 384)), ptr(f(384)), None, ptr(f(100)), 0, ptr(out32.t), s)),
        ("svc_op_diffsvc_condproj", (ptr(f(16, 384)), 16, 0, ptr(f(1, 768, 384)), ptr(f(1, 768)), 0, o, s)),
    ]
    for name, args in cases:
        with _Launched() as ran:
            with pytest.raises(_lib.SVCError, match="status 1"):
                _lib.call(name, *args)
            torch.cuda.synchronize()
        assert ran.tags == set(), (name, ran.tags)
        out16.assert_untouched(name)
        out32.assert_untouched(name)
