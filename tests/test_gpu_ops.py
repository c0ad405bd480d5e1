"""GPU parity, op level: every HIP kernel family against a torch-CPU fp32 reference of the same op.

Tolerances: MFMA operands are fp16 (inputs and weights rounded to binary16, fp32 accumulation), so
GEMM-shaped ops are checked with a relative L2 error <= 2e-3 (fp16 unit roundoff 4.9e-4, a few
roundings per output); element-wise f32 ops with fp16 outputs <= 1e-3; frame counts and index maps
bit-exact.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import amp_ref as AR  # noqa: E402
from gpu_util import call, dev, ptr, rel_l2, stream  # noqa: E402
from oracle import models as OM  # noqa: E402


def _tm(x):  # [B, C, T] -> time-major [B*T, C]
    return x.permute(0, 2, 1).contiguous()


# (gemm_variant, gemm3_direct kernel switches): every conv_gemm3 tile and conv_gemm4 with conv_gemm3's register
# epilogues (15 = every form), and the LDS-staged epilogue (0) on the tiles pick3 chooses in production
_GEMM_MODES = ([(v, "15") for v in ("10", "11", "12", "13", "14", "15", "16", "20", "24")] +
               [(v, "0") for v in ("10", "13", "14", "16")])


@pytest.mark.parametrize("B,T,Cin,Cout,k,stride,dil,pad,act", [
    (2, 93, 384, 768, 3, 1, 1, 1, 0),        # DiffSVC dilated conv, d=1
    (2, 93, 384, 768, 3, 1, 8, 8, 0),        # d=8
    (1, 200, 100, 384, 1, 1, 1, 0, 2),       # mel_preprocess (Cin not a multiple of 8/64), relu
    (2, 60, 80, 128, 3, 1, 1, 1, 1),         # whisper conv1 (gelu)
    (2, 60, 128, 128, 3, 2, 1, 1, 1),        # whisper conv2 (stride 2)
    (1, 37, 100, 1536, 7, 1, 1, 3, 0),       # conv_pre
    (2, 301, 24, 24, 11, 1, 5, 25, 0),       # last BigVGAN stage
    (1, 130, 48, 48, 7, 1, 3, 9, 0),
    (1, 70, 96, 96, 3, 1, 1, 1, 0),
    (3, 17, 384, 100, 1, 1, 1, 0, 0),        # output projection (N=100)
    (3, 700, 384, 768, 3, 1, 2, 2, 0),       # several M tiles + M tail (gemm3 tile shapes)
    (2, 333, 256, 512, 3, 1, 4, 4, 2),
    (2, 300, 384, 384, 11, 1, 5, 25, 0),     # BigVGAN stage 2 k=11 d=5
    (1, 150, 768, 768, 7, 1, 3, 9, 0),       # BigVGAN stage 1 k=7 d=3
    (3, 129, 192, 192, 11, 1, 3, 15, 0),     # utterance boundaries inside tiles
    (1, 90, 128, 256, 7, 1, 7, 21, 0),       # |shift| 21, T < tile
])
@pytest.mark.parametrize("variant,direct", _GEMM_MODES)
def test_conv1d(B, T, Cin, Cout, k, stride, dil, pad, act, variant, direct, tune):
    # gemm_variant 10..14 / 16: conv_gemm3 tiles (16: 256 x 192 on 4 x 2 waves), 15: auto, 20/24: conv_gemm4;
    # gemm3_direct: conv_gemm3 register epilogues
    # (all forms) or the LDS-staged C tile
    tune(None, gemm_variant=variant, gemm3_direct=direct)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, k, generator=g) / np.sqrt(Cin * k)
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv1d(x, w, b, stride=stride, padding=pad, dilation=dil)
    ref = [ref, F.gelu(ref), F.relu(ref)][act]
    To = ref.shape[-1]
    y = torch.empty(B * To, Cout, device="cuda")
    xd, wd, bd = dev(_tm(x)), dev(w), dev(b)  # keep device tensors alive across the call
    call("svc_op_conv1d", ptr(xd), B, T, Cin, ptr(wd), ptr(bd), Cout, k, stride, dil, pad, act, ptr(y), stream())
    out = y.cpu().view(B, To, Cout).permute(0, 2, 1).numpy()
    assert rel_l2(out, ref.numpy()) < 2e-3


@pytest.mark.parametrize("B,T,Cin,Cout,k,s", [(2, 25, 768, 384, 8, 4), (1, 40, 96, 48, 4, 2), (2, 33, 48, 24, 4, 2),
                                              (1, 9, 1536, 768, 8, 4)])
@pytest.mark.parametrize("variant", ["10", "14", "15", "16", "20", "24"])
def test_conv_transpose1d(B, T, Cin, Cout, k, s, variant, tune):
    tune(None, gemm_variant=variant)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cin, Cout, k, generator=g) / np.sqrt(Cin * k / s)
    b = torch.randn(Cout, generator=g) * 0.1
    pad = (k - s) // 2
    ref = F.conv_transpose1d(x, w, b, stride=s, padding=pad)
    To = ref.shape[-1]
    assert To == T * s
    y = torch.empty(B * To, Cout, device="cuda")
    xd, wd, bd = dev(_tm(x)), dev(w), dev(b)
    call("svc_op_conv_transpose1d", ptr(xd), B, T, Cin, ptr(wd), ptr(bd), Cout, k, s, pad, ptr(y), stream())
    out = y.cpu().view(B, To, Cout).permute(0, 2, 1).numpy()
    assert rel_l2(out, ref.numpy()) < 2e-3


@pytest.mark.parametrize("x16", [False, True])
@pytest.mark.parametrize("B,L,C", [(2, 37, 24), (1, 1, 24), (1, 2, 48), (1, 3, 8), (2, 11, 12), (3, 129, 96),
                                   (1, 300, 768), (2, 64, 40), (2, 257, 48), (2, 700, 1536), (3, 1000, 192)])
def test_activation1d(B, L, C, x16):
    """f32 input (the generator's residual stream) and f16 input (an AMPBlock1 convs1 output): the reference runs on
    the same f16-rounded values. L = 700 / 1000 hold runs clear of both utterance ends (the clamp-free form)."""
    from svc_inference_pipeline_amd import weights as W
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, C, L, generator=g) * 2
    if x16:
        x = x.half().float()
    al = torch.randn(C, generator=g) * 0.3
    be = torch.randn(C, generator=g) * 0.3
    f = W.kaiser_sinc_filter1d(0.25, 0.3, 12).view(-1)
    ref = OM.activation1d(x, al, be, f)
    y = torch.empty(B * L, C, device="cuda")
    xd, ad, bd, fd = dev(_tm(x), torch.float16 if x16 else torch.float32), dev(al), dev(be), dev(f)
    call("svc_op_activation1d_x16" if x16 else "svc_op_activation1d", ptr(xd), B, L, C, ptr(ad), ptr(bd), ptr(fd),
         ptr(y), stream())
    out = y.cpu().view(B, L, C).permute(0, 2, 1).numpy()
    assert rel_l2(out, ref.numpy()) < 1e-3
    # fp16 output rounding bound, element-wise
    assert np.max(np.abs(out - ref.numpy()) / (np.abs(ref.numpy()) + 1e-2)) < 5e-3


@pytest.mark.parametrize("C", [24, 48, 96, 192])
@pytest.mark.parametrize("B,L,k,d", [(2, 37, 3, 1), (1, 1, 11, 5), (1, 5, 7, 3), (2, 130, 11, 5), (1, 300, 7, 3),
                                     (3, 257, 11, 1), (2, 600, 3, 5)])
def test_amp_conv(B, L, k, d, C):
    """Fused SnakeBeta Activation1d -> dilated conv -> bias + residual (BigVGAN C <= 192 stages; C <= 48 run the
    packed channel-pair activation; C = 96 on 256-row tiles of 2 x 2 waves, C = 192 of 2 x 4)."""
    from svc_inference_pipeline_amd import weights as W
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, L, generator=g) * 2
    al = torch.randn(C, generator=g) * 0.3
    be = torch.randn(C, generator=g) * 0.3
    f = W.kaiser_sinc_filter1d(0.25, 0.3, 12).view(-1)
    w = torch.randn(C, C, k, generator=g) / np.sqrt(C * k)
    b = torch.randn(C, generator=g) * 0.1
    res = torch.randn(B, C, L, generator=g)
    ref = F.conv1d(OM.activation1d(x, al, be, f), w, b, padding=(k - 1) // 2 * d, dilation=d) + res
    y = torch.empty(B * L, C, device="cuda")
    xd, ad, bd, fd, wd, bbd, rd = dev(_tm(x)), dev(al), dev(be), dev(f), dev(w), dev(b), dev(_tm(res))
    call("svc_op_amp_conv", ptr(xd), B, L, C, ptr(ad), ptr(bd), ptr(fd), ptr(wd), ptr(bbd), k, d, ptr(rd), ptr(y),
         stream())
    out = y.cpu().view(B, L, C).permute(0, 2, 1).numpy()
    assert rel_l2(out, ref.numpy()) < 2e-3


class _Gpu:
    """amp_ref backend: the library's op-level entry points (svc_op_amp_conv_ex, svc_op_conv_transpose1d_comb, the
    amp_conv calls svc_bigvgan makes)."""

    def amp_conv(self, x, x16, al, be, f, w, bias, k, d, tv, tv_mul, add_row, acc32, acc_div, out32, out16):
        B, L, C = x.shape
        xd = dev(x, torch.float16 if x16 else torch.float32)
        ad, bd, fd, wd, bbd = dev(al), dev(be), dev(f), dev(w), dev(bias)
        tvd = None if tv is None else dev(np.asarray(tv, np.int32), torch.int32)
        rd = None if add_row is None else dev(add_row)
        cd = None if acc32 is None else dev(acc32)
        o32 = cd if isinstance(out32, str) else (None if out32 is None else dev(out32))
        o16 = None if out16 is None else dev(out16, torch.float16)
        call("svc_op_amp_conv_ex", None if x16 else ptr(xd), ptr(xd) if x16 else None, B, L, C, ptr(ad), ptr(bd),
             ptr(fd), ptr(wd), ptr(bbd), k, d, ptr(tvd), tv_mul, ptr(rd), ptr(cd), float(acc_div), ptr(o32), ptr(o16),
             stream())
        return (None if o32 is None else o32.cpu().numpy()), (None if o16 is None else o16.cpu().numpy())

    def ups_comb(self, x, w, bias, k, s, tv, tv_mul, out):
        B, T, cin = x.shape
        xd, wd, bd, od = dev(x, torch.float16), dev(w), dev(bias), dev(out)
        tvd = None if tv is None else dev(np.asarray(tv, np.int32), torch.int32)
        call("svc_op_conv_transpose1d_comb", ptr(xd), B, T, cin, ptr(wd), ptr(bd), w.shape[1], k, s, ptr(tvd), tv_mul,
             ptr(od), stream())
        return od.cpu().numpy()

    def ups_phase(self, x, w, bias, k, s):
        B, T, cin = x.shape
        xd, wd, bd = dev(x), dev(w), dev(bias)
        y = torch.empty(B, T * s, w.shape[1], device="cuda")
        call("svc_op_conv_transpose1d", ptr(xd), B, T, cin, ptr(wd), ptr(bd), w.shape[1], k, s, (k - s) // 2, ptr(y),
             stream())
        return y.cpu().numpy()


class _Launched:
    """The amp_conv kernel forms launched inside the block, by profiler tag ("amp_conv<C>", "<C,x16>", "<C,conv>")."""

    def __enter__(self):
        from svc_inference_pipeline_amd import _lib
        _lib.profile_enable(True)
        self.tags = None
        return self

    def __exit__(self, *exc):
        from svc_inference_pipeline_amd import _lib
        try:
            if exc[0] is None:
                ran = _lib.profile_read()
                self.tags = {n.split("@")[0] for n, v in ran.items() if n.startswith("amp_conv") and v["launches"] > 0}
        finally:
            _lib.profile_enable(False)


_AMP_CASES = {C: {c[0]: c[1:] for c in AR.length_cases(C)} for C in (24, 48, 96, 192)}
_AMP_LEN_NAMES = ["Lm1", "L0", "Lp1", "L2p1", "ragged", "ragged_mul8", "L1", "L2", "L5", "L13"]


def _amp_case(C, name):
    BT = AR.tile_rows(C)
    key = {"Lm1": "L%d" % (BT - 1), "L0": "L%d" % BT, "Lp1": "L%d" % (BT + 1), "L2p1": "L%d" % (2 * BT + 1)}.get(name, name)
    return _AMP_CASES[C][key]


@pytest.mark.parametrize("length", _AMP_LEN_NAMES)
@pytest.mark.parametrize("x16", [False, True])
@pytest.mark.parametrize("C", [24, 48, 96, 192])
def test_amp_conv_tap_probes(C, x16, length):
    """The activation image amp_conv builds in LDS, element by element (amp_ref.check_tap_probes): one-tap identity
    weights make out32 the f16 image row each tap reads, halo rows and zero padding included. Lengths (BT = 512 rows for
    C <= 48, 256 otherwise): BT - 1, BT, BT + 1, 2 BT + 1; a ragged batch ending on, one past and far before a tile edge,
    and with a clamping frame multiplier; 1, 2, 5, 13 rows. (k, d) = (11, 5), (3, 1), (7, 5), first / centre / last tap;
    every utterance also bit-equal to itself run alone.
    Largest observed on MI355X: rel-L2 1.2e-5, element ratio |d| / (|ref| + 1e-2) 9.8e-4 (bounds 1e-3, 5e-3): the image
    differs from the f64 reference's f16 rounding by single f16 ulps only."""
    B, L, tv, mul = _amp_case(C, length)
    with _Launched() as ran:
        l2, el = AR.check_tap_probes(_Gpu(), C, x16, B, L, tv, mul, [(11, 5), (3, 1), (7, 5)])
    print("amp_conv tap probes C=%d x16=%d %s: rel-L2 %.3e element %.3e" % (C, x16, length, l2, el))
    assert ran.tags == {"amp_conv<%d%s>" % (C, ",x16" if x16 else "")}, ran.tags


@pytest.mark.parametrize("length", _AMP_LEN_NAMES)
@pytest.mark.parametrize("k,d", [(11, 5), (7, 3), (3, 1)])
@pytest.mark.parametrize("C", [24, 48, 96, 192])
def test_amp_conv_epilogues(C, k, d, length):
    """Conv + each epilogue svc_bigvgan uses (c1: out16 only; c2: add_row + out32; the resblock sum in place:
    + acc32 with out32 = acc32; the resblock mean: + acc_div = 3 to out16, and to out32 in place) against the f64 sum
    of the kernel's own A operands (its k tap probes) times the f16-rounded weights, every element within
    2 K 2^-24 S + 2^-23 |ref| (+ 2^-11 |ref| for f16), K = k C; rows past each utterance's end bit-untouched.
    f16 input at C = 24 / 96, f32 at 48 / 192.
    Largest observed err / bound on MI355X: f32 outputs 0.015 (C = 24), 0.0072 (48), 0.0036 (96), 0.0017 (192); f16
    outputs 0.95 / 0.88 / 0.80 / 0.64: an f16 output's bound is mostly its own half ulp, which a rounding reaches."""
    x16 = C in (24, 96)
    B, L, tv, mul = _amp_case(C, length)
    with _Launched() as ran:
        w32, w16 = AR.check_epilogues(_Gpu(), C, x16, B, L, tv, mul, k, d)
    print("amp_conv epilogues C=%d k=%d d=%d %s: err/bound f32 %.4f f16 %.4f" % (C, k, d, length, w32, w16))
    assert ran.tags == {"amp_conv<%d%s>" % (C, ",x16" if x16 else "")}, ran.tags


@pytest.mark.parametrize("C,x16", [(24, False), (96, True)])
def test_amp_conv_f16_saturation(C, x16):
    """A bias of 1e5 in two channels: out16 reads 65504 there (f16_sat), finite everywhere, on the ragged batch."""
    B, L, tv, mul = _amp_case(C, "ragged")
    AR.check_saturation(_Gpu(), C, x16, B, L, tv, mul, 3, 1)


_UPS_NAMES = ["T1", "T2", "T40", "Tm1", "T0", "Tp1", "ragged", "ragged_mul4"]


@pytest.mark.parametrize("length", _UPS_NAMES)
@pytest.mark.parametrize("cin", [48, 96, 192])
def test_conv_transpose1d_comb(cin, length):
    """The rate-2 ConvTranspose1d as svc_bigvgan's combined conv (pack_conv_transpose_comb + amp_conv's plain-conv form,
    k = 3, d = -1) against an f64 conv_transpose1d of the f16-rounded input and weights, every element within the
    accumulation bound (K = 2 cin); rows >= 2 Lb untouched; at cin 96 / 192 bit-identical to the phase GEMMs
    (svc_op_conv_transpose1d) on the same input, at cin 48 within the bound only (the 32-deep MFMA steps straddle taps).
    T = 1, 2, 40, BT - 1, BT, BT + 1 and ragged batches.
    Largest observed err / bound on MI355X: 0.0080 at cin 48, 0.0042 at 96, 0.0024 at 192."""
    BT = AR.tile_rows(cin)
    key = {"Tm1": "T%d" % (BT - 1), "T0": "T%d" % BT, "Tp1": "T%d" % (BT + 1)}.get(length, length)
    B, T, tv, mul = {c[0]: c[1:] for c in AR.ups_cases(cin)}[key]
    with _Launched() as ran:
        worst = AR.check_ups(_Gpu(), cin, B, T, tv, mul)
    print("conv_transpose1d_comb cin=%d %s: err/bound %.4f" % (cin, length, worst))
    assert ran.tags == {"amp_conv<%d,conv>" % cin}, ran.tags


@pytest.mark.parametrize("cin,cout,k,s", [(384, 192, 4, 2), (96, 24, 4, 2), (96, 48, 8, 4)])
def test_conv_transpose1d_comb_rejects(cin, cout, k, s):
    """Shapes without a combined form are an error (SVC_ERR_INVALID), not another path: nothing is launched or written."""
    from svc_inference_pipeline_amd import _lib
    T = 9
    xd, wd, bd = dev(np.ones((T, cin)), torch.float16), dev(np.ones((cin, cout, k))), dev(np.zeros(cout))
    y = torch.full((T * s, cout), float(AR.SENT32), device="cuda")
    with _Launched() as ran:
        with pytest.raises(_lib.SVCError, match="status 1:.*no combined form"):
            call("svc_op_conv_transpose1d_comb", ptr(xd), 1, T, cin, ptr(wd), ptr(bd), cout, k, s, None, 1, ptr(y),
                 stream())
    assert ran.tags == set()
    assert bool((y == float(AR.SENT32)).all())


def test_bigvgan_activation_launch_chunks():
    """Batches whose activation input spans more than 2 GiB: activation1d and amp_conv address x through 32-bit buffer
    descriptors, so the host splits the batch into launches of < 2^31 bytes (98 + 2 utterances here). Each utterance
    of the big batch must equal the same utterance run alone, bit for bit, on both sides of the split."""
    from svc_inference_pipeline_amd import weights as W
    B, L, C, k, d = 100, 224000, 24, 3, 1
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(B * L, C, device="cuda", generator=g) * 2
    al = torch.randn(C, device="cuda", generator=g) * 0.3
    be = torch.randn(C, device="cuda", generator=g) * 0.3
    f = W.kaiser_sinc_filter1d(0.25, 0.3, 12).view(-1).cuda()
    w = torch.randn(C, C, k, device="cuda", generator=g) / np.sqrt(C * k)
    b = torch.randn(C, device="cuda", generator=g) * 0.1
    y = torch.empty(B * L, C, device="cuda")
    y1 = torch.empty(L, C, device="cuda")
    for op in ("act", "amp"):
        if op == "act":
            call("svc_op_activation1d", ptr(x), B, L, C, ptr(al), ptr(be), ptr(f), ptr(y), stream())
        else:
            call("svc_op_amp_conv", ptr(x), B, L, C, ptr(al), ptr(be), ptr(f), ptr(w), ptr(b), k, d, None, ptr(y),
                 stream())
        for u in (0, 97, 98, 99):
            xu = x[u * L:(u + 1) * L]
            if op == "act":
                call("svc_op_activation1d", ptr(xu), 1, L, C, ptr(al), ptr(be), ptr(f), ptr(y1), stream())
            else:
                call("svc_op_amp_conv", ptr(xu), 1, L, C, ptr(al), ptr(be), ptr(f), ptr(w), ptr(b), k, d, None,
                     ptr(y1), stream())
            torch.cuda.synchronize()
            assert torch.equal(y[u * L:(u + 1) * L], y1), (op, u)


@pytest.mark.parametrize("B,L,D", [(1, 1500, 1024), (2, 100, 128), (1, 64, 64), (2, 1, 64), (1, 129, 256)])
def test_attention(B, L, D):
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, L, D, generator=g) for _ in range(3))
    H = D // 64
    sc = 64 ** -0.25
    qh = q.view(B, L, H, 64).permute(0, 2, 1, 3) * sc
    kh = k.view(B, L, H, 64).permute(0, 2, 3, 1) * sc
    vh = v.view(B, L, H, 64).permute(0, 2, 1, 3)
    ref = (F.softmax(qh @ kh, dim=-1) @ vh).permute(0, 2, 1, 3).reshape(B, L, D)
    out = torch.empty(B * L, D, device="cuda")
    qd, kd, vd = dev(q.reshape(B * L, D)), dev(k.reshape(B * L, D)), dev(v.reshape(B * L, D))
    call("svc_op_attention", ptr(qd), ptr(kd), ptr(vd), B, L, D, ptr(out), stream())
    assert rel_l2(out.cpu().view(B, L, D).numpy(), ref.numpy()) < 3e-3


@pytest.mark.parametrize("mode", ["ramp", "outlier"])
def test_attention_rescale(mode):
    """The deferred online-softmax rescale (attention.hip: the running max moves only when a tile's P column sum exceeds
    ATT_PSUM) on inputs that make it fire: key norms ramping up along the sequence (the max grows on many tiles), and
    one outlier key per head far past the first tile (P of a column jumps from <= 1 to ~2^40 in one tile). Against the
    fp32 torch reference at the Whisper-medium head layout (L = 1500, 4 heads)."""
    B, L, D = 2, 1500, 256
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(B, L, D, generator=g) for _ in range(3))
    if mode == "ramp":
        k = k * torch.linspace(0.5, 4.0, L)[None, :, None]
    else:
        k[:, 1100] *= 12.0
        q = q + 0.5 * k[:, 1100:1101]
    H = D // 64
    sc = 64 ** -0.25
    qh = q.view(B, L, H, 64).permute(0, 2, 1, 3) * sc
    kh = k.view(B, L, H, 64).permute(0, 2, 3, 1) * sc
    vh = v.view(B, L, H, 64).permute(0, 2, 1, 3)
    ref = (F.softmax(qh @ kh, dim=-1) @ vh).permute(0, 2, 1, 3).reshape(B, L, D)
    out = torch.empty(B * L, D, device="cuda")
    qd, kd, vd = dev(q.reshape(B * L, D)), dev(k.reshape(B * L, D)), dev(v.reshape(B * L, D))
    call("svc_op_attention", ptr(qd), ptr(kd), ptr(vd), B, L, D, ptr(out), stream())
    o = out.cpu().view(B, L, D).numpy()
    assert np.isfinite(o).all()
    assert rel_l2(o, ref.numpy()) < 3e-3


def test_layernorm():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(300, 1024, generator=g) * 3 + 1
    gm = torch.randn(1024, generator=g)
    bt = torch.randn(1024, generator=g)
    ref = F.layer_norm(x, (1024,), gm, bt)
    y = torch.empty(300, 1024, device="cuda")
    xd, gd, bd = dev(x), dev(gm), dev(bt)
    call("svc_op_layernorm", ptr(xd), ptr(gd), ptr(bd), 300, 1024, ptr(y), stream())
    np.testing.assert_allclose(y.cpu().numpy(), ref.numpy(), rtol=0, atol=2e-5)


def _layernorm_f64(x, g, b):
    x = x.astype(np.float64)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * g.astype(np.float64) + b.astype(np.float64), np.sqrt(var)


def _layernorm_run(x, g, b):
    """svc_op_layernorm into a buffer with 4 guard rows of SENT32 after `rows` -> (y [rows, D], guard rows intact)."""
    rows, D = x.shape
    y = torch.full((rows + 4, D), float(AR.SENT32), device="cuda")
    xd, gd, bd = dev(x), dev(g), dev(b)
    call("svc_op_layernorm", ptr(xd), ptr(gd), ptr(bd), rows, D, ptr(y), stream())
    return y[:rows].cpu().numpy(), bool((y[rows:] == float(AR.SENT32)).all())


@pytest.mark.parametrize("rows", [1, 3, 5, 301])
@pytest.mark.parametrize("D", [64, 256, 384, 768, 1024])
def test_layernorm_forms(D, rows):
    """Both LayerNorm kernels against float64: layernorm_kernel (D = 64, Whisper-tiny's 384) and layernorm_v4_kernel
    with nq = 1, 3 (HuBERT's 768) and 4; one row, row counts that leave the last 4-row block partial, and many blocks.
    N(1, 3^2) data at the project's atol = 2e-5; the rows after `rows` are not written.
    Largest |y - ref| observed on MI355X: 1.4e-6 (D = 768, 301 rows)."""
    rng = np.random.default_rng([D, rows])
    x = (rng.standard_normal((rows, D)) * 3 + 1).astype(np.float32)
    g, b = rng.standard_normal(D).astype(np.float32), rng.standard_normal(D).astype(np.float32)
    y, guards = _layernorm_run(x, g, b)
    ref, _ = _layernorm_f64(x, g, b)
    print("layernorm D=%d rows=%d: max |d| %.3e" % (D, rows, np.max(np.abs(y - ref))))
    np.testing.assert_allclose(y, ref, rtol=0, atol=2e-5)
    assert guards


@pytest.mark.parametrize("D", [384, 768])
def test_layernorm_offset_rows(D):
    """Rows with a mean far from zero (mean 50, sigma 0.5), one case per kernel form: x - mean cancels two decimal
    digits, so each output carries the rounding of that difference, <= 4 u max|x| / sigma_row |gamma| (u = 2^-24: the
    rounding of the f32 mean and of the difference, in units of the row's sigma), on top of the project's 2e-5.
    Largest err / bound observed on MI355X: 0.28 (D = 384), 0.20 (D = 768)."""
    rows = 5
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((rows, D)) * 0.5 + 50).astype(np.float32)
    g, b = rng.standard_normal(D).astype(np.float32), rng.standard_normal(D).astype(np.float32)
    y, guards = _layernorm_run(x, g, b)
    ref, sig = _layernorm_f64(x, g, b)
    bound = 2e-5 + 4 * 2.0 ** -24 * np.abs(x).max(axis=1, keepdims=True) / sig * np.abs(g)[None, :]
    print("layernorm offset D=%d: max err/bound %.3f" % (D, np.max(np.abs(y - ref) / bound)))
    assert np.all(np.abs(y - ref) <= bound)
    assert guards


@pytest.mark.parametrize("D", [1088, 96])
def test_layernorm_rejects(D):
    """A width the kernels have no form for (> 1024, or no multiple of 64) is SVC_ERR_INVALID; nothing is written."""
    from svc_inference_pipeline_amd import _lib
    x, g, b = np.ones((3, D), np.float32), np.ones(D, np.float32), np.zeros(D, np.float32)
    y = torch.full((3, D), float(AR.SENT32), device="cuda")
    xd, gd, bd = dev(x), dev(g), dev(b)
    with pytest.raises(_lib.SVCError, match="status 1:.*layernorm: D=%d" % D):
        call("svc_op_layernorm", ptr(xd), ptr(gd), ptr(bd), 3, D, ptr(y), stream())
    assert bool((y == float(AR.SENT32)).all())
