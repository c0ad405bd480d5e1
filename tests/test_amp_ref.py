"""The amp_conv parity checks (tests/amp_ref.py, run on the GPU by tests/test_gpu_ops.py) on a torch-CPU emulation of
the kernel's arithmetic: activation in f32 -> round to f16 -> fp32 conv -> epilogue. A correct fp32 implementation
meets every bound, and each deliberate defect of the kind those checks exist for fails at least one assertion."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import amp_ref as R
from oracle import models as OM


class Emu:
    """amp_ref backend: the kernel's arithmetic on the CPU, tile by tile (each tile builds its own image of
    BT + 2 P rows, as a workgroup does). `mutant` plants one defect."""

    def __init__(self, mutant=None):
        self.mutant = mutant

    def _image(self, x, Lb, L, al, be, f):
        """f16 activation image of one utterance, rows [0, L): zeros past Lb."""
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
        n = L if self.mutant in ("pad_at_L", "read_past_Lb") else Lb
        y = OM.activation1d(t(x[:n].T[None]), t(al), t(be), t(f))[0].T  # [n, C]
        img = torch.zeros(L, x.shape[1])
        if self.mutant == "read_past_Lb":
            y[:Lb] = OM.activation1d(t(x[:Lb].T[None]), t(al), t(be), t(f))[0].T
            img[:n] = y
        else:
            img[:Lb] = y[:Lb]
        return img.clamp(-R.F16_MAX, R.F16_MAX).half().float()

    def amp_conv(self, x, x16, al, be, f, w, bias, k, d, tv, tv_mul, add_row, acc32, acc_div, out32, out16):
        B, L, C = x.shape
        BT, P = R.tile_rows(C), (k - 1) // 2 * d
        Lbs = R.row_counts(B, L, tv, tv_mul)
        if isinstance(out32, str):
            out32 = acc32
        w16 = torch.from_numpy(np.asarray(w, np.float32)).half().float()
        bt = torch.from_numpy(np.asarray(bias, np.float32))
        for b, Lb in enumerate(Lbs):
            img = F.pad(self._image(x[b], Lb, L, al, be, f), (0, 0, P, P + BT))  # row r of img = utterance row r - P
            for t0 in range(0, Lb, BT):
                nv = min(BT, Lb - t0)
                tile = img[t0:t0 + BT + 2 * P].clone()  # image rows t0 - P .. t0 + BT + P
                if self.mutant == "drop_halo":
                    tile[-1] = 0.0
                v = torch.zeros(nv, C)
                for j in range(k):
                    off = j * d + (1 if self.mutant == "dil_off" and j == 0 else 0)
                    v += tile[off:off + nv] @ w16[:, :, j].T
                v = v + bt
                rows = slice(t0, t0 + nv)
                if add_row is not None:
                    v = v + torch.from_numpy(add_row[b, rows])
                if acc32 is not None:
                    a = torch.from_numpy(acc32[b, rows])
                    if self.mutant == "div_before_acc":
                        v = a + v / np.float32(acc_div)
                    else:
                        v = (a + v) / np.float32(acc_div) if acc_div != 1.0 else a + v
                if out32 is not None:
                    out32[b, rows] = v.numpy()
                if out16 is not None:
                    out16[b, rows] = v.clamp(-R.F16_MAX, R.F16_MAX).half().numpy()
        return out32, out16

    def ups_comb(self, x, w, bias, k, s, tv, tv_mul, out):
        B, T, cin = x.shape
        w16 = torch.from_numpy(np.asarray(w, np.float32)).half().float()
        for b, Lb in enumerate(R.row_counts(B, T, tv, tv_mul)):
            xb = torch.from_numpy(x[b, :Lb].T[None].copy())
            y = F.conv_transpose1d(xb, w16, torch.from_numpy(bias), stride=s, padding=(k - s) // 2)[0].T.numpy()
            if self.mutant == "phase_swap":
                y = y.reshape(Lb, s, -1)[:, ::-1].reshape(s * Lb, -1)
            out[b, :s * Lb] = y
        return out

    def ups_phase(self, x, w, bias, k, s):
        return None


def _ragged(C):
    return [c for c in R.length_cases(C) if c[0] == "ragged"][0][1:]


KDS_A = [(11, 5), (3, 1), (7, 5)]


@pytest.mark.parametrize("C,x16", [(24, False), (96, True)])
def test_emulation_passes_tap_probes(C, x16):
    B, L, tv, mul = _ragged(C)
    l2, el = R.check_tap_probes(Emu(), C, x16, B, L, tv, mul, KDS_A)
    assert 0 < l2 < 1e-3 and 0 < el < 5e-3


@pytest.mark.parametrize("C,x16", [(24, True), (96, False)])
def test_emulation_passes_epilogues(C, x16):
    B, L, tv, mul = _ragged(C)
    for k, d in [(11, 5), (7, 3), (3, 1)]:
        assert max(R.check_epilogues(Emu(), C, x16, B, L, tv, mul, k, d)) <= 1.0
    R.check_saturation(Emu(), C, x16, B, L, tv, mul, 3, 1)


@pytest.mark.parametrize("cin", [48, 96])
def test_emulation_passes_ups(cin):
    for name, B, T, tv, mul in R.ups_cases(cin):
        if name.startswith("ragged"):
            assert R.check_ups(Emu(), cin, B, T, tv, mul) <= 1.0


def test_short_and_clamped_lengths_on_emulation():
    """The shortest lengths and the clamping frame multiplier run through the reference helpers too."""
    for name, B, L, tv, mul in R.length_cases(24):
        if name in ("L1", "L2", "L5", "L13", "ragged_mul8"):
            R.check_tap_probes(Emu(), 24, False, B, L, tv, mul, [(11, 5)], alone=False)
            R.check_epilogues(Emu(), 24, False, B, L, tv, mul, 3, 1)
    assert R.row_counts(4, 1064, [136, 64, 65, 1], 8) == [1064, 512, 520, 8]


@pytest.mark.parametrize("mutant", ["drop_halo", "pad_at_L", "read_past_Lb", "dil_off"])
def test_tap_probes_catch(mutant):
    """The trailing halo row of each tile dropped; replicate padding taken at L instead of Lb; rows past Lb read
    instead of zeroed; one tap's dilation off by one."""
    B, L, tv, mul = _ragged(24)
    with pytest.raises(AssertionError):
        R.check_tap_probes(Emu(mutant), 24, False, B, L, tv, mul, KDS_A, alone=False)


def test_epilogues_catch_div_before_acc():
    B, L, tv, mul = _ragged(24)
    with pytest.raises(AssertionError, match="mean"):
        R.check_epilogues(Emu("div_before_acc"), 24, False, B, L, tv, mul, 3, 1)


def test_ups_catches_phase_swap():
    with pytest.raises(AssertionError):
        R.check_ups(Emu("phase_swap"), 48, 3, 60, [60, 33, 1], 1)


def test_untouched_and_bound_helpers():
    init = np.full((1, 4, 2), R.SENT32, np.float32)
    out = init.copy()
    out[0, 3, 1] = 0.0
    with pytest.raises(AssertionError):
        R.assert_untouched(out, init, [2], "x")
    R.assert_untouched(out, init, [4], "x")
    # one product per output: the bound is 2 * 2^-24 * S + 2^-23 |ref|, and an f16 output adds half an ulp
    ref, S = R.conv_ref64([np.array([[2.0]])], np.array([[[0.5]]]), np.array([0.25]))
    assert ref[0, 0] == 1.25 and S[0, 0] == 1.25
    _, b32 = R.acc_bound(ref, S, 1)
    _, b16 = R.acc_bound(ref, S, 1, out16=True)
    assert b32[0, 0] == 1.25 * (2.0 ** -23 + 2.0 ** -23) and b16[0, 0] == b32[0, 0] + 1.25 * 2.0 ** -11
    assert R.acc_bound(np.array([1e5]), np.array([1e5]), 1, out16=True)[0][0] == R.F16_MAX
