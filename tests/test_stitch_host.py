"""CPU: audio.stitch, the host definition of the long-form join (DESIGN.md "Long-form conversion"; svc_stitch reproduces
it on the device, tests/test_gpu_stitch.py), and the C-ABI declaration of svc_stitch."""
import ctypes
import os
import re

import numpy as np
import pytest

from stitch_util import chain_case, known_shift_case, random_songs_case
from svc_inference_pipeline_amd import _lib
from svc_inference_pipeline_amd import audio as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_known_shifts_give_the_signal_back():
    """Chunks cut from one signal, rows offset by delta = (0, +5, -7), X = 64, R = 8: the displacements are delta and
    the output is the signal, bit for bit."""
    x, rows, plan = known_shift_case()
    out, shifts, q = A.stitch(rows, plan, return_shifts=True, return_q=True)
    assert shifts.dtype == np.int32 and shifts.tolist() == [0, 5, -7]
    assert out.dtype == np.float32 and np.array_equal(out, x[:plan.out_len])
    assert q.shape == (3, 16) and not q[0].any()
    for b, d in ((1, 5), (2, -7)):  # the aligned candidate stands far above the rest
        rest = np.delete(q[b], d + 8)
        assert q[b, d + 8] > 10 * np.abs(rest).max()


def test_the_chain_matters():
    """The same rows stitched with d_{b-1} ignored in the predecessor's continuation: chunk 2 is then aligned to a
    continuation that was never played, and the result differs."""
    x, rows, plan = known_shift_case()
    out = A.stitch(rows, plan)
    flat, flat_shifts = A.stitch(rows, plan, return_shifts=True, chain=False)
    assert flat_shifts.tolist()[:2] == [0, 5]  # chunk 1's predecessor is not displaced: nothing changes for it
    assert flat_shifts[2] != -7 or not np.array_equal(flat, out)
    assert not np.array_equal(flat, out)
    assert np.array_equal(flat[:plan.out_off[2]], out[:plan.out_off[2]])  # only chunk 2 is affected


def test_silence():
    """Silent rows: every q is 0, the tie rule picks d = 0, and the output is exact zeros. A silent chunk after a loud
    one, and a loud one after a silent one, likewise pick 0 (nom = 0 for every candidate)."""
    _, rows, plan = known_shift_case()
    zeros = [np.zeros_like(r) for r in rows]
    out, shifts, q = A.stitch(zeros, plan, return_shifts=True, return_q=True)
    assert shifts.tolist() == [0, 0, 0] and not out.any() and not q.any()
    mixed = [rows[0], zeros[1], rows[2]]
    out, shifts = A.stitch(mixed, plan, return_shifts=True)
    assert shifts.tolist() == [0, 0, 0]
    assert np.array_equal(out[:plan.body[0]], rows[0][:plan.body[0]])
    assert not out[plan.out_off[1] + plan.xfade:plan.out_off[2]].any()


def test_search_zero_is_a_linear_crossfade():
    rows, plan = random_songs_case(11, 64, 0)
    out, shifts, q = A.stitch(rows, plan, return_shifts=True, return_q=True)
    assert not shifts.any() and q.shape == (len(rows), 1)
    X = 64
    w = (np.arange(X) + 0.5) / X
    for b in range(len(rows)):
        lead, body, off = plan.lead[b], plan.body[b], plan.out_off[b]
        c = rows[b][lead:lead + body]
        if plan.joined[b]:
            pa = plan.lead[b - 1] + plan.body[b - 1]
            a = rows[b - 1][pa:pa + X].astype(np.float64)
            want = (a + w * (c[:X].astype(np.float64) - a)).astype(np.float32)
            assert np.array_equal(out[off:off + X], want)
            assert np.array_equal(out[off + X:off + body], c[X:])
        else:
            assert np.array_equal(out[off:off + body], c)
    # nothing but the bodies is written
    mask = np.zeros(plan.out_len, bool)
    for b in range(len(rows)):
        mask[plan.out_off[b]:plan.out_off[b] + plan.body[b]] = True
    assert not out[~mask].any() and (~mask).sum() > 0


@pytest.mark.parametrize("X,R", [(64, 8), (63, 1), (16, 4)])
def test_q_and_the_order_from_first_principles(X, R):
    """q(d) against math.fsum-free straight loops in Python floats (IEEE f64, j ascending), and the winner against a
    sort by (-q, |d|, -d)."""
    rows, plan = (chain_case(seams=6, X=X, R=R) if X == 16 else random_songs_case(5, X, R))
    out, shifts, q = A.stitch(rows, plan, return_shifts=True, return_q=True)
    for b in range(len(rows)):
        if not plan.joined[b]:
            assert shifts[b] == 0 and not q[b].any()
            continue
        pa = plan.lead[b - 1] + int(shifts[b - 1]) + plan.body[b - 1]
        a = [float(v) for v in rows[b - 1][pa:pa + X]]
        want = []
        for d in range(-R, R):
            c = [float(v) for v in rows[b][plan.lead[b] + d:plan.lead[b] + d + X]]
            nom = den = 0.0
            for aj, cj in zip(a, c):
                nom += aj * cj
                den += cj * cj
            want.append(nom * abs(nom) / (den + plan.eps))
        assert q[b].tolist() == want
        order = sorted(range(-R, R), key=lambda d: (-want[d + R], abs(d), -d))
        assert shifts[b] == order[0]


def test_tie_rule():
    """Equal q: the smaller |d| wins, then the greater d. A period-2 signal makes d and d +- 2 exact ties."""
    X, R = 8, 3
    per = np.tile(np.array([0.25, -0.5], np.float32), 40)
    plan = A.StitchPlan([60, 60], [0, 10], [20, 20], [0, 1], [0, 20], 40, X, R, 1e-8)
    out, shifts, q = A.stitch([per[:60], per[:60]], plan, return_shifts=True, return_q=True)
    # candidates -3..2: d even lines up (q > 0, all equal), d odd is in antiphase (q < 0)
    assert q[1, 1] == q[1, 3] == q[1, 5] > 0 > q[1, 0] == q[1, 2] == q[1, 4]
    assert shifts[1] == 0
    assert A.stitch_pick(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), 3) == 1   # d = -3 and d = 1: the smaller |d|
    assert A.stitch_pick(np.array([0.0, 1.0, 0.0, 0.0, 0.0, 1.0]), 3) == 2   # d = -2 and d = 2: the greater d
    assert A.stitch_pick(np.array([0.0, 0.0]), 1) == 0


def test_plan_errors():
    x, rows, plan = known_shift_case()
    A.check_stitch_plan(plan, [len(r) for r in rows])
    bad = [plan._replace(xfade=0), plan._replace(xfade=8193), plan._replace(search=-1), plan._replace(search=1025),
           plan._replace(eps=0.0), plan._replace(eps=float("nan")), plan._replace(joined=[1, 1, 1]),
           plan._replace(out_off=[0, 1001, 2100]), plan._replace(out_off=[0, 999, 2100]),
           plan._replace(body=[1000, 63, 900], out_off=[0, 1000, 1063]), plan._replace(body=[0, 1100, 900]),
           plan._replace(out_len=2999), plan._replace(out_off=[-1, 999, 2099]),
           plan._replace(joined=[0, 0, 0], out_off=[0, 900, 2100]),          # two unjoined intervals overlap
           plan._replace(lead=[0, 7, 100]),                                  # lead - R < 0
           plan._replace(n=[plan.n[0], plan.n[1], plan.lead[2] + 7 + plan.body[2] - 1]),   # lead + R - 1 + body > n
           plan._replace(n=[plan.body[0] + 63, plan.n[1], plan.n[2]]),       # the predecessor's continuation ends past n
           plan._replace(n=[plan.n[0], plan.lead[1] + 7 + plan.body[1] + 64 - 1, plan.n[2]])]
    for p in bad:
        with pytest.raises(ValueError):
            A.stitch(rows, p)
    with pytest.raises(ValueError):
        A.stitch(rows[:2], plan)
    with pytest.raises(ValueError):
        A.stitch([rows[0], rows[1], rows[2][:-1]], plan)  # a row shorter than its n
    # the tightest rows pass
    tight = plan._replace(n=[plan.body[0] + 64, plan.lead[1] + 7 + plan.body[1] + 64, plan.lead[2] + 7 + plan.body[2]])
    A.stitch(rows, tight)


def test_header_declares_the_entry_point():
    header = open(os.path.join(REPO, "include", "svc_hip.h")).read()
    m = re.search(r"^svc_status\s+svc_stitch\s*\(([^;]*)\);", header, re.M)
    assert m, "svc_stitch is not declared"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["svc_ctx* ctx", "const float* const* rows", "int B", "const int64_t* n", "const int64_t* lead",
                    "const int64_t* body", "const int32_t* joined", "const int64_t* out_off", "int xfade", "int search",
                    "double eps", "float* out", "int64_t out_len", "int32_t* shift_out", "double* q_out", "void* stream"]
    res, argtypes = _lib.PROTOTYPES["svc_stitch"]
    want = [ctypes.c_int if a.startswith("int ") else ctypes.c_int64 if a.startswith("int64_t ") else
            ctypes.c_double if a.startswith("double ") else ctypes.c_void_p for a in args]
    assert res is ctypes.c_int and argtypes == want
    assert hasattr(_lib.load(), "svc_stitch")
    # null context: rejected before anything else, naming the entry point
    assert _lib.load().svc_stitch(None, None, 1, None, None, None, None, None, 64, 8, 1e-8, None, 1, None, None, None) == 1
    assert b"stitch" in _lib.load().svc_last_error()


def test_cli_flags(capsys):
    from svc_inference_pipeline_amd import infer
    ap = infer.build_parser()
    a = ap.parse_args(["--wav", "a.wav"])
    assert a.clip is None and a.clip_context is None
    a = ap.parse_args(["--wav", "a.wav", "--clip", "0.8", "--clip-context", "0.32"])
    assert a.clip == 0.8 and a.clip_context == 0.32
    for argv, word in ((["--clip-context", "0.3"], "--clip"), (["--clip", "0"], "clip_s"),
                       (["--clip", "10", "--clip-context", "0.1"], "right context")):
        with pytest.raises(SystemExit) as exc:  # before any model is loaded
            infer.main(["--wav", "a.wav", "--random-weights", "tiny-test"] + argv)
        assert exc.value.code == 2 and word in capsys.readouterr().err
