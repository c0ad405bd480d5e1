"""The long-form join on the GPU: svc_stitch against the host definition audio.stitch.

What is compared, and why at these tolerances:
  - displacements and q: bit-equal. nom and den are f64 sums, in ascending j, of products of two f32 values, which are
    exact in f64; so fused and unfused multiply-adds round alike, q follows in three IEEE operations, and the order on
    (q, |d|, d) is total;
  - copied samples: bit-equal;
  - crossfade samples: within 1 f32 ulp (the definition's f64 operations in the same order; the bound allows a
    differently rounded f64 intermediate to move the final f32 rounding by one step), exact where c == a;
  - only the body intervals are written: every output buffer is pre-filled with a sentinel, a guard region after the
    last sample included, and rows and outputs start 1 and 3 elements off a 16-byte boundary.
Inputs have |x| in [0.05, 0.5], so no window is silent except where silence is the test."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import ptr, stream  # noqa: E402
from stitch_util import chain_case, known_shift_case, random_songs_case, ulps  # noqa: E402
from svc_inference_pipeline_amd import _lib  # noqa: E402
from svc_inference_pipeline_amd import audio as A  # noqa: E402
from svc_inference_pipeline_amd import config as C  # noqa: E402
from svc_inference_pipeline_amd.runtime import SVCEngine  # noqa: E402

SENTINEL = 77.0
GUARD = 64


@pytest.fixture(scope="module")
def engine():
    """A context without weights: svc_stitch needs none."""
    e = SVCEngine(C.load_config(), 0)
    yield e
    e.close()


def launch(e, rows, plan, row_off=1, out_off=3, want_q=True):
    """Enqueue one svc_stitch call: the rows live in one sentinel-filled device buffer, row b starting row_off + b
    elements past a 16-byte boundary, each followed by sentinels; out starts out_off elements into its buffer."""
    B = len(rows)
    starts, pos = [], 0
    for b, r in enumerate(rows):
        pos = (pos + 3) // 4 * 4 + (row_off + b) % 4
        starts.append(pos)
        pos += len(r) + 2
    host = np.full(pos + 4, SENTINEL, np.float32)
    for s, r in zip(starts, rows):
        host[s:s + len(r)] = r
    rbuf = torch.from_numpy(host).cuda()
    obuf = torch.full((out_off + plan.out_len + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    nc = max(2 * plan.search, 1)
    sbuf = torch.full((B + 1,), -99, dtype=torch.int32, device="cuda")
    qbuf = torch.full(((B + 1) * nc,), -1.0, dtype=torch.float64, device="cuda") if want_q else None
    i64 = lambda v: (ctypes.c_int64 * B)(*[int(x) for x in v])
    _lib.call("svc_stitch", e._ctx, (ctypes.c_void_p * B)(*[rbuf.data_ptr() + 4 * s for s in starts]), B, i64(plan.n),
              i64(plan.lead), i64(plan.body), (ctypes.c_int32 * B)(*plan.joined), i64(plan.out_off), plan.xfade,
              plan.search, plan.eps, ctypes.c_void_p(obuf.data_ptr() + 4 * out_off), plan.out_len, ptr(sbuf), ptr(qbuf),
              stream())
    return rbuf, obuf, sbuf, qbuf, (B, nc, out_off, plan)


def collect(handles):
    """-> (out f32 [out_len] with the sentinel wherever nothing was written, shifts, q) once the stream has drained; the
    sentinels around out, shifts and q are asserted."""
    _, obuf, sbuf, qbuf, (B, nc, out_off, plan) = handles
    torch.cuda.synchronize()
    flat, s = obuf.cpu().numpy(), sbuf.cpu().numpy()
    assert np.all(flat[:out_off] == SENTINEL), "samples before out were written"
    assert np.all(flat[out_off + plan.out_len:] == SENTINEL), "the guard region after out was written"
    assert s[B] == -99
    q = None
    if qbuf is not None:
        q = qbuf.cpu().numpy()
        assert np.all(q[B * nc:] == -1.0), "q's guard row was written"
        q = q[:B * nc].reshape(B, nc)
    return flat[out_off:out_off + plan.out_len], s[:B], q


def body_mask(plan):
    m = np.zeros(plan.out_len, bool)
    for off, body in zip(plan.out_off, plan.body):
        m[off:off + body] = True
    return m


def compare(got, rows, plan):
    """The device result against audio.stitch of the same rows."""
    out, shifts, q = got
    want, want_shifts, want_q = A.stitch(rows, plan, return_shifts=True, return_q=True)
    assert shifts.tolist() == want_shifts.tolist()
    if q is not None:
        assert np.array_equal(q, want_q), float(np.abs(q - want_q).max())
    m = body_mask(plan)
    assert np.all(out[~m] == SENTINEL), "a sample outside every body interval was written"
    fade = np.zeros(plan.out_len, bool)  # the crossfade samples
    for b in range(len(rows)):
        if plan.joined[b]:
            fade[plan.out_off[b]:plan.out_off[b] + plan.xfade] = True
    assert np.array_equal(out[m & ~fade], want[m & ~fade]), "a copied sample differs"
    d = ulps(out[fade], want[fade])
    print(f"X={plan.xfade} R={plan.search} B={len(rows)}: shifts {shifts.tolist()}, crossfade max ulp "
          f"{int(d.max()) if d.size else 0}")
    assert d.size == 0 or d.max() <= 1, int(d.max())
    return out, shifts, q


def test_known_shifts(engine):
    """The host test's case: displacements = delta, output bit-equal to the signal."""
    x, rows, plan = known_shift_case()
    out, shifts, q = compare(collect(launch(engine, rows, plan)), rows, plan)
    assert shifts.tolist() == [0, 5, -7]
    assert np.array_equal(out, x[:plan.out_len])  # exact where c == a, the crossfade included


@pytest.mark.parametrize("X,R", [(64, 8), (63, 1), (64, 0)])
def test_against_the_host_definition(engine, X, R):
    """7 chunks: two songs of 3 chunks and a stand-alone chunk, independent random rows, odd bodies and a body equal to
    X, rows as short as the range rule allows; and each song stitched alone equals its interval of the batched call."""
    rows, plan = random_songs_case(X + R, X, R)
    assert len(rows) == 7 and plan.joined == [0, 1, 1, 0, 1, 1, 0] and X in plan.body
    out, shifts, q = compare(collect(launch(engine, rows, plan)), rows, plan)
    for lo, hi in ((0, 3), (3, 6), (6, 7)):
        base = plan.out_off[lo]
        length = plan.out_off[hi - 1] + plan.body[hi - 1] - base
        solo = A.StitchPlan(plan.n[lo:hi], plan.lead[lo:hi], plan.body[lo:hi], plan.joined[lo:hi],
                            [o - base for o in plan.out_off[lo:hi]], length, X, R, plan.eps)
        o1, s1, q1 = collect(launch(engine, rows[lo:hi], solo, row_off=2, out_off=1))
        assert np.array_equal(o1, out[base:base + length]) and s1.tolist() == shifts[lo:hi].tolist()
        assert np.array_equal(q1, q[lo:hi])


def test_one_seam_at_the_defaults(engine):
    """X = 1024, R = 192: 384 candidates of 1024 terms, one candidate per thread; bodies that span several write
    blocks and end off the 16-byte grid."""
    rows, plan = random_songs_case(7, 1024, 192, bodies=((4099, 2051),), margin=0)
    out, shifts, q = compare(collect(launch(engine, rows, plan)), rows, plan)
    assert q.shape == (2, 384) and -192 <= shifts[1] < 192
    # and a seam whose answer is known, at the defaults
    x, rows, plan = known_shift_case(seed=2, X=1024, R=192, deltas=(0, -192, 191), cuts=(0, 3000, 6000, 9000), lead=200,
                                     tail=1500)
    out, shifts, _ = compare(collect(launch(engine, rows, plan)), rows, plan)
    assert shifts.tolist() == [0, -192, 191] and np.array_equal(out, x[:plan.out_len])


def test_largest_windows(engine):
    """xfade = 8192 and search = 1024, the entry point's limits: 72 KiB of LDS, two candidates per thread."""
    rows, plan = random_songs_case(9, 8192, 1024, bodies=((100, 8192),), margin=0)
    out, shifts, q = compare(collect(launch(engine, rows, plan)), rows, plan)
    assert q.shape == (2, 2048)


def test_chain_of_40_seams(engine):
    rows, plan = chain_case()
    assert len(rows) == 41 and sum(plan.joined) == 40 and min(plan.body[1:]) == 16 and max(plan.body) == 40
    out, shifts, q = compare(collect(launch(engine, rows, plan)), rows, plan)
    assert len(set(shifts.tolist())) > 3  # the displacements vary along the chain
    flat = A.stitch(rows, plan, chain=False)  # and the chain is what the device follows
    assert not np.array_equal(flat[body_mask(plan)], out[body_mask(plan)])


def test_silence_gives_zero_displacement(engine):
    _, rows, plan = known_shift_case()
    zeros = [np.zeros_like(r) for r in rows]
    out, shifts, q = compare(collect(launch(engine, zeros, plan)), zeros, plan)
    assert shifts.tolist() == [0, 0, 0] and not out.any() and not q.any()


@pytest.mark.parametrize("B", [1, 7])
def test_two_launches_whatever_the_batch(engine, B):
    rows, plan = random_songs_case(1, 64, 8, bodies=((257,),) if B == 1 else ((301, None, 77), (130, 513, 64), (257,)))
    assert len(rows) == B
    _lib.profile_filter("stitch")
    _lib.profile_enable(True)
    try:
        collect(launch(engine, rows, plan))
        stats = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
        _lib.profile_filter("")
    assert {k.split("@")[0]: v["launches"] for k, v in stats.items()} == {"stitch_seams": 1, "stitch_write": 1}


def test_no_state_between_calls(engine):
    """Two calls back to back on one stream, other shapes and parameters: each equals its own host result (the staged
    tables and displacements of the first are not reused by the second)."""
    ra, pa = random_songs_case(21, 64, 8)
    rb, pb = chain_case(seed=5, seams=9)
    h1 = launch(engine, ra, pa)
    h2 = launch(engine, rb, pb, row_off=0, out_off=2, want_q=False)
    compare(collect(h1), ra, pa)
    compare(collect(h2), rb, pb)


def test_engine_method(engine):
    """SVCEngine.stitch with row views of one padded batch (the pipeline's form) is the same call."""
    rows, plan = random_songs_case(3, 64, 8)
    S = max(len(r) for r in rows)
    pad = torch.zeros(len(rows), S)
    for b, r in enumerate(rows):
        pad[b, :len(r)] = torch.from_numpy(r)
    pad = pad.cuda()
    views = [pad[b, :len(r)] for b, r in enumerate(rows)]
    out, shifts, q = engine.stitch(views, plan, return_shifts=True, return_q=True)
    want, ws, wq = A.stitch(rows, plan, return_shifts=True, return_q=True)
    assert shifts.cpu().tolist() == ws.tolist() and np.array_equal(q.cpu().numpy(), wq)
    assert ulps(out.cpu().numpy(), want).max() <= 1 and not out.cpu().numpy()[~body_mask(plan)].any()
    given = torch.full((plan.out_len,), SENTINEL, device="cuda")
    assert engine.stitch(views, plan, out=given) is given
    assert torch.equal(given[torch.from_numpy(body_mask(plan)).cuda()], out[torch.from_numpy(body_mask(plan)).cuda()])
    with pytest.raises(ValueError, match="rows for"):
        engine.stitch(views[:-1], plan)
    with pytest.raises(ValueError, match="out must be"):
        engine.stitch(views, plan, out=torch.empty(plan.out_len + 1, device="cuda"))


def test_argument_errors(engine):
    """Every SVC_ERR_INVALID case: status 1 before any HIP call, svc_last_error names stitch; the engine still works."""
    x, rows, plan = known_shift_case()
    lib = _lib.load()
    dev_rows = [torch.from_numpy(r).cuda() for r in rows]
    out = torch.full((plan.out_len + GUARD,), SENTINEL, device="cuda")
    B = 3

    def status(p=plan, ctx=engine._ctx, rws=dev_rows, o=out, null=None, B=B, o_ptr=None):
        i64 = lambda v: (ctypes.c_int64 * len(v))(*[int(k) for k in v])
        tabs = dict(rows=(ctypes.c_void_p * len(rws))(*[None if r is None else r.data_ptr() for r in rws]), n=i64(p.n),
                    lead=i64(p.lead), body=i64(p.body), joined=(ctypes.c_int32 * len(p.joined))(*p.joined),
                    out_off=i64(p.out_off))
        if null:
            tabs[null] = None
        po = o_ptr if o_ptr is not None else (None if o is None else ctypes.c_void_p(o.data_ptr()))
        return lib.svc_stitch(ctx, tabs["rows"], B, tabs["n"], tabs["lead"], tabs["body"], tabs["joined"],
                              tabs["out_off"], p.xfade, p.search, p.eps, po, p.out_len, None, None, stream())

    assert status() == 0
    R, X = plan.search, plan.xfade
    bad = [dict(ctx=None), dict(o=None), dict(rws=[dev_rows[0], None, dev_rows[2]]), dict(B=0), dict(B=-1)]
    bad += [dict(null=t) for t in ("rows", "n", "lead", "body", "joined", "out_off")]
    bad += [dict(p=p) for p in (
        plan._replace(xfade=0), plan._replace(xfade=8193), plan._replace(search=-1), plan._replace(search=1025),
        plan._replace(eps=0.0), plan._replace(eps=-1e-8), plan._replace(eps=float("nan")),
        plan._replace(joined=[1, 1, 1]), plan._replace(joined=[0, 2, 1]),
        plan._replace(out_off=[0, 1001, 2100]), plan._replace(out_off=[0, 999, 2100]),   # a joined chunk must abut
        plan._replace(body=[1000, X - 1, 900], out_off=[0, 1000, 1000 + X - 1]),         # body < xfade
        plan._replace(body=[0, 1100, 900]), plan._replace(body=[1000, 1100, -5]),
        plan._replace(out_len=2999), plan._replace(out_len=0), plan._replace(out_off=[-1, 999, 2099]),
        plan._replace(joined=[0, 0, 0], out_off=[0, 900, 2100]),                          # two intervals overlap
        plan._replace(joined=[0, 0, 0], out_off=[2000, 0, 1050]),                         # ... given out of order
        plan._replace(lead=[0, R - 1, 100]), plan._replace(lead=[-1, 100, 100]),          # a read before the row
        plan._replace(n=[plan.n[0], plan.n[1], plan.lead[2] + R - 1 + plan.body[2] - 1]),   # the displaced body's end
        plan._replace(n=[plan.body[0] + X - 1, plan.n[1], plan.n[2]]),                    # an unjoined predecessor's continuation
        plan._replace(n=[plan.n[0], plan.lead[1] + R - 1 + plan.body[1] + X - 1, plan.n[2]]),  # a displaced one's
        plan._replace(n=[plan.n[0], 0, plan.n[2]]))]
    bad += [dict(o_ptr=ctypes.c_void_p(dev_rows[1].data_ptr() + 4 * 10))]                  # out inside a row
    for kw in bad:
        assert status(**kw) == 1, kw  # SVC_ERR_INVALID
        assert b"stitch" in lib.svc_last_error(), kw
    torch.cuda.synchronize()
    # the tightest rows pass, and the engine still works
    tight = plan._replace(n=[plan.body[0] + X, plan.lead[1] + R - 1 + plan.body[1] + X, plan.lead[2] + R - 1 + plan.body[2]])
    assert status(p=tight) == 0
    with pytest.raises(_lib.SVCError, match="chunk 1"):
        engine.stitch(dev_rows, plan._replace(lead=[0, R - 1, 100]))
    compare(collect(launch(engine, rows, plan)), rows, plan)
