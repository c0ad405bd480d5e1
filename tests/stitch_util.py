"""Inputs shared by the stitch tests (host: test_stitch_host.py, device: test_gpu_stitch.py)."""
import numpy as np

from svc_inference_pipeline_amd import audio as A


def signal(rng, n):
    """|x| in [0.05, 0.5], random sign: no silent window, so no candidate's q is decided by eps."""
    return (rng.uniform(0.05, 0.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def known_shift_case(seed=0, X=64, R=8, deltas=(0, 5, -7), cuts=(0, 1000, 2100, 3000), lead=100, tail=200):
    """Chunks cut from ONE signal x, chunk k's row offset so that its body sample j sits at row index
    lead_k + deltas[k] + j. The aligned candidate reproduces the predecessor's continuation exactly (q = nom^2 / den with
    c = a, the Cauchy-Schwarz maximum, which a random signal reaches nowhere else), so the stitch must find d = deltas,
    and the crossfade of two equal signals is the signal: the output is x[:cuts[-1]] bit for bit.
    -> (x, rows, StitchPlan)."""
    rng = np.random.default_rng(seed)
    x = signal(rng, cuts[-1] + 1000)
    K = len(cuts) - 1
    rows, n, leads, body, off = [], [], [], [], []
    for k in range(K):
        b0, b1 = cuts[k], cuts[k + 1]
        L = lead if k else 0
        s = b0 - L - deltas[k]
        e = b1 + (tail if k < K - 1 else 2 * R + 3)  # the last row ends as soon as the range rule allows for any delta
        rows.append(x[s:e].copy())
        n.append(e - s), leads.append(L), body.append(b1 - b0), off.append(b0)
    return x, rows, A.StitchPlan(n, leads, body, [0] + [1] * (K - 1), off, cuts[-1], X, R, 1e-8)


def random_songs_case(seed, X, R, bodies=((301, None, 77), (130, 513, 64), (257,)), margin=5):
    """Songs of independent random rows (nothing lines up: the displacements are whatever the definition says). bodies:
    per song its chunks' body lengths, None standing for a body of exactly X samples; a body shorter than X is raised
    to X. Every row is as short as the range rule allows plus `margin` samples. -> (rows, StitchPlan); the songs' outputs
    are laid out back to back with a gap of 3 unwritten samples between songs."""
    rng = np.random.default_rng(seed)
    rows, n, leads, body, joined, off = [], [], [], [], [], []
    pos = 2
    for song in bodies:
        for k, bl in enumerate(song):
            bl = X if bl is None else (max(bl, X) if k else bl)
            lead = (R + 1 + k) if k else 3
            d_hi = max(R - 1, 0) if k else 0
            tail = X if k + 1 < len(song) else 0
            nk = lead + d_hi + bl + tail + (margin if k % 2 == 0 else 0)
            rows.append(signal(rng, nk + 2))
            n.append(nk), leads.append(lead), body.append(bl), joined.append(1 if k else 0), off.append(pos)
            pos += bl
        pos += 3
    return rows, A.StitchPlan(n, leads, body, joined, off, pos + 1, X, R, 1e-8)


def chain_case(seed=3, seams=40, X=16, R=4):
    """One song of seams + 1 chunks with bodies of 16..40 samples."""
    rng = np.random.default_rng(seed)
    bodies = [int(b) for b in rng.integers(16, 41, seams + 1)]
    bodies[1], bodies[2] = 16, 40
    return random_songs_case(seed, X, R, bodies=(tuple(bodies),), margin=1)


def ulps(got, want):
    """Distance in f32 steps (the two zeros coincide)."""
    o = lambda a: np.where(a.view(np.int32) < 0, -(a.view(np.int32).astype(np.int64) & 0x7FFFFFFF),
                           a.view(np.int32).astype(np.int64))
    return np.abs(o(np.ascontiguousarray(got, dtype=np.float32)) - o(np.ascontiguousarray(want, dtype=np.float32)))
