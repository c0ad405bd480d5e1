"""Host reference of index compaction (include/svc_hip.h svc_index_assign / svc_index_update / svc_index_kmeans), numpy
on top of tests/retrieve_ref.py. It is the contract restated, not the kernels: the assignment is retrieval's score and
total order (s, j) with k = 1; the update is the exact integer mean; the loop starts from rows floor(i N / K).

The scores are f64 here and f32 on the device, so a device label may differ from the reference's where a row's two best
scores lie within 2 tau of each other (retrieve_ref.tau bounds one device score's error); near_ties() counts such rows.
The update has no such slack: given the same labels, the device's centroids and norms are these bit for bit.
"""
import numpy as np

import retrieve_ref as R


def init_rows(N, K):
    """The rows the centroids start from: floor(i N / K), SVCPipeline.enroll's index_max_rows rule."""
    return [i * int(N) // int(K) for i in range(int(K))]


def assign(x16, c16, norms=None):
    """-> dict(labels int64 [N], s f64 [N, K], best f64 [N], gap f64 [N] (second best - best, inf for K = 1),
    tau f64 [N], counts int64 [K], inertia float: sum_r max(|x_r|^2 + s_label, 0) in f64)."""
    s = R.scores(x16, c16, norms)
    N, K = s.shape
    labels = np.array([R.order(row)[0] for row in s], np.int64)
    srt = np.sort(s, axis=1)
    gap = srt[:, 1] - srt[:, 0] if K > 1 else np.full(N, np.inf)
    x = np.asarray(x16, np.float16).astype(np.float64)
    x2 = np.einsum("rc,rc->r", x, x)
    best = s[np.arange(N), labels]
    return dict(labels=labels, s=s, best=best, gap=gap, tau=R.tau(x16, c16, norms),
                counts=np.bincount(labels, minlength=K).astype(np.int64),
                inertia=float(np.maximum(x2 + best, 0.0).sum()), x2=x2)


def near_ties(a):
    """Rows of an assign() result whose best-to-second gap is below 2 tau: where a device label may differ."""
    return a["gap"] < 2.0 * a["tau"]


def to_int(x16):
    """I(v) = v 2^24 as int64: exact for every finite f16 value, |I| < 2^40."""
    v = np.asarray(x16, np.float16).astype(np.float64) * 2.0 ** 24
    i = v.astype(np.int64)
    assert np.array_equal(i.astype(np.float64), v)
    return i


def exact_mean(x16, members):
    """f16 [D]: (half)(float)(((double)S / (double)count) 2^-24) over the member rows; S an exact int64 sum."""
    members = np.asarray(members, np.int64)
    S = to_int(np.asarray(x16, np.float16)[members]).sum(axis=0, dtype=np.int64)
    q = S.astype(np.float64) / np.float64(members.size)
    return (q * 2.0 ** -24).astype(np.float32).astype(np.float16)


def update(x16, labels, prev16):
    """-> (centroids f16 [K, D], norms f32 [K], counts int64 [K]); an empty cluster keeps prev16's row. Labels outside
    [0, K) join no cluster."""
    prev16 = np.asarray(prev16, np.float16)
    labels = np.asarray(labels, np.int64)
    K = prev16.shape[0]
    out = prev16.copy()
    counts = np.zeros(K, np.int64)
    order = np.argsort(labels, kind="stable")
    lo = np.searchsorted(labels[order], np.arange(K), "left")
    hi = np.searchsorted(labels[order], np.arange(K), "right")
    for j in range(K):
        counts[j] = hi[j] - lo[j]
        if counts[j]:
            out[j] = exact_mean(x16, order[lo[j]:hi[j]])
    return out, R.index_norms(out), counts


def kmeans(x16, K, iters):
    """-> dict(centroids, norms, labels, counts, inertia [iters + 1], steps: every assign() result in order)."""
    x16 = np.asarray(x16, np.float16)
    c = x16[init_rows(x16.shape[0], K)].copy()
    norms = R.index_norms(c)
    steps, inertia = [], []
    for _ in range(int(iters)):
        a = assign(x16, c, norms)
        steps.append(a)
        inertia.append(a["inertia"])
        c, norms, _ = update(x16, a["labels"], c)
    a = assign(x16, c, norms)
    steps.append(a)
    inertia.append(a["inertia"])
    return dict(centroids=c, norms=norms, labels=a["labels"], counts=a["counts"], inertia=np.array(inertia), steps=steps)


def brute_force(x16, K, iters):
    """The same by Python ints and scalar loops (tiny shapes only) -> (centroid bit patterns [K][D], labels [N])."""
    x = [[float(v) for v in row] for row in np.asarray(x16, np.float16)]
    xi = [[int(v * 2 ** 24) for v in row] for row in x]
    N, D = len(x), len(x[0])
    c = [list(x[i]) for i in init_rows(N, K)]

    def labels_of(c):
        out = []
        for xr in x:
            sc = []
            for j, cr in enumerate(c):
                nrm = 0.0
                for v in cr:
                    nrm += v * v
                dot = 0.0
                for a, b in zip(xr, cr):
                    dot += a * b
                sc.append((float(np.float32(nrm)) - 2.0 * dot, j))
            out.append(min(sc)[1])
        return out

    for _ in range(int(iters)):
        lab = labels_of(c)
        for j in range(K):
            mem = [r for r in range(N) if lab[r] == j]
            if mem:
                S = [sum(xi[r][col] for r in mem) for col in range(D)]
                c[j] = [float(np.float16(np.float32(np.float64(s) / np.float64(len(mem)) * 2.0 ** -24))) for s in S]
    bits = [[int(np.float16(v).view(np.uint16)) for v in row] for row in c]
    return bits, labels_of(c)
