"""Host reference of feature retrieval (include/svc_hip.h svc_index_norms / svc_content_retrieve), numpy in f64 from the
f16 values. It is the contract restated, not the kernel: scores norms[j] - 2 dot(q, x_j), the k smallest under the total
order (s, j), distances clamped at the floor, inverse-distance weights, the blend and the mix with the query.

tau(r) is the worst-case error of a device f32 score of row r, derived and not measured: a dot product of D products
accumulated in f32 in any order is within D * 2^-24 * sum_i |q_i x_ji| of the exact one (each partial sum is bounded by
that sum of magnitudes; gamma_D to first order, doubled below for the higher-order terms), the score doubles it, and the
final subtraction from the f32 norm adds one rounding of a value bounded by 2 * bound + norm. Hence
    tau(r) = (D + 8) * 2^-23 * (2 * max_j sum_i |q_i x_ji| + max_j norms[j]).
"""
import numpy as np


def index_norms(x16):
    """f32 [N]: the f64 sum of squares of each row in column order, rounded to f32."""
    x = np.asarray(x16, np.float16).astype(np.float64)
    acc = np.zeros(x.shape[0], np.float64)
    for c in range(x.shape[1]):  # column order; every square is exact in f64
        acc += x[:, c] * x[:, c]
    return acc.astype(np.float32)


def scores(q16, x16, norms=None):
    """f64 [M, N]: norms[j] - 2 dot(q_r, x_j) from the f16 values and the f32 norms."""
    q = np.asarray(q16, np.float16).astype(np.float64)
    x = np.asarray(x16, np.float16).astype(np.float64)
    n = index_norms(x16) if norms is None else np.asarray(norms, np.float32)
    return n.astype(np.float64)[None, :] - 2.0 * (q @ x.T)


def tau(q16, x16, norms=None):
    """f64 [M]: the bound on |device f32 score - scores()| of each row (module docstring)."""
    q = np.abs(np.asarray(q16, np.float16).astype(np.float64))
    x = np.abs(np.asarray(x16, np.float16).astype(np.float64))
    n = index_norms(x16) if norms is None else np.asarray(norms, np.float32)
    D = q.shape[1]
    dot_bound = (q @ x.T).max(axis=1)
    return (D + 8) * 2.0 ** -23 * (2.0 * dot_bound + float(n.max()))


def order(s_row):
    """Indices of one row's scores sorted by the total order (s, j)."""
    return np.lexsort((np.arange(s_row.shape[0]), s_row))


def topk(s, k):
    """int64 [M, min(k, N)]: each row's selected j in rank order."""
    k_eff = min(int(k), s.shape[1])
    return np.stack([order(row)[:k_eff] for row in s]) if s.shape[0] else np.zeros((0, k_eff), np.int64)


def blend_row(q16_row, x16, s_row, idx, rate, dist_floor):
    """One row's blend over the index set `idx` (rank order) -> (out f64 [D] before the f16 rounding, d2 f64 [len(idx)]).
    dist_floor is taken as the device takes it, as an f32 value."""
    q = np.asarray(q16_row, np.float16).astype(np.float64)
    idx = np.asarray(idx, np.int64)
    if idx.size == 0:
        return (1.0 - rate) * q, np.zeros(0)
    x = np.asarray(x16, np.float16)[idx].astype(np.float64)
    d2 = np.maximum(float(q @ q) + s_row[idx], float(np.float32(dist_floor)))
    w = (1.0 / d2) / np.sum(1.0 / d2)
    y = w @ x
    return rate * y + (1.0 - rate) * q, d2


def f16_ulp(v):
    """The spacing of binary16 at |v| (the subnormal spacing 2^-24 below 2^-14)."""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def retrieve(q16, x16, k, rate, dist_floor, norms=None):
    """All rows take part. -> dict(s=[M, N] f64, sorted=[M, N] f64 ascending, idx=[M, k_eff], out=[M, D] f64 (before
    the f16 rounding), d2=[M, k_eff], tau=[M])."""
    s = scores(q16, x16, norms)
    idx = topk(s, k)
    M, D = np.asarray(q16).shape
    out = np.zeros((M, D))
    d2 = np.zeros(idx.shape)
    for r in range(M):
        out[r], d2[r] = blend_row(q16[r], x16, s[r], idx[r], rate, dist_floor)
    return dict(s=s, sorted=np.sort(s, axis=1), idx=idx, out=out, d2=d2, tau=tau(q16, x16, norms))


def brute_force(q16, x16, k, rate, dist_floor):
    """The same by plain Python loops over scalars (tiny shapes only): (idx lists, out rows, d2 lists)."""
    q = [[float(v) for v in row] for row in np.asarray(q16, np.float16)]
    x = [[float(v) for v in row] for row in np.asarray(x16, np.float16)]
    floor = float(np.float32(dist_floor))
    res = []
    for qr in q:
        sc = []
        for j, xr in enumerate(x):
            nrm = 0.0
            for v in xr:
                nrm += v * v
            nrm = float(np.float32(nrm))
            dot = 0.0
            for a, b in zip(qr, xr):
                dot += a * b
            sc.append((nrm - 2.0 * dot, j))
        sc.sort()
        pick = sc[:min(k, len(x))]
        q2 = sum(a * a for a in qr)
        d2 = [max(q2 + s, floor) for s, _ in pick]
        tot = sum(1.0 / d for d in d2)
        w = [(1.0 / d) / tot for d in d2]
        y = [sum(w[i] * x[pick[i][1]][c] for i in range(len(pick))) for c in range(len(qr))]
        res.append(([j for _, j in pick], [rate * yc + (1.0 - rate) * qc for yc, qc in zip(y, qr)], d2))
    return res
