"""Plain numpy fp64 references of K33 ``bisect_step`` in the direct form (a row goes right iff it is strictly closer to
the right child: no hyperplane, no expanded square), of the whole BisectingKMeans fit given the noise vectors, and the
precision yardstick (the kernel's formulation in plain torch fp32 on the CPU).  An entry is [c~_L, c~_R], a missing
child is None."""
import functools

import numpy as np
import torch

WEIGHTS = np.array([0.0, 1.0, 2.0, 0.5])


def _unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-30)


def dist(xs, c, cosine):
    """D of every row (already shifted, or normalised for the cosine) to the centre c; inf for a missing one"""
    if c is None:
        return np.full(len(xs), np.inf)
    return ((xs - (_unit(c) if cosine else c)) ** 2).sum(1) * (0.5 if cosine else 1.0)   # |x^ - c^|^2 = 2 (1 - cos)


def table(ents, d):
    """(h, t) of the op from the entries' child centres"""
    h = np.array([np.zeros(d) if l is None or r is None else r - l for l, r in ents])
    t = [(np.inf if r is None else -np.inf) if l is None or r is None else (r @ r - l @ l) / 2 for l, r in ents]
    return h, t


def rights(xs, ents, e, cosine):
    """per row at entry e >= 0: strictly closer to the right child"""
    out = np.zeros(len(xs), dtype=bool)
    for j in np.unique(e[e >= 0]):
        m = e == j
        out[m] = dist(xs[m], ents[j][1], cosine) < dist(xs[m], ents[j][0], cosine)
    return out


def step(X, ents, node, w, cosine=False, shift=0.0):
    """W, cnt [M, 2], S [M, 2, d], Q [M, 2] of BISECT_STEP and the sides"""
    xs = _unit(np.asarray(X, np.float64)) if cosine else np.asarray(X, np.float64) - shift
    r = rights(xs, ents, node, cosine)
    M, d = len(ents), xs.shape[1]
    W, cnt, S, Q = np.zeros((M, 2)), np.zeros((M, 2)), np.zeros((M, 2, d)), np.zeros((M, 2))
    for e in range(M):
        for s in (0, 1):
            m = (node == e) & (r == bool(s))
            W[e, s], cnt[e, s], S[e, s], Q[e, s] = w[m].sum(), m.sum(), w[m] @ xs[m], w[m] @ (xs[m] ** 2).sum(1)
    return dict(W=W, cnt=cnt, S=S, Q=Q, right=r)


def predict(X, ents, left, right, centres, w, cosine=False, shift=0.0):
    """(leaf, cost) of BISECT_PREDICT: the walk from entry 0"""
    xs = _unit(np.asarray(X, np.float64)) if cosine else np.asarray(X, np.float64) - shift
    e = np.zeros(len(xs), dtype=np.int64)
    while (e >= 0).any():
        e = np.where(e >= 0, np.where(rights(xs, ents, e, cosine), np.asarray(right)[e], np.asarray(left)[e]), e)
    leaf = -1 - e
    D = np.array([dist(xs[i:i + 1], centres[j], cosine)[0] for i, j in enumerate(leaf)])
    return leaf.astype(np.int32), float(w @ D)


def yardstick(X, ents, node, w, cosine, shift, right):
    """(S, Q) of the kernel's formulation in plain torch fp32, at the reference's sides"""
    Xt, wt = torch.tensor(X), torch.tensor(w, dtype=torch.float32)
    xs = Xt / torch.linalg.vector_norm(Xt, dim=1, keepdim=True).clamp_min(1e-30) if cosine else Xt - torch.tensor(shift)
    A = torch.zeros(len(X), 2 * len(ents))
    live = node >= 0
    A[np.nonzero(live)[0], torch.tensor(2 * node + right)[live]] = wt[live]
    return (A.T @ xs).double().numpy().reshape(len(ents), 2, -1), (A.T @ (xs * xs).sum(1)).double().numpy().reshape(-1, 2)


def yard_cost(X, C, w, cosine, shift):
    """the PREDICT cost in plain torch fp32, row i at the centre C[i] (c~, or c^)"""
    Xt, Ct, wt = torch.tensor(X), torch.tensor(C, dtype=torch.float32), torch.tensor(w, dtype=torch.float32)
    if cosine:
        return float((wt * (1.0 - (Xt * Ct).sum(1) / torch.linalg.vector_norm(Xt, dim=1).clamp_min(1e-30))).sum())
    return float((wt * ((Xt - torch.tensor(shift) - Ct) ** 2).sum(1)).sum())


@functools.lru_cache(maxsize=None)
def exact_case(n, d, M):
    """Integers: rows in [-8, 8], integer child centres (c~_R - c~_L even and non-zero) and shift, weights from
    WEIGHTS.  From M = 3 on entry 0 misses its right child, entry 1 its left one and no row stands at entry M - 1;
    M = 2: entry 0 misses its left child.  Row 0 lies exactly on the hyperplane of the last entry rows stand at."""
    g = np.random.default_rng(1000 * n + 10 * d + M)
    X = g.integers(-8, 9, (n, d)).astype(np.float32)
    shift = g.integers(-3, 4, d).astype(np.float32)
    cl = g.integers(-8, 9, (M, d)).astype(np.float64)
    cr = cl + 2.0 * g.integers(-2, 3, (M, d))
    cr[:, 0] = cl[:, 0] + 2.0
    ents = [[cl[e], cr[e]] for e in range(M)]
    if M >= 3:
        ents[0][1], ents[1][0] = None, None
    elif M == 2:
        ents[0][0] = None
    used = M - 1 if M >= 3 else M
    node = g.integers(-1, used, n).astype(np.int32)
    node[0] = used - 1
    X[0] = (cl[used - 1] + cr[used - 1]) / 2 + shift
    w = WEIGHTS[g.integers(0, 4, n)]
    w[0] = 1.0
    left, right = g.integers(-5, M, M), g.integers(-5, M, M)
    return dict(X=X, shift=shift, ents=ents, node=node, w=w, left=left, right=right,
                ref=step(X, ents, node, w, False, shift.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def tree_case(n, d, chain):
    """A PREDICT tree on integers: a chain of depth 31 along column 0 (entry e sends x~_0 <= e + 1/2 to leaf e), or the
    balanced tree of 128 leaves in heap order with random children."""
    g = np.random.default_rng(n + d + chain)
    X = g.integers(-8, 9, (n, d)).astype(np.float32)
    shift = g.integers(-3, 4, d).astype(np.float32)
    w = WEIGHTS[g.integers(0, 4, n)]
    if chain:
        X[:, 0] = g.integers(-2, 35, n) + shift[0]
        u = np.eye(d)[0]
        ents = [[e * u, (e + 1) * u] for e in range(31)]
        left, right = -1 - np.arange(31), np.append(np.arange(1, 31), -32)
    else:
        cl = g.integers(-8, 9, (127, d)).astype(np.float64)
        ents = [[c, c + 2.0 * np.eye(d)[0] * (1 + (i % 3))] for i, c in enumerate(cl)]
        kid = lambda c: np.where(c < 127, c, 126 - c)   # noqa: E731  (leaf c - 127 is the target 126 - c)
        left, right = kid(2 * np.arange(127) + 1), kid(2 * np.arange(127) + 2)
    cen = g.integers(-8, 9, (len(ents) + 1, d)).astype(np.float64)
    return dict(X=X, shift=shift, w=w, ents=ents, left=left, right=right, cen=cen,
                ref=predict(X, ents, left, right, cen, w, False, shift.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def blob_case(n, d, M, cosine):
    """2 M Gaussian blobs far from the origin (centres 1000 + 100 N(0, 1), rows centre + N(0, 1)); entry e splits the
    blobs 2 e and 2 e + 1 at centres moved by 0.1 N(0, 1), every row stands at its blob's entry.  ``margin`` is
    |x~ . h - t| / (|x~| |h| + |t|) per row, in the frame the kernel works in."""
    g = np.random.default_rng(d + 7 * M)
    T = 1000.0 + 100.0 * g.standard_normal((2 * M, d))
    b = g.integers(0, 2 * M, n)
    X = (T[b] + g.standard_normal((n, d))).astype(np.float32)
    C = T + 0.1 * g.standard_normal((2 * M, d))
    shift = np.zeros(d, np.float32) if cosine else C.mean(0).astype(np.float32)
    Ct = _unit(C) if cosine else C - shift.astype(np.float64)
    ents = [[Ct[2 * e], Ct[2 * e + 1]] for e in range(M)]
    node, w = (b // 2).astype(np.int32), 0.5 + g.random(n)
    h, t = table(ents, d)
    xs = X.astype(np.float64) - shift
    margin = np.abs((xs * h[node]).sum(1) - np.asarray(t)[node]) / (
        np.linalg.norm(xs, axis=1) * np.linalg.norm(h[node], axis=1) + np.abs(np.asarray(t)[node]))
    ref = step(X, ents, node, w, cosine, shift.astype(np.float64))
    return dict(X=X, shift=shift, ents=ents, node=node, w=w, ref=ref, margin=margin, cen=Ct,
                yard=yardstick(X, ents, node, w, cosine, shift, ref["right"]))


def fit(X, w, k, max_iter, min_div, cosine, noise):
    """The level-wise fit in fp64, the noise vectors given in the order they are drawn: {tree index: (W, centre,
    cost)} and the leaves' indices depth-first, left first."""
    X = _unit(np.asarray(X, np.float64)) if cosine else np.asarray(X, np.float64)
    w, noise = np.ones(len(X)) if w is None else np.asarray(w, np.float64), iter(noise)

    def summary(m):
        S = w[m] @ X[m]
        c = _unit(S) if cosine else S / w[m].sum()
        return w[m].sum(), c, float(w[m] @ dist(X[m], c, cosine))
    at = np.ones(len(X), dtype=np.int64)
    info, need, active = {1: summary(at == 1)}, k - 1, [1]
    min_size = min_div if min_div >= 1 else min_div * info[1][0]
    while need > 0 and active and max_iter > 0:
        div = [i for i in active if info[i][0] >= min_size and info[i][2] > 2.220446049250313e-16 * info[i][0]]
        div = sorted(sorted(div, key=lambda i: (-info[i][0], i))[:need])
        if not div:
            break
        cen = {}
        for i in div:
            c, z = info[i][1], next(noise)
            lv = 1e-4 * np.linalg.norm(c)
            cen[2 * i], cen[2 * i + 1] = c - lv * z, c + lv * z
        for it in range(max_iter + 1):     # the last round assigns with the final centres and summarises nothing
            ents = [[cen.get(2 * i), cen.get(2 * i + 1)] for i in div]
            e = np.array([div.index(i) if i in div else -1 for i in at])
            child = np.where(e >= 0, 2 * at + rights(X, ents, e, cosine), at)
            if it == max_iter:
                break
            new = {c: summary(child == c) for c in cen if (w[child == c]).sum() > 0}
            cen = {c: new[c][1] for c in new}
        at, active, need = child, sorted(new), need - len(div)
        info.update(new)

    def leaves(i):
        kids = [c for c in (2 * i, 2 * i + 1) if c in info]
        return [x for c in kids for x in leaves(c)] if kids else [i]
    return info, leaves(1)
