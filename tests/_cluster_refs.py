"""Plain numpy references of K30 ``cluster_step``: the direct form sum (x - c)^2 in int64-exact fp64, and the
precision yardstick (the kernel's shifted, expanded formulation in plain torch fp32 on the CPU)."""
import functools

import numpy as np
import torch

WEIGHTS = np.array([0.0, 1.0, 2.0, 0.5])


def step(X, C, w=None, cosine=False):
    """assign (the lowest index among equal distances), sums [k, d], N [k], cost, and per row the margin
    (D_second - D_best) / (|x|^2 + |c_best|^2), in fp64 (exact for small integers)."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    w = np.ones(len(X)) if w is None else np.asarray(w, dtype=np.float64)
    if cosine:
        X = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-30)
        C = C / np.maximum(np.linalg.norm(C, axis=1, keepdims=True), 1e-30)
    D = np.stack([((X - c) ** 2).sum(1) for c in C], 1) * (0.5 if cosine else 1.0)   # |x^ - c^|^2 = 2 (1 - cos)
    a = D.argmin(1)
    A = np.zeros((len(X), len(C)))
    A[np.arange(len(X)), a] = w
    best = D[np.arange(len(X)), a]
    second = np.sort(D, 1)[:, 1] if len(C) > 1 else np.full(len(X), np.inf)
    margin = (second - best) / ((X ** 2).sum(1) + (C[a] ** 2).sum(1))
    return dict(assign=a.astype(np.int32), sums=A.T @ X, N=A.sum(0), cost=float((w * best).sum()), margin=margin)


@functools.lru_cache(maxsize=None)
def exact_case(d, k, n, seed=0):
    """Integers in [-8, 8], integer centres (the last a copy of the first: ties; from k = 3 on centre 1 far from every
    row: empty) and shift, weights from WEIGHTS: every fp32 product and partial sum of the kernel is exact."""
    g = np.random.default_rng(1000 * d + 10 * k + n + seed)
    X = g.integers(-8, 9, (n, d)).astype(np.float32)
    C = g.integers(-8, 9, (k, d)).astype(np.float64)
    C[-1] = C[0]
    if k >= 3:
        C[1] = 64.0
    w = WEIGHTS[g.integers(0, 4, n)]
    shift = g.integers(-3, 4, d).astype(np.float32)
    return dict(X=X, C=C, w=w, shift=shift, ref=step(X, C, w), ref1=step(X, C))


@functools.lru_cache(maxsize=None)
def blob_case(d, k, n, cosine, seed=0):
    """Well-separated Gaussian blobs far from the origin: centres 1000 + 100 N(0, 1), rows centre + N(0, 1); the
    centres handed to the op are the true ones moved by 0.1 N(0, 1).  With the reference and the yardstick."""
    g = np.random.default_rng(seed + d + 7 * k)
    T = 1000.0 + 100.0 * g.standard_normal((k, d))
    X = (T[g.integers(0, k, n)] + g.standard_normal((n, d))).astype(np.float32)
    C = T + 0.1 * g.standard_normal((k, d))
    w = 0.5 + g.random(n)
    shift = C.mean(0).astype(np.float32)
    ref = step(X, C, w, cosine)
    if not cosine:   # the margin in the shifted frame the kernel works in
        ref["margin"] = step(X - shift.astype(np.float64), C - shift.astype(np.float64), w)["margin"]
    return dict(X=X, C=C, w=w, shift=shift, ref=ref, yard=yardstick(X, C, w, shift, cosine))


def yardstick(X, C, w, shift, cosine):
    """(sums, cost) of the kernel's formulation in plain torch fp32."""
    Xt, wt, st = torch.tensor(X), torch.tensor(w, dtype=torch.float32), torch.tensor(shift)
    if cosine:
        xs = Xt / torch.linalg.vector_norm(Xt, dim=1, keepdim=True).clamp_min(1e-30)
        ct = torch.tensor(C / np.linalg.norm(C, axis=1, keepdims=True), dtype=torch.float32)
        D = 1.0 - xs @ ct.T
    else:
        xs = Xt - st
        ct = torch.tensor(C - shift.astype(np.float64), dtype=torch.float32)
        D = (xs * xs).sum(1)[:, None] - 2.0 * xs @ ct.T + (ct * ct).sum(1)[None, :]
    best, a = D.min(1)
    A = torch.zeros(D.shape).scatter_(1, a[:, None], wt[:, None])
    sums = A.T @ xs + (0.0 if cosine else A.sum(0)[:, None] * st[None, :])
    return sums.double().numpy(), float((wt * best).sum())
