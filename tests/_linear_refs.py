"""References for ``K.linear_step`` (K31), written independently of the package code.

Softmax (K = C >= 2): z = W x + b, loss = w (logsumexp(z) - z_y), R = w (softmax(z) - onehot(y)).  Binomial (K = 1):
m = x.w + b, loss = w (log(1 + e^m) - y m), R = w (sigmoid(m) - y), raw = [-m, m], prob = [1 - p, p].  The gradient is
[R^T X (class-major) | column sums of R].  ``reference``: ``np.longdouble`` terms, exact sums; ``yardstick``: plain
numpy fp64 in row order; the criterion is ``_aft_refs.check`` (8 x the yardstick's error, floor 4 ulps of the largest).
"""
import functools

import numpy as np

from tests._aft_refs import ULP, _fsum, check


def make_data(d, n, K, weighted, seed=0):
    """(X fp32, y, w or None, W [K, d], b [K]): standard-normal rows, labels uniform over the classes."""
    rng = np.random.default_rng(seed + 1000 * d + 10 * n + K)
    X = rng.normal(size=(n, d)).astype(np.float32)
    y = rng.integers(0, max(K, 2), size=n).astype(np.float64)
    w = rng.uniform(0.5, 2.0, size=n) if weighted else None
    return X, y, w, rng.normal(scale=1.0 / np.sqrt(d), size=(K, d)), rng.normal(scale=0.3, size=K)


def _terms(X, y, w, W, b, T):
    """(loss terms [n], R [n, K], raw [n, C], prob [n, C]) in the float type T."""
    X, W, b = np.asarray(X).astype(T), np.asarray(W, dtype=np.float64).astype(T), np.asarray(b, np.float64).astype(T)
    n, K = X.shape[0], W.shape[0]
    w = np.ones(n, dtype=T) if w is None else np.asarray(w, dtype=np.float64).astype(T)
    yi = np.asarray(y).astype(np.int64)
    if T is np.longdouble and X.size <= 1 << 16:
        z = np.array([[_fsum(X[r] * W[c]) for c in range(K)] for r in range(n)], dtype=T) + b
    else:
        z = np.cumsum(X[:, None, :] * W[None, :, :], axis=2)[:, :, -1] + b
    if K == 1:
        m = z[:, 0]
        t = np.exp(-np.abs(m))
        p = np.where(m >= 0, T(1), t) / (1 + t)
        return w * (np.log1p(t) + np.maximum(m, 0) - yi * m), (w * (p - yi))[:, None], np.stack([-m, m], 1), \
            np.stack([1 - p, p], 1)
    mx = z.max(1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(1, keepdims=True)
    P = e / s
    oh = (np.arange(K)[None, :] == yi[:, None]).astype(T)
    return w * (mx[:, 0] + np.log(s[:, 0]) - z[np.arange(n), yi]), w[:, None] * (P - oh), z, P


def sums(X, y, w, W, b, T):
    """(loss, grad [K (d + 1)], raw, prob) in fp64 from terms in T: longdouble with exact sums (the reference, which
    also asserts that no two probabilities of a row tie), or float64 summed in row order (the yardstick)."""
    loss, R, raw, prob = _terms(X, y, w, W, b, T)
    XT = np.asarray(X).astype(T)
    tot = _fsum if T is np.longdouble else (lambda v: np.cumsum(v)[-1])
    g = [tot(R[:, c] * XT[:, i]) for c in range(R.shape[1]) for i in range(XT.shape[1])]
    g += [tot(R[:, c]) for c in range(R.shape[1])]
    top = np.sort(prob, axis=1)
    assert T is not np.longdouble or ((top[:, -1] - top[:, -2]) > 64 * ULP).all(), "two probabilities of a row tie"
    return float(tot(loss)), np.array(g, dtype=np.float64), raw.astype(np.float64), prob.astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(d, n, K, weighted):
    """make_data with the reference and yardstick results, computed once and shared (read-only)."""
    X, y, w, W, b = make_data(d, n, K, weighted)
    return dict(X=X, y=y, w=w, W=W, b=b, ref=sums(X, y, w, W, b, np.longdouble), yard=sums(X, y, w, W, b, np.float64))


def check_all(tag, c, out, pr):
    """STEP's (loss, grad, wsum, bad) and PREDICT's (raw, prob, pred), as numpy, against the case's reference."""
    n = c["X"].shape[0]
    assert out[3] == 0 and abs(out[2] - (n if c["w"] is None else c["w"].sum())) <= 1e-12 * n
    for i, (name, got) in enumerate((("loss", out[0]), ("grad", out[1]), ("raw", pr[0]), ("prob", pr[1]))):
        check(f"{tag} {name}", got, c["ref"][i], c["yard"][i])
    assert np.array_equal(pr[2], c["ref"][3].argmax(1))


def exact_case(d, n, C, seed=0):
    """Integer rows in [-8, 8], integer weights in [1, 4], W = 0, b = 0: every P is 1 / C, and the gradient
    sum_r w_r (1 / C - [y_r == c]) x_r is an integer over C (a power of two): exact in fp64, computed here in int64."""
    rng = np.random.default_rng(seed + 31 * d + n + C)
    X = rng.integers(-8, 9, size=(n, d))
    y, w = rng.integers(0, C, size=n), rng.integers(1, 5, size=n)
    A = w[:, None] * (1 - C * (np.arange(C)[None, :] == y[:, None]).astype(np.int64))      # C R, [n, C]
    grad = np.concatenate([(A.T @ X).reshape(-1), A.sum(0)]).astype(np.float64) / C
    return X.astype(np.float32), y.astype(np.float64), w.astype(np.float64), grad
