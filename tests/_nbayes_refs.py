"""References for ``K.nb_step`` (K34) and NaiveBayes, written independently of the package code.

STATS: W_c = sum w, S_c = sum w x, Q_c = sum w x^2 over the rows of label c; on integer data they are int64 sums.
PREDICT: ``scores`` in ``np.longdouble`` (the reference) and in plain numpy fp64 (the yardstick); the criterion is
``_aft_refs.check`` (8 x the yardstick's error, floor 4 ulps of the largest).  ``params``: Spark's closed forms.
"""
import functools

import numpy as np

from tests._aft_refs import bound

TYPES = ("multinomial", "complement", "bernoulli", "gaussian")


def exact_case(d, n, C, seed=0):
    """(X fp32 with integers in [0, 7], y covering every class, integer weights in [0, 4], S, Q, W in int64)."""
    rng = np.random.default_rng(seed + 31 * d + n + C)
    X = rng.integers(0, 8, size=(n, d))
    y, w = np.arange(n) % C if n >= C else rng.integers(0, C, size=n), rng.integers(0, 5, size=n)
    y = rng.permutation(y)
    R = w[:, None] * (np.arange(C)[None, :] == y[:, None]).astype(np.int64)
    return X.astype(np.float32), y.astype(np.float64), w.astype(np.float64), R.T @ X, R.T @ (X * X), R.sum(0)


def make_data(mt, d, n, C, seed=0):
    """(X fp32, y) for a model type: counts, 0 / 1 values, or Gaussian rows at a mean offset of 1e3 drawn with
    |x - mu| <= 6 sqrt(sigma)."""
    rng = np.random.default_rng(seed + 1000 * d + 10 * n + C + len(mt))
    y = rng.permutation(np.arange(n) % C) if n >= C else rng.integers(0, C, size=n)
    if mt == "gaussian":
        mu = 1e3 + rng.normal(scale=1.0, size=(C, d))
        sd = rng.uniform(0.5, 1.5, size=(C, d))
        X = mu[y] + sd[y] * np.clip(rng.normal(size=(n, d)), -6, 6)
    else:
        p = rng.dirichlet(np.ones(d) * 0.5, size=C) if d > 1 else np.full((C, 1), 0.5)
        lam = 4.0 + 40.0 * p[y] * d
        X = rng.poisson(lam)
        if mt == "bernoulli":
            X = (rng.uniform(size=(n, d)) < 0.1 + 0.8 * rng.uniform(size=(C, d))[y]).astype(np.int64)
    return X.astype(np.float32), y.astype(np.float64)


def params(mt, X, y, w, C, lam=1.0):
    """(pi, theta, sigma or None): Spark's closed forms in fp64 numpy from longdouble sums about the column mean."""
    X, yi = np.asarray(X).astype(np.longdouble), np.asarray(y).astype(np.int64)
    n, d = X.shape
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    R = (w[:, None] * (np.arange(C)[None, :] == yi[:, None])).astype(np.longdouble)
    W, S = R.sum(0).astype(np.float64), (R.T @ X).astype(np.float64)
    pi = np.log(W + lam) - np.log(W.sum() + C * lam)
    if mt == "multinomial":
        return pi, np.log(S + lam) - np.log(S.sum(1, keepdims=True) + d * lam), None
    if mt == "bernoulli":
        return pi, np.log(S + lam) - np.log(W[:, None] + 2 * lam), None
    if mt == "complement":
        comp = S.sum(0, keepdims=True) - S + lam
        return pi, np.log(comp.sum(1, keepdims=True)) - np.log(comp), None
    Wd = np.maximum(W, 1.0)[:, None].astype(np.longdouble)
    mu = (R.T @ X) / Wd
    var = (np.stack([(R[:, c:c + 1] * (X - mu[c]) ** 2).sum(0) for c in range(C)]) / Wd).astype(np.float64)
    return pi, mu.astype(np.float64), np.maximum(var, 1e-9) + 1e-9 * var.max()


def scores(mt, X, pi, theta, sigma, T):
    """(raw [n, C], prob [n, C]) of a model in the float type T."""
    X, pi, th = np.asarray(X).astype(T), np.asarray(pi).astype(T), np.asarray(theta).astype(T)
    if mt == "multinomial":
        raw = X @ th.T + pi
    elif mt == "complement":
        raw = X @ th.T
    elif mt == "bernoulli":
        neg = np.log1p(-np.minimum(np.exp(th), T(1) - T(1e-12)))
        raw = X @ (th - neg).T + neg.sum(1) + pi
    else:
        sg = np.asarray(sigma).astype(T)
        raw = pi - (((X[:, None, :] - th[None]) ** 2) / sg[None] + np.log(2 * T(np.pi) * sg[None])).sum(2) / 2
    e = np.exp(raw - raw.max(1, keepdims=True))
    return raw, e / e.sum(1, keepdims=True)


@functools.lru_cache(maxsize=None)
def case(mt, d, n, C):
    """A model fitted by ``params`` on ``make_data`` with its reference and yardstick scores, computed once and
    shared (read-only).  ``sure``: the rows whose two largest reference probabilities differ by more than the
    criterion's bound; the others (fewer than 1 %) are exempt from the comparison of the predictions."""
    X, y = make_data(mt, d, n, C)
    pi, th, sg = params(mt, X, y, None, C)
    ref = [a.astype(np.float64) for a in scores(mt, X, pi, th, sg, np.longdouble)]
    yard = scores(mt, X, pi, th, sg, np.float64)
    top = np.sort(ref[1], axis=1)
    sure = (top[:, -1] - top[:, -2]) > bound(ref[1], yard[1])
    assert (~sure).mean() < 0.01, (~sure).mean()
    return dict(X=X, y=y, pi=pi, theta=th, sigma=sg, ref=ref, yard=yard, sure=sure)


def plant(X, y, C, bad_value):
    """(X, y, w, clean rows mask, expected [non-finite, rule, label or weight] counts) with the bad rows planted;
    ``bad_value`` breaks the pass's value rule (None: FINITE has none)."""
    X, y, w = X.copy(), y.copy(), np.ones(len(y))
    X[3, 0], X[17, -1], y[40], y[41], w[50], w[51] = np.nan, np.inf, 2.5, C, np.nan, -1.0
    rows = [3, 17, 40, 41, 50, 51]
    if bad_value is not None:
        X[29, X.shape[1] // 2] = bad_value
        rows.append(29)
    return X, y, w, ~np.isin(np.arange(len(y)), rows), [2, int(bad_value is not None), 4]
