"""Independent references for ``K.margin_step`` (K32): longdouble reference, fp64 yardstick, ``_aft_refs``' criterion."""
import functools

import numpy as np

from tests._aft_refs import _fsum, check  # noqa: F401  (check: the criterion, used by the tests)

HINGE, HUBER = 0, 1
SIGMA, EPS = 0.7, 1.35


def evaluate(X, y, w, coef, b, loss, sigma=SIGMA, eps=EPS, keep=None, exact=True):
    """(loss sum, [sum u x | sum u | sum v], sum w, margins [n]) over the rows of ``keep`` (all)."""
    F = np.longdouble if exact else np.float64
    X, y, coef = np.asarray(X).astype(F), np.asarray(y, np.float64).astype(F), np.asarray(coef, np.float64).astype(F)
    w = np.ones(len(y), dtype=F) if w is None else np.asarray(w, np.float64).astype(F)
    total = _fsum if exact else (lambda v: float(np.cumsum(v)[-1]) if len(v) else 0.0)
    sigma, eps = F(sigma), F(eps)
    m = (np.array([_fsum(r * coef) for r in X], dtype=F) if exact else np.cumsum(X * coef, axis=1)[:, -1]) + F(b)
    Xs, ys, ws, ms = [a[slice(None) if keep is None else np.asarray(keep)] for a in (X, y, w, m)]
    if loss == HINGE:
        s = 2 * ys - 1
        t = 1 - s * ms
        ls, u, v = np.where(t > 0, ws * t * t, 0), np.where(t > 0, -2 * ws * s * t, 0), np.zeros_like(ms)
    else:
        r = ys - ms
        quad = np.abs(r) <= eps * sigma
        ls = ws * np.where(quad, sigma + r * r / sigma, sigma + 2 * eps * np.abs(r) - sigma * eps * eps) / 2
        u = np.where(quad, -ws * r / sigma, -ws * eps * np.sign(r))
        v = ws * np.where(quad, 1 - (r / sigma) ** 2, 1 - eps * eps) / 2
    grad = [total(u * Xs[:, i]) for i in range(X.shape[1])] + [total(u), total(v)]
    return total(ls), np.array(grad, dtype=np.float64), total(ws), m.astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(d, n, loss, weighted):
    """fp32 rows, 0 / 1 labels (hinge) or a linear label with 10 % gross outliers (Huber), a point near the generating
    one (every branch of both tops is populated), the reference and the yardstick; computed once and shared."""
    rng = np.random.default_rng(1000 * d + n)
    X = rng.normal(size=(n, d)).astype(np.float32)
    beta = rng.normal(scale=1.0 / np.sqrt(d), size=d)
    y = X.astype(np.float64) @ beta + 0.5 + rng.normal(scale=0.5, size=n)
    y = (y > 0.5).astype(np.float64) if loss == HINGE else y + rng.choice([-20.0, 20.0], n) * (rng.random(n) < 0.1)
    w = rng.uniform(0.25, 2.0, size=n) if weighted else None
    coef, b = beta + rng.normal(scale=0.3 / np.sqrt(d), size=d), 0.7
    return dict(X=X, y=y, w=w, coef=coef, b=b, ref=evaluate(X, y, w, coef, b, loss),
                yard=evaluate(X, y, w, coef, b, loss, exact=False))


def edge_case(loss, n=130):
    """Exact dyadic inputs (integer X, dyadic coef and weights, sigma = 0.5, epsilon = 1.5: fp64 sums are exact in any
    order) with rows on the branch boundaries, 1 - s m == 0 or |r| == epsilon sigma, beside rows of every other
    branch.  Returns the case and the boundary rows' mask."""
    rng = np.random.default_rng(5 + loss)
    X = rng.integers(-2, 3, size=(n, 4)).astype(np.float32)
    X[0::8], X[4::8] = [1, 0, 0, 0], [-1, 0, -1, 0]          # m == 1 and m == -1
    coef, b = np.array([0.5, -0.25, 1.0, 0.75]), 0.5
    m = X.astype(np.float64) @ coef + b
    if loss == HINGE:
        y = rng.integers(0, 2, size=n).astype(np.float64)
        y[m == 1.0], y[m == -1.0] = 1.0, 0.0
        edge = np.abs(m) == 1.0
    else:
        r = np.resize([0.25, 0.75, -0.75, 2.0, -3.0], n)
        y, edge = m + r, np.abs(r) == 0.75
    assert 4 <= edge[:64].sum() < 60          # boundary and other rows share the first tile
    return dict(X=X, y=y, w=rng.choice([0.5, 1.0, 2.0], size=n), coef=coef, b=b, sigma=0.5, eps=1.5), edge


def plant_bad(c, loss, rows):
    """X, y, w with a NaN and an inf feature, a NaN weight and the labels 0.5 and 2 (hinge) or inf (Huber) at rows."""
    X, y, w = c["X"].copy(), c["y"].copy(), c["w"].copy()
    X[rows[0], -1], X[rows[1], 0], w[rows[2]] = np.nan, np.inf, np.nan
    y[rows[3:]] = [0.5, 2.0] if loss == HINGE else [np.inf]
    return X, y, w
