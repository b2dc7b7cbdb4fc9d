"""References for ``K.aft_step`` (K26) and AFTSurvivalRegression, written independently of the package code.

The model is Spark's Weibull accelerated failure time model.  Per row, with eps = (log t - x.beta - b) / sigma:
loss = delta log sigma - delta eps + e^eps, m = (delta - e^eps) / sigma, and the gradient terms are m x (beta), m (b)
and delta + (delta - e^eps) eps (log sigma).  predict = exp(x.beta + b), quantile_p = predict exp(sigma log(-log(1-p))).

* ``reference``: every row's terms in ``np.longdouble``; each sum is ``math.fsum`` over the terms split into a double
  and the double of what is left, so the sums are exact far below fp64 rounding.
* ``yardstick``: the same formulas in plain numpy fp64, every sum taken in row (or column) order.
* the criterion of the K24 / K25 tests: the error under test is at most M = 8 times the yardstick's, with a floor of
  4 fp64 ulps (2^-53) of the largest entry for the cases where the yardstick happens to land closer than that.
"""
import functools
import math

import numpy as np

M = 8
ULP = 2.0 ** -53
SIGMA = 0.7
PROBS = [0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99]      # Spark's default quantileProbabilities


def make_data(d, n, seed=0, dtype=np.float32):
    """(X, t, censor, beta, b): standard-normal rows, Weibull AFT times log T = x.beta + b + SIGMA log(Exp(1)), and an
    independent exponential censoring time; t = min(T, C), censor = [T <= C] (1: the event occurred)."""
    rng = np.random.default_rng(seed + 1000 * d + n)
    X = rng.normal(size=(n, d)).astype(dtype)
    beta = rng.normal(scale=0.5 / np.sqrt(d), size=d)
    b = 1.0
    logT = X.astype(np.float64) @ beta + b + SIGMA * np.log(rng.exponential(size=n))
    C = rng.exponential(scale=2.5 * np.exp(b), size=n)
    T = np.exp(logT)
    return X, np.minimum(T, C), (T <= C).astype(np.float64), beta, b


def _fsum(v):
    """The exact sum of longdouble terms, rounded once: fsum over their double parts and the remainders."""
    v = np.asarray(v, dtype=np.longdouble).reshape(-1)
    hi = v.astype(np.float64)
    lo = (v - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


def reference(X, t, censor, coef, b, log_sigma, probs=PROBS, keep=None):
    """(loss sum, gradient sums [d + 2], predictions [n], quantiles [n, Q]) over the rows of ``keep`` (all); the
    predictions and quantiles for every row."""
    L = np.longdouble
    X = np.asarray(X).astype(L)
    coef = np.asarray(coef, dtype=np.float64).astype(L)
    b, ls = L(b), L(log_sigma)
    sigma = np.exp(ls)
    n, d = X.shape
    dot = np.array([_fsum(X[r] * coef) for r in range(n)], dtype=L) if d * n <= 4096 else X @ coef
    pred = np.exp(dot + b)
    qf = np.exp(L(math.exp(float(log_sigma))) * np.log(-np.log1p(-np.asarray(probs, dtype=np.float64).astype(L))))
    quant = pred[:, None] * qf[None, :]
    sel = slice(None) if keep is None else np.asarray(keep)
    with np.errstate(divide="ignore", invalid="ignore"):
        lt = np.log(np.asarray(t, dtype=np.float64).astype(L))
    dl = np.asarray(censor, dtype=np.float64).astype(L)
    Xs, lt, dl, dot = X[sel], lt[sel], dl[sel], dot[sel]
    eps = (lt - dot - b) / sigma
    ee = np.exp(eps)
    m = (dl - ee) / sigma
    grad = [_fsum(m * Xs[:, i]) for i in range(d)] + [_fsum(m), _fsum(dl + (dl - ee) * eps)]
    return _fsum(dl * ls - dl * eps + ee), np.array(grad), pred.astype(np.float64), quant.astype(np.float64)


def yardstick(X, t, censor, coef, b, log_sigma, probs=PROBS, keep=None):
    """The same quantities in plain numpy fp64; x.beta summed in column order, the row sums in row order."""
    X = np.asarray(X, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    sigma = np.exp(log_sigma)
    d = X.shape[1]
    dot = np.cumsum(X * coef, axis=1)[:, -1]
    pred = np.exp(dot + b)
    quant = pred[:, None] * np.exp(sigma * np.log(-np.log1p(-np.asarray(probs, dtype=np.float64))))[None, :]
    sel = slice(None) if keep is None else np.asarray(keep)
    with np.errstate(divide="ignore", invalid="ignore"):
        lt = np.log(np.asarray(t, dtype=np.float64))
    dl = np.asarray(censor, dtype=np.float64)
    Xs, lt, dl, dot = X[sel], lt[sel], dl[sel], dot[sel]
    if Xs.shape[0] == 0:
        return 0.0, np.zeros(d + 2), pred, quant
    eps = (lt - dot - b) / sigma
    ee = np.exp(eps)
    m = (dl - ee) / sigma
    grad = np.concatenate([np.cumsum(m[:, None] * Xs, axis=0)[-1], [np.cumsum(m)[-1]],
                           [np.cumsum(dl + (dl - ee) * eps)[-1]]])
    return float(np.cumsum(dl * log_sigma - dl * eps + ee)[-1]), grad, pred, quant


def point(d, beta, b, seed=0):
    """A parameter point near the generating one, not the optimum: (coef, intercept, log sigma)."""
    rng = np.random.default_rng(77 + seed + d)
    return beta + rng.normal(scale=0.3 / np.sqrt(d), size=d), b + 0.2, math.log(SIGMA) + 0.15


@functools.lru_cache(maxsize=None)
def case(d, n, seed=0):
    """make_data and point with the reference and yardstick results, computed once and shared (read-only)."""
    X, t, censor, beta, b = make_data(d, n, seed)
    coef, b0, ls = point(d, beta, b, seed)
    loss, grad, pred, quant = reference(X, t, censor, coef, b0, ls)
    yl, yg, yp, yq = yardstick(X, t, censor, coef, b0, ls)
    return dict(X=X, t=t, logt=np.log(t), censor=censor, beta=beta, b=b, coef=coef, b0=b0, ls=ls, loss=loss,
                grad=grad, pred=pred, quant=quant, y_loss=yl, y_grad=yg, y_pred=yp, y_quant=yq)


def bound(ref, yard):
    """The largest error allowed against ``ref`` (a scalar or an array: one bound for all its entries)."""
    ref, yard = np.asarray(ref, dtype=np.float64), np.asarray(yard, dtype=np.float64)
    return max(M * float(np.abs(yard - ref).max()), 4 * ULP * float(np.abs(ref).max()))


def check(tag, got, ref, yard):
    """Print the figures, then assert ``got`` within ``bound`` of ``ref``."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, yerr, bd = float(np.abs(got - ref).max()), float(np.abs(np.asarray(yard) - ref).max()), bound(ref, yard)
    scale = max(float(np.abs(ref).max()), 1e-300)
    print(f"aft {tag}: error / max {err / scale:.2e} yardstick {yerr / scale:.2e} bound {bd / scale:.2e} "
          f"ratio {err / yerr if yerr > 0 else (0.0 if err == 0 else float('inf')):.2f}")
    assert np.isfinite(got).all() and err <= bd, (tag, err, bd)


def objective(theta, X, logt, censor, fit_intercept=True):
    """(mean loss, gradient) at theta = [beta (d), b, log sigma] in plain numpy fp64: what scipy minimises."""
    d = X.shape[1]
    b = theta[d] if fit_intercept else 0.0
    sigma = np.exp(theta[d + 1])
    eps = (logt - X @ theta[:d] - b) / sigma
    ee = np.exp(eps)
    m = (censor - ee) / sigma
    g = np.concatenate([X.T @ m, [m.sum() if fit_intercept else 0.0], [(censor + (censor - ee) * eps).sum()]])
    return float((censor * theta[d + 1] - censor * eps + ee).sum()) / len(logt), g / len(logt)


def scipy_fit(X, t, censor, fit_intercept=True):
    """The minimiser of ``objective`` from the all-zero point by scipy's L-BFGS-B."""
    from scipy.optimize import minimize
    X = np.asarray(X, dtype=np.float64)
    res = minimize(objective, np.zeros(X.shape[1] + 2), args=(X, np.log(t), np.asarray(censor, np.float64),
                                                             fit_intercept),
                   method="L-BFGS-B", jac=True, options=dict(ftol=1e-16, gtol=1e-11, maxiter=2000, maxfun=5000))
    return res.x, res.fun
