"""References for ``K.label_stats`` (K27), the univariate tests of ``pyspark.ml.stat`` and the selectors, written
independently of the package code.

* ``count_table``: the exact contingency tables in numpy integers.
* ``class_reference`` / ``regress_reference`` and the ``*_f_reference`` statistics: every term in ``np.longdouble``;
  each sum is ``math.fsum`` over the terms split into a double and the double of what is left, so the sums are exact
  far below fp64 rounding.
* ``class_yardstick`` / ``regress_yardstick``: the same formulas in plain numpy fp64, every sum taken in row order.
* the criterion of tests/_aft_refs.py: the error under test is at most M = 8 times the yardstick's, with a floor of
  4 fp64 ulps (2^-53) of the largest entry for the cases where the yardstick happens to land closer than that.
"""
import functools
import math

import numpy as np

M = 8
ULP = 2.0 ** -53
L = np.longdouble


def _fsum(v):
    """The exact sum of longdouble terms, rounded once: fsum over their double parts and the remainders."""
    v = np.asarray(v, dtype=L).reshape(-1)
    hi = v.astype(np.float64)
    lo = (v - hi.astype(L)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


def _fsum_l(v):
    """The same sum kept in longdouble (double part + the double of the remainder)."""
    v = np.asarray(v, dtype=L).reshape(-1)
    hi = v.astype(np.float64)
    lo = (v - hi.astype(L)).astype(np.float64)
    s = math.fsum(hi.tolist() + lo.tolist())
    r = math.fsum(hi.tolist() + lo.tolist() + [-s])
    return L(s) + L(r)


# ------------------------------------------------------------------------------------------------ data
def make_counts(d, n, K, C, seed=0):
    """(X fp32 [n, d] of category indices below K, codes int32 [n] below C); feature j depends on the label with a
    strength that falls with j."""
    rng = np.random.default_rng(seed + 1000 * d + n + 7 * K + C)
    y = rng.integers(0, C, size=n)
    X = rng.integers(0, K, size=(n, d))
    tied = rng.random(size=(n, d)) < (0.5 / (1 + np.arange(d)))[None, :]
    X = np.where(tied, (y[:, None] + np.arange(d)[None, :]) % K, X)
    return X.astype(np.float32), y.astype(np.int32)


def make_continuous(d, n, C=3, seed=0, dtype=np.float32):
    """(X [n, d], codes int32 [n] below C, y fp64 [n]): feature j's class means and its slope against y fall with j;
    the columns sit at different offsets."""
    rng = np.random.default_rng(seed + 1000 * d + n + C)
    codes = rng.integers(0, C, size=n).astype(np.int32)
    y = rng.normal(size=n) * 2.0 + 5.0
    w = 1.0 / (1 + np.arange(d)) ** 1.5
    X = rng.normal(size=(n, d)) + w[None, :] * ((codes[:, None] - (C - 1) / 2.0) + 0.5 * (y[:, None] - 5.0)) + \
        (np.arange(d) % 5)[None, :] * 3.0
    return X.astype(dtype), codes, y


def shift_of(X, lead=1024):
    """The mean of the leading rows, in fp64: the shift the package passes on one rank."""
    X = np.asarray(X, dtype=np.float64)
    return X[:lead].mean(0) if len(X) else np.zeros(X.shape[1])


# ------------------------------------------------------------------------------------------------ COUNT
def count_table(X, codes, K, C):
    """(table int64 [d, K, C], bad int64 [d], bad_label): a cell is bad when x is non-finite, not an integer, < 0 or
    >= K; a row whose code is outside 0 .. C-1 is skipped and counted in bad_label."""
    X = np.asarray(X, dtype=np.float64)
    codes = np.asarray(codes).astype(np.int64)
    n, d = X.shape
    okl = (codes >= 0) & (codes < C)
    table = np.zeros((d, K, C), dtype=np.int64)
    bad = np.zeros(d, dtype=np.int64)
    for j in range(d):
        x = X[:, j]
        with np.errstate(invalid="ignore"):
            good = np.isfinite(x) & (x >= 0) & (x < K) & (x == np.floor(x)) & okl
        np.add.at(table[j], (x[good].astype(np.int64), codes[good]), 1)
        bad[j] = int((~good & okl).sum())
    return table, bad, int((~okl).sum())


# ------------------------------------------------------------------------------------------------ CLASS
def class_reference(X, codes, C, shift):
    """(sums [C, d], sq [d], n [C]) of (double)x - shift over the rows with a code in 0 .. C-1 and finite cells."""
    X = np.asarray(X, dtype=np.float64)
    codes = np.asarray(codes).astype(np.int64)
    d = X.shape[1]
    sums, sq = np.zeros((C, d)), np.zeros(d)
    okl = (codes >= 0) & (codes < C)
    for j in range(d):
        fin = np.isfinite(X[:, j]) & okl
        v = X[fin, j].astype(L) - L(shift[j])
        sq[j] = _fsum(v * v)
        cj = codes[fin]
        for c in range(C):
            sums[c, j] = _fsum(v[cj == c])
    return sums, sq, np.bincount(codes[okl], minlength=C).astype(np.float64)


def class_yardstick(X, codes, C, shift):
    X = np.asarray(X, dtype=np.float64)
    codes = np.asarray(codes).astype(np.int64)
    okl = (codes >= 0) & (codes < C)
    V = np.where(np.isfinite(X) & okl[:, None], X - np.asarray(shift)[None, :], 0.0)
    sums = np.stack([np.cumsum(np.where((codes == c)[:, None], V, 0.0), axis=0)[-1] for c in range(C)])
    return sums, np.cumsum(V * V, axis=0)[-1], np.bincount(codes[okl], minlength=C).astype(np.float64)


# ------------------------------------------------------------------------------------------------ REGRESS
def regress_reference(X, y, shift, yshift):
    """(sx, sxx, sxy [d], sy, syy, n) over the rows with a finite y, of the finite cells."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    d = X.shape[1]
    oky = np.isfinite(y)
    yy = y[oky].astype(L) - L(yshift)
    sx, sxx, sxy = np.zeros(d), np.zeros(d), np.zeros(d)
    for j in range(d):
        fin = np.isfinite(X[:, j]) & oky
        v = X[fin, j].astype(L) - L(shift[j])
        yj = y[fin].astype(L) - L(yshift)
        sx[j], sxx[j], sxy[j] = _fsum(v), _fsum(v * v), _fsum(v * yj)
    return sx, sxx, sxy, _fsum(yy), _fsum(yy * yy), float(oky.sum())


def regress_yardstick(X, y, shift, yshift):
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    oky = np.isfinite(y)
    yy = np.where(oky, y - yshift, 0.0)
    V = np.where(np.isfinite(X) & oky[:, None], X - np.asarray(shift)[None, :], 0.0)
    return (np.cumsum(V, axis=0)[-1], np.cumsum(V * V, axis=0)[-1], np.cumsum(V * yy[:, None], axis=0)[-1],
            float(np.cumsum(yy)[-1]), float(np.cumsum(yy * yy)[-1]), float(oky.sum()))


# ------------------------------------------------------------------------------------------------ the statistics
def anova_f_reference(X, labels):
    """The one-way ANOVA F per feature in longdouble, from exactly centred values (rounded to fp64 at the end)."""
    X = np.asarray(X, dtype=np.float64)
    labels = np.asarray(labels)
    vals = np.unique(labels)
    n, d = X.shape
    F = np.zeros(d)
    for j in range(d):
        x = X[:, j].astype(L)
        mu = _fsum_l(x) / L(n)
        between, within = L(0), L(0)
        for c in vals:
            xc = x[labels == c]
            mc = _fsum_l(xc) / L(len(xc))
            between += L(len(xc)) * (mc - mu) ** 2
            within += _fsum_l((xc - mc) ** 2)
        F[j] = float((between / L(len(vals) - 1)) / (within / L(n - len(vals))))
    return F


def fvalue_f_reference(X, y):
    """The F-value of the Pearson correlation per feature in longdouble, from exactly centred values."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).astype(L)
    n, d = X.shape
    yc = y - _fsum_l(y) / L(n)
    syy = _fsum_l(yc * yc)
    F = np.zeros(d)
    for j in range(d):
        x = X[:, j].astype(L)
        xc = x - _fsum_l(x) / L(n)
        r2 = _fsum_l(xc * yc) ** 2 / (_fsum_l(xc * xc) * syy)
        F[j] = float(r2 / (L(1) - r2) * L(n - 2))
    return F


def anova_from_sums(sums, sq, nc):
    """Spark's computeANOVA on (shifted) sums in plain fp64: what a yardstick's sums give."""
    n = nc.sum()
    S = sums.sum(0)
    between = (sums ** 2 / nc[:, None]).sum(0) - S ** 2 / n
    within = (sq - S ** 2 / n) - between
    return (between / (len(nc) - 1)) / (within / (n - len(nc)))


def fvalue_from_sums(sx, sxx, sxy, sy, syy, n):
    r = (sxy - sx * sy / n) / np.sqrt((sxx - sx ** 2 / n) * (syy - sy ** 2 / n))
    return r ** 2 / (1.0 - r ** 2) * (n - 2)


def chi2_reference(O):
    """(statistic, df) of a contingency table in longdouble; empty rows and columns are dropped."""
    O = np.asarray(O, dtype=np.float64)
    O = O[O.sum(1) > 0][:, O.sum(0) > 0]
    df = (O.shape[0] - 1) * (O.shape[1] - 1) if O.size else 0
    if df <= 0:
        return 0.0, 0
    Ol = O.astype(L)
    E = np.outer(Ol.sum(1), Ol.sum(0)) / Ol.sum()
    return _fsum((Ol - E) ** 2 / E), int(df)


# ------------------------------------------------------------------------------------------------ selection
def select(p, mode, thr):
    """Spark's selection written as plain loops: the selected feature indices, ascending."""
    p = [float(v) for v in p]
    d = len(p)
    order = sorted(range(d), key=lambda i: (p[i], i))
    if mode == "numTopFeatures":
        sel = order[:int(thr)]
    elif mode == "percentile":
        sel = order[:int(d * thr)]
    elif mode == "fpr":
        sel = [i for i in range(d) if p[i] < thr]
    elif mode == "fwe":
        sel = [i for i in range(d) if p[i] < thr / d]
    else:
        last = -1
        for rank, i in enumerate(order):
            if p[i] <= thr * (rank + 1) / d:
                last = rank
        sel = order[:last + 1]
    return sorted(sel)


# ------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def count_case(d, n, K, C, seed=0):
    X, codes = make_counts(d, n, K, C, seed)
    table, bad, bad_label = count_table(X, codes, K, C)
    return dict(X=X, codes=codes, table=table, bad=bad, bad_label=bad_label)


@functools.lru_cache(maxsize=None)
def cont_case(d, n, C=3, seed=0):
    """make_continuous with a non-zero shift (the leading 16 rows' mean, to two decimals) and the reference and yardstick sums of both modes, computed once and
    shared (read-only)."""
    X, codes, y = make_continuous(d, n, C, seed)
    # near the means but not the means themselves: a sum of exactly centred values is all rounding error, which no
    # criterion relative to the sum can judge
    shift, yshift = np.round(shift_of(X, 16), 2), float(np.round(np.mean(y[:16]), 2))
    return dict(X=X, codes=codes, y=y, shift=shift, yshift=yshift,
                cls=class_reference(X, codes, C, shift), y_cls=class_yardstick(X, codes, C, shift),
                reg=regress_reference(X, y, shift, yshift), y_reg=regress_yardstick(X, y, shift, yshift))


def bound(ref, yard):
    """The largest error allowed against ``ref`` (a scalar or an array: one bound for all its entries)."""
    ref, yard = np.asarray(ref, dtype=np.float64), np.asarray(yard, dtype=np.float64)
    return max(M * float(np.abs(yard - ref).max()), 4 * ULP * float(np.abs(ref).max()))


def check(tag, got, ref, yard):
    """Print the figures, then assert ``got`` within ``bound`` of ``ref``."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, yerr, bd = float(np.abs(got - ref).max()), float(np.abs(np.asarray(yard) - ref).max()), bound(ref, yard)
    scale = max(float(np.abs(ref).max()), 1e-300)
    print(f"select {tag}: error / max {err / scale:.2e} yardstick {yerr / scale:.2e} bound {bd / scale:.2e} "
          f"ratio {err / yerr if yerr > 0 else (0.0 if err == 0 else float('inf')):.2f}")
    assert np.isfinite(got).all() and err <= bd, (tag, err, bd)


def check_class(tag, got, ref, yard):
    """``got``: label_stats' LABEL_CLASS dict as numpy; the counts exactly, the sums to the criterion."""
    check(tag + " sums", got["sums"], ref[0], yard[0])
    check(tag + " sq", got["sq"], ref[1], yard[1])
    assert np.array_equal(got["n"], ref[2]), tag


def check_regress(tag, got, ref, yard):
    for i, k in enumerate(("sx", "sxx", "sxy", "sy", "syy")):
        check(f"{tag} {k}", got[k], ref[i], yard[i])
    assert float(got["n"]) == ref[5], tag
