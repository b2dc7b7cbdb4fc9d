"""Plain numpy references for the K28 radix select (``K.col_digit_hist``, ``K.col_quantiles``) and the scalers on it.

The key map, ``np.sort`` of each column's keys without the NaNs, the rank rule r = min(max(ceil(q m), 1), m) with the
product in fp64, and back to float.  Results are compared as bit patterns (``bits``), so -0.0 != +0.0 and the exact
NaN placement are checked.
"""
import math

import numpy as np

# the kinds of columns a case cycles through
MENU = ("gauss", "const", "two", "onehot", "allnan", "nan30", "inf", "zeros", "denormal", "lowbit", "sign", "big")


def column(kind, n, rng):
    """n fp32 values of one kind of the menu."""
    if kind == "gauss":
        return rng.normal(size=n).astype(np.float32)
    if kind == "const":
        return np.full(n, 3.25, dtype=np.float32)
    if kind == "two":
        return rng.choice(np.array([-1.5, 7.0], dtype=np.float32), size=n)
    if kind == "onehot":
        return (rng.random(n) < 0.3).astype(np.float32)
    if kind == "allnan":
        return np.full(n, np.nan, dtype=np.float32)
    if kind == "nan30":        # 30 % NaN, of both signs
        x = rng.normal(size=n).astype(np.float32).view(np.uint32)
        r = rng.random(n)
        x[r < 0.15] = 0x7FC00000
        x[(r >= 0.15) & (r < 0.30)] = 0xFFC00001
        return x.view(np.float32)
    if kind == "inf":
        x = rng.normal(size=n).astype(np.float32)
        r = rng.random(n)
        x[r < 0.2] = np.inf
        x[r > 0.8] = -np.inf
        return x
    if kind == "zeros":        # both zeros
        return np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    if kind == "denormal":
        u = rng.integers(1, 1 << 23, size=n).astype(np.uint32) | (rng.integers(0, 2, size=n).astype(np.uint32) << 31)
        return u.view(np.float32)
    if kind == "lowbit":       # values that differ only in the lowest mantissa bit: the last pass decides
        return (np.float32(1.7).view(np.uint32) & ~np.uint32(1) | rng.integers(0, 2, size=n).astype(np.uint32)) \
            .view(np.float32)
    if kind == "sign":         # values that differ only in sign
        return np.where(rng.random(n) < 0.5, np.float32(-2.5), np.float32(2.5)).astype(np.float32)
    if kind == "big":          # large integers near 2^24
        return (float(1 << 24) + rng.integers(-4, 5, size=n)).astype(np.float32)
    raise ValueError(kind)


def menu_case(d, n, seed=7, kinds=None):
    """X fp32 [n, d] whose columns cycle through ``kinds`` (the whole menu by default)."""
    rng = np.random.default_rng(seed + 1000 * d + n)
    kinds = MENU if kinds is None else kinds
    X = np.empty((n, d), dtype=np.float32)
    for c in range(d):
        X[:, c] = column(kinds[c % len(kinds)], n, rng)
    return X


def fine_case64(d, n, seed=11):
    """fp64 [n, d] whose values differ only below fp32 precision (all equal after a cast to fp32), of both signs, with
    a NaN column when d > 2."""
    rng = np.random.default_rng(seed + 1000 * d + n)
    X = 1.0 + rng.integers(0, 1 << 20, size=(n, d)).astype(np.float64) * 2.0 ** -50
    X[:, 1::3] *= -1.0
    if d > 2:
        X[:, 2] = np.nan
    assert np.unique(X[:, 0].astype(np.float32)).size == 1
    return X


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def keys_of(x):
    """The order-preserving unsigned keys of fp32 / fp64 values (NaNs included: mask them out first)."""
    u = bits(x)
    if u.dtype == np.uint32:
        return u ^ np.where(u >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    return u ^ np.where(u >> np.uint64(63) != 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1 << 63))


def values_of(k, dtype):
    if k.dtype == np.uint32:
        u = k ^ np.where(k >> np.uint32(31) != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))
    else:
        u = k ^ np.where(k >> np.uint64(63) != 0, np.uint64(1 << 63), np.uint64(0xFFFFFFFFFFFFFFFF))
    return u.view(dtype)


def rank_of(q, m):
    """The 1-based rank of probability q among m values; 0 when m = 0."""
    return min(max(math.ceil(float(q) * float(m)), 1), m)


def quantiles(X, probs):
    """{"q" [Q, d], "count", "nan" int64 [d], "min", "max" [d]} of X fp32 / fp64 [n, d] by sorting the keys."""
    n, d = X.shape
    q = np.full((len(probs), d), np.nan, dtype=X.dtype)
    lo, hi = np.full(d, np.nan, dtype=X.dtype), np.full(d, np.nan, dtype=X.dtype)
    count, nan = np.zeros(d, dtype=np.int64), np.zeros(d, dtype=np.int64)
    for c in range(d):
        x = np.ascontiguousarray(X[:, c])
        ok = ~np.isnan(x)
        k = np.sort(keys_of(x[ok]))
        m = count[c] = k.size
        nan[c] = n - m
        if m == 0:
            continue
        v = values_of(k, X.dtype)
        lo[c], hi[c] = v[0], v[-1]
        for t, p in enumerate(probs):
            q[t, c] = v[rank_of(p, m) - 1]
    return {"q": q, "count": count, "nan": nan, "min": lo, "max": hi}


def digit_hist(X, nbits, shift, prefix=None):
    """The pass's counts by ``np.bincount``: {"hist" int64 [d, Q', 2^nbits]} and in FIRST mode (prefix None) "nan",
    "kmin", "kmax" int64 [d] (2^32 - 1 / 0 for a column without a value).  fp32 X; prefix integer [d, Q]."""
    n, d = X.shape
    nd = 1 << nbits
    first = prefix is None
    Q = 1 if first else prefix.shape[1]
    hist = np.zeros((d, Q, nd), dtype=np.int64)
    nan, kmin, kmax = np.zeros(d, np.int64), np.full(d, (1 << 32) - 1, np.int64), np.zeros(d, np.int64)
    for c in range(d):
        x = np.ascontiguousarray(X[:, c])
        ok = ~np.isnan(x)
        k = keys_of(x[ok]).astype(np.int64)
        digit = (k >> shift) & (nd - 1)
        nan[c] = n - k.size
        if first:
            hist[c, 0] = np.bincount(digit, minlength=nd)
            if k.size:
                kmin[c], kmax[c] = k.min(), k.max()
            continue
        hi = k >> (shift + nbits)
        for t in range(Q):
            hist[c, t] = np.bincount(digit[hi == int(prefix[c, t])], minlength=nd)
    out = {"hist": hist}
    if first:
        out.update(nan=nan, kmin=kmin, kmax=kmax)
    return out


def prefixes(X, probs, width):
    """int64 [d, Q]: the top ``width`` key bits of the reference quantiles of fp32 X -- what the select steps have
    found after passes that took ``width`` bits (0 for a column without a value)."""
    q = quantiles(X, probs)["q"]
    k = keys_of(np.ascontiguousarray(q.T)).astype(np.int64) >> (32 - width)
    return np.where(np.isnan(q.T), 0, k)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def assert_quantiles(got, ref):
    """``got``: a ``K.col_quantiles`` result as numpy arrays."""
    for k in ("q", "min", "max"):
        assert same_bits(got[k], ref[k]), (k, got[k], ref[k])
    for k in ("count", "nan"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])


def robust_reference(X, lower=0.25, upper=0.75):
    """(median, range) fp64 [d] as RobustScaler fits them."""
    q = quantiles(X, [lower, 0.5, upper])["q"].astype(np.float64)
    return q[1], q[2] - q[0]


def max_abs_reference(X):
    r = quantiles(X, [0.5])
    m = np.maximum(np.abs(r["min"].astype(np.float64)), np.abs(r["max"].astype(np.float64)))
    return np.where(r["count"] > 0, m, 0.0)
