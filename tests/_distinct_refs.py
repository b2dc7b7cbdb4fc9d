"""Plain numpy references for K29 and VectorIndexer on the fp64 image of fp32 inputs: ``np.unique`` per column with the
zero rule, a dict lookup for the recode.  Everything is exact: every comparison is equality (of bits for floats)."""
import functools

import numpy as np

# the kinds of columns a case cycles through, from a kind that depends on the case (d = 1 and 5 cannot hold them all)
KINDS = ("exact_cap", "cap_plus_1", "last_row", "other_half", "split", "zeros", "no_zero", "neg_inf", "nans", "const",
         "gauss")
FIXED = {"zeros": [-0.0, 0.0, 1.0], "no_zero": [3.0, 5.0], "neg_inf": [-np.inf, np.inf, -1.5],
         "nans": [np.nan, 1.0, 2.0], "const": [7.25]}


def spread(k, n, rng, shift=0):
    """n draws of k distinct fp32 values around zero (or of the list k) in which every value occurs if n allows."""
    values = np.asarray(k if isinstance(k, list) else (np.arange(k) - k // 3 + shift) * 1.5, dtype=np.float32)
    x = rng.choice(values, size=n)
    m = min(len(values), n)
    x[rng.permutation(n)[:m]] = values[:m]
    return x


def column(kind, n, cap, rng):
    if kind in FIXED:
        return spread(FIXED[kind], n, rng)
    if kind == "gauss":
        return rng.normal(size=n).astype(np.float32)
    if kind in ("exact_cap", "cap_plus_1"):     # comes out categorical / continuous (when n > cap)
        return spread(cap + (kind == "cap_plus_1"), n, rng)
    if kind == "split":                         # every block within cap, the union of two blocks not
        rpb = -(-(-(-n // -(-n // 1024))) // 64) * 64       # the kernels' rows per block
        return np.concatenate([spread(cap, min(n, rpb), rng), spread(cap, max(n - rpb, 0), rng, shift=1)])
    x = spread(cap - 1, n, rng)
    if kind == "last_row":                      # a value that first appears in the last row
        x[-1] = 77.0
    else:                                       # other_half: a value that only rows 32 .. 63 of the first tile see
        x[40:41] = -55.0
        x[32:64][rng.random(len(x[32:64])) < 0.5] = -55.0
    return x


def distinct(X, cap):
    """values f64 [d, cap + 1] (NaN from the count on, and for more than cap values), count, nan."""
    d = X.shape[1]
    values = np.full((d, cap + 1), np.nan)
    count, nan = np.zeros(d, dtype=np.int64), np.zeros(d, dtype=np.int64)
    for c in range(d):
        v = X[:, c].astype(np.float64)
        nan[c] = np.isnan(v).sum()
        u = np.unique(v[~np.isnan(v)]) + 0.0        # -0.0 and +0.0 are one value, +0.0
        count[c] = min(len(u), cap + 1)
        if len(u) <= cap:
            values[c, :len(u)] = u
    return {"values": values, "count": count, "nan": nan}


def category_maps(ref, cap):
    """{feature: {value: index}}: ascending, 0.0 first when present (Spark's getCategoryMaps)."""
    maps = {}
    for c, m in enumerate(ref["count"].tolist()):
        if 1 <= m <= cap:
            vals = ref["values"][c, :m].tolist()
            maps[c] = {v: i for i, v in enumerate(([0.0] if 0.0 in vals else []) + [v for v in vals if v != 0.0])}
    return maps


def recode(X, maps):
    """{mode: (Y fp32, bad [d], drop [n] or None)}: what ``K.col_recode`` returns for X under the three modes."""
    n, d = X.shape
    idx = np.zeros((n, d), dtype=np.int64)
    for c, m in maps.items():
        idx[:, c] = [m.get(v, -1) for v in X[:, c].astype(np.float64).tolist()]
    cat = np.isin(np.arange(d), list(maps))[None, :]
    ncat = np.array([len(maps.get(c, ())) for c in range(d)], dtype=np.float32)[None, :]
    miss = cat & (idx < 0)
    Y, bad = np.where(cat & (idx >= 0), idx.astype(np.float32), X), miss.sum(0)
    return {"error": (Y, bad, None), "skip": (Y, bad, miss.any(1)), "keep": (np.where(miss, ncat, Y), bad, None)}


@functools.lru_cache(maxsize=None)
def reference(n, d, cap):
    """What the tests of one case share: X fp32 [n, d], the fit reference, the transform input (X with an unseen value
    and a NaN in every categorical column, where there are rows for them) and its recode."""
    rng = np.random.default_rng(97 * n + 13 * d + cap)
    X = np.stack([column(KINDS[(c + n + cap) % len(KINDS)], n, cap, rng) for c in range(d)], 1).astype(np.float32)
    ref, X2 = distinct(X, cap), X.copy()
    maps = category_maps(ref, cap)
    for c in maps:
        rows = rng.permutation(n)[:2]
        X2[rows[:1], c], X2[rows[1:], c] = 1234.5, np.nan
    return X, ref, X2, recode(X2, maps)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_distinct(got, ref, dtype=np.float32):
    """The result of ``K.col_distinct`` equals the reference, bit for bit (free slots hold the default NaN)."""
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert np.array_equal(got["count"], ref["count"]) and np.array_equal(got["nan"], ref["nan"])
    assert got["values"].dtype == dtype and np.array_equal(bits(got["values"]), bits(ref["values"].astype(dtype)))


def assert_recode(got, want, dtype=np.float32):
    """(Y, bad, drop) of ``K.col_recode`` for one mode equals ``recode``'s."""
    Y, bad, drop = (None if t is None else t.cpu().numpy() for t in got)
    assert Y.dtype == dtype and np.array_equal(bits(Y), bits(want[0].astype(dtype))) and np.array_equal(bad, want[1])
    assert (drop is None) if want[2] is None else np.array_equal(drop, want[2])
