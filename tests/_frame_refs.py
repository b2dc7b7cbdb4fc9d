"""Plain references for the DataFrame kernels K18 to K20 (expr.hip, relational.hip): numpy, Python int / float /
fractions, and mpmath when it can be imported.  Nothing here imports the package, and nothing is written from
``fused.interpret``: every rule is Spark's (non-ANSI) rule for the operation, stated where it is implemented.

A column is a pair ``(values, valid)``: ``valid`` is a bool array, ``values`` is float64 for double / float /
boolean columns (booleans as 0.0 / 1.0) and int64 for int / long columns, so a long keeps all 64 bits.  The
value of a null row is unspecified; comparisons go through ``same`` which looks at valid rows only."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

try:
    import mpmath
except ImportError:  # the tests then use np.longdouble (64-bit mantissa on x86) for the transcendentals
    mpmath = None

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

# the edge table of the tests (None is a null)
EDGES = [0.0, -0.0, 0.5, -0.5, 0.49999999999999994, 1.0, -1.0, 2.5, -2.5, 2.0 ** 31 - 0.5, 2.0 ** 31, 3e10, -3e10,
         2.0 ** 52 + 1, 2.0 ** 53, 2.0 ** 63, 1e19, -1e19, 1e308, 5e-324, math.inf, -math.inf, math.nan, None]


def column(items):
    """(values fp64, valid) of a list of floats with None for null (null rows hold 0.0)."""
    return (np.array([0.0 if x is None else x for x in items], dtype=np.float64),
            np.array([x is not None for x in items], dtype=bool))


def edge_pairs():
    """All ordered pairs of the edge table as two columns."""
    a = [x for x in EDGES for _ in EDGES]
    b = [y for _ in EDGES for y in EDGES]
    return column(a), column(b)


def _f(a):
    """The fp64 view of a column's values (long -> double is Java l2d: round to nearest)."""
    return a[0].astype(np.float64)


# ------------------------------------------------------------------------------------------ arithmetic
def _arith(f):
    def op(a, b):
        with np.errstate(all="ignore"):
            return f(_f(a), _f(b)), a[1] & b[1]
    return op


add, sub, mul = _arith(np.add), _arith(np.subtract), _arith(np.multiply)


def div(a, b):
    """Spark: x / 0 is null (also 0 / 0 and inf / 0); everything else is IEEE."""
    x, y = _f(a), _f(b)
    with np.errstate(all="ignore"):
        return x / np.where(y == 0, 1.0, y), a[1] & b[1] & (y != 0)


def mod(a, b):
    """Spark: x % 0 is null; otherwise Java's %, which is C fmod (sign of the dividend)."""
    x, y = _f(a), _f(b)
    v = np.array([math.nan if (yy == 0 or math.isinf(xx) or xx != xx or yy != yy) else math.fmod(xx, yy)
                  for xx, yy in zip(x.tolist(), y.tolist())], dtype=np.float64).reshape(x.shape)
    return v, a[1] & b[1] & (y != 0)


def neg(a):
    if a[0].dtype == np.int64:
        return a[0] * -1, a[1]          # callers wrap to the width (wrap32) where the type is int
    return -a[0], a[1]


def abs_(a):
    return np.abs(a[0]), a[1]           # int64: |Long.MIN| stays Long.MIN (numpy wraps, as Java does)


def signum(a):
    x = _f(a)
    return np.where(x > 0, 1.0, np.where(x < 0, -1.0, x)), a[1]    # +-0 and NaN come back unchanged


# ------------------------------------------------------------------------------------------ math functions
def _to_f64(y) -> float:
    """An mpmath number -> the nearest fp64 (ties to even), also in the subnormal range."""
    if mpmath.isnan(y):
        return math.nan
    if mpmath.isinf(y):
        return math.inf if y > 0 else -math.inf
    man, exp = int(y.man), int(y.exp)
    if man == 0:
        return 0.0
    top = exp + abs(man).bit_length()   # the value lies in [2^(top-1), 2^top)
    if top > 1100:
        return math.inf if y > 0 else -math.inf
    if top < -1100:
        return 0.0 if y > 0 else -0.0
    fr = Fraction(man) * (Fraction(2) ** exp)
    if y < 0 and fr > 0:
        fr = -fr
    try:
        return float(fr)                # int / int true division: correctly rounded
    except OverflowError:
        return math.inf if fr > 0 else -math.inf


_MP = {"ln": "log", "log10": "log10", "log1p": "log1p", "exp": "exp", "expm1": "expm1", "sqrt": "sqrt",
       "sin": "sin", "cos": "cos", "tan": "tan"}
_LD = {"ln": np.log, "log10": np.log10, "log2": np.log2, "log1p": np.log1p, "exp": np.exp, "expm1": np.expm1,
       "sqrt": np.sqrt, "sin": np.sin, "cos": np.cos, "tan": np.tan}


def _mp_unary(name, x: float) -> float:
    if x != x:
        return math.nan
    if math.isinf(x):
        if name in ("sin", "cos", "tan"):
            return math.nan
        if x > 0:
            return math.inf
        return {"exp": 0.0, "expm1": -1.0}.get(name, math.nan)
    if x == 0.0 and name in ("sin", "tan", "expm1", "log1p", "sqrt"):
        return x                        # the sign of zero
    with mpmath.workprec(200):
        X = mpmath.mpf(x)
        if name == "log2":
            y = mpmath.log(X) / mpmath.log(2)
        else:
            y = getattr(mpmath, _MP[name])(X)
        return _to_f64(y)


def math_values(name, x: np.ndarray) -> np.ndarray:
    """name(x) correctly rounded to fp64 (mpmath at 200 bits); out-of-domain inputs give NaN.  Without mpmath:
    np.longdouble rounded to fp64."""
    x = np.asarray(x, dtype=np.float64)
    if mpmath is None:
        with np.errstate(all="ignore"):
            return _LD[name](x.astype(np.longdouble)).astype(np.float64)
    dom = {"ln": lambda v: v > 0, "log10": lambda v: v > 0, "log2": lambda v: v > 0, "log1p": lambda v: v > -1,
           "sqrt": lambda v: v >= 0}.get(name, lambda v: True)
    return np.array([_mp_unary(name, v) if (v != v or dom(v)) else math.nan for v in x.tolist()], dtype=np.float64)


def pow_values(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """x ** y correctly rounded for x > 0 and finite operands (the inputs of the ulp test)."""
    if mpmath is None:
        with np.errstate(all="ignore"):
            return np.power(x.astype(np.longdouble), y.astype(np.longdouble)).astype(np.float64)
    out = []
    with mpmath.workprec(200):
        for a, b in zip(x.tolist(), y.tolist()):
            out.append(_to_f64(mpmath.power(mpmath.mpf(a), mpmath.mpf(b))))
    return np.array(out, dtype=np.float64)


def math_fn(name, a):
    """Spark: log / log10 / log2 of x <= 0, log1p of x <= -1 and sqrt of x < 0 are null; NaN stays a valid NaN."""
    x = _f(a)
    bad = {"ln": x <= 0, "log10": x <= 0, "log2": x <= 0, "log1p": x <= -1, "sqrt": x < 0}.get(name)
    return math_values(name, x), a[1] if bad is None else a[1] & ~bad


def pow_(a, b):
    """Java Math.pow (Spark's pow): y = +-0 gives 1; otherwise a NaN operand gives NaN, and so does |x| = 1 with an
    infinite y.  C99's pow says 1 for pow(1, NaN) and pow(+-1, +-inf); in every other special case the two agree,
    and there, as for ordinary operands, libm's pow is used (the ulp test has its own correctly rounded reference)."""
    x, y = _f(a), _f(b)
    with np.errstate(all="ignore"):
        v = np.power(x, y)
    java_nan = (y != 0) & (np.isnan(y) | np.isnan(x) | ((np.abs(x) == 1) & np.isinf(y)))
    return np.where(java_nan, math.nan, np.where(y == 0, 1.0, v)), a[1] & b[1]


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in units of the last place between fp64 arrays: 0 for two NaNs, huge for NaN against a number."""
    def key(v):
        i = np.asarray(v, dtype=np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i).astype(object)   # -0.0 and 0.0 both map to 0
    an, bn = np.isnan(a), np.isnan(b)
    d = np.abs(key(np.where(an, 0.0, a)) - key(np.where(bn, 0.0, b)))
    d[an != bn] = 2 ** 64
    d[an & bn] = 0
    return d


# ------------------------------------------------------------------------------------------ comparisons, logic
def cmp(op, a, b):
    """IEEE comparisons: anything against NaN is false, != is true."""
    x, y = _f(a), _f(b)
    f = {"==": np.equal, "!=": np.not_equal, "<": np.less, "<=": np.less_equal, ">": np.greater,
         ">=": np.greater_equal}[op]
    return f(x, y).astype(np.float64), a[1] & b[1]


def eqns(a, b):
    """<=>: true for two nulls, false for one null, else ==; never null."""
    x, y = _f(a), _f(b)
    return ((a[1] & b[1] & (x == y)) | (~a[1] & ~b[1])).astype(np.float64), np.ones(len(x), dtype=bool)


def and_(a, b):
    """Kleene: false AND anything = false, true AND null = null."""
    bx, by = (_f(a) != 0) & a[1], (_f(b) != 0) & b[1]
    fx, fy = (_f(a) == 0) & a[1], (_f(b) == 0) & b[1]
    return (bx & by).astype(np.float64), (bx & by) | fx | fy


def or_(a, b):
    """Kleene: true OR anything = true, false OR null = null."""
    bx, by = (_f(a) != 0) & a[1], (_f(b) != 0) & b[1]
    fx, fy = (_f(a) == 0) & a[1], (_f(b) == 0) & b[1]
    return (bx | by).astype(np.float64), bx | by | (fx & fy)


def not_(a):
    return (_f(a) == 0).astype(np.float64), a[1]


def bit(op, a, b):
    """& | ^ of two booleans: plain two-valued logic, null if either side is null."""
    x, y = _f(a) != 0, _f(b) != 0
    v = {"&": x & y, "|": x | y, "^": x != y}[op]
    return v.astype(np.float64), a[1] & b[1]


def isnull(a):
    return (~a[1]).astype(np.float64), np.ones(len(a[1]), dtype=bool)


def isnotnull(a):
    return a[1].astype(np.float64), np.ones(len(a[1]), dtype=bool)


def isnan(a):
    x = _f(a)
    return np.isnan(x).astype(np.float64), a[1]


def when(branches, otherwise=None):
    """CASE WHEN: the first branch whose condition is true (a null condition is false) gives the value; with no
    match the otherwise value, or null without one."""
    n = len(branches[0][0][1])
    dt = np.int64 if all(v[0].dtype == np.int64 for _, v in branches) and (
        otherwise is None or otherwise[0].dtype == np.int64) else np.float64
    out = np.zeros(n, dtype=dt) if otherwise is None else otherwise[0].astype(dt)
    valid = np.zeros(n, dtype=bool) if otherwise is None else otherwise[1].copy()
    for cond, val in reversed(branches):
        take = cond[1] & (_f(cond) != 0)
        out = np.where(take, val[0].astype(dt), out)
        valid = np.where(take, val[1], valid)
    return out, valid


# ------------------------------------------------------------------------------------------ casts (Java)
def _d2l(x: float, lo: int, hi: int) -> int:
    """Java d2i / d2l (JLS 5.1.3): NaN -> 0, otherwise round toward zero and saturate at the type's limits."""
    if x != x:
        return 0
    if x >= hi:
        return hi
    if x <= lo:
        return lo
    return int(x)


def _d2(a, lo, hi):
    x = _f(a)
    return np.array([_d2l(v, lo, hi) for v in x.tolist()], dtype=np.int64)


def cast_int(a):
    """double / float -> int: saturating truncation; NaN and +-inf give null (the project's documented rule)."""
    return _d2(a, I32_MIN, I32_MAX), a[1] & np.isfinite(_f(a))


def cast_long(a):
    """double / float -> long: saturating truncation; NaN and +-inf give null."""
    return _d2(a, I64_MIN, I64_MAX), a[1] & np.isfinite(_f(a))


def floor_long(a):
    """floor to long: Java (long) Math.floor(x): saturates, NaN -> 0, never null by itself."""
    return _d2((np.floor(_f(a)), a[1]), I64_MIN, I64_MAX), a[1]


def ceil_long(a):
    return _d2((np.ceil(_f(a)), a[1]), I64_MIN, I64_MAX), a[1]


def wrap32(a):
    """long -> int (Java l2i), and int arithmetic that overflows: the low 32 bits, sign-extended."""
    return np.array([((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31 for v in a[0].tolist()], dtype=np.int64), a[1]


def to_double(a):
    return _f(a), a[1]


def to_f32(a):
    with np.errstate(all="ignore"):
        return _f(a).astype(np.float32).astype(np.float64), a[1]


def to_bool(a):
    return (_f(a) != 0).astype(np.float64), a[1]


def _round_half_up(x: float, s: int) -> float:
    if x != x or math.isinf(x):
        return x
    q = Fraction(10) ** s
    t = abs(Fraction(x)) * q                         # exact
    f = t.numerator // t.denominator
    if t - f >= Fraction(1, 2):
        f += 1
    r = Fraction(f) / q
    try:
        y = float(r)                                 # one rounding, to nearest
    except OverflowError:
        y = math.inf
    return -y if (x < 0 and y != 0) else y           # a BigDecimal has no negative zero


def round_(a, s: int):
    """round(x, s): exact HALF_UP on the binary value of the double (Spark rounds BigDecimal(x)), then the nearest
    double.  Ties that exist only in the shortest decimal string (2.675, 1.005, whose doubles lie below the tie)
    are a known, separate deviation from Spark and are kept out of the inputs: use k / 2^m with small k, integers,
    and the carry cases 0.49999999999999994, 2^52 + 1, 1e308."""
    return np.array([_round_half_up(v, s) for v in _f(a).tolist()], dtype=np.float64), a[1]


def same(got, ref, what=""):
    """Assert two columns equal: the validity masks exactly, and the values of valid rows bit for bit (NaN equals
    NaN; the sign of a zero counts for float values)."""
    gv, gm = got
    rv, rm = ref
    assert np.array_equal(gm, rm), f"{what}: validity differs at rows {np.flatnonzero(gm != rm)[:8]}"
    gv, rv = np.asarray(gv)[rm], np.asarray(rv)[rm]
    if rv.dtype == np.int64:
        bad = gv.astype(np.int64) != rv
    else:
        bad = np.asarray(gv, dtype=np.float64).view(np.int64) != rv.view(np.int64)
        bad &= ~(np.isnan(np.asarray(gv, dtype=np.float64)) & np.isnan(rv))
    assert not bad.any(), (f"{what}: {int(bad.sum())} values differ, first at valid row {np.flatnonzero(bad)[0]}: "
                           f"got {gv[bad][0]!r}, expected {rv[bad][0]!r}")


# ------------------------------------------------------------------------------------------ K20
def _exact_sums(x: np.ndarray):
    """(sum, sum of squares) of finite doubles as exact Fractions."""
    k = x * 1024.0
    if len(x) and np.all(k == np.round(k)) and np.abs(k).max() < 2.0 ** 22:
        ki = k.astype(np.int64)                      # n * k^2 < 2^17 * 2^44: exact in int64
        return Fraction(int(ki.sum()), 1024), Fraction(int((ki * ki).sum()), 1024 * 1024)
    fr = [Fraction(v) for v in x.tolist()]
    return sum(fr, Fraction(0)), sum((v * v for v in fr), Fraction(0))


def ref_moments(X: np.ndarray, valid=None) -> np.ndarray:
    """Per-column (count, mean, M2, min, max) of X [n, d] as fp64 [d, 5], what K.col_moments documents.

    Nulls (valid == 0) are skipped.  Finite columns: exact rational sums, mean = S / n and M2 = Q - S^2 / n, each
    rounded once to fp64.  NaN is a value: mean, M2 and max become NaN and min skips it.  An infinity gives what
    sum / count gives: only +inf (or only -inf) among the non-finite values: mean +-inf and M2 NaN; both: mean NaN.
    Count 0 gives (0, 0, 0, +inf, -inf).  An all-NaN column has min = +inf: the kernel header's "min skips NaNs" is
    pinned here (Spark itself, ordering NaN above every number, would report NaN)."""
    X = np.asarray(X)
    n, d = X.shape
    out = np.zeros((d, 5), dtype=np.float64)
    for c in range(d):
        x = X[:, c].astype(np.float64)
        if valid is not None:
            x = x[np.asarray(valid)[:, c].astype(bool)]
        cnt = len(x)
        if cnt == 0:
            out[c] = (0.0, 0.0, 0.0, math.inf, -math.inf)
            continue
        nan, pinf, ninf = np.isnan(x).any(), (x == math.inf).any(), (x == -math.inf).any()
        nn = x[~np.isnan(x)]
        mn = nn.min() if len(nn) else math.inf
        mx = math.nan if nan else x.max()
        if nan or (pinf and ninf):
            mean, m2 = math.nan, math.nan
        elif pinf or ninf:
            mean, m2 = (math.inf if pinf else -math.inf), math.nan
        else:
            S, Q = _exact_sums(x)
            mean, m2 = float(S / cnt), float(Q - S * S / cnt)
        out[c] = (cnt, mean, m2, mn, mx)
    return out


def moment_matrix(n, d, rng):
    """X [n, d >= 8] of non-negative k / 2^10 (exact sums are cheap, and a mean without cancellation is defined to
    the ulp) with ~10% nulls, and validity; columns 0 to 6: all null, all NaN, one NaN, only +inf, both infinities,
    constant, mean 1e8 with unit spread."""
    X = rng.integers(0, 2 ** 20, (n, d)).astype(np.float64) / 1024.0
    v = rng.random((n, d)) < 0.9
    sp = [[math.nan] * n, [math.nan] + [1.5] * (n - 1), [math.inf] * min(n, 2) + [2.0] * max(n - 2, 0),
          [math.inf, -math.inf] + [0.5] * (n - 2), [102 / 1024] * n,
          list(1e8 + rng.integers(-1024, 1024, n) / 1024.0)]
    for j, colv in enumerate(sp):
        X[:, j + 1] = np.asarray(colv[:n])
        v[:, j + 1] = True
    v[:, 0] = False                                   # all null
    return X, v


def m2_tolerance(ref_m2, n):
    return 4 * np.spacing(np.abs(ref_m2)) + 4 * n * np.finfo(np.float64).eps * np.abs(ref_m2)


def moments_close(got, ref, n):
    """count / min / max exact; mean within 4 ulp; M2 within 4 ulp + 4 n eps M2 (the reference's own rounding)."""
    got, ref = np.asarray(got), np.asarray(ref)
    for j in (0, 3, 4):
        assert np.array_equal(got[:, j], ref[:, j], equal_nan=True), (j, np.flatnonzero(got[:, j] != ref[:, j])[:8])
    dm = ulp_distance(got[:, 1], ref[:, 1])
    assert dm.max() <= 4, f"mean {dm.max()} ulp off in column {int(np.argmax(dm))}"
    assert np.array_equal(np.isnan(got[:, 2]), np.isnan(ref[:, 2]))
    fin = np.isfinite(ref[:, 2])
    err = np.abs(got[fin, 2] - ref[fin, 2])
    tol = m2_tolerance(ref[fin, 2], n)
    worst = int(np.argmax(err - tol))
    assert (err <= tol).all(), f"M2 off by {err[worst]} (tolerance {tol[worst]}) in column {np.flatnonzero(fin)[worst]}"
    return int(dm.max()), float((err / np.maximum(np.abs(ref[fin, 2]), 1e-300)).max())


# ------------------------------------------------------------------------------------------ K19 / K16
def ref_compact(mask: np.ndarray) -> np.ndarray:
    return np.flatnonzero(np.asarray(mask).reshape(-1)).astype(np.int64)


def ref_partition_dest(dest: np.ndarray, W: int):
    dest = np.asarray(dest).astype(np.int64)
    return np.argsort(dest, kind="stable").astype(np.int64), np.bincount(dest, minlength=W).astype(np.int64)


def ref_gather(src: np.ndarray, idx: np.ndarray, nsrc: int) -> np.ndarray:
    """src[idx], with 0 where idx < 0 or idx >= nsrc (GatherArgs: such an index reads nothing and writes 0)."""
    idx = np.asarray(idx).astype(np.int64)
    ok = (idx >= 0) & (idx < nsrc)
    return np.where(ok, src[np.where(ok, idx, 0)], np.zeros((), dtype=src.dtype)).astype(src.dtype)
