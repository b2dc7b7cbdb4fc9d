"""The DataFrame kernels K18 to K20 without a GPU: the plain references of tests/_frame_refs.py checked by hand, then
the operator path (``Expr.eval``) and the host model of expr.hip (``fused.interpret``) against them on the edge
table, and the CPU formulations of col_moments / partition_dest / compact_mask against theirs.  The kernels
themselves are in tests/test_frame_kernels_gpu.py, against the same references."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _frame_cases as FC
from tests import _frame_refs as R
from cdnaml.ops import kernels as K, relops as RO
from cdnaml.sql import fused
from cdnaml.sql.column import EvalContext

INF, NAN = math.inf, math.nan
# glibc / SLEEF document at most 1 to 2 ulp for the fp64 functions used here; the references are correctly rounded
CPU_ULP = 4
CASES = FC.cases()


def col(*items):
    return R.column(list(items))


def vals(a):
    return [None if not m else (int(v) if a[0].dtype == np.int64 else float(v)) for v, m in zip(a[0], a[1])]


def same_list(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w is None or g is None:
            assert g is None and w is None, (got, want)
        elif isinstance(w, float) and w != w:
            assert g != g, (got, want)
        else:
            assert g == w and math.copysign(1, g) == math.copysign(1, w), (got, want)


# ------------------------------------------------------------------------------------------ the references
def test_ref_casts_follow_java():
    x = col(3e10, -3e10, 2.0 ** 31 - 0.5, 2.0 ** 31, -2.0 ** 31 - 1, 1e19, -1e19, 2.0 ** 63, 1e308, -2.9, 2.9, NAN,
            INF, -INF, None)
    same_list(vals(R.cast_int(x)), [2147483647, -2147483648, 2147483647, 2147483647, -2147483648, 2147483647,
                                    -2147483648, 2147483647, 2147483647, -2, 2, None, None, None, None])
    same_list(vals(R.cast_long(x)), [30000000000, -30000000000, 2147483647, 2147483648, -2147483649,
                                     2 ** 63 - 1, -2 ** 63, 2 ** 63 - 1, 2 ** 63 - 1, -2, 2, None, None, None, None])
    # the saturated value flows on: (x * 1.0).cast("int") + 0.5 at 3e10, and Long.MAX as a double is 2^63
    same_list(vals(R.add(R.cast_int(col(3e10, -3e10)), col(0.5, 0.5))), [2147483647.5, -2147483647.5])
    same_list(vals(R.add(R.cast_long(col(1e19)), col(0.5))), [2.0 ** 63])
    # floor / ceil to long saturate, and NaN is Java's 0; long -> int keeps the low 32 bits
    same_list(vals(R.floor_long(col(1e308, -1e308, 2.5, -2.5, INF, -INF, NAN, None))),
              [2 ** 63 - 1, -2 ** 63, 2, -3, 2 ** 63 - 1, -2 ** 63, 0, None])
    same_list(vals(R.ceil_long(col(2.5, -2.5, -0.5, 1e19))), [3, -2, 0, 2 ** 63 - 1])
    same_list(vals(R.wrap32(R.floor_long(col(3e10, -3e10, 1e19, -1e19, 2.0 ** 31, 2.0 ** 32 + 5)))),
              [-64771072, 64771072, -1, 0, -2147483648, 5])
    same_list(vals(R.wrap32(R.abs_((np.array([-2 ** 31, -5], dtype=np.int64), np.ones(2, bool))))), [-2 ** 31, 5])


def test_ref_round_is_exact_half_up():
    x = col(0.49999999999999994, 0.5, -0.5, 2.5, -2.5, 4503599627370497.0, 1e308, 1.125, -1.125, 0.375, 150.0, -250.0,
            49.0, NAN, INF, None)
    same_list(vals(R.round_(x, 0)), [0.0, 1.0, -1.0, 3.0, -3.0, 4503599627370497.0, 1e308, 1.0, -1.0, 0.0, 150.0,
                                     -250.0, 49.0, NAN, INF, None])
    same_list(vals(R.round_(x, 2)), [0.5, 0.5, -0.5, 2.5, -2.5, 4503599627370497.0, 1e308, 1.13, -1.13, 0.38, 150.0,
                                     -250.0, 49.0, NAN, INF, None])
    same_list(vals(R.round_(x, -2)), [0.0, 0.0, 0.0, 0.0, 0.0, 4503599627370500.0, 1e308, 0.0, 0.0, 0.0, 200.0, -300.0,
                                      0.0, NAN, INF, None])


def test_ref_arithmetic_and_null_rules():
    x, y = col(1.0, 1.0, 0.0, INF, 5.5, -5.5, NAN, None, 1.0), col(0.0, -0.0, 0.0, 0.0, 2.0, 2.0, 1.0, 1.0, None)
    same_list(vals(R.div(x, y)), [None, None, None, None, 2.75, -2.75, NAN, None, None])
    same_list(vals(R.mod(x, y)), [None, None, None, None, 1.5, -1.5, NAN, None, None])
    same_list(vals(R.mod(col(INF, 5.0, -0.0), col(2.0, INF, 3.0))), [NAN, 5.0, -0.0])
    z = col(0.0, -1.0, 1.0, NAN, INF, -INF, None)
    same_list(vals(R.math_fn("ln", z)), [None, None, 0.0, NAN, INF, None, None])
    same_list(vals(R.math_fn("log10", col(100.0, 0.0))), [2.0, None])
    same_list(vals(R.math_fn("log2", col(8.0, -8.0))), [3.0, None])
    same_list(vals(R.math_fn("log1p", col(-1.0, -0.5, 0.0, NAN))), [None, math.log1p(-0.5), 0.0, NAN])
    same_list(vals(R.math_fn("sqrt", col(-1.0, -0.0, 4.0, 2.0, NAN))), [None, -0.0, 2.0, math.sqrt(2.0), NAN])
    same_list(vals(R.signum(col(-3.0, 0.0, -0.0, 7.0, NAN, None))), [-1.0, 0.0, -0.0, 1.0, NAN, None])
    same_list(vals(R.abs_(col(-3.0, -0.0, -INF))), [3.0, 0.0, INF])
    same_list(vals(R.to_f32(col(1e308, 0.1, 5e-324))), [INF, float(np.float32(0.1)), 0.0])
    same_list(vals(R.to_bool(col(0.0, -0.0, NAN, 2.0, None))), [0.0, 0.0, 1.0, 1.0, None])


def test_ref_comparisons_and_kleene_logic():
    x, y = col(1.0, NAN, NAN, 0.0, None, None, INF), col(2.0, NAN, 1.0, -0.0, 1.0, None, INF)
    same_list(vals(R.cmp("<", x, y)), [1.0, 0.0, 0.0, 0.0, None, None, 0.0])
    same_list(vals(R.cmp("==", x, y)), [0.0, 0.0, 0.0, 1.0, None, None, 1.0])
    same_list(vals(R.cmp("!=", x, y)), [1.0, 1.0, 1.0, 0.0, None, None, 0.0])
    same_list(vals(R.eqns(x, y)), [0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0])
    t, f, n = 1.0, 0.0, None
    p, q = col(t, t, t, f, f, f, n, n, n), col(t, f, n, t, f, n, t, f, n)
    same_list(vals(R.and_(p, q)), [t, f, n, f, f, f, n, f, n])
    same_list(vals(R.or_(p, q)), [t, t, t, t, f, n, t, n, n])
    same_list(vals(R.not_(col(t, f, n))), [f, t, n])
    same_list(vals(R.bit("^", p, q)), [f, t, n, t, f, n, n, n, n])
    same_list(vals(R.isnull(col(1.0, NAN, None))), [0.0, 0.0, 1.0])
    same_list(vals(R.isnotnull(col(1.0, NAN, None))), [1.0, 1.0, 0.0])
    same_list(vals(R.isnan(col(1.0, NAN, None))), [0.0, 1.0, None])
    # first match wins, a null condition is false, no match without otherwise is null
    c1, c2 = col(t, t, f, n, f), col(t, f, t, t, n)
    v1, v2, o = col(1.0, 1.0, 1.0, 1.0, 1.0), col(2.0, 2.0, None, 2.0, 2.0), col(9.0, 9.0, 9.0, 9.0, 9.0)
    same_list(vals(R.when([(c1, v1), (c2, v2)], o)), [1.0, 1.0, None, 2.0, 9.0])
    same_list(vals(R.when([(c1, v1), (c2, v2)])), [1.0, 1.0, None, 2.0, None])


def test_ref_ulp_distance_and_rounding_of_the_math_reference():
    a = np.array([1.0, 1.0, 0.0, -0.0, NAN, NAN, INF, 5e-324])
    b = np.array([np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), -0.0, 5e-324, NAN, 1.0, np.finfo(np.float64).max,
                  -5e-324])
    assert list(R.ulp_distance(a, b)) == [1, 1, 0, 1, 0, 2 ** 64, 1, 2]
    # correctly rounded where libm's answer is known to be exact or is the nearest double
    got = R.math_values("exp", np.array([0.0, 1.0, -INF, 710.0, -745.0]))
    assert list(got[:4]) == [1.0, math.e, 0.0, INF] and got[4] == 5e-324
    assert list(R.math_values("log2", np.array([2.0 ** -1074, 2.0 ** 1000]))) == [-1074.0, 1000.0]
    got = R.pow_values(np.array([2.0, 10.0, 2.0]), np.array([0.5, -2.0, -1074.0]))
    assert list(got) == [math.sqrt(2.0), 0.01, 5e-324]
    # Java's special cases of pow, where C99 says 1
    p = R.pow_(col(1.0, 1.0, -1.0, -1.0, NAN, NAN, 2.0, 1.0, INF, None),
               col(NAN, INF, -INF, 2.0, 0.0, 1.0, NAN, -0.0, 0.0, 1.0))
    same_list(vals(p), [NAN, NAN, NAN, 1.0, 1.0, NAN, NAN, 1.0, 1.0, None])


def test_ref_moments_by_hand():
    X = np.array([[1.0, NAN, INF, INF, 5.0, 1e8, NAN, 2.0],
                  [2.0, 1.0, 1.0, -INF, 5.0, 1e8 + 1, NAN, 7.0],
                  [6.0, 3.0, 2.0, 0.0, 5.0, 1e8 + 2, NAN, 9.0]])
    v = np.ones_like(X, dtype=bool)
    v[:, 7] = False
    m = R.ref_moments(X, v)
    same_list(list(m[0]), [3.0, 3.0, 14.0, 1.0, 6.0])
    same_list(list(m[1]), [3.0, NAN, NAN, 1.0, NAN])
    same_list(list(m[2]), [3.0, INF, NAN, 1.0, INF])
    same_list(list(m[3]), [3.0, NAN, NAN, -INF, INF])
    same_list(list(m[4]), [3.0, 5.0, 0.0, 5.0, 5.0])
    same_list(list(m[5]), [3.0, 1e8 + 1, 2.0, 1e8, 1e8 + 2])
    same_list(list(m[6]), [3.0, NAN, NAN, INF, NAN])          # all NaN: min skips NaNs (pinned)
    same_list(list(m[7]), [0.0, 0.0, 0.0, INF, -INF])
    same_list(list(R.ref_moments(np.array([[-INF], [3.0]]))[0]), [2.0, -INF, NAN, -INF, 3.0])
    # the exact path: 0.1 is not k / 2^10, its sums go through Fractions
    m = R.ref_moments(np.array([[0.1], [0.2], [0.3]]))
    assert m[0, 1] == float(sum(map(Fraction, [0.1, 0.2, 0.3])) / 3)


def test_ref_relational_by_hand():
    assert list(R.ref_compact(np.array([0, 1, 1, 0, 2], dtype=np.uint8))) == [1, 2, 4]
    perm, cnt = R.ref_partition_dest(np.array([2, 0, 2, 1, 0]), 4)
    assert list(perm) == [1, 4, 3, 0, 2] and list(cnt) == [2, 1, 2, 0]
    src = np.array([10, 11, 12], dtype=np.int16)
    assert list(R.ref_gather(src, np.array([2, -1, 0, 3, 2]), 3)) == [12, 0, 10, 0, 12]
    assert list(R.ref_gather(src, np.array([2, 1]), 2)) == [0, 11]      # nsrc of the shortest source of the call


# ------------------------------------------------------------------------------------------ K18 on the host
def check(name, got, ref, tol, bound, rows):
    """Validity exactly; values bit for bit, or within ``bound`` ulp of the reference for a transcendental."""
    if tol is None:
        return R.same(got, ref, name)
    assert np.array_equal(got[1], ref[1]), f"{name}: validity differs at rows {np.flatnonzero(got[1] != ref[1])[:8]}"
    sel = ref[1] & rows
    d = R.ulp_distance(np.asarray(got[0], dtype=np.float64)[sel], ref[0][sel])
    print(f"{name}: max {d.max()} ulp")
    assert len(d) and d.max() <= bound, f"{name}: {d.max()} ulp from the reference (bound {bound})"


@pytest.fixture(scope="module", params=[True, False], ids=["valid", "novalid"])
def host(request):
    cols = FC.make_inputs(request.param, tile=1)
    return cols, FC.to_batch(cols, torch.device("cpu"), request.param), FC.ref_cols(cols)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_operator_path_and_interpret_match_reference(host, case):
    """Both host evaluations of every case equal the plain reference on all pairs of the edge table; the cast,
    narrowing and round cases are the ones that failed before casts saturated and ROUND stopped carrying."""
    cols, b, rc = host
    name, mk, mkref, out_t, tol = case
    e = mk(FC.columns())._expr
    ref = mkref(rc)
    bound = {None: 0, "sqrt": 0}.get(tol, CPU_ULP)
    rows = FC.compared_rows(cols, tol)
    op = e.eval(b, EvalContext(None))
    # torch's vectorised CPU sqrt is not correctly rounded (sqrt(0.5) is one ulp low); numpy's and the GPU's are
    check(name + " (operator path)", FC.result(op), ref, tol, 1 if tol == "sqrt" else bound, rows)
    prog = fused._program(e, b)
    assert prog is not None, f"{name} does not fuse"
    got = fused.interpret(prog[0], prog[1], b)
    assert got.values.dtype == out_t and type(got.dtype) is type(op.dtype), name
    check(name + " (interpret)", FC.result(got), ref, tol, bound, rows)


def test_cases_cover_every_opcode(host):
    """The union of the opcodes of the compiled case programs is all of fused.OP."""
    _, b, _ = host
    seen = set()
    for name, mk, _, _, _ in CASES:
        seen |= {ins & 0xFF for ins in fused._program(mk(FC.columns())._expr, b)[0].code}
    assert seen == set(fused.OP.values()), sorted(set(fused.OP.values()) ^ seen)


def test_numbers_of_the_findings():
    """Each number quoted when the gap was found, on all three host-visible paths."""
    from cdnaml.sql import functions as F
    from cdnaml.sql import types as T
    from cdnaml.sql.batch import Batch, ColumnData
    xs = [3e10, 1e19, 1e308, 0.49999999999999994, 4503599627370497.0]
    b = Batch({"x": ColumnData(torch.tensor(xs, dtype=torch.float64), T.DoubleType())})
    x = F.col("x")
    want = {"cast_int": ((x * 1.0).cast("int") + 0.5, [2147483647.5] * 3 + [0.5, 2147483647.5]),
            "cast_long": ((x * 1.0).cast("long") + 0.0, [3e10, 2.0 ** 63, 2.0 ** 63, 0.0, 4503599627370497.0]),
            "floor": (F.floor(x * 1.0), [30000000000, 2 ** 63 - 1, 2 ** 63 - 1, 0, 4503599627370497]),
            "floor_int": (F.floor(x * 1.0).cast("int"), [-64771072, -1, -1, 0, 1]),
            "round0": (F.round(x * 1.0, 0), [3e10, 1e19, 1e308, 0.0, 4503599627370497.0]),
            "round2": (F.round(x * 1.0, 2), [3e10, 1e19, 1e308, 0.5, 4503599627370497.0])}
    for name, (e, w) in want.items():
        op = e._expr.eval(b, EvalContext(None))
        prog = fused._program(e._expr, b)
        assert prog is not None, name
        it = fused.interpret(prog[0], prog[1], b)
        for c in (op, it):
            assert c.valid_mask().all() and c.values.tolist() == w, (name, c.values.tolist())


def test_program_limits():
    """256 instructions and 16 stack slots fuse; one more of either falls back to the operator path."""
    from cdnaml.sql import functions as F
    b = FC.to_batch(FC.make_inputs(True, tile=1), torch.device("cpu"))
    cols = FC.make_inputs(True, tile=1)
    sizes = []
    for e, fits, ref in FC.limit_programs(F.col("x")):
        prog = fused._program(e._expr, b)
        assert (prog is not None) == fits
        R.same(FC.result(e._expr.eval(b, EvalContext(None))), ref(FC.ref_cols(cols)), "operator path")
        if fits:
            sizes.append((len(prog[0].code), prog[0].maxdepth))
            R.same(FC.result(fused.interpret(prog[0], prog[1], b)), ref(FC.ref_cols(cols)), "interpret")
    assert sizes[0][0] == 256 and sizes[1][1] == 16


# ------------------------------------------------------------------------------------------ K19 / K20 on the host
@pytest.mark.parametrize("n,d", [(1, 1), (3, 8), (257, 65)])
def test_cpu_col_moments_matches_reference(n, d):
    rng = np.random.default_rng(n)
    if d < 8:
        X, v = rng.integers(0, 2 ** 20, (n, d)) / 1024.0, np.ones((n, d), dtype=bool)
    else:
        X, v = R.moment_matrix(n, d, rng)
    R.moments_close(K.col_moments(torch.from_numpy(X), torch.from_numpy(v)), R.ref_moments(X, v), n)
    R.moments_close(K.col_moments(torch.from_numpy(X)), R.ref_moments(X), n)


def test_merge_moments_follows_the_rules():
    """The device-side merge of per-block partials: a part that saw an infinity carries mean +-inf and M2 NaN, and
    the merged column follows ref_moments; a constant column keeps M2 = 0 exactly.  With c = 1 / 3 and blocks of
    256, 256 and 113 rows the weighted mean sum(w * c) rounds to c + 5.6e-17, outside the block means: without the
    clamp M2 comes out as 625 * (5.6e-17)^2 instead of 0."""
    c = 1.0 / 3.0
    w = torch.tensor([256.0, 256.0, 113.0], dtype=torch.float64) / 625.0
    assert float((w * c).sum()) != c          # the case does leave the range unclamped
    part = torch.tensor([[[256, c, 0, c, c], [256, INF, NAN, 1, INF], [256, INF, NAN, 1, INF], [2, NAN, NAN, 1, NAN],
                          [0, 0, 0, INF, -INF]],
                         [[256, c, 0, c, c], [256, 2.0, 3.0, 0, 4], [256, -INF, NAN, -INF, 4], [9, 1.0, 1.0, 0, 2],
                          [0, 0, 0, INF, -INF]],
                         [[113, c, 0, c, c], [0, 0, 0, INF, -INF], [7, 3.0, 1.0, 2, 4], [9, 1.0, 1.0, 0, 2],
                          [0, 0, 0, INF, -INF]]], dtype=torch.float64)
    m = RO._merge_moments(part).numpy()
    same_list(list(m[0]), [625.0, c, 0.0, c, c])
    same_list(list(m[1]), [512.0, INF, NAN, 0.0, INF])
    same_list(list(m[2]), [519.0, NAN, NAN, -INF, INF])
    same_list(list(m[3]), [20.0, NAN, NAN, 0.0, NAN])
    same_list(list(m[4]), [0.0, 0.0, 0.0, INF, -INF])


@pytest.mark.parametrize("n", [1, 255, 4097])
def test_cpu_compact_and_partition_match_reference(n):
    rng = np.random.default_rng(n)
    for mask in (rng.random(n) < 0.5, np.zeros(n, dtype=bool), np.ones(n, dtype=bool)):
        assert np.array_equal(K.compact_mask(torch.from_numpy(mask)).numpy(), R.ref_compact(mask))
    for W in (1, 2, 64, 8193):
        dest = rng.integers(0, W, n).astype(np.int32)
        perm, cnt = K.partition_dest(torch.from_numpy(dest), W)
        rp, rc = R.ref_partition_dest(dest, W)
        assert np.array_equal(perm.numpy(), rp) and np.array_equal(cnt.numpy(), rc)
