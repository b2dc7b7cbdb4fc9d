"""The K18 expression cases shared by tests/test_frame_kernels_cpu.py (operator path and fused.interpret) and
tests/test_frame_kernels_gpu.py (expr.hip): inputs built from the edge table of tests/_frame_refs.py, and for every
case the expression next to its reference, composed from the plain rules of that module.

Every program needs two operators to fuse, so single opcodes are wrapped in an operator that changes nothing:
``* 1.0`` on a double, ``| false`` on a boolean (both are part of the reference too)."""
import numpy as np
import torch

from tests import _frame_refs as R
from cdnaml.sql import functions as F
from cdnaml.sql import types as T
from cdnaml.sql.batch import Batch, ColumnData
from cdnaml.sql.column import BinOp, Column

I32 = np.array([0, 1, -1, 2, -2, 3, 2 ** 31 - 1, -2 ** 31, 65536, -65537, 46341], dtype=np.int32)
I64 = np.array([0, 1, -1, 2 ** 31, -2 ** 31 - 1, 2 ** 53 - 1, -(2 ** 53 - 1), 500_000, 500_001, 999_999, 7],
               dtype=np.int64)
TYPES = {"x": T.DoubleType, "y": T.DoubleType, "xf": T.FloatType, "k": T.IntegerType, "ke": T.IntegerType,
         "l": T.LongType, "p": T.BooleanType, "q": T.BooleanType}
TRIG = ("sin", "cos", "tan")
TRANSCENDENTAL = ("ln", "log10", "log2", "log1p", "exp", "expm1", "pow", "sin", "cos", "tan")


def compared_rows(cols, tol):
    """The rows whose values are compared: the trigonometric functions, and the chains that hold one, only for
    |x| <= 1e6 (and non-finite x)."""
    n = len(cols["x"][1])
    if tol not in TRIG and tol != "compose":
        return np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        small = lambda v: ~np.isfinite(v) | (np.abs(v) <= 1e6)      # noqa: E731
        return small(cols["x"][0]) & small(cols["xf"][0].astype(np.float64))


def make_inputs(with_valid=True, tile=8):
    """name -> (values, valid) numpy columns: x, y all ordered pairs of the edge table (nulls become 0.0 without
    validity), xf = y in fp32, k in [-3, 3], ke / l the int / long edges, p / q booleans in every Kleene pairing."""
    (xv, xm), (yv, ym) = R.edge_pairs()
    xv, xm, yv, ym = (np.tile(a, tile) for a in (xv, xm, yv, ym))
    n = len(xv)
    r = np.arange(n)
    with np.errstate(all="ignore"):
        cols = {"x": (xv, xm), "y": (yv, ym), "xf": (yv.astype(np.float32), ym),
                "k": (((r * 5) % 7 - 3).astype(np.int32), r % 11 != 0), "ke": (I32[r % len(I32)], r % 13 != 0),
                "l": (I64[r % len(I64)], r % 17 != 0), "p": (r % 3 == 0, r % 5 != 0), "q": (r % 2 == 0, r % 7 != 0)}
    if not with_valid:
        cols = {k: (v, np.ones(n, dtype=bool)) for k, (v, m) in cols.items()}
    return cols


def to_batch(cols, device, with_valid=True) -> Batch:
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    return Batch({k: ColumnData(t(v), TYPES[k](), t(m) if with_valid else None) for k, (v, m) in cols.items()})


def ref_cols(cols):
    """The reference's view of the inputs: float64 for double / float / boolean columns, int64 for int / long."""
    return {k: ((v.astype(np.int64) if v.dtype.kind == "i" else v.astype(np.float64)), m.copy())
            for k, (v, m) in cols.items()}


def result(c: ColumnData):
    """A ColumnData as the (values, valid) pair of the references (integers as int64, the rest as float64)."""
    v = c.values.detach().cpu()
    v = v.to(torch.int64).numpy() if v.dtype in (torch.int32, torch.int64) else v.to(torch.float64).numpy()
    return v, c.valid_mask().cpu().numpy().astype(bool)


def _const(r, value):
    n = len(r["x"][1])
    return np.full(n, float(value)), np.ones(n, dtype=bool)


def _null(r):
    n = len(r["x"][1])
    return np.zeros(n), np.zeros(n, dtype=bool)


def cases():
    """[(name, expression(columns) -> Column, reference(ref columns) -> (values, valid), out torch dtype, tol)]:
    tol is None for bit-exact cases, else the transcendental whose ulp bound applies (tests/test_frame_kernels_gpu
    ULP), or "compose" for the two chains of transcendentals."""
    C = []
    one = lambda r: _const(r, 1.0)      # noqa: E731
    false = lambda r: _const(r, 0.0)    # noqa: E731
    lit_f = F.lit(False)

    def case(name, e, ref, out=torch.float64, tol=None):
        C.append((name, e, ref, out, tol))

    def x1(c):
        return c["x"] * 1.0

    def rx1(r):
        return R.mul(r["x"], one(r))

    # ---- binary arithmetic, all pairs
    for nm, op, rf in [("ADD", lambda a, b: a + b, R.add), ("SUB", lambda a, b: a - b, R.sub),
                       ("MUL", lambda a, b: a * b, R.mul), ("DIV", lambda a, b: a / b, R.div),
                       ("MOD", lambda a, b: a % b, R.mod)]:
        case(nm, lambda c, op=op: op(c["x"], c["y"]) * 1.0, lambda r, rf=rf: R.mul(rf(r["x"], r["y"]), one(r)))
    case("POW", lambda c: F.pow(c["x"], c["y"]) * 1.0, lambda r: R.mul(R.pow_(r["x"], r["y"]), one(r)), tol="pow")
    # ---- comparisons, all pairs
    for nm, op in [("EQ", "=="), ("NE", "!="), ("LT", "<"), ("LE", "<="), ("GT", ">"), ("GE", ">=")]:
        case(nm, lambda c, op=op: Column(BinOp(op, c["x"]._expr, c["y"]._expr)) | lit_f,
             lambda r, op=op: R.or_(R.cmp(op, r["x"], r["y"]), false(r)), torch.bool)
    case("EQNS", lambda c: c["x"].eqNullSafe(c["y"]) | lit_f, lambda r: R.or_(R.eqns(r["x"], r["y"]), false(r)),
         torch.bool)
    case("CMP_typed", lambda c: (c["ke"] <= c["k"]) | (c["l"] * 1.0 > c["xf"]) | (c["p"] == c["q"]),
         lambda r: R.or_(R.or_(R.cmp("<=", r["ke"], r["k"]), R.cmp(">", R.mul(r["l"], one(r)), r["xf"])),
                         R.cmp("==", r["p"], r["q"])), torch.bool)
    # ---- logic
    case("AND", lambda c: (c["p"] & c["q"]) | lit_f, lambda r: R.or_(R.and_(r["p"], r["q"]), false(r)), torch.bool)
    case("OR", lambda c: (c["p"] | c["q"]) & F.lit(True), lambda r: R.and_(R.or_(r["p"], r["q"]), one(r)),
         torch.bool)
    case("AND_num", lambda c: (c["x"] > 0) & (c["y"] > 0),
         lambda r: R.and_(R.cmp(">", r["x"], false(r)), R.cmp(">", r["y"], false(r))), torch.bool)
    case("NOT", lambda c: ~(c["x"] > c["y"]) | lit_f,
         lambda r: R.or_(R.not_(R.cmp(">", r["x"], r["y"])), false(r)), torch.bool)
    for nm, op in [("BAND", "&"), ("BOR", "|"), ("BXOR", "^")]:
        case(nm, lambda c, op=op: Column(BinOp(op, c["p"]._expr, c["q"]._expr)) | lit_f,
             lambda r, op=op: R.or_(R.bit(op, r["p"], r["q"]), false(r)), torch.bool)
    # ---- unary
    case("NEG", lambda c: (-c["x"]) * 1.0, lambda r: R.mul(R.neg(r["x"]), one(r)))
    case("NEG_i32", lambda c: (-c["ke"]) * 1.0, lambda r: R.mul(R.wrap32(R.neg(r["ke"])), one(r)))
    case("ABS", lambda c: F.abs(c["x"]) * 1.0, lambda r: R.mul(R.abs_(r["x"]), one(r)))
    case("ABS_i32", lambda c: F.abs(c["ke"]) * 1.0, lambda r: R.mul(R.wrap32(R.abs_(r["ke"])), one(r)))
    case("ABS_f32", lambda c: F.abs(c["xf"]) * 1.0, lambda r: R.mul(R.abs_(r["xf"]), one(r)))
    for nm, fn in [("ln", F.log), ("log10", F.log10), ("log2", F.log2), ("log1p", F.log1p), ("exp", F.exp),
                   ("expm1", F.expm1), ("sin", F.sin), ("cos", F.cos), ("tan", F.tan)]:
        case(nm.upper(), lambda c, fn=fn: fn(c["x"]) * 1.0, lambda r, nm=nm: R.mul(R.math_fn(nm, r["x"]), one(r)),
             tol=nm)
    case("SQRT", lambda c: F.sqrt(c["x"]) * 1.0, lambda r: R.mul(R.math_fn("sqrt", r["x"]), one(r)), tol="sqrt")
    case("SIGNUM", lambda c: F.signum(c["x"]) * 1.0, lambda r: R.mul(R.signum(r["x"]), one(r)))
    case("FLOOR", lambda c: F.floor(x1(c)), lambda r: R.floor_long(rx1(r)), torch.int64)
    case("CEIL", lambda c: F.ceil(x1(c)), lambda r: R.ceil_long(rx1(r)), torch.int64)
    case("FLOOR_flows_on", lambda c: F.floor(c["x"]) + 0.5, lambda r: R.add(R.floor_long(r["x"]), _const(r, 0.5)))
    case("CEIL_flows_on", lambda c: F.ceil(c["x"]) + 0.5, lambda r: R.add(R.ceil_long(r["x"]), _const(r, 0.5)))
    for s in (-2, 0, 2):
        case(f"ROUND_{s}", lambda c, s=s: F.round(x1(c), s), lambda r, s=s: R.round_(rx1(r), s))
    # ---- casts
    case("TO_I32", lambda c: x1(c).cast("int"), lambda r: R.cast_int(rx1(r)), torch.int32)
    case("TO_I32_flows_on", lambda c: x1(c).cast("int") + 0.5, lambda r: R.add(R.cast_int(rx1(r)), _const(r, 0.5)))
    case("TO_I32_f32", lambda c: (c["xf"] * 1.0).cast("float").cast("int"),
         lambda r: R.cast_int(R.to_f32(R.mul(r["xf"], one(r)))), torch.int32)
    case("TO_I64", lambda c: x1(c).cast("long"), lambda r: R.cast_long(rx1(r)), torch.int64)
    case("TO_I64_flows_on", lambda c: x1(c).cast("long") + 0.5, lambda r: R.add(R.cast_long(rx1(r)), _const(r, 0.5)))
    case("WRAP_I32", lambda c: F.floor(x1(c)).cast("int"), lambda r: R.wrap32(R.floor_long(rx1(r))), torch.int32)
    case("WRAP_I32_cast", lambda c: x1(c).cast("long").cast("int"), lambda r: R.wrap32(R.cast_long(rx1(r))),
         torch.int32)
    case("I32_to_I64", lambda c: x1(c).cast("int").cast("long"), lambda r: R.cast_int(rx1(r)), torch.int64)
    case("TO_BOOL", lambda c: x1(c).cast("boolean"), lambda r: R.to_bool(rx1(r)), torch.bool)
    case("TO_F32", lambda c: x1(c).cast("float"), lambda r: R.to_f32(rx1(r)), torch.float32)
    case("TO_F64", lambda c: (c["ke"] * 1.0).cast("double") + c["l"].cast("double"),
         lambda r: R.add(R.mul(r["ke"], one(r)), R.to_double(r["l"])))
    # ---- null tests
    case("ISNULL", lambda c: F.isnull(x1(c)) | lit_f, lambda r: R.or_(R.isnull(rx1(r)), false(r)), torch.bool)
    case("ISNOTNULL", lambda c: x1(c).isNotNull() | lit_f, lambda r: R.or_(R.isnotnull(rx1(r)), false(r)), torch.bool)
    case("ISNAN", lambda c: F.isnan(x1(c)) | lit_f, lambda r: R.or_(R.isnan(rx1(r)), false(r)), torch.bool)
    case("ISNAN_i32", lambda c: F.isnan(c["ke"]) | lit_f, lambda r: R.or_(R.isnan(r["ke"]), false(r)), torch.bool)
    case("ISNULL_div", lambda c: F.isnull(c["x"] / c["y"]) | lit_f,
         lambda r: R.or_(R.isnull(R.div(r["x"], r["y"])), false(r)), torch.bool)
    case("NULL", lambda c: x1(c) + F.lit(None), lambda r: R.add(rx1(r), _null(r)))
    # ---- CASE
    case("CASE", lambda c: F.when(c["x"] > c["y"], x1(c)).when(c["p"], c["y"] * 2.0).otherwise(-1.0),
         lambda r: R.when([(R.cmp(">", r["x"], r["y"]), rx1(r)), (r["p"], R.mul(r["y"], _const(r, 2.0)))],
                          _const(r, -1.0)))
    case("CASE_no_otherwise", lambda c: F.when(c["p"], x1(c)).when(c["x"] < c["y"], c["y"] * 1.0),
         lambda r: R.when([(r["p"], rx1(r)), (R.cmp("<", r["x"], r["y"]), R.mul(r["y"], one(r)))]))
    case("CASE_first_match", lambda c: F.when(c["x"] >= c["y"], 1.0).when(c["x"] >= c["y"], 2.0).when(c["q"], 3.0)
         .otherwise(F.lit(None)) * 1.0,
         lambda r: R.mul(R.when([(R.cmp(">=", r["x"], r["y"]), _const(r, 1.0)),
                                 (R.cmp(">=", r["x"], r["y"]), _const(r, 2.0)), (r["q"], _const(r, 3.0))], _null(r)),
                         one(r)))
    case("CASE_i32", lambda c: F.when(c["x"] > 0, x1(c).cast("int")).otherwise(c["ke"]),
         lambda r: R.when([(R.cmp(">", r["x"], false(r)), R.cast_int(rx1(r)))], r["ke"]), torch.int32)

    # ---- whole expressions: the eleven of test_fused_expressions_match_operator_path on the edge table
    def c_(v):
        return lambda r: _const(r, v)
    x_, y_, k_, b_, big = (lambda c: c["x"]), (lambda c: c["xf"]), (lambda c: c["k"]), (lambda c: c["p"]), \
        (lambda c: c["l"])
    case("arith", lambda c: (x_(c) * 2.0 + y_(c)) / (k_(c) - 1.0),
         lambda r: R.div(R.add(R.mul(r["x"], c_(2.0)(r)), r["xf"]), R.sub(r["k"], one(r))))
    case("mod", lambda c: (x_(c) + 0.5) % (k_(c) * 1.0),
         lambda r: R.mod(R.add(r["x"], c_(0.5)(r)), R.mul(r["k"], one(r))))
    case("logexp", lambda c: F.exp(F.log(F.abs(x_(c)) + 1.0)) - F.log1p(y_(c) * 1.0)
         + F.sqrt(x_(c) * 1.0) * F.log10(k_(c) * 1.0),
         lambda r: R.add(R.sub(R.math_fn("exp", R.math_fn("ln", R.add(R.abs_(r["x"]), one(r)))),
                               R.math_fn("log1p", R.mul(r["xf"], one(r)))),
                         R.mul(R.math_fn("sqrt", rx1(r)), R.math_fn("log10", R.mul(r["k"], one(r))))), tol="compose")
    case("cmp3", lambda c: ((x_(c) > 0) & (y_(c) < 0.5)) | ~(k_(c) == 2),
         lambda r: R.or_(R.and_(R.cmp(">", r["x"], false(r)), R.cmp("<", r["xf"], c_(0.5)(r))),
                         R.not_(R.cmp("==", r["k"], c_(2.0)(r)))), torch.bool)
    case("when", lambda c: F.when(x_(c) > 1.0, x_(c) * 2.0).when(k_(c) < 0, y_(c) * 1.0).otherwise(-1.0) + 0.0,
         lambda r: R.add(R.when([(R.cmp(">", r["x"], one(r)), R.mul(r["x"], c_(2.0)(r))),
                                 (R.cmp("<", r["k"], false(r)), R.mul(r["xf"], one(r)))], c_(-1.0)(r)), false(r)))
    case("when_null", lambda c: F.when(b_(c), k_(c) * 1.0).when(x_(c) < 0, 3.0) * 2.0,
         lambda r: R.mul(R.when([(r["p"], R.mul(r["k"], one(r))), (R.cmp("<", r["x"], false(r)), c_(3.0)(r))]),
                         c_(2.0)(r)))
    case("casts", lambda c: (x_(c) * 3.0).cast("int") + (y_(c) * 1.0).cast("float") * 0.5,
         lambda r: R.add(R.cast_int(R.mul(r["x"], c_(3.0)(r))), R.mul(R.to_f32(R.mul(r["xf"], one(r))), c_(0.5)(r))))
    case("casts2", lambda c: ((x_(c) * 10.0).cast("long") + 1.0).cast("double") * k_(c).cast("double"),
         lambda r: R.mul(R.add(R.cast_long(R.mul(r["x"], c_(10.0)(r))), one(r)), R.to_double(r["k"])))
    case("round", lambda c: F.round(x_(c) * 1.0, 2) + F.floor(y_(c) * 3.0) - F.ceil(x_(c) * 1.0)
         + F.signum(x_(c) * 1.0),
         lambda r: R.add(R.sub(R.add(R.round_(rx1(r), 2), R.floor_long(R.mul(r["xf"], c_(3.0)(r)))),
                               R.ceil_long(rx1(r))), R.signum(rx1(r))))
    case("nulls", lambda c: F.isnull(x_(c) * 1.0) | F.isnan(x_(c) * 2.0) | (big(c) * 1.0 > 5e5),
         lambda r: R.or_(R.or_(R.isnull(rx1(r)), R.isnan(R.mul(r["x"], c_(2.0)(r)))),
                         R.cmp(">", R.mul(r["l"], one(r)), c_(5e5)(r))), torch.bool)
    case("pow", lambda c: F.pow(F.abs(x_(c)) * 1.0, 0.5) + F.sin(x_(c) * 1.0) * F.cos(y_(c) * 1.0),
         lambda r: R.add(R.pow_(R.mul(R.abs_(r["x"]), one(r)), c_(0.5)(r)),
                         R.mul(R.math_fn("sin", rx1(r)), R.math_fn("cos", R.mul(r["xf"], one(r))))), tol="compose")
    return C


def limit_programs(x):
    """[(expression, fits, reference)]: LOAD + k * (CONST, ADD) [+ NEG] is 1 + 2k [+ 1] instructions, and a
    right-nested sum of m loads needs m stack slots; the limits are 256 instructions and 16 slots."""
    def chain(k, neg):
        e = x
        for i in range(k):
            e = e + float(i)
        return -e if neg else e

    def chain_ref(k, neg):
        def ref(r):
            v = r["x"]
            for i in range(k):
                v = R.add(v, _const(r, float(i)))
            return R.neg(v) if neg else v
        return ref

    def nest(m):
        e = x
        for _ in range(m - 1):
            e = x + e
        return e

    def nest_ref(m):
        def ref(r):
            v = r["x"]
            for _ in range(m - 1):
                v = R.add(r["x"], v)
            return v
        return ref
    return [(chain(127, True), True, chain_ref(127, True)), (chain(128, False), False, chain_ref(128, False)),
            (nest(16), True, nest_ref(16)), (nest(17), False, nest_ref(17))]


def columns():
    return {k: F.col(k) for k in TYPES}
