"""The DataFrame kernels K18 expr_eval (expr.hip) and K19 compact_mask / gather, K20 col_moments, partition_dest
(relational.hip) against the plain references of tests/_frame_refs.py, at the value edges (all pairs of the edge
table, every opcode, every input and output dtype, with and without validity) and at the loop edges (a second
grid-stride trip, a block whose last round is partial in the middle of the array, the LDS limit of partition_dest).

Everything but the transcendentals is compared bit for bit.  The transcendentals are held to ``ULP``: twice the
largest distance to the correctly rounded value measured on an MI355X (profiles/r19/frame_kernels.md), never below
2 ulp; the margin covers libm changes between ROCm releases."""
import numpy as np
import pytest
import torch

from tests import _frame_cases as FC
from tests import _frame_refs as R
from cdnaml.ops import _lib, kernels as K, relops as RO
from cdnaml.sql import functions as F
from cdnaml.sql import fused
from cdnaml.sql import types as T
from cdnaml.sql.batch import Batch, ColumnData
from cdnaml.sql.column import EvalContext

pytestmark = pytest.mark.gpu

# measured maxima (ulp) over the inputs of test_transcendentals_within_measured_ulp: see the profile note
MEASURED = {"ln": 1, "log10": 0, "log2": 1, "log1p": 1, "exp": 1, "expm1": 1, "pow": 1, "sin": 1, "cos": 1, "tan": 1}
ULP = {k: max(2, 2 * v) for k, v in MEASURED.items()}
MEASURED_CHAIN = {"logexp": 0, "pow": 1}        # the whole expressions that chain transcendentals, on the edge table
CASES = FC.cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch.device("cuda")


@pytest.fixture(autouse=True)
def small_frames_reach_the_kernels(monkeypatch):
    monkeypatch.setattr(fused, "FUSE", True)
    monkeypatch.setattr(fused, "FUSE_MIN_ROWS", 0)
    monkeypatch.setattr(RO, "GATHER_MIN", 0)


@pytest.fixture(scope="module", params=[True, False], ids=["valid", "novalid"])
def frame(request, dev):
    cols = FC.make_inputs(request.param)           # 576 pairs tiled to 4608 rows: 18 blocks
    return cols, FC.to_batch(cols, dev, request.param), FC.ref_cols(cols), request.param


def run_fused(e, b):
    """``e`` through expr.hip; fails if it would fall back to the operator path."""
    assert fused.can_fuse(e, b), f"{e} does not fuse"
    return fused.evaluate(e, b, EvalContext(None)), fused._program(e, b)[0]


# ------------------------------------------------------------------------------------------ K18
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_expr_eval_matches_reference(frame, case):
    """Every opcode, and the eleven whole expressions of test_fused_expressions_match_operator_path, on all pairs of
    the edge table.  Without validity the programs that cannot produce a null run with outv == nullptr."""
    cols, b, rc, with_valid = frame
    name, mk, mkref, out_t, tol = case
    got, prog = run_fused(mk(FC.columns())._expr, b)
    ref = mkref(rc)
    assert got.values.dtype == out_t, name
    assert (got.valid is None) == (not prog.nullable), name
    if tol is None or tol == "sqrt":
        return R.same(FC.result(got), ref, name)
    # the two chains of transcendentals: twice what was measured on the edge table, never below 2 ulp; POW is
    # compared with libm's pow (at most 1 ulp off itself) on the pairs, where the special cases matter
    bound = max(2, 2 * MEASURED_CHAIN[name]) if tol == "compose" else ULP[tol] + (tol == "pow")
    g = FC.result(got)
    assert np.array_equal(g[1], ref[1]), f"{name}: validity differs at rows {np.flatnonzero(g[1] != ref[1])[:8]}"
    sel = ref[1] & FC.compared_rows(cols, tol)
    d = R.ulp_distance(g[0][sel], ref[0][sel])
    print(f"{name}: max {d.max()} ulp on the edge table")
    assert d.max() <= bound, f"{name}: {d.max()} ulp from the reference at row {np.flatnonzero(sel)[int(np.argmax(d))]}"


def test_program_limits_run(dev):
    """256 instructions and 16 stack slots run in the kernel; one more of either goes to the operator path."""
    cols = FC.make_inputs(True)
    b, rc = FC.to_batch(cols, dev), FC.ref_cols(cols)
    for e, fits, ref in FC.limit_programs(F.col("x")):
        assert fused.can_fuse(e._expr, b) == fits
        got = fused.evaluate(e._expr, b, EvalContext(None))
        R.same(FC.result(got), ref(rc), "fused" if fits else "operator path")


def _log_spaced(lo, hi, n=4096):
    return np.exp(np.linspace(np.log(lo), np.log(hi), n))


@pytest.mark.parametrize("name", FC.TRANSCENDENTAL + ("sqrt",))
def test_transcendentals_within_measured_ulp(dev, name):
    """4096 log-spaced magnitudes in [1e-300, 1e300] of either sign within the function's domain (|x| <= 1e6 for
    sin / cos / tan), against mpmath at 200 bits rounded to fp64.  sqrt is exact."""
    mag = _log_spaced(1e-300, 1e6 if name in FC.TRIG else 1e300)
    x = np.concatenate([mag, -mag])
    fns = {"ln": F.log, "log10": F.log10, "log2": F.log2, "log1p": F.log1p, "exp": F.exp, "expm1": F.expm1,
           "sin": F.sin, "cos": F.cos, "tan": F.tan, "sqrt": F.sqrt}
    if name == "pow":
        x = mag
        with np.errstate(all="ignore"):
            y = 250.0 / np.log10(x) * np.cos(np.arange(len(x)))      # results spread over [1e-250, 1e250]
        y = np.where(np.isfinite(y), y, 1.0)
        ref, ok = R.pow_values(x, y), np.ones(len(x), dtype=bool)
        e = F.pow(F.col("x"), F.col("y")) * 1.0
    else:
        y = np.zeros_like(x)
        ref = R.math_values(name, x)
        ok = ~np.isnan(ref)                       # out of the domain: null (checked on the edge table)
        e = fns[name](F.col("x")) * 1.0
    t = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
    b = Batch({"x": ColumnData(t(x), T.DoubleType()), "y": ColumnData(t(y), T.DoubleType())})
    got, _ = run_fused(e._expr, b)
    g, m = FC.result(got)
    assert np.array_equal(m, ok)
    d = R.ulp_distance(g[ok], ref[ok])
    print(f"MEASURED {name}: max {d.max()} ulp at x = {x[ok][int(np.argmax(d))]!r}")
    assert d.max() <= (0 if name == "sqrt" else ULP[name])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1_048_576 + 257])
def test_expr_eval_rows(dev, n):
    """Block and grid edges: the last size gives the grid-stride loop (4096 blocks of 256 rows) a second trip with a
    partial last block.  The row id is an operand, so a row evaluated at the wrong index shows."""
    rng = np.random.default_rng(n)
    x = rng.normal(size=n) * 5
    r = np.arange(n, dtype=np.float64)
    k = rng.integers(-3, 4, n).astype(np.int32)
    xm = rng.random(n) < 0.9
    t = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
    b = Batch({"x": ColumnData(t(x), T.DoubleType(), t(xm)), "r": ColumnData(t(r), T.DoubleType()),
               "k": ColumnData(t(k), T.IntegerType())})
    got, _ = run_fused(((F.col("x") * 2.0 + F.col("r")) / (F.col("k") - 1.0))._expr, b)
    with np.errstate(all="ignore"):
        ref = ((x * 2.0 + r) / np.where(k == 1, 1.0, k - 1.0), xm & (k != 1))
    R.same(FC.result(got), ref, f"n = {n}")


# ------------------------------------------------------------------------------------------ K19
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096, 4097, 16_777_216 + 4097])
def test_compact_mask(dev, n):
    """rows_per_block is max(4096, ceil(n / 4096)): 4097 at the last size, so every block but the first starts off
    a multiple of 256 and ends its last round partial in the middle of the array."""
    rng = np.random.default_rng(n)
    first, last = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    first[0], last[-1] = True, True
    for what, mask in [("none", np.zeros(n, dtype=bool)), ("all", np.ones(n, dtype=bool)),
                       ("half", rng.random(n) < 0.5), ("first", first), ("last", last)]:
        got = K.compact_mask(torch.from_numpy(mask).to(dev))
        ref = torch.from_numpy(R.ref_compact(mask)).to(dev)
        assert got.dtype == torch.int64 and torch.equal(got, ref), (n, what)


GATHER_DT = [np.int8, np.int16, np.int32, np.int64, np.float32, np.float64, np.bool_, np.uint8, np.float16]


@pytest.mark.parametrize("m", [1, 2047, 2048, 2049])
def test_gather_cols(dev, m):
    """All four element widths and bool in one call of nine columns (two launches), around the 8 x 256 rows of a
    block's first trip."""
    rng = np.random.default_rng(m)
    srcs = [(rng.integers(1, 100, 1000) % (2 if dt is np.bool_ else 128)).astype(dt) for dt in GATHER_DT]
    idx = rng.integers(0, 1000, m)
    idx[-1] = 999
    got = K.gather_cols([torch.from_numpy(s).to(dev) for s in srcs], torch.from_numpy(idx).to(dev))
    for s, g in zip(srcs, got):
        assert g is not None and np.array_equal(g.cpu().numpy(), R.ref_gather(s, idx, 1000)), s.dtype


def test_gather_second_trip(dev):
    """8192 blocks x 256 threads x 8 rows cover 16 777 216 rows: 2049 more enter the loop's second trip."""
    m = 16_777_216 + 2049
    src = (np.arange(1000) % 251 + 1).astype(np.uint8)
    idx = torch.randint(0, 1000, (m,), generator=torch.Generator().manual_seed(5))
    idx[-1], idx[16_777_216] = 999, 998
    got, = K.gather_cols([torch.from_numpy(src).to(dev)], idx.to(dev))
    assert torch.equal(got.cpu(), torch.from_numpy(R.ref_gather(src, idx.numpy(), 1000)))


def test_gather_sources_of_different_lengths(dev):
    """nsrc is the shortest source of the call: an index outside [0, nsrc) reads nothing and writes 0, in every
    column (GatherArgs)."""
    rng = np.random.default_rng(9)
    lens = [700, 1000, 523, 4000]
    srcs = [rng.integers(1, 100, n).astype(dt) for n, dt in zip(lens, [np.int64, np.int8, np.float32, np.int16])]
    idx = rng.integers(0, 523, 3000)
    idx[[0, 7, 2999, 1500, 64]] = [-1, 522, 523, 522, -1]
    got = K.gather_cols([torch.from_numpy(s).to(dev) for s in srcs], torch.from_numpy(idx).to(dev))
    for s, g in zip(srcs, got):
        assert np.array_equal(g.cpu().numpy(), R.ref_gather(s, idx, 523)), s.dtype


# ------------------------------------------------------------------------------------------ K20
_MOM = {}
BIG_MEAN = 6          # the column of R.moment_matrix with mean 1e8 and unit spread


def _moments_case(n, d, dtype):
    """(X wide, validity wide, reference) shared by the tests of one shape; the reference is computed once."""
    key = (n, d, dtype)
    if key not in _MOM:
        rng = np.random.default_rng(n * 1000 + d)
        if d >= 8:
            X, v = R.moment_matrix(n, d, rng)
        else:
            X, v = rng.integers(0, 2 ** 20, (n, d)) / 1024.0, rng.random((n, d)) < 0.9
        X = X.astype(dtype)                              # fp32 rounds the 1e8 column: the reference sees that
        _MOM[key] = (X, v, R.ref_moments(X.astype(np.float64), v), R.ref_moments(X.astype(np.float64)))
    return _MOM[key]


@pytest.mark.parametrize("n", [1, 255, 257, 70_001])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_col_moments(dev, dtype, d, n):
    """X and the validity mask are column slices of wider tensors with different row strides.  d = 65 and 130 give a
    last column group of one and two columns (256 and 128 row lanes)."""
    X, v, ref_v, ref = _moments_case(n, d, dtype)
    wide = torch.zeros((n, d + 7), dtype=torch.from_numpy(X).dtype)
    wide[:, 3:3 + d] = torch.from_numpy(X)
    vwide = torch.zeros((n, d + 5), dtype=torch.bool)
    vwide[:, 1:1 + d] = torch.from_numpy(v)
    Xd, vd = wide.to(dev)[:, 3:3 + d], vwide.to(dev)[:, 1:1 + d]
    assert Xd.stride(0) == d + 7 and vd.stride(0) == d + 5
    got = K.col_moments(Xd, vd)
    um, em = R.moments_close(got.cpu().numpy(), ref_v, n)
    again = K.col_moments(Xd, vd)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))      # two runs are bit-identical
    um2, em2 = R.moments_close(K.col_moments(Xd).cpu().numpy(), ref, n)
    print(f"K20 n={n} d={d} {np.dtype(dtype).name}: mean {max(um, um2)} ulp, M2 rel {max(em, em2):.3g}")


@pytest.mark.parametrize("n", [255, 257, 70_001])
def test_col_moments_m2_of_a_large_mean(dev, n):
    """The column with mean 1e8 and unit spread, held to the same 4 ulp + 4 n eps M2 as every other column: Welford
    on x - mean would carry the rounding of a mean near 1e8 (1.5e-8) into every delta and miss it by four orders of
    magnitude (6.35e-07 against 1.87e-11 at n = 255); the kernel accumulates x minus the column's first value."""
    X, v, ref_v, _ = _moments_case(n, 65, np.float64)
    got = K.col_moments(torch.from_numpy(X).to(dev), torch.from_numpy(v).to(dev)).cpu().numpy()
    err, tol = abs(got[BIG_MEAN, 2] - ref_v[BIG_MEAN, 2]), R.m2_tolerance(ref_v[BIG_MEAN, 2], n)
    print(f"K20 large mean n={n}: M2 {ref_v[BIG_MEAN, 2]!r}, off by {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol


def test_col_moments_integer_input(dev):
    """An int32 X (converted to fp64 by the wrapper), non-negative so that the mean is well-conditioned, under the
    same per-column bounds as every other K20 case; one column is signed with a mean far from zero."""
    rng = np.random.default_rng(4)
    X = rng.integers(0, 2000, (257, 65)).astype(np.int32)
    X[:, 5] = rng.integers(-3000, -1000, 257)
    v = rng.random(X.shape) < 0.8
    got = K.col_moments(torch.from_numpy(X).to(dev), torch.from_numpy(v).to(dev)).cpu().numpy()
    R.moments_close(got, R.ref_moments(X.astype(np.float64), v), 257)


# ------------------------------------------------------------------------------------------ partition_dest
@pytest.mark.parametrize("n", [1, 1023, 1025, 2_097_152 + 1031])
@pytest.mark.parametrize("W", [1, 2, 64, 8192, 8193])
def test_partition_dest(dev, W, n):
    """rows_per_block is max(1024, ceil(n / 2048)): 1025 at the last size.  W = 8192 fills the 32 KiB of LDS and
    W = 8193 takes the torch fallback, with the same result."""
    rng = np.random.default_rng(n + W)
    r = np.arange(n)
    pats = {"one bucket": np.full(n, W - 1), "lanes apart": r % min(W, 64), "random": rng.integers(0, W, n)}
    if W > 1:
        pats["an empty bucket"] = rng.integers(1, W, n)
    for what, dest in pats.items():
        dest = dest.astype(np.int32)
        perm, cnt = K.partition_dest(torch.from_numpy(dest).to(dev), W)
        rp, rc = R.ref_partition_dest(dest, W)
        assert torch.equal(perm, torch.from_numpy(rp).to(dev)), (what, W, n)
        assert torch.equal(cnt, torch.from_numpy(rc).to(dev)), (what, W, n)
