"""The host formulation of the K28 radix select (``K.col_quantiles``, ``K.col_digit_hist``, ``K.col_extrema``) against
the plain numpy references of ``tests/_quantile_refs.py``, bit for bit, and RobustScaler / MaxAbsScaler on top.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import _lib, kernels as K
from tests import _quantile_refs as R

NINE = [0.0, 0.1, 0.2, 0.3, 0.5, 0.7, 0.8, 0.9, 1.0]          # Q > 8
PROBS = [[0.5], [0.25, 0.5, 0.75], [0.0, 1.0], NINE]


def to_np(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


# ------------------------------------------------------------------------------------------------ host formulation
@pytest.mark.parametrize("d", [1, 5, 129])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1025])
def test_host_quantiles_equal_the_reference(n, d):
    X = R.menu_case(d, n)
    Xt = torch.tensor(X)
    assert K.col_quantiles_plan(Xt, 3)["path"] == "host"
    for probs in PROBS:
        R.assert_quantiles(to_np(K.col_quantiles(Xt, probs)), R.quantiles(X, probs))
    ext = to_np(K.col_extrema(Xt))
    ref = R.quantiles(X, [0.5])
    assert R.same_bits(ext["min"], ref["min"]) and R.same_bits(ext["max"], ref["max"])
    assert np.array_equal(ext["count"], ref["count"]) and np.array_equal(ext["nan"], ref["nan"])


def test_host_quantiles_in_chunks_and_without_rows(monkeypatch):
    X = R.menu_case(13, 130)
    monkeypatch.setattr(K, "LABEL_HOST_CHUNK", 48)
    R.assert_quantiles(to_np(K.col_quantiles(torch.tensor(X), [0.25, 0.5, 0.75])), R.quantiles(X, [0.25, 0.5, 0.75]))
    for dt in (np.float32, np.float64):
        E = np.zeros((0, 4), dtype=dt)
        R.assert_quantiles(to_np(K.col_quantiles(torch.tensor(E), [0.0, 0.5])), R.quantiles(E, [0.0, 0.5]))


@pytest.mark.parametrize("m", [1, 2, 8, 100, 1000])
def test_ranks_at_exact_products_and_at_the_ends(m):
    """q m an exact integer (q = j / m for m a power of two or q a dyadic fraction), and q giving rank 1 and rank m."""
    rng = np.random.default_rng(m)
    X = rng.permutation(m).astype(np.float32)[:, None] * np.ones((1, 2), np.float32)
    X[:, 1] *= -1
    probs = [0.0, 1.0 / (2 * m), 1.0 / m, 0.25, 0.5, 0.75, (m - 1) / m, 1.0 - 1.0 / (4 * m), 1.0]
    assert [R.rank_of(p, m) for p in (0.0, 1.0 / (2 * m), 1.0 / m)] == [1, 1, 1]
    assert R.rank_of(1.0, m) == m and R.rank_of(1.0 - 1.0 / (4 * m), m) == m
    if m % 4 == 0:
        assert [R.rank_of(p, m) for p in (0.25, 0.5, 0.75)] == [m // 4, m // 2, 3 * m // 4]
    got = to_np(K.col_quantiles(torch.tensor(X), probs))
    R.assert_quantiles(got, R.quantiles(X, probs))
    assert got["q"][0, 0] == 0 and got["q"][-1, 0] == m - 1 and got["q"][0, 1] == -(m - 1)


@pytest.mark.parametrize("bad", [[-0.1], [1.5], [float("nan")], []])
def test_probabilities_outside_the_unit_interval_raise(bad):
    with pytest.raises(ValueError):
        K.col_quantiles(torch.zeros((3, 2)), bad)


@pytest.mark.parametrize("d,n", [(1, 1), (5, 65), (7, 1025)])
def test_fp64_values_that_differ_below_fp32_precision(d, n):
    X = R.fine_case64(d, n)
    Xt = torch.tensor(X)
    assert Xt.dtype == torch.float64 and K.col_quantiles_plan(Xt, 3) == {"path": "host", "widths": [8] * 8}
    for probs in PROBS:
        got = K.col_quantiles(Xt, probs)
        assert got["q"].dtype == torch.float64
        R.assert_quantiles(to_np(got), R.quantiles(X, probs))
    if n > 2:
        q = K.col_quantiles(Xt, [0.0, 1.0])["q"][:, 0]
        assert float(q[0]) < float(q[1]) and np.float32(q[0]) == np.float32(q[1])


def test_fp64_menu_equals_the_reference():
    X = R.menu_case(12, 257).astype(np.float64)
    R.assert_quantiles(to_np(K.col_quantiles(torch.tensor(X), [0.25, 0.5, 0.75])), R.quantiles(X, [0.25, 0.5, 0.75]))


# ------------------------------------------------------------------------------------------------ one pass
def assert_hist(got, ref):
    got = to_np(got)
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])


@pytest.mark.parametrize("bits", range(1, 9))
def test_digit_hist_host_model_equals_bincount(bits):
    d, n = 13, 300
    X = R.menu_case(d, n)
    Xt = torch.tensor(X)
    assert_hist(K.col_digit_hist(Xt, bits, 32 - bits), R.digit_hist(X, bits, 32 - bits))
    assert int(K.col_digit_hist(Xt, bits, 32 - bits)["hist"].sum()) == int((~np.isnan(X)).sum())
    probs = [0.25, 0.5, 0.75]
    # a middle digit, and the last digit (shift = 0), below the prefixes of the true quantiles
    for shift in (32 - 8 - bits, 0):
        pre = R.prefixes(X, probs, 32 - shift - bits)
        ref = R.digit_hist(X, bits, shift, pre)
        assert_hist(K.col_digit_hist(Xt, bits, shift, torch.tensor(pre)), ref)
        assert ref["hist"][0].sum() > 0


def test_digit_hist_last_partial_digit_and_shared_prefixes():
    d, n = 13, 300
    X = R.menu_case(d, n)
    pre = R.prefixes(X, [0.25, 0.5, 0.75], 31)
    shared = [c for c in range(d) if pre[c, 0] == pre[c, 1] == pre[c, 2] and not np.isnan(X[:, c]).all()]
    assert 1 in shared                                              # the constant column
    ref = R.digit_hist(X, 1, 0, pre)
    got = K.col_digit_hist(torch.tensor(X), 1, 0, torch.tensor(pre))
    assert_hist(got, ref)
    h = got["hist"].numpy()
    assert np.array_equal(h[1, 0], h[1, 1]) and np.array_equal(h[1, 1], h[1, 2]) and h[1, 0].sum() == n


def test_digit_hist_rejects_shifts_outside_the_key():
    X = torch.zeros((4, 2))
    pre = torch.zeros((2, 1), dtype=torch.int64)
    for bits, shift, p in [(8, 23, None), (8, 25, None), (0, 32, None), (9, 23, None), (8, 24, pre), (4, -1, pre)]:
        with pytest.raises(ValueError):
            K.col_digit_hist(X, bits, shift, p)
    with pytest.raises(ValueError):
        K.col_digit_hist(X, 4, 0, torch.zeros((3, 1), dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ the plan's widths
def plan_widths(d, Q):
    """Through the host plan function where the library loads, else the pure-Python mirror (tests/test_quantile_gpu.py
    asserts that the two agree)."""
    if not _lib.available():
        return K.col_quantile_widths(d, Q)
    out = np.zeros(40, dtype=np.int64)
    _lib.check(_lib.lib().cdna_col_quantiles_plan(None, 1025, d, d, Q, out.ctypes.data), "cdna_col_quantiles_plan")
    assert out[0] == 1
    return [int(v) for v in out[8:8 + int(out[7])]]


def max_bits(d, Q):
    return max(b for b in range(0, 9) if Q * 2 ** b * (d | 1) * 4 <= 96 * 1024)


@pytest.mark.parametrize("d", [1, 5, 31, 64, 100, 127, 128])
@pytest.mark.parametrize("Q", [1, 2, 3, 8])
def test_plan_widths(d, Q):
    w = plan_widths(d, Q)
    assert w == K.col_quantile_widths(d, Q)
    assert sum(w) == 32 and w[0] == max_bits(d, 1)
    assert all(b == max_bits(d, Q) for b in w[1:-1]) and 1 <= w[-1] <= max_bits(d, Q)
    assert 2 ** w[0] * (d | 1) * 4 <= 96 * 1024 and Q * 2 ** max(w[1:]) * (d | 1) * 4 <= 96 * 1024     # table bytes
    assert max_bits(d, Q) >= 4


def test_plan_widths_of_the_headline_shape():
    assert plan_widths(100, 3) == [7, 6, 6, 6, 6, 1]
    assert K.col_quantiles_plan(torch.zeros((4, 100)), 3) == {"path": "host", "widths": [8, 8, 8, 8]}


# ------------------------------------------------------------------------------------------------ the existing path
def test_cross_check_with_approx_quantile(spark):
    """Five columns, none holding zeros of both signs (the existing path sorts values, not keys)."""
    kinds = ("gauss", "two", "onehot", "inf", "big")
    X = R.menu_case(5, 257, kinds=kinds)
    df = spark.createDataFrame(pd.DataFrame(X.astype(np.float64), columns=list(kinds)))
    got = K.col_quantiles(torch.tensor(X, device=spark.device), [0.25, 0.5, 0.75])["q"].cpu().numpy()
    for c, name in enumerate(kinds):
        assert df.approxQuantile(name, [0.25, 0.5, 0.75], 0) == [float(v) for v in got[:, c]], name


# ------------------------------------------------------------------------------------------------ RobustScaler
def vector_frame(spark, X, names=None):
    from cdnaml.ml.feature import VectorAssembler
    names = names or [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X.astype(np.float64), columns=names)
    return VectorAssembler(inputCols=names, outputCol="features", handleInvalid="keep") \
        .transform(spark.createDataFrame(pdf))                      # keep: the NaNs stay in the vectors


def column_values(df, name):
    from cdnaml.models.util import local_batch
    return local_batch(df, [name]).columns[name].values


SCALER_KINDS = ("gauss", "const", "two", "onehot", "allnan", "nan30", "big")


@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_robust_scaler_fit_and_transform(spark, precision):
    from cdnaml.ml.feature import RobustScaler, RobustScalerModel
    X = R.menu_case(len(SCALER_KINDS), 301, kinds=SCALER_KINDS)
    spark.conf.set("cdnaml.ml.vectorPrecision", precision)
    try:
        df = vector_frame(spark, X, list(SCALER_KINDS))
        dt = torch.float32 if precision == "fp32" else torch.float64
        Xv = column_values(df, "features")
        assert Xv.dtype == dt
        med, rng = R.robust_reference(X if precision == "fp32" else X.astype(np.float64), 0.2, 0.9)
        assert rng[1] == 0 and np.isnan(rng[4]) and np.isnan(med[4])          # the constant, the all-NaN column
        for wc in (False, True):
            for ws in (False, True):
                m = RobustScaler(inputCol="features", outputCol="out", lower=0.2, upper=0.9, withCentering=wc,
                                 withScaling=ws).fit(df)
                assert type(m) is RobustScalerModel
                assert R.same_bits(m.median.toArray(), med) and R.same_bits(m.range.toArray(), rng)
                out = m.transform(df)
                Y = column_values(out, "out")
                assert Y.dtype == dt                                            # Float stays Float, Double Double
                want = Xv.clone()
                if wc:
                    want = want - torch.tensor(med).to(Xv)
                if ws:
                    with np.errstate(divide="ignore"):
                        want = want * torch.tensor(np.where(rng == 0, 0.0, 1.0 / rng)).to(Xv)
                assert R.same_bits(Y.cpu().numpy(), want.cpu().numpy())
                if ws:
                    assert float(Y[:, 1].abs().max()) == 0.0                    # zero range gives 0
                    assert bool(torch.isnan(Y[:, 4]).all())
                meta = out.schema["out"].metadata
                assert meta == df.schema["features"].metadata and "ml_attr" in meta
    finally:
        spark.conf.set("cdnaml.ml.vectorPrecision", "auto")


def test_robust_scaler_defaults_and_bad_params(spark):
    from cdnaml.ml.feature import RobustScaler
    from cdnaml.models.util import IllegalArgumentException
    r = RobustScaler()
    assert (r.getLower(), r.getUpper(), r.getWithCentering(), r.getWithScaling(), r.getRelativeError()) == \
        (0.25, 0.75, False, True, 0.001)
    df = vector_frame(spark, R.menu_case(3, 40))
    for kw in (dict(lower=0.0), dict(upper=1.0), dict(lower=0.6, upper=0.4), dict(lower=0.5, upper=0.5),
               dict(relativeError=-0.1), dict(relativeError=1.5)):
        with pytest.raises(IllegalArgumentException):
            RobustScaler(inputCol="features", outputCol="o", **kw).fit(df)
    m = RobustScaler(inputCol="features", outputCol="o", relativeError=1.0).fit(df)     # exact meets any bound
    med, rng = R.robust_reference(R.menu_case(3, 40).astype(np.float64))
    assert R.same_bits(m.median.toArray(), med) and R.same_bits(m.range.toArray(), rng)


def test_robust_scaler_persistence_and_pipeline(spark, tmp_path):
    from cdnaml.ml import Pipeline, PipelineModel
    from cdnaml.ml.feature import RobustScaler, RobustScalerModel, VectorAssembler
    X = R.menu_case(4, 120, kinds=("gauss", "two", "big", "const"))
    df = vector_frame(spark, X)
    m = RobustScaler(inputCol="features", outputCol="o", withCentering=True).fit(df)
    m.write().overwrite().save(str(tmp_path / "rs"))
    back = RobustScalerModel.load(str(tmp_path / "rs"))
    assert type(back) is RobustScalerModel and back.getWithCentering() and back.getOutputCol() == "o"
    assert R.same_bits(back.median.toArray(), m.median.toArray())
    assert R.same_bits(back.range.toArray(), m.range.toArray())
    a, b = (column_values(s.transform(df), "o").cpu().numpy() for s in (m, back))
    assert R.same_bits(a, b)
    names = [f"x{i}" for i in range(4)]
    raw = spark.createDataFrame(pd.DataFrame(X.astype(np.float64), columns=names))
    pm = Pipeline(stages=[VectorAssembler(inputCols=names, outputCol="features"),
                          RobustScaler(inputCol="features", outputCol="o", withCentering=True)]).fit(raw)
    assert R.same_bits(pm.stages[-1].median.toArray(), m.median.toArray())
    pm.write().overwrite().save(str(tmp_path / "pipe"))
    pb = PipelineModel.load(str(tmp_path / "pipe"))
    assert isinstance(pb.stages[-1], RobustScalerModel)
    assert R.same_bits(column_values(pb.transform(raw), "o").cpu().numpy(), a)


def test_pyspark_aliases():
    import cdnaml.compat
    cdnaml.compat.install()
    from pyspark.ml.feature import MaxAbsScaler, MaxAbsScalerModel, RobustScaler, RobustScalerModel
    from cdnaml.ml import feature
    assert RobustScaler is feature.RobustScaler and RobustScalerModel is feature.RobustScalerModel
    assert MaxAbsScaler is feature.MaxAbsScaler and MaxAbsScalerModel is feature.MaxAbsScalerModel


# ------------------------------------------------------------------------------------------------ MaxAbsScaler
@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_max_abs_scaler(spark, tmp_path, precision):
    from cdnaml.ml.feature import MaxAbsScaler, MaxAbsScalerModel
    kinds = ("gauss", "nan30", "allnan", "big", "sign")
    X = np.concatenate([R.menu_case(5, 200, kinds=kinds), np.zeros((200, 1), np.float32)], axis=1)    # a zero column
    spark.conf.set("cdnaml.ml.vectorPrecision", precision)
    try:
        df = vector_frame(spark, X)
        Xv = column_values(df, "features")
        want = R.max_abs_reference(X)
        assert want[2] == 0 and want[5] == 0 and want[4] == 2.5 and want[0] == np.abs(X[:, 0]).max()
        m = MaxAbsScaler(inputCol="features", outputCol="o").fit(df)
        assert type(m) is MaxAbsScalerModel and R.same_bits(m.maxAbs.toArray(), want)
        out = m.transform(df)
        Y = column_values(out, "o")
        assert Y.dtype == Xv.dtype
        assert R.same_bits(Y.cpu().numpy(), (Xv / torch.tensor(np.where(want != 0, want, 1.0)).to(Xv)).cpu().numpy())
        assert float(Y[:, 0].abs().max()) == 1.0 and float(Y[:, 5].abs().max()) == 0.0
        assert out.schema["o"].metadata == df.schema["features"].metadata
        m.write().overwrite().save(str(tmp_path / "ma"))
        back = MaxAbsScalerModel.load(str(tmp_path / "ma"))
        assert R.same_bits(back.maxAbs.toArray(), want) and back.getOutputCol() == "o"
        assert R.same_bits(column_values(back.transform(df), "o").cpu().numpy(), Y.cpu().numpy())
    finally:
        spark.conf.set("cdnaml.ml.vectorPrecision", "auto")
