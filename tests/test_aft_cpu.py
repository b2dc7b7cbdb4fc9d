"""AFTSurvivalRegression (pyspark.ml) and the K26 ``aft_step`` op's host formulation.

* the host formulation against the longdouble reference of ``tests/_aft_refs.py`` under its criterion (at most M = 8
  times the error of the plain numpy fp64 yardstick, floor 4 fp64 ulps of the largest entry), the gradient against
  finite differences, the bad-row rule and the overflow rule;
* the estimator against scipy's L-BFGS-B on the same objective;
* the estimator's and the model's API: params, validation, quantiles, persistence, Pipeline, CrossValidator, the
  pyspark aliases.
"""
import math

import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _aft_refs as R

SHAPES = [(5, 1), (5, 130), (1, 130), (33, 600), (100, 1100), (129, 300)]     # (d, n)


def frame(spark, X, t, censor):
    from cdnaml.ml.feature import VectorAssembler
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(np.asarray(X, dtype=np.float64), columns=names)
    pdf["label"] = t
    pdf["censor"] = censor
    return VectorAssembler(inputCols=names, outputCol="features", handleInvalid="keep").transform(
        spark.createDataFrame(pdf))


def vectors(pdf_col):
    return np.stack([np.asarray(v.toArray() if hasattr(v, "toArray") else v) for v in pdf_col])


def params(m):
    return np.concatenate([m.coefficients.toArray(), [m.intercept, math.log(m.scale)]])


def step(c, X=None, **kw):
    X = torch.from_numpy(c["X"]) if X is None else X
    return K.aft_step(X, torch.from_numpy(c["logt"]), torch.from_numpy(c["censor"]), c["coef"], c["b0"], c["ls"], **kw)


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("d,n", SHAPES)
def test_host_formulation_matches_reference(d, n, f64):
    c = R.case(d, n)
    X = torch.from_numpy(c["X"])
    X = X.double() if f64 else X
    assert K.aft_plan(X) == {"path": "host"}
    ls, g, bad = step(c, X)
    assert g.dtype == torch.float64 and g.shape == (d + 2,) and float(bad) == 0.0
    tag = f"host d={d} n={n} f64={f64}"
    R.check(tag + " loss", float(ls), c["loss"], c["y_loss"])
    R.check(tag + " grad", g.numpy(), c["grad"], c["y_grad"])
    pred, quant = step(c, X, mode=K.AFT_PREDICT, probs=R.PROBS)
    assert pred.shape == (n,) and quant.shape == (n, 9) and pred.dtype == quant.dtype == torch.float64
    R.check(tag + " pred", pred.numpy(), c["pred"], c["y_pred"])
    R.check(tag + " quant", quant.numpy(), c["quant"], c["y_quant"])
    assert torch.equal(step(c, X, mode=K.AFT_PREDICT), pred)


def test_chunked_passes_and_an_empty_shard(monkeypatch):
    c = R.case(5, 130)
    whole = step(c)
    monkeypatch.setattr(K, "AFT_HOST_CHUNK", 48)
    parts = step(c)
    R.check("chunked loss", float(parts[0]), c["loss"], c["y_loss"])
    R.check("chunked grad", parts[1].numpy(), c["grad"], c["y_grad"])
    assert float(parts[2]) == float(whole[2]) == 0.0
    assert step(c, mode=K.AFT_PREDICT).shape == (130,)
    e = torch.zeros(0, dtype=torch.float64)
    ls, g, bad = K.aft_step(torch.zeros((0, 5)), e, e, np.zeros(5), 0.0, 0.0)
    assert float(ls) == 0.0 and not g.any() and g.shape == (7,) and float(bad) == 0.0
    pred, quant = K.aft_step(torch.zeros((0, 5)), None, None, np.zeros(5), 0.0, 0.0, K.AFT_PREDICT, [0.5])
    assert pred.shape == (0,) and quant.shape == (0, 1)


@pytest.mark.parametrize("d,n", [(3, 40), (33, 200)])
def test_gradient_matches_finite_differences(d, n):
    """scipy's check_grad (forward differences, h = 1.5e-8) on the op's sums: truncation h |f''| / 2 and rounding
    eps |f| / h are both ~1e-8 of the sums' size per entry; the 2-norm of the gap must be within 1e-5 |g|."""
    from scipy.optimize import check_grad
    c = R.case(d, n)
    X, lt, dl = torch.from_numpy(c["X"]), torch.from_numpy(c["logt"]), torch.from_numpy(c["censor"])
    f = lambda th: float(K.aft_step(X, lt, dl, th[:d], th[d], th[d + 1])[0])        # noqa: E731
    g = lambda th: K.aft_step(X, lt, dl, th[:d], th[d], th[d + 1])[1].numpy()         # noqa: E731
    th = np.concatenate([c["coef"], [c["b0"], c["ls"]]])
    gap, size = check_grad(f, g, th), float(np.linalg.norm(g(th)))
    print(f"aft fd d={d} n={n}: |fd - g| / |g| = {gap / size:.2e}")
    assert gap <= 1e-5 * size


BAD_KINDS = ["label zero", "label negative", "label nan", "censor half", "feature nan", "feature inf"]


def plant(c, kinds, rows):
    """Copies of the case's X, t and censor with one bad row of each kind planted at ``rows``."""
    X, t, dl = c["X"].copy(), c["t"].copy(), c["censor"].copy()
    for kind, r in zip(kinds, rows):
        if kind == "label zero":
            t[r] = 0.0
        elif kind == "label negative":
            t[r] = -1.5
        elif kind == "label nan":
            t[r] = np.nan
        elif kind == "censor half":
            dl[r] = 0.5
        elif kind == "feature nan":
            X[r, X.shape[1] // 2] = np.nan
        else:
            X[r, 0] = np.inf
    return X, t, dl


def test_bad_rows_are_counted_and_add_nothing():
    c = R.case(5, 130)
    rows = [0, 17, 63, 64, 100, 129]
    X, t, dl = plant(c, BAD_KINDS, rows)
    keep = np.ones(130, dtype=bool)
    keep[rows] = False
    rl, rg, _, _ = R.reference(c["X"], c["t"], c["censor"], c["coef"], c["b0"], c["ls"], keep=keep)
    yl, yg, _, _ = R.yardstick(c["X"], c["t"], c["censor"], c["coef"], c["b0"], c["ls"], keep=keep)
    with np.errstate(divide="ignore", invalid="ignore"):
        lt = torch.from_numpy(np.log(t))
    ls, g, bad = K.aft_step(torch.from_numpy(X), lt, torch.from_numpy(dl), c["coef"], c["b0"], c["ls"])
    assert float(bad) == len(rows)
    R.check("bad rows loss", float(ls), rl, yl)
    R.check("bad rows grad", g.numpy(), rg, yg)


def test_overflow_is_reported_as_bad_rows_with_finite_sums():
    """log sigma = -8 puts eps past 710 on the rows with a positive residual: e^eps overflows there, the rows are
    counted as bad and the other sums stay finite."""
    c = R.case(5, 130)
    eps = (c["logt"] - c["X"].astype(np.float64) @ c["coef"] - c["b0"]) / math.exp(-8.0)
    over = int((eps > 710).sum())
    assert 0 < over < 130
    ls, g, bad = K.aft_step(torch.from_numpy(c["X"]), torch.from_numpy(c["logt"]), torch.from_numpy(c["censor"]),
                            c["coef"], c["b0"], -8.0)
    assert over <= float(bad) < 130 and np.isfinite(float(ls)) and torch.isfinite(g).all()


def test_op_errors():
    X = torch.zeros((4, 3))
    v = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="coefficients"):
        K.aft_step(X, v, v, np.zeros(2), 0.0, 0.0)
    with pytest.raises(ValueError, match="mode"):
        K.aft_step(X, v, v, np.zeros(3), 0.0, 0.0, mode=2)
    with pytest.raises(ValueError, match=r"\[n\]"):
        K.aft_step(X, v[:3], v, np.zeros(3), 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("n,d", [(200, 3), (3000, 33)])
def test_fit_matches_scipy(spark, n, d):
    from cdnaml.ml.regression import AFTSurvivalRegression
    X, t, dl, _, _ = R.make_data(d, n, dtype=np.float64)
    want, _ = R.scipy_fit(X, t, dl)
    m = AFTSurvivalRegression(tol=1e-14, maxIter=500).fit(frame(spark, X, t, dl))
    got = params(m)
    _, g = R.objective(got, X, np.log(t), dl)
    print(f"aft fit n={n} d={d}: |theta - scipy's| {np.abs(got - want).max():.2e}, |mean-loss gradient| "
          f"{np.abs(g).max():.2e}")
    assert m.numFeatures == d and np.abs(got - want).max() <= 1e-6
    assert np.abs(g).max() <= 1e-6


def test_default_tolerance_fit(spark):
    from cdnaml.ml.regression import AFTSurvivalRegression
    n, d = 5000, 20
    X, t, dl, beta, b = R.make_data(d, n, dtype=np.float64)
    _, fmin = R.scipy_fit(X, t, dl)
    m = AFTSurvivalRegression().fit(frame(spark, X, t, dl))
    f, _ = R.objective(params(m), X, np.log(t), dl)
    gap = np.abs(m.coefficients.toArray() - beta).max()
    print(f"aft default tol: loss {f:.12f} scipy {fmin:.12f} rel {abs(f - fmin) / abs(fmin):.2e}, |coef - generating| "
          f"{gap:.3f}, scale {m.scale:.3f}")
    assert abs(f - fmin) <= 1e-7 * abs(fmin)
    assert gap <= 0.1


def test_fit_without_intercept(spark):
    from cdnaml.ml.regression import AFTSurvivalRegression
    X, t, dl, _, _ = R.make_data(3, 200, dtype=np.float64)
    want, _ = R.scipy_fit(X, t, dl, fit_intercept=False)
    m = AFTSurvivalRegression(fitIntercept=False, tol=1e-14, maxIter=500).fit(frame(spark, X, t, dl))
    assert m.intercept == 0.0 and want[3] == 0.0
    assert np.abs(params(m) - want).max() <= 1e-6


def test_zero_std_column_gets_coefficient_zero(spark):
    from cdnaml.ml.regression import AFTSurvivalRegression
    X, t, dl, _, _ = R.make_data(3, 200, dtype=np.float64)
    Xc = np.concatenate([X[:, :2], np.full((200, 1), 4.0), X[:, 2:]], 1)
    m = AFTSurvivalRegression(tol=1e-14, maxIter=500).fit(frame(spark, Xc, t, dl))
    want, _ = R.scipy_fit(X, t, dl)
    got = params(m)
    assert got[2] == 0.0
    assert np.abs(np.delete(got, 2) - want).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ API
def test_params_and_defaults():
    from cdnaml.ml.regression import AFTSurvivalRegression
    from cdnaml.models.util import IllegalArgumentException
    e = AFTSurvivalRegression()
    assert (e.getFeaturesCol(), e.getLabelCol(), e.getPredictionCol(), e.getCensorCol()) == \
        ("features", "label", "prediction", "censor")
    assert e.getQuantileProbabilities() == R.PROBS and e.getQuantilesCol() is None
    assert (e.getFitIntercept(), e.getMaxIter(), e.getTol(), e.getAggregationDepth(), e.getMaxBlockSizeInMB()) == \
        (True, 100, 1e-6, 2, 0.0)
    assert not hasattr(e, "getWeightCol") and not hasattr(e, "getRegParam")
    e.setCensorCol("c").setQuantilesCol("q").setQuantileProbabilities([0.5])
    assert (e.getCensorCol(), e.getQuantilesCol(), e.getQuantileProbabilities()) == ("c", "q", [0.5])
    for probs in ([0.0, 0.5], [0.5, 1.0], [-0.1], [1.5], []):
        with pytest.raises(IllegalArgumentException, match="quantileProbabilities"):
            AFTSurvivalRegression(quantileProbabilities=probs)


def test_predictions_and_quantiles_are_the_closed_form(spark):
    from cdnaml.ml.linalg import DenseVector, Vectors
    from cdnaml.ml.regression import AFTSurvivalRegression
    X, t, dl, _, _ = R.make_data(4, 300, dtype=np.float64)
    df = frame(spark, X, t, dl)
    m = AFTSurvivalRegression(maxIter=20).fit(df)
    assert isinstance(m.coefficients, DenseVector) and isinstance(m.intercept, float) and m.scale > 0
    want = np.exp(X @ m.coefficients.toArray() + m.intercept)
    # quantilesCol unset: no column
    out = m.transform(df)
    assert "quantiles" not in out.columns and set(out.columns) >= {"prediction", "features", "censor"}
    got = out.select("prediction").toPandas().prediction.to_numpy()
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    for probs in (R.PROBS, [0.5], list(np.linspace(0.02, 0.98, 20))):          # 20: past the kernel's 16
        qf = np.exp(m.scale * np.log(-np.log1p(-np.asarray(probs))))
        mq = m.copy().setQuantilesCol("q").setQuantileProbabilities(probs)
        res = mq.transform(df).select("prediction", "q").toPandas()
        q = vectors(res.q)
        assert q.shape == (300, len(probs)) and q.dtype == np.float64
        np.testing.assert_allclose(res.prediction.to_numpy(), want, rtol=1e-13, atol=0)
        np.testing.assert_allclose(q, want[:, None] * qf[None, :], rtol=1e-13, atol=0)
        for i in (0, 299):
            v = Vectors.dense(X[i])
            assert abs(mq.predict(v) - want[i]) <= 1e-13 * want[i]
            pq = mq.predictQuantiles(v)
            assert isinstance(pq, DenseVector)
            np.testing.assert_allclose(pq.toArray(), want[i] * qf, rtol=1e-13, atol=0)
    assert np.all(np.diff(q, axis=1) > 0)                                      # quantiles increase with p
    empty = m.copy().setQuantilesCol("q").transform(df.filter("label < 0"))
    assert empty.count() == 0 and {"prediction", "q"} <= set(empty.columns)


def test_persistence_alone_and_in_a_pipeline(spark, tmp_path):
    from cdnaml.ml import Pipeline, PipelineModel
    from cdnaml.ml.feature import VectorAssembler
    from cdnaml.ml.regression import AFTSurvivalRegression, AFTSurvivalRegressionModel
    X, t, dl, _, _ = R.make_data(3, 150, dtype=np.float64)
    df = frame(spark, X, t, dl)
    m = AFTSurvivalRegression(maxIter=15, quantilesCol="q", quantileProbabilities=[0.25, 0.75]).fit(df)
    m.write().overwrite().save(str(tmp_path / "aft"))
    back = AFTSurvivalRegressionModel.load(str(tmp_path / "aft"))
    assert back.getQuantilesCol() == "q" and back.getQuantileProbabilities() == [0.25, 0.75]
    assert np.array_equal(params(back), params(m)) and back.scale == m.scale and back.numFeatures == 3
    a, b = (s.transform(df).select("prediction", "q").toPandas() for s in (m, back))
    assert np.array_equal(a.prediction.to_numpy(), b.prediction.to_numpy())
    assert np.array_equal(vectors(a.q), vectors(b.q))
    est = AFTSurvivalRegression(censorCol="c", fitIntercept=False, quantileProbabilities=[0.5])
    est.write().overwrite().save(str(tmp_path / "est"))
    e2 = AFTSurvivalRegression.load(str(tmp_path / "est"))
    assert (e2.getCensorCol(), e2.getFitIntercept(), e2.getQuantileProbabilities()) == ("c", False, [0.5])
    names = [f"x{i}" for i in range(3)]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"], pdf["censor"] = t, dl
    raw_df = spark.createDataFrame(pdf)
    pm = Pipeline(stages=[VectorAssembler(inputCols=names, outputCol="features"),
                          AFTSurvivalRegression(maxIter=15)]).fit(raw_df)
    pm.write().overwrite().save(str(tmp_path / "pipe"))
    pb = PipelineModel.load(str(tmp_path / "pipe"))
    assert isinstance(pb.stages[-1], AFTSurvivalRegressionModel)
    assert np.array_equal(pb.transform(raw_df).select("prediction").toPandas().prediction.to_numpy(),
                          pm.transform(raw_df).select("prediction").toPandas().prediction.to_numpy())


def test_pyspark_alias_and_cross_validator(spark):
    from cdnaml import compat
    compat.install()
    try:
        from pyspark.ml.evaluation import RegressionEvaluator
        from pyspark.ml.regression import AFTSurvivalRegression, AFTSurvivalRegressionModel
        from pyspark.ml.tuning import CrossValidator, ParamGridBuilder
        X, t, dl, _, _ = R.make_data(3, 300, dtype=np.float64)
        est = AFTSurvivalRegression()
        grid = ParamGridBuilder().addGrid(est.maxIter, [0, 50]).build()
        cv = CrossValidator(estimator=est, estimatorParamMaps=grid, numFolds=2, seed=5,
                            evaluator=RegressionEvaluator(metricName="rmse")).fit(frame(spark, X, t, dl))
        assert isinstance(cv.bestModel, AFTSurvivalRegressionModel) and len(cv.avgMetrics) == 2
        assert np.isfinite(cv.avgMetrics).all() and cv.avgMetrics[1] != cv.avgMetrics[0]
    finally:
        compat.uninstall()


@pytest.mark.parametrize("kind", BAD_KINDS)
def test_invalid_rows_raise(spark, kind):
    from cdnaml.ml.regression import AFTSurvivalRegression
    from cdnaml.models.util import IllegalArgumentException
    c = R.case(5, 130)
    X, t, dl = plant(c, [kind], [40])
    # from tensors: a NaN label stays a NaN (a pandas NaN would arrive as a null label, and the row be dropped)
    df = spark.createDataFrameFromLocalTensors({"features": torch.from_numpy(X), "label": torch.from_numpy(t),
                                                "censor": torch.from_numpy(dl)})
    with pytest.raises(IllegalArgumentException, match="1 rows are invalid: the label must be positive"):
        AFTSurvivalRegression(maxIter=5).fit(df)
    if kind != "label nan":
        with pytest.raises(IllegalArgumentException, match="1 rows are invalid"):
            AFTSurvivalRegression(maxIter=5).fit(frame(spark, X, t, dl))
