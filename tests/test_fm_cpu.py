"""FMRegressor / FMClassifier (pyspark.ml) and the K25 ``fm_step`` op's host formulation.

* the numpy reference of ``tests/_fm_refs.py`` (pairwise form) against central differences, the host formulation
  (sum-of-squares form) against the reference to fp64 rounding, the flat layout on a hand-built model, the row
  selection against ``K.uniform``;
* the two updaters and the stopping rule on hand-computed steps;
* a product term and a sign-of-product label that the linear models cannot fit;
* the estimators' and the models' API: params, errors, thresholds, empty frames, seeds, persistence, Pipeline, the
  pyspark aliases, CrossValidator.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _fm_refs as R

SHAPES = [(5, 3), (33, 8), (100, 32)]     # (d, k)


def frame(spark, X, y):
    from cdnaml.ml.feature import VectorAssembler
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"] = y
    return VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))


def vectors(pdf_col):
    return np.stack([np.asarray(v.toArray() if hasattr(v, "toArray") else v) for v in pdf_col])


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("loss", [R.SQUARED, R.LOGISTIC])
@pytest.mark.parametrize("d,k", SHAPES)
def test_reference_gradient_matches_central_differences(d, k, loss):
    """h = 1e-6 in fp64: truncation h^2 |f'''| / 6 ~ 1e-12 and rounding eps |f| / h ~ 1e-9 per entry of the
    un-normalised sums; the worst entry must be within 1e-6 max|g|."""
    X, y, theta = R.make_case(d, k, 40, loss, dtype=np.float64)
    _, g, cnt = R.step(X, y, theta, k, loss)
    assert cnt == 40
    rng = np.random.default_rng(0)
    idx = np.unique(np.concatenate([rng.integers(0, len(theta), 60), [0, d * k, len(theta) - 1]]))
    h, worst = 1e-6, 0.0
    for i in idx:
        e = np.zeros_like(theta)
        e[i] = h
        fd = (R.step(X, y, theta + e, k, loss)[0] - R.step(X, y, theta - e, k, loss)[0]) / (2 * h)
        worst = max(worst, abs(fd - g[i]))
    print(f"fm fd d={d} k={k} loss={loss}: worst / max|g| = {worst / np.abs(g).max():.2e}")
    assert worst <= 1e-6 * np.abs(g).max()


@pytest.mark.parametrize("lin,icpt", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("n", [0, 1, 130])
@pytest.mark.parametrize("loss", [R.SQUARED, R.LOGISTIC])
def test_host_formulation_equals_reference(loss, n, f64, lin, icpt):
    """fp64 arithmetic on both sides (fp32 rows are widened; the parameters of make_case are fp32 values, so the
    op's rounding of them for fp32 rows changes nothing).  The two differ in the formulation (sum of squares against
    pairwise) and the order of the sums: the cancellation in s_f^2 - sum v^2 x^2 is between terms of the size of the
    result's own, so 1e-12 relative to the largest entry leaves two orders of slack over n d k 2^-53."""
    for d, k in SHAPES:
        X, y, theta = R.make_case(d, k, n, loss, lin=lin, icpt=icpt, dtype=np.float64 if f64 else np.float32)
        Xt = torch.from_numpy(X)
        assert K.fm_plan(Xt, k, lin) == {"path": "host"}
        ls, g, cnt = K.fm_step(Xt, torch.from_numpy(y), theta, k, loss, K.FM_STEP, lin, icpt)
        rl, rg, rc = R.step(X, y, theta, k, loss, lin, icpt)
        assert g.dtype == torch.float64 and g.shape == (R.num_params(d, k, lin, icpt),) and float(cnt) == rc == n
        assert abs(float(ls) - rl) <= 1e-12 * max(abs(rl), 1.0)
        np.testing.assert_allclose(g.numpy(), rg, rtol=0, atol=1e-12 * max(np.abs(rg).max(), 1.0) if n else 0)
        r = K.fm_step(Xt, None, theta, k, loss, K.FM_PREDICT, lin, icpt)
        assert r.shape == (n,) and r.dtype == torch.float64
        if n:
            rr = R.raw(X, theta, k, lin, icpt)
            np.testing.assert_allclose(r.numpy(), rr, rtol=0, atol=1e-12 * max(np.abs(rr).max(), 1.0))


def test_host_formulation_rounds_the_parameters_for_fp32_rows():
    X, y, theta = R.make_case(5, 3, 20, R.SQUARED)
    bumped = theta * (1 + 2.0 ** -30)                 # rounds back to theta in fp32
    assert np.array_equal(bumped.astype(np.float32), theta.astype(np.float32)) and not np.array_equal(bumped, theta)
    a = K.fm_step(torch.from_numpy(X), torch.from_numpy(y), bumped, 3)[1]
    b = K.fm_step(torch.from_numpy(X), torch.from_numpy(y), theta, 3)[1]
    c = K.fm_step(torch.from_numpy(X).double(), torch.from_numpy(y), bumped, 3)[1]
    assert torch.equal(a, b) and not torch.equal(c, b)


def test_flat_layout_on_a_hand_built_model():
    """d = 2, k = 1: theta = (v1, v2, w1, w2, b) and raw = b + w.x + v1 v2 x1 x2."""
    v1, v2, w1, w2, b = 2.0, -3.0, 0.5, 0.25, 7.0
    theta = np.array([v1, v2, w1, w2, b])
    x = np.array([[1.5, -2.0]])
    want = b + w1 * 1.5 + w2 * -2.0 + v1 * v2 * 1.5 * -2.0
    assert want == 25.25
    assert K.fm_step(torch.from_numpy(x), None, theta, 1, mode=K.FM_PREDICT).tolist() == [want]
    assert R.raw(x, theta, 1).tolist() == [want]
    V, w, bb = K.fm_unpack(torch.from_numpy(theta), 2, 1)
    assert V.tolist() == [[v1], [v2]] and w.tolist() == [w1, w2] and float(bb) == b
    # without the linear term the intercept follows the factors; without both there are only factors
    assert K.fm_step(torch.from_numpy(x), None, np.array([v1, v2, b]), 1, mode=K.FM_PREDICT,
                     fit_linear=False).tolist() == [b + 18.0]
    assert K.fm_step(torch.from_numpy(x), None, np.array([v1, v2]), 1, mode=K.FM_PREDICT, fit_linear=False,
                     fit_intercept=False).tolist() == [18.0]
    # squared loss at y = 25.25 - 1: m = 2, so d b = 2, d w = 2 x, d v1 = 2 v2 x1 x2, d v2 = 2 v1 x1 x2
    ls, g, cnt = K.fm_step(torch.from_numpy(x), torch.tensor([want - 1.0]), theta, 1)
    assert float(ls) == 1.0 and float(cnt) == 1.0
    assert g.tolist() == [2 * v2 * -3.0, 2 * v1 * -3.0, 3.0, -4.0, 2.0]
    # k = 2 is row-major [d][k]: entry (i, f) at i k + f
    V2 = K.fm_unpack(torch.arange(6.0, dtype=torch.float64), 2, 2, False, False)[0]
    assert V2.tolist() == [[0.0, 1.0], [2.0, 3.0]]


def test_logistic_loss_and_multiplier():
    theta = np.array([0.0, 0.0, 1.0, 0.0, 0.0])      # raw = x1
    x = torch.tensor([[2.0, 0.0], [2.0, 0.0], [-800.0, 0.0], [800.0, 0.0]], dtype=torch.float64)
    y = torch.tensor([1.0, 0.0, 1.0, 1.0], dtype=torch.float64)
    for i, (l, m) in enumerate([(np.log1p(np.exp(-2.0)), 1 / (1 + np.exp(-2.0)) - 1),
                                (np.log1p(np.exp(2.0)), 1 / (1 + np.exp(-2.0))), (800.0, -1.0), (0.0, 0.0)]):
        ls, g, _ = K.fm_step(x[i:i + 1], y[i:i + 1], theta, 1, K.FM_LOGISTIC)
        assert abs(float(ls) - l) <= 1e-15 * max(l, 1.0) and abs(float(g[4]) - m) <= 1e-15, (i, float(ls), g)


def test_sample_selects_the_rows_of_uniform():
    n, d, k = 700, 6, 4
    X, y, theta = R.make_case(d, k, n, R.SQUARED, dtype=np.float64)
    seed, off, frac = 12, 5000, 0.5
    mask = K.uniform(n, seed, off, K.FM_STREAM).numpy() < frac
    assert 300 < mask.sum() < 400
    ls, g, cnt = K.fm_step(torch.from_numpy(X), torch.from_numpy(y), theta, k, sample=(seed, off, frac))
    rl, rg, rc = R.step(X, y, theta, k, R.SQUARED, mask=mask)
    assert float(cnt) == rc == mask.sum()
    assert abs(float(ls) - rl) <= 1e-12 * abs(rl)
    np.testing.assert_allclose(g.numpy(), rg, rtol=0, atol=1e-12 * np.abs(rg).max())
    # the selection is keyed by the global row id: two shards select what the whole does
    a = K.fm_step(torch.from_numpy(X[:300]), torch.from_numpy(y[:300]), theta, k, sample=(seed, off, frac))
    b = K.fm_step(torch.from_numpy(X[300:]), torch.from_numpy(y[300:]), theta, k, sample=(seed, off + 300, frac))
    assert float(a[2]) + float(b[2]) == rc
    np.testing.assert_allclose((a[1] + b[1]).numpy(), rg, rtol=0, atol=1e-12 * np.abs(rg).max())
    # frac >= 1 and sample=None select every row without a draw
    full = K.fm_step(torch.from_numpy(X), torch.from_numpy(y), theta, k)
    one = K.fm_step(torch.from_numpy(X), torch.from_numpy(y), theta, k, sample=(seed, off, 1.0))
    assert float(one[2]) == n and torch.equal(full[1], one[1])


def test_op_errors():
    with pytest.raises(ValueError, match="parameters"):
        K.fm_step(torch.zeros(2, 3), torch.zeros(2), np.zeros(5), 2)
    with pytest.raises(ValueError, match="prepared"):
        K.fm_step(torch.zeros(2, 3), torch.zeros(2), np.zeros(10), 2, prepared=K.FmPrepared(np.zeros(7), 3, 1))
    assert K.FM_MAX_D == 128 and K.FM_MAX_K == 32


# ------------------------------------------------------------------------------------------------ the updaters
def test_gd_updater_two_hand_computed_steps():
    """SquaredL2Updater: eta_i = stepSize / sqrt(i), theta <- theta (1 - eta_i regParam) - eta_i g."""
    from cdnaml.models.regression import fm_update_gd
    theta = np.array([1.0, -2.0])
    t1 = fm_update_gd(theta, np.array([0.5, 0.25]), 1, 0.5, 0.1)
    np.testing.assert_allclose(t1, [1.0 * 0.95 - 0.25, -2.0 * 0.95 - 0.125], rtol=1e-15)
    eta = 0.5 / np.sqrt(2.0)
    t2 = fm_update_gd(t1, np.array([-1.0, 2.0]), 2, 0.5, 0.1)
    np.testing.assert_allclose(t2, [0.7 * (1 - 0.1 * eta) + eta, -2.025 * (1 - 0.1 * eta) - 2 * eta], rtol=1e-15)


def test_adamw_updater_two_hand_computed_steps():
    """AdamWUpdater: at i = 1 the corrected moments are g and g^2, so the step is stepSize g / (|g| + eps)."""
    from cdnaml.models.regression import fm_update_adamw
    theta, st = np.array([1.0, -2.0]), {"m": np.zeros(2), "v": np.zeros(2)}
    g1 = np.array([0.5, -0.25])
    t1 = fm_update_adamw(theta, g1, st, 1, 0.1, 0.01)
    np.testing.assert_allclose(st["m"], [0.05, -0.025], rtol=1e-15)
    np.testing.assert_allclose(st["v"], [0.00025, 0.0000625], rtol=1e-13)
    want1 = np.array([1.0 - (0.1 * 0.5 / (0.5 + 1e-8) + 0.01), -2.0 - (0.1 * -0.25 / (0.25 + 1e-8) - 0.02)])
    np.testing.assert_allclose(t1, want1, rtol=1e-14)
    g2 = np.array([-1.0, 0.5])
    t2 = fm_update_adamw(t1, g2, st, 2, 0.1, 0.01)
    m = 0.9 * np.array([0.05, -0.025]) + 0.1 * g2               # (-0.055, 0.0275)
    v = 0.999 * np.array([0.00025, 0.0000625]) + 0.001 * g2 ** 2
    np.testing.assert_allclose(m, [-0.055, 0.0275], rtol=1e-14)
    mh, vh = m / (1 - 0.81), v / (1 - 0.999 ** 2)
    np.testing.assert_allclose(t2, t1 - (0.1 * mh / (np.sqrt(vh) + 1e-8) + 0.01 * t1), rtol=1e-14)
    assert t2[0] > t1[0] - 0.01 * t1[0] - 1e-12 and t2[1] < t1[1] + 0.02 * 1.1   # against the sign of m-hat


def test_stopping_rule(spark):
    """|prev - cur|_2 < tol max(|cur|_2, 1), checked from the second update on."""
    from cdnaml.ml.regression import FMRegressor
    from cdnaml.models.regression import fm_converged
    assert fm_converged(np.array([3.0, 4.0]), np.array([3.0, 4.0 + 4e-3]), 1e-3)        # 4e-3 < 1e-3 * 5.0
    assert not fm_converged(np.array([3.0, 4.0]), np.array([3.0, 4.0 + 6e-3]), 1e-3)
    assert fm_converged(np.array([0.1]), np.array([0.1009]), 1e-3)                      # the floor of 1
    assert not fm_converged(np.array([0.1]), np.array([0.1011]), 1e-3)
    X, y = R.product_data(200, 4, seed=0)
    df = frame(spark, X, y)
    # adamW's first steps have size stepSize per entry: with a huge tol the fit stops at the second update, not
    # the first; with tol = 0 it runs to maxIter
    m = FMRegressor(maxIter=10, stepSize=0.01, tol=10.0, seed=1).fit(df)
    assert len(m.fitHistory) == 2
    assert len(FMRegressor(maxIter=10, stepSize=0.01, tol=0.0, seed=1).fit(df).fitHistory) == 10


def test_fit_is_the_reference_iteration(spark):
    """Three gd iterations with regParam and a minibatch, replayed in numpy on the reference."""
    from cdnaml.ml.regression import FMRegressor
    from cdnaml.models.regression import fm_initial_params
    X, y = R.product_data(300, 4, seed=2)
    df = frame(spark, X, y)
    kw = dict(factorSize=3, maxIter=3, stepSize=0.1, regParam=0.05, miniBatchFraction=0.5, solver="gd", seed=7,
              tol=0.0)
    m = FMRegressor(**kw).fit(df)
    theta = fm_initial_params(4, 3, True, True, 0.01, 7)
    for i in (1, 2, 3):
        mask = K.uniform(300, 7 + i, 0, K.FM_STREAM).numpy() < 0.5
        ls, g, cnt = R.step(X, y, theta, 3, R.SQUARED, mask=mask)
        assert m.fitHistory[i - 1][1] == cnt and abs(m.fitHistory[i - 1][0] - ls / cnt) <= 1e-12 * ls / cnt
        eta = 0.1 / np.sqrt(i)
        theta = theta * (1 - eta * 0.05) - eta * g / cnt
    got = np.concatenate([m.factors.toArray().reshape(-1), m.linear.toArray(), [m.intercept]])
    np.testing.assert_allclose(got, theta, rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------ fits
REG_FIT = dict(factorSize=4, maxIter=300, stepSize=0.05, initStd=0.1)
CLS_FIT = dict(factorSize=4, maxIter=300, stepSize=0.05, initStd=0.1)


@pytest.mark.parametrize("seed", range(6))
def test_product_term(spark, seed):
    """y = x1 x2 + x3: the linear model's residual is the product term (std 1); the FM's RMSE is at most half."""
    from cdnaml.ml.evaluation import RegressionEvaluator
    from cdnaml.ml.regression import FMRegressor, LinearRegression
    X, y = R.product_data(600, 4, seed=seed)
    df = frame(spark, X, y)
    ev = RegressionEvaluator(metricName="rmse")
    m = FMRegressor(seed=seed, **REG_FIT).fit(df)
    r_fm = ev.evaluate(m.transform(df))
    r_lr = ev.evaluate(LinearRegression().fit(df).transform(df))
    print(f"product term seed {seed}: FM rmse {r_fm:.4f} LinearRegression rmse {r_lr:.4f} "
          f"iterations {len(m.fitHistory)}")
    assert r_lr > 0.8 and r_fm <= 0.5 * r_lr


@pytest.mark.parametrize("seed", range(6))
def test_sign_of_product(spark, seed):
    """label = [x1 x2 > 0]: no linear boundary beats chance; in-sample a linear fit gains O(sqrt(d / n)) over 1 / 2
    by chance, 0.04 at n = 2000, so LogisticRegression stays below 0.6."""
    from cdnaml.ml.classification import FMClassifier, LogisticRegression
    from cdnaml.ml.evaluation import MulticlassClassificationEvaluator
    X, y = R.sign_data(2000, 3, seed=seed)
    df = frame(spark, X, y)
    acc = MulticlassClassificationEvaluator(metricName="accuracy")
    m = FMClassifier(seed=seed, **CLS_FIT).fit(df)
    a_fm = acc.evaluate(m.transform(df))
    a_lr = acc.evaluate(LogisticRegression().fit(df).transform(df))
    print(f"sign of product seed {seed}: FM {a_fm:.4f} LogisticRegression {a_lr:.4f} iterations {len(m.fitHistory)}")
    assert a_fm >= 0.9 and a_lr <= 0.6


# ------------------------------------------------------------------------------------------------ API
def test_params_and_defaults():
    from cdnaml.ml.classification import FMClassifier
    from cdnaml.ml.regression import FMRegressor
    for cls in (FMRegressor, FMClassifier):
        e = cls()
        assert (e.getFactorSize(), e.getFitIntercept(), e.getFitLinear(), e.getRegParam(), e.getMiniBatchFraction(),
                e.getInitStd(), e.getMaxIter(), e.getStepSize(), e.getTol(), e.getSolver(), e.getSeed()) == \
            (8, True, True, 0.0, 1.0, 0.01, 100, 1.0, 1e-6, "adamW", None)
        assert (e.getFeaturesCol(), e.getLabelCol(), e.getPredictionCol()) == ("features", "label", "prediction")
        assert not hasattr(e, "getWeightCol")
        e.setFactorSize(3).setSolver("gd").setMiniBatchFraction(0.25)
        assert (e.getFactorSize(), e.getSolver(), e.getMiniBatchFraction()) == (3, "gd", 0.25)
    c = FMClassifier(thresholds=[0.3, 0.7])
    assert (c.getProbabilityCol(), c.getRawPredictionCol(), c.getThresholds()) == \
        ("probability", "rawPrediction", [0.3, 0.7])


def test_errors(spark):
    from cdnaml.ml.classification import FMClassifier
    from cdnaml.ml.regression import FMRegressor
    from cdnaml.models.util import IllegalArgumentException
    X, y = R.sign_data(60, 3, seed=0)
    df = frame(spark, X, y)
    for cls in (FMRegressor, FMClassifier):
        with pytest.raises(IllegalArgumentException, match="solver must be gd or adamW"):
            cls(solver="l-bfgs").fit(df)
        for frac in (0.0, 1.5, -0.1):
            with pytest.raises(IllegalArgumentException, match=r"miniBatchFraction must be in \(0, 1\]"):
                cls(miniBatchFraction=frac).fit(df)
    with pytest.raises(IllegalArgumentException, match="labels other than 0 and 1"):
        FMClassifier().fit(frame(spark, X, y + 1.0))
    with pytest.raises(IllegalArgumentException, match="labels other than 0 and 1"):
        FMClassifier().fit(frame(spark, X, y * 0.5))


def test_model_properties_thresholds_and_empty_frame(spark):
    from cdnaml.ml.classification import FMClassifier
    from cdnaml.ml.linalg import DenseMatrix, DenseVector, Vectors
    from cdnaml.ml.regression import FMRegressor
    X, y = R.sign_data(200, 3, seed=5)
    df = frame(spark, X, y)
    m = FMClassifier(factorSize=4, maxIter=20, stepSize=0.05, seed=2).fit(df)
    assert (m.numFeatures, m.numClasses) == (3, 2)
    assert isinstance(m.linear, DenseVector) and isinstance(m.factors, DenseMatrix) and isinstance(m.intercept, float)
    assert m.factors.toArray().shape == (3, 4) and (m.factors.numRows, m.factors.numCols) == (3, 4)
    theta = np.concatenate([m.factors.toArray().reshape(-1), m.linear.toArray(), [m.intercept]])
    rr = R.raw(X, theta, 4)
    out = m.transform(df).select("rawPrediction", "probability", "prediction").toPandas()
    raw, prob = vectors(out.rawPrediction), vectors(out.probability)
    assert raw.dtype == np.float64 and prob.dtype == np.float64
    np.testing.assert_allclose(raw, np.stack([-rr, rr], 1), rtol=0, atol=1e-12 * np.abs(rr).max())
    sg = 1.0 / (1.0 + np.exp(-rr))
    np.testing.assert_allclose(prob, np.stack([1 - sg, sg], 1), rtol=0, atol=1e-13)
    assert np.array_equal(out.prediction.to_numpy(), (rr > 0).astype(np.float64))
    for i in (0, 199):
        v = Vectors.dense(X[i])
        np.testing.assert_allclose(m.predictRaw(v).toArray(), [-rr[i], rr[i]], rtol=0, atol=1e-12)
        np.testing.assert_allclose(m.predictProbability(v).toArray(), [1 - sg[i], sg[i]], rtol=0, atol=1e-13)
        assert m.predict(v) == float(rr[i] > 0)
    # thresholds: the class with the largest p / t
    t = [0.9, 0.1]
    pt = m.copy().setThresholds(t).transform(df).select("prediction").toPandas().prediction.to_numpy()
    assert np.array_equal(pt, (sg / 0.1 > (1 - sg) / 0.9).astype(np.float64)) and (pt != (rr > 0)).any()
    empty = m.transform(df.filter("label > 100"))
    assert empty.count() == 0 and {"rawPrediction", "probability", "prediction"} <= set(empty.columns)
    # an empty training frame: the initial model, no update
    e = FMClassifier(maxIter=3).fit(df.filter("label > 100"))
    assert [c for _, c in e.fitHistory] == [0.0] * 3 and e.intercept == 0.0
    # the regressor: prediction is raw; fitLinear / fitIntercept off leave zeros
    Xr, yr = R.product_data(100, 4, seed=1)
    dr = frame(spark, Xr, yr)
    r = FMRegressor(factorSize=2, maxIter=5, stepSize=0.05, fitLinear=False, fitIntercept=False, seed=3).fit(dr)
    assert r.intercept == 0.0 and not r.linear.toArray().any() and r.numFeatures == 4
    want = R.raw(Xr, r.factors.toArray().reshape(-1), 2, False, False)
    got = r.transform(dr).select("prediction").toPandas().prediction.to_numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    assert abs(r.predict(Vectors.dense(Xr[3])) - want[3]) <= 1e-13
    assert r.transform(dr.filter("label > 1e9")).count() == 0


def test_seeds(spark):
    from cdnaml.ml.regression import FMRegressor
    from cdnaml.models.regression import fm_initial_params
    X, y = R.product_data(150, 4, seed=7)
    df = frame(spark, X, y)
    kw = dict(factorSize=3, maxIter=5, stepSize=0.05, miniBatchFraction=0.5)
    f = [FMRegressor(seed=s, **kw).fit(df).factors.toArray() for s in (11, 11, 12)]
    assert np.array_equal(f[0], f[1]) and not np.array_equal(f[0], f[2])
    t0 = fm_initial_params(4, 3, True, True, 0.01, 11)
    assert t0.shape == (17,) and not t0[12:].any() and 0.002 < t0[:12].std() < 0.03
    m0 = FMRegressor(seed=11, factorSize=3, maxIter=0).fit(df)      # maxIter = 0 returns the initial parameters
    assert np.array_equal(m0.factors.toArray().reshape(-1), t0[:12]) and m0.intercept == 0.0


def test_persistence_alone_and_in_a_pipeline(spark, tmp_path):
    from cdnaml.ml import Pipeline, PipelineModel
    from cdnaml.ml.classification import FMClassificationModel, FMClassifier
    from cdnaml.ml.feature import VectorAssembler
    from cdnaml.ml.regression import FMRegressionModel, FMRegressor
    X, y = R.sign_data(120, 3, seed=9)
    df = frame(spark, X, y)
    m = FMClassifier(factorSize=3, maxIter=10, stepSize=0.05, seed=4, probabilityCol="pr", fitLinear=False).fit(df)
    m.write().overwrite().save(str(tmp_path / "fmc"))
    back = FMClassificationModel.load(str(tmp_path / "fmc"))
    assert back.getProbabilityCol() == "pr" and back.numFeatures == 3 and back.getFitLinear() is False
    assert np.array_equal(back.factors.toArray(), m.factors.toArray()) and back.intercept == m.intercept
    assert np.array_equal(vectors(m.transform(df).select("pr").toPandas().pr),
                          vectors(back.transform(df).select("pr").toPandas().pr))
    r = FMRegressor(factorSize=2, maxIter=5, stepSize=0.05, seed=4).fit(df)
    r.write().overwrite().save(str(tmp_path / "fmr"))
    rb = FMRegressionModel.load(str(tmp_path / "fmr"))
    assert np.array_equal(rb.linear.toArray(), r.linear.toArray()) and rb.factors.toArray().shape == (3, 2)
    assert np.array_equal(rb.transform(df).select("prediction").toPandas().prediction.to_numpy(),
                          r.transform(df).select("prediction").toPandas().prediction.to_numpy())
    est = FMRegressor(factorSize=5, solver="gd", miniBatchFraction=0.5)
    est.write().overwrite().save(str(tmp_path / "est"))
    e2 = FMRegressor.load(str(tmp_path / "est"))
    assert (e2.getFactorSize(), e2.getSolver(), e2.getMiniBatchFraction()) == (5, "gd", 0.5)
    names = [f"x{i}" for i in range(3)]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"] = y
    raw_df = spark.createDataFrame(pdf)
    pm = Pipeline(stages=[VectorAssembler(inputCols=names, outputCol="features"),
                          FMClassifier(factorSize=3, maxIter=10, stepSize=0.05, seed=4)]).fit(raw_df)
    pm.write().overwrite().save(str(tmp_path / "pipe"))
    pb = PipelineModel.load(str(tmp_path / "pipe"))
    assert isinstance(pb.stages[-1], FMClassificationModel)
    assert np.array_equal(pb.stages[-1].factors.toArray(), pm.stages[-1].factors.toArray())
    assert np.array_equal(pb.transform(raw_df).select("prediction").toPandas().prediction.to_numpy(),
                          pm.transform(raw_df).select("prediction").toPandas().prediction.to_numpy())


def test_pyspark_alias_and_cross_validator(spark):
    from cdnaml import compat
    compat.install()
    try:
        from pyspark.ml.classification import FMClassificationModel, FMClassifier
        from pyspark.ml.evaluation import MulticlassClassificationEvaluator, RegressionEvaluator
        from pyspark.ml.regression import FMRegressionModel, FMRegressor
        from pyspark.ml.tuning import CrossValidator, ParamGridBuilder
        X, y = R.sign_data(300, 3, seed=1)
        df = frame(spark, X, y)
        est = FMClassifier(seed=3, **CLS_FIT)
        grid = ParamGridBuilder().addGrid(est.maxIter, [1, CLS_FIT["maxIter"]]).build()
        cv = CrossValidator(estimator=est, estimatorParamMaps=grid, numFolds=2, seed=5,
                            evaluator=MulticlassClassificationEvaluator(metricName="accuracy")).fit(df)
        assert isinstance(cv.bestModel, FMClassificationModel)
        assert len(cv.avgMetrics) == 2 and cv.avgMetrics[1] > cv.avgMetrics[0] and cv.avgMetrics[1] >= 0.85
        Xr, yr = R.product_data(300, 4, seed=1)
        reg = FMRegressor(seed=3, **REG_FIT)
        grid = ParamGridBuilder().addGrid(reg.maxIter, [1, REG_FIT["maxIter"]]).build()
        cv = CrossValidator(estimator=reg, estimatorParamMaps=grid, numFolds=2, seed=5,
                            evaluator=RegressionEvaluator(metricName="rmse")).fit(frame(spark, Xr, yr))
        assert isinstance(cv.bestModel, FMRegressionModel) and cv.avgMetrics[1] < 0.5 * cv.avgMetrics[0]
    finally:
        compat.uninstall()
