"""MultilayerPerceptronClassifier (pyspark.ml.classification) and the K24 ``mlp_step`` op's host formulation.

* the numpy reference of ``tests/_mlp_refs.py`` against central differences, the host formulation against the
  reference to fp64 rounding, the flat weight layout on a hand-built net;
* ``layers=[d, C]`` against multinomial LogisticRegression (the same convex problem), the XOR clusters a linear model
  cannot fit;
* the estimator's and the model's API: params, errors, thresholds, empty frames, seeds, persistence, Pipeline, the
  pyspark alias, CrossValidator.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _mlp_refs as R

NETS = [[5, 4, 3], [33, 33, 2], [100, 64, 32, 3]]


def frame(spark, X, y):
    from cdnaml.ml.feature import VectorAssembler
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"] = y
    return VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))


def vectors(pdf_col):
    return np.stack([np.asarray(v.toArray() if hasattr(v, "toArray") else v) for v in pdf_col])


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("layers", NETS)
def test_reference_gradient_matches_central_differences(layers):
    """h = 1e-6 in fp64: truncation h^2 |f'''| / 6 ~ 1e-12 and rounding eps |f| / h ~ 1e-9 per entry of the
    un-normalised sums; the worst entry must be within 1e-6 max|g| (measured 1e-9 .. 2e-9)."""
    X, y, theta = R.make_case(layers, 40, dtype=np.float64)
    _, g = R.step(X, y, theta, layers)
    rng = np.random.default_rng(0)
    idx = np.unique(np.concatenate([rng.integers(0, len(theta), 60), [0, len(theta) - 1]]))
    h, worst = 1e-6, 0.0
    for i in idx:
        e = np.zeros_like(theta)
        e[i] = h
        fd = (R.step(X, y, theta + e, layers)[0] - R.step(X, y, theta - e, layers)[0]) / (2 * h)
        worst = max(worst, abs(fd - g[i]))
    print(f"mlp fd {layers}: worst / max|g| = {worst / np.abs(g).max():.2e}")
    assert worst <= 1e-6 * np.abs(g).max()


@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("n", [0, 1, 130])
@pytest.mark.parametrize("layers", NETS + [[7, 3]])
def test_host_formulation_equals_reference(layers, n, f64):
    """fp64 arithmetic on both sides (fp32 rows are widened; the weights of make_case are fp32 values, so the op's
    rounding of them for fp32 rows changes nothing): they differ in the order of the sums only, n 2^-53 per sum with
    two orders of slack -> 1e-12 relative to the largest entry."""
    X, y, theta = R.make_case(layers, n, dtype=np.float64 if f64 else np.float32)
    assert K.mlp_plan(torch.from_numpy(X), layers) == {"path": "host"}
    loss, g = K.mlp_step(torch.from_numpy(X), torch.from_numpy(y), theta, layers, K.MLP_STEP)
    rl, rg = R.step(X, y, theta, layers)
    assert g.dtype == torch.float64 and g.shape == (R.num_params(layers),)
    assert abs(float(loss) - rl) <= 1e-12 * max(abs(rl), 1.0)
    np.testing.assert_allclose(g.numpy(), rg, rtol=0, atol=1e-12 * max(np.abs(rg).max(), 1.0) if n else 0)
    raw, prob, pred = K.mlp_step(torch.from_numpy(X), None, theta, layers, K.MLP_PREDICT)
    rr, rp, rd = R.predict(X, theta, layers)
    assert raw.shape == (n, layers[-1]) and prob.dtype == torch.float64 and pred.dtype == torch.int32
    if n:
        np.testing.assert_allclose(raw.numpy(), rr, rtol=0, atol=1e-12 * np.abs(rr).max())
        np.testing.assert_allclose(prob.numpy(), rp, rtol=0, atol=1e-13)
        assert np.array_equal(pred.numpy(), rd)


def test_host_formulation_rounds_the_weights_for_fp32_rows():
    layers = [5, 4, 3]
    X, y, theta = R.make_case(layers, 20)
    bumped = theta * (1 + 2.0 ** -30)                 # rounds back to theta in fp32
    assert np.array_equal(bumped.astype(np.float32), theta.astype(np.float32)) and not np.array_equal(bumped, theta)
    a = K.mlp_step(torch.from_numpy(X), torch.from_numpy(y), bumped, layers)[1]
    b = K.mlp_step(torch.from_numpy(X), torch.from_numpy(y), theta, layers)[1]
    c = K.mlp_step(torch.from_numpy(X).double(), torch.from_numpy(y), bumped, layers)[1]
    assert torch.equal(a, b) and not torch.equal(c, b)


def test_flat_layout_on_a_hand_built_net():
    """[2, 2, 2] with distinct weights: layer 1 W = [[1, 3], [2, 4]] (column-major 1, 2, 3, 4), b = (5, 6); layer 2
    W = [[7, 9], [8, 10]], b = (11, 12).  For x = (1, -1): z1 = (1 - 3 + 5, 2 - 4 + 6) = (3, 4), a = sigmoid(z1),
    logits = (7 a0 + 9 a1 + 11, 8 a0 + 10 a1 + 12)."""
    theta = np.arange(1.0, 13.0)
    x = np.array([[1.0, -1.0]])
    a = 1.0 / (1.0 + np.exp(-np.array([3.0, 4.0])))
    want = np.array([[7 * a[0] + 9 * a[1] + 11, 8 * a[0] + 10 * a[1] + 12]])
    raw, _, pred = K.mlp_step(torch.from_numpy(x), None, theta, [2, 2, 2], K.MLP_PREDICT)
    np.testing.assert_allclose(raw.numpy(), want, rtol=1e-15)
    np.testing.assert_allclose(R.predict(x, theta, [2, 2, 2])[0], want, rtol=1e-15)
    assert pred.item() == 1
    W, b = K.mlp_unpack(torch.from_numpy(theta), [2, 2, 2])[1]
    assert W.tolist() == [[7.0, 9.0], [8.0, 10.0]] and b.tolist() == [11.0, 12.0]
    # the bias gradient sits behind the weight block: d loss / d b of the last layer is softmax - onehot
    _, g = K.mlp_step(torch.from_numpy(x), torch.tensor([0]), theta, [2, 2, 2])
    p = np.exp(want - want.max())
    p /= p.sum()
    np.testing.assert_allclose(g.numpy()[10:], (p - [1.0, 0.0])[0], rtol=1e-12)


def test_ties_predict_the_lowest_index():
    theta = np.zeros(R.num_params([3, 4]))
    raw, prob, pred = K.mlp_step(torch.ones(5, 3, dtype=torch.float64), None, theta, [3, 4], K.MLP_PREDICT)
    assert pred.tolist() == [0] * 5 and torch.equal(prob, torch.full((5, 4), 0.25, dtype=torch.float64))


def test_op_errors():
    with pytest.raises(ValueError, match="weights"):
        K.mlp_step(torch.zeros(2, 3), torch.zeros(2), np.zeros(5), [3, 2])
    with pytest.raises(ValueError, match="columns"):
        K.mlp_step(torch.zeros(2, 4), torch.zeros(2), np.zeros(8), [3, 2])
    assert K.MLP_MAX_WIDTH == 128 and K.MLP_MAX_LAYERS == 3


# ------------------------------------------------------------------------------------------------ fits
def test_no_hidden_layer_is_multinomial_logistic_regression(spark):
    """``layers=[d, C]`` and LogisticRegression(regParam=0, family="multinomial") minimise the same convex function
    with the same optimiser from different starting points and scalings; the data overlap, so the minimum is finite
    and unique in probability space.  Both stop once a step lowers f by less than tol f.  With a linear rate rho the
    remaining gap is at most rho / (1 - rho) tol f <= 100 tol f for rho <= 0.99, so the two losses differ by at
    most 200 tol f.  Near the minimum f - f* is the mean over the rows of dz^T (diag(p) - p p^T) dz / 2 with dp =
    (diag(p) - p p^T) dz and |diag(p) - p p^T| <= 1 / 2, so mean |dp|^2 <= (f - f*) and the largest row is within
    sqrt(n (f - f*)); two fits: 2 sqrt(100 n tol f)."""
    from cdnaml.ml.classification import LogisticRegression, MultilayerPerceptronClassifier
    X, y = R.three_class_data(600, 4, seed=3)
    df = frame(spark, X, y)
    tol = 1e-10
    mlp = MultilayerPerceptronClassifier(layers=[4, 3], tol=tol, maxIter=500, seed=1).fit(df)
    lr = LogisticRegression(regParam=0.0, family="multinomial", tol=tol, maxIter=500).fit(df)
    f_mlp, f_lr = mlp.summary.objectiveHistory[-1], lr.summary.objectiveHistory[-1]
    assert 0.3 < f_lr < 1.1                                            # far from separable
    pm = vectors(mlp.transform(df).select("probability").toPandas().probability)
    pl = vectors(lr.transform(df).select("probability").toPandas().probability)
    print(f"mlp [d, C] vs LR: loss {f_mlp:.12f} {f_lr:.12f}  max |dp| {np.abs(pm - pl).max():.2e}")
    assert abs(f_mlp - f_lr) <= 200 * tol * f_lr
    assert np.abs(pm - pl).max() <= 2 * np.sqrt(100 * len(y) * tol * f_lr)
    # the reported objective is the mean of the reference's loss at the fitted weights
    assert abs(f_mlp - R.step(X, y, mlp.weights.toArray(), [4, 3])[0] / len(y)) <= 1e-12


@pytest.mark.parametrize("seed", range(6))
def test_xor_clusters(spark, seed):
    from cdnaml.ml.classification import LogisticRegression, MultilayerPerceptronClassifier
    from cdnaml.ml.evaluation import MulticlassClassificationEvaluator
    X, y = R.xor_data(400, seed=seed)
    df = frame(spark, X, y)
    acc = MulticlassClassificationEvaluator(metricName="accuracy")
    m = MultilayerPerceptronClassifier(layers=[2, 8, 2], maxIter=100, seed=seed).fit(df)
    a_mlp = acc.evaluate(m.transform(df))
    a_lr = acc.evaluate(LogisticRegression().fit(df).transform(df))
    print(f"xor seed {seed}: mlp {a_mlp:.4f} lr {a_lr:.4f} iterations {m.summary.totalIterations}")
    assert a_mlp >= 0.95 and a_lr <= 0.8
    assert m.summary.accuracy == a_mlp
    h = m.summary.objectiveHistory
    assert 2 <= len(h) <= m.summary.totalIterations + 1 <= 101 and h[-1] < h[0]


# ------------------------------------------------------------------------------------------------ API
def test_params_and_defaults():
    from cdnaml.ml.classification import MultilayerPerceptronClassifier
    e = MultilayerPerceptronClassifier(layers=[4, 5, 3])
    assert (e.getMaxIter(), e.getTol(), e.getBlockSize(), e.getSolver(), e.getStepSize()) == \
        (100, 1e-6, 128, "l-bfgs", 0.03)
    assert e.getLayers() == [4, 5, 3] and e.getInitialWeights() is None and e.getSeed() is None
    assert (e.getFeaturesCol(), e.getLabelCol(), e.getPredictionCol(), e.getProbabilityCol(),
            e.getRawPredictionCol()) == ("features", "label", "prediction", "probability", "rawPrediction")
    e.setMaxIter(7).setSeed(3).setInitialWeights(np.arange(3.0))
    assert e.getMaxIter() == 7 and e.getSeed() == 3 and e.getInitialWeights() == [0.0, 1.0, 2.0]


def test_errors(spark):
    from cdnaml.ml.classification import MultilayerPerceptronClassifier as MLP
    from cdnaml.models.util import IllegalArgumentException
    X, y = R.three_class_data(60, 4, seed=0)
    df = frame(spark, X, y)
    with pytest.raises(IllegalArgumentException, match=r"layers\[0\] = 5"):
        MLP(layers=[5, 3]).fit(df)
    with pytest.raises(IllegalArgumentException, match="max label value = 2.0"):
        MLP(layers=[4, 3, 2]).fit(df)
    with pytest.raises(IllegalArgumentException, match="not non-negative integers"):
        MLP(layers=[4, 3]).fit(frame(spark, X, y - 0.5))
    with pytest.raises(IllegalArgumentException, match="initialWeights has 4 entries"):
        MLP(layers=[4, 3], initialWeights=[0.0] * 4).fit(df)
    with pytest.raises(IllegalArgumentException, match="at least 2"):
        MLP(layers=[4]).fit(df)
    with pytest.raises(NotImplementedError, match="gd"):
        MLP(layers=[4, 3], solver="gd").fit(df)


def test_model_properties_thresholds_and_empty_frame(spark):
    from cdnaml.ml.classification import MultilayerPerceptronClassifier
    from cdnaml.ml.linalg import Vectors
    X, y = R.three_class_data(200, 4, seed=5)
    df = frame(spark, X, y)
    m = MultilayerPerceptronClassifier(layers=[4, 5, 3], maxIter=15, seed=2).fit(df)
    assert (m.numFeatures, m.numClasses, m.getLayers()) == (4, 3, [4, 5, 3])
    theta = m.weights.toArray()
    assert theta.shape == (R.num_params([4, 5, 3]),) and m.hasSummary
    out = m.transform(df).select("rawPrediction", "probability", "prediction").toPandas()
    raw, prob = vectors(out.rawPrediction), vectors(out.probability)
    rr, rp, rd = R.predict(X, theta, [4, 5, 3])
    assert raw.dtype == np.float64
    np.testing.assert_allclose(raw, rr, rtol=0, atol=1e-12 * np.abs(rr).max())
    np.testing.assert_allclose(prob, rp, rtol=0, atol=1e-13)
    assert np.array_equal(out.prediction.to_numpy(), rd.astype(np.float64))
    for i in (0, 199):
        v = Vectors.dense(X[i])
        np.testing.assert_allclose(m.predictRaw(v).toArray(), rr[i], rtol=0, atol=1e-12 * np.abs(rr).max())
        np.testing.assert_allclose(m.predictProbability(v).toArray(), rp[i], rtol=0, atol=1e-13)
        assert m.predict(v) == float(rd[i])
    # thresholds: the class with the largest p / t
    t = [0.9, 0.05, 0.05]
    pt = m.copy().setThresholds(t).transform(df).select("prediction").toPandas().prediction.to_numpy()
    assert np.array_equal(pt, np.argmax(rp / np.array(t), 1).astype(np.float64)) and (pt != rd).any()
    empty = m.transform(df.filter("label > 100"))
    assert empty.count() == 0 and {"rawPrediction", "probability", "prediction"} <= set(empty.columns)
    ev = m.evaluate(df)
    assert 0.0 < ev.accuracy <= 1.0 and ev.accuracy == m.summary.accuracy


def test_seeds_and_initial_weights(spark):
    from cdnaml.ml.classification import MultilayerPerceptronClassifier as MLP
    from cdnaml.models.classification import mlp_initial_weights
    X, y = R.three_class_data(150, 4, seed=7)
    df = frame(spark, X, y)
    w = [MLP(layers=[4, 6, 3], maxIter=5, seed=s).fit(df).weights.toArray() for s in (11, 11, 12)]
    assert np.array_equal(w[0], w[1]) and not np.array_equal(w[0], w[2])
    t0 = mlp_initial_weights([4, 6, 3], 11)
    b = np.sqrt(6.0 / 10)
    assert np.abs(t0[:24]).max() <= b and np.abs(t0[:24]).max() > 0.5 * b and not t0[24:30].any()
    assert not t0[30 + 18:].any() and np.abs(t0[30:48]).max() <= np.sqrt(6.0 / 9)
    # maxIter = 0 returns the initial weights; initialWeights replaces the draw
    assert np.array_equal(MLP(layers=[4, 6, 3], maxIter=0, seed=11).fit(df).weights.toArray(), t0)
    m = MLP(layers=[4, 6, 3], maxIter=5, seed=99, initialWeights=t0).fit(df)
    assert np.array_equal(m.weights.toArray(), w[0])


def test_persistence_alone_and_in_a_pipeline(spark, tmp_path):
    from cdnaml.ml import Pipeline, PipelineModel
    from cdnaml.ml.classification import MultilayerPerceptronClassificationModel, MultilayerPerceptronClassifier
    from cdnaml.ml.feature import VectorAssembler
    X, y = R.three_class_data(120, 3, seed=9)
    df = frame(spark, X, y)
    m = MultilayerPerceptronClassifier(layers=[3, 4, 3], maxIter=10, seed=4, probabilityCol="pr").fit(df)
    m.write().overwrite().save(str(tmp_path / "mlp"))
    back = MultilayerPerceptronClassificationModel.load(str(tmp_path / "mlp"))
    assert back.getLayers() == [3, 4, 3] and back.getProbabilityCol() == "pr" and not back.hasSummary
    assert np.array_equal(back.weights.toArray(), m.weights.toArray())
    a = m.transform(df).select("pr").toPandas().pr
    b = back.transform(df).select("pr").toPandas().pr
    assert np.array_equal(vectors(a), vectors(b))
    est = MultilayerPerceptronClassifier(layers=[3, 2], tol=0.5, initialWeights=[1.0] * 8)
    est.write().overwrite().save(str(tmp_path / "est"))
    e2 = MultilayerPerceptronClassifier.load(str(tmp_path / "est"))
    assert (e2.getLayers(), e2.getTol(), e2.getInitialWeights()) == ([3, 2], 0.5, [1.0] * 8)
    names = [f"x{i}" for i in range(3)]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"] = y
    raw_df = spark.createDataFrame(pdf)
    pm = Pipeline(stages=[VectorAssembler(inputCols=names, outputCol="features"),
                          MultilayerPerceptronClassifier(layers=[3, 4, 3], maxIter=10, seed=4)]).fit(raw_df)
    pm.write().overwrite().save(str(tmp_path / "pipe"))
    pb = PipelineModel.load(str(tmp_path / "pipe"))
    assert isinstance(pb.stages[-1], MultilayerPerceptronClassificationModel)
    assert np.array_equal(pb.stages[-1].weights.toArray(), m.weights.toArray())
    assert np.array_equal(pb.transform(raw_df).select("prediction").toPandas().prediction.to_numpy(),
                          pm.transform(raw_df).select("prediction").toPandas().prediction.to_numpy())


def test_pyspark_alias_and_cross_validator(spark):
    from cdnaml import compat
    compat.install()
    try:
        from pyspark.ml.classification import (MultilayerPerceptronClassificationModel,
                                               MultilayerPerceptronClassifier)
        from pyspark.ml.evaluation import MulticlassClassificationEvaluator
        from pyspark.ml.tuning import CrossValidator, ParamGridBuilder
        X, y = R.xor_data(200, seed=1)
        df = frame(spark, X, y)
        est = MultilayerPerceptronClassifier(layers=[2, 6, 2], seed=3)
        grid = ParamGridBuilder().addGrid(est.maxIter, [1, 60]).build()
        cv = CrossValidator(estimator=est, estimatorParamMaps=grid, numFolds=2, seed=5,
                            evaluator=MulticlassClassificationEvaluator(metricName="accuracy")).fit(df)
        assert isinstance(cv.bestModel, MultilayerPerceptronClassificationModel)
        assert len(cv.avgMetrics) == 2 and cv.avgMetrics[1] > cv.avgMetrics[0] and cv.avgMetrics[1] >= 0.9
    finally:
        compat.uninstall()
