"""GaussianMixture (pyspark.ml.clustering) and the K23 ``gmm_step`` op's host formulation, on the CPU.

* the host formulation of the op (STEP / PREDICT / EVAL; fp32 and fp64 rows) against the numpy reference of
  ``tests/_gmm_refs.py``, within the bounds that module derives from the inputs (for fp32 rows the host's sgemm
  stands in for the MFMA: the same fmaf-chain bound holds for it);
* fitted models against the reference EM loop from the same initial state: same number of iterations, and
  log-likelihood, weights, means and covariances to relative 1e-9.  Both sides sum in fp64 and differ in the
  order of the sums only: n 2^-53 ~ 1e-12 per pass, through at most 100 passes of a map that contracts near its
  fixed point, with an order of slack;
* properties of the estimator and the model, persistence, Pipeline, the pyspark alias, and one loose cross-check
  against scikit-learn.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _gmm_refs as G
from tests.conftest import session_device

REL = 1e-9

# (n, d, k, zero weights, fp64 rows)
OP_SHAPES = [(1, 4, 2, False, False), (1, 4, 2, False, True), (65, 3, 2, False, False), (300, 7, 3, True, False),
             (300, 7, 3, True, True), (400, 20, 32, False, False), (257, 127, 3, False, False),
             (200, 1, 2, False, True)]


def tt(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def check_against_ref(ref, S=None, R=None, assign=None, stats=None):
    """The comparisons the CPU and the GPU tests share: every output against the reference within its bound.
    ``assign`` must equal the reference's argmax on every row whose top two reference responsibilities differ by
    more than 2 dr (r_a - dr > r_b + dr is what guarantees the order); at least half the rows must be such."""
    assert ref.overlap_ok()
    if stats is not None:
        assert stats[2] == ref.stats[2]
        np.testing.assert_allclose(stats[1], ref.stats[1], rtol=1e-12)
        assert abs(stats[0] - ref.stats[0]) <= ref.dstats0, (stats[0], ref.stats[0], ref.dstats0)
    if R is not None:
        assert np.isnan(R[ref.bad]).all() and (assign[ref.bad] == 0).all()
        err = np.abs(R[ref.good] - ref.R[ref.good]).max(1)
        assert (err <= ref.dr[ref.good]).all(), (err / ref.dr[ref.good]).max()
        # the argmax is decided where the reference's top two differ by more than 2 dr: each of the two
        # responsibilities may move by the dr bound, in opposite directions
        sure = ref.good & (ref.top2_gap() > 2 * ref.dr)
        assert sure.sum() >= 0.5 * ref.good.sum()
        assert np.array_equal(assign[sure], ref.assign[sure])
    if S is not None:
        Sr, dS = ref.moments()
        assert (np.abs(S - Sr) <= dS).all(), (np.abs(S - Sr) / dS).max()


@pytest.mark.parametrize("n,d,k,zero_w,f64", OP_SHAPES)
def test_host_formulation_matches_reference(n, d, k, zero_w, f64):
    X, w, mu, A, logc = G.make_inputs(n, d, k, None, zero_w, f64)
    ref = G.ref_for(n, d, k, None, zero_w, f64)
    args = (tt(X), tt(w), tt(mu), tt(A), tt(logc))
    S, st = K.gmm_step(*args, K.GMM_STEP)
    R, a, st_p = K.gmm_step(*args, K.GMM_PREDICT)
    st_e = K.gmm_step(*args, K.GMM_EVAL)
    assert S.dtype == R.dtype == st.dtype == torch.float64 and a.dtype == torch.int32
    assert torch.equal(st, st_p) and torch.equal(st, st_e)
    check_against_ref(ref, S.numpy(), R.numpy(), a.numpy(), st.numpy())
    np.testing.assert_allclose(R.numpy().sum(1), 1.0, rtol=1e-14)
    assert np.array_equal(a.numpy(), np.argmax(R.numpy(), 1))


@pytest.mark.parametrize("f64", [False, True])
def test_far_row_is_uniform_and_nan_row_is_left_out(f64):
    n, d, k = 120, 5, 3
    X, w, mu, A, logc = G.make_inputs(n, d, k, None, False, f64)
    X = X.copy()
    X[11] = 1e3            # thousands of sd from every component: every density underflows
    X[57, 2] = np.nan
    ref = G.Ref(X, w, mu, A, logc)
    assert ref.bad.sum() == 1 and ref.bad[57]
    assert np.array_equal(ref.R[11], np.full(k, 1.0 / k))
    args = (tt(X), None, tt(mu), tt(A), tt(logc))
    S, st = K.gmm_step(*args, K.GMM_STEP)
    R, a, _ = K.gmm_step(*args, K.GMM_PREDICT)
    assert st[2].item() == 1 and torch.isfinite(S).all()
    assert np.array_equal(R[11].numpy(), np.full(k, 1.0 / k)) and a[11].item() == 0
    check_against_ref(ref, S.numpy(), R.numpy(), a.numpy(), st.numpy())


# ---------------------------------------------------------------------------------------------------- estimator
@pytest.fixture
def spark(tmp_path):
    import cdnaml
    with session_device("cpu"):
        s = cdnaml.SparkSession.builder.config("cdnaml.warehouse.dir", str(tmp_path / "warehouse")).getOrCreate()
        yield s
        s.stop()


def frame(spark, X, w=None, keep_invalid=False):
    from cdnaml.ml.feature import VectorAssembler
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    if w is not None:
        pdf["w"] = w
    va = VectorAssembler(inputCols=names, outputCol="features", handleInvalid="keep" if keep_invalid else "error")
    return va.transform(spark.createDataFrame(pdf))


def params(m):
    return (np.array(m.weights), np.stack([g.mean.toArray() for g in m.gaussians]),
            np.stack([g.cov.toArray() for g in m.gaussians]))


def fit(spark, X, w=None, **kw):
    from cdnaml.ml.clustering import GaussianMixture
    df = frame(spark, X, w)
    return GaussianMixture(weightCol="w" if w is not None else None, **kw).fit(df), df


def assert_matches_reference(spark, X, w, k, seed, tol=0.01, max_iter=100):
    m0, _ = fit(spark, X, w, k=k, seed=seed, maxIter=0)
    m, _ = fit(spark, X, w, k=k, seed=seed, tol=tol, maxIter=max_iter)
    rw, rm, rc, trace = G.ref_em(X, w, *params(m0), tol, max_iter)
    assert m.summary.numIter == len(trace)
    assert abs(m.summary.logLikelihood - trace[-1]) <= REL * abs(trace[-1])
    pw, pm, pc = params(m)
    np.testing.assert_allclose(pw, rw, rtol=REL)
    np.testing.assert_allclose(pm, rm, rtol=0, atol=REL * np.abs(rm).max())
    np.testing.assert_allclose(pc, rc, rtol=0, atol=REL * np.abs(rc).max())
    return m, trace


def test_fit_matches_reference_em(spark):
    X = G.overlapping_data(3000, 4, 3, seed=3)
    m, trace = assert_matches_reference(spark, X, None, 3, seed=11)
    assert 2 < len(trace) < 100 and all(b >= a - 1e-9 * abs(a) for a, b in zip(trace, trace[1:]))
    assert sum(m.summary.clusterSizes) == 3000 and m.summary.k == 3


def test_weighted_fit_matches_reference_em(spark):
    X = G.overlapping_data(2000, 3, 2, seed=5)
    w = np.random.default_rng(0).uniform(0.0, 2.0, 2000)
    w[::7] = 0.0
    assert_matches_reference(spark, X, w, 2, seed=4)


def test_properties(spark):
    X = G.overlapping_data(1500, 3, 3, seed=9)
    m, df = fit(spark, X, k=3, seed=2)
    assert abs(sum(m.weights) - 1.0) < 1e-12 and m.hasSummary
    out = m.transform(df).select("prediction", "probability").toPandas()
    P = np.stack([np.asarray(v.toArray() if hasattr(v, "toArray") else v) for v in out.probability])
    np.testing.assert_allclose(P.sum(1), 1.0, rtol=1e-14)
    assert np.array_equal(out.prediction.to_numpy(), np.argmax(P, 1))
    assert str(out.prediction.dtype).startswith("int")
    assert np.array_equal(np.bincount(out.prediction.to_numpy(), minlength=3), m.summary.clusterSizes)
    from cdnaml.ml.linalg import Vectors
    for i in (0, 17, 1499):
        pp = m.predictProbability(Vectors.dense(X[i]))
        np.testing.assert_allclose(pp.toArray(), P[i], rtol=1e-13)
        assert m.predict(Vectors.dense(X[i])) == out.prediction[i]
    s = m.summary
    assert (s.featuresCol, s.predictionCol, s.probabilityCol) == ("features", "prediction", "probability")
    assert s.cluster.columns == ["prediction"] and s.probability.columns == ["probability"]
    assert s.predictions.count() == 1500
    # an empty column name leaves the column out
    assert "probability" not in m.copy().setProbabilityCol("").transform(df).columns
    assert "prediction" not in m.copy().setPredictionCol("").transform(df).columns


def test_same_seed_same_model_and_max_iter_zero(spark):
    X = G.overlapping_data(1200, 3, 2, seed=1)
    a, _ = fit(spark, X, k=2, seed=5)
    b, _ = fit(spark, X, k=2, seed=5)
    for u, v in zip(params(a), params(b)):
        assert np.array_equal(u, v)
    m0, _ = fit(spark, X, k=2, seed=5, maxIter=0)
    w0, mu0, cov0 = params(m0)
    assert m0.summary.numIter == 0 and np.array_equal(w0, [0.5, 0.5])
    # Spark's initial state: means and diagonal variances of 5 sampled rows each
    assert all(np.count_nonzero(c - np.diag(np.diag(c))) == 0 for c in cov0)
    ref = G.Ref(X, None, mu0, *G.tables(w0, mu0, cov0))
    assert abs(m0.summary.logLikelihood - ref.stats[0]) <= REL * abs(ref.stats[0])


def test_integer_weights_equal_duplicated_rows(spark, monkeypatch):
    from cdnaml.ml.clustering import GaussianMixture
    X = G.overlapping_data(800, 3, 2, seed=21)
    w = np.random.default_rng(1).integers(0, 4, 800).astype(float)
    m0, _ = fit(spark, X, k=2, seed=3, maxIter=0)
    state = params(m0)
    monkeypatch.setattr(GaussianMixture, "_init_state", lambda self, *a: state)   # the same initial state for both
    a, _ = fit(spark, X, w, k=2, tol=1e-6)
    b, _ = fit(spark, np.repeat(X, w.astype(int), 0), k=2, tol=1e-6)
    assert a.summary.numIter == b.summary.numIter
    assert abs(a.summary.logLikelihood - b.summary.logLikelihood) <= REL * abs(b.summary.logLikelihood)
    for u, v in zip(params(a), params(b)):
        np.testing.assert_allclose(u, v, rtol=0, atol=REL * np.abs(v).max())


def test_singular_covariance_fits_through_the_pseudo_inverse(spark):
    X = G.overlapping_data(1000, 2, 2, seed=8)
    X = np.concatenate([X, X[:, :1]], 1)               # a duplicated feature column: every covariance is singular
    m, trace = assert_matches_reference(spark, X, None, 2, seed=6)
    assert len(trace) > 1 and np.isfinite(m.summary.logLikelihood)
    assert all(np.linalg.matrix_rank(g.cov.toArray(), tol=1e-9) == 2 for g in m.gaussians)


def test_errors(spark):
    from cdnaml.ml.clustering import GaussianMixture
    X = np.tile(np.array([[1.0, 2.0]]), (50, 1))       # identical rows: every eigenvalue is dropped
    with pytest.raises(ValueError, match="singular"):
        fit(spark, X, k=2, seed=1)
    with pytest.raises(ValueError):
        GaussianMixture(k=1).fit(frame(spark, G.overlapping_data(100, 2, 2, seed=0)))
    Xn = G.overlapping_data(200, 2, 2, seed=0)
    Xn[5, 0] = np.nan
    Xn[9, 1] = np.inf
    # for every seed, also where the initial draw hits a bad row (seed 11 does), and with maxIter = 0
    dfn = frame(spark, Xn, keep_invalid=True)
    for seed in range(1, 21):
        with pytest.raises(ValueError, match="2 rows"):
            GaussianMixture(k=2, seed=seed, maxIter=seed % 2 * 100).fit(dfn)


def test_persistence_round_trip(spark, tmp_path):
    from cdnaml.ml.clustering import GaussianMixture, GaussianMixtureModel
    X = G.overlapping_data(600, 3, 2, seed=2)
    m, df = fit(spark, X, k=2, seed=1, probabilityCol="pr")
    m.write().overwrite().save(str(tmp_path / "gmm"))
    back = GaussianMixtureModel.load(str(tmp_path / "gmm"))
    assert back.getProbabilityCol() == "pr" and back.getK() == 2 and not back.hasSummary
    for u, v in zip(params(m), params(back)):
        assert np.array_equal(u, v)
    a = m.transform(df).select("prediction").toPandas().prediction.to_numpy()
    b = back.transform(df).select("prediction").toPandas().prediction.to_numpy()
    assert np.array_equal(a, b)
    GaussianMixture(k=4, tol=0.5).write().overwrite().save(str(tmp_path / "est"))
    e2 = GaussianMixture.load(str(tmp_path / "est"))
    assert (e2.getK(), e2.getTol(), e2.getMaxIter()) == (4, 0.5, 100)


def test_pipeline_and_pyspark_alias(spark):
    from cdnaml import compat
    compat.install()
    try:
        from pyspark.ml import Pipeline
        from pyspark.ml.clustering import GaussianMixture, GaussianMixtureModel, GaussianMixtureSummary
        from pyspark.ml.feature import VectorAssembler
        X = G.separated_data(500, 2, 2, seed=4)
        pdf = pd.DataFrame(X, columns=["a", "b"])
        pipe = Pipeline(stages=[VectorAssembler(inputCols=["a", "b"], outputCol="features"),
                                GaussianMixture(k=2, seed=7)])
        pm = pipe.fit(spark.createDataFrame(pdf))
        assert isinstance(pm.stages[-1], GaussianMixtureModel)
        assert isinstance(pm.stages[-1].summary, GaussianMixtureSummary)
        out = pm.transform(spark.createDataFrame(pdf)).toPandas()
        assert set(out.prediction.unique()) == {0, 1}
    finally:
        compat.uninstall()


def test_matches_sklearn_on_separated_data(spark):
    skm = pytest.importorskip("sklearn.mixture")
    X = G.separated_data(3000, 3, 3, seed=12)
    m0, _ = fit(spark, X, k=3, seed=2, maxIter=0)
    m, _ = fit(spark, X, k=3, seed=2)
    w0, mu0, cov0 = params(m0)
    # scikit-learn stops on the change of the MEAN log-likelihood: at its default 1e-3 it stops on the plateau this
    # initial state crosses around iteration 8, where Spark's rule (total log-likelihood, 0.01) goes on
    sk = skm.GaussianMixture(3, covariance_type="full", reg_covar=0.0, tol=1e-9, weights_init=w0, means_init=mu0,
                             precisions_init=np.stack([np.linalg.inv(c) for c in cov0]), max_iter=500).fit(X)
    _, mu, cov = params(m)
    for j in range(3):
        i = int(np.argmin(((sk.means_ - mu[j]) ** 2).sum(1)))
        sd = np.sqrt(np.diag(cov[j]))
        assert (np.abs(sk.means_[i] - mu[j]) <= 1e-3 * sd).all(), (sk.means_[i], mu[j])
