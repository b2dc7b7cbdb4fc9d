"""K34 ``nb_step``'s host formulation and NaiveBayes end to end on the CPU, against ``tests/_nbayes_refs.py``."""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ml.classification import NaiveBayes, NaiveBayesModel
from cdnaml.ml.feature import VectorAssembler
from cdnaml.models.util import IllegalArgumentException
from cdnaml.ops import kernels as K
from tests import _nbayes_refs as R
from tests._aft_refs import check

RULES = {"multinomial": (K.NB_NONNEG, -1.0), "complement": (K.NB_NONNEG, -1.0), "bernoulli": (K.NB_BINARY, 0.5),
         "gaussian": (K.NB_FINITE, None)}


def tables_of(mt, c):
    m = NaiveBayesModel(c["pi"], c["theta"], c["sigma"], mt)
    return m._tables()


def check_stats(out, S, Q, W, bad):
    """STATS' (S, Q, W, bad) equal to the bit."""
    got = [None if t is None else t.cpu().numpy() for t in out]
    assert np.array_equal(got[0], S) and np.array_equal(got[2], W) and list(got[3]) == list(bad)
    assert Q is None or np.array_equal(got[1], Q)


def check_predict(tag, mt, c, out):
    """PREDICT's (raw, prob, pred, bad) against the case's reference."""
    raw, prob, pred, bad = [t.cpu().numpy() for t in out]
    check(f"{tag} raw", raw, c["ref"][0], c["yard"][0])
    check(f"{tag} prob", prob, c["ref"][1], c["yard"][1])
    print(f"{tag}: {100 * (~c['sure']).mean():.3f} % of the rows exempt from the comparison of pred")
    assert bad == 0 and np.array_equal(pred[c["sure"]], c["ref"][1].argmax(1)[c["sure"]])


def frame(spark, X, y, w=None):
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(np.asarray(X, dtype=np.float64), columns=names)
    pdf["label"], pdf["w"] = y, np.ones(len(y)) if w is None else w
    return VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))


def rows_on(dev, X, strided=False):
    """X on the device; ``strided``: a column slice of a wider NaN-filled tensor (odd row stride, the pointer off
    16-byte alignment)."""
    Xd = torch.tensor(X, device=dev)
    if not strided:
        return Xd
    wide = torch.full((X.shape[0], X.shape[1] + 3), float("nan"), device=dev)
    wide[:, 1:X.shape[1] + 1] = Xd
    return wide[:, 1:X.shape[1] + 1]


def stats_case(dev, d, n, C, quad, strided=False):
    """Integer data: the sums equal the int64 reference bit for bit, and two calls return the same bits."""
    X, y, w, S, Q, W = R.exact_case(d, n, C)
    args = (rows_on(dev, X, strided), torch.tensor(y, device=dev), C)
    a, b = (K.nb_step(*args, w=torch.tensor(w, device=dev), quad=quad, rule=K.NB_NONNEG) for _ in range(2))
    check_stats(a, S, Q if quad else None, W, [0, 0, 0])
    assert all(u is v or torch.equal(u, v) for u, v in zip(a, b))


def bad_rows_case(dev, mt):
    """Each planted bad row lands in its own counter and adds nothing; PREDICT marks exactly the non-finite rows."""
    rule, bad_value = RULES[mt]
    X0, y0 = R.exact_case(5, 130, 3)[:2]
    X, y, w, clean, counts = R.plant(np.minimum(X0, 1) if mt == "bernoulli" else X0, y0, 3, bad_value)
    t = lambda v: torch.tensor(v, device=dev)  # noqa: E731
    out = K.nb_step(t(X), t(y), 3, w=t(w), quad=True, rule=rule)
    ref = K.nb_step(t(X[clean]), t(y[clean]), 3, quad=True, rule=rule)
    check_stats(out, *[v.cpu().numpy() for v in ref[:3]], counts)
    c = R.case(mt, 5, 130, 3)
    Xp = c["X"].copy()
    Xp[[3, 17], [0, 4]] = np.nan, -np.inf
    raw, prob, pred, bad = K.nb_step(t(Xp), None, 3, K.NB_PREDICT, tables=tables_of(mt, c))
    nanrow = torch.isnan(raw).all(1) & torch.isnan(prob).all(1)
    assert bad == 2 and nanrow.nonzero().reshape(-1).tolist() == [3, 17] and pred[3] == pred[17] == 0
    keep = np.setdiff1d(np.arange(130), [3, 17])
    assert np.abs(prob.cpu().numpy()[keep] - c["ref"][1][keep]).max() <= 1e-9


def predict_case(dev, mt, d, n, C, strided=False):
    c = R.case(mt, d, n, C)
    out = K.nb_step(rows_on(dev, c["X"], strided), None, C, K.NB_PREDICT, tables=tables_of(mt, c))
    check_predict(f"{dev} {mt} d={d} n={n} C={C}", mt, c, out)


@pytest.mark.parametrize("d,n,C", [(5, 130, 3), (17, 65, 17), (129, 70, 33)])
def test_host_sums_are_exact(d, n, C):
    stats_case("cpu", d, n, C, True)


@pytest.mark.parametrize("mt", R.TYPES)
def test_host_bad_rows_and_predict(mt):
    bad_rows_case("cpu", mt)
    predict_case("cpu", mt, 17, 300, 17)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mt", R.TYPES)
def test_estimator_matches_closed_forms(spark, tmp_path, mt, weighted):
    c = R.case(mt, 5, 130, 3)
    w = 1.0 + (np.arange(130) % 3) if weighted else None
    pi, theta, sigma = R.params(mt, c["X"], c["y"], w, 3)
    df = frame(spark, c["X"], c["y"], w)
    m = NaiveBayes(modelType=mt, weightCol="w").fit(df)     # "complement" is new with K34
    assert np.abs(m.pi.toArray() - pi).max() <= 1e-12 and np.abs(m.theta.toArray() - theta).max() <= 1e-9
    sg = m.sigma.toArray()
    assert sg.shape == ((3, 5) if mt == "gaussian" else (0, 0))
    assert mt != "gaussian" or np.abs(sg / sigma - 1).max() <= 1e-9
    m.write().overwrite().save(str(tmp_path / "nb"))
    assert np.array_equal(NaiveBayesModel.load(str(tmp_path / "nb")).sigma.toArray(), sg)
    if not weighted:
        out = m.transform(df).toPandas()
        prob = np.stack([np.asarray(v.toArray()) for v in out["probability"]])
        assert np.abs(prob - c["ref"][1]).max() <= 1e-8
        assert np.array_equal(out["prediction"].to_numpy()[c["sure"]], c["ref"][1].argmax(1)[c["sure"]])


def test_estimator_refuses_bad_values_and_model_types(spark):
    c = R.case("multinomial", 5, 130, 3)
    X = c["X"].copy()
    X[7, 2] = -1.0
    with pytest.raises(IllegalArgumentException, match="requires nonnegative feature values"):
        NaiveBayes().fit(frame(spark, X, c["y"]))
    X[7, 2] = 0.5
    with pytest.raises(IllegalArgumentException, match="requires 0 or 1 feature values"):
        NaiveBayes(modelType="bernoulli").fit(frame(spark, np.minimum(X, 1), c["y"]))
    with pytest.raises(IllegalArgumentException, match="modelType"):
        NaiveBayes(modelType="poisson").fit(frame(spark, c["X"], c["y"]))
