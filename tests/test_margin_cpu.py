"""``K.margin_step``'s host formulation (checks shared with ``tests/test_margin_gpu.py``), LinearSVC and the Huber
LinearRegression end to end on both devices, and their two-rank gloo fits (this file is its own SPMD worker)."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cdnaml.ops import kernels as K  # noqa: E402
from tests import _margin_refs as R  # noqa: E402

# (d, n, load width): tile boundaries; the 32-column quarters; the edge of the native range; two blocks
SHAPES = [(5, 1, 1), (5, 64, 1), (5, 65, 1), (1, 130, 1), (4, 130, 4), (33, 130, 1), (127, 600, 1), (128, 600, 4),
          (100, 1025, 4)]
LOSSES = [R.HINGE, R.HUBER]


def step(dev, c, native, loss, X=None, y=None, w=None, **kw):
    w = c["w"] if w is None else w
    return K.margin_step(torch.tensor(c["X"], device=dev) if X is None else X,
                         torch.tensor(c["y"] if y is None else y, device=dev), c["coef"], c["b"],
                         None if w is None else torch.tensor(w, device=dev), loss=loss,
                         sigma=c.get("sigma", R.SIGMA), epsilon=c.get("eps", R.EPS), native=native, **kw)


def check_case(tag, dev, native, c, loss, X=None):
    a, b = step(dev, c, native, loss, X), step(dev, c, native, loss, X)
    assert all(torch.equal(u, v) for u, v in zip(a, b))          # no float atomics: the same bits twice
    m = step(dev, c, native, loss, X, mode=K.MARGIN_PREDICT)
    assert a[1].shape == (c["X"].shape[1] + 2,) and m.shape == (len(c["y"]),) and float(a[3]) == 0.0
    for i, got in enumerate([a[0].item(), a[1].cpu().numpy(), a[2].item(), m.cpu().numpy()]):
        R.check(f"margin {tag} {['loss', 'grad', 'wsum', 'margin'][i]}", got, c["ref"][i], c["yard"][i])


def check_edges(dev, native, loss):
    """Exact inputs, sums equal to the bit; the hinge's t == 0 rows add nothing: the reference leaves them out."""
    c, edge = R.edge_case(loss)
    ls, g, ws, bad = step(dev, c, native, loss)
    rl, rg, _, _ = R.evaluate(c["X"], c["y"], c["w"], c["coef"], c["b"], loss, c["sigma"], c["eps"],
                              keep=~edge if loss == R.HINGE else None)
    assert float(bad) == 0.0 and ls.item() == rl and np.array_equal(g.cpu().numpy(), rg) and ws.item() == c["w"].sum()


def check_bad_rows(dev, native, loss, d, n):
    """One bad row of each kind: the count is exact, the other sums are the reference's without those rows."""
    c = R.case(d, n, loss, True)
    rows = [0, 17, 63, 64, n - 1][:5 if loss == R.HINGE else 4]
    X, y, w = R.plant_bad(c, loss, rows)
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    ref, yard = [R.evaluate(c["X"], c["y"], c["w"], c["coef"], c["b"], loss, keep=keep, exact=e) for e in (True, False)]
    ls, g, ws, bad = step(dev, c, native, loss, torch.tensor(X, device=dev), y, w)
    assert float(bad) == len(rows)
    for i, got in enumerate([ls.item(), g.cpu().numpy(), ws.item()]):
        R.check(f"margin bad rows d={d} n={n} {['loss', 'grad', 'wsum'][i]}", got, ref[i], yard[i])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("d,n,vw", SHAPES)
def test_host_formulation_matches_reference(d, n, vw, loss, weighted):
    check_case(f"host d={d} n={n}", "cpu", False, R.case(d, n, loss, weighted), loss)


@pytest.mark.parametrize("loss", LOSSES)
def test_host_formulation_edges_and_bad_rows(loss):
    check_edges("cpu", False, loss)
    check_bad_rows("cpu", False, loss, 5, 130)


# ------------------------------------------------------------------------------------------------ end to end
HUBER_KW = dict(loss="huber", epsilon=1.5, regParam=0.01, standardization=False, tol=1e-8, maxIter=500)


def frames(spark, n=600, d=5):
    """(X, y, frame with the regression label y (10 % gross outliers), frame with a 0 / 1 label), fp32 vectors."""
    from cdnaml.ml.feature import VectorAssembler
    rng = np.random.default_rng(3)
    X = rng.normal(size=(n, d)).astype(np.float32)
    lin = X.astype(np.float64) @ np.linspace(-1.0, 1.5, d) + 0.5
    y = lin + rng.normal(scale=0.3, size=n) + rng.choice([-30.0, 40.0], n) * (rng.random(n) < 0.1)
    names = [f"x{i}" for i in range(d)]
    va = VectorAssembler(inputCols=names, outputCol="features")
    spark.conf.set("cdnaml.ml.vectorPrecision", "fp32")
    return X, y, *[va.transform(spark.createDataFrame(pd.DataFrame(X, columns=names).assign(label=lab)))
                   for lab in (y, (lin + rng.normal(scale=0.3, size=n) > 0.5).astype(np.float64))]


def native_calls(spark, fn):
    from tests.test_aft_gpu import Counting
    with Counting() as calls:
        res = fn()
    assert (calls.count("cdna_margin_step") >= 3) == (spark.device.type == "cuda"), calls
    return res


def test_huber_fit_reaches_sklearns_optimum(spark, tmp_path):
    """Both fits minimise one convex function: ours may exceed sklearn's optimum by the estimator's own tol."""
    from sklearn.linear_model import HuberRegressor
    from cdnaml.ml.regression import LinearRegression, LinearRegressionModel
    X, y, df, _ = frames(spark)
    m = native_calls(spark, lambda: LinearRegression(**HUBER_KW).fit(df))
    eps, reg = HUBER_KW["epsilon"], HUBER_KW["regParam"]
    sk = HuberRegressor(alpha=len(y) * reg, epsilon=eps, tol=1e-10, max_iter=5000).fit(X.astype(np.float64), y)
    f = [R.evaluate(X, y, None, cf, b, R.HUBER, s, eps)[0] / len(y) + 0.5 * reg * float(np.dot(cf, cf))
         for cf, b, s in [(m.coefficients.toArray(), m.intercept, m.scale), (sk.coef_, sk.intercept_, sk.scale_)]]
    print(f"huber fit: f(ours) {f[0]:.12f} f(sklearn) {f[1]:.12f} scale {m.scale:.6f} (sklearn {sk.scale_:.6f})")
    assert m.scale > 0 and len(m.summary.objectiveHistory) > 1 and f[0] <= f[1] + HUBER_KW["tol"] * abs(f[1])
    m.write().overwrite().save(str(tmp_path / "huber"))
    assert LinearRegressionModel.load(str(tmp_path / "huber")).scale == m.scale


def test_linear_svc_fit_and_transform(spark):
    from cdnaml.ml.classification import LinearSVC
    from cdnaml.ml.evaluation import MulticlassClassificationEvaluator
    from cdnaml.models.util import IllegalArgumentException
    from tests.test_ml import _cls_frame
    df, _, _ = _cls_frame(spark, n=1500)
    acc = native_calls(spark, lambda: MulticlassClassificationEvaluator(metricName="accuracy").evaluate(
        LinearSVC(maxIter=50).fit(df).transform(df)))
    assert acc > 0.7                                         # the bound of tests/test_ml.py
    with pytest.raises(IllegalArgumentException, match="label that is not 0 or 1"):
        LinearSVC(maxIter=5).fit(df.withColumn("label", df["label"] * 2.0))


# ------------------------------------------------------------------------------------------------ two ranks (gloo)
def fit_both(spark):
    from cdnaml.ml.classification import LinearSVC
    from cdnaml.ml.regression import LinearRegression
    _, _, dfh, dfs = frames(spark)
    h, s = LinearRegression(**HUBER_KW).fit(dfh), LinearSVC(regParam=0.01, tol=1e-10, maxIter=500).fit(dfs)
    return {"world": spark.comm.world_size, "theta": h.coefficients.toArray().tolist() +
            [h.intercept, h.scale] + s.coefficients.toArray().tolist() + [s.intercept]}


def _run(tmp_path, nproc):
    from tests.test_distributed import _free_port
    out = tmp_path / f"margin_{nproc}.json"
    env = dict(os.environ, CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2",
               CDNAML_CONF_CDNAML__WAREHOUSE__DIR=str(tmp_path / f"wh{nproc}"))
    launch = [] if nproc == 1 else ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
                                    "--master-addr", "127.0.0.1", "--master-port", str(_free_port())]
    r = subprocess.run([sys.executable] + launch + [os.path.abspath(__file__), str(out)], env=env,
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(out.read_text())


@pytest.mark.slow
def test_two_rank_fits_equal_the_single_rank_fits(tmp_path):
    """Two ranks sum the same fp64 terms in another order, so both runs minimise (nearly) the same function to tol
    1e-8 / 1e-10: the parameters agree to 1e-5 of the largest; a shard dropped or counted twice moves them by ~1e-2."""
    one, two = _run(tmp_path, 1), _run(tmp_path, 2)
    t1 = np.array(one["theta"])
    gap = np.abs(np.array(two["theta"]) - t1).max()
    print(f"margin models at two ranks: |theta - one rank's| = {gap:.2e}")
    assert (one["world"], two["world"]) == (1, 2) and gap <= 1e-5 * np.abs(t1).max()


if __name__ == "__main__":
    import cdnaml
    session = cdnaml.SparkSession.builder.getOrCreate()
    result = fit_both(session)
    if int(os.environ.get("RANK", "0")) == 0:
        with open(sys.argv[1], "w") as fh:
            json.dump(result, fh)
    session.comm.shutdown()
