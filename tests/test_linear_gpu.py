"""K31 ``linear_step`` on the device: the exact lane-layout case, the reference and criterion of
``tests/_linear_refs.py``, the bad-row rule, and LogisticRegression end to end.  Every case first asserts the plan."""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _linear_refs as R
from tests._aft_refs import check
from tests.conftest import session_device
from tests.test_aft_gpu import Counting

pytestmark = pytest.mark.gpu

# (d, n, K, load width, weighted, strided): tile boundaries at d = 5; d around the MFMA k step of 4 and the 16-column
# gradient blocks; the edges of the native range; K = 1 is the binomial top.  A block takes at least 1024 rows, so
# n = 600 plans one block (several tiles, a partial last one) and only the n = 1025 cases cross the seam of two blocks
SHAPES = [(5, 1, 3, 1, 0, 0), (5, 63, 1, 1, 1, 0), (5, 64, 2, 1, 0, 0), (5, 65, 3, 1, 1, 0), (5, 130, 15, 1, 0, 0),
          (1, 130, 3, 1, 1, 0), (3, 130, 1, 1, 0, 0), (4, 130, 16, 4, 1, 0), (15, 130, 17, 1, 0, 0),
          (16, 130, 32, 4, 1, 0), (17, 130, 2, 1, 0, 0), (127, 600, 32, 1, 1, 0), (128, 600, 17, 4, 0, 0),
          (128, 600, 1, 4, 1, 0), (100, 1025, 3, 4, 1, 0), (100, 1025, 16, 4, 0, 0), (100, 1025, 3, 1, 0, 1)]


def dev_t(dev, a):
    return None if a is None else torch.tensor(a, device=dev)


def assert_plan(X, Kn, vw):
    plan = K.linear_plan(X, Kn)
    want = ("native", vw, 1 if Kn <= 16 else 2, 2 if X.shape[0] >= 1025 else 1)
    assert (plan["path"], plan["vw"], plan["KB"], plan["nblk"]) == want, plan


def step(X, y, w, W, b, **kw):
    binomial = np.asarray(W).shape[0] == 1
    return K.linear_step(X, y, W[0] if binomial else W, b, w, binomial=binomial, **kw)


@pytest.mark.parametrize("d,n", [(5, 64), (17, 130), (128, 600)])
@pytest.mark.parametrize("C", [2, 4, 16, 32])
def test_lane_layout_exact(gpu_device, d, n, C):
    X, y, w, grad = R.exact_case(d, n, C)
    Xd = dev_t(gpu_device, X)
    assert_plan(Xd, C, 4 if d % 4 == 0 else 1)
    _, g, wsum, bad = K.linear_step(Xd, dev_t(gpu_device, y), np.zeros((C, d)), np.zeros(C), dev_t(gpu_device, w))
    assert float(bad) == 0.0 and float(wsum) == w.sum() and np.array_equal(g.cpu().numpy(), grad)


@pytest.mark.parametrize("d,n,Kn,vw,weighted,strided", SHAPES)
def test_device_matches_reference(gpu_device, d, n, Kn, vw, weighted, strided):
    c = R.case(d, n, Kn, bool(weighted))
    Xd, yd, wd = dev_t(gpu_device, c["X"]), dev_t(gpu_device, c["y"]), dev_t(gpu_device, c["w"])
    if strided:   # a column slice of a wider tensor: odd row stride, pointer off 16-byte alignment
        wide = torch.full((n, d + 3), float("nan"), device=gpu_device)
        wide[:, 1:d + 1] = Xd
        Xd = wide[:, 1:d + 1]
    assert_plan(Xd, Kn, vw)
    a, b = step(Xd, yd, wd, c["W"], c["b"]), step(Xd, yd, wd, c["W"], c["b"])
    pr = step(Xd, None, None, c["W"], c["b"], mode=K.LINEAR_PREDICT)
    assert all(torch.equal(u, v) for u, v in zip(a, b))      # no float atomics: the same bits twice
    R.check_all(f"d={d} n={n} K={Kn}", c, [t.cpu().numpy() for t in a], [t.cpu().numpy() for t in pr])


def test_plan_outside_the_native_range_is_the_host_formulation(gpu_device):
    X = torch.zeros((300, 129), device=gpu_device)
    cases = ((X, 3), (X[:, :20].double(), 3), (X[:, :20], 33), (X[:, :20], 32))
    assert [K.linear_plan(*a)["path"] for a in cases] == ["host", "host", "host", "native"]
    # a rank with an empty shard is on its peers' route and returns their shapes: one all-reduce length for all
    e = K.linear_step(X[:0, :20], torch.zeros(0), np.zeros((3, 20)), np.zeros(3))
    assert [K.linear_on_range(a[0][:0], a[1]) for a in cases] == [False, False, False, True]
    assert e[1].shape == (63,) and not e[1].any() and float(e[0]) == float(e[3]) == 0.0


@pytest.mark.parametrize("Kn", [1, 3])
def test_bad_rows_are_counted_and_add_nothing(gpu_device, Kn):
    from tests.test_linear_cpu import plant
    c = R.case(5, 130, Kn, True)
    X, y, w, wc = plant(c)
    Xd, Xc, yc = dev_t(gpu_device, X), dev_t(gpu_device, c["X"]), dev_t(gpu_device, c["y"])
    assert_plan(Xd, Kn, 1)
    bad = step(Xd, dev_t(gpu_device, y), dev_t(gpu_device, w), c["W"], c["b"])
    clean = step(Xc, yc, dev_t(gpu_device, wc), c["W"], c["b"])
    assert float(bad[3]) == 5 and float(clean[3]) == 0.0
    assert all(torch.equal(u, v) for u, v in zip(bad[:3], clean[:3])) and torch.isfinite(bad[1]).all()
    # margins beyond +-800
    ls, g, _, nb = step(Xc, yc, None, 2000.0 * c["W"], c["b"])
    raw = step(Xc, None, None, 2000.0 * c["W"], c["b"], mode=K.LINEAR_PREDICT)[0]
    assert float(raw.abs().max()) > 800.0 and float(nb) == 0.0
    assert torch.isfinite(ls) and torch.isfinite(g).all()


def _fit(tmp_path, X, y, w, prec, **kw):
    import cdnaml
    from cdnaml.ml.classification import LogisticRegression
    from cdnaml.ml.feature import VectorAssembler
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"], pdf["w"] = y, w
    with session_device("cuda"):
        spark = cdnaml.SparkSession.builder.config("cdnaml.warehouse.dir", str(tmp_path / f"wh_{prec}")).getOrCreate()
        spark.conf.set("cdnaml.ml.vectorPrecision", prec)
        try:
            df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))
            with Counting() as fit_calls:
                m = LogisticRegression(weightCol="w", regParam=0.01, **kw).fit(df)
            with Counting() as tr_calls:
                out = m.transform(df).select("rawPrediction", "probability", "prediction").toPandas()
            cols = [np.stack([np.asarray(v.toArray()) for v in out[k]]) for k in ("rawPrediction", "probability")]
            res = (m, m.summary.objectiveHistory[-1], cols[0], cols[1], out.prediction.to_numpy())
        finally:
            spark.conf.set("cdnaml.ml.vectorPrecision", "auto")
            spark.stop()
    return res, fit_calls, tr_calls


@pytest.mark.parametrize("C", [2, 3])
def test_fit_and_transform_run_the_kernel(gpu_device, tmp_path, C):
    from cdnaml.models.classification import BINOMIAL_ON_K31
    n, d, tol = 2000, 6, 1e-9
    X, _, w, W, b = R.make_data(d, n, C, True)
    z = X.astype(np.float64) @ (3.0 * W.T) + b + np.random.default_rng(5).gumbel(size=(n, C))
    y = z.argmax(1).astype(np.float64)
    (m, f32, raw, prob, pred), fit_calls, tr_calls = _fit(tmp_path, X, y, w, "fp32", tol=tol, maxIter=500)
    (_, f64, _, _, _), calls64, tr64 = _fit(tmp_path, X, y, w, "fp64", tol=tol, maxIter=500)
    if C > 2 or BINOMIAL_ON_K31:
        assert fit_calls.count("cdna_linear_step") >= 3, fit_calls
    assert "cdna_linear_step" not in calls64 + tr64 and tr_calls.count("cdna_linear_step") >= 1, tr_calls
    assert abs(f32 - f64) <= 10 * tol * abs(f64)
    Wm, bv = np.asarray(m.coefficientMatrix.toArray()), np.asarray(m.interceptVector.toArray())
    host = K.linear_step(torch.tensor(X, device=gpu_device), None, Wm[0] if C == 2 else Wm, bv,
                         mode=K.LINEAR_PREDICT, binomial=C == 2, native=False)
    ref, yard = R.sums(X, y, w, Wm, bv, np.longdouble), R.sums(X, y, w, Wm, bv, np.float64)
    for tag, got in (("transform", (raw, prob, pred)), ("host", [t.cpu().numpy() for t in host])):
        check(f"{tag} C={C} raw", got[0], ref[2], yard[2])
        check(f"{tag} C={C} prob", got[1], ref[3], yard[3])
        assert np.array_equal(got[2], ref[3].argmax(1))
