"""K30 ``cluster_step``'s host formulation against the numpy reference of ``tests/_cluster_refs.py``, and KMeans with
``weightCol`` on both devices and at two ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _cluster_refs as R
from tests.test_distributed import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("d,k,n", [(1, 1, 1), (5, 3, 65), (33, 33, 130), (100, 8, 1100)])
def test_host_formulation_is_exact_on_integers(d, k, n, monkeypatch):
    monkeypatch.setattr(K, "CLUSTER_HOST_ELEMS", 50 * k * d)     # several chunks
    c = R.exact_case(d, k, n)
    a, S, N, cost, bad = K.cluster_step(torch.tensor(c["X"]), c["C"], K.CLUSTER_STEP, torch.tensor(c["w"]),
                                        shift=c["shift"])
    r = c["ref"]
    assert np.array_equal(a.numpy(), r["assign"]) and np.array_equal(S.numpy(), r["sums"])
    assert np.array_equal(N.numpy(), r["N"]) and float(cost) == r["cost"] and float(bad) == 0
    a1, cost1, _ = K.cluster_step(torch.tensor(c["X"]).double(), c["C"], K.CLUSTER_PREDICT)
    assert np.array_equal(a1.numpy(), c["ref1"]["assign"]) and float(cost1) == c["ref1"]["cost"]


def test_host_formulation_cosine_and_bad_rows():
    c = R.blob_case(20, 4, 300, True)
    X = torch.tensor(c["X"])
    a, S, N, cost, _ = K.cluster_step(X, c["C"], K.CLUSTER_STEP, torch.tensor(c["w"]), cosine=True)
    r = c["ref"]
    assert np.array_equal(a.numpy(), r["assign"]) and abs(float(cost) - r["cost"]) <= 1e-12 * 300
    np.testing.assert_allclose(S.numpy(), r["sums"], rtol=0, atol=1e-12 * np.abs(r["sums"]).max())
    X[3, 2], X[7, 0] = float("nan"), float("inf")
    a, S2, N2, cost, bad = K.cluster_step(X, c["C"], K.CLUSTER_STEP, torch.tensor(c["w"]), cosine=True)
    assert float(bad) == 2 and a[3] == 0 and a[7] == 0 and np.isnan(float(cost)) and torch.isfinite(S2).all()


def _blobs(n, seed):
    g = np.random.default_rng(seed)
    X = (np.array([[5.0, 0, 0, 0], [-5.0, 0, 0, 0]])[g.integers(0, 2, n)] + g.standard_normal((n, 4)))
    return X.astype(np.float32), 1 + 2 * (X[:, 1] > 0).astype(np.int64)


def _fit(spark, X, w=None, **kw):
    from cdnaml.models.clustering import KMeans
    cols = {"features": torch.tensor(X).to(spark.device)}
    if w is not None:
        cols["w"] = torch.tensor(w, dtype=torch.float64).to(spark.device)
        kw["weightCol"] = "w"
    m = KMeans(k=2, seed=3, maxIter=30, tol=0.0, **kw).fit(spark.createDataFrameFromLocalTensors(cols))
    C = np.array(m.clusterCenters())
    return C[np.argsort(C[:, 0])], m.summary


def test_integer_weights_are_repeated_rows(spark):
    """Weights 1 and 3 against the fit on the rows repeated that often.  Both converge to the two blobs' weighted
    means; the fp32 partial sums of at most 512 rows are ordered differently: 512 2^-24 = 3e-5 relative."""
    X, w = _blobs(900, 0)
    Cw, sw = _fit(spark, X, w)
    Cr, sr = _fit(spark, np.repeat(X, w, 0))
    Cu, su = _fit(spark, X)
    print(f"weighted KMeans on {spark.device}: |Cw - Cr| {np.abs(Cw - Cr).max():.2e} |Cw - Cu| "
          f"{np.abs(Cw - Cu).max():.2e} cost {sw.trainingCost:.6f} / {sr.trainingCost:.6f}")
    assert np.abs(Cw - Cr).max() <= 1e-4 * 5 and abs(sw.trainingCost - sr.trainingCost) <= 1e-4 * sr.trainingCost
    assert np.abs(Cw - Cu).max() > 0.1                           # the weights pull every centre towards x1 > 0
    assert sorted(sw.clusterSizes) == sorted(su.clusterSizes) and sum(sw.clusterSizes) == 900   # row counts


@pytest.mark.slow
def test_weighted_fit_at_two_ranks_equals_one_rank(tmp_path):
    """gloo on the CPU: both world sizes run the fp64 host formulation and differ in the order of fp64 sums only."""
    res = {}
    for nproc in (1, 2):
        out = tmp_path / f"km_{nproc}.json"
        env = dict(os.environ, CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT,
                   CDNAML_CONF_CDNAML__WAREHOUSE__DIR=str(tmp_path / f"wh{nproc}"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
               os.path.join(ROOT, "tests", "cluster_dist_worker.py"), str(out)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        res[nproc] = json.loads(out.read_text())
    assert res[1]["world"] == 1 and res[2]["world"] == 2 and sum(res[2]["rows"]) == 4000
    c1, c2 = np.array(res[1]["centres"]), np.array(res[2]["centres"])
    assert np.abs(c1 - c2).max() <= 1e-9 * np.abs(c1).max()
    assert abs(res[1]["cost"] - res[2]["cost"]) <= 1e-9 * res[1]["cost"] and res[1]["sizes"] == res[2]["sizes"]
