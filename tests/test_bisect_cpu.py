"""K33 ``bisect_step``'s host formulation and BisectingKMeans on it against the numpy references of
``tests/_bisect_refs.py``, the model's tree descent and persistence, and the fit at two ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _bisect_refs as R
from tests.test_distributed import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,d,M", [(1, 5, 1), (65, 31, 2), (130, 33, 33), (600, 100, 64)])
def test_host_formulation_is_exact_on_integers(n, d, M, monkeypatch):
    monkeypatch.setattr(K, "BISECT_HOST_ELEMS", 50 * d)     # several chunks
    c, t = R.exact_case(n, d, M), R.tree_case(n, d, M % 2 == 0)
    r, tab = c["ref"], R.table(c["ents"], d) + (c["left"], c["right"])
    node, w = torch.tensor(c["node"]), torch.tensor(c["w"])
    W, cnt, S, Q, bad = K.bisect_step(torch.tensor(c["X"]), *tab, K.BISECT_STEP, node, w, shift=c["shift"])
    assert all(np.array_equal(u.numpy(), r[k]) for u, k in ((W, "W"), (cnt, "cnt"), (S, "S"), (Q, "Q"))) and bad == 0
    out, _ = K.bisect_step(torch.tensor(c["X"]), *tab, K.BISECT_ASSIGN, node, shift=c["shift"])
    want = np.where(c["node"] >= 0, np.where(r["right"], c["right"][c["node"]], c["left"][c["node"]]), -1)
    assert out is node and np.array_equal(node.numpy(), want)
    leaf, cost, bad = K.bisect_step(torch.tensor(t["X"]), *R.table(t["ents"], d), t["left"], t["right"],
                                    K.BISECT_PREDICT, w=torch.tensor(t["w"]), shift=t["shift"],
                                    centres=t["cen"] + t["shift"].astype(np.float64))
    assert np.array_equal(leaf.numpy(), t["ref"][0]) and float(cost) == t["ref"][1] and bad == 0


def _data(seed=0, n=400):
    g = np.random.default_rng(seed)
    T = np.array([[9.0, 1, 2, 0], [1.0, 8, 0, 1], [2.0, 1, 9, 3], [8.0, 7, 1, 6], [1.0, 2, 1, 9]])
    return T[g.choice(5, n, p=[0.4, 0.25, 0.2, 0.1, 0.05])] + 0.3 * g.standard_normal((n, 4)), 0.25 + g.random(n)


def _fit(spark, X, w=None, **kw):
    import pandas as pd
    from cdnaml.ml.clustering import BisectingKMeans
    from cdnaml.ml.feature import VectorAssembler
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    if w is not None:
        pdf["w"] = w
        kw["weightCol"] = "w"
    df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))   # Double rows
    return BisectingKMeans(seed=7, maxIter=6, **kw).fit(df), df


@pytest.mark.parametrize("cosine,weighted,k,min_div,fewer", [(False, False, 5, 1.0, False), (False, True, 5, 1.0, False),
                                                             (True, False, 4, 1.0, False), (True, True, 4, 1.0, False),
                                                             (False, False, 5, 150.0, True), (False, True, 5, 0.45, True)])
def test_fit_equals_the_reference_fit(spark, cosine, weighted, k, min_div, fewer):
    X, w = _data()
    w = w if weighted else None
    m, _ = _fit(spark, X, w, k=k, minDivisibleClusterSize=min_div, distanceMeasure="cosine" if cosine else "euclidean")
    info, leaves = R.fit(X, w, k, 6, min_div, cosine, np.random.default_rng(7).random((k, 4)))
    assert m._index.tolist() == sorted(info) and [int(m._index[i]) for i in m._tables()["leaves"]] == leaves
    assert (len(leaves) < k) == fewer and m.summary.k == len(leaves) and m.summary.numIter == 6
    for j, i in enumerate(m._index):
        assert abs(m._W[j] - info[i][0]) <= 1e-10 * info[i][0] and np.abs(m._C[j] - info[i][1]).max() <= 1e-10 * 10
        assert abs(m._cost[j] - info[i][2]) <= 1e-10 * info[1][2]
    assert abs(m.summary.trainingCost - sum(info[i][2] for i in leaves)) <= 1e-10 * info[1][2]
    assert sum(m.summary.clusterSizes) == len(X)


def test_fewer_distinct_points_than_k_give_fewer_leaves(spark):
    m, df = _fit(spark, np.repeat(np.array([[0.0, 1], [5.0, 1], [5.0, 9]]), [7, 5, 3], 0), k=6)
    assert sorted(map(tuple, m.clusterCenters())) == [(0.0, 1.0), (5.0, 1.0), (5.0, 9.0)]
    assert sorted(m.summary.clusterSizes) == [3, 5, 7] and m.computeCost(df) == 0.0


def test_prediction_follows_the_tree_not_the_nearest_leaf_and_survives_save_load(spark, tmp_path):
    from cdnaml.ml.clustering import BisectingKMeansModel
    C = np.array([[1.0, 0], [0.0, 0], [3.0, 0], [0.0, -5], [0.0, 5]])
    m = BisectingKMeansModel([1, 2, 3, 4, 5], C, np.zeros(5), np.ones(5))
    x = np.array([1.4, 1.0])                     # closer to node 2 than to node 3, but closest to the leaf 3
    assert np.array_equal(np.array(m.clusterCenters()), C[[3, 4, 2]]) and m.predict(x) == 1
    assert int(np.argmin(((C[[3, 4, 2]] - x) ** 2).sum(1))) == 2
    df = spark.createDataFrameFromLocalTensors({"features": torch.tensor([[1.4, 1.0], [2.0, 0], [1.5, -1]]).to(spark.device)})
    assert [r["prediction"] for r in m.transform(df).collect()] == [1, 2, 0]      # [1.5, -1] is on the root's bisector
    assert m.computeCost(df) == pytest.approx(1.96 + 16 + 1 + 2.25 + 16)
    m.save(str(tmp_path / "bkm"))
    back = BisectingKMeansModel.load(str(tmp_path / "bkm"))
    assert all(np.array_equal(getattr(m, a), getattr(back, a)) for a in ("_index", "_C", "_cost", "_W", "_shift"))
    assert [r["prediction"] for r in back.transform(df).collect()] == [1, 2, 0]


@pytest.mark.slow
def test_fit_at_two_ranks_equals_one_rank(tmp_path):
    """gloo on the CPU: both world sizes run the fp64 host formulation and differ in the order of fp64 sums only."""
    res = {}
    for nproc in (1, 2):
        out = tmp_path / f"bkm_{nproc}.json"
        env = dict(os.environ, CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT,
                   CDNAML_CONF_CDNAML__WAREHOUSE__DIR=str(tmp_path / f"wh{nproc}"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
               os.path.join(ROOT, "tests", "bisect_dist_worker.py"), str(out)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        res[nproc] = json.loads(out.read_text())
    assert res[1]["world"] == 1 and res[2]["world"] == 2 and len(res[1]["sizes"]) == 5
    c1, c2 = np.array(res[1]["centres"]), np.array(res[2]["centres"])
    assert res[1]["index"] == res[2]["index"] and res[1]["sizes"] == res[2]["sizes"]
    assert np.abs(c1 - c2).max() <= 1e-9 * np.abs(c1).max() and abs(res[1]["cost"] - res[2]["cost"]) <= 1e-9 * res[1]["cost"]
