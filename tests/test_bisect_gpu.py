"""K33 ``bisect_step`` on the device against the numpy references of ``tests/_bisect_refs.py``, and BisectingKMeans on it.

Integer cases are exact in fp32 and compared bit for bit.  Real-valued cases follow K24's and K30's criterion: the
kernel's error against the fp64 reference may be M = 8 times that of the same formulation in plain torch fp32 on the
CPU, with a floor of 4 fp32 ulps of the largest entry.  Every case asserts the plan first, runs twice and requires equal
bits.
"""
import numpy as np
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _bisect_refs as R
from tests.conftest import session_device
from tests.test_fm_gpu import Counting

pytestmark = pytest.mark.gpu

M8 = 8
ULP = 2.0 ** -24

# (n, d, entries, sum tiles per wave, load width).  n: tile edges, one fold after 8 tiles (600), two blocks (1100); d
# around the 32-tile; 1, 2 and 4 tiles per wave; the last is a slice with an odd row stride off 16-byte alignment.
SHAPES = [(1, 5, 1, 1, 1), (63, 5, 2, 1, 1), (64, 1, 2, 1, 1), (65, 31, 33, 1, 1), (130, 32, 33, 1, 4),
          (130, 33, 64, 2, 1), (600, 100, 33, 4, 4), (1100, 100, 2, 1, 4), (600, 128, 64, 4, 4), (1100, 128, 1, 1, 4),
          (1100, 100, 64, 4, 1)]


def run_twice(X, tab, mode, plan, leaves=1, **kw):
    """The op twice on the native path (asserted: plan = (slots, vw, nblk)); the results as numpy, equal bit for bit."""
    p = K.bisect_plan(X, len(tab[1]), mode, leaves)
    assert (p["path"], p["slots"], p["vw"], p["nblk"], p.get("fold_rows")) == ("native",) + plan + (512,), p
    node = kw.pop("node", None)
    with Counting() as calls:
        a, b = (K.bisect_step(X, *tab, mode, None if node is None else node.clone(), **kw) for _ in range(2))
    assert calls.count("cdna_bisect_step") == 2, calls
    assert all(torch.equal(u, v) or (u.isnan().all() and v.isnan().all()) for u, v in zip(a, b))
    return [t.cpu().numpy() for t in a]


def device_rows(X, dev, odd):
    Xd = torch.tensor(X, device=dev)
    if odd:      # a column slice of a wider tensor: odd row stride, off 16-byte alignment
        n, d = X.shape
        Xd = torch.full((n, d + 3), float("nan"), device=dev)[:, 1:d + 1].copy_(Xd)
        assert Xd.stride(0) == d + 3 and Xd.data_ptr() % 16 != 0
    return Xd


@pytest.mark.parametrize("n,d,M,slots,vw", SHAPES)
def test_integer_step_and_assign_bit_for_bit(gpu_device, n, d, M, slots, vw):
    c = R.exact_case(n, d, M)
    r, nblk = c["ref"], 2 if n > 1024 else 1
    assert not r["right"][0] and (M < 3 or (r["W"][0, 1] == 0 and r["W"][1, 0] == 0 and not r["cnt"][M - 1].any()))
    assert (c["node"] == -1).any() or n == 1
    Xd = device_rows(c["X"], gpu_device, vw == 1 and d % 4 == 0)
    tab = R.table(c["ents"], d) + (c["left"], c["right"])
    kw = dict(node=torch.tensor(c["node"], device=gpu_device), shift=c["shift"])
    W, cnt, S, Q, bad = run_twice(Xd, tab, K.BISECT_STEP, (slots, vw, nblk), w=torch.tensor(c["w"], device=gpu_device),
                                  **kw)
    assert all(np.array_equal(u, r[k]) for u, k in ((W, "W"), (cnt, "cnt"), (S, "S"), (Q, "Q"))) and bad == 0
    node, bad = run_twice(Xd, tab, K.BISECT_ASSIGN, (0, vw, nblk), **kw)
    want = np.where(c["node"] >= 0, np.where(r["right"], c["right"][c["node"]], c["left"][c["node"]]), -1)
    assert np.array_equal(node, want) and bad == 0


@pytest.mark.parametrize("n,d,chain,vw", [(130, 1, True, 1), (1100, 100, True, 4), (600, 33, False, 1),
                                          (1100, 128, False, 4)])
def test_integer_predict_bit_for_bit(gpu_device, n, d, chain, vw):
    c = R.tree_case(n, d, chain)
    leaf, cost = c["ref"]
    assert leaf.max() == len(c["cen"]) - 1 or not chain           # the worst-case walk: 31 steps
    tab = R.table(c["ents"], d) + (c["left"], c["right"])
    out = run_twice(torch.tensor(c["X"], device=gpu_device), tab, K.BISECT_PREDICT, (0, vw, 2 if n > 1024 else 1),
                    len(c["cen"]), w=torch.tensor(c["w"], device=gpu_device), shift=c["shift"], centres=c["cen"] +
                    c["shift"].astype(np.float64))
    assert np.array_equal(out[0], leaf) and out[1] == cost and out[2] == 0


def test_nan_and_overflowing_rows_follow_the_host_formulation(gpu_device):
    c = R.exact_case(130, 32, 33)
    X = torch.tensor(c["X"], device=gpu_device)
    X[5, 7], X[64, 0], X[70] = float("nan"), float("inf"), 3e38
    w = torch.tensor(c["w"], device=gpu_device).clamp_min(0.5)
    tab = R.table(c["ents"], 32) + (c["left"], c["right"])
    node = torch.tensor(c["node"], device=gpu_device)
    cen = np.arange(5.0)[:, None] * np.ones(32)
    ptab = (np.ones((4, 32)), [0.0, 1.0, 2.0, 3.0], [-1, -2, -3, -4], [1, 2, 3, -5])
    for mode, plan, t, kw in ((K.BISECT_STEP, (1, 4, 1), tab, dict(node=node, w=w)),
                              (K.BISECT_ASSIGN, (0, 4, 1), tab, dict(node=node)),
                              (K.BISECT_PREDICT, (0, 4, 1), ptab, dict(w=w, centres=cen))):
        dev = run_twice(X, t, mode, plan, 5, shift=c["shift"], **kw)
        nd = kw.pop("node", None)
        host = K.bisect_step(X, *t, mode, None if nd is None else nd.clone(), shift=c["shift"], native=False, **kw)
        assert all(np.array_equal(u, v.cpu().numpy(), equal_nan=True) for u, v in zip(dev, host)) and dev[-1] == 3
    assert np.isnan(dev[1]) and list(dev[0][[5, 64, 70]]) == [0, 0, 0]
    assert float(K.bisect_step(X[6:], *ptab, K.BISECT_PREDICT, w=w[6:], shift=c["shift"], centres=cen)[1]) == float("inf")


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("n,d,M,slots", [(600, 20, 2, 1), (1100, 100, 4, 1), (1100, 100, 33, 4)])
def test_blobs_far_from_the_origin_within_the_yardstick(gpu_device, n, d, M, slots, cosine):
    c = R.blob_case(n, d, M, cosine)
    r, (ys, yq) = c["ref"], c["yard"]
    assert c["margin"].min() > 1e-3, c["margin"].min()
    Xd, wd = torch.tensor(c["X"], device=gpu_device), torch.tensor(c["w"], device=gpu_device)
    node = torch.tensor(c["node"], device=gpu_device)
    tab = R.table(c["ents"], d) + ([2 * e for e in range(M)], [2 * e + 1 for e in range(M)])
    nblk = 2 if n > 1024 else 1
    W, cnt, S, Q, bad = run_twice(Xd, tab, K.BISECT_STEP, (slots, 4, nblk), node=node, w=wd, cosine=cosine,
                                  shift=c["shift"])
    side, _ = run_twice(Xd, tab, K.BISECT_ASSIGN, (0, 4, nblk), node=node, cosine=cosine, shift=c["shift"])
    # PREDICT on the rows of entry 0 (the margin holds at their own entry only): the one-entry tree of its two blobs,
    # whose centres are fp32 values, as the op rounds them for fp32 rows
    m0, sh64 = c["node"] == 0, c["shift"].astype(np.float64)
    cen = c["cen"][:2].astype(np.float32).astype(np.float64)
    ptab = (tab[0][:1], tab[1][:1], [-1], [-2])
    pref = R.predict(c["X"][m0], c["ents"][:1], [-1], [-2], cen, c["w"][m0], cosine, sh64)
    leaf, cost, pbad = run_twice(Xd[torch.tensor(m0)], ptab, K.BISECT_PREDICT, (0, 4, 1), 2, w=wd[torch.tensor(m0)],
                                 cosine=cosine, shift=c["shift"], centres=cen if cosine else cen + sh64)
    yc = R.yard_cost(c["X"][m0], cen[pref[0]], c["w"][m0], cosine, c["shift"])
    errs = [np.abs(S - r["S"]).max(), np.abs(Q - r["Q"]).max(), abs(cost - pref[1])]
    yard = [np.abs(ys - r["S"]).max(), np.abs(yq - r["Q"]).max(), abs(yc - pref[1])]
    big = [np.abs(r["S"]).max(), np.abs(r["Q"]).max(), abs(pref[1])]
    print(f"bisect n={n} d={d} M={M} cosine={cosine}: S, Q, cost errors {errs} yardstick {yard} largest {big} margin "
          f"{c['margin'].min():.2e}")
    assert np.array_equal(side, 2 * c["node"] + r["right"]) and np.array_equal(leaf, pref[0]) and bad == pbad == 0
    assert np.abs(W - r["W"]).max() <= 1e-12 * r["W"].max() and np.array_equal(cnt, r["cnt"])
    assert all(e <= max(M8 * y, 4 * ULP * b) for e, y, b in zip(errs, yard, big))


def test_fit_runs_the_kernel_without_a_copy_of_the_rows(gpu_device, tmp_path):
    import cdnaml
    from cdnaml.models.clustering import BisectingKMeans
    n, d, k = 200000, 16, 6
    X = R.blob_case(2000, d, 4, False)["X"]
    with session_device("cuda"):
        spark = cdnaml.SparkSession.builder.config("cdnaml.warehouse.dir", str(tmp_path / "wh")).getOrCreate()
        try:
            df = spark.createDataFrameFromLocalTensors({"features": torch.tensor(X, device=spark.device)
                                                        .repeat(n // 2000, 1)})
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            with Counting() as calls:
                m = BisectingKMeans(k=k, seed=5, maxIter=8).fit(df)
            peak = torch.cuda.max_memory_allocated() - base
        finally:
            spark.stop()
    assert calls.count("cdna_bisect_step") >= 10 and not {"cdna_kmeans_step", "cdna_cluster_step"} & set(calls), calls
    assert peak < n * d * 4, (peak, n * d * 4)
    noise = np.random.default_rng(5).random((k, d))
    info, leaves = R.fit(np.tile(X.astype(np.float64), (n // 2000, 1)), None, k, 8, 1.0, False, noise)
    assert [int(m._index[i]) for i in m._tables()["leaves"]] == leaves and sorted(info) == m._index.tolist()
    C, ref = np.array(m.clusterCenters()), np.array([info[i][1] for i in leaves])
    assert np.abs(C - ref).max() <= 1e-5 * np.abs(ref).max(), np.abs(C - ref).max()
    assert m.summary.clusterSizes == [int(info[i][0]) for i in leaves]
