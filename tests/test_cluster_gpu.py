"""K30 ``cluster_step`` on the device against the numpy reference of ``tests/_cluster_refs.py``, and KMeans on it.

Integer cases are exact in fp32 and compared bit for bit.  Real-valued cases follow K24's criterion: the kernel's error
against the fp64 reference may be M = 8 times that of the same formulation in plain torch fp32 on the CPU, with a floor
of 4 fp32 ulps of the largest entry.  Every case asserts the plan first, runs twice and requires equal bits.
"""
import numpy as np
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _cluster_refs as R
from tests.conftest import session_device
from tests.test_fm_gpu import Counting

pytestmark = pytest.mark.gpu

M = 8
ULP = 2.0 ** -24

# (d, k, n, sum tiles per wave, load width).  n: tile edges, one fold after 8 tiles (600), two blocks (1100); d and k
# around the 32-tile; tiles per wave 1, 2 and 4; (128, 128) is the edge of the native range.
SHAPES = [(5, 3, 1, 1, 1), (5, 3, 63, 1, 1), (5, 3, 64, 1, 1), (5, 3, 65, 1, 1), (5, 2, 130, 1, 1), (1, 1, 130, 1, 1),
          (31, 31, 130, 1, 1), (32, 32, 130, 1, 4), (33, 33, 130, 1, 1), (100, 8, 1100, 1, 4), (128, 31, 600, 1, 4),
          (100, 33, 600, 2, 4), (100, 65, 1100, 4, 4), (33, 128, 600, 2, 1), (128, 65, 130, 4, 4),
          (128, 128, 600, 4, 4)]


def run_twice(X, C, mode, plan, **kw):
    """The op twice on the native path (asserted: plan = (slots, vw, nblk)); the results as numpy, equal bit for bit."""
    p = K.cluster_plan(X, len(C), mode)
    assert (p["path"], p["slots"], p["vw"], p["nblk"], p.get("fold_rows")) == ("native",) + plan + (512,), p
    with Counting() as calls:
        a, b = K.cluster_step(X, C, mode, **kw), K.cluster_step(X, C, mode, **kw)
    assert calls.count("cdna_cluster_step") == 2, calls
    assert all(torch.equal(u, v) or (u.isnan().all() and v.isnan().all()) for u, v in zip(a, b))
    return [t.cpu().numpy() for t in a]


def check_exact(c, Xd, slots, vw):
    nblk = 2 if len(c["X"]) > 1024 else 1
    kw = dict(w=torch.tensor(c["w"], device=Xd.device), shift=c["shift"])
    a, S, N, cost, bad = run_twice(Xd, c["C"], K.CLUSTER_STEP, (slots, vw, nblk), **kw)
    r = c["ref"]
    assert np.array_equal(a, r["assign"]) and np.array_equal(S, r["sums"]) and np.array_equal(N, r["N"])
    assert cost == r["cost"] and bad == 0
    a, cost, bad = run_twice(Xd, c["C"], K.CLUSTER_PREDICT, (0, vw, nblk))
    assert np.array_equal(a, c["ref1"]["assign"]) and cost == c["ref1"]["cost"] and bad == 0


@pytest.mark.parametrize("d,k,n,slots,vw", SHAPES + [(100, 8, 1100, 1, 1)])
def test_integer_cases_bit_for_bit(gpu_device, d, k, n, slots, vw):
    c = R.exact_case(d, k, n)
    assert k < 3 or (c["ref"]["N"][1] == 0 and c["ref"]["N"][-1] == 0)   # the empty centre, the tied one
    Xd = torch.tensor(c["X"], device=gpu_device)
    if vw == 1 and d % 4 == 0:      # a column slice of a wider tensor: odd row stride, off 16-byte alignment
        Xd = torch.full((n, d + 3), float("nan"), device=gpu_device)[:, 1:d + 1].copy_(Xd)
        assert Xd.stride(0) == d + 3 and Xd.data_ptr() % 16 != 0
    check_exact(c, Xd, slots, vw)


def test_nan_and_overflowing_rows_follow_the_host_formulation(gpu_device):
    c = R.exact_case(32, 3, 130)
    X = torch.tensor(c["X"], device=gpu_device)
    X[5, 7], X[64, 0], X[70] = float("nan"), float("inf"), 3e38
    w = torch.tensor(c["w"], device=gpu_device).clamp_min(0.5)
    dev = run_twice(X, c["C"], K.CLUSTER_STEP, (1, 4, 1), w=w, shift=c["shift"])
    host = [t.cpu().numpy() for t in K.cluster_step(X, c["C"], K.CLUSTER_STEP, w, shift=c["shift"], native=False)]
    assert dev[4] == host[4] == 3 and list(dev[0][[5, 64, 70]]) == [0, 0, 0] and np.isnan(dev[3]) and np.isnan(host[3])
    assert all(np.array_equal(u, v) for u, v in zip(dev[:3], host[:3])) and np.isfinite(dev[1]).all()
    assert float(K.cluster_step(X[6:], c["C"], K.CLUSTER_PREDICT, w[6:], shift=c["shift"])[1]) == float("inf")


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("d,k,n,slots", [(20, 4, 600, 1), (100, 8, 1100, 1), (100, 65, 1100, 4)])
def test_blobs_far_from_the_origin_within_the_yardstick(gpu_device, d, k, n, slots, cosine):
    c = R.blob_case(d, k, n, cosine)
    r, (ys, yc) = c["ref"], c["yard"]
    assert r["margin"].min() > 1e-3, r["margin"].min()
    kw = dict(w=torch.tensor(c["w"], device=gpu_device), cosine=cosine, shift=c["shift"])
    a, S, N, cost, bad = run_twice(torch.tensor(c["X"], device=gpu_device), c["C"], K.CLUSTER_STEP,
                                   (slots, 4, 2 if n > 1024 else 1), **kw)
    es, ec = np.abs(S - r["sums"]).max(), abs(cost - r["cost"])
    bs = max(M * np.abs(ys - r["sums"]).max(), 4 * ULP * np.abs(r["sums"]).max())
    bc = max(M * abs(yc - r["cost"]), 4 * ULP * abs(r["cost"]))
    print(f"cluster d={d} k={k} n={n} cosine={cosine}: sums kernel {es:.2e} yardstick {np.abs(ys - r['sums']).max():.2e}"
          f" bound {bs:.2e} | cost kernel {ec:.2e} yardstick {abs(yc - r['cost']):.2e} bound {bc:.2e} | margin "
          f"{r['margin'].min():.2e}")
    assert np.array_equal(a, r["assign"]) and bad == 0 and np.abs(N - r["N"]).max() <= 1e-12 * r["N"].max()
    assert es <= bs and ec <= bc


def test_cosine_fit_and_transform_run_the_kernel_without_a_copy_of_the_rows(gpu_device, tmp_path):
    import cdnaml
    from cdnaml.models.clustering import KMeans
    from cdnaml.models.util import local_batch
    n, d = 200000, 16
    c = R.blob_case(d, 4, 2000, True)
    with session_device("cuda"):
        spark = cdnaml.SparkSession.builder.config("cdnaml.warehouse.dir", str(tmp_path / "wh")).getOrCreate()
        try:
            X = torch.tensor(c["X"], device=spark.device).repeat(n // 2000, 1)
            df = spark.createDataFrameFromLocalTensors({"features": X})
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            with Counting() as calls:
                m = KMeans(k=4, seed=1, maxIter=5, distanceMeasure="cosine").fit(df)
                pred = local_batch(m.transform(df), ["prediction"]).columns["prediction"].values
            peak = torch.cuda.max_memory_allocated() - base
        finally:
            spark.stop()
    assert calls.count("cdna_cluster_step") >= 3 and "cdna_kmeans_step" not in calls, calls
    assert peak < n * d * 4, (peak, n * d * 4)                   # no normalised copy of the rows
    ref = R.step(c["X"], np.array(m.clusterCenters()), cosine=True)
    assert np.array_equal(pred.cpu().numpy()[:2000], ref["assign"]) and sorted(m.summary.clusterSizes)[0] > 0
