"""K28 ``col_digit_hist`` / ``col_select`` on the device against the numpy references of ``tests/_quantile_refs.py``, bit
for bit, and RobustScaler / MaxAbsScaler fitted on the GPU.

Every case first asserts the plan (the native path and the load width), so none silently tests the host formulation,
and counts the native calls.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _quantile_refs as R
from tests.conftest import session_device
from tests.test_aft_gpu import Counting
from tests.test_select_gpu import N2, SHAPES

pytestmark = pytest.mark.gpu

PROBS = {1: [0.5], 3: [0.25, 0.5, 0.75], 8: [0.0, 0.1, 0.25, 0.5, 0.6, 0.75, 0.99, 1.0]}


def to_np(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


def same_bits(a, b):
    """Two results of an op hold the same bits (a NaN equals the same NaN)."""
    return a.keys() == b.keys() and all(R.same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in a)


def assert_plan(Xd, Q, vw, n):
    plan = K.col_quantiles_plan(Xd, Q)
    assert (plan["path"], plan["vw"]) == ("native", vw), plan
    assert plan["nblk"] == (2 if n >= N2 else 1), plan
    if n == N2:
        assert K.col_quantiles_plan(Xd[:N2 - 1], Q)["nblk"] == 1
    assert plan["widths"] == K.col_quantile_widths(Xd.shape[1], Q) and sum(plan["widths"]) == 32
    assert plan["lds"] <= 160 * 1024
    return plan


def assert_hist(got, ref):
    got = to_np(got)
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k].dtype == np.int64 and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k


def check_passes(X, Xd, Q, plan):
    """Every pass of the plan on Xd, below the prefixes of the true quantiles: FIRST, then NEXT down to the last
    (partial) digit."""
    probs = PROBS[Q]
    n, d = X.shape
    keys = [R.keys_of(np.ascontiguousarray(X[:, c][~np.isnan(X[:, c])])).astype(np.int64) for c in range(d)]
    shift = 32
    for i, b in enumerate(plan["widths"]):
        shift -= b
        pre = None if i == 0 else R.prefixes(X, probs, 32 - shift - b)
        pd_ = None if i == 0 else torch.tensor(pre, device=Xd.device)
        with Counting() as calls:
            a = K.col_digit_hist(Xd, b, shift, pd_)
            again = K.col_digit_hist(Xd, b, shift, pd_)
        assert calls.count("cdna_col_digit_hist") == 2, calls
        assert same_bits(a, again)
        assert_hist(a, R.digit_hist(X, b, shift, pre))
        tot = a["hist"].sum(-1).cpu().numpy()
        if i == 0:
            assert np.array_equal(tot[:, 0], [k.size for k in keys])
        else:       # the values that match each target's prefix
            assert np.array_equal(tot, [[int((keys[c] >> (shift + b) == pre[c, t]).sum()) for t in range(Q)]
                                        for c in range(d)])
    assert shift == 0


@pytest.mark.parametrize("Q", [1, 3, 8])
@pytest.mark.parametrize("d,n,vw", SHAPES)
def test_digit_hist_equals_numpy(gpu_device, d, n, vw, Q):
    X = R.menu_case(d, n)
    Xd = torch.tensor(X, device=gpu_device)
    check_passes(X, Xd, Q, assert_plan(Xd, Q, vw, n))


@pytest.mark.parametrize("Q", [1, 3, 8])
def test_strided_misaligned_rows_take_the_scalar_loads(gpu_device, Q):
    """X as a column slice of a wider tensor: odd row stride, pointer off 16-byte alignment, d = 128."""
    d, n = 128, N2
    X = R.menu_case(d, n)
    wide = torch.full((n, 131), float("nan"), device=gpu_device)
    Xs = wide[:, 1:129]
    Xs.copy_(torch.tensor(X))
    assert Xs.stride(0) == 131 and Xs.data_ptr() % 16 != 0
    plan = assert_plan(Xs, Q, 1, n)
    check_passes(X, Xs, Q, plan)
    with Counting() as calls:
        got = K.col_quantiles(Xs, PROBS[Q])
    assert calls.count("cdna_col_digit_hist") == len(plan["widths"]), calls
    R.assert_quantiles(to_np(got), R.quantiles(X, PROBS[Q]))


@pytest.mark.parametrize("Q", [1, 3, 8])
@pytest.mark.parametrize("d,n,vw", [(5, 1, 1), (5, 65, 1), (33, 130, 1), (128, 600, 4), (100, N2, 4)])
def test_quantiles_equal_the_reference(gpu_device, d, n, vw, Q):
    X = R.menu_case(d, n)
    Xd = torch.tensor(X, device=gpu_device)
    plan = assert_plan(Xd, Q, vw, n)
    with Counting() as calls:
        got = K.col_quantiles(Xd, PROBS[Q])
        again = K.col_quantiles(Xd, PROBS[Q])
    assert calls.count("cdna_col_digit_hist") == 2 * len(plan["widths"]), calls
    assert calls.count("cdna_col_select") == 2 * len(plan["widths"]), calls
    assert same_bits(got, again)
    assert got["q"].dtype == torch.float32 and got["q"].shape == (Q, d)
    R.assert_quantiles(to_np(got), R.quantiles(X, PROBS[Q]))
    with Counting() as calls:
        host = K.col_quantiles(Xd, PROBS[Q], native=False)
        ext = K.col_extrema(Xd)
    assert calls.count("cdna_col_digit_hist") == 1 and "cdna_col_select" not in calls, calls
    assert host["q"].device == Xd.device
    R.assert_quantiles(to_np(host), to_np(got))
    for k in ("min", "max", "count", "nan"):
        assert R.same_bits(ext[k].cpu().numpy(), got[k].cpu().numpy()), k


@pytest.mark.parametrize("d,n", [(5, 65), (100, N2)])
def test_rows_past_the_end_are_neither_read_nor_counted(gpu_device, d, n):
    """The first n rows of a buffer whose other rows are NaN give the bits (the NaN counts too) of a tight buffer."""
    X = R.menu_case(d, n)
    Xd = torch.tensor(X, device=gpu_device)
    big = torch.full((n + 200, d), float("nan"), device=gpu_device)
    big[:n] = Xd
    assert K.col_quantiles_plan(big[:n], 3)["path"] == "native"
    with Counting() as calls:
        a = K.col_quantiles(Xd, PROBS[3])
        b = K.col_quantiles(big[:n], PROBS[3])
    assert calls.count("cdna_col_digit_hist") == 2 * len(K.col_quantiles_plan(Xd, 3)["widths"]), calls
    assert same_bits(a, b)
    R.assert_quantiles(to_np(b), R.quantiles(X, PROBS[3]))


def test_no_rows_launch_nothing_and_return_zeros(gpu_device):
    E = torch.zeros((0, 5), device=gpu_device)
    plan = K.col_quantiles_plan(E, 3)
    assert (plan["path"], plan["nblk"], plan["widths"]) == ("native", 0, K.col_quantile_widths(5, 3)), plan
    st = K.col_digit_hist(E, 8, 24)
    assert int(st["hist"].sum()) == 0 and int(st["nan"].sum()) == 0
    assert st["kmin"].tolist() == [2 ** 32 - 1] * 5 and st["kmax"].tolist() == [0] * 5
    R.assert_quantiles(to_np(K.col_quantiles(E, PROBS[3])), R.quantiles(np.zeros((0, 5), np.float32), PROBS[3]))


def test_the_python_mirror_of_the_widths_agrees_with_the_plan(gpu_device):
    Z = torch.zeros((4, 128), device=gpu_device)
    for d in range(1, 129):
        for Q in range(1, 9):
            plan = K.col_quantiles_plan(Z[:, :d], Q)
            assert plan["path"] == "native" and plan["widths"] == K.col_quantile_widths(d, Q), (d, Q, plan)
            assert plan["max_bits"][1] >= 4
    assert K.col_quantiles_plan(Z[:, :100], 3)["widths"] == [7, 6, 6, 6, 6, 1]


@pytest.mark.parametrize("what", ["f64", "d", "Q"])
def test_outside_the_native_range_takes_the_host_formulation(gpu_device, what):
    d, n = (129 if what == "d" else 20), 300
    probs = [0.0, 0.1, 0.2, 0.3, 0.5, 0.7, 0.8, 0.9, 1.0] if what == "Q" else PROBS[3]
    X = R.menu_case(d, n)
    X = X.astype(np.float64) if what == "f64" else X
    Xd = torch.tensor(X, device=gpu_device)
    assert K.col_quantiles_plan(Xd, len(probs))["path"] == "host"
    with Counting() as calls:
        got = K.col_quantiles(Xd, probs)
    assert "cdna_col_digit_hist" not in calls and "cdna_col_select" not in calls, calls
    assert got["q"].device == Xd.device
    R.assert_quantiles(to_np(got), R.quantiles(X, probs))


# ------------------------------------------------------------------------------------------------ end to end
def test_scalers_on_the_device_match_the_reference(gpu_device, tmp_path):
    import cdnaml
    from cdnaml.ml.feature import MaxAbsScaler, RobustScaler, VectorAssembler
    from cdnaml.models.util import local_batch
    d, n = 100, N2
    X = R.menu_case(d, n)
    names = [f"x{i}" for i in range(d)]
    with session_device("cuda"):
        spark = cdnaml.SparkSession.builder.config("cdnaml.warehouse.dir", str(tmp_path / "wh")).getOrCreate()
        spark.conf.set("cdnaml.ml.vectorPrecision", "fp32")
        try:
            df = VectorAssembler(inputCols=names, outputCol="features", handleInvalid="keep").transform(
                spark.createDataFrame(pd.DataFrame(X.astype(np.float64), columns=names)))
            Xv = local_batch(df, ["features"]).columns["features"].values
            assert Xv.is_cuda and Xv.dtype == torch.float32
            plan = assert_plan(Xv, 3, 4, n)
            with Counting() as calls:
                rs = RobustScaler(inputCol="features", outputCol="r", withCentering=True).fit(df)
            assert calls.count("cdna_col_digit_hist") == len(plan["widths"]), calls
            with Counting() as calls:
                ma = MaxAbsScaler(inputCol="features", outputCol="m").fit(df)
            assert calls.count("cdna_col_digit_hist") == 1, calls
            med, rng = R.robust_reference(X)
            want = R.max_abs_reference(X)
            assert R.same_bits(rs.median.toArray(), med) and R.same_bits(rs.range.toArray(), rng)
            assert R.same_bits(ma.maxAbs.toArray(), want)
            Yr = local_batch(rs.transform(df), ["r"]).columns["r"].values
            Ym = local_batch(ma.transform(df), ["m"]).columns["m"].values
            with np.errstate(divide="ignore"):
                scale = torch.tensor(np.where(rng == 0, 0.0, 1.0 / rng)).to(Xv)
            assert Yr.dtype == torch.float32 and torch.equal(Yr.view(torch.int32),
                                                             ((Xv - torch.tensor(med).to(Xv)) * scale).view(torch.int32))
            assert torch.equal(Ym.view(torch.int32),
                               (Xv / torch.tensor(np.where(want != 0, want, 1.0)).to(Xv)).view(torch.int32))
        finally:
            spark.conf.set("cdnaml.ml.vectorPrecision", "auto")
            spark.stop()
