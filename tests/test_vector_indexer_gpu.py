"""K29 ``col_distinct`` / ``col_recode`` on the device against the references of ``tests/_distinct_refs.py``.  Every
case first asserts the plan (the native path, the load width, the blocks): none silently tests the host formulation."""
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _distinct_refs as R
from tests.test_aft_gpu import Counting

pytestmark = pytest.mark.gpu


def on_device(X, layout, dev):
    """``vec``: contiguous rows; ``odd``: a column slice of a wider tensor (row stride d + 3, base off 16 bytes)."""
    if layout == "vec":
        return torch.tensor(X, device=dev)
    wide = torch.full((X.shape[0], X.shape[1] + 3), float("nan"), device=dev)
    wide[:, 1:1 + X.shape[1]] = torch.tensor(X, device=dev)
    return wide[:, 1:1 + X.shape[1]]


@pytest.mark.parametrize("d,cap,dtype,path", [(128, 94, "float32", "native"), (128, 95, "float32", "host"),
                                              (100, 120, "float32", "native"), (100, 121, "float32", "host"),
                                              (129, 2, "float32", "host"), (128, 2, "float64", "host")])
def test_plan_native_range(gpu_device, d, cap, dtype, path):
    X = torch.zeros((70, d), dtype=getattr(torch, dtype), device=gpu_device)
    assert K.col_distinct_plan(X, cap)["path"] == path
    with Counting() as calls:
        st = K.col_distinct(X, cap)
        K.col_recode(X, st, "keep")
    assert ("cdna_col_distinct" in calls) == ("cdna_col_recode" in calls) == (path == "native"), calls
    assert st["count"].tolist() == [1] * d and st["values"].dtype == X.dtype


@pytest.mark.parametrize("layout", ["vec", "odd"])
@pytest.mark.parametrize("capk", [2, 20, "max"])
@pytest.mark.parametrize("d", [1, 5, 100, 128])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 3000])      # 1025: the first n with two blocks
def test_distinct_and_recode_equal_numpy(gpu_device, n, d, capk, layout):
    cap = K.col_distinct_max_cap(d) if capk == "max" else capk
    X, ref, X2, recoded = R.reference(n, d, cap)
    Xd, X2d = on_device(X, layout, gpu_device), on_device(X2, layout, gpu_device)
    plan = K.col_distinct_plan(Xd, cap)
    assert (plan["path"], plan["vw"]) == ("native", 4 if layout == "vec" and d % 4 == 0 else 1), plan
    assert plan["nblk"] == -(-n // 1024) and plan["max_cap"] == K.col_distinct_max_cap(d) and plan["lds"] <= 160 * 1024
    with Counting() as calls:
        st = K.col_distinct(Xd, cap)
        got = {mode: K.col_recode(X2d, st, mode) for mode in K.HANDLE_INVALID}
    assert calls.count("cdna_col_distinct") == 1 and calls.count("cdna_col_recode") == 3, calls
    R.assert_distinct(st, ref)
    R.assert_distinct(K.col_distinct(Xd, cap, native=False), ref)      # the host formulation on the device
    for mode in K.HANDLE_INVALID:
        R.assert_recode(got[mode], recoded[mode])
        R.assert_recode(K.col_recode(X2d, st, mode, native=False), recoded[mode])
