"""K32 ``margin_step`` on the device under the checks of ``tests/test_margin_cpu.py`` (whose end-to-end fits run on
the GPU as well).  Every case first asserts the plan, so none silently tests the host formulation."""
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _margin_refs as R
from tests.test_aft_gpu import Counting
from tests.test_margin_cpu import LOSSES, SHAPES, check_bad_rows, check_case, check_edges

pytestmark = pytest.mark.gpu

N2 = 1025           # the smallest n the plan gives two blocks


def native_plan(X, vw, n):
    plan = K.margin_plan(X)
    assert (plan["path"], plan["vw"], plan["nblk"]) == ("native", vw, 2 if n >= N2 else 1), plan
    assert plan["slot"] == K.MARGIN_MAX_D + 5 and plan["per_cu"] == (4 if vw == 4 else 2), plan


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("d,n,vw", SHAPES)
def test_device_matches_reference(gpu_device, d, n, vw, loss, weighted):
    c = R.case(d, n, loss, weighted)
    native_plan(torch.tensor(c["X"], device=gpu_device), vw, n)
    with Counting() as calls:
        check_case(f"d={d} n={n} loss={loss} weighted={weighted}", gpu_device, True, c, loss)
    assert calls.count("cdna_margin_step") == 3, calls            # two steps and the margins


@pytest.mark.parametrize("loss", LOSSES)
def test_strided_misaligned_rows_take_the_scalar_loads(gpu_device, loss):
    """A slice of a wider, longer NaN tensor: odd row stride, off 16-byte alignment, nothing outside it is read."""
    d, n = 100, N2
    c = R.case(d, n, loss, True)
    wide = torch.full((n + 70, 103), float("nan"), device=gpu_device)
    Xs = wide[:n, 1:101]
    Xs.copy_(torch.tensor(c["X"]))
    assert Xs.stride(0) == 103 and Xs.data_ptr() % 16 != 0
    native_plan(Xs, 1, n)
    check_case(f"strided loss={loss}", gpu_device, True, c, loss, Xs)


@pytest.mark.parametrize("loss", LOSSES)
def test_branch_edges_and_bad_rows(gpu_device, loss):
    native_plan(torch.tensor(R.edge_case(loss)[0]["X"], device=gpu_device), 4, 130)
    check_edges(gpu_device, True, loss)
    for d, n, vw in [(5, 130, 1), (100, N2, 4)]:
        native_plan(torch.tensor(R.case(d, n, loss, True)["X"], device=gpu_device), vw, n)
        check_bad_rows(gpu_device, True, loss, d, n)
