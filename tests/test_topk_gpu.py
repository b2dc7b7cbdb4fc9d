"""K35 ``als_topk`` on the device: exact values and positions with the tie rule, the criterion by value of
``tests/_topk_refs.py`` for rounded scores, NaN scores and the range.  Every case first asserts the plan."""
import numpy as np
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _topk_refs as R
from tests.test_topk_cpu import exact_case, nan_case, rows_on

pytestmark = pytest.mark.gpu


def assert_plan(dev, ns, nd, r, k, layout="plain"):
    plan = K.als_topk_plan(rows_on(dev, np.zeros((ns, r), np.float32), layout),
                           rows_on(dev, np.zeros((nd, r), np.float32), layout), k)
    vw = 4 if r % 4 == 0 and layout != "strided" else 1
    assert (plan["path"], plan["vw"], plan["src_blocks"]) == ("native", vw, (ns + 127) // 128), plan
    assert plan["slabs"] == -(-nd // plan["rows_per_slab"]) and (plan["slabs"] == 1) == (nd <= R.SLAB_ROWS), plan
    assert (plan["workspace"] > 0) == (plan["slabs"] > 1) and plan["lds"] <= 160 * 1024 and plan["per_cu"] >= 1, plan
    return plan


@pytest.mark.parametrize("ns,nd,r,k,layout", R.EXACT)
def test_values_and_positions_are_exact_and_repeat(gpu_device, ns, nd, r, k, layout):
    assert_plan(gpu_device, ns, nd, r, k, layout)
    exact_case(gpu_device, ns, nd, r, k, layout, True)


@pytest.mark.parametrize("ns,nd,r,k", R.ROUNDED)
def test_rounded_scores_meet_the_criterion_by_value(gpu_device, ns, nd, r, k):
    assert assert_plan(gpu_device, ns, nd, r, k)["slabs"] >= 2
    g = np.random.default_rng(1)
    S, D = g.standard_normal((ns, r), np.float32), g.standard_normal((nd, r), np.float32)
    val, idx = K.als_topk(torch.tensor(S, device=gpu_device), torch.tensor(D, device=gpu_device), k)
    R.check_rounded(S, D, k, val.cpu().numpy().astype(np.float64), idx.cpu().numpy())


def test_nan_scores_are_never_returned(gpu_device):
    assert_plan(gpu_device, 33, 65, 5, 64)
    nan_case(gpu_device, True)


def test_plan_outside_the_native_range_is_the_host_formulation(gpu_device):
    Z = torch.zeros((300, 129), device=gpu_device)
    cases = ((Z, Z, 3), (Z[:, :20].double(), Z[:, :20].double(), 3), (Z[:, :20], Z[:, :20], 65),
             (Z[:, :20].cpu(), Z[:, :20].cpu(), 3), (Z[:, :128], Z[:, :128], 64))
    assert [K.als_topk_plan(*a)["path"] for a in cases] == ["host"] * 4 + ["native"]
    exact_case(gpu_device, 33, 65, 12, 10, "plain", False)     # the host formulation on the device's tensors
