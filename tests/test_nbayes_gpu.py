"""K34 ``nb_step`` on the device: exact sums, the reference and criterion of ``tests/_nbayes_refs.py``, the bad-row
rule and the range.  Every case first asserts the plan."""
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _nbayes_refs as R
from tests.test_nbayes_cpu import bad_rows_case, predict_case, rows_on, stats_case

pytestmark = pytest.mark.gpu

# (d, n, C, load width, strided): tile boundaries at d = 5; d around the MFMA k step of 4 and the 16-column blocks;
# C around the seam of the two class blocks; the edges of the native range.  A block takes at least 1024 rows, so
# n = 600 plans one block (several tiles, a partial last one) and only the n = 1025 cases cross two blocks
SHAPES = [(5, 1, 3, 1, 0), (5, 63, 3, 1, 0), (5, 64, 2, 1, 0), (5, 65, 3, 1, 0), (5, 130, 3, 1, 0),
          (1, 130, 3, 1, 0), (3, 130, 16, 1, 0), (4, 130, 17, 4, 0), (15, 130, 32, 1, 0), (16, 130, 2, 4, 0),
          (17, 130, 17, 1, 0), (127, 600, 32, 1, 0), (128, 600, 16, 4, 0), (100, 1025, 3, 4, 0),
          (100, 1025, 32, 4, 0), (100, 1025, 3, 1, 1)]
PREDICT_SHAPES = [(5, 130, 3, 1, 0), (4, 130, 17, 4, 0), (17, 130, 17, 1, 0), (128, 600, 32, 4, 0),
                  (100, 1025, 3, 4, 0), (100, 1025, 3, 1, 1)]


def assert_plan(dev, d, n, C, vw, strided, mode, quad):
    plan = K.nb_plan(rows_on(dev, torch.zeros((n, d)).numpy(), strided), C, mode, quad)
    want = ("native", vw, 1 if C <= 16 else 2, 2 if n >= 1025 else 1)
    assert (plan["path"], plan["vw"], plan["KB"], plan["nblk"]) == want, plan


@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("d,n,C,vw,strided", SHAPES)
def test_sums_are_exact_and_repeat(gpu_device, d, n, C, vw, strided, quad):
    assert_plan(gpu_device, d, n, C, vw, strided, K.NB_STATS, quad)
    stats_case(gpu_device, d, n, C, quad, strided)


@pytest.mark.parametrize("mt", R.TYPES)
@pytest.mark.parametrize("d,n,C,vw,strided", PREDICT_SHAPES)
def test_predict_matches_reference(gpu_device, mt, d, n, C, vw, strided):
    assert_plan(gpu_device, d, n, C, vw, strided, K.NB_PREDICT, mt == "gaussian")
    predict_case(gpu_device, mt, d, n, C, strided)


@pytest.mark.parametrize("mt", R.TYPES)
def test_bad_rows_are_counted_and_add_nothing(gpu_device, mt):
    assert_plan(gpu_device, 5, 130, 3, 1, 0, K.NB_STATS, True)
    bad_rows_case(gpu_device, mt)


def test_plan_outside_the_native_range_is_the_host_formulation(gpu_device):
    X = torch.zeros((300, 129), device=gpu_device)
    cases = ((X, 3), (X[:, :20].double(), 3), (X[:, :20], 33), (X[:, :20], 32))
    assert [K.nb_plan(*a)["path"] for a in cases] == ["host", "host", "host", "native"]
    assert [K.nb_on_range(a[0][:0], a[1]) for a in cases] == [False, False, False, True]
    # a rank with an empty shard returns its peers' shapes: one all-reduce length for all
    S, Q, W, bad = K.nb_step(X[:0, :20], torch.zeros(0), 3, quad=True)
    assert S.shape == Q.shape == (3, 20) and W.shape == bad.shape == (3,)
    assert not (S.any() or Q.any() or W.any() or bad.any())
