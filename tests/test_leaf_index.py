"""Leaf indices on the device (K21 tree_leaf_index_kernel, K.tree_leaf_index, Forest.predict_leaf_index, leafCol)."""
import numpy as np
import pytest
import torch

import cdnaml
from cdnaml.models.util import local_batch
from cdnaml.ops import kernels as K

from tests.conftest import session_device
from tests.test_tree_shap import fitted, hand_forests, hand_rows


def walk(forest, X):
    """Straight per-row walk: numeric left iff x <= thr as fp32 (NaN right), categorical left iff the mask bit of
    int(x) is set (outside [0, 256) right) -> global node ids [n, T]."""
    X = X.numpy()
    out = np.zeros((X.shape[0], len(forest.roots)), dtype=np.int64)
    for r in range(X.shape[0]):
        for t, i in enumerate(forest.roots):
            while forest.feat[i] >= 0:
                v = X[r, forest.feat[i]]
                if forest.is_cat[i]:
                    c = int(v) if 0 <= v < 256 else -1
                    left = c >= 0 and (int(forest.catmask[i][c >> 5]) >> (c & 31)) & 1
                else:
                    left = np.float32(v) <= np.float32(forest.thr[i])
                i = forest.left[i] if left else forest.right[i]
            out[r, t] = i
    return torch.from_numpy(out)


def _check(forest, X, device):
    nodes, roots, _, masks = forest.device_arrays(torch.device(device))
    got = K.tree_leaf_index(X.to(device), nodes, roots, masks)
    assert got.dtype == torch.int32 and tuple(got.shape) == (X.shape[0], len(forest.roots))
    want = walk(forest, X)
    assert torch.equal(got.cpu().long(), want)
    via = forest.predict_leaf_index(X.to(device))
    assert via.dtype == torch.int64 and torch.equal(via.cpu(), want)
    assert bool((forest.feat.array()[want.numpy()] < 0).all())  # every id is a leaf


@pytest.mark.parametrize("k", [0, 1])
def test_leaf_index_hand_forests_cpu(k):
    _check(hand_forests()[k][0], hand_rows(), "cpu")


def test_leaf_index_fitted_forest_cpu():
    forest, _, X = fitted("rf100", "cpu")
    _check(forest, X, "cpu")
    assert tuple(forest.predict_leaf_index(X[:0]).shape) == (0, 20)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1])
def test_leaf_index_hand_forests_gpu(gpu_device, k):
    _check(hand_forests()[k][0], hand_rows(), gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rf100", "rf7", "rf300", "dt12"])
def test_leaf_index_fitted_forest_gpu(gpu_device, case):
    forest, _, X = fitted(case)
    _check(forest, X, gpu_device)
    assert tuple(forest.predict_leaf_index(X[:0].to(gpu_device)).shape) == (0, len(forest.roots))


def _leaf_column(model, X, y, device):
    with session_device(device):
        spark = cdnaml.SparkSession.builder.getOrCreate()
        try:
            df = spark.createDataFrameFromLocalTensors({"features": X.to(spark.device),
                                                        "label": y.to(spark.device)})
            out = model.transform(df)
            assert out.columns[-1] == "leaf"
            return local_batch(out, ["leaf"]).columns["leaf"].values.cpu()
        finally:
            spark.stop()


def test_leaf_col_cpu():
    """leafCol is served by the kernel's host twin: the column equals the walk."""
    forest, tw, X = fitted("rf100", "cpu")
    from cdnaml.models.regression import RandomForestRegressionModel
    m = RandomForestRegressionModel(forest, 100, tw).setLeafCol("leaf")
    col = _leaf_column(m, X, torch.zeros(X.shape[0], dtype=torch.float64), "cpu")
    assert col.dtype == torch.float64 and torch.equal(col.long(), walk(forest, X))


@pytest.mark.gpu
def test_leaf_col_cuda_equals_cpu(gpu_device):
    forest, tw, X = fitted("rf100")
    from cdnaml.models.regression import RandomForestRegressionModel
    m = RandomForestRegressionModel(forest, 100, tw).setLeafCol("leaf")
    y = torch.zeros(X.shape[0], dtype=torch.float64)
    on_gpu, on_cpu = _leaf_column(m, X, y, "cuda"), _leaf_column(m, X, y, "cpu")
    assert on_gpu.dtype == torch.float64 and torch.equal(on_gpu, on_cpu)
