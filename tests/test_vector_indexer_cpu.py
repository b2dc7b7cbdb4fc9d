"""VectorIndexer and the host formulation of K29 against ``tests/_distinct_refs.py``.  The tests that take conftest's
``spark`` fixture run twice: on the CPU, and (marked gpu) on the device, where fp32 vectors take the K29 kernels."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _distinct_refs as R
from tests.test_quantile_cpu import column_values, vector_frame


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,d,cap", [(1, 5, 2), (65, 128, 94), (1025, 100, 20), (3000, 5, 2)])
def test_host_formulation_equals_numpy(n, d, cap, dtype):
    X, ref, X2, recoded = R.reference(n, d, cap)
    st = K.col_distinct(torch.tensor(X.astype(dtype)), cap)
    assert K.col_distinct_plan(torch.tensor(X), cap) == {"path": "host"} and K.col_distinct_max_cap(128) == 94
    R.assert_distinct(st, ref, dtype)
    for mode in K.HANDLE_INVALID:
        R.assert_recode(K.col_recode(torch.tensor(X2.astype(dtype)), st, mode), recoded[mode], dtype)


FRAME = np.array([[-1.0, 3.0, 0.5, 2.0], [0.0, 3.0, 1.5, 2.0], [-0.0, 5.0, 2.5, 2.0], [2.0, 5.0, 3.5, 2.0],
                  [0.0, 3.0, 4.5, 2.0]], dtype=np.float32)


@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_fit_transform_attributes_and_persistence(spark, tmp_path, precision):
    from cdnaml.ml.feature import VectorIndexer, VectorIndexerModel
    from cdnaml.models.util import IllegalArgumentException, categorical_info, local_batch
    spark.conf.set("cdnaml.ml.vectorPrecision", precision)
    try:
        df = vector_frame(spark, FRAME)
        with pytest.raises(IllegalArgumentException):
            VectorIndexer(inputCol="features", outputCol="ix", maxCategories=1).fit(df)
        m = VectorIndexer(inputCol="features", outputCol="ix", maxCategories=3).fit(df)
        assert m.numFeatures == 4 and m.getMaxCategories() == 3 and m.getHandleInvalid() == "error"
        assert m.categoryMaps == {0: {0.0: 0, -1.0: 1, 2.0: 2}, 1: {3.0: 0, 5.0: 1}, 3: {2.0: 0}}   # 0.0 first
        col = local_batch(m.transform(df), ["ix"]).columns["ix"]
        want = FRAME.copy()
        want[:, 0], want[:, 1], want[:, 3] = [1, 0, 0, 2, 0], [0, 0, 1, 1, 0], 0
        assert col.values.dtype == column_values(df, "features").dtype
        assert np.array_equal(col.values.cpu().numpy(), want)
        assert categorical_info(col.meta, 4, "ix") == {0: 3, 1: 2, 3: 1}
        assert [a["type"] for a in col.meta["ml_attr"]["attrs"]] == ["nominal", "binary", "numeric", "nominal"]
        m.write().overwrite().save(str(tmp_path / "vi"))
        back = VectorIndexerModel.load(str(tmp_path / "vi"))
        assert back.categoryMaps == m.copy().categoryMaps == m.categoryMaps and back.numFeatures == 4
        assert np.array_equal(column_values(back.transform(df), "ix").cpu().numpy(), want)
        unseen = FRAME.copy()
        unseen[1, 1], unseen[4, 0] = 4.0, np.nan
        du = vector_frame(spark, unseen)
        with pytest.raises(Exception, match="feature index 0"):
            m.transform(du).count()
        assert m.setHandleInvalid("skip").transform(du).count() == 3
        kept = column_values(m.setHandleInvalid("keep").transform(du), "ix").cpu().numpy()
        assert kept[1, 1] == 2 and kept[4, 0] == 3 and np.array_equal(kept[[0, 2, 3]], want[[0, 2, 3]])
        with pytest.raises(IllegalArgumentException):
            m.transform(vector_frame(spark, FRAME[:, :3])).count()
    finally:
        spark.conf.set("cdnaml.ml.vectorPrecision", "auto")


def test_decision_tree_splits_on_indexed_categories(spark):
    from cdnaml.ml.classification import DecisionTreeClassifier
    from cdnaml.ml.feature import VectorAssembler, VectorIndexer
    rng = np.random.default_rng(3)
    code = rng.integers(0, 6, size=600).astype(np.float64) * 10
    pdf = pd.DataFrame({"x0": code, "x1": rng.normal(size=600), "label": np.isin(code, [10, 40]).astype(np.float64)})
    df = VectorAssembler(inputCols=["x0", "x1"], outputCol="features").transform(spark.createDataFrame(pdf))
    ix = VectorIndexer(inputCol="features", outputCol="indexed", maxCategories=6).fit(df).transform(df)
    dt = DecisionTreeClassifier(maxDepth=2, seed=1)
    assert any(dt.setFeaturesCol("indexed").fit(ix)._forest.is_cat)
    assert not any(dt.setFeaturesCol("features").fit(df)._forest.is_cat)


@pytest.mark.slow
def test_two_ranks_fit_the_single_rank_model(tmp_path):
    """One and two ranks under torchrun (gloo, CPU), launched as tests/test_quantile_distributed.py launches."""
    from tests import vector_indexer_dist_worker as W
    from tests.test_distributed import _free_port, _port_clash
    ref = R.distinct(R.reference(W.N, W.D, W.CAP)[0], W.CAP)
    want = {str(c): [[v, i] for v, i in sorted(m.items())] for c, m in R.category_maps(ref, W.CAP).items()}
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=os.path.dirname(os.path.dirname(W.__file__)))
    for nproc in (1, 2):
        for attempt in (0, 1):      # once more on another port if the free port was taken meanwhile
            cmd = [sys.executable, "-m", "torch.distributed.run", f"--nproc-per-node={nproc}", "--master-addr",
                   "127.0.0.1", "--master-port", str(_free_port()), W.__file__, str(tmp_path / f"{nproc}.json")]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
            if r.returncode == 0 or not _port_clash(r.stderr):
                break
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        res = json.loads((tmp_path / f"{nproc}.json").read_text())
        assert 0 < len(want) < W.D and res == {"world": nproc, "numFeatures": W.D, "maps": want}
