"""FMRegressor and FMClassifier under SPMD: run single-process and under torchrun (gloo, CPU) by
tests/test_fm_distributed.py.

    python -m torch.distributed.run --nproc-per-node W --master-addr 127.0.0.1 --master-port P \
        tests/fm_dist_worker.py <out.json>

Every rank fits the same global table: the first 4000 of 6001 rows, kept by a filter, so the shards are uneven at
W = 2 and the last rank's shard is empty at W = 3.  Rank 0 writes the models.
"""
import json
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIT = dict(factorSize=3, maxIter=25, miniBatchFraction=0.5, regParam=0.001, tol=0.0, seed=5)


def main(out_path):
    import cdnaml
    from cdnaml.ml.classification import FMClassifier
    from cdnaml.ml.feature import VectorAssembler
    from cdnaml.ml.regression import FMRegressor
    from cdnaml.models.util import local_batch
    from tests._fm_refs import product_data
    spark = cdnaml.SparkSession.builder.getOrCreate()
    n, d = 6001, 4
    X, y = product_data(n, d, seed=17)
    names = [f"x{i}" for i in range(d)]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"] = y
    pdf["sign"] = (X[:, 0] * X[:, 1] > 0).astype(np.float64)
    pdf["keep"] = (np.arange(n) < 4000).astype(np.float64)
    df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf)) \
        .filter("keep > 0")
    local_rows = int(local_batch(df, ["label"]).columns["label"].values.shape[0])
    res = {"world": spark.comm.world_size, "rows": spark.comm.all_gather_object(local_rows)}
    for name, est in (("regressor", FMRegressor(solver="adamW", stepSize=0.05, initStd=0.1, **FIT)),
                      ("classifier", FMClassifier(solver="gd", stepSize=1.0, initStd=0.5, labelCol="sign", **FIT))):
        m = est.fit(df)
        theta = np.concatenate([m.factors.toArray().reshape(-1), m.linear.toArray(), [m.intercept]])
        res[name] = {"theta": theta.tolist(), "counts": [c for _, c in m.fitHistory],
                     "loss": [float(l) for l, _ in m.fitHistory], "predicted": int(m.transform(df).count())}
    if int(os.environ.get("RANK", "0")) == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    # orderly teardown (barrier, then destroy the group), as tests/dist_worker.py
    spark.comm.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])
