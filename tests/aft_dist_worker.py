"""AFTSurvivalRegression under SPMD: run single-process and under torchrun (gloo, CPU) by
tests/test_aft_distributed.py.

    python -m torch.distributed.run --nproc-per-node W --master-addr 127.0.0.1 --master-port P \
        tests/aft_dist_worker.py <out.json>

Every rank fits the same global table: the first 4000 of 6001 rows, kept by a filter, so the shards are uneven at
W = 2 and the last rank's shard is empty at W = 3.  Rank 0 writes the model.
"""
import json
import math
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(out_path):
    import cdnaml
    from cdnaml.ml.feature import VectorAssembler
    from cdnaml.ml.regression import AFTSurvivalRegression
    from cdnaml.models.util import local_batch
    from tests._aft_refs import make_data
    spark = cdnaml.SparkSession.builder.getOrCreate()
    n, d = 6001, 4
    X, t, censor, _, _ = make_data(d, n, seed=17, dtype=np.float64)
    names = [f"x{i}" for i in range(d)]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"], pdf["censor"] = t, censor
    pdf["keep"] = (np.arange(n) < 4000).astype(np.float64)
    df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf)) \
        .filter("keep > 0")
    local_rows = int(local_batch(df, ["label"]).columns["label"].values.shape[0])
    res = {"world": spark.comm.world_size, "rows": spark.comm.all_gather_object(local_rows)}
    m = AFTSurvivalRegression(tol=1e-14, maxIter=500, quantilesCol="q").fit(df)
    res["theta"] = m.coefficients.toArray().tolist() + [m.intercept, math.log(m.scale)]
    res["predicted"] = int(m.transform(df).count())
    if int(os.environ.get("RANK", "0")) == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    # orderly teardown (barrier, then destroy the group), as tests/dist_worker.py
    spark.comm.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])
