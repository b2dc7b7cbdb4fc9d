"""MultilayerPerceptronClassifier under SPMD: run single-process and under torchrun (gloo, CPU) by
tests/test_mlp_distributed.py.

    python -m torch.distributed.run --nproc-per-node W --master-addr 127.0.0.1 --master-port P \
        tests/mlp_dist_worker.py <out.json>

Every rank fits the same global table: the first 4000 of 6001 rows, kept by a filter, so the shards are uneven at
W = 2 and the last rank's shard is empty at W = 3.  Rank 0 writes the model.
"""
import json
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS = [4, 5, 3]
MAX_ITER = 25


def main(out_path):
    import cdnaml
    from cdnaml.ml.classification import MultilayerPerceptronClassifier
    from cdnaml.ml.feature import VectorAssembler
    from cdnaml.models.classification import mlp_initial_weights
    from tests._mlp_refs import three_class_data
    spark = cdnaml.SparkSession.builder.getOrCreate()
    n = 6001
    X, y = three_class_data(n, LAYERS[0], seed=17)
    names = [f"x{i}" for i in range(LAYERS[0])]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"] = y
    pdf["keep"] = (np.arange(n) < 4000).astype(np.float64)
    df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf)) \
        .filter("keep > 0")
    from cdnaml.models.util import local_batch
    local_rows = int(local_batch(df, ["label"]).columns["label"].values.shape[0])
    m = MultilayerPerceptronClassifier(layers=LAYERS, maxIter=MAX_ITER, tol=0.0,
                                       initialWeights=mlp_initial_weights(LAYERS, 5)).fit(df)
    rows = spark.comm.all_gather_object(local_rows)
    res = {"world": spark.comm.world_size, "rows": rows, "iterations": m.summary.totalIterations,
           "objectiveHistory": [float(v) for v in m.summary.objectiveHistory],
           "weights": m.weights.toArray().tolist(), "predicted": int(m.transform(df).count())}
    if int(os.environ.get("RANK", "0")) == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    # orderly teardown (barrier, then destroy the group), as tests/dist_worker.py
    spark.comm.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])
