"""GaussianMixture under SPMD: run single-process and under torchrun (gloo, CPU) by tests/test_gmm_distributed.py.

    python -m torch.distributed.run --nproc-per-node W --master-addr 127.0.0.1 --master-port P \
        tests/gmm_dist_worker.py <out.json>

Every rank fits the same global table (6001 rows: the shards are uneven at W = 2 and 3); rank 0 writes the model.
"""
import json
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(out_path):
    import cdnaml
    from cdnaml.ml.clustering import GaussianMixture
    from cdnaml.ml.feature import VectorAssembler
    from tests._gmm_refs import overlapping_data
    spark = cdnaml.SparkSession.builder.getOrCreate()
    n, d, k = 6001, 4, 3
    X = overlapping_data(n, d, k, seed=17, sep=4.0)
    names = [f"x{i}" for i in range(d)]
    pdf = pd.DataFrame(X, columns=names)
    pdf["w"] = np.random.default_rng(2).uniform(0.5, 1.5, n)
    df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))
    m = GaussianMixture(k=k, seed=5, weightCol="w").fit(df)
    res = {"world": spark.comm.world_size, "numIter": m.summary.numIter, "logLikelihood": m.summary.logLikelihood,
           "clusterSizes": m.summary.clusterSizes, "weights": m.weights,
           "means": [g.mean.toArray().tolist() for g in m.gaussians],
           "covs": [g.cov.toArray().tolist() for g in m.gaussians],
           "predicted": int(m.transform(df).count())}
    if int(os.environ.get("RANK", "0")) == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    # orderly teardown (barrier, then destroy the group), as tests/dist_worker.py
    spark.comm.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])
