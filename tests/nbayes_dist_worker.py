"""NaiveBayes under SPMD: run single-process and under torchrun (gloo, CPU) by tests/test_nbayes_distributed.py.

    python -m torch.distributed.run --nproc-per-node W --master-addr 127.0.0.1 --master-port P \\
        tests/nbayes_dist_worker.py <out.json>

Every rank builds the same global tables (counts, and Gaussian rows at an offset of 1e3); rank 0 writes the models.
"""
import json
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(out_path, d=6, n=701, C=3):
    import cdnaml
    from cdnaml.ml.classification import NaiveBayes
    from cdnaml.ml.feature import VectorAssembler
    from tests._nbayes_refs import TYPES, make_data
    spark = cdnaml.SparkSession.builder.getOrCreate()
    names = [f"x{i}" for i in range(d)]
    res = {"world": spark.comm.world_size}
    for mt in TYPES:
        X, y = make_data(mt, d, n, C)
        pdf = pd.DataFrame(X.astype(np.float64), columns=names)
        pdf["label"], pdf["w"] = y, 1.0 + np.arange(n) % 3
        df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))
        m = NaiveBayes(modelType=mt, weightCol="w").fit(df)
        res[mt] = [m.pi.toArray().tolist(), m.theta.toArray().tolist(), m.sigma.toArray().tolist()]
    if int(os.environ.get("RANK", "0")) == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    spark.comm.shutdown()   # orderly teardown (barrier, then destroy the group), as tests/dist_worker.py


if __name__ == "__main__":
    main(sys.argv[1])
