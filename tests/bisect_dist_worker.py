"""BisectingKMeans with ``weightCol`` under SPMD (gloo, CPU), run by tests/test_bisect_cpu.py at one and two ranks: the
same global table, the first 4000 of 6001 rows kept by a filter.  Rank 0 writes the model."""
import json
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(out_path):
    import cdnaml
    from cdnaml.ml.clustering import BisectingKMeans
    from cdnaml.ml.feature import VectorAssembler
    spark = cdnaml.SparkSession.builder.getOrCreate()
    g = np.random.default_rng(11)
    n, names = 6001, ["x0", "x1", "x2"]
    X = np.array([[4.0, 0, 0], [-4.0, 0, 0], [0, 6.0, 0], [0, -6.0, 5.0]])[g.integers(0, 4, n)] \
        + g.standard_normal((n, 3))
    pdf = pd.DataFrame(X, columns=names)
    pdf["w"] = 0.25 + g.random(n)
    pdf["keep"] = (np.arange(n) < 4000).astype(np.float64)
    df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf)) \
        .filter("keep > 0")
    m = BisectingKMeans(k=5, seed=2, maxIter=10, weightCol="w").fit(df)
    if int(os.environ.get("RANK", "0")) == 0:
        with open(out_path, "w") as f:
            json.dump({"world": spark.comm.world_size, "index": m._index.tolist(), "cost": m.computeCost(df),
                       "centres": np.array(m.clusterCenters()).tolist(), "sizes": m.summary.clusterSizes}, f)
    else:
        m.computeCost(df)
    spark.comm.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])
