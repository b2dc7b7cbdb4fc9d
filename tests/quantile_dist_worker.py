"""K.col_quantiles and RobustScaler / MaxAbsScaler under SPMD: run single-process and under torchrun (gloo, CPU) by
tests/test_quantile_distributed.py.

    python -m torch.distributed.run --nproc-per-node W --master-addr 127.0.0.1 --master-port P \
        tests/quantile_dist_worker.py <out.json>

Every rank works on the same global table: the first 4000 of 6001 rows, kept by a filter, so the shards are uneven at
W = 2 and the last rank's shard is empty at W = 3.  Rank 0 writes the results as bit patterns.
"""
import json
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, KEPT, D = 6001, 4000, 12
PROBS = [0.0, 0.25, 0.5, 0.75, 1.0]
LOWER, UPPER = 0.1, 0.8


def table():
    """X fp32 [N, D] of the adversarial menu: the global table, the same in every process."""
    from tests._quantile_refs import menu_case
    return menu_case(D, N, seed=21)


def main(out_path):
    import cdnaml
    from cdnaml.ml.feature import MaxAbsScaler, RobustScaler, VectorAssembler
    from cdnaml.models.util import local_xyw
    from cdnaml.ops import kernels as K
    from tests._quantile_refs import bits
    spark = cdnaml.SparkSession.builder.getOrCreate()
    comm = spark.comm
    names = [f"x{i}" for i in range(D)]
    pdf = pd.DataFrame(table().astype(np.float64), columns=names)
    pdf["keep"] = (np.arange(N) < KEPT).astype(np.float64)
    res = {"world": comm.world_size}
    for precision in ("fp32", "auto"):
        spark.conf.set("cdnaml.ml.vectorPrecision", precision)
        df = VectorAssembler(inputCols=names, outputCol="features", handleInvalid="keep") \
            .transform(spark.createDataFrame(pdf)).filter("keep > 0")
        X, _, _ = local_xyw(df, "features", keep_f64=True)
        res["rows"] = comm.all_gather_object(int(X.shape[0]))
        st = K.col_quantiles(X, PROBS, comm)
        ext = K.col_extrema(X, comm)
        assert all(np.array_equal(bits(st[k].numpy()), bits(ext[k].numpy())) for k in ("min", "max", "count", "nan"))
        rs = RobustScaler(inputCol="features", outputCol="r", lower=LOWER, upper=UPPER).fit(df)
        ma = MaxAbsScaler(inputCol="features", outputCol="m").fit(df)
        assert int(ma.transform(rs.transform(df)).count()) == KEPT
        res[precision] = {"dtype": str(X.dtype), "q": bits(st["q"].numpy()).reshape(-1).tolist(),
                          "min": bits(st["min"].numpy()).tolist(), "max": bits(st["max"].numpy()).tolist(),
                          "count": st["count"].tolist(), "nan": st["nan"].tolist(),
                          "median": bits(rs.median.toArray()).tolist(), "range": bits(rs.range.toArray()).tolist(),
                          "maxAbs": bits(ma.maxAbs.toArray()).tolist()}
    if int(os.environ.get("RANK", "0")) == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    # orderly teardown (barrier, then destroy the group), as tests/dist_worker.py
    spark.comm.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])
