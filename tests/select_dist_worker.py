"""The univariate tests and selectors under SPMD: run single-process and under torchrun (gloo, CPU) by
tests/test_select_distributed.py.

    python -m torch.distributed.run --nproc-per-node W --master-addr 127.0.0.1 --master-port P \
        tests/select_dist_worker.py <out.json>

Every rank works on the same global tables: the first 4000 of 6001 rows, kept by a filter, so the shards are uneven
at W = 2 and the last rank's shard is empty at W = 3.  Rank 0 writes the results.
"""
import json
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, KEPT, D, KC, CC = 6001, 4000, 8, 7, 3


def tables():
    """(X of categories, X continuous, codes, y): the global tables, the same in every process."""
    from tests._select_refs import make_continuous, make_counts
    Xk, codes = make_counts(D, N, KC, CC, seed=21)
    Xc, _, y = make_continuous(D, N, CC, seed=21, dtype=np.float64)
    # the class signal of the continuous table follows the count table's label
    Xc = Xc + (1.0 / (1 + np.arange(D)) ** 1.5)[None, :] * (codes[:, None] - 1.0)
    return Xk.astype(np.float64), Xc, codes, y


def main(out_path):
    import cdnaml
    from cdnaml.ml.feature import UnivariateFeatureSelector, VectorAssembler
    from cdnaml.ml.stat import ANOVATest, ChiSquareTest, FValueTest
    from cdnaml.models.util import local_xyw
    from cdnaml.ops import kernels as K
    spark = cdnaml.SparkSession.builder.getOrCreate()
    comm = spark.comm
    Xk, Xc, codes, y = tables()
    names = [f"x{i}" for i in range(D)]

    def frame(X):
        pdf = pd.DataFrame(X, columns=names)
        pdf["label"], pdf["y"] = codes.astype(np.float64), y
        pdf["keep"] = (np.arange(N) < KEPT).astype(np.float64)
        return VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf)) \
            .filter("keep > 0")

    dk, dc = frame(Xk), frame(Xc)
    X, lab, _ = local_xyw(dk, "features", "label", keep_f64=True)
    res = {"world": comm.world_size, "rows": comm.all_gather_object(int(X.shape[0]))}
    table = K.label_stats(X, lab.int(), K.LABEL_COUNT, C=CC, K=KC)["table"].double()
    comm.all_reduce(table)
    res["table"] = table.long().reshape(-1).tolist()

    def row(df):
        r = df.head()
        return [list(map(float, r[0].toArray())), [int(v) for v in r[1]], list(map(float, r[2].toArray()))]

    res["chi2"] = row(ChiSquareTest.test(dk, "features", "label"))
    res["anova"] = row(ANOVATest.test(dc, "features", "label"))
    res["fvalue"] = row(FValueTest.test(dc, "features", "y"))
    sel = {}
    for name, df, ft, lt, lc in [("chi2", dk, "categorical", "categorical", "label"),
                                 ("anova", dc, "continuous", "categorical", "label"),
                                 ("fvalue", dc, "continuous", "continuous", "y")]:
        m = UnivariateFeatureSelector(outputCol="sel", labelCol=lc).setFeatureType(ft).setLabelType(lt) \
            .setSelectionThreshold(3).fit(df)
        sel[name] = m.selectedFeatures
        assert int(m.transform(df).count()) == KEPT
    res["selected"] = sel
    if int(os.environ.get("RANK", "0")) == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    # orderly teardown (barrier, then destroy the group), as tests/dist_worker.py
    spark.comm.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])
