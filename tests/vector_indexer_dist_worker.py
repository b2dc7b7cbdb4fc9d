"""VectorIndexer under SPMD: run under torchrun (gloo, CPU) with the repository root in PYTHONPATH by
tests/test_vector_indexer_cpu.py.  Rank r fits on its own uneven contiguous shard of the same global table; rank 0
writes the fitted model."""
import json
import sys

N, D, CAP = 3000, 11, 5


def main(out_path):
    import cdnaml
    import torch
    from cdnaml.ml.feature import VectorIndexer
    from tests._distinct_refs import reference
    spark = cdnaml.SparkSession.builder.getOrCreate()
    rank, world = spark.comm.rank, spark.comm.world_size
    cut = [0] + [N // 3 * (r + 1) for r in range(world - 1)] + [N]        # rank 0 of two holds a third of the rows
    X = reference(N, D, CAP)[0][cut[rank]:cut[rank + 1]]
    df = spark.createDataFrameFromLocalTensors({"features": torch.tensor(X, device=spark.device)})
    m = VectorIndexer(inputCol="features", outputCol="ix", maxCategories=CAP, handleInvalid="keep").fit(df)
    assert int(m.transform(df).count()) == N
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump({"world": world, "numFeatures": m.numFeatures,
                       "maps": {str(c): sorted(v.items()) for c, v in m.categoryMaps.items()}}, f)
    spark.comm.shutdown()


if __name__ == "__main__":
    main(sys.argv[1])
