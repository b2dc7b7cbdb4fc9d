"""K33 bisect_step microbenchmark: one STEP pass with 1, 8 and 64 split entries and one PREDICT pass down balanced trees
of 16 and 128 leaves, beside K26's STEP as the HBM yardstick of the same job, and optionally a whole fit.

python bench/bisect_micro.py --rows 1e7 --features 100 [--fit]
On fp32 standard-normal rows (the child centres are rows of X, every row stands at a random entry): every variant is
called once per round, the rounds interleave all variants, and each is reported as the median of --rounds (11) calls
with its spread (min .. max), its achieved n d 4 bytes per second and the fraction of the HBM floor it reaches (the time
K26's STEP reads the same rows in).  Each time is a host clock around one call that ends in a device synchronise, so it
includes the call's table preparation and upload.  --fit times BisectingKMeans(k=8, maxIter=20).fit on the same rows.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdnaml.ops import kernels as K  # noqa: E402


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--fit", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, d = int(a.rows), a.features
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    for i0 in range(0, n, 1 << 20):
        m = min(1 << 20, n - i0)
        X[i0:i0 + m] = torch.randn((m, d), generator=g, device=dev)
    w = 0.5 + torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    logt = torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    censor = torch.ones(n, dtype=torch.float64, device=dev)
    coef = np.random.default_rng(0).normal(0.0, d ** -0.5, d)
    gb = n * d * 4 / 1e9
    C = X[:256].double().cpu().numpy()
    shift = np.zeros(d, dtype=np.float32)
    variants = {"K26 aft_step STEP (HBM yardstick)":
                lambda: K.aft_step(X, logt, censor, coef, 1.0, -0.3, K.AFT_STEP)}
    for M in (1, 8, 64):
        cl, cr = C[:M], C[M:2 * M]
        tab = (cr - cl, ((cr ** 2).sum(1) - (cl ** 2).sum(1)) / 2, [-1] * M, [-1] * M)
        node = torch.randint(0, M, (n,), generator=g, device=dev, dtype=torch.int32)
        print(f"STEP {M} entries: {K.bisect_plan(X, M, K.BISECT_STEP)}", flush=True)
        for cosine in (False, True):
            variants[f"K33 STEP    {M:3d} entries {'cosine   ' if cosine else 'euclidean'} weighted"] = \
                (lambda tab=tab, node=node, cosine=cosine: K.bisect_step(X, *tab, K.BISECT_STEP, node, w, cosine, shift))
        variants[f"K33 ASSIGN  {M:3d} entries euclidean"] = \
            (lambda tab=tab, node=node: K.bisect_step(X, *tab, K.BISECT_ASSIGN, node.clone(), None, False, shift))
    for L in (16, 128):
        cl, cr, e = C[:L - 1], C[L - 1:2 * L - 2], np.arange(L - 1)
        kid = lambda c, L=L: np.where(c < L - 1, c, L - 2 - c)   # noqa: E731  heap order, leaves behind the entries
        tab = (cr - cl, ((cr ** 2).sum(1) - (cl ** 2).sum(1)) / 2, kid(2 * e + 1), kid(2 * e + 2))
        print(f"PREDICT {L} leaves: {K.bisect_plan(X, L - 1, K.BISECT_PREDICT, L)}", flush=True)
        variants[f"K33 PREDICT {L:3d} leaves  euclidean"] = \
            (lambda tab=tab, L=L: K.bisect_step(X, *tab, K.BISECT_PREDICT, None, None, False, shift, C[:L]))
    for fn in variants.values():     # warm up every shape
        fn()
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            times[name].append(once(fn))
    floor = float(np.median(times["K26 aft_step STEP (HBM yardstick)"]))
    for name, ts in times.items():
        med = float(np.median(ts))
        print(f"  {name:46s} median {med:9.3f} ms  spread {min(ts):9.3f} .. {max(ts):9.3f}  {gb / med:6.3f} TB/s  "
              f"HBM floor / time {floor / med:6.1%}", flush=True)
    if a.fit:
        import cdnaml
        from cdnaml.ml.clustering import BisectingKMeans
        spark = cdnaml.SparkSession.builder.getOrCreate()
        df = spark.createDataFrameFromLocalTensors({"features": X})
        est = BisectingKMeans(k=8, maxIter=20, seed=1)
        est.fit(df)
        ts = [once(lambda: est.fit(df)) for _ in range(3)]
        print(f"  BisectingKMeans(k=8, maxIter=20).fit: median {float(np.median(ts)):10.1f} ms  spread {min(ts):10.1f} .. "
              f"{max(ts):10.1f}", flush=True)


if __name__ == "__main__":
    main()
