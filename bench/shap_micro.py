"""K21 tree_shap microbenchmark: TreeSHAP contributions beside the predict kernel on the same rows.

python bench/shap_micro.py --rows 1e6 --features 100
Times K.tree_shap for the headline forest (20 trees, depth 5, raw fp32 rows) and a boosted one (100 trees, depth
8, uint8 bins), with the phi tile in LDS and in the global tile (A/B), and prints the fp64 operation count of the
path loops and the fraction of the fp64 vector rate it amounts to.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdnaml.models.tree.forest import Forest  # noqa: E402
from cdnaml.ops import kernels as K  # noqa: E402

# MI355X fp64 vector peak 78.6 TFLOP/s counts an FMA as two; the path loops run uncontracted (one operation per
# instruction, for bit-reproducible sums), so their ceiling is half of it
FP64_OPS_PER_S = 78.6e12 / 2


def complete_forest(T, depth, d, bins=0, seed=0):
    """T complete trees of ``depth`` on random features; covers split by random fractions in [0.1, 0.9]."""
    rng = np.random.default_rng(seed)
    f = Forest(1)
    for _ in range(T):
        level = [f.add([0.0], 1e6, 0)]
        f.roots.append(level[0])
        for dep in range(depth):
            nxt = []
            for i in level:
                frac = rng.uniform(0.1, 0.9)
                lt = f.add([0.0], f.weight[i] * frac, dep + 1)
                rt = f.add([0.0], f.weight[i] * (1 - frac), dep + 1)
                f.feat[i], f.left[i], f.right[i] = int(rng.integers(0, d)), lt, rt
                f.thr[i] = float(np.float32(rng.normal()))
                f.bin[i] = int(rng.integers(0, max(bins - 1, 1)))
                nxt += [lt, rt]
            level = nxt
        for i in level:
            f.value[i] = np.array([rng.normal()])
    return f


def path_ops(sp) -> float:
    """fp64 operations of the extend and unwind loops per row (shap.hip, the fixed form: constant coefficients):
    5 per extend step (m (m + 1) / 2 steps), 7 per unwind step (m^2 steps), 5 per slot for the contribution."""
    m = sp["hdr"][:, 3].astype(np.float64)
    return float((2.5 * m * (m + 1) + 7 * m * m + 5 * m).sum())


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e6)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grid-lds", type=int, default=K.SHAP_GRID_LDS, help="blocks of the LDS arrangement")
    ap.add_argument("--grid-global", type=int, default=K.SHAP_GRID_GLOBAL, help="blocks of the global arrangement")
    ap.add_argument("--modes", default="lds,global", help="phi arrangements to time")
    a = ap.parse_args()
    K.SHAP_GRID_LDS, K.SHAP_GRID_GLOBAL = a.grid_lds, a.grid_global
    dev = torch.device("cuda")
    n, d = int(a.rows), a.features
    X = torch.randn((n, d), device=dev)
    B = 32
    bins = torch.randint(0, B, ((d + 7) // 8, n, 8), dtype=torch.uint8, device=dev)
    for name, T, depth, binned in (("headline rf", 20, 5, False), ("boosted", 100, 8, True)):
        f = complete_forest(T, depth, d, bins=B if binned else 0)
        tw = np.full(T, 1.0 / T)
        sp = f.shap_paths(binned)
        ops = path_ops(sp) * n
        if binned:
            trees = [f.binned_arrays(dev, t) for t in range(T)]
            F = torch.zeros(n, dtype=torch.float32, device=dev)

            def predict():
                for nodes, vals, masks in trees:
                    K.predict_binned_add(bins, nodes, 0, vals, masks, 0.1, F)
            src = bins
        else:
            def predict():
                f.predict(X, tw, [0.0])
            src = X
        ms_p = timed(predict, a.reps)
        print(f"{name}: T={T} depth={depth} paths={sp['hdr'].shape[0]} max_slots={sp['max_slots']} "
              f"{'bins' if binned else 'fp32 rows'} {n} x {d}", flush=True)
        print(f"  predict               {ms_p:9.2f} ms", flush=True)
        for mode in a.modes.split(","):
            ms = timed(lambda: f.shap_values(src, tw, [0.0], binned=binned, d=d, phi=mode), a.reps)
            print(f"  tree_shap phi={mode:6s}  {ms:9.2f} ms  {ms / ms_p:7.1f} x predict  {ops:.3e} fp64 ops  "
                  f"{ops / ms / 1e9:6.2f} Tops/s = {100 * ops / (ms * 1e-3) / FP64_OPS_PER_S:5.1f} % of the "
                  f"uncontracted fp64 vector rate", flush=True)


if __name__ == "__main__":
    main()
