"""K30 cluster_step microbenchmark: one k-means step on the fused kernel beside K10 kmeans_step (the route of every
fit before K30), the op's host formulation and K26's STEP as the HBM yardstick of the same job.

python bench/cluster_micro.py --rows 1e7 --features 100
On fp32 standard-normal rows, for k = 8 and k = 64 (the centres are rows of X): every variant is called once per
round, the rounds interleave all variants, and each is reported as the median of --rounds (11) calls with its spread
(min .. max) and the fraction of the HBM floor it reaches: n d 4 bytes over the rate K26's STEP reads the same rows
at.  The host formulation is called once per k, outside the rounds.  Each time is a host clock around one call that
ends in a device synchronise, so it includes the call's table preparation and upload.
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
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 64])
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
    variants = {"K26 aft_step STEP (HBM yardstick)":
                lambda: K.aft_step(X, logt, censor, coef, 1.0, -0.3, K.AFT_STEP)}
    host = {}
    for k in a.ks:
        C = X[:k].double().cpu().numpy()
        Cd = X[:k].clone()
        shift = C.mean(0).astype(np.float32)
        print(f"cluster_step micro: {n} x {d} fp32 ({gb:.2f} GB), k = {k}, STEP plan "
              f"{K.cluster_plan(X, k, K.CLUSTER_STEP)}, PREDICT plan {K.cluster_plan(X, k, K.CLUSTER_PREDICT)}",
              flush=True)
        if K.cluster_plan(X, k)["path"] != "native":
            raise SystemExit("the shape is outside the native range")
        for mode, mname in ((K.CLUSTER_STEP, "STEP"), (K.CLUSTER_PREDICT, "PREDICT")):
            for cosine in (False, True):
                for ww in (None, w):
                    name = f"k={k:3d} K30 {mname:7s} {'cosine   ' if cosine else 'euclidean'} " \
                           f"{'weighted' if ww is not None else 'unweighted'}"
                    variants[name] = (lambda mode=mode, cosine=cosine, ww=ww, C=C, shift=shift:
                                      K.cluster_step(X, C, mode, ww, cosine, shift))
            variants[f"k={k:3d} K10 kmeans_step {'with sums' if mode == K.CLUSTER_STEP else 'assign only'}"] = \
                (lambda mode=mode, Cd=Cd: K.kmeans_step(X, Cd, with_sums=mode == K.CLUSTER_STEP))
        host[k] = lambda C=C, shift=shift: K.cluster_step(X, C, K.CLUSTER_STEP, w, False, shift, native=False)
    for fn in variants.values():     # warm up every shape
        fn()
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            times[name].append(once(fn))
    floor = float(np.median(times["K26 aft_step STEP (HBM yardstick)"]))   # n d 4 bytes at K26's rate
    for name, ts in times.items():
        med = float(np.median(ts))
        print(f"  {name:52s} median {med:9.3f} ms  spread {min(ts):9.3f} .. {max(ts):9.3f}  {gb / med:6.3f} TB/s  "
              f"HBM floor / time {floor / med:6.1%}", flush=True)
    for k, fn in host.items():
        print(f"  k={k:3d} host formulation, STEP euclidean weighted (one call) {once(fn):12.3f} ms", flush=True)
    # the two routes agree: the assignment on every row, the sums to fp32 rounding
    for k in a.ks:
        C = X[:k].double().cpu().numpy()
        a30, s30, n30, c30, _ = K.cluster_step(X, C, K.CLUSTER_STEP, None, False, C.mean(0).astype(np.float32))
        a10, s10, n10, c10 = K.kmeans_step(X, X[:k].clone())
        print(f"  k={k:3d} K30 against K10: rows assigned differently {int((a30 != a10).sum())}, max |sums K30 - K10| / "
              f"max |sums| {float((s30 - s10).abs().max() / s10.abs().max()):.2e}, cost {float(c30):.9e} / "
              f"{float(c10):.9e}", flush=True)


if __name__ == "__main__":
    main()
