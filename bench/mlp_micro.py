"""K24 mlp_step microbenchmark: one objective evaluation on the fused kernel beside the op's host formulation.

python bench/mlp_micro.py --rows 1e7 --features 100
Times, on fp32 standard-normal rows with uniform labels, for the nets [d, 64, 32, 3] and [d, 3]:
  * K.mlp_step on the native path (mlp_step_kernel + mlp_reduce_kernel) in STEP and PREDICT mode;
  * the host formulation of the same op on the same device (fp64 torch matmuls and elementwise passes over
    [rows, width] intermediates, K.MLP_HOST_CHUNK rows at a time), each mode under its own time limit: a mode that
    passes --host-limit seconds on its first call is reported from that one call;
  * the arithmetic floor of the padded net on the fp32 MFMA at 155 TF: per row and layer 2 (in up to 2) (out up to
    32) flop forward, 2 (in up to 32) (out up to 32) for the weight gradient and 2 (out up to 2) (in up to 32) for
    the backward delta of every layer but the first.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdnaml.ops import kernels as K  # noqa: E402

MFMA_F32_TF = 155.0


def timed(fn, reps, limit=None):
    """ms per call: one warm-up call, then ``reps`` timed ones; only the warm-up call's time if it passes ``limit``."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    if limit is not None and first > limit:
        return first * 1e3
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def padded_flop_per_row(layers, step):
    """fp32 MFMA flop per row of the padded net: every product in 32-wide tiles, k rounded up to 2."""
    up = lambda v, m: -(-v // m) * m  # noqa: E731
    f = 0
    for l, (i, o) in enumerate(zip(layers[:-1], layers[1:])):
        f += 2 * up(i, 2) * up(o, 32)                       # forward
        if step:
            f += 2 * up(i, 32) * up(o, 32)                  # weight gradient
            if l > 0:
                f += 2 * up(o, 2) * up(i, 32)               # backward delta
    return f


def theta_for(layers, seed=0):
    rng = np.random.default_rng(seed)
    parts = []
    for i, o in zip(layers[:-1], layers[1:]):
        b = np.sqrt(6.0 / (i + o))
        parts += [rng.uniform(-b, b, o * i), np.zeros(o)]
    return np.concatenate(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-limit", type=float, default=20.0)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, d = int(a.rows), a.features
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    for i0 in range(0, n, 1 << 20):
        m = min(1 << 20, n - i0)
        X[i0:i0 + m] = torch.randn((m, d), generator=g, device=dev)
    y = torch.randint(3, (n,), generator=g, device=dev)
    for layers in ([d, 64, 32, 3], [d, 3]):
        theta = theta_for(layers)
        prep = K.MlpPrepared(theta, layers)
        plan = K.mlp_plan(X, layers)
        print(f"mlp_step micro: {n} x {d} fp32, layers {layers}, plan {plan}", flush=True)
        if plan["path"] != "native":
            raise SystemExit("the shape is outside the native range")
        call = lambda mode, native: K.mlp_step(X, y, theta, layers, mode, native=native, prepared=prep)  # noqa: E731
        for name, mode in (("STEP", K.MLP_STEP), ("PREDICT", K.MLP_PREDICT)):
            floor = n * padded_flop_per_row(layers, mode == K.MLP_STEP) / (MFMA_F32_TF * 1e12) * 1e3
            ms = timed(lambda: call(mode, True), a.reps)
            hs = timed(lambda: call(mode, False), a.host_reps, a.host_limit)
            print(f"  {name:8s} native (K24) {ms:9.3f} ms   padded fp32 MFMA floor {floor:7.3f} ms "
                  f"({floor / ms:5.1%})   host formulation {hs:10.3f} ms   native / host = {ms / hs:6.4f}", flush=True)
        ln, gn = call(K.MLP_STEP, True)
        lh, gh = call(K.MLP_STEP, False)
        print(f"  max |g native - g host| / max |g| = {float((gn - gh).abs().max() / gh.abs().max()):.2e}   "
              f"loss {float(ln):.9e} / {float(lh):.9e}", flush=True)


if __name__ == "__main__":
    main()
