"""K25 fm_step microbenchmark: one training step on the fused kernel beside the op's host formulation.

python bench/fm_micro.py --rows 1e7 --features 100
Times, on fp32 standard-normal rows, for factorSize 8 and 32 (linear weights and intercept on):
  * K.fm_step on the native path (fm_step_kernel + fm_reduce_kernel) in STEP mode with the squared and the logistic
    loss, and in PREDICT mode;
  * the host formulation of the same op on the same device (fp64 torch matmuls and elementwise passes,
    K.FM_HOST_CHUNK rows at a time), each under its own time limit: a mode that passes --host-limit seconds on its
    first call is reported from that one call;
  * the arithmetic floor of the padded products on the fp32 MFMA at 155 TF: per row 2 (d up to 2) (kc up to 32) flop
    for X [V | w] and, in a step, 2 (d up to 32) (kc up to 32) for the gradient X^T (m s | m); kc = factorSize + 1.
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


def padded_flop_per_row(d, k, step):
    up = lambda v, m: -(-v // m) * m  # noqa: E731
    kc = up(k + 1, 32)
    return 2 * up(d, 2) * kc + (2 * up(d, 32) * kc if step else 0)


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
    y = torch.randint(2, (n,), generator=g, device=dev).double()
    for k in (8, 32):
        rng = np.random.default_rng(0)
        theta = np.concatenate([rng.normal(0.0, 0.7 / (d * k) ** 0.25, d * k), rng.normal(0.0, d ** -0.5, d), [0.3]])
        prep = K.FmPrepared(theta, d, k)
        plan = K.fm_plan(X, k)
        print(f"fm_step micro: {n} x {d} fp32, factorSize {k}, plan {plan}", flush=True)
        if plan["path"] != "native":
            raise SystemExit("the shape is outside the native range")
        call = lambda loss, mode, native: K.fm_step(X, y, theta, k, loss, mode, native=native,  # noqa: E731
                                                    prepared=prep)
        for name, loss, mode in (("STEP sq", K.FM_SQUARED, K.FM_STEP), ("STEP log", K.FM_LOGISTIC, K.FM_STEP),
                                 ("PREDICT", K.FM_SQUARED, K.FM_PREDICT)):
            floor = n * padded_flop_per_row(d, k, mode == K.FM_STEP) / (MFMA_F32_TF * 1e12) * 1e3
            ms = timed(lambda: call(loss, mode, True), a.reps)
            hs = timed(lambda: call(loss, mode, False), a.host_reps, a.host_limit)
            print(f"  {name:8s} native (K25) {ms:9.3f} ms   padded fp32 MFMA floor {floor:7.3f} ms "
                  f"({floor / ms:5.1%})   host formulation {hs:10.3f} ms   native / host = {ms / hs:6.4f}", flush=True)
        ms = timed(lambda: K.fm_step(X, y, theta, k, sample=(1, 0, 0.5), prepared=prep), a.reps)
        print(f"  STEP sq, miniBatchFraction 0.5 (drawn in the kernel) {ms:9.3f} ms", flush=True)
        for loss in (K.FM_SQUARED, K.FM_LOGISTIC):
            ln, gn, _ = call(loss, K.FM_STEP, True)
            lh, gh, _ = call(loss, K.FM_STEP, False)
            print(f"  loss {loss}: max |g native - g host| / max |g| = "
                  f"{float((gn - gh).abs().max() / gh.abs().max()):.2e}   loss {float(ln):.9e} / {float(lh):.9e}",
                  flush=True)


if __name__ == "__main__":
    main()
