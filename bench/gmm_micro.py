"""K23 gmm_step microbenchmark: one EM pass on the fused kernels beside the op's host formulation.

python bench/gmm_micro.py --rows 1e7 --features 100 --k 8
Times, on fp32 rows drawn from k overlapping Gaussians:
  * K.gmm_step on the native path (gmm_resp_kernel + gmm_moment_kernel + gmm_reduce_kernel) in STEP, PREDICT and
    EVAL mode;
  * the host formulation of the same op on the same device (torch matmuls and elementwise fp64 passes over
    [rows, d] intermediates, K.GMM_HOST_CHUNK rows at a time), STEP and PREDICT;
  * the arithmetic floor: 2 n k d dc flop for the distances (dc = d rounded up to 32) plus 2 n k 1024 npairs for the
    moments (the upper-triangular 32 x 32 tile pairs of the (d+1) x (d+1) matrix) at 155 TF of the fp32 MFMA.
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


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def make(n, d, k, dev):
    """Rows of k overlapping components (column sd 0.1 .. 0.25, means about one Mahalanobis unit apart) and the
    parameters of the generating mixture, A_j the inverse Cholesky factor."""
    rng = np.random.default_rng(0)
    L0 = (np.eye(d) + 0.3 / np.sqrt(d) * np.tril(rng.standard_normal((d, d)), -1)) * rng.uniform(0.1, 0.25, d)[:, None]
    scale = 1.0 + 0.04 * np.arange(k) / k
    means = 0.5 * rng.standard_normal(d) + (0.7 / np.sqrt(d) * rng.standard_normal((k, d))) @ L0.T
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    Lt = torch.tensor(L0.T, dtype=torch.float32, device=dev)
    mt = torch.tensor(means, dtype=torch.float32, device=dev)
    st = torch.tensor(scale, dtype=torch.float32, device=dev)
    for i0 in range(0, n, 1 << 20):
        m = min(1 << 20, n - i0)
        comp = torch.randint(k, (m,), generator=g, device=dev)
        X[i0:i0 + m] = mt[comp] + (torch.randn((m, d), generator=g, device=dev) @ Lt) * st[comp][:, None]
    A = np.stack([np.linalg.inv(L0 * s) for s in scale])
    logc = np.log(1.0 / k) - 0.5 * (d * np.log(2 * np.pi) + 2 * (np.log(np.abs(np.diag(L0))).sum() + d * np.log(scale)))
    return X, torch.tensor(means), torch.tensor(A), torch.tensor(logc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, d, k = int(a.rows), a.features, a.k
    X, mu, A, logc = make(n, d, k, dev)
    mu, A, logc = mu.to(dev), A.to(dev), logc.to(dev)
    print(f"gmm_step micro: {n} x {d} fp32, k = {k}", flush=True)
    dc, T = -(-d // 32) * 32, -(-(d + 1) // 32)
    floor_e = 2.0 * n * k * d * dc / (MFMA_F32_TF * 1e12) * 1e3
    floor_m = 2.0 * n * k * 1024 * (T * (T + 1) // 2) / (MFMA_F32_TF * 1e12) * 1e3
    ms_s = timed(lambda: K.gmm_step(X, None, mu, A, logc, K.GMM_STEP), a.reps)
    ms_p = timed(lambda: K.gmm_step(X, None, mu, A, logc, K.GMM_PREDICT), a.reps)
    ms_e = timed(lambda: K.gmm_step(X, None, mu, A, logc, K.GMM_EVAL), a.reps)
    print(f"  native STEP (K23)       {ms_s:9.3f} ms   floor {floor_e:.2f} + {floor_m:.2f} ms  "
          f"({(floor_e + floor_m) / ms_s:5.1%} of the fp32 MFMA)", flush=True)
    print(f"  native PREDICT          {ms_p:9.3f} ms   floor {floor_e:.2f} ms", flush=True)
    print(f"  native EVAL             {ms_e:9.3f} ms   -> moments + reduction {ms_s - ms_e:9.3f} ms", flush=True)
    hs = timed(lambda: K.gmm_step(X, None, mu, A, logc, K.GMM_STEP, native=False), a.host_reps)
    hp = timed(lambda: K.gmm_step(X, None, mu, A, logc, K.GMM_PREDICT, native=False), a.host_reps)
    print(f"  host formulation STEP   {hs:9.3f} ms   native / host = {ms_s / hs:5.3f}", flush=True)
    print(f"  host formulation PREDICT{hp:9.3f} ms   native / host = {ms_p / hp:5.3f}", flush=True)
    S, st = K.gmm_step(X, None, mu, A, logc, K.GMM_STEP)
    Sh, sth = K.gmm_step(X, None, mu, A, logc, K.GMM_STEP, native=False)
    print(f"  max |S native - S host| / max |S| = {float((S - Sh).abs().max() / Sh.abs().max()):.2e}   "
          f"log-likelihood {float(st[0]):.9e} / {float(sth[0]):.9e}", flush=True)


if __name__ == "__main__":
    main()
