"""K22 glm_step microbenchmark: one fused IRLS step beside the unfused composition of the older ops.

python bench/glm_micro.py --rows 1e7 --features 100
Times, on fp32 rows:
  * K.glm_step (one launch that reads X once) in STEP and EVAL mode;
  * the unfused step: a torch GEMV for eta, elementwise passes for mu / W / z, a sqrt(W)-scaled copy of X with
    sqrt(W) as an extra column, K.gram(fp64=False) on the copy (X read three times, written once);
  * K.gram(fp64=False) alone, the floor of any step that forms the fp32 Gram;
  * a Poisson / log GeneralizedLinearRegression fit held to exactly --iters iterations.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdnaml.ops import kernels as K  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def unfused_step(X, y, beta32, beta0, shift, zshift):
    """A Poisson / log IRLS step from the ops the package had before K22."""
    eta = (X @ beta32).double() + beta0
    mu = torch.exp(eta).clamp_min(K.GLM_EPS)
    W = mu                                      # w / (V g'^2) = mu for poisson / log
    z = eta + (y - mu) / mu
    sw = torch.sqrt(W)
    sw32 = sw.float()[:, None]
    Xw = torch.cat([(X - shift) * sw32, sw32], 1)
    G3 = K.gram(Xw, (sw * (z - zshift)).float(), None, 0.0, fp64=False)
    dev = 2.0 * (torch.xlogy(y, y / mu) - (y - mu)).sum()
    return G3, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, d = int(a.rows), a.features
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand((n, d), generator=g, device=dev) * 2 - 1
    beta = (torch.rand(d, generator=g, device=dev, dtype=torch.float64) * 2 - 1) * 0.5 / d ** 0.5
    y = torch.poisson(torch.exp(0.3 + (X @ beta.float()).double()), generator=g)
    shift = X[:4096].mean(0)
    print(f"glm_step micro: {n} x {d} fp32, poisson / log", flush=True)
    args = (X, y, None, None, beta, 0.3, shift, 0.3, "poisson", "log", 0.0, 0.0)
    ms_f = timed(lambda: K.glm_step(*args, K.GLM_STEP), a.reps)
    ms_e = timed(lambda: K.glm_step(*args, K.GLM_EVAL), a.reps)
    ms_i = timed(lambda: K.glm_step(*args, K.GLM_INIT), a.reps)
    ms_u = timed(lambda: unfused_step(X, y, beta.float(), 0.3, shift, 0.3), a.reps)
    ms_g = timed(lambda: K.gram(X, y.float(), shift, 0.0, fp64=False), a.reps)
    gb = n * d * 4 / 1e9
    print(f"  fused step (K22)        {ms_f:9.3f} ms  {gb / ms_f * 1e3:7.1f} GB/s of X", flush=True)
    print(f"  fused INIT              {ms_i:9.3f} ms", flush=True)
    print(f"  fused EVAL (no Gram)    {ms_e:9.3f} ms  {gb / ms_e * 1e3:7.1f} GB/s of X", flush=True)
    print(f"  unfused composition     {ms_u:9.3f} ms  fused / unfused = {ms_f / ms_u:5.3f}", flush=True)
    print(f"  K.gram(fp64=False)      {ms_g:9.3f} ms  fused / gram    = {ms_f / ms_g:5.3f}", flush=True)
    Gf, _ = K.glm_step(*args, K.GLM_STEP)
    G3, _ = unfused_step(X, y, beta.float(), 0.3, shift, 0.3)
    keep = torch.tensor(list(range(d + 1)) + [d + 2], device=dev)
    Gu = G3[keep][:, keep]
    print(f"  max |G fused - G unfused| / max |G| = {float((Gf - Gu).abs().max() / Gu.abs().max()):.2e}", flush=True)

    import cdnaml
    from cdnaml.ml.regression import GeneralizedLinearRegression
    spark = cdnaml.SparkSession.builder.getOrCreate()
    df = spark.createDataFrameFromLocalTensors({"features": X, "label": y})
    est = GeneralizedLinearRegression(family="poisson", link="log", maxIter=a.iters, tol=0.0)
    est.fit(df)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = est.fit(df)
    torch.cuda.synchronize()
    ms_fit = (time.perf_counter() - t0) * 1e3
    print(f"  poisson fit, {m.summary.numIterations} iterations   {ms_fit:9.2f} ms  "
          f"({ms_fit / (m.summary.numIterations + 2):.2f} ms per pass over X, deviance {m.summary.deviance:.6e})",
          flush=True)
    spark.stop()


if __name__ == "__main__":
    main()
