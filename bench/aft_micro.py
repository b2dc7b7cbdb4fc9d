"""K26 aft_step microbenchmark: one loss-and-gradient evaluation of AFTSurvivalRegression on the fused kernel beside
the op's host formulation and the neighbouring one-pass kernels.

python bench/aft_micro.py --rows 1e7 --features 100
Times, on fp32 standard-normal rows with Weibull AFT times (sigma 0.7, ~30 % censored), in one job:
  * K.aft_step on the native path (aft_step_kernel + aft_reduce_kernel) in STEP mode, and in PREDICT mode without
    and with Spark's 9 default quantiles;
  * the host formulation of the same op on the same device (fp64 torch ops, K.AFT_HOST_CHUNK rows at a time), each
    under its own time limit: a mode that passes --host-limit seconds on its first call is reported from that call;
  * K.fm_step (factorSize 8, squared loss, STEP) and K.logistic_grad at the same shape;
  * with --fit-iters N > 0, AFTSurvivalRegression.fit with maxIter = N on the same rows, at the default tol and at
    tol = 0 (every iteration runs; past convergence the line search takes many evaluations per iteration).
Every figure is ms per call after one warm-up call, with the effective read rate n d 4 bytes / time.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdnaml.ops import kernels as K  # noqa: E402

PROBS = [0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-limit", type=float, default=20.0)
    ap.add_argument("--fit-iters", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, d = int(a.rows), a.features
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    beta = rng.normal(0.0, 0.5 * d ** -0.5, d)
    beta_d = torch.tensor(beta, device=dev)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    logT = torch.empty(n, dtype=torch.float64, device=dev)
    for i0 in range(0, n, 1 << 20):
        m = min(1 << 20, n - i0)
        X[i0:i0 + m] = torch.randn((m, d), generator=g, device=dev)
        logT[i0:i0 + m] = X[i0:i0 + m].double() @ beta_d
    e = -torch.log1p(-torch.rand(n, generator=g, device=dev, dtype=torch.float64))
    logT += 1.0 + 0.7 * torch.log(e)
    C = -torch.log1p(-torch.rand(n, generator=g, device=dev, dtype=torch.float64)) * (2.5 * np.e)
    T = torch.exp(logT)
    t = torch.minimum(T, C)
    censor = (T <= C).double()
    logt = torch.log(t)
    y01 = censor
    del e, C, T, logT
    coef = beta + rng.normal(0.0, 0.3 * d ** -0.5, d)
    b0, ls = 1.2, float(np.log(0.7)) + 0.15
    gb = n * d * 4 / 1e9
    plan = K.aft_plan(X)
    print(f"aft_step micro: {n} x {d} fp32 ({gb:.2f} GB), censored {1.0 - float(censor.mean()):.3f}, plan {plan}",
          flush=True)
    if plan["path"] != "native":
        raise SystemExit("the shape is outside the native range")

    def report(name, ms, extra=""):
        print(f"  {name:44s} {ms:10.3f} ms   {gb / ms:7.3f} TB/s{extra}", flush=True)

    call = lambda mode, probs, native: K.aft_step(X, logt, censor, coef, b0, ls, mode, probs,  # noqa: E731
                                                  native=native)
    res = {}
    for name, mode, probs in (("STEP", K.AFT_STEP, None), ("PREDICT", K.AFT_PREDICT, None),
                              ("PREDICT + 9 quantiles", K.AFT_PREDICT, PROBS)):
        res[name] = timed(lambda: call(mode, probs, True), a.reps)
        report(f"aft_step {name} native (K26)", res[name])
    for name, mode, probs in (("STEP", K.AFT_STEP, None), ("PREDICT", K.AFT_PREDICT, None),
                              ("PREDICT + 9 quantiles", K.AFT_PREDICT, PROBS)):
        hs = timed(lambda: call(mode, probs, False), a.host_reps, a.host_limit)
        report(f"aft_step {name} host formulation", hs, f"   native / host = {res[name] / hs:6.4f}")
    k = 8
    theta = np.concatenate([rng.normal(0.0, 0.7 / (d * k) ** 0.25, d * k), rng.normal(0.0, d ** -0.5, d), [0.3]])
    prep = K.FmPrepared(theta, d, k)
    fm = timed(lambda: K.fm_step(X, logt, theta, k, K.FM_SQUARED, K.FM_STEP, prepared=prep), a.reps)
    report("fm_step STEP sq, factorSize 8 (K25)", fm, f"   aft STEP / fm STEP = {res['STEP'] / fm:6.4f}")
    w = torch.tensor(coef, device=dev)
    lg = timed(lambda: K.logistic_grad(X, y01, w, b0), a.reps)
    report("logistic_grad (K11)", lg, f"   aft STEP / logistic_grad = {res['STEP'] / lg:6.4f}")
    ln, gn, bn = call(K.AFT_STEP, None, True)
    lh, gh, bh = call(K.AFT_STEP, None, False)
    print(f"  max |g native - g host| / max |g| = {float((gn - gh).abs().max() / gh.abs().max()):.2e}   loss "
          f"{float(ln):.12e} / {float(lh):.12e}   bad {float(bn):.0f} / {float(bh):.0f}", flush=True)
    if a.fit_iters > 0:
        import cdnaml
        from cdnaml.ml.regression import AFTSurvivalRegression
        spark = cdnaml.SparkSession.builder.getOrCreate()
        df = spark.createDataFrameFromLocalTensors({"features": X, "label": t, "censor": censor})
        counts = {"step": 0}
        orig = K.aft_step

        def counting(*args, **kw):
            counts["step"] += 1
            return orig(*args, **kw)
        K.aft_step = counting
        try:
            for tol in (1e-6, 0.0):
                counts["step"] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = AFTSurvivalRegression(maxIter=a.fit_iters, tol=tol).fit(df)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(f"  AFTSurvivalRegression.fit maxIter={a.fit_iters} tol={tol:g}: {dt * 1e3:.1f} ms, "
                      f"{counts['step']} evaluations ({dt * 1e3 / max(counts['step'], 1):.3f} ms each, the std pass "
                      f"included), scale {m.scale:.4f}, |coef - generating| "
                      f"{np.abs(m.coefficients.toArray() - beta).max():.4f}", flush=True)
        finally:
            K.aft_step = orig


if __name__ == "__main__":
    main()
