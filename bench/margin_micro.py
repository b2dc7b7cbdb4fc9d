"""K32 margin_step microbenchmark: one loss-and-gradient evaluation of LinearSVC (squared hinge) and of the Huber
LinearRegression on the fused kernel beside the neighbouring one-margin kernels, the op's host formulation and the
torch evaluation LinearSVC used before K32.

python bench/margin_micro.py --rows 1e7 --features 100
Times, on fp32 standard-normal rows, in one job and in interleaved rounds (every contender runs once per round, ``--inner``
calls between two device synchronisations, so drift of the shared machine hits all of them alike):
  * K.margin_step on the native path (margin_step_kernel + margin_reduce_kernel): STEP with the squared hinge, STEP with
    the Huber top, and PREDICT;
  * K.aft_step STEP (K26) and K.linear_step STEP with one margin (K31, binomial) at the same shape;
  * the torch evaluation of LinearSVC before K32: two fp32 GEMVs and the [n] temporaries between them;
  * the host formulation of margin_step (fp64 torch ops, K.MARGIN_HOST_CHUNK rows at a time), in ``--host-rounds`` of
    the rounds only.
Every figure is the median over the rounds of ms per call, with the rounds' minimum and maximum, and the effective read
rate n d 4 bytes / median.  The first round is a warm-up and is not counted.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdnaml.ops import kernels as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("margin_micro needs a GPU: a CPU run gives no timing")
    dev = torch.device("cuda")
    n, d = int(a.rows), a.features
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    beta = rng.normal(0.0, d ** -0.5, d)
    beta_d = torch.tensor(beta, device=dev)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    lin = torch.empty(n, dtype=torch.float64, device=dev)
    for i0 in range(0, n, 1 << 20):
        m = min(1 << 20, n - i0)
        X[i0:i0 + m] = torch.randn((m, d), generator=g, device=dev)
        lin[i0:i0 + m] = X[i0:i0 + m].double() @ beta_d
    noise = torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    y01 = (lin + 0.5 * noise > 0).double()
    yreg = lin + 0.5 * noise + torch.where(torch.rand(n, generator=g, device=dev) < 0.1, 20.0, 0.0)
    logt = 0.7 * noise + lin               # K26's log t; every row an event
    ones = torch.ones(n, dtype=torch.float64, device=dev)
    del noise, lin
    coef = beta + rng.normal(0.0, 0.3 * d ** -0.5, d)
    b0 = 0.2
    gb = n * d * 4 / 1e9
    plan = K.margin_plan(X)
    print(f"margin_step micro: {n} x {d} fp32 ({gb:.2f} GB), plan {plan}", flush=True)
    if plan["path"] != "native":
        raise SystemExit("the shape is outside the native range")

    ys = 2 * y01 - 1

    def torch_svc():
        """LinearSVC's evaluation before K32 (the all-reduce and the host copy left out)."""
        wt = torch.tensor(coef, dtype=torch.float32, device=dev)
        m = (X @ wt).double() + b0
        marg = 1 - ys * m
        act = marg > 0
        loss = (ones * torch.where(act, marg * marg, torch.zeros_like(marg))).sum()
        r = torch.where(act, -2 * ys * marg, torch.zeros_like(marg)) * ones
        return torch.cat([(r.float() @ X).double(), r.sum().reshape(1), loss.reshape(1)])

    step = lambda y, loss, native: K.margin_step(X, y, coef, b0, loss=loss, sigma=0.7, native=native)  # noqa: E731
    fast = {
        "margin_step STEP squared hinge (K32)": lambda: step(y01, K.MARGIN_SQUARED_HINGE, True),
        "margin_step STEP huber (K32)": lambda: step(yreg, K.MARGIN_HUBER, True),
        "margin_step PREDICT (K32)": lambda: K.margin_step(X, None, coef, b0, mode=K.MARGIN_PREDICT),
        "aft_step STEP (K26)": lambda: K.aft_step(X, logt, ones, coef, b0, float(np.log(0.7))),
        "linear_step STEP, one margin (K31)": lambda: K.linear_step(X, y01, coef, [b0], binomial=True),
        "torch evaluation of LinearSVC before K32": torch_svc,
    }
    slow = {
        "margin_step STEP squared hinge, host formulation": lambda: step(y01, K.MARGIN_SQUARED_HINGE, False),
        "margin_step STEP huber, host formulation": lambda: step(yreg, K.MARGIN_HUBER, False),
    }
    times = {k: [] for k in list(fast) + list(slow)}

    def run(name, fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / calls * 1e3)

    for r in range(a.rounds + 1):
        for name, fn in fast.items():
            run(name, fn, a.inner)
        if r <= a.host_rounds:
            for name, fn in slow.items():
                run(name, fn, 1)
    ref = None
    for name, ts in times.items():
        ts = np.array(ts[1:])                          # the first round warmed up
        med = float(np.median(ts))
        ref = med if ref is None else ref
        print(f"  {name:52s} {med:9.3f} ms  [{ts.min():9.3f} .. {ts.max():9.3f}] over {len(ts)} rounds  "
              f"{gb / med:6.3f} TB/s   / K32 hinge = {med / ref:7.3f}", flush=True)
    for loss, y in ((K.MARGIN_SQUARED_HINGE, y01), (K.MARGIN_HUBER, yreg)):
        ln, gn, wn, bn = step(y, loss, True)
        lh, gh, wh, bh = step(y, loss, False)
        print(f"  loss {loss}: max |g native - g host| / max |g| = {float((gn - gh).abs().max() / gh.abs().max()):.2e}"
              f"   loss {float(ln):.12e} / {float(lh):.12e}   bad {float(bn):.0f} / {float(bh):.0f}", flush=True)
    gt = torch_svc()
    ln, gn, _, _ = step(y01, K.MARGIN_SQUARED_HINGE, True)
    print(f"  torch evaluation against K32: max |g torch - g| / max |g| = "
          f"{float((gt[:d + 1] - gn[:d + 1]).abs().max() / gn.abs().max()):.2e}", flush=True)


if __name__ == "__main__":
    main()
