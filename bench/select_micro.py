"""K27 label_stats microbenchmark: the one pass behind ChiSquareTest, ANOVATest and FValueTest on the fused kernel
beside the op's host formulation and K26's STEP, the neighbouring one-pass fp64 kernel.

python bench/select_micro.py --rows 1e7 --features 100
Times, on fp32 rows in one job:
  * K.label_stats on the native path in its three modes: COUNT (category indices below 40, 2 labels), CLASS
    (3 classes) and REGRESS;
  * K.aft_step STEP (K26) at the same shape, interleaved with them: round i runs every native call once, so a drift
    of the machine moves all of them alike;
  * the host formulation of every mode on the same device (fp64 torch ops, K.LABEL_HOST_CHUNK rows at a time), each
    under its own time limit: a mode that passes --host-limit seconds on its first call is reported from that call.
Every native figure is the median over --reps rounds of the time of one call (a host clock around a call that ends
in a device synchronise), after one warm-up round, with the spread (min .. max) and the effective read rate
n d 4 bytes / time.  The last lines compare the native results with the host formulation's.
"""
import argparse
import os
import statistics
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
    ap.add_argument("--categories", type=int, default=40)
    ap.add_argument("--labels", type=int, default=2)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-limit", type=float, default=20.0)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, d, Kc, Cl, Cc = int(a.rows), a.features, a.categories, a.labels, a.classes
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    Xk = torch.empty((n, d), dtype=torch.float32, device=dev)
    for i0 in range(0, n, 1 << 20):
        m = min(1 << 20, n - i0)
        X[i0:i0 + m] = torch.randn((m, d), generator=g, device=dev) + 3.0
        Xk[i0:i0 + m] = torch.randint(0, Kc, (m, d), generator=g, device=dev).float()
    lab2 = torch.randint(0, Cl, (n,), generator=g, device=dev, dtype=torch.int32)
    lab3 = torch.randint(0, Cc, (n,), generator=g, device=dev, dtype=torch.int32)
    y = torch.randn(n, generator=g, device=dev, dtype=torch.float64) * 2.0 + 5.0
    shift = X[:1024].double().mean(0).cpu().numpy()
    yshift = float(y[:1024].mean())
    logt, censor = y * 0.1, (lab2 > 0).double()
    coef = rng.normal(0.0, 0.5 * d ** -0.5, d)
    gb = n * d * 4 / 1e9
    plans = {"COUNT": K.label_stats_plan(Xk, K.LABEL_COUNT, C=Cl, K=Kc),
             "CLASS": K.label_stats_plan(X, K.LABEL_CLASS, C=Cc), "REGRESS": K.label_stats_plan(X, K.LABEL_REGRESS)}
    print(f"label_stats micro: {n} x {d} fp32 ({gb:.2f} GB)", flush=True)
    for name, plan in plans.items():
        print(f"  plan {name}: {plan}", flush=True)
        if plan["path"] != "native":
            raise SystemExit("the shape is outside the native range")

    def calls(native):
        return {"COUNT": lambda: K.label_stats(Xk, lab2, K.LABEL_COUNT, C=Cl, K=Kc, native=native),
                "CLASS": lambda: K.label_stats(X, lab3, K.LABEL_CLASS, C=Cc, shift=shift, native=native),
                "REGRESS": lambda: K.label_stats(X, y, K.LABEL_REGRESS, shift=shift, yshift=yshift, native=native)}

    nat = calls(True)
    nat["aft_step STEP (K26)"] = lambda: K.aft_step(X, logt, censor, coef, 1.2, -0.2)
    times = {k: [] for k in nat}
    for rep in range(a.reps + 1):          # round 0 warms up
        for name, fn in nat.items():
            t = once(fn)
            if rep:
                times[name].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    step = med["aft_step STEP (K26)"]
    for name, v in times.items():
        label = name if name.startswith("aft") else f"label_stats {name} native (K27)"
        print(f"  {label:40s} {med[name]:9.3f} ms  ({min(v):.3f} .. {max(v):.3f})  {gb / med[name]:7.3f} TB/s   "
              f"/ K26 STEP = {med[name] / step:5.2f}", flush=True)
    res_host = {}
    for name, fn in calls(False).items():
        first = once(fn)
        if first > a.host_limit * 1e3:
            hs = first
        else:
            hs = statistics.median([once(fn) for _ in range(a.host_reps)])
        res_host[name] = fn()
        print(f"  label_stats {name} host formulation {hs:12.3f} ms   native / host = {med[name] / hs:6.4f}", flush=True)
    for name, fn in calls(True).items():
        got, want = fn(), res_host[name]
        if name == "COUNT":
            same = all(torch.equal(got[k], want[k]) for k in got)
            print(f"  COUNT native == host formulation: {same}", flush=True)
        else:
            gap = max(float((got[k] - want[k]).abs().max() / want[k].abs().max().clamp_min(1e-300))
                      for k in got if k not in ("bad", "bad_label"))
            print(f"  {name} max |native - host| / max |host| over the outputs = {gap:.2e}", flush=True)


if __name__ == "__main__":
    main()
