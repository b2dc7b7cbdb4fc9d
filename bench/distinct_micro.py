"""K29 col_distinct / col_recode microbenchmark: VectorIndexer's fit and transform passes beside K28's FIRST pass and
the host formulation.

python bench/distinct_micro.py --rows 1e7 --features 100
Times, on fp32 rows in one job, in interleaved rounds (round i runs every entry once, so a drift of the machine moves
all of them alike):
  (a) K.col_distinct on a matrix of --features - --codes Gaussian columns and --codes code columns (the Gaussian columns
      overflow within a handful of rows per block and then only count NaNs);
  (a0) K.col_distinct with every column Gaussian: no wave holds a code column, every thread exits early;
  (b) K.col_distinct with every column holding codes (--categories values, cap = --cap): no early exit ever happens;
  (c) K.col_recode of (b)'s matrix by (b)'s tables (every value is searched and every row written);
  (d) K28's FIRST pass (col_digit_hist) on (a)'s matrix: the known row-streaming yardstick.
(e) the host formulation of col_distinct on the same device (torch.unique of every column) is timed after the rounds,
--host-reps times.  Every figure is the median over --reps rounds of the time of one call (a host clock around a call
that ends in a device synchronise), after one warm-up round, with the spread (min .. max) and the effective read rate
n d 4 bytes / time (col_recode also writes as much).  The last lines compare the native and the host results' bits.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdnaml.ops import kernels as K  # noqa: E402


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def same(a, b):
    """two results of col_distinct hold the same values (a NaN slot equals a NaN slot)"""
    return all(torch.equal(a[k].double().nan_to_num(nan=-7.0), b[k].double().nan_to_num(nan=-7.0)) for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--codes", type=int, default=10)
    ap.add_argument("--categories", type=int, default=16)
    ap.add_argument("--cap", type=int, default=20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-reps", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, d, cap = int(a.rows), a.features, a.cap
    g = torch.Generator(device=dev).manual_seed(0)
    Xa = torch.empty((n, d), dtype=torch.float32, device=dev)
    Xb = torch.empty((n, d), dtype=torch.float32, device=dev)
    for i0 in range(0, n, 1 << 20):
        m = min(1 << 20, n - i0)
        Xb[i0:i0 + m] = torch.randint(0, a.categories, (m, d), generator=g, device=dev).float()
        Xa[i0:i0 + m] = torch.randn((m, d), generator=g, device=dev)
        Xa[i0:i0 + m, :a.codes] = Xb[i0:i0 + m, :a.codes]
    Xg = Xa.clone()
    Xg[:, :a.codes] = Xa[:, a.codes:2 * a.codes]
    gb = n * d * 4 / 1e9
    plan = K.col_distinct_plan(Xa, cap)
    print(f"col_distinct micro: {n} x {d} fp32 ({gb:.2f} GB), cap {cap}, {a.categories} categories", flush=True)
    print(f"  plan: {plan}", flush=True)
    if plan["path"] != "native":
        raise SystemExit("the shape is outside the native range")
    tables = K.col_distinct(Xb, cap)
    b1 = K.col_quantiles_plan(Xa, 1)["max_bits"][0]
    entries = {
        f"(a) col_distinct, {d - a.codes} Gaussian + {a.codes} code columns": lambda: K.col_distinct(Xa, cap),
        f"(a0) col_distinct, {d} Gaussian columns": lambda: K.col_distinct(Xg, cap),
        f"(b) col_distinct, {d} code columns": lambda: K.col_distinct(Xb, cap),
        "(c) col_recode of (b), keep": lambda: K.col_recode(Xb, tables, "keep"),
        f"(d) col_digit_hist FIRST, {b1} bits (K28)": lambda: K._digit_hist_native(Xa, 1, b1, 32 - b1, None),
    }
    times = {k: [] for k in entries}
    for rep in range(a.reps + 1):          # round 0 warms up
        for name, fn in entries.items():
            t = once(fn)
            if rep:
                times[name].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, v in times.items():
        print(f"  {name:52s} {med[name]:10.3f} ms  ({min(v):.3f} .. {max(v):.3f})  "
              f"{gb / med[name] * 1e3:8.1f} GB/s of X", flush=True)
    ka, k0, kb, _, kd = list(entries)
    print(f"  (b) - (a) = {med[kb] - med[ka]:.3f} ms, (b) / (a) = {med[kb] / med[ka]:.3f}, "
          f"(b) / (d) = {med[kb] / med[kd]:.3f}, (a) / (d) = {med[ka] / med[kd]:.3f}, "
          f"(a0) / (d) = {med[k0] / med[kd]:.3f}", flush=True)
    for label, X in (("(a)", Xa), ("(b)", Xb)):
        host_fn = lambda X=X: K.col_distinct(X, cap, native=False)  # noqa: E731
        once(host_fn)
        hs = [once(host_fn) for _ in range(a.host_reps)]
        print(f"  (e) host formulation of {label} on the device {statistics.median(hs):10.3f} ms  "
              f"({min(hs):.3f} .. {max(hs):.3f})", flush=True)
        print(f"      native == host formulation, bit for bit: {same(K.col_distinct(X, cap), host_fn())}", flush=True)
    Yn, Yh = K.col_recode(Xb, tables, "keep"), K.col_recode(Xb, tables, "keep", native=False)
    print(f"  col_recode native == host formulation: {torch.equal(Yn[0], Yh[0]) and torch.equal(Yn[1], Yh[1])}",
          flush=True)


if __name__ == "__main__":
    main()
