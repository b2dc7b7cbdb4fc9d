"""K28 col_quantiles microbenchmark: the exact radix select behind RobustScaler beside its host formulation, the
per-column sort it replaces and K27's one-pass kernels.

python bench/quantile_micro.py --rows 1e7 --features 100
Times, on fp32 rows in one job, in interleaved rounds (round i runs every entry once, so a drift of the machine moves
all of them alike):
  * K.col_quantiles(X, [0.25, 0.5, 0.75]) on the native path (every pass, select step and the extrema);
  * the yardstick: what the engine had to do before K28 -- torch.sort of each of the d columns (a strided column
    extraction and a sort per column) and the three ranks picked from the sorted column;
  * the FIRST pass and every NEXT pass of the plan (each below the true quantiles' prefixes) alone;
  * K27 label_stats COUNT (category indices below 40, 2 labels) and REGRESS at the same shape.
The host formulation of col_quantiles on the same device (torch ops, K.LABEL_HOST_CHUNK rows at a time) is timed after
the rounds, --host-reps times.  Every figure is the median over --reps rounds of the time of one call (a host clock
around a call that ends in a device synchronise), after one warm-up round, with the spread (min .. max); the single
passes and K27 also get the effective read rate n d 4 bytes / time.  The last lines compare the three results' bits.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdnaml.ops import kernels as K  # noqa: E402

PROBS = [0.25, 0.5, 0.75]


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def as_bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def sort_columns(X, probs):
    """[Q, d]: the quantiles by a sort of each column and the rank rule of K.col_quantiles (no NaN in X)."""
    n, d = X.shape
    ranks = [min(max(int(torch.ceil(torch.tensor(p * n, dtype=torch.float64))), 1), n) - 1 for p in probs]
    idx = torch.tensor(ranks, device=X.device)
    return torch.stack([torch.sort(X[:, c]).values[idx] for c in range(d)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--categories", type=int, default=40)
    ap.add_argument("--labels", type=int, default=2)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, d, Kc, Cl = int(a.rows), a.features, a.categories, a.labels
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    Xk = torch.empty((n, d), dtype=torch.float32, device=dev)
    for i0 in range(0, n, 1 << 20):
        m = min(1 << 20, n - i0)
        X[i0:i0 + m] = torch.randn((m, d), generator=g, device=dev) + 3.0
        Xk[i0:i0 + m] = torch.randint(0, Kc, (m, d), generator=g, device=dev).float()
    lab2 = torch.randint(0, Cl, (n,), generator=g, device=dev, dtype=torch.int32)
    y = torch.randn(n, generator=g, device=dev, dtype=torch.float64) * 2.0 + 5.0
    shift = X[:1024].double().mean(0).cpu().numpy()
    yshift = float(y[:1024].mean())
    gb = n * d * 4 / 1e9
    plan = K.col_quantiles_plan(X, len(PROBS))
    print(f"col_quantiles micro: {n} x {d} fp32 ({gb:.2f} GB), probabilities {PROBS}", flush=True)
    print(f"  plan: {plan}", flush=True)
    if plan["path"] != "native":
        raise SystemExit("the shape is outside the native range")
    w = plan["widths"]
    native = K.col_quantiles(X, PROBS)
    # the targets' prefixes before every NEXT pass: the top bits of the quantiles' keys (as the quantile call holds
    # them: u32 in int32 storage, so the passes are timed without the op's conversion)
    qkeys = K._colq_keys(native["q"].T.contiguous())[0]
    Q = len(PROBS)
    passes, low = {}, 32 - w[0]                     # low: the key bits below the prefix
    for i, b in enumerate(w[1:], 1):
        pre = (qkeys >> low).to(torch.int32)        # at most 31 bits
        low -= b
        passes[f"col_digit_hist NEXT pass {i}, {b} bits, Q = {Q}"] = \
            lambda b=b, low=low, pre=pre: K._digit_hist_native(X, Q, b, low, pre)

    entries = {
        "col_quantiles native (K28)": lambda: K.col_quantiles(X, PROBS),
        f"torch.sort of each of the {d} columns": lambda: sort_columns(X, PROBS),
        f"col_digit_hist FIRST, {w[0]} bits": lambda: K._digit_hist_native(X, Q, w[0], 32 - w[0], None),
        **passes,
        "label_stats COUNT native (K27)": lambda: K.label_stats(Xk, lab2, K.LABEL_COUNT, C=Cl, K=Kc),
        "label_stats REGRESS native (K27)":
            lambda: K.label_stats(X, y, K.LABEL_REGRESS, shift=shift, yshift=yshift),
    }
    times = {k: [] for k in entries}
    for rep in range(a.reps + 1):          # round 0 warms up
        for name, fn in entries.items():
            t = once(fn)
            if rep:
                times[name].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, v in times.items():
        rate = "" if "col_quantiles" in name or "sort" in name else f"  {gb / med[name] * 1e3:8.1f} GB/s of X"
        print(f"  {name:44s} {med[name]:10.3f} ms  ({min(v):.3f} .. {max(v):.3f}){rate}", flush=True)
    nat, srt = "col_quantiles native (K28)", f"torch.sort of each of the {d} columns"
    print(f"  native / per-column sort = {med[nat] / med[srt]:.4f}  (sort's fastest round {min(times[srt]):.3f} ms, "
          f"native's slowest {max(times[nat]):.3f} ms)", flush=True)
    host_fn = lambda: K.col_quantiles(X, PROBS, native=False)  # noqa: E731
    once(host_fn)
    hs = [once(host_fn) for _ in range(a.host_reps)]
    print(f"  col_quantiles host formulation on the device {statistics.median(hs):10.3f} ms  "
          f"({min(hs):.3f} .. {max(hs):.3f})   native / host = {med[nat] / statistics.median(hs):.4f}", flush=True)
    host = host_fn()
    same = all(torch.equal(as_bits(native[k]), as_bits(host[k])) for k in native)
    print(f"  native == host formulation, bit for bit: {same}", flush=True)
    print(f"  native q == sorted columns' values: {torch.equal(native['q'], sort_columns(X, PROBS))}", flush=True)


if __name__ == "__main__":
    main()
