"""K34 nb_step microbenchmark: the NaiveBayes sufficient statistics and predictions on the fused kernel beside the
neighbouring row-streaming kernels and the formulation NaiveBayes used before K34.

python bench/nbayes_micro.py --rows 1e7 --features 100 --classes 3,32
Times, on fp32 count rows, per class count, in one job and in interleaved rounds (every contender runs once per round,
``--inner`` calls between two device synchronisations, so drift of the shared machine hits all of them alike):
  * K.nb_step on the native path: STATS without and with QUAD, PREDICT linear and Gaussian;
  * K.label_stats CLASS (K27) and K.linear_step STEP / PREDICT (K31) on the same tensors;
  * the formulation before K34: the weighted one-hot matrix and its two fp32 GEMMs (fit), ``X.double() @ theta^T`` and
    the softmax (linear predict), and the [rows, C, d] fp64 broadcast in chunks of ``--chunk`` rows (Gaussian predict:
    unchunked it is rows x C x d x 8 bytes), the last in ``--slow-rounds`` of the rounds only.
Every figure is the median over the rounds of ms per call, with the rounds' minimum and maximum, and the effective read
rate n d 4 bytes / median.  The first round is a warm-up and is not counted.
"""
import argparse
import math
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
    ap.add_argument("--classes", default="3,32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--slow-rounds", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=1 << 15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nbayes_micro needs a GPU: a CPU run gives no timing")
    dev = torch.device("cuda")
    n, d = int(a.rows), a.features
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    for i0 in range(0, n, 1 << 20):
        m = min(1 << 20, n - i0)
        X[i0:i0 + m] = torch.poisson(torch.full((m, d), 3.0, device=dev), generator=g)
    gb = n * d * 4 / 1e9
    rng = np.random.default_rng(0)
    for C in [int(v) for v in a.classes.split(",")]:
        y = torch.randint(0, C, (n,), generator=g, device=dev).double()
        yi = y.int()
        theta = np.log(rng.dirichlet(np.ones(d), size=C))
        pi = np.log(np.full(C, 1.0 / C))
        mu, sg = 3.0 + rng.normal(scale=0.3, size=(C, d)), rng.uniform(2.0, 4.0, size=(C, d))
        lin = K.NbTables.linear(theta, pi)
        gau = K.NbTables.gaussian(pi, mu, sg, mu.mean(0).astype(np.float32))
        shift = torch.full((d,), 3.0, device=dev)
        plans = {k: K.nb_plan(X, C, m, q) for k, m, q in (("stats", K.NB_STATS, False), ("stats quad", K.NB_STATS, True),
                                                          ("predict", K.NB_PREDICT, False),
                                                          ("predict quad", K.NB_PREDICT, True))}
        print(f"nb_step micro: {n} x {d} fp32 ({gb:.2f} GB), C = {C}, plans {plans}", flush=True)
        if any(p["path"] != "native" for p in plans.values()):
            raise SystemExit("the shape is outside the native range")
        th_t, pi_t = torch.tensor(theta, device=dev), torch.tensor(pi, device=dev)
        mu_t, sg_t = torch.tensor(mu, device=dev), torch.tensor(sg, device=dev)

        def parent_fit():
            """NaiveBayes._fit before K34 (the all-reduce left out)."""
            Yoh = torch.nn.functional.one_hot(y.long(), C).double()
            return Yoh.sum(0), (Yoh.float().T @ X).double(), (Yoh.float().T @ (X * X)).double()

        def parent_linear():
            raw = X.double() @ th_t.T + pi_t
            prob = torch.softmax(raw, 1)
            return raw, prob, torch.argmax(prob, 1)

        def parent_gaussian():
            """The parent's [rows, C, d] broadcast, ``--chunk`` rows at a time."""
            out = []
            for i0 in range(0, n, a.chunk):
                Xc = X[i0:i0 + a.chunk].double()
                raw = -0.5 * (((Xc[:, None, :] - mu_t[None]) ** 2) / sg_t[None] +
                              torch.log(2 * math.pi * sg_t[None])).sum(2) + pi_t
                out.append(torch.softmax(raw, 1))
            return out

        fast = {
            "nb_step STATS (K34)": lambda: K.nb_step(X, y, C, rule=K.NB_NONNEG),
            "nb_step STATS QUAD (K34)": lambda: K.nb_step(X, y, C, quad=True, shift=shift),
            "nb_step PREDICT linear (K34)": lambda: K.nb_step(X, None, C, K.NB_PREDICT, tables=lin),
            "nb_step PREDICT gaussian (K34)": lambda: K.nb_step(X, None, C, K.NB_PREDICT, tables=gau),
            "label_stats CLASS (K27)": lambda: K.label_stats(X, yi, K.LABEL_CLASS, C=C),
            "linear_step STEP (K31)": lambda: K.linear_step(X, y, theta, pi),
            "linear_step PREDICT (K31)": lambda: K.linear_step(X, None, theta, pi, mode=K.LINEAR_PREDICT),
            "before K34: one-hot and two fp32 GEMMs": parent_fit,
            "before K34: X.double() @ theta^T, softmax": parent_linear,
        }
        slow = {"before K34: chunked [rows, C, d] broadcast": parent_gaussian}
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
            if r <= a.slow_rounds:
                for name, fn in slow.items():
                    run(name, fn, 1)
        for name, ts in times.items():
            ts = np.array(ts[1:])                          # the first round warmed up
            med = float(np.median(ts))
            print(f"  C={C:2d} {name:46s} {med:10.3f} ms  [{ts.min():10.3f} .. {ts.max():10.3f}] over {len(ts)} rounds  "
                  f"{gb / med:6.3f} TB/s", flush=True)
        # the results agree
        S, Q, W, bad = K.nb_step(X, y, C, quad=True)
        cnt, Sp, Qp = parent_fit()
        print(f"  C={C:2d} fit: max |S - S parent| / max S = {float((S - Sp).abs().max() / S.abs().max()):.2e}   "
              f"Q: {float((Q - Qp).abs().max() / Q.abs().max()):.2e}   W equal {bool(torch.equal(W, cnt))}   "
              f"bad {bad.tolist()}", flush=True)
        raw, prob, pred, _ = K.nb_step(X, None, C, K.NB_PREDICT, tables=lin)
        rp, pp, ap_ = parent_linear()
        print(f"  C={C:2d} linear predict: max |raw - raw parent| / max |raw| = "
              f"{float((raw - rp).abs().max() / rp.abs().max()):.2e}   prob {float((prob - pp).abs().max()):.2e}   "
              f"pred differ {int((pred.long() != ap_).sum())}", flush=True)
        pg = K.nb_step(X[:1 << 20], None, C, K.NB_PREDICT, tables=gau)[1]
        ph = K.nb_step(X[:1 << 20], None, C, K.NB_PREDICT, tables=gau, native=False)[1]
        print(f"  C={C:2d} gaussian predict, first 2^20 rows: max |prob native - prob host| = "
              f"{float((pg - ph).abs().max()):.2e}", flush=True)
        del y, yi, raw, prob, pred, rp, pp, ap_, S, Q, Sp, Qp


if __name__ == "__main__":
    main()
