"""K31 linear_step microbenchmark: one evaluation of a logistic model on the fused fp64-MFMA kernel beside the code
it replaces and the neighbouring one-pass kernels.

python bench/linear_micro.py --rows 1e7 --features 100
Times, on fp32 standard-normal rows with labels drawn from a softmax model, in one job:
  * K.linear_step on the native path (linear_step_kernel + linear_reduce_kernel) in STEP and PREDICT mode at K = 1
    (the binomial top), 3, 16 and 32 margins;
  * K.logistic_grad (K11) on the same tensors as the K = 1 STEP;
  * the multinomial evaluation LogisticRegression ran before K31, at C = 3, in both its forms: fp64 through chunked
    copies of X (what it took below MULTINOMIAL_F64_MAX) and the fp32 GEMMs (above);
  * K.mlp_step with layers [d, 3] (K24: the same objective on the fp32 MFMA) and K.aft_step (K26: the fp64 one-pass
    kernel without a matrix instruction, the HBM yardstick), both in STEP mode.
The variants run interleaved: every round times each of them once (``--reps`` calls after the warm-up round; the
slow torch forms one call), so drift and neighbours on the machine hit all alike.  Every figure is the median ms per
call over the rounds with the spread (min .. max), and the effective read rate n d 4 bytes / median.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdnaml.ops import kernels as K  # noqa: E402


def old_multinomial(X, Yoh, W, b, wv, f64, chunk=1 << 20):
    """The torch evaluation of LogisticRegression._fit's multinomial branch: (gradient [C d + C], loss)."""
    Wt = W.double() if f64 else W.float()
    if f64:
        logits = torch.empty((X.shape[0], W.shape[0]), dtype=torch.float64, device=X.device)
        for r0 in range(0, X.shape[0], chunk):
            logits[r0:r0 + chunk] = X[r0:r0 + chunk].double() @ Wt.T
    else:
        logits = (X @ Wt.T).double()
    logits = logits + b
    ll = (torch.logsumexp(logits, 1) - (logits * Yoh).sum(1)) * wv
    R = (torch.softmax(logits, 1) - Yoh) * wv[:, None]
    gW = (R.T @ X.double()) if f64 else (R.float().T @ X).double()
    return torch.cat([gW.reshape(-1), R.sum(0)]), ll.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, d = int(a.rows), a.features
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    Ws = {k: rng.normal(0.0, d ** -0.5, (k, d)) for k in (1, 3, 16, 32)}
    bs = {k: rng.normal(0.0, 0.3, k) for k in Ws}
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    ys = {k: torch.empty(n, dtype=torch.float64, device=dev) for k in Ws}
    for i0 in range(0, n, 1 << 20):
        m = min(1 << 20, n - i0)
        X[i0:i0 + m] = torch.randn((m, d), generator=g, device=dev)
        for k in Ws:
            z = X[i0:i0 + m].double() @ torch.tensor(Ws[k].T, device=dev)
            z = torch.cat([torch.zeros_like(z), z], 1) if k == 1 else z
            u = torch.rand(z.shape, generator=g, device=dev, dtype=torch.float64).clamp_min(1e-300)
            ys[k][i0:i0 + m] = (z - torch.log(-torch.log(u))).argmax(1).double()
    wv = torch.rand(n, generator=g, device=dev, dtype=torch.float64) + 0.5
    gb = n * d * 4 / 1e9
    print(f"linear_step micro: {n} x {d} fp32 ({gb:.2f} GB), weighted rows", flush=True)
    variants = []
    for k in Ws:
        plan = K.linear_plan(X, k)
        print(f"  plan K={k}: {plan}", flush=True)
        if plan["path"] != "native":
            raise SystemExit("the shape is outside the native range")
        W, b, bi = (Ws[k][0] if k == 1 else Ws[k]), bs[k], k == 1
        variants.append((f"linear_step STEP K={k} (K31)", a.reps,
                         lambda W=W, b=b, bi=bi, k=k: K.linear_step(X, ys[k], W, b, wv, binomial=bi)))
        variants.append((f"linear_step PREDICT K={k} (K31)", a.reps,
                         lambda W=W, b=b, bi=bi: K.linear_step(X, None, W, b, mode=K.LINEAR_PREDICT, binomial=bi)))
    w1 = torch.tensor(Ws[1][0], device=dev)
    variants.append(("logistic_grad (K11)", a.reps, lambda: K.logistic_grad(X, ys[1], w1, float(bs[1][0]), wv)))
    Yoh = torch.nn.functional.one_hot(ys[3].long(), 3).double()
    W3, b3 = torch.tensor(Ws[3], device=dev), torch.tensor(bs[3], device=dev)
    variants.append(("multinomial C=3, torch fp64 (before K31)", 1, lambda: old_multinomial(X, Yoh, W3, b3, wv, True)))
    variants.append(("multinomial C=3, torch fp32 GEMMs (before K31)", 1,
                     lambda: old_multinomial(X, Yoh, W3, b3, wv, False)))
    layers = [d, 3]
    theta = np.concatenate([Ws[3].reshape(-1), bs[3]])
    prep = K.MlpPrepared(theta, layers)
    variants.append(("mlp_step STEP [d, 3] (K24)", a.reps,
                     lambda: K.mlp_step(X, ys[3], theta, layers, K.MLP_STEP, prepared=prep)))
    logt = wv.log()
    variants.append(("aft_step STEP (K26)", a.reps, lambda: K.aft_step(X, logt, ys[1], Ws[1][0], 1.2, -0.2)))

    times = {name: [] for name, _, _ in variants}
    for rnd in range(a.rounds + 1):          # round 0 warms every variant up
        for name, reps, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps if rnd else 1):
                fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) / reps * 1e3)
    for name, _, _ in variants:
        t = np.array(times[name])
        med = float(np.median(t))
        print(f"  {name:48s} {med:10.3f} ms  ({t.min():.3f} .. {t.max():.3f})   {gb / med:7.3f} TB/s", flush=True)
    # the two paths compute the same thing
    for k in (1, 3):
        bi = k == 1
        nat = K.linear_step(X, ys[k], Ws[k][0] if bi else Ws[k], bs[k], wv, binomial=bi)
        if bi:
            g11, l11 = K.logistic_grad(X, ys[1], w1, float(bs[1][0]), wv)
            other, tag = (l11, g11), "K11"
        else:
            g_old, l_old = old_multinomial(X, Yoh, W3, b3, wv, True)
            other, tag = (l_old, g_old), "torch fp64"
        print(f"  K={k}: max |g K31 - g {tag}| / max |g| = "
              f"{float((nat[1] - other[1]).abs().max() / other[1].abs().max()):.2e}   loss {float(nat[0]):.12e} / "
              f"{float(other[0]):.12e}   bad {float(nat[3]):.0f}", flush=True)


if __name__ == "__main__":
    main()
