"""K35 als_topk microbenchmark: the fused score-and-select kernel beside the formulation ALSModel._recommend used
before K35 (the full score matrix ``S @ D.T``, then ``torch.topk``) on the same device tensors.

python bench/topk_micro.py --shapes 131072x32768x12,131072x32768x64,131072x32768x128,256x1048576x64 \
    --big 1000000x100000x12 --k 10
Per shape ns x nd x r, in one job and in interleaved rounds (every contender runs once per round, ``--inner`` calls
between two device synchronisations, so drift of the shared machine hits both alike): ms per call as the median over
the rounds with the rounds' minimum and maximum, the ratio of the medians, and for K35 the achieved rate of
2 ns nd r flops and its share of ``--peak`` (the fp32 MFMA rate, TFLOP/s).  The first round is a warm-up and is not
counted.  ``--big`` shapes run K35 alone: their score matrix is what the formulation before K35 cannot hold.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdnaml.ops import kernels as K  # noqa: E402


def shapes(text):
    return [tuple(int(float(v)) for v in s.split("x")) for s in text.split(",") if s]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="131072x32768x12,131072x32768x64,131072x32768x128,256x1048576x64")
    ap.add_argument("--big", default="1000000x100000x12")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--peak", type=float, default=157.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_micro needs a GPU: a CPU run gives no timing")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    for (ns, nd, r), with_parent in [(s, True) for s in shapes(a.shapes)] + [(s, False) for s in shapes(a.big)]:
        S = torch.randn((ns, r), generator=g, device=dev)
        D = torch.randn((nd, r), generator=g, device=dev)
        plan = K.als_topk_plan(S, D, a.k)
        print(f"als_topk micro: {ns} x {nd}, r = {r}, k = {a.k}, plan {plan}", flush=True)
        if plan["path"] != "native":
            raise SystemExit("the shape is outside the native range")
        runs = {"als_topk (K35)": lambda: K.als_topk(S, D, a.k)}
        if with_parent:
            runs["before K35: S @ D.T, torch.topk"] = lambda: torch.topk(S @ D.T, min(a.k, nd), dim=1)
        times = {name: [] for name in runs}
        for _ in range(a.rounds + 1):
            for name, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.inner * 1e3)
        med = {}
        for name, ts in times.items():
            ts = np.array(ts[1:])                          # the first round warmed up
            med[name] = float(np.median(ts))
            print(f"  {name:34s} {med[name]:10.3f} ms  [{ts.min():10.3f} .. {ts.max():10.3f}] over {len(ts)} rounds",
                  flush=True)
        tf = 2.0 * ns * nd * r / (med["als_topk (K35)"] * 1e-3) / 1e12
        print(f"  K35: {tf:.2f} TFLOP/s, {100 * tf / a.peak:.1f} % of {a.peak} (whole call: both kernels and the "
              f"launches)", flush=True)
        if with_parent:
            print(f"  ratio before / K35 = {med['before K35: S @ D.T, torch.topk'] / med['als_topk (K35)']:.2f}",
                  flush=True)
            # the results agree: values to fp32 rounding of a dot product, positions except at near-ties
            val, idx = K.als_topk(S, D, a.k)
            top = torch.topk(S @ D.T, min(a.k, nd), dim=1)
            err = float(((val - top.values).abs() / top.values.abs().clamp_min(1.0)).max())
            print(f"  max |val - val before| / max(1, |val|) = {err:.2e}   positions that differ "
                  f"{int((idx.long() != top.indices).sum())} of {idx.numel()}", flush=True)
            del top
        del S, D


if __name__ == "__main__":
    main()
