"""The plain reference of K35 ``als_topk`` (fp64 scores, a stable argsort on (-score, position), the padding rule) and
the cases its CPU and GPU tests share."""
import numpy as np

# (ns, nd, r, k, layout) with integer factors: every fp32 partial sum is exact, so values and positions must equal the
# reference, and with so few distinct scores almost every row ties at its k-th place.  layout "strided": rows of
# stride r + 3 starting one float off alignment (scalar loads); "f4": rows of stride r + 4 (float4 loads).
EXACT = (
    # r: the MFMA k-step of 2 and the column pairs of 4, the float4 width, the instantiations' widths, the range edge
    [(33, 65, r, 10, "plain") for r in (1, 2, 3, 4, 5, 33, 127, 128)]
    # nd: the 32-row destination tile; nd = 1 also pads (k > nd)
    + [(33, nd, 5, 10, "plain") for nd in (1, 31, 32, 33)]
    # the slab split at 512 rows a slab: one slab, two slabs (the merge kernel), three slabs of two source blocks
    + [(33, 512, 12, 10, "plain"), (33, 513, 12, 10, "plain"), (129, 1500, 12, 64, "plain")]
    # ns: a wave's 32 rows, a block's 128, the second block
    + [(ns, 65, 12, 10, "plain") for ns in (1, 31, 32, 128, 129)]
    # k: the range, k = nd, k > nd
    + [(33, 65, 12, 1, "plain"), (33, 65, 12, 64, "plain"), (33, 10, 5, 10, "plain"), (33, 5, 5, 10, "plain")]
    # both load widths on strided rows
    + [(33, 65, 12, 10, "strided"), (33, 65, 12, 10, "f4")])
ROUNDED = [(129, 1000, 12, 10), (33, 4097, 128, 64)]
SLAB_ROWS = 512


def topk(S, D, k):
    """(val fp64 [ns, k], idx int32 [ns, k]): per row of S the k positions of D with the largest fp64 score, (score
    descending, position ascending), NaN scores never, the tail (-inf, -1)."""
    sc = np.asarray(S, np.float64) @ np.asarray(D, np.float64).T
    order = np.argsort(-sc, axis=1, kind="stable")        # NaN sorts last
    valid = (~np.isnan(sc)).sum(1)
    val = np.full((sc.shape[0], k), -np.inf)
    idx = np.full((sc.shape[0], k), -1, dtype=np.int32)
    kk = min(k, sc.shape[1])
    ok = np.arange(kk)[None, :] < valid[:, None]
    val[:, :kk] = np.where(ok, np.take_along_axis(sc, order[:, :kk], 1), -np.inf)
    idx[:, :kk] = np.where(ok, order[:, :kk], -1)
    return val, idx


def integer_factors(ns, nd, r, seed=0):
    g = np.random.default_rng(seed)
    return (g.integers(-3, 4, (ns, r)).astype(np.float32), g.integers(-3, 4, (nd, r)).astype(np.float32))


def check_rounded(S, D, k, val, idx):
    """The criterion by value for fp32 scores: with tol(i, j) = 2 r 2^-24 sum_t |s_it d_jt|, every returned value is
    within tol of the fp64 score of its position, a row's positions are distinct, and no destination left out scores
    more than the row's last returned one plus the two tolerances involved."""
    S, D = np.asarray(S, np.float64), np.asarray(D, np.float64)
    sc, tol = S @ D.T, 2.0 * S.shape[1] * 2.0 ** -24 * (np.abs(S) @ np.abs(D).T)
    assert idx.min() >= 0 and all(len(set(row)) == k for row in idx.tolist())
    got, gtol = np.take_along_axis(sc, idx, 1), np.take_along_axis(tol, idx, 1)
    worst = float((np.abs(val - got) / gtol).max())
    out = np.ones(sc.shape, dtype=bool)
    np.put_along_axis(out, idx, False, 1)
    slack = np.where(out, sc - (got[:, -1:] + gtol[:, -1:] + tol), -np.inf).max()
    print(f"rounded {sc.shape} k={k}: worst |val - score| / tol = {worst:.3f}, worst excess of a left-out score "
          f"{slack:.3e}")
    assert worst <= 1.0 and slack <= 0.0 and (np.diff(val, axis=1) <= 0).all()
