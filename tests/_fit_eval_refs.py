"""Independent high-precision references for K10 kmeans_step, K11 logistic_grad, K13 reg_metrics and K14 score_hist.

Plain numpy on the CPU, nothing from ``cdnaml.ops.kernels``.  Every reference takes the exact stored input values
(fp32 inputs widen to the wide type without rounding) and works in ``np.longdouble`` (the x87 80-bit format, 64
significand bits, wherever numpy has it; plain fp64 otherwise), then rounds once to fp64: its own error is a few
2^-64 of the sum of absolute terms, three orders of magnitude below the 2^-52 bounds the tests derive for the kernels.
"""
import functools
import math

import numpy as np
import torch

LD = np.longdouble

# shapes shared by the GPU module and the CPU pre-checks: (n, d, k)
KMEANS_SHAPES = [(1, 1, 1), (255, 3, 2), (10000, 4, 5), (524288 + 300, 4, 5)]
KMEANS_LDS_SHAPES = {"float32": (3000, 127, 64), "float64": (3000, 127, 32)}   # (2kd + k) * sizeof(T) = 65280 B
KMEANS_OVER_LDS = (500, 128, 64)                                              # fp32: 65792 B, the host path


LOGISTIC_D = [1, 63, 64, 65, 128, 129, 448, 511, 512]   # both sides of every lane + 64 q slot boundary
LOGISTIC_N_CAP = 4096 * 2 + 5                            # past the grid cap of 1024 blocks x 4 waves, odd tail
# (n, d, weighted) beyond the d sweep at LOGISTIC_N_CAP: fewer rows than waves, the widest d at a long row loop
LOGISTIC_SMALL = [(1, 129, False), (3, 512, False), (4, 65, True), (5, 129, False)]
LOGISTIC_LARGE = (50000, 512)

METRICS_N = [1, 255, 256, 257, 262144 + 257, 1 << 20]
SCORE_N = [1, 300, 262144 + 257, 1 << 20]
SCORE_NB = [1, 2, 1000]


def _np(t, dtype=LD):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t).astype(dtype)


def eps_of(dtype) -> float:
    return float(torch.finfo(dtype).eps)


# ------------------------------------------------------------------------------------------------ inputs
def kmeans_data(n, d, k, dtype, seed=0, clustered=None):
    """X [n, d] and C [k, d] of ``dtype``.  Low d: plain normal rows and centres.  High d: rows scattered around k true
    centres and C those centres slightly moved -- among many centres in many dimensions the distances of a normal row
    concentrate, and a few percent of the rows would sit within rounding of a tie."""
    g = torch.Generator().manual_seed(1000 * seed + n % 9973 + 31 * d + k)
    clustered = d > 16 if clustered is None else clustered
    if not clustered:
        X = torch.randn(n, d, generator=g, dtype=torch.float64)
        C = torch.randn(k, d, generator=g, dtype=torch.float64)
    else:
        C0 = torch.randn(k, d, generator=g, dtype=torch.float64)
        lab = torch.randint(0, k, (n,), generator=g)
        X = C0[lab] + 0.1 * torch.randn(n, d, generator=g, dtype=torch.float64)
        C = C0 + 0.01 * torch.randn(k, d, generator=g, dtype=torch.float64)
    return X.to(dtype), C.to(dtype)


def logistic_data(n, d, dtype, seed=0, weighted=False):
    """X[:, f] = randn * (1 + f/d) (every column has its own scale, so a swapped or dropped feature slot moves the
    gradient), w of alternating sign and ~1/sqrt(d) size (margins of order 1), labels 0/1, optional weights with
    exact zeros."""
    g = torch.Generator().manual_seed(7000 * seed + 13 * n % 10007 + d)
    X = torch.randn(n, d, generator=g, dtype=torch.float64) * (1.0 + torch.arange(d, dtype=torch.float64) / d)
    w = (0.5 + torch.rand(d, generator=g, dtype=torch.float64)) / math.sqrt(d)
    w = w * (1.0 - 2.0 * (torch.arange(d) % 2).double())
    y = (torch.rand(n, generator=g) > 0.5).double()
    wt = None
    if weighted:
        wt = torch.rand(n, generator=g, dtype=torch.float64) * 3.0
        wt[torch.rand(n, generator=g) < 0.1] = 0.0
    return X.to(dtype), y, w, wt


def kmeans_tie_data(dtype, n=3000):
    """Integer rows in [-5, 5]^3 (every distance exact in fp32) and centres with both kinds of tie: C[3] == C[1], and
    C[0], C[2] mirror each other in x0 (equidistant from every row with x0 == 0).  C[4] is far from everything."""
    g = torch.Generator().manual_seed(11)
    X = torch.randint(-5, 6, (n, 3), generator=g).to(dtype)
    C = torch.tensor([[1, 0, 0], [4, 4, 4], [-1, 0, 0], [4, 4, 4], [100, 100, 100]]).to(dtype)
    return X, C


def logistic_exact_data(n, d, dtype):
    """Integer X in [-8, 8], labels 0/1, weights in {0, 1/4, ..., 2}: at w = 0, b = 0 every term wt (1/2 - y) x is a
    multiple of 1/8 far below 2^53 / 8, so the gradient is exact in any summation order."""
    g = torch.Generator().manual_seed(17)
    X = torch.randint(-8, 9, (n, d), generator=g).to(dtype)
    y = (torch.rand(n, generator=g) > 0.5).double()
    wt = torch.randint(0, 9, (n,), generator=g).double() / 4
    return X, y, wt


def logistic_margin_data(dtype, d=65):
    """200 ordinary rows, then for every margin M in +-800, +-40, +-25 and y in {0, 1} one row scaled so that
    x . w + b ~ M.  Returns (X, y, w, b, mask of the rows whose residual sigmoid(m) - y is exactly 0 in fp64:
    M = -800 with y = 0 and M = +800 with y = 1)."""
    b = 0.3
    X, y, w, _ = logistic_data(200, d, torch.float64, seed=3)
    g = torch.Generator().manual_seed(23)
    rows, ys, big = [], [], []
    for M in (800.0, -800.0, 40.0, -40.0, 25.0, -25.0):
        for yy in (0.0, 1.0):
            u = torch.randn(d, generator=g, dtype=torch.float64)
            rows.append(u * ((M - b) / float(u @ w)))
            ys.append(yy)
            big.append((M == -800.0 and yy == 0.0) or (M == 800.0 and yy == 1.0))
    X = torch.cat([X, torch.stack(rows)]).to(dtype)
    y = torch.cat([y, torch.tensor(ys, dtype=torch.float64)])
    mask = torch.cat([torch.zeros(200, dtype=torch.bool), torch.tensor(big)])
    return X, y, w, b, mask


def metrics_data(n, weighted, seed=0, offset=0.0):
    g = torch.Generator().manual_seed(100 * seed + n % 7919)
    y = offset + torch.randn(n, generator=g, dtype=torch.float64)
    p = y + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    w = None
    if weighted:
        w = torch.rand(n, generator=g, dtype=torch.float64) * 2.5 + 0.01
        w[torch.rand(n, generator=g) < 0.1] = 0.0
    return y, p, w


def score_data(n, lo, hi, seed=0):
    """Scores over and beyond [lo, hi] with exact lo / hi values planted, labels from {0.5, 1, 2, 0, -1}."""
    g = torch.Generator().manual_seed(50 * seed + n % 7919)
    span = (hi - lo) if hi > lo else 1.0
    s = lo + span * (torch.rand(n, generator=g, dtype=torch.float64) * 1.2 - 0.1)   # ~8 % below lo, ~8 % above hi
    idx = torch.arange(n)
    s[idx % 11 == 0] = lo
    s[idx % 13 == 1] = hi
    vals = torch.tensor([0.5, 1.0, 2.0, 0.0, -1.0], dtype=torch.float64)
    lab = vals[torch.randint(0, 5, (n,), generator=g)]
    return s, lab


# ------------------------------------------------------------------------------------------------ K10
def ref_kmeans(X, C) -> np.ndarray:
    """Squared distances d2 [n, k] (fp64, computed wide from the stored values)."""
    Xl, Cl = _np(X), _np(C)
    n, k = Xl.shape[0], Cl.shape[0]
    d2 = np.empty((n, k), dtype=np.float64)
    for c in range(k):
        df = Xl - Cl[c][None, :]
        d2[:, c] = (df * df).sum(axis=1).astype(np.float64)
    return d2


def kmeans_gap_rows(d2: np.ndarray, rel: float) -> np.ndarray:
    """Mask of the rows whose best-to-second-best relative gap exceeds ``rel`` (k = 1: every row)."""
    if d2.shape[1] == 1:
        return np.ones(d2.shape[0], dtype=bool)
    part = np.partition(d2, 1, axis=1)
    best, second = part[:, 0], part[:, 1]
    return (second - best) > rel * best


def kmeans_grid(n: int):
    """(nblk, rows_per_block) of the K10 launch: 256-thread blocks, at most 2048 of them."""
    nblk = min(max((n + 255) // 256, 1), 2048)
    return nblk, -(-n // nblk)


def check_kmeans(X, C, out, d2, with_sums=True):
    """Every K10 assertion for one (assign, sums, counts, cost) result against d2 = ref_kmeans(X, C); returns the
    largest error / bound ratios {"assign", "sums", "cost"}.

    * assign: each computed distance is off by at most (d + 2) u relative (u = eps / 2: one rounding of the
      difference, one of the square, d - 1 of the sum), so the chosen centre is within (1 + 2 (d + 2) eps) of the
      minimum on EVERY row, and equals the argmin wherever the two best differ by more than 4 (d + 2) eps relative.
    * counts: exactly the bincount of the assignment.
    * sums: against the fp64 sums by the SAME assignment.  fp32: the block's LDS accumulator takes one fp32 rounding
      per row, rows_per_block 2^-24 sum|x|.  fp64: (rows_per_block + nblk) 2^-52 sum|x| for the LDS chain and the
      global atomics.
    * cost: (d + 2) eps sum d2[r, assign[r]] for the distances, n 2^-52 of it for the unordered fp64 atomics."""
    n, d = X.shape
    k = C.shape[0]
    eps = eps_of(X.dtype)
    assign, sums, counts, cost = out
    assert assign.dtype == torch.int32 and assign.shape == (n,)
    a = assign.cpu().numpy().astype(np.int64)
    assert a.min() >= 0 and a.max() < k
    rows = np.arange(n)
    da, mn = d2[rows, a], d2.min(axis=1)
    ratios = {}
    excess = da - mn
    assert (excess <= mn * (2 * (d + 2) * eps)).all(), "a row is assigned to a centre that is not nearest"
    with np.errstate(invalid="ignore", divide="ignore"):
        ratios["assign"] = float(np.nan_to_num(excess / (mn * (2 * (d + 2) * eps))).max())
    gap = kmeans_gap_rows(d2, 4 * (d + 2) * eps)
    assert (~gap).sum() <= 1e-4 * n
    assert np.array_equal(a[gap], d2.argmin(axis=1)[gap])
    tot = float(da.astype(LD).sum())
    cost = float(cost)
    cbound = ((d + 2) * eps + n * 2.0 ** -52) * tot
    assert abs(cost - tot) <= cbound, (cost, tot, cbound)
    ratios["cost"] = abs(cost - tot) / cbound if cbound else 0.0
    if not with_sums:
        assert not sums.any() and not counts.any()
        return ratios
    assert np.array_equal(counts.cpu().numpy(), np.bincount(a, minlength=k).astype(np.float64))
    Xl = _np(X)
    ref = np.zeros((k, d), dtype=LD)
    ab = np.zeros((k, d), dtype=LD)
    for c in np.unique(a):
        rc = Xl[a == c]
        ref[c], ab[c] = rc.sum(axis=0), np.abs(rc).sum(axis=0)
    nblk, rpb = kmeans_grid(n)
    bound = (rpb * 2.0 ** -24 if X.dtype == torch.float32 else (rpb + nblk) * 2.0 ** -52) * ab.astype(np.float64)
    err = np.abs(sums.cpu().numpy() - ref.astype(np.float64))
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (err[bound == 0] == 0).all()
    ratios["sums"] = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    return ratios


# ------------------------------------------------------------------------------------------------ K11
def check_logistic(ref, out, n):
    """|g - ref| <= (n + 32) 2^-52 sum_r |res_r x_rf| per gradient entry (sum|res_r| for the intercept, sum|loss_r|
    for the loss): n 2^-52 is the worst case of n unordered fp64 additions, 32 ulp cover exp / log1p and the dot
    product.  ``ref`` is ref_logistic's tuple; returns the largest error / bound ratios {"grad", "loss"}."""
    g_ref, l_ref, ag, al = ref
    grad, loss = out
    g = grad.cpu().numpy()
    assert grad.dtype == torch.float64 and g.shape == g_ref.shape
    u = (n + 32) * 2.0 ** -52
    err, bound = np.abs(g - g_ref), u * ag
    assert (err <= bound).all(), (int(np.argmax(err / np.maximum(bound, 1e-300))),
                                  float((err / np.maximum(bound, 1e-300)).max()))
    lerr, lbound = abs(float(loss) - l_ref), u * al
    assert math.isfinite(float(loss)) and lerr <= lbound, (float(loss), l_ref, lbound)
    return {"grad": float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0,
            "loss": lerr / lbound if lbound else 0.0}


def ref_logistic(X, y, w, b, wt=None):
    """(grad [d+1], loss, abs_grad [d+1], abs_loss): gradient and loss of the weighted binary logistic objective with
    loss_r = wt_r (logaddexp(0, m_r) - y_r m_r), and the sums of absolute terms sum|res_r x_rf| (the last entry
    sum|res_r|, the intercept's) and sum|loss_r| that scale the error bounds."""
    n, d = X.shape
    yl, wl = _np(y), _np(w)
    wtl = np.ones(n, dtype=LD) if wt is None else _np(wt)
    grad, agrad = np.zeros(d + 1, dtype=LD), np.zeros(d + 1, dtype=LD)
    loss = aloss = LD(0)
    step = max(1, (1 << 21) // max(d, 1))         # rows per chunk: the wide copies stay at a few tens of MB
    for r0 in range(0, n, step):
        sl = slice(r0, min(n, r0 + step))
        Xl = _np(X[sl])
        m = (Xl * wl[None, :]).sum(axis=1) + LD(b)
        p = np.exp(-np.logaddexp(LD(0), -m))      # sigmoid without overflow: 0 at m = -800, 1 at m = +800
        res = wtl[sl] * (p - yl[sl])
        li = wtl[sl] * (np.logaddexp(LD(0), m) - yl[sl] * m)
        terms = res[:, None] * Xl
        grad[:d] += terms.sum(axis=0)
        agrad[:d] += np.abs(terms).sum(axis=0)
        grad[d] += res.sum()
        agrad[d] += np.abs(res).sum()
        loss += li.sum()
        aloss += np.abs(li).sum()
    return grad.astype(np.float64), float(loss), agrad.astype(np.float64), float(aloss)


# ------------------------------------------------------------------------------------------------ K13
def ref_reg_metrics(y, p, w=None):
    """(sums [8], abs_sums [8]) in the kernel's order: w, w e^2, w|e|, w y, w y^2, w p, w p^2, w y p."""
    yl, pl = _np(y), _np(p)
    wl = np.ones_like(yl) if w is None else _np(w)
    e = yl - pl
    terms = [wl, wl * e * e, wl * np.abs(e), wl * yl, wl * yl * yl, wl * pl, wl * pl * pl, wl * yl * pl]
    if LD is np.float64 or np.finfo(LD).nmant < 60:   # no wide type: exact sums of the fp64 terms
        s = [math.fsum(t.tolist()) for t in terms]
        a = [math.fsum(np.abs(t).tolist()) for t in terms]
    else:
        s = [float(t.sum()) for t in terms]
        a = [float(np.abs(t).sum()) for t in terms]
    return np.array(s, dtype=np.float64), np.array(a, dtype=np.float64)


def reg_metrics_grid(n: int):
    """(nblk, trips) of the K13 launch: 256-thread blocks, at most 1024 of them, a grid-stride loop beyond."""
    nblk = min(max((n + 255) // 256, 1), 1024)
    return nblk, -(-n // (nblk * 256))


def check_reg_metrics(ref, out, n):
    """|out - ref| <= (trips + 9 + nblk) 2^-52 sum|term| for each of the 8 sums: a thread adds trips =
    ceil(n / (nblk 256)) terms in a chain, the wave butterfly adds 6 roundings, the four-wave add 3, and the final
    pass adds the nblk <= 1024 block partials one after the other.  ``ref`` is ref_reg_metrics' pair; returns the
    largest error / bound ratio."""
    s_ref, a_ref = ref
    nblk, trips = reg_metrics_grid(n)
    o = out.cpu().numpy()
    assert out.dtype == torch.float64 and o.shape == (8,)
    err, bound = np.abs(o - s_ref), (trips + 9 + nblk) * 2.0 ** -52 * a_ref
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).tolist()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------ K14
def ref_score_hist(score, label, lo, hi, nb) -> np.ndarray:
    """Integer counts [nb, 2] (column 1: label > 0.5).  Bucket = (s - lo) * (nb / (hi - lo)) in fp64, truncated, then
    clamped to [0, nb - 1]; the scale is 0 when hi <= lo.  Non-finite products are placed explicitly, never through
    a float -> int conversion: +inf -> nb - 1, -inf -> 0, NaN -> 0."""
    s = _np(score, np.float64)
    lab = _np(label, np.float64)
    scale = float(nb) / (hi - lo) if hi > lo else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        t = (s - lo) * scale
    b = np.zeros(s.shape[0], dtype=np.int64)
    top = t >= nb                                   # +inf included
    mid = (t > 0) & ~top                            # NaN and -inf fail both
    b[top] = nb - 1
    b[mid] = np.trunc(t[mid]).astype(np.int64)
    out = np.zeros((nb, 2), dtype=np.int64)
    np.add.at(out, (b, (lab > 0.5).astype(np.int64)), 1)
    return out


# ------------------------------------------------------------------------------------------------ shared cases
# inputs and references are built once per (shape, type) and shared by the CPU and the GPU module; nobody writes to them
@functools.lru_cache(maxsize=16)
def kmeans_case(n, d, k, dtype):
    X, C = kmeans_data(n, d, k, dtype)
    return X, C, ref_kmeans(X, C)


@functools.lru_cache(maxsize=4)
def logistic_case(n, d, dtype, weighted=False):
    X, y, w, wt = logistic_data(n, d, dtype, weighted=weighted)
    return X, y, w, wt, ref_logistic(X, y, w, 0.3, wt)


@functools.lru_cache(maxsize=16)
def metrics_case(n, weighted, offset=0.0):
    y, p, w = metrics_data(n, weighted, offset=offset)
    return y, p, w, ref_reg_metrics(y, p, w)
