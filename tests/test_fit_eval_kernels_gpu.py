"""K10 kmeans_step, K11 logistic_grad, K13 reg_metrics and K14 score_hist on the device against the independent
high-precision references of tests/_fit_eval_refs.py, at the shapes where each kernel takes another path: every
feature-slot boundary of K11, the grid-stride tails of all four, the LDS limit of K10, row strides, both element
types, weights, ties and non-finite inputs.  The bounds are derived from the kernels' summation orders (stated next
to each check in _fit_eval_refs.py), never from what the kernels return.  Run with -s to see error / bound ratios."""
import math

import numpy as np
import pytest
import torch

from cdnaml.ops import _lib, kernels as K
from tests import _fit_eval_refs as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()  # must load: no silent fallback on a GPU box
    return torch.device("cuda:0")


def _report(kernel, case, ratios):
    print(f"\n[{kernel}] {case}: error/bound " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


def _cpu(out):
    return tuple(o.cpu() if isinstance(o, torch.Tensor) else o for o in out)


# ======================================================================================================= K13
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", R.METRICS_N)
def test_reg_metrics_bound(dev, n, weighted):
    y, p, w, ref = R.metrics_case(n, weighted)
    yd, pd_, wd = y.to(dev), p.to(dev), None if w is None else w.to(dev)
    out = K.reg_metrics(yd, pd_, wd)
    _report("K13", f"n={n} weighted={weighted}", {"sums": R.check_reg_metrics(ref, out, n)})
    # the fixed-order sum the kernel promises: a second call gives the same bits
    assert torch.equal(out, K.reg_metrics(yd, pd_, wd))


@pytest.mark.parametrize("n", [257, 262144 + 257])
def test_reg_metrics_fp32_and_strided_inputs(dev, n):
    """The wrapper's conversions: fp32 inputs widen exactly, a strided view is gathered before the launch."""
    y, p, w, _ = R.metrics_case(n, True)
    y32, p32, w32 = y.float(), p.float(), w.float()
    ref = R.ref_reg_metrics(y32, p32, w32)
    out = K.reg_metrics(y32.to(dev), p32.to(dev), w32.to(dev))
    r32 = R.check_reg_metrics(ref, out, n)
    # every second element of buffers twice as long
    big = [torch.stack([t, t + 1000.0], dim=1).reshape(-1).to(dev) for t in (y, p, w)]
    views = [b[::2] for b in big]
    assert all(v.stride(0) == 2 and not v.is_contiguous() for v in views)
    out = K.reg_metrics(*views)
    rs = R.check_reg_metrics(R.metrics_case(n, True)[3], out, n)
    _report("K13", f"n={n} fp32 / strided", {"fp32": r32, "strided": rs})


def test_reg_metrics_large_offset(dev):
    """y = 1e8 + randn: an fp32 intermediate anywhere would be off by ~1e-8 relative, the bound is ~1e-13."""
    n = 262144 + 257
    y, p, w, ref = R.metrics_case(n, True, 1e8)
    out = K.reg_metrics(y.to(dev), p.to(dev), w.to(dev))
    _report("K13", f"n={n} offset 1e8", {"sums": R.check_reg_metrics(ref, out, n)})


def test_reg_metrics_poisoned_workspace(dev, monkeypatch):
    """n = 257 writes two block partials; the final pass must read those two and nothing else of the workspace."""
    n = 257
    y, p, w, ref = R.metrics_case(n, False)
    real_empty = torch.empty
    poisoned = []

    def nan_empty(*a, **kw):
        t = real_empty(*a, **kw)
        if t.dtype == torch.float64 and t.numel() == 8 * 1024:
            t.fill_(float("nan"))
            poisoned.append(t)
        return t

    yd, pd_ = y.to(dev), p.to(dev)
    monkeypatch.setattr(K.torch, "empty", nan_empty)
    out = K.reg_metrics(yd, pd_)
    monkeypatch.undo()
    assert len(poisoned) == 1
    R.check_reg_metrics(ref, out, n)
    part = poisoned[0].cpu()
    assert not part[:16].isnan().any() and part[16:].isnan().all()   # two blocks' partials written, the rest untouched


# ======================================================================================================= K14
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-7.5, 3.25)])
@pytest.mark.parametrize("nb", R.SCORE_NB)
@pytest.mark.parametrize("n", R.SCORE_N)
def test_score_hist_exact(dev, n, nb, lo, hi):
    s, lab = R.score_data(n, lo, hi)
    ref = R.ref_score_hist(s, lab, lo, hi, nb)
    out = K.score_hist(s.to(dev), lab.to(dev), lo, hi, nb).cpu()
    assert out.dtype == torch.float64 and out.shape == (nb, 2)
    assert np.array_equal(out.numpy(), ref.astype(np.float64))      # fp64 atomicAdd of 1.0 is exact below 2^53
    assert int(ref.sum()) == n


def test_score_hist_edges(dev):
    """Exactly lo, exactly hi (the clamp puts it into the last bucket), below lo, above hi; labels 0.5 / 0 / -1 count
    as negative and 1 / 2 as positive."""
    lo, hi, nb = -7.5, 3.25, 1000
    s = torch.tensor([lo, hi, lo - 1.0, hi + 1.0, hi, lo, math.nextafter(hi, -math.inf)], dtype=torch.float64)
    lab = torch.tensor([0.5, 1.0, 2.0, 0.0, -1.0, 1.0, 1.0], dtype=torch.float64)
    out = K.score_hist(s.to(dev), lab.to(dev), lo, hi, nb).cpu()
    exp = torch.zeros(nb, 2, dtype=torch.float64)
    exp[0] = torch.tensor([1.0, 2.0])          # lo / 0.5 -> negative; lo - 1 / 2.0 and lo / 1.0 -> positive
    exp[nb - 1] = torch.tensor([2.0, 2.0])     # hi + 1 / 0.0 and hi / -1.0 negative; hi / 1.0 and just below hi positive
    assert torch.equal(out, exp)
    assert np.array_equal(R.ref_score_hist(s, lab, lo, hi, nb), exp.numpy().astype(np.int64))


@pytest.mark.parametrize("nb", [1, 7])
def test_score_hist_degenerate_range(dev, nb):
    """hi == lo: the scale is 0 and every row goes to bucket 0."""
    s, lab = R.score_data(300, 2.0, 2.0)
    out = K.score_hist(s.to(dev), lab.to(dev), 2.0, 2.0, nb).cpu()
    ref = R.ref_score_hist(s, lab, 2.0, 2.0, nb)
    assert np.array_equal(out.numpy(), ref.astype(np.float64))
    assert out[0].sum() == 300 and out[1:].sum() == 0


def test_score_hist_non_finite(dev):
    """+inf -> the last bucket, -inf -> bucket 0, NaN -> bucket 0, on the device and on the host path."""
    inf, nan = float("inf"), float("nan")
    s = torch.tensor([inf, -inf, nan, 0.25, inf, nan], dtype=torch.float64)
    lab = torch.tensor([1.0, 1.0, 0.0, 1.0, 0.0, 1.0], dtype=torch.float64)
    nb = 4
    exp = torch.tensor([[1.0, 2.0], [0.0, 1.0], [0.0, 0.0], [1.0, 1.0]], dtype=torch.float64)
    assert np.array_equal(R.ref_score_hist(s, lab, 0.0, 1.0, nb), exp.numpy().astype(np.int64))
    assert torch.equal(K.score_hist(s, lab, 0.0, 1.0, nb), exp)
    assert torch.equal(K.score_hist(s.to(dev), lab.to(dev), 0.0, 1.0, nb).cpu(), exp)


# ======================================================================================================= K10
def _kmeans_shapes():
    for dt in DTYPES:
        for shape in R.KMEANS_SHAPES + [R.KMEANS_LDS_SHAPES[str(dt).split(".")[1]]]:
            yield pytest.param(shape, dt, id=f"{'x'.join(map(str, shape))}-{str(dt).split('.')[1]}")


@pytest.mark.parametrize("shape,dtype", list(_kmeans_shapes()))
def test_kmeans_step_bounds(dev, shape, dtype):
    n, d, k = shape
    X, C, d2 = R.kmeans_case(n, d, k, dtype)
    assert (2 * k * d + k) * X.element_size() <= 64 * 1024          # the kernel's range: this runs on the device
    Xd, Cd = X.to(dev), C.to(dev)
    out = K.kmeans_step(Xd, Cd)
    _report("K10", f"{shape} {dtype}", R.check_kmeans(X, C, out, d2))
    # with_sums=False: the same assignment, the cost within the atomics' bound, nothing accumulated
    out0 = K.kmeans_step(Xd, Cd, with_sums=False)
    assert torch.equal(out0[0], out[0])
    R.check_kmeans(X, C, out0, d2, with_sums=False)
    assert abs(float(out0[3]) - float(out[3])) <= 2 * n * 2.0 ** -52 * float(out[3])


def test_kmeans_step_over_lds_limit_takes_host_path(dev, monkeypatch):
    """(500, 128, 64) fp32 needs 65792 B of LDS, one step over the limit: the wrapper computes on the device tensors
    with torch and never reaches the kernel; the result passes the same assertions."""
    n, d, k = R.KMEANS_OVER_LDS
    X, C, d2 = R.kmeans_case(n, d, k, torch.float32)
    assert (2 * k * d + k) * 4 > 64 * 1024 >= (2 * k * (d - 1) + k) * 4
    native = _lib.lib().cdna_kmeans_step
    # the C guard agrees with the Python guard: this launch is refused, not attempted
    Xd, Cd = X.to(dev), C.to(dev)
    scratch = torch.zeros(n, dtype=torch.int32, device=dev)
    cost = torch.zeros(1, dtype=torch.float64, device=dev)
    assert native(Xd.data_ptr(), n, d, d, Cd.data_ptr(), k, scratch.data_ptr(), None, None, cost.data_ptr(), 0,
                  torch.cuda.current_stream(dev).cuda_stream) != 0

    def no_kernel(*a):
        raise AssertionError("kmeans_kernel launched beyond its LDS limit")

    monkeypatch.setattr(_lib.lib(), "cdna_kmeans_step", no_kernel)
    out = K.kmeans_step(Xd, Cd)
    monkeypatch.undo()
    assert out[0].is_cuda and out[1].is_cuda
    _report("K10", f"{(n, d, k)} host path on device tensors", R.check_kmeans(X, C, out, d2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_kmeans_step_row_stride(dev, dtype, monkeypatch):
    """A column slice (ldx = d + 5, start 3 elements into the row) goes to the kernel as it is: no copy, the same
    assignment bit for bit as the contiguous call."""
    n, d, k = 10000, 4, 5
    X, C, d2 = R.kmeans_case(n, d, k, dtype)
    base = torch.full((n, d + 5), 1e6, dtype=dtype)      # the columns around the slice would ruin every distance
    base[:, 3:3 + d] = X
    base = base.to(dev)
    Xv = base[:, 3:3 + d]
    assert Xv.stride() == (d + 5, 1) and not Xv.is_contiguous()
    seen = {}
    native = _lib.lib().cdna_kmeans_step

    def spy(xp, n_, d_, ldx, *rest):
        seen["ptr"], seen["ldx"] = xp, ldx
        return native(xp, n_, d_, ldx, *rest)

    monkeypatch.setattr(_lib.lib(), "cdna_kmeans_step", spy)
    out = K.kmeans_step(Xv, C.to(dev))
    monkeypatch.undo()
    assert seen == {"ptr": Xv.data_ptr(), "ldx": d + 5}
    assert Xv.data_ptr() == base.data_ptr() + 3 * base.element_size()
    _report("K10", f"{(n, d, k)} {dtype} ldx={d + 5}", R.check_kmeans(X, C, out, d2))
    ref = K.kmeans_step(X.to(dev), C.to(dev))
    assert torch.equal(out[0], ref[0]) and torch.equal(out[2], ref[2])


@pytest.mark.parametrize("dtype", DTYPES)
def test_kmeans_step_ties_and_empty_centre(dev, dtype):
    """Integer data, exact distances: C[3] == C[1], C[0] and C[2] mirror each other in x0, C[4] is far from all
    rows.  The lowest index wins every tie, on the device and on the host: nothing reaches centre 3, rows with
    x0 == 0 go to centre 0 and not 2, and the far centre's count and sums are exactly 0."""
    X, C = R.kmeans_tie_data(dtype)
    d2 = R.ref_kmeans(X, C)
    exp = torch.from_numpy(d2.argmin(axis=1)).int()       # numpy's argmin: the first of equal minima
    host = K.kmeans_step(X, C)
    devo = _cpu(K.kmeans_step(X.to(dev), C.to(dev)))
    assert (X[:, 0] == 0).any() and (d2[:, 1] == d2.min(axis=1)).any()     # both kinds of tie occur
    for out in (host, devo):
        assign, sums, counts, cost = out
        assert torch.equal(assign, exp)
        assert counts[3] == 0 and counts[4] == 0 and not sums[3].any() and not sums[4].any()
        assert torch.equal(counts, torch.bincount(exp.long(), minlength=5).double())
        ref_sums = torch.zeros(5, X.shape[1], dtype=torch.float64).index_add_(0, exp.long(), X.double())
        assert torch.equal(sums, ref_sums)                # small integers: every partial sum is exact
    assert float(devo[3]) == float(d2.min(axis=1).sum())  # and so is the device's cost


@pytest.mark.parametrize("dtype", DTYPES)
def test_kmeans_step_nan_row(dev, dtype):
    """A row holding a NaN has no nearest centre.  The host path is the contract: the cost is NaN, the row goes
    to centre 0, every other row keeps its assignment."""
    X, C, d2 = R.kmeans_case(255, 3, 2, dtype)
    clean = K.kmeans_step(X.to(dev), C.to(dev))[0].cpu()
    Xn = X.clone()
    Xn[100, 1] = float("nan")
    host = K.kmeans_step(Xn, C)
    out = _cpu(K.kmeans_step(Xn.to(dev), C.to(dev)))
    assert math.isnan(float(host[3])) and math.isnan(float(out[3]))
    assert torch.equal(out[0], host[0])
    keep = torch.arange(255) != 100
    assert torch.equal(out[0][keep], clean[keep])
    assert torch.equal(out[2], host[2])


def test_kmeans_step_overflowing_row(dev):
    """An fp32 row of magnitude 1e20: every squared distance overflows.  Host contract: cost inf, centre 0."""
    X, C, d2 = R.kmeans_case(255, 3, 2, torch.float32)
    clean = K.kmeans_step(X.to(dev), C.to(dev))[0].cpu()
    Xn = X.clone()
    Xn[100] = 1e20
    host = K.kmeans_step(Xn, C)
    out = _cpu(K.kmeans_step(Xn.to(dev), C.to(dev)))
    assert float(host[3]) == math.inf and float(out[3]) == math.inf
    assert torch.equal(out[0], host[0]) and int(out[0][100]) == 0
    keep = torch.arange(255) != 100
    assert torch.equal(out[0][keep], clean[keep])
    assert torch.equal(out[2], host[2])


# ======================================================================================================= K11
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", R.LOGISTIC_D)
def test_logistic_grad_feature_slots(dev, d, dtype):
    n = R.LOGISTIC_N_CAP
    X, y, w, wt, ref = R.logistic_case(n, d, dtype)
    out = K.logistic_grad(X.to(dev), y.to(dev), w.to(dev), 0.3)
    _report("K11", f"n={n} d={d} {dtype}", R.check_logistic(ref, out, n))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,weighted", R.LOGISTIC_SMALL + [(R.LOGISTIC_N_CAP, 129, True)])
def test_logistic_grad_few_rows_and_weights(dev, n, d, weighted, dtype):
    X, y, w, wt, ref = R.logistic_case(n, d, dtype, weighted)
    out = K.logistic_grad(X.to(dev), y.to(dev), w.to(dev), 0.3, None if wt is None else wt.to(dev))
    _report("K11", f"n={n} d={d} weighted={weighted} {dtype}", R.check_logistic(ref, out, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_logistic_grad_long_row_loop(dev, dtype):
    n, d = R.LOGISTIC_LARGE
    X, y, w, wt, ref = R.logistic_case(n, d, dtype)
    out = K.logistic_grad(X.to(dev), y.to(dev), w.to(dev), 0.3)
    _report("K11", f"n={n} d={d} {dtype}", R.check_logistic(ref, out, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_logistic_grad_over_d_limit_takes_host_path(dev, dtype, monkeypatch):
    """d = 513 is beyond the eight register slots: torch on the device tensors, and still right."""
    n, d = 300, 513
    X, y, w, wt, ref = R.logistic_case(n, d, dtype)

    def no_kernel(*a):
        raise AssertionError("logistic_kernel launched beyond d = 512")

    monkeypatch.setattr(_lib.lib(), "cdna_logistic_grad", no_kernel)
    out = K.logistic_grad(X.to(dev), y.to(dev), w.to(dev), 0.3)
    monkeypatch.undo()
    assert out[0].is_cuda
    _report("K11", f"n={n} d={d} {dtype} host path on device tensors", R.check_logistic(ref, out, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_logistic_grad_row_stride(dev, dtype, monkeypatch):
    """A column slice with ldx = d + 3 reaches the kernel without a copy."""
    n, d = R.LOGISTIC_N_CAP, 129
    X, y, w, wt, ref = R.logistic_case(n, d, dtype, True)
    base = torch.full((n, d + 3), 1e6, dtype=dtype)
    base[:, 2:2 + d] = X
    base = base.to(dev)
    Xv = base[:, 2:2 + d]
    assert Xv.stride() == (d + 3, 1)
    seen = {}
    native = _lib.lib().cdna_logistic_grad

    def spy(xp, n_, d_, ldx, *rest):
        seen["ptr"], seen["ldx"] = xp, ldx
        return native(xp, n_, d_, ldx, *rest)

    monkeypatch.setattr(_lib.lib(), "cdna_logistic_grad", spy)
    out = K.logistic_grad(Xv, y.to(dev), w.to(dev), 0.3, wt.to(dev))
    monkeypatch.undo()
    assert seen == {"ptr": Xv.data_ptr(), "ldx": d + 3}
    _report("K11", f"n={n} d={d} {dtype} ldx={d + 3}", R.check_logistic(ref, out, n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_logistic_grad_exact_case(dev, dtype):
    """Integer X, w = 0, b = 0: p = 0.5 exactly, every gradient term is a multiple of 1/8 (weights are multiples
    of 1/4) and every partial sum is exact in any order, so the gradient is equal bit for bit; loss = sum(wt) ln 2."""
    n, d = R.LOGISTIC_N_CAP, 129
    X, y, wt = R.logistic_exact_data(n, d, dtype)
    w = torch.zeros(d, dtype=torch.float64)
    res = wt * (0.5 - y)
    exp = torch.cat([X.double().T @ res, res.sum()[None]])
    assert torch.equal(exp, torch.from_numpy(R.ref_logistic(X, y, w, 0.0, wt)[0]))
    for wts in (None, wt):
        r = (0.5 - y) if wts is None else res
        e = torch.cat([X.double().T @ r, r.sum()[None]])
        g, loss = K.logistic_grad(X.to(dev), y.to(dev), w.to(dev), 0.0, None if wts is None else wts.to(dev))
        assert torch.equal(g.cpu(), e)
        tot = float(n if wts is None else wt.sum()) * math.log(2.0)
        assert abs(float(loss) - tot) <= (n + 32) * 2.0 ** -52 * tot


@pytest.mark.parametrize("dtype", DTYPES)
def test_logistic_grad_large_margins(dev, dtype):
    """Rows scaled to margins of about +-800, +-40 and +-25 among ordinary ones: the loss stays finite and within
    the bound, and a row with m = -800, y = 0 (or m = +800, y = 1) adds exactly 0 to the gradient."""
    X, y, w, b, big = R.logistic_margin_data(dtype)
    n = X.shape[0]
    ref = R.ref_logistic(X, y, w, b)
    out = K.logistic_grad(X.to(dev), y.to(dev), w.to(dev), b)
    _report("K11", f"large margins {dtype}", R.check_logistic(ref, out, n))
    # only the saturated rows whose residual is exactly 0: the gradient is exactly 0
    Xs, ys = X[big], y[big]
    g, loss = K.logistic_grad(Xs.to(dev), ys.to(dev), w.to(dev), b)
    assert not g.cpu().any() and math.isfinite(float(loss))
