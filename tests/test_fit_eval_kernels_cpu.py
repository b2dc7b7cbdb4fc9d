"""The host fallbacks of K.kmeans_step, K.logistic_grad, K.reg_metrics and K.score_hist against the references of
tests/_fit_eval_refs.py at the small shapes of tests/test_fit_eval_kernels_gpu.py, the pre-checks of the input
conditions the GPU module relies on, and the argument that its assertions would catch a wrong kernel: four
one-line kernel mutations, replayed in numpy, each miss a bound or an equality."""
import math

import numpy as np
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _fit_eval_refs as R

DTYPES = [torch.float32, torch.float64]
SMALL_KMEANS = [s for s in R.KMEANS_SHAPES if s[0] <= 10000]


def _name(dt):
    return str(dt).split(".")[1]


# ======================================================================================================= inputs
@pytest.mark.parametrize("dtype", DTYPES)
def test_kmeans_inputs_have_few_near_ties(dtype):
    """From the reference alone: at every shape the GPU module uses, the rows left out of the exact-argmin check
    (best and second best within 4 (d + 2) eps relative) are at most 1e-4 of n."""
    for n, d, k in R.KMEANS_SHAPES + [R.KMEANS_LDS_SHAPES[_name(dtype)], R.KMEANS_OVER_LDS]:
        X, C, d2 = R.kmeans_case(n, d, k, dtype)
        gap = R.kmeans_gap_rows(d2, 4 * (d + 2) * R.eps_of(dtype))
        assert (~gap).sum() <= 1e-4 * n, (n, d, k, int((~gap).sum()))
        if n >= 40 * k:
            assert len(np.unique(d2.argmin(axis=1))) == k      # every centre is somebody's nearest


def test_kmeans_lds_shapes_sit_at_the_limit():
    for dt, size in ((torch.float32, 4), (torch.float64, 8)):
        n, d, k = R.KMEANS_LDS_SHAPES[_name(dt)]
        assert (2 * k * d + k) * size == 65280
    n, d, k = R.KMEANS_OVER_LDS
    assert (2 * k * d + k) * 4 == 65792 > 64 * 1024


def test_grid_models_match_the_launch_caps():
    assert R.reg_metrics_grid(257) == (2, 1)
    assert R.reg_metrics_grid(262144 + 257) == (1024, 2)      # some threads run two trips, most one
    assert R.reg_metrics_grid(1 << 20) == (1024, 4)
    assert R.kmeans_grid(524288 + 300) == (2048, 257)
    assert R.LOGISTIC_N_CAP > 1024 * 4 * 2                    # every wave of the capped K11 grid loops, some 3 times


def test_score_data_covers_the_edges():
    for lo, hi in ((0.0, 1.0), (-7.5, 3.25)):
        s, lab = R.score_data(300, lo, hi)
        assert (s == lo).any() and (s == hi).any() and (s < lo).any() and (s > hi).any()
        assert set(lab.tolist()) == {0.5, 1.0, 2.0, 0.0, -1.0}
        ref = R.ref_score_hist(s, lab, lo, hi, 1000)
        # the documented placement: label 0.5 is negative, a score of exactly hi is in the last bucket
        assert ref[:, 1].sum() == int((lab > 0.5).sum()) and ref[999].sum() == int((s >= hi).sum())
        assert ref[0].sum() == int((s < lo + (hi - lo) / 1000).sum())


def test_logistic_margin_rows():
    X, y, w, b, big = R.logistic_margin_data(torch.float64)
    m = X @ w + b
    tgt = torch.tensor([800.0, -800.0, 40.0, -40.0, 25.0, -25.0]).repeat_interleave(2).double()
    assert torch.allclose(m[200:], tgt, rtol=1e-9) and m[:200].abs().max() < 15
    m32 = R.logistic_margin_data(torch.float32)[0].double() @ w + b
    assert torch.allclose(m32[200:], tgt, rtol=1e-4)
    assert int(big.sum()) == 2 and set(zip(tgt[big[200:]].tolist(), y[big].tolist())) == {(800.0, 1.0), (-800.0, 0.0)}


# ======================================================================================================= K13
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [n for n in R.METRICS_N if n <= 257])
def test_reg_metrics_host(n, weighted):
    y, p, w, ref = R.metrics_case(n, weighted)
    out = K.reg_metrics(y, p, w)
    R.check_reg_metrics(ref, out, n)
    assert torch.equal(out, K.reg_metrics(y, p, w))
    if weighted and n > 1:
        assert (w == 0).any() and (w != w.round()).any()
    # fp32 and strided inputs give the sums of the values they hold
    y32, p32 = y.float(), p.float()
    R.check_reg_metrics(R.ref_reg_metrics(y32, p32, w), K.reg_metrics(y32, p32, w), n)
    yy = torch.stack([y, y + 1000.0], dim=1).reshape(-1)[::2]
    R.check_reg_metrics(ref, K.reg_metrics(yy, p, w), n)


def test_reg_metrics_host_large_offset():
    y, p, w, ref = R.metrics_case(257, True, 1e8)
    R.check_reg_metrics(ref, K.reg_metrics(y, p, w), 257)
    # the case has teeth: the same sums from fp32-rounded inputs miss the bound by orders of magnitude
    with pytest.raises(AssertionError):
        R.check_reg_metrics(ref, K.reg_metrics(y.float(), p.float(), w), 257)


# ======================================================================================================= K14
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-7.5, 3.25), (2.0, 2.0)])
@pytest.mark.parametrize("nb", R.SCORE_NB)
@pytest.mark.parametrize("n", [1, 300])
def test_score_hist_host(n, nb, lo, hi):
    s, lab = R.score_data(n, lo, hi)
    ref = R.ref_score_hist(s, lab, lo, hi, nb)
    out = K.score_hist(s, lab, lo, hi, nb)
    assert np.array_equal(out.numpy(), ref.astype(np.float64))
    if hi == lo:
        assert out[0].sum() == n


def test_score_hist_host_non_finite():
    inf, nan = float("inf"), float("nan")
    s = torch.tensor([inf, -inf, nan, 0.25, inf, nan], dtype=torch.float64)
    lab = torch.tensor([1.0, 1.0, 0.0, 1.0, 0.0, 1.0], dtype=torch.float64)
    exp = torch.tensor([[1.0, 2.0], [0.0, 1.0], [0.0, 0.0], [1.0, 1.0]], dtype=torch.float64)
    assert np.array_equal(R.ref_score_hist(s, lab, 0.0, 1.0, 4), exp.numpy().astype(np.int64))
    assert torch.equal(K.score_hist(s, lab, 0.0, 1.0, 4), exp)


# ======================================================================================================= K10
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SMALL_KMEANS + ["lds", R.KMEANS_OVER_LDS])
def test_kmeans_step_host(shape, dtype):
    n, d, k = R.KMEANS_LDS_SHAPES[_name(dtype)] if shape == "lds" else shape
    X, C, d2 = R.kmeans_case(n, d, k, dtype)
    out = K.kmeans_step(X, C)
    R.check_kmeans(X, C, out, d2)
    base = torch.full((n, d + 5), 1e6, dtype=dtype)
    base[:, 3:3 + d] = X
    outv = K.kmeans_step(base[:, 3:3 + d], C)
    assert torch.equal(outv[0], out[0])
    R.check_kmeans(X, C, outv, d2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_kmeans_step_host_ties_and_empty_centre(dtype):
    X, C = R.kmeans_tie_data(dtype)
    d2 = R.ref_kmeans(X, C)
    exp = torch.from_numpy(d2.argmin(axis=1)).int()
    assert (X[:, 0] == 0).any() and ((d2[:, 1] == d2.min(axis=1)) & (d2[:, 0] > d2[:, 1])).any()
    assign, sums, counts, cost = K.kmeans_step(X, C)
    assert torch.equal(assign, exp)
    assert counts[3] == 0 and counts[4] == 0 and not sums[3].any() and not sums[4].any()
    assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_kmeans_step_host_non_finite(dtype):
    """The contract the device is held to: NaN row -> cost NaN, overflowing fp32 row -> cost inf, centre 0 either way,
    the other rows untouched."""
    X, C, d2 = R.kmeans_case(255, 3, 2, dtype)
    clean = K.kmeans_step(X, C)[0]
    keep = torch.arange(255) != 100
    Xn = X.clone()
    Xn[100, 1] = float("nan")
    a, s, c, cost = K.kmeans_step(Xn, C)
    assert math.isnan(float(cost)) and int(a[100]) == 0 and torch.equal(a[keep], clean[keep])
    if dtype == torch.float32:
        Xn = X.clone()
        Xn[100] = 1e20
        a, s, c, cost = K.kmeans_step(Xn, C)
        assert float(cost) == math.inf and int(a[100]) == 0 and torch.equal(a[keep], clean[keep])


# ======================================================================================================= K11
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 65, 129, 513])
def test_logistic_grad_host(d, dtype):
    n = 300
    X, y, w, wt, ref = R.logistic_case(n, d, dtype, True)
    R.check_logistic(ref, K.logistic_grad(X, y, w, 0.3, wt), n)
    assert (wt == 0).any()
    base = torch.full((n, d + 3), 1e6, dtype=dtype)
    base[:, 2:2 + d] = X
    R.check_logistic(ref, K.logistic_grad(base[:, 2:2 + d], y, w, 0.3, wt), n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,weighted", R.LOGISTIC_SMALL)
def test_logistic_grad_host_few_rows(n, d, weighted, dtype):
    X, y, w, wt, ref = R.logistic_case(n, d, dtype, weighted)
    R.check_logistic(ref, K.logistic_grad(X, y, w, 0.3, wt), n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_logistic_grad_host_exact_case(dtype):
    n, d = 1000, 129
    X, y, wt = R.logistic_exact_data(n, d, dtype)
    w = torch.zeros(d, dtype=torch.float64)
    res = wt * (0.5 - y)
    exp = torch.cat([X.double().T @ res, res.sum()[None]])
    assert torch.equal(exp, torch.from_numpy(R.ref_logistic(X, y, w, 0.0, wt)[0]))
    g, loss = K.logistic_grad(X, y, w, 0.0, wt)
    assert torch.equal(g, exp)
    tot = float(wt.sum()) * math.log(2.0)
    assert abs(float(loss) - tot) <= (n + 32) * 2.0 ** -52 * tot


@pytest.mark.parametrize("dtype", DTYPES)
def test_logistic_grad_host_large_margins(dtype):
    X, y, w, b, big = R.logistic_margin_data(dtype)
    ref = R.ref_logistic(X, y, w, b)
    assert math.isfinite(ref[1]) and ref[1] > 800
    R.check_logistic(ref, K.logistic_grad(X, y, w, b), X.shape[0])
    g, loss = K.logistic_grad(X[big], y[big], w, b)
    assert not g.any() and math.isfinite(float(loss))


# ================================================================================ the assertions have teeth
# Each of four one-line changes to misc.hip, replayed in numpy on the GPU module's inputs, misses an assertion that
# module makes: lane + 32 q in K11, a single-trip loop in K13, a clamp to nb - 2 in K14, dist <= best in K10.
@pytest.mark.parametrize("d", [63, 65, 129, 512])
def test_mutant_logistic_lane_slot_is_caught(d):
    """f = lane + 32 q instead of lane + 64 q: features 32 .. 255 are visited twice (their products enter the margin
    twice, their gradient is added twice), features 256 .. 287 once and features >= 288 never.  Only d <= 32
    survives."""
    n = 300
    X, y, w, wt, ref = R.logistic_case(n, d, torch.float64, True)
    f = np.arange(d)
    mult = ((f[None, :] == (np.arange(64)[:, None, None] + 32 * np.arange(8)[None, :, None])).sum(axis=(0, 1)))
    assert (mult == np.where(f < 32, 1, np.where(f < 256, 2, np.where(f < 288, 1, 0)))).all()
    Xn, wn = X.numpy(), w.numpy()
    m = (Xn * (wn * mult)[None, :]).sum(axis=1) + 0.3
    res = wt.numpy() * (1.0 / (1.0 + np.exp(-m)) - y.numpy())
    g = np.concatenate([(res[:, None] * Xn).sum(axis=0) * mult, [res.sum()]])
    loss = (wt.numpy() * (np.logaddexp(0.0, m) - y.numpy() * m)).sum()
    with pytest.raises(AssertionError):
        R.check_logistic(ref, (torch.from_numpy(g), torch.tensor(loss)), n)
    # the unmutated replay passes: the failure is the mutation's
    m = (Xn * wn[None, :]).sum(axis=1) + 0.3
    res = wt.numpy() * (1.0 / (1.0 + np.exp(-m)) - y.numpy())
    g = np.concatenate([(res[:, None] * Xn).sum(axis=0), [res.sum()]])
    loss = (wt.numpy() * (np.logaddexp(0.0, m) - y.numpy() * m)).sum()
    R.check_logistic(ref, (torch.from_numpy(g), torch.tensor(loss)), n)


def test_mutant_reg_metrics_single_trip_is_caught():
    """The grid-stride loop cut to one trip drops the rows past 1024 x 256: at n = 262144 + 257 every sum loses 257
    terms, about 1e-3 of it against a bound of about 2e-13."""
    n = 262144 + 257
    y, p, w, ref = R.metrics_case(n, False)
    cut = 1024 * 256
    with pytest.raises(AssertionError):
        R.check_reg_metrics(ref, K.reg_metrics(y[:cut], p[:cut]), n)
    R.check_reg_metrics(ref, K.reg_metrics(y, p), n)


@pytest.mark.parametrize("nb", [2, 1000])
def test_mutant_score_hist_clamp_is_caught(nb):
    """Clamping to nb - 2 moves every score >= hi one bucket down; the inputs hold such scores, so exact equality
    fails."""
    lo, hi = -7.5, 3.25
    s, lab = R.score_data(300, lo, hi)
    ref = R.ref_score_hist(s, lab, lo, hi, nb)
    t = (s.numpy() - lo) * (nb / (hi - lo))
    b = np.where(t >= nb, nb - 2, np.clip(np.trunc(t), 0, None)).astype(np.int64)
    mut = np.zeros((nb, 2), dtype=np.int64)
    np.add.at(mut, (b, (lab.numpy() > 0.5).astype(np.int64)), 1)
    assert not np.array_equal(mut, ref) and mut.sum() == ref.sum()


@pytest.mark.parametrize("dtype", DTYPES)
def test_mutant_kmeans_last_tie_wins_is_caught(dtype):
    """dist <= best makes the LAST of equal distances win: rows nearest to C[1] == C[3] move to centre 3."""
    X, C = R.kmeans_tie_data(dtype)
    d2 = R.ref_kmeans(X, C)
    last = d2.shape[1] - 1 - d2[:, ::-1].argmin(axis=1)
    assert not np.array_equal(last, d2.argmin(axis=1)) and (last == 3).any()
