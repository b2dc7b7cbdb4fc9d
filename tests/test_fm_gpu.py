"""K25 ``fm_step`` on the device against the numpy fp64 reference of ``tests/_fm_refs.py`` (pairwise form), and
FMRegressor fitted end to end on the GPU.

The criterion is K24's.  The precision yardstick is the kernel's sum-of-squares formulation in plain torch fp32 on the
CPU (``_fm_refs.yardstick``): the kernel's error against the reference may be M = 8 times the yardstick's, with a
floor of 4 fp32 ulps (2^-24) of the largest entry for the cases where the yardstick happens to land closer than that.
Every case first asserts the plan, so none silently tests the host formulation; every test prints its kernel /
yardstick figures before it asserts (``-s`` shows them; profiles/r15/fm.md records a run).
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import _lib, kernels as K
from tests import _fm_refs as R
from tests.conftest import session_device

pytestmark = pytest.mark.gpu

M = 8
ULP = 2.0 ** -24
FOLD = 512          # rows a block accumulates in fp32 between folds (asserted against the plan)

# (d, k, n, gradient tiles per wave, load width).  n: tile boundaries, one tile past the fold interval (600 rows in
# one block: a fold after 8 tiles, then 2 more), two blocks (1100).  d and k: around the 32-tile; k = 31 with the
# linear column fills one column block exactly, k = 32 opens the second; (128, 32) is the edge of the native range.
SHAPES = [(5, 3, 1, 1, 1), (5, 3, 63, 1, 1), (5, 3, 64, 1, 1), (5, 3, 65, 1, 1), (5, 3, 130, 1, 1),
          (5, 3, 600, 1, 1), (1, 8, 130, 1, 1), (31, 8, 130, 1, 1), (32, 8, 130, 1, 4), (33, 8, 130, 1, 1),
          (100, 8, 1100, 1, 4), (128, 8, 600, 1, 4), (100, 1, 130, 1, 4), (100, 31, 600, 1, 4),
          (100, 32, 1100, 2, 4), (128, 32, 600, 2, 4)]


class Counting:
    """The native entry points a block of code called (a counting wrapper around ``_lib.check``)."""

    def __enter__(self):
        self.calls = []
        self.orig = _lib.check

        def counting(code, name):
            self.calls.append(name)
            return self.orig(code, name)
        _lib.check = counting
        return self.calls

    def __exit__(self, *exc):
        _lib.check = self.orig


def bounds(c):
    """(loss, gradient entry, raw entry) bounds of a case from its yardstick."""
    return (max(M * abs(c["y_loss"] - c["loss"]), 4 * ULP * abs(c["loss"])),
            max(M * np.abs(c["y_grad"] - c["grad"]).max(), 4 * ULP * np.abs(c["grad"]).max()),
            max(M * np.abs(c["y_raw"] - c["raw"]).max(), 4 * ULP * np.abs(c["raw"]).max()))


def check_step(tag, c, loss, g):
    bl, bg, _ = bounds(c)
    el, eg = abs(loss - c["loss"]), np.abs(g - c["grad"]).max()
    yl, yg = abs(c["y_loss"] - c["loss"]), np.abs(c["y_grad"] - c["grad"]).max()
    gm = max(np.abs(c["grad"]).max(), 1e-300)
    print(f"fm {tag}: loss kernel {el:.2e} yardstick {yl:.2e} bound {bl:.2e} | grad / max|g| kernel {eg / gm:.2e} "
          f"yardstick {yg / gm:.2e} ratio {eg / max(yg, 1e-300):.2f}")
    assert np.isfinite(loss) and np.isfinite(g).all()
    assert el <= bl and eg <= bg


def check_raw(tag, c, raw):
    br = bounds(c)[2]
    er = np.abs(raw - c["raw"]).max()
    print(f"fm {tag}: raw kernel {er:.2e} yardstick {np.abs(c['y_raw'] - c['raw']).max():.2e} bound {br:.2e}")
    assert np.isfinite(raw).all() and er <= br


def on_device(dev, c):
    return torch.tensor(c["X"], device=dev), torch.tensor(c["y"], device=dev)


@pytest.mark.parametrize("loss", [R.SQUARED, R.LOGISTIC])
@pytest.mark.parametrize("d,k,n,slots,vw", SHAPES)
def test_device_matches_reference(gpu_device, d, k, n, slots, vw, loss):
    c = R.case(d, k, n, loss)
    Xd, yd = on_device(gpu_device, c)
    plan = K.fm_plan(Xd, k)
    assert (plan["path"], plan["slots"], plan["vw"], plan["fold_rows"]) == ("native", slots, vw, FOLD), plan
    assert plan["nblk"] == (2 if n > 1024 else 1)
    with Counting() as calls:
        ls, g, cnt = K.fm_step(Xd, yd, c["theta"], k, loss)
        ls2, g2, cnt2 = K.fm_step(Xd, yd, c["theta"], k, loss)
        raw = K.fm_step(Xd, None, c["theta"], k, loss, K.FM_PREDICT)
    assert calls.count("cdna_fm_step") == 3, calls
    # no float atomics: the same bits twice
    assert torch.equal(ls, ls2) and torch.equal(g, g2) and float(cnt) == float(cnt2) == n
    assert g.dtype == raw.dtype == torch.float64 and raw.shape == (n,)
    tag = f"d={d} k={k} n={n} loss={loss}"
    check_step(tag, c, ls.item(), g.cpu().numpy())
    check_raw(tag, c, raw.cpu().numpy())


@pytest.mark.parametrize("loss", [R.SQUARED, R.LOGISTIC])
@pytest.mark.parametrize("lin,icpt", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("d,k,n,td", [(33, 8, 130, 2), (100, 32, 600, 4)])
def test_without_linear_or_intercept(gpu_device, d, k, n, td, lin, icpt, loss):
    """Without the linear column k = 32 fits one column block; the flat layout shrinks accordingly."""
    c = R.case(d, k, n, loss, 0, lin, icpt)
    Xd, yd = on_device(gpu_device, c)
    plan = K.fm_plan(Xd, k, lin)
    assert plan["path"] == "native" and plan["tiles"] == td * (2 if lin and k == 32 else 1), plan
    ls, g, cnt = K.fm_step(Xd, yd, c["theta"], k, loss, K.FM_STEP, lin, icpt)
    raw = K.fm_step(Xd, None, c["theta"], k, loss, K.FM_PREDICT, lin, icpt)
    assert g.shape == (R.num_params(d, k, lin, icpt),) and float(cnt) == n
    tag = f"d={d} k={k} n={n} loss={loss} lin={lin} icpt={icpt}"
    check_step(tag, c, ls.item(), g.cpu().numpy())
    check_raw(tag, c, raw.cpu().numpy())


def test_strided_misaligned_rows_take_the_scalar_loads(gpu_device):
    """X as a column slice of a wider tensor: odd row stride, pointer off 16-byte alignment."""
    d, k, n = 100, 8, 1100
    c = R.case(d, k, n, R.SQUARED)
    wide = torch.full((n, 103), float("nan"), device=gpu_device)
    Xs = wide[:, 1:101]
    Xs.copy_(torch.tensor(c["X"]))
    assert Xs.stride(0) == 103 and Xs.data_ptr() % 16 != 0
    plan = K.fm_plan(Xs, k)
    assert (plan["path"], plan["vw"]) == ("native", 1), plan
    yd = torch.tensor(c["y"], device=gpu_device)
    ls, g, _ = K.fm_step(Xs, yd, c["theta"], k)
    check_step("strided", c, ls.item(), g.cpu().numpy())
    check_raw("strided", c, K.fm_step(Xs, None, c["theta"], k, mode=K.FM_PREDICT).cpu().numpy())


@pytest.mark.parametrize("d,k,n", [(5, 3, 65), (100, 8, 1100)])
def test_rows_past_the_end_are_neither_read_nor_summed(gpu_device, d, k, n):
    """The first n rows of a buffer whose other rows are NaN give the bits of a tight buffer."""
    c = R.case(d, k, n, R.LOGISTIC)
    Xd, yd = on_device(gpu_device, c)
    big = torch.full((n + 200, d), float("nan"), device=gpu_device)
    big[:n] = Xd
    assert K.fm_plan(big[:n], k)["path"] == "native"
    a = K.fm_step(Xd, yd, c["theta"], k, R.LOGISTIC)
    b = K.fm_step(big[:n], yd, c["theta"], k, R.LOGISTIC)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.isfinite(b[1]).all()
    assert torch.equal(K.fm_step(Xd, None, c["theta"], k, mode=K.FM_PREDICT),
                       K.fm_step(big[:n], None, c["theta"], k, mode=K.FM_PREDICT))


@pytest.mark.parametrize("d,k,n", [(100, 32, 1100), (33, 8, 130)])
def test_poisoned_workspace(gpu_device, monkeypatch, d, k, n):
    """The workspace arrives full of NaN with a NaN guard band behind it: everything the reduction reads has been
    written (the result is the unpoisoned call's, bit for bit) and nothing behind the workspace is."""
    c = R.case(d, k, n, R.SQUARED)
    Xd, yd = on_device(gpu_device, c)
    plan = K.fm_plan(Xd, k)
    assert plan["path"] == "native"
    ws_n = _lib.lib().cdna_fm_step_workspace(n, d, k, 1)
    assert ws_n == plan["nblk"] * (plan["tiles"] * 1024 + K.FM_MAX_D + 4)
    clean = K.fm_step(Xd, yd, c["theta"], k)
    guard = 4096
    real_empty = torch.empty
    poisoned = []

    def nan_empty(*a, **kw):
        if kw.get("dtype") == torch.float64 and len(a) == 1 and a[0] == ws_n:
            t = real_empty(ws_n + guard, **kw)
            t.fill_(float("nan"))
            poisoned.append(t)
            return t[:ws_n]
        return real_empty(*a, **kw)

    monkeypatch.setattr(K.torch, "empty", nan_empty)
    out = K.fm_step(Xd, yd, c["theta"], k)
    monkeypatch.undo()
    assert len(poisoned) == 1
    assert all(torch.equal(u, v) for u, v in zip(out, clean)) and torch.isfinite(out[1]).all()
    assert poisoned[0][ws_n:].isnan().all()


@pytest.mark.parametrize("loss", [R.SQUARED, R.LOGISTIC])
@pytest.mark.parametrize("d,k,n", [(5, 3, 130), (100, 8, 1100)])
def test_minibatch_selection_is_the_host_mask(gpu_device, d, k, n, loss):
    """frac = 0.5 at a row offset past 2^32: exactly the rows ``K.uniform`` selects, the sums within the usual bound
    of the reference on that mask; an unselected row adds exactly nothing (NaN labels there change no bit)."""
    c = dict(R.case(d, k, n, loss))
    Xd, yd = on_device(gpu_device, c)
    seed, off, frac = 77, (1 << 32) + 12345, 0.5
    mask = (K.uniform(n, seed, off, K.FM_STREAM, device=gpu_device) < frac).cpu().numpy()
    assert np.array_equal(mask, K.uniform(n, seed, off, K.FM_STREAM).numpy() < frac)
    assert K.fm_plan(Xd, k)["path"] == "native"
    ls, g, cnt = K.fm_step(Xd, yd, c["theta"], k, loss, sample=(seed, off, frac))
    assert float(cnt) == mask.sum()
    c["loss"], c["grad"], _ = R.step(c["X"], c["y"], c["theta"], k, loss, mask=mask)
    c["y_loss"], c["y_grad"], _ = R.yardstick(c["X"], c["y"], c["theta"], k, loss, mask=mask)
    check_step(f"minibatch d={d} k={k} n={n} loss={loss}", c, ls.item(), g.cpu().numpy())
    ynan = yd.clone()
    ynan[torch.tensor(~mask, device=gpu_device)] = float("nan")
    again = K.fm_step(Xd, ynan, c["theta"], k, loss, sample=(seed, off, frac))
    assert all(torch.equal(u, v) for u, v in zip(again, (ls, g, cnt)))
    # the host formulation on the device draws the same mask
    hl, hg, hc = K.fm_step(Xd, yd, c["theta"], k, loss, sample=(seed, off, frac), native=False)
    assert float(hc) == mask.sum() and abs(float(hl) - c["loss"]) <= 1e-12 * abs(c["loss"])


def test_large_logistic_margins_stay_finite(gpu_device):
    """Parameters scaled until the margins pass +-1e4: the sigmoid and log1p(exp) must not overflow.  The loss is
    within the usual bound of the reference, the gradient finite."""
    d, k, n = 20, 8, 500
    X, y, theta = R.make_case(d, k, n, R.LOGISTIC, seed=5, scale=60.0)
    r = R.raw(X, theta, k)
    assert r.max() > 1e4 and r.min() < -1e4
    c = dict(X=X, y=y, theta=theta, raw=r)
    c["loss"], c["grad"], _ = R.step(X, y, theta, k, R.LOGISTIC)
    c["y_loss"], c["y_grad"], c["y_raw"] = R.yardstick(X, y, theta, k, R.LOGISTIC)
    assert np.isfinite(c["loss"]) and np.isfinite(c["y_loss"])
    Xd, yd = on_device(gpu_device, c)
    assert K.fm_plan(Xd, k)["path"] == "native"
    ls, g, _ = K.fm_step(Xd, yd, theta, k, R.LOGISTIC)
    raw = K.fm_step(Xd, None, theta, k, mode=K.FM_PREDICT)
    check_step("large margins", c, ls.item(), g.cpu().numpy())
    check_raw("large margins", c, raw.cpu().numpy())


@pytest.mark.parametrize("d,k,f64", [(K.FM_MAX_D + 1, 8, False), (20, K.FM_MAX_K + 1, False), (20, 8, True)])
def test_outside_the_native_range_takes_the_host_formulation(gpu_device, d, k, f64):
    n = 300
    for loss in (R.SQUARED, R.LOGISTIC):
        X, y, theta = R.make_case(d, k, n, loss, dtype=np.float64 if f64 else np.float32)
        Xd, yd = torch.tensor(X, device=gpu_device), torch.tensor(y, device=gpu_device)
        assert K.fm_plan(Xd, k) == {"path": "host"}
        with Counting() as calls:
            ls, g, cnt = K.fm_step(Xd, yd, theta, k, loss)
            raw = K.fm_step(Xd, None, theta, k, loss, K.FM_PREDICT)
        assert "cdna_fm_step" not in calls, calls
        rl, rg, _ = R.step(X, y, theta, k, loss)
        rr = R.raw(X, theta, k)
        # fp64 on both sides: the formulation and the order of the sums only (tests/test_fm_cpu.py)
        assert abs(ls.item() - rl) <= 1e-12 * abs(rl) and float(cnt) == n
        np.testing.assert_allclose(g.cpu().numpy(), rg, rtol=0, atol=1e-12 * np.abs(rg).max())
        np.testing.assert_allclose(raw.cpu().numpy(), rr, rtol=0, atol=1e-12 * np.abs(rr).max())


# ------------------------------------------------------------------------------------------------ end to end
def _fit(device, tmp_path, X, y, **kw):
    import cdnaml
    from cdnaml.ml.evaluation import RegressionEvaluator
    from cdnaml.ml.feature import VectorAssembler
    from cdnaml.ml.regression import FMRegressor, LinearRegression
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"] = y
    with session_device(device):
        spark = cdnaml.SparkSession.builder.config("cdnaml.warehouse.dir", str(tmp_path / f"wh_{device}")) \
            .getOrCreate()
        spark.conf.set("cdnaml.ml.vectorPrecision", "fp32")
        try:
            with Counting() as calls:
                df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))
                m = FMRegressor(**kw).fit(df)
                rmse = RegressionEvaluator(metricName="rmse").evaluate(m.transform(df))
            lr = RegressionEvaluator(metricName="rmse").evaluate(LinearRegression().fit(df).transform(df))
            theta = np.concatenate([m.factors.toArray().reshape(-1), m.linear.toArray(), [m.intercept]])
            out = (theta, rmse, lr, m.fitHistory)
        finally:
            spark.conf.set("cdnaml.ml.vectorPrecision", "auto")
            spark.stop()
    return out, calls


def test_product_term_fit_on_the_device(gpu_device, tmp_path):
    from tests.test_fm_cpu import REG_FIT
    X, y = R.product_data(600, 4, seed=0)
    (theta, rmse, lr, hist), calls = _fit("cuda", tmp_path, X, y, seed=0, **REG_FIT)
    print(f"fm product term on the device: FM rmse {rmse:.4f} LinearRegression rmse {lr:.4f} after {len(hist)} "
          f"iterations")
    # every iteration and the transform ran the kernel
    assert calls.count("cdna_fm_step") >= len(hist) + 1, calls
    assert lr > 0.8 and rmse <= 0.5 * lr


def test_one_adamw_iteration_on_the_device_matches_the_cpu_session(gpu_device, tmp_path):
    """maxIter = 1, the same seed, fp32 feature vectors in both sessions: the CPU session evaluates the host
    formulation (fp64 at the same parameters), so the two mean gradients differ by the STEP error, at most eps =
    bound(un-normalised gradient) / n per entry.  AdamW's first update is theta0 - stepSize g / (|g| + 1e-8) (the
    corrected moments are g and g^2), whose derivative in g is 1e-8 / (|g| + 1e-8)^2 <= 1 for |g| >= 1e-4 (asserted
    on the reference gradient): the weights agree within stepSize eps."""
    from cdnaml.models.regression import fm_initial_params
    n, d, k, step = 3000, 4, 3, 0.05
    X, y = R.product_data(n, d, seed=3)
    X = X.astype(np.float32)
    kw = dict(factorSize=k, maxIter=1, stepSize=step, initStd=0.5, seed=9)
    (tg, _, _, hg), calls = _fit("cuda", tmp_path, X, y, **kw)
    (tc, _, _, hc), _ = _fit("cpu", tmp_path, X, y, **kw)
    assert calls.count("cdna_fm_step") >= 2 and len(hg) == len(hc) == 1 and hg[0][1] == hc[0][1] == n
    theta0 = fm_initial_params(d, k, True, True, 0.5, 9)
    t32 = theta0.astype(np.float32).astype(np.float64)
    c = dict(raw=R.raw(X, t32, k))
    c["loss"], c["grad"], _ = R.step(X, y, t32, k, R.SQUARED)
    c["y_loss"], c["y_grad"], c["y_raw"] = R.yardstick(X, y, t32, k, R.SQUARED)
    assert np.abs(c["grad"] / n).min() >= 1e-4
    bound = step * bounds(c)[1] / n
    moved = np.abs(tc - theta0).max()
    print(f"fm one adamW iteration: |theta_gpu - theta_cpu| {np.abs(tg - tc).max():.2e} bound {bound:.2e} "
          f"(step {moved:.2e}), loss {hg[0][0]:.6f} / {hc[0][0]:.6f}")
    assert abs(moved - step) <= 1e-6 * step and np.abs(tg - tc).max() <= bound
