"""K26 ``aft_step`` on the device against the longdouble reference of ``tests/_aft_refs.py``, and
AFTSurvivalRegression fitted end to end on the GPU.

The criterion is that of the host-formulation tests: the kernel's error against the reference may be M = 8 times the
error of the plain numpy fp64 yardstick, with a floor of 4 fp64 ulps (2^-53) of the largest entry.  Every case first
asserts the plan, so none silently tests the host formulation; every case prints its kernel / yardstick figures
before it asserts (``-s`` shows them; profiles/r16/aft.md records a run).
"""
import math

import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import _lib, kernels as K
from tests import _aft_refs as R
from tests.conftest import session_device

pytestmark = pytest.mark.gpu

N2 = 1025           # the smallest n the plan gives two blocks (asserted)

# (d, n, load width): tile boundaries; d around the four threads of a row and their 32-column quarters; the edge of
# the native range; two blocks
SHAPES = [(5, 1, 1), (5, 63, 1), (5, 64, 1), (5, 65, 1), (5, 130, 1),
          (1, 130, 1), (3, 130, 1), (4, 130, 4), (31, 130, 1), (32, 130, 4), (33, 130, 1),
          (127, 600, 1), (128, 600, 4), (100, N2, 4)]


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


def on_device(dev, c, X=None, t=None, censor=None):
    with np.errstate(divide="ignore", invalid="ignore"):
        lt = c["logt"] if t is None else np.log(t)
    return (torch.tensor(c["X"] if X is None else X, device=dev), torch.tensor(lt, device=dev),
            torch.tensor(c["censor"] if censor is None else censor, device=dev))


def step(c, Xd, ltd, dld, **kw):
    return K.aft_step(Xd, ltd, dld, c["coef"], c["b0"], c["ls"], **kw)


def check_all(tag, c, Xd, ltd, dld):
    ls, g, bad = step(c, Xd, ltd, dld)
    pred, quant = step(c, Xd, None, None, mode=K.AFT_PREDICT, probs=R.PROBS)
    n, d = c["X"].shape
    assert g.dtype == pred.dtype == quant.dtype == torch.float64
    assert g.shape == (d + 2,) and pred.shape == (n,) and quant.shape == (n, len(R.PROBS))
    assert float(bad) == 0.0
    R.check(tag + " loss", ls.item(), c["loss"], c["y_loss"])
    R.check(tag + " grad", g.cpu().numpy(), c["grad"], c["y_grad"])
    R.check(tag + " pred", pred.cpu().numpy(), c["pred"], c["y_pred"])
    R.check(tag + " quant", quant.cpu().numpy(), c["quant"], c["y_quant"])
    assert torch.equal(step(c, Xd, None, None, mode=K.AFT_PREDICT), pred)
    return ls, g, bad, pred, quant


@pytest.mark.parametrize("d,n,vw", SHAPES)
def test_device_matches_reference(gpu_device, d, n, vw):
    c = R.case(d, n)
    Xd, ltd, dld = on_device(gpu_device, c)
    plan = K.aft_plan(Xd)
    assert (plan["path"], plan["vw"]) == ("native", vw), plan
    assert plan["nblk"] == (2 if n >= N2 else 1), plan
    if n == N2:
        assert K.aft_plan(Xd[:N2 - 1])["nblk"] == 1
    with Counting() as calls:
        a = step(c, Xd, ltd, dld)
        b = step(c, Xd, ltd, dld)
    assert calls.count("cdna_aft_step") == 2, calls
    # no float atomics: the same bits twice
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    with Counting() as calls:
        check_all(f"d={d} n={n}", c, Xd, ltd, dld)
    assert calls.count("cdna_aft_step") == 3, calls


def test_more_quantiles_than_the_kernel_writes(gpu_device):
    c = R.case(33, 130)
    Xd, _, _ = on_device(gpu_device, c)
    probs = list(np.linspace(0.02, 0.98, K.AFT_MAX_Q + 1))
    assert K.aft_plan(Xd)["path"] == "native"
    with Counting() as calls:
        pred, quant = step(c, Xd, None, None, mode=K.AFT_PREDICT, probs=probs)
    assert calls.count("cdna_aft_step") == 1 and quant.shape == (130, K.AFT_MAX_Q + 1)
    _, _, rp, rq = R.reference(c["X"], c["t"], c["censor"], c["coef"], c["b0"], c["ls"], probs)
    _, _, yp, yq = R.yardstick(c["X"], c["t"], c["censor"], c["coef"], c["b0"], c["ls"], probs)
    R.check("17 quantiles pred", pred.cpu().numpy(), rp, yp)
    R.check("17 quantiles quant", quant.cpu().numpy(), rq, yq)


def test_strided_misaligned_rows_take_the_scalar_loads(gpu_device):
    """X as a column slice of a wider tensor: odd row stride, pointer off 16-byte alignment."""
    d, n = 100, N2
    c = R.case(d, n)
    wide = torch.full((n, 103), float("nan"), device=gpu_device)
    Xs = wide[:, 1:101]
    Xs.copy_(torch.tensor(c["X"]))
    assert Xs.stride(0) == 103 and Xs.data_ptr() % 16 != 0
    plan = K.aft_plan(Xs)
    assert (plan["path"], plan["vw"], plan["nblk"]) == ("native", 1, 2), plan
    _, ltd, dld = on_device(gpu_device, c)
    check_all("strided", c, Xs, ltd, dld)


@pytest.mark.parametrize("d,n", [(5, 65), (100, N2)])
def test_rows_past_the_end_are_neither_read_nor_summed(gpu_device, d, n):
    """The first n rows of a buffer whose other rows are NaN give the bits of a tight buffer."""
    c = R.case(d, n)
    Xd, ltd, dld = on_device(gpu_device, c)
    big = torch.full((n + 200, d), float("nan"), device=gpu_device)
    big[:n] = Xd
    assert K.aft_plan(big[:n])["path"] == "native"
    a = step(c, Xd, ltd, dld)
    b = step(c, big[:n], ltd, dld)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.isfinite(b[1]).all() and float(b[2]) == 0.0
    pa = step(c, Xd, None, None, mode=K.AFT_PREDICT, probs=R.PROBS)
    pb = step(c, big[:n], None, None, mode=K.AFT_PREDICT, probs=R.PROBS)
    assert all(torch.equal(u, v) for u, v in zip(pa, pb))


@pytest.mark.parametrize("d,n", [(100, N2), (33, 130)])
def test_poisoned_workspace(gpu_device, monkeypatch, d, n):
    """The workspace arrives full of NaN with a NaN guard band behind it: everything the reduction reads has been
    written (the result is the unpoisoned call's, bit for bit) and nothing behind the workspace is."""
    c = R.case(d, n)
    Xd, ltd, dld = on_device(gpu_device, c)
    plan = K.aft_plan(Xd)
    assert plan["path"] == "native"
    ws_n = _lib.lib().cdna_aft_step_workspace(n, d)
    assert ws_n == plan["nblk"] * plan["slot"] == plan["nblk"] * (K.AFT_MAX_D + 4) and ws_n != d + 4
    clean = step(c, Xd, ltd, dld)
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
    out = step(c, Xd, ltd, dld)
    monkeypatch.undo()
    assert len(poisoned) == 1
    assert all(torch.equal(u, v) for u, v in zip(out, clean)) and torch.isfinite(out[1]).all()
    assert poisoned[0][ws_n:].isnan().all()


@pytest.mark.parametrize("d,n", [(5, 130), (100, N2)])
def test_bad_rows_are_counted_and_add_nothing(gpu_device, d, n):
    """One bad row of each kind: ``bad`` is their number, the other sums are the reference's without those rows."""
    from tests.test_aft_cpu import BAD_KINDS, plant
    c = R.case(d, n)
    rows = [0, 17, 63, 64, 100, n - 1]
    X, t, dl = plant(c, BAD_KINDS, rows)
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    rl, rg, _, _ = R.reference(c["X"], c["t"], c["censor"], c["coef"], c["b0"], c["ls"], keep=keep)
    yl, yg, _, _ = R.yardstick(c["X"], c["t"], c["censor"], c["coef"], c["b0"], c["ls"], keep=keep)
    Xd, ltd, dld = on_device(gpu_device, c, X, t, dl)
    assert K.aft_plan(Xd)["path"] == "native"
    ls, g, bad = step(c, Xd, ltd, dld)
    assert float(bad) == len(rows)
    R.check(f"bad rows d={d} n={n} loss", ls.item(), rl, yl)
    R.check(f"bad rows d={d} n={n} grad", g.cpu().numpy(), rg, yg)


def test_overflow_is_reported_as_bad_rows_with_finite_sums(gpu_device):
    c = R.case(5, 130)
    Xd, ltd, dld = on_device(gpu_device, c)
    assert K.aft_plan(Xd)["path"] == "native"
    ls, g, bad = K.aft_step(Xd, ltd, dld, c["coef"], c["b0"], -8.0)
    hl, hg, hbad = K.aft_step(Xd, ltd, dld, c["coef"], c["b0"], -8.0, native=False)
    print(f"aft overflow: bad {float(bad):.0f} (host formulation {float(hbad):.0f})")
    assert 0 < float(bad) < 130 and abs(float(bad) - float(hbad)) <= 1
    assert math.isfinite(ls.item()) and torch.isfinite(g).all()


@pytest.mark.parametrize("d,f64", [(K.AFT_MAX_D + 1, False), (20, True)])
def test_outside_the_native_range_takes_the_host_formulation(gpu_device, d, f64):
    n = 300
    c = R.case(d, n)
    Xd, ltd, dld = on_device(gpu_device, c)
    Xd = Xd.double() if f64 else Xd
    assert K.aft_plan(Xd) == {"path": "host"}
    with Counting() as calls:
        check_all(f"host on the device d={d} f64={f64}", c, Xd, ltd, dld)
    assert "cdna_aft_step" not in calls, calls


# ------------------------------------------------------------------------------------------------ end to end
def _fit(device, tmp_path, X, t, dl, **kw):
    import cdnaml
    from cdnaml.ml.feature import VectorAssembler
    from cdnaml.ml.regression import AFTSurvivalRegression
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"], pdf["censor"] = t, dl
    with session_device(device):
        spark = cdnaml.SparkSession.builder.config("cdnaml.warehouse.dir", str(tmp_path / f"wh_{device}")) \
            .getOrCreate()
        spark.conf.set("cdnaml.ml.vectorPrecision", "fp32")
        try:
            with Counting() as calls:
                df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))
                m = AFTSurvivalRegression(quantilesCol="q", **kw).fit(df)
                out = m.transform(df).select("prediction", "q").toPandas()
            theta = np.concatenate([m.coefficients.toArray(), [m.intercept, math.log(m.scale)]])
            q = np.stack([np.asarray(v.toArray() if hasattr(v, "toArray") else v) for v in out.q])
            res = (theta, m.scale, out.prediction.to_numpy(), q)
        finally:
            spark.conf.set("cdnaml.ml.vectorPrecision", "auto")
            spark.stop()
    return res, calls


def test_fit_on_the_device_matches_the_cpu_session(gpu_device, tmp_path):
    n, d = 3000, 33
    X, t, dl, _, _ = R.make_data(d, n)
    (tg, scale, pred, q), calls = _fit("cuda", tmp_path, X, t, dl, tol=1e-14, maxIter=500)
    (tc, _, _, _), ccalls = _fit("cpu", tmp_path, X, t, dl, tol=1e-14, maxIter=500)
    print(f"aft fit on the device: |theta_gpu - theta_cpu| {np.abs(tg - tc).max():.2e}, "
          f"{calls.count('cdna_aft_step')} native calls")
    assert calls.count("cdna_aft_step") >= 3 and "cdna_aft_step" not in ccalls
    assert np.abs(tg - tc).max() <= 1e-6
    want = np.exp(X.astype(np.float64) @ tg[:d] + tg[d])
    qf = np.exp(scale * np.log(-np.log1p(-np.asarray(R.PROBS))))
    np.testing.assert_allclose(pred, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(q, want[:, None] * qf[None, :], rtol=1e-12, atol=0)
