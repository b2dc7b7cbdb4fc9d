"""K24 ``mlp_step`` on the device against the numpy fp64 reference of ``tests/_mlp_refs.py``, and
MultilayerPerceptronClassifier fitted end to end on the GPU.

The precision yardstick is the same computation in plain torch fp32 on the CPU (``_mlp_refs.yardstick``): the kernel's
error against the reference may be M = 8 times the yardstick's (another summation order within and across the 64-row
tiles, a device exp a few ulps from torch's), with a floor of 4 fp32 ulps (2^-24) of the largest entry for the cases
where the yardstick happens to land closer than that.  Every case first asserts the plan, so none silently tests the
host formulation; every test prints its kernel / yardstick figures before it asserts (``-s`` shows them;
profiles/r14/mlp.md records a run).
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import _lib, kernels as K
from tests import _mlp_refs as R
from tests.conftest import session_device

pytestmark = pytest.mark.gpu

M = 8
ULP = 2.0 ** -24
WIDEST = [K.MLP_MAX_WIDTH] * (K.MLP_MAX_LAYERS + 1)

# (layers, n, gradient tiles per wave, load width): tile boundaries, widths straddling a 32-tile, the benchmark net,
# the upper edge of the native range, no hidden layer
SHAPES = [([5, 4, 3], 1, 1, 1), ([5, 4, 3], 63, 1, 1), ([5, 4, 3], 64, 1, 1), ([5, 4, 3], 65, 1, 1),
          ([5, 4, 3], 130, 1, 1), ([33, 33, 2], 257, 3, 1), ([100, 64, 32, 3], 1000, 3, 4), (WIDEST, 200, 12, 4),
          ([100, 3], 300, 1, 4), ([64, 128, 2], 700, 3, 4), ([128, 96, 5], 2100, 6, 4)]


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
    print(f"mlp {tag}: loss kernel {el:.2e} yardstick {yl:.2e} bound {bl:.2e} | grad / max|g| kernel "
          f"{eg / np.abs(c['grad']).max():.2e} yardstick {yg / np.abs(c['grad']).max():.2e} ratio "
          f"{eg / max(yg, 1e-300):.2f}")
    assert np.isfinite(loss) and np.isfinite(g).all()
    assert el <= bl and eg <= bg


def check_predict(tag, c, raw, prob, pred):
    _, _, br = bounds(c)
    er, ep = np.abs(raw - c["raw"]).max(), np.abs(prob - c["prob"]).max()
    # pred is the argmax of the kernel's own raw, the lowest index among equals
    assert np.array_equal(pred, np.argmax(raw, 1))
    # and the reference's wherever the reference's top two logits are further apart than both raw errors
    top = np.sort(c["raw"], 1)
    sure = top[:, -1] - top[:, -2] > 2 * br
    print(f"mlp {tag}: raw kernel {er:.2e} yardstick {np.abs(c['y_raw'] - c['raw']).max():.2e} bound {br:.2e} | "
          f"prob {ep:.2e} | rows inside the raw bound {(~sure).sum()} of {len(sure)}")
    assert er <= br
    assert ep <= br                      # softmax: sum_j |dp_i / dz_j| = 2 p_i (1 - p_i) <= 1 / 2
    assert (~sure).sum() <= 0.01 * len(sure) and np.array_equal(pred[sure], c["pred"][sure])
    np.testing.assert_allclose(prob.sum(1), 1.0, rtol=0, atol=1e-12)


def device_case(dev, c):
    return torch.tensor(c["X"], device=dev), torch.tensor(c["y"], device=dev)


@pytest.mark.parametrize("layers,n,slots,vw", SHAPES)
def test_device_matches_reference(gpu_device, layers, n, slots, vw):
    c = R.case(tuple(layers), n)
    Xd, yd = device_case(gpu_device, c)
    plan = K.mlp_plan(Xd, layers)
    assert (plan["path"], plan["slots"], plan["vw"]) == ("native", slots, vw), plan
    with Counting() as calls:
        loss, g = K.mlp_step(Xd, yd, c["theta"], layers, K.MLP_STEP)
        loss2, g2 = K.mlp_step(Xd, yd, c["theta"], layers, K.MLP_STEP)
        raw, prob, pred = K.mlp_step(Xd, None, c["theta"], layers, K.MLP_PREDICT)
    assert calls.count("cdna_mlp_step") == 3, calls
    # no float atomics: the same bits twice
    assert torch.equal(loss, loss2) and torch.equal(g, g2)
    assert g.dtype == raw.dtype == prob.dtype == torch.float64 and pred.dtype == torch.int32
    tag = f"{layers} n={n}"
    check_step(tag, c, loss.item(), g.cpu().numpy())
    check_predict(tag, c, raw.cpu().numpy(), prob.cpu().numpy(), pred.cpu().numpy())


def test_strided_misaligned_rows_take_the_scalar_loads(gpu_device):
    """X as a column slice of a wider tensor: odd row stride, pointer off 16-byte alignment."""
    layers, n = [100, 64, 32, 3], 1000
    c = R.case(tuple(layers), n)
    wide = torch.full((n, 103), float("nan"), device=gpu_device)
    Xs = wide[:, 1:101]
    Xs.copy_(torch.tensor(c["X"]))
    assert Xs.stride(0) == 103 and Xs.data_ptr() % 16 != 0
    plan = K.mlp_plan(Xs, layers)
    assert (plan["path"], plan["slots"], plan["vw"]) == ("native", 3, 1), plan
    yd = torch.tensor(c["y"], device=gpu_device)
    loss, g = K.mlp_step(Xs, yd, c["theta"], layers, K.MLP_STEP)
    raw, prob, pred = K.mlp_step(Xs, None, c["theta"], layers, K.MLP_PREDICT)
    check_step("strided", c, loss.item(), g.cpu().numpy())
    check_predict("strided", c, raw.cpu().numpy(), prob.cpu().numpy(), pred.cpu().numpy())


@pytest.mark.parametrize("layers,n", [([5, 4, 3], 65), ([100, 64, 32, 3], 1000)])
def test_rows_past_the_end_are_neither_read_nor_summed(gpu_device, layers, n):
    """The first n rows of a buffer whose other rows are NaN give the bits of a tight buffer."""
    c = R.case(tuple(layers), n)
    Xd, yd = device_case(gpu_device, c)
    big = torch.full((n + 200, layers[0]), float("nan"), device=gpu_device)
    big[:n] = Xd
    assert K.mlp_plan(big[:n], layers)["path"] == "native"
    a = K.mlp_step(Xd, yd, c["theta"], layers, K.MLP_STEP)
    b = K.mlp_step(big[:n], yd, c["theta"], layers, K.MLP_STEP)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(b[1]).all()
    pa = K.mlp_step(Xd, None, c["theta"], layers, K.MLP_PREDICT)
    pb = K.mlp_step(big[:n], None, c["theta"], layers, K.MLP_PREDICT)
    assert all(torch.equal(u, v) for u, v in zip(pa, pb))


def test_saturated_net_stays_finite(gpu_device):
    """Weights scaled until the hidden pre-activations reach +-80 and the logits +-1e4: the sigmoid and the softmax
    must not overflow.  The loss is within the usual bound of the reference, the gradient has no NaN."""
    layers, n = [20, 16, 3], 500
    X, y, theta = R.make_case(layers, n, seed=5)
    theta = theta.copy()
    theta[:20 * 16 + 16] *= 60.0                       # layer 0: z ~ N(0, 20^2) and beyond
    theta[20 * 16 + 16:] *= 4000.0                     # layer 1: logits of a few thousand
    theta = theta.astype(np.float32).astype(np.float64)
    acts, z = R.forward(X, theta, layers)
    z0 = acts[0] @ R.unpack(theta, layers)[0][0].T + R.unpack(theta, layers)[0][1]
    assert np.abs(z0).max() > 80 and np.abs(z).max() > 1e4
    c = dict(X=X, y=y, theta=theta)
    c["loss"], c["grad"] = R.step(X, y, theta, layers)
    c["raw"], c["prob"], c["pred"] = R.predict(X, theta, layers)
    c["y_loss"], c["y_grad"], c["y_raw"] = R.yardstick(X, y, theta, layers)
    assert np.isfinite(c["loss"]) and np.isfinite(c["y_loss"])
    Xd, yd = device_case(gpu_device, c)
    assert K.mlp_plan(Xd, layers)["path"] == "native"
    loss, g = K.mlp_step(Xd, yd, theta, layers, K.MLP_STEP)
    raw, prob, pred = K.mlp_step(Xd, None, theta, layers, K.MLP_PREDICT)
    bl = bounds(c)[0]
    print(f"mlp saturated: loss {loss.item():.6e} reference {c['loss']:.6e} kernel {abs(loss.item() - c['loss']):.2e} "
          f"yardstick {abs(c['y_loss'] - c['loss']):.2e} bound {bl:.2e}")
    assert np.isfinite(loss.item()) and abs(loss.item() - c["loss"]) <= bl
    assert not torch.isnan(g).any() and torch.isfinite(raw).all() and torch.isfinite(prob).all()
    assert np.array_equal(pred.cpu().numpy(), np.argmax(raw.cpu().numpy(), 1))


@pytest.mark.parametrize("layers,n", [([100, 64, 32, 3], 2500), ([33, 33, 2], 257)])
def test_poisoned_workspace(gpu_device, monkeypatch, layers, n):
    """The workspace arrives full of NaN with a NaN guard band behind it: everything the reduction reads has been
    written (the result is the unpoisoned call's, bit for bit) and nothing behind the workspace is."""
    c = R.case(tuple(layers), n)
    Xd, yd = device_case(gpu_device, c)
    plan = K.mlp_plan(Xd, layers)
    assert plan["path"] == "native"
    lay = np.asarray(layers, dtype=np.int32)
    ws_n = _lib.lib().cdna_mlp_step_workspace(n, lay.ctypes.data, len(lay))
    assert ws_n == plan["nblk"] * (plan["tiles"] * 1024 + K.MLP_MAX_LAYERS * K.MLP_MAX_WIDTH + 2)
    clean = K.mlp_step(Xd, yd, c["theta"], layers, K.MLP_STEP)
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
    out = K.mlp_step(Xd, yd, c["theta"], layers, K.MLP_STEP)
    monkeypatch.undo()
    assert len(poisoned) == 1
    assert torch.equal(out[0], clean[0]) and torch.equal(out[1], clean[1]) and torch.isfinite(out[1]).all()
    assert poisoned[0][ws_n:].isnan().all()


@pytest.mark.parametrize("layers,f64", [([K.MLP_MAX_WIDTH + 1, 4, 3], False), ([6, K.MLP_MAX_WIDTH + 1, 3], False),
                                        ([6, 5, 4, 3, 2], False), ([5, 4, 3], True)])
def test_outside_the_native_range_takes_the_host_formulation(gpu_device, layers, f64):
    assert max(layers) > K.MLP_MAX_WIDTH or len(layers) - 1 > K.MLP_MAX_LAYERS or f64
    n = 300
    X, y, theta = R.make_case(layers, n, dtype=np.float64 if f64 else np.float32)
    Xd, yd = torch.tensor(X, device=gpu_device), torch.tensor(y, device=gpu_device)
    assert K.mlp_plan(Xd, layers) == {"path": "host"}
    with Counting() as calls:
        loss, g = K.mlp_step(Xd, yd, theta, layers, K.MLP_STEP)
        raw, prob, pred = K.mlp_step(Xd, None, theta, layers, K.MLP_PREDICT)
    assert "cdna_mlp_step" not in calls, calls
    rl, rg = R.step(X, y, theta, layers)
    rr, rp, rd = R.predict(X, theta, layers)
    # fp64 on both sides: the order of the sums only (tests/test_mlp_cpu.py)
    assert abs(loss.item() - rl) <= 1e-12 * abs(rl)
    np.testing.assert_allclose(g.cpu().numpy(), rg, rtol=0, atol=1e-12 * np.abs(rg).max())
    np.testing.assert_allclose(raw.cpu().numpy(), rr, rtol=0, atol=1e-12 * np.abs(rr).max())
    np.testing.assert_allclose(prob.cpu().numpy(), rp, rtol=0, atol=1e-13)
    top = np.sort(rr, 1)
    sure = top[:, -1] - top[:, -2] > 1e-9
    assert np.array_equal(pred.cpu().numpy()[sure], rd[sure])


# ------------------------------------------------------------------------------------------------ end to end
def _fit(device, tmp_path, X, y, **kw):
    import cdnaml
    from cdnaml.ml.classification import MultilayerPerceptronClassifier
    from cdnaml.ml.evaluation import MulticlassClassificationEvaluator
    from cdnaml.ml.feature import VectorAssembler
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
                m = MultilayerPerceptronClassifier(**kw).fit(df)
                acc = MulticlassClassificationEvaluator(metricName="accuracy").evaluate(m.transform(df))
            out = (m.weights.toArray(), acc, m.summary.objectiveHistory, m.summary.totalIterations)
        finally:
            spark.conf.set("cdnaml.ml.vectorPrecision", "auto")
            spark.stop()
    return out, calls


def test_xor_fit_on_the_device(gpu_device, tmp_path):
    X, y = R.xor_data(400, seed=0)
    (theta, acc, hist, iters), calls = _fit("cuda", tmp_path, X, y, layers=[2, 8, 2], maxIter=100, seed=0)
    print(f"mlp xor on the device: accuracy {acc:.4f} after {iters} iterations, loss {hist[0]:.4f} -> {hist[-1]:.2e}")
    # every objective evaluation and the two transforms (summary, evaluation) ran the kernel
    assert calls.count("cdna_mlp_step") >= len(hist) + 2, calls
    assert acc >= 0.95


def test_one_iteration_on_the_device_matches_the_cpu_session(gpu_device, tmp_path):
    """maxIter = 1 from fixed initialWeights (fp32 values), fp32 feature vectors in both sessions: the CPU session
    evaluates the host formulation (fp64 at the same weights), so the two gradients g differ by the STEP error, at
    most eps = bound(un-normalised gradient) / n per entry.  The one iteration is theta1 = theta0 - alpha s g with
    s = min(1, 1 / |g|_2) and the same Armijo alpha = 2^-k <= 1 on both sides (asserted: the same history length and
    a first step accepted with margin).  For |g|_2 < 1: |d theta1| <= eps.  Else g / |g|_2 moves by at most
    2 |dg|_2 / |g|_2 <= 2 sqrt(P) eps.  The bound asserted is 2 sqrt(P) eps; nothing else differs."""
    layers, n = [10, 12, 3], 3000
    X, y, theta0 = R.make_case(layers, n, seed=3)
    y = y.astype(np.float64)
    kw = dict(layers=layers, maxIter=1, initialWeights=theta0)
    (tg, _, hg, ig), calls = _fit("cuda", tmp_path, X, y, **kw)
    (tc, _, hc, ic), _ = _fit("cpu", tmp_path, X, y, **kw)
    assert calls.count("cdna_mlp_step") >= 2 and len(hg) == len(hc) == 2 and ig == ic == 1
    c = R.case(tuple(layers), n, 3)
    assert np.array_equal(c["theta"], theta0)
    eps = bounds(c)[1] / n
    bound = 2 * np.sqrt(len(theta0)) * eps
    moved = np.abs(tc - theta0).max()
    print(f"mlp one iteration: |theta_gpu - theta_cpu| {np.abs(tg - tc).max():.2e} bound {bound:.2e} "
          f"(step {moved:.2e}), loss {hg[0]:.6f} -> {hg[1]:.6f} / {hc[1]:.6f}")
    assert hc[1] < hc[0] - 1e-3 * abs(hc[0])            # the Armijo decision is far from its threshold
    assert moved > 100 * bound and np.abs(tg - tc).max() <= bound
