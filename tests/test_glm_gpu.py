"""K22 ``glm_step`` on the device against the op's host formulation on the same fp32 inputs, and a GLM fitted
end to end on the GPU against the CPU fit.

Shapes are the smallest at which the kernel can go wrong: a single row, the 64-row tile edge with d % 4 != 0 (the
scalar-load variant), one feature, the benchmark's d = 100, the d + 2 = 128 cap with many blocks and a ragged last
tile, one past the cap (the composition through K1, no K22 launch), strided rows, zero weights with an offset, a
65..96-wide Gram (two tile pairs per wave) with either kind of load.

Tolerances: G to rtol 1e-5 and atol 1e-3 sqrt(n) max(W) (test_gram_f32's bound for the exact-fp32 MFMA with fp32
block accumulation; the weight's factor follows from linearity); the fp64 scalars to rtol 1e-10 (fp64 exp / log
differ by a few ulp between the device and the host library, two orders of slack; the data keeps mu away from y).
"""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import _lib, kernels as K
from tests.conftest import session_device

pytestmark = pytest.mark.gpu

PAIRS = [("poisson", "log"), ("binomial", "logit"), ("gamma", "inverse")]
# (n, d, ldx or None, zero weights + offset)
SHAPES = [(1, 4, None, False), (63, 3, None, False), (64, 3, None, False), (65, 3, None, False),
          (200, 1, None, False), (5000, 100, None, False), (70001, 126, None, False), (3000, 127, None, False),
          (9000, 100, 101, False), (4096, 30, None, True),
          # float4-load variant with 3 tile pairs (one per wave), at the widest d % 4 == 0, and with a row stride
          (4097, 60, None, False), (20000, 124, None, True), (5000, 100, 104, False),
          # 65 <= d + 2 <= 96: 6 tile pairs, two per wave; float4 loads and a ragged last tile, then scalar loads
          (4097, 64, None, False), (1500, 66, None, True)]


@functools.lru_cache(maxsize=None)
def inputs(n, d, ldx, degenerate, fam, link):
    """CPU inputs with W = O(1): |x.beta| <~ 0.5 around an intercept inside the link's domain."""
    rng = np.random.default_rng(1000 * d + n % 997)
    X = torch.tensor(rng.uniform(-1, 1, (n, ldx or d)), dtype=torch.float32)[:, :d]
    beta = rng.uniform(-1, 1, d) * 0.5 / np.sqrt(d)
    b0 = {"log": 0.3, "logit": 0.1, "inverse": 1.0}[link]
    eta = b0 + X.double().numpy() @ beta
    mu = {"log": np.exp, "logit": lambda e: 1 / (1 + np.exp(-e)), "inverse": lambda e: 1 / e}[link](eta)
    if fam == "poisson":
        y = rng.poisson(mu).astype(float)
    elif fam == "binomial":
        y = (rng.uniform(size=n) < mu).astype(float)
    else:
        y = rng.gamma(5.0, mu / 5.0)
    w = off = None
    if degenerate:
        w = rng.uniform(0.5, 2.0, n)
        w[rng.uniform(size=n) < 0.1] = 0.0
        off = rng.uniform(-0.1, 0.1, n)
    shift = X[:4096].double().mean(0).float()
    t = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)  # noqa: E731
    return X, t(y), t(w), t(off), t(beta), b0, shift, b0 + 0.05


@functools.lru_cache(maxsize=None)
def host_step(n, d, ldx, degenerate, fam, link, mode):
    """The host formulation on the CPU copies (the oracle), and max(W) for the tolerance."""
    X, y, w, off, beta, b0, shift, zs = inputs(n, d, ldx, degenerate, fam, link)
    G, st = K.glm_step(X, y, w, off, beta, b0, shift, zs, fam, link, 0.0, 0.0, mode)
    ww = torch.ones_like(y) if w is None else w
    oo = torch.zeros_like(y) if off is None else off
    W = K.glm_row_terms(y, ww, oo, b0 + X.double() @ beta, fam, link, 0.0, 0.0, mode)[2]
    return G, st, float(W.max())


def device_step(dev, n, d, ldx, degenerate, fam, link, mode):
    X, y, w, off, beta, b0, shift, zs = inputs(n, d, ldx, degenerate, fam, link)
    g = lambda a: None if a is None else a.to(dev)  # noqa: E731
    Xd = torch.empty((n, ldx or d), dtype=torch.float32, device=dev)[:, :d]   # keeps the row stride on the device
    Xd.copy_(X)
    calls = []
    orig = _lib.check

    def counting(code, name):
        calls.append(name)
        return orig(code, name)
    _lib.check = counting
    try:
        G, st = K.glm_step(Xd, g(y), g(w), g(off), g(beta), b0, g(shift), zs, fam, link, 0.0, 0.0, mode)
        G2, st2 = K.glm_step(Xd, g(y), g(w), g(off), g(beta), b0, g(shift), zs, fam, link, 0.0, 0.0, mode)
    finally:
        _lib.check = orig
    if d <= K.GLM_MAX_D:    # K22 has no float atomics: the same bits twice (past the cap: a composition of torch ops and K1)
        assert torch.equal(G, G2)
    assert torch.equal(st, st2)
    return G.cpu(), st.cpu(), calls


def check_step(dev, n, d, ldx, degenerate, fam, link, mode):
    G, st, calls = device_step(dev, n, d, ldx, degenerate, fam, link, mode)
    Gh, sth, wmax = host_step(n, d, ldx, degenerate, fam, link, mode)
    if d <= K.GLM_MAX_D:
        assert calls == ["cdna_glm_step"] * 2, calls
    else:                                                       # past the cap: the composition through K1
        assert "cdna_glm_step" not in calls and "cdna_gram" in calls, calls
    assert st[3].item() == 0 and sth[3].item() == 0
    np.testing.assert_allclose(st.numpy(), sth.numpy(), rtol=1e-10, atol=0)
    if mode == K.GLM_EVAL:
        assert not G.any()
    else:
        np.testing.assert_allclose(G.numpy(), Gh.numpy(), rtol=1e-5, atol=1e-3 * np.sqrt(n) * wmax)
        assert torch.equal(G, G.T)


@pytest.mark.parametrize("fam,link", PAIRS)
@pytest.mark.parametrize("n,d,ldx,degenerate", SHAPES)
def test_device_step_matches_host(gpu_device, n, d, ldx, degenerate, fam, link):
    check_step(gpu_device, n, d, ldx, degenerate, fam, link, K.GLM_STEP)


@pytest.mark.parametrize("fam,link", PAIRS)
@pytest.mark.parametrize("mode", [K.GLM_INIT, K.GLM_EVAL])
def test_device_step_modes(gpu_device, fam, link, mode):
    check_step(gpu_device, 5000, 100, None, False, fam, link, mode)   # GLM_STEP at this shape: the test above


def test_device_counts_non_finite_rows(gpu_device):
    n, d = 300, 4
    X, y, w, off, beta, b0, shift, zs = inputs(n, d, None, False, "poisson", "log")
    X = X.clone()
    X[7] = 800.0 / float(beta.sum()) if abs(float(beta.sum())) > 1e-3 else 0.0   # eta ~ 800: exp overflows
    X[200] = float("inf")     # a non-finite feature: counted, and zeroed in the tile, not scaled by 0 into NaN
    args = (b0, shift, zs, "poisson", "log", 0.0, 0.0, K.GLM_STEP)
    Gh, sth = K.glm_step(X, y, None, None, beta, *args)
    G, st = K.glm_step(X.to(gpu_device), y.to(gpu_device), None, None, beta.to(gpu_device), b0,
                       shift.to(gpu_device), *args[2:])
    assert sth[3].item() == 2 and st[3].item() == 2
    assert torch.isfinite(G).all()
    np.testing.assert_allclose(st.cpu().numpy(), sth.numpy(), rtol=1e-10)
    np.testing.assert_allclose(G.cpu().numpy(), Gh.numpy(), rtol=1e-5, atol=1e-3 * np.sqrt(n) * 3.0)


# ------------------------------------------------------------------------------------------------ end to end
# Largest relative coefficient difference of the device fit against the fp64 reference IRLS on the same
# fp32-rounded data, as measured on an MI355X (profiles/r8/glm.md); the bound is 4x that (accumulation order
# across seeds), and never looser than the project's fp32 cross-device coefficient bound of 1e-4.
MEASURED_COEF_GAP = {"poisson": 3.254e-7, "gamma": 2.193e-7}


def _fit(device, tmp_path, pdf, names, fam):
    import cdnaml
    from cdnaml.ml.feature import VectorAssembler
    from cdnaml.ml.regression import GeneralizedLinearRegression
    with session_device(device):
        spark = cdnaml.SparkSession.builder.config("cdnaml.warehouse.dir", str(tmp_path / f"wh_{device}")) \
            .getOrCreate()
        spark.conf.set("cdnaml.ml.vectorPrecision", "fp32")
        calls = []
        orig = _lib.check

        def counting(code, name):
            calls.append(name)
            return orig(code, name)
        _lib.check = counting
        try:
            df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))
            m = GeneralizedLinearRegression(family=fam, link="log").fit(df)
            out = (np.r_[m.coefficients.toArray(), m.intercept], m.summary.numIterations, m.summary.deviance)
        finally:
            _lib.check = orig
            spark.conf.set("cdnaml.ml.vectorPrecision", "auto")
            spark.stop()
    return out, calls


@pytest.mark.parametrize("fam", ["poisson", "gamma"])
def test_fit_on_device_matches_cpu(gpu_device, tmp_path, fam):
    from tests.test_glm_cpu import ref_irls
    n, d = 20000, 20
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (n, d)).astype(np.float32).astype(np.float64)
    mu = np.exp(0.5 + X @ rng.uniform(-0.3, 0.3, d))
    y = rng.poisson(mu).astype(float) if fam == "poisson" else rng.gamma(5.0, mu / 5.0)
    names = [f"x{i}" for i in range(d)]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"] = y
    (cg, ig, dg), calls = _fit("cuda", tmp_path, pdf, names, fam)
    (cc, ic, dc), _ = _fit("cpu", tmp_path, pdf, names, fam)
    assert calls.count("cdna_glm_step") == ig + 2, calls       # INIT, one per iteration, EVAL
    assert abs(ig - ic) <= 1, (ig, ic)
    ref = ref_irls(X, y, None, None, fam, "log", 0.0, 0.0, True, 0.0, 1e-12, 100)[0]
    scale = np.abs(ref).max()
    gap_ref, gap_cpu = np.abs(cg - ref).max() / scale, np.abs(cg - cc).max() / scale
    print(f"glm e2e {fam}: device vs fp64 reference {gap_ref:.3e}, device vs cpu fit {gap_cpu:.3e}, "
          f"iterations {ig} / {ic}, deviance {dg!r} / {dc!r}")
    bound = min(4.0 * MEASURED_COEF_GAP[fam], 1e-4)
    assert gap_cpu <= bound and gap_ref <= bound, (gap_cpu, gap_ref, bound)
    assert abs(dg - dc) <= 1e-6 * abs(dc), (dg, dc)
