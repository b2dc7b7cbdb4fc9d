"""GeneralizedLinearRegression (pyspark.ml.regression) and the K22 ``glm_step`` op's host formulation.

* the host formulation of one IRLS step (INIT / STEP / EVAL) against a numpy reference written here, family and
  link one at a time;
* fitted models against a textbook fp64 IRLS written here (relative 1e-8), against scikit-learn's GLMs where the
  penalty is zero, and against the score equations;
* the summary's fields against the same reference; cross-checks with LinearRegression and LogisticRegression;
* validation, linkPredictionCol, persistence, the pyspark alias, and shard additivity of the step.

The Gram and the scalars of a step are compared element by element at a plain relative tolerance (1e-12 against
the numpy reference, 1e-13 for the shard sums), with no absolute term: an entry that is exactly zero on one side
(a single row equal to its own shift) is exactly zero on the other.  The score equations, a sum of signed terms
that is zero at the fit, are bounded relative to the sum of the terms' magnitudes.
"""
import numpy as np
import pandas as pd
import pytest
import scipy.special as sps
import scipy.stats as sst
import torch

from cdnaml.ops import kernels as K

EPS = 1e-16

# ------------------------------------------------------------------------------------------- numpy reference
LINK = {
    "identity": (lambda m: m, lambda e: e, lambda m: np.ones_like(m)),
    "log": (np.log, np.exp, lambda m: 1 / m),
    "inverse": (lambda m: 1 / m, lambda e: 1 / e, lambda m: -1 / m ** 2),
    "logit": (lambda m: np.log(m / (1 - m)), lambda e: 1 / (1 + np.exp(-e)), lambda m: 1 / (m * (1 - m))),
    "probit": (sps.ndtri, sps.ndtr, lambda m: np.sqrt(2 * np.pi) * np.exp(0.5 * sps.ndtri(m) ** 2)),
    "cloglog": (lambda m: np.log(-np.log(1 - m)), lambda e: 1 - np.exp(-np.exp(e)),
                lambda m: 1 / ((m - 1) * np.log(1 - m))),
    "sqrt": (np.sqrt, lambda e: e * e, lambda m: 0.5 / np.sqrt(m)),
}


def link_fns(link, lp):
    if link == "power":
        return (lambda m: m ** lp, lambda e: e ** (1 / lp), lambda m: lp * m ** (lp - 1))
    return LINK[link]


def variance(fam, mu, vp):
    return {"gaussian": np.ones_like(mu), "binomial": mu * (1 - mu), "poisson": mu, "gamma": mu * mu,
            "tweedie": mu ** vp}[fam]


def clamp(fam, mu):
    if fam == "binomial":
        return np.minimum(np.maximum(mu, EPS), 1 - EPS)
    return mu if fam == "gaussian" else np.maximum(mu, EPS)


def ylogy(y, mu):
    return np.where(y == 0, 0.0, y * np.log(np.where(y == 0, 1.0, y) / mu))


def unit_dev(fam, y, mu, vp):
    if fam == "gaussian":
        return (y - mu) ** 2
    if fam == "binomial":
        return 2 * (ylogy(y, mu) + ylogy(1 - y, 1 - mu))
    if fam == "poisson":
        return 2 * (ylogy(y, mu) - (y - mu))
    if fam == "gamma":
        return -2 * (np.log(y / mu) - (y - mu) / mu)
    y1 = np.maximum(y, 0.1) if 1 <= vp < 2 else y

    def yp(a, b, p):
        return np.log(a / b) if p == 0 else (a ** p - b ** p) / p
    return 2 * (y * yp(y1, mu, 1 - vp) - yp(y, mu, 2 - vp))


def init_mu(fam, y, w):
    if fam == "binomial":
        return (w * y + 0.5) / (w + 1)
    return np.maximum(y, 0.1) if fam in ("poisson", "tweedie") else y


def ref_rows(X, y, w, off, beta, b, fam, link, vp, lp, mode):
    g, ginv, gp_ = link_fns(link, lp)
    if mode == K.GLM_INIT:
        mu = clamp(fam, init_mu(fam, y, w))
        eta = g(mu)
    else:
        eta = off + b + X @ beta
        mu = clamp(fam, ginv(eta))
    gp = gp_(mu)
    return eta, mu, w / (variance(fam, mu, vp) * gp * gp), eta - off + (y - mu) * gp


def ref_step(X, y, w, off, beta, b, shift, zshift, fam, link, vp, lp, mode):
    """(G, stats) of the step, all numpy fp64."""
    n, d = X.shape
    w = np.ones(n) if w is None else w
    off = np.zeros(n) if off is None else off
    _, mu, W, z = ref_rows(X, y, w, off, beta, b, fam, link, vp, lp, mode)
    A = np.sqrt(W)[:, None] * np.c_[X - shift, np.ones(n), z - np.float32(zshift)]
    return A.T @ A, np.array([(w * unit_dev(fam, y, mu, vp)).sum(), w.sum(), (w * y).sum(), 0.0])


# (family, link, variancePower, linkPower): every pair Spark accepts, and two tweedie settings
PAIRS = [("gaussian", "identity", 0, 0), ("gaussian", "log", 0, 0), ("gaussian", "inverse", 0, 0),
         ("binomial", "logit", 0, 0), ("binomial", "probit", 0, 0), ("binomial", "cloglog", 0, 0),
         ("poisson", "log", 0, 0), ("poisson", "identity", 0, 0), ("poisson", "sqrt", 0, 0),
         ("gamma", "inverse", 0, 0), ("gamma", "identity", 0, 0), ("gamma", "log", 0, 0),
         ("tweedie", "log", 1.5, 0.0), ("tweedie", "power", 1.5, -0.5), ("tweedie", "power", 2.5, 0.3)]


def make_data(fam, link, lp, n, d, seed, vp=0.0, b0=None):
    """Features, a coefficient vector whose linear predictor sits inside every link's domain, and labels."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, d))
    beta = rng.uniform(-0.3, 0.3, d)
    if b0 is None:
        b0 = 0.2 if fam == "binomial" else 1.2     # eta in (0.3, 2.1): positive for inverse / sqrt / power links
    eta = b0 + X @ beta
    mu = link_fns(link, lp)[1](eta)
    if fam == "gaussian":
        y = mu + 0.1 * rng.normal(size=n)
    elif fam == "binomial":
        y = (rng.uniform(size=n) < mu).astype(float)
    elif fam == "poisson":
        y = rng.poisson(mu).astype(float)
    elif fam == "gamma":
        y = rng.gamma(5.0, mu / 5.0)
    else:
        y = mu * rng.gamma(2.0, 0.5, n)
        if vp < 2:
            y[rng.uniform(size=n) < 0.1] = 0.0
    return X, y, beta, b0


def T64(a):
    return None if a is None else torch.tensor(np.asarray(a, dtype=np.float64))


# ----------------------------------------------------------------------------------------- the step, on the host
@pytest.mark.parametrize("fam,link,vp,lp", PAIRS)
@pytest.mark.parametrize("mode", [K.GLM_INIT, K.GLM_STEP, K.GLM_EVAL])
@pytest.mark.parametrize("variant", ["plain", "w_off", "no_shift", "zero_w", "n1"])
def test_host_step_matches_numpy(fam, link, vp, lp, mode, variant):
    n, d = (1 if variant == "n1" else 57), 3
    X, y, beta, b0 = make_data(fam, link, lp, n, d, 7, vp)
    rng = np.random.default_rng(3)
    w = off = None
    if variant in ("w_off", "zero_w"):
        w = rng.uniform(0.5, 2.0, n)
        off = rng.uniform(-0.05, 0.05, n)
    if variant == "zero_w":
        w[::5] = 0.0
    shift = np.zeros(d) if variant == "no_shift" else X[: max(n // 2, 1)].mean(0).astype(np.float32).astype(float)
    b = 0.0 if variant == "no_shift" else b0
    if variant == "no_shift":                       # no intercept: keep eta in the links' domain through an offset
        off = np.full(n, b0)
    zshift = 0.0 if variant == "no_shift" else 0.7
    G, stats = K.glm_step(T64(X), T64(y), T64(w), T64(off), T64(beta), b, None if variant == "no_shift"
                          else T64(shift).float(), zshift, fam, link, vp, lp, mode)
    Gr, sr = ref_step(X, y, w, off, beta, b, shift, zshift, fam, link, vp, lp, mode)
    assert stats[3].item() == 0
    np.testing.assert_allclose(stats[:3].numpy(), sr[:3], rtol=1e-12, atol=0)
    if mode == K.GLM_EVAL:
        assert not G.any()
    else:
        np.testing.assert_allclose(G.numpy(), Gr, rtol=1e-12, atol=0)


def test_step_counts_non_finite_rows():
    X = torch.tensor([[1.0], [1.0], [800.0]], dtype=torch.float64)
    y = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    G, st = K.glm_step(X, y, None, None, torch.ones(1, dtype=torch.float64), 0.0, None, 0.0, "poisson", "log")
    assert st[3].item() == 1 and torch.isfinite(G).all() and st[1].item() == 2.0   # exp(800) overflows: 1 row out
    # a non-finite feature makes eta non-finite: the row is counted and zeroed, not scaled by 0 into NaN
    for bad in (float("inf"), float("nan")):
        for dt in (torch.float64, torch.float32):
            Xb = torch.tensor([[1.0], [1.0], [bad]], dtype=dt)
            Gb, sb = K.glm_step(Xb, y, None, None, torch.ones(1, dtype=torch.float64), 0.0,
                                torch.tensor([0.5]), 0.0, "poisson", "log")
            G2, s2 = K.glm_step(Xb[:2], y[:2], None, None, torch.ones(1, dtype=torch.float64), 0.0,
                                torch.tensor([0.5]), 0.0, "poisson", "log")
            assert sb[3].item() == 1 and torch.equal(Gb, G2) and torch.equal(sb[:3], s2[:3])


@pytest.mark.parametrize("fam,link,vp,lp", [("poisson", "log", 0, 0), ("binomial", "logit", 0, 0),
                                            ("gamma", "inverse", 0, 0), ("tweedie", "log", 1.5, 0.0)])
@pytest.mark.parametrize("mode", [K.GLM_INIT, K.GLM_STEP, K.GLM_EVAL])
def test_shard_additivity(fam, link, vp, lp, mode):
    """glm_step on the two halves of a table sums to the call on the whole table (what the all-reduce relies on)."""
    n, d = 401, 5
    X, y, beta, b0 = make_data(fam, link, lp, n, d, 11, vp)
    w = np.random.default_rng(5).uniform(0.5, 2.0, n)
    shift = X[:64].mean(0).astype(np.float32)
    args = (T64(beta), b0, torch.tensor(shift), 0.4, fam, link, vp, lp, mode)
    G, st = K.glm_step(T64(X), T64(y), T64(w), None, *args)
    h = 200
    Ga, sa = K.glm_step(T64(X[:h]), T64(y[:h]), T64(w[:h]), None, *args)
    Gb, sb = K.glm_step(T64(X[h:]), T64(y[h:]), T64(w[h:]), None, *args)
    np.testing.assert_allclose((Ga + Gb).numpy(), G.numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose((sa + sb).numpy(), st.numpy(), rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------------ models
def ref_wls(A, W, z, fit_int, lam):
    """The weighted least squares of one IRLS iteration; lam > 0: the L2 penalty of the standardised normal-
    equation solver (features and response scaled by their weighted standard deviations)."""
    if lam == 0.0:
        M = A.T @ (A * W[:, None])
        return np.linalg.solve(M, A.T @ (W * z)), M
    assert fit_int
    Xf = A[:, :-1]
    n = W.sum()
    mx, mz = (W[:, None] * Xf).sum(0) / n, (W * z).sum() / n
    Xc, zc = Xf - mx, z - mz
    Cxx, Cxz = Xc.T @ (Xc * W[:, None]), Xc.T @ (W * zc)
    sdx2, sdz = np.diag(Cxx) / n, np.sqrt((W * zc * zc).sum() / n)
    coef = np.linalg.solve(Cxx + np.diag(n * lam / sdz * sdx2), Cxz)
    return np.r_[coef, mz - coef @ mx], None


def ref_irls(X, y, w, off, fam, link, vp, lp, fit_int=True, lam=0.0, tol=1e-10, max_iter=50):
    """Textbook IRLS in fp64 with the estimator's start and stopping rule; returns (coefficients with the
    intercept last when fitted, iterations, the last X^T W X)."""
    n, d = X.shape
    w = np.ones(n) if w is None else w
    off = np.zeros(n) if off is None else off
    A = np.c_[X, np.ones(n)] if fit_int else X
    _, _, W, z = ref_rows(X, y, w, off, None, 0.0, fam, link, vp, lp, K.GLM_INIT)
    beta, M = ref_wls(A, W, z, fit_int, lam)
    it = 0
    if (fam, link) != ("gaussian", "identity"):
        while it < max_iter:
            _, _, W, z = ref_rows(A, y, w, off, beta, 0.0, fam, link, vp, lp, K.GLM_STEP)
            nb, M = ref_wls(A, W, z, fit_int, lam)
            it += 1
            delta = np.abs(nb - beta).max()
            beta = nb
            if delta < tol:
                break
    return beta, it, M


def frame(spark, X, y, w=None, off=None):
    from cdnaml.ml.feature import VectorAssembler
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"] = y
    if w is not None:
        pdf["w"] = w
    if off is not None:
        pdf["off"] = off
    return VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))


def fit(spark, X, y, w=None, off=None, **kw):
    from cdnaml.ml.regression import GeneralizedLinearRegression
    kw.setdefault("tol", 1e-10)
    kw.setdefault("maxIter", 50)
    est = GeneralizedLinearRegression(weightCol="w" if w is not None else None,
                                      offsetCol="off" if off is not None else None, **kw)
    df = frame(spark, X, y, w, off)
    return est.fit(df), df


def est_kw(fam, link, vp, lp):
    if fam == "tweedie":
        return dict(family="tweedie", variancePower=vp, linkPower=lp)
    return dict(family=fam, link=link)


def got_vec(m, fit_int=True):
    return np.r_[m.coefficients.toArray(), m.intercept] if fit_int else m.coefficients.toArray()


N, D = 2000, 6
# each family with its canonical link and one other; then weights, an exposure offset, no intercept, a penalty
CASES = {
    "gaussian-identity": ("gaussian", "identity", 0, 0, {}),
    "gaussian-log": ("gaussian", "log", 0, 0, {}),
    "binomial-logit": ("binomial", "logit", 0, 0, {}),
    "binomial-probit": ("binomial", "probit", 0, 0, {}),
    "poisson-log": ("poisson", "log", 0, 0, {}),
    "poisson-sqrt": ("poisson", "sqrt", 0, 0, {}),
    "gamma-inverse": ("gamma", "inverse", 0, 0, {}),
    "gamma-log": ("gamma", "log", 0, 0, {}),
    "tweedie-canonical": ("tweedie", "power", 1.5, -0.5, {}),
    "tweedie-log": ("tweedie", "log", 1.5, 0.0, {}),
    "poisson-weights": ("poisson", "log", 0, 0, {"w": True}),
    "poisson-exposure": ("poisson", "log", 0, 0, {"off": True}),
    "gamma-log-weights-no-intercept": ("gamma", "log", 0, 0, {"w": True, "fit_int": False}),
    "poisson-ridge": ("poisson", "log", 0, 0, {"lam": 0.05}),
    "gamma-log-ridge-weights": ("gamma", "log", 0, 0, {"lam": 0.1, "w": True}),
}


def case_data(name):
    fam, link, vp, lp, opt = CASES[name]
    # a model without an intercept gets data without one (plain Fisher scoring diverges on the misspecified fit)
    X, y, _, _ = make_data(fam, link, lp, N, D, 2024, vp, None if opt.get("fit_int", True) else 0.0)
    rng = np.random.default_rng(99)
    w = rng.uniform(0.5, 2.0, N) if opt.get("w") else None
    off = None
    if opt.get("off"):                          # a Poisson exposure: counts drawn at rate exposure * mu
        expo = rng.uniform(0.5, 3.0, N)
        off = np.log(expo)
        y = rng.poisson(expo * np.maximum(y, 0.2)).astype(float)
    return fam, link, vp, lp, X, y, w, off, opt.get("fit_int", True), opt.get("lam", 0.0)


@pytest.mark.parametrize("name", list(CASES))
def test_model_matches_reference_irls(spark, name):
    fam, link, vp, lp, X, y, w, off, fit_int, lam = case_data(name)
    m, _ = fit(spark, X, y, w, off, fitIntercept=fit_int, regParam=lam, **est_kw(fam, link, vp, lp))
    ref, it, _ = ref_irls(X, y, w, off, fam, link, vp, lp, fit_int, lam)
    got = got_vec(m, fit_int)
    rel = np.abs(got - ref).max() / np.abs(ref).max()
    assert rel <= 1e-8, rel
    assert m.summary.numIterations == it and m.numFeatures == D
    if lam == 0.0:
        # score equations, reference-free: X^T [w (y - mu) / (V(mu) g'(mu))] = 0 at the fit
        A = np.c_[X, np.ones(N)] if fit_int else X
        ww = np.ones(N) if w is None else w
        oo = np.zeros(N) if off is None else off
        mu = clamp(fam, link_fns(link, lp)[1](oo + A @ got))
        t = ww * (y - mu) / (variance(fam, mu, vp) * link_fns(link, lp)[2](mu))
        score, mag = np.abs(A.T @ t), np.abs(A).T @ np.abs(t)
        assert (score <= 1e-8 * mag).all(), (score / mag).max()


def test_matches_sklearn(spark):
    """regParam = 0 against scikit-learn's GLMs (alpha = 0, Newton solver at tol 1e-12): 1e-7 absolute."""
    from sklearn.linear_model import GammaRegressor, LogisticRegression, PoissonRegressor, TweedieRegressor
    w = np.random.default_rng(1).uniform(0.5, 2.0, N)
    for name, sk in [("poisson-log", PoissonRegressor(alpha=0, solver="newton-cholesky", tol=1e-12, max_iter=1000)),
                     ("gamma-log", GammaRegressor(alpha=0, solver="newton-cholesky", tol=1e-12, max_iter=1000)),
                     ("tweedie-log", TweedieRegressor(power=1.5, link="log", alpha=0, solver="newton-cholesky",
                                                      tol=1e-12, max_iter=1000)),
                     ("binomial-logit", LogisticRegression(penalty=None, solver="newton-cholesky", tol=1e-12,
                                                           max_iter=1000))]:
        fam, link, vp, lp, X, y, _, _, _, _ = case_data(name)
        m, _ = fit(spark, X, y, w, **est_kw(fam, link, vp, lp))
        sk.fit(X, y, sample_weight=w)
        ref = np.r_[np.ravel(sk.coef_), np.ravel(sk.intercept_)]
        np.testing.assert_allclose(got_vec(m), ref, rtol=0, atol=1e-7, err_msg=name)


def ref_summary(fam, link, vp, lp, X, y, w, off, beta, M, fit_int=True):
    n = len(y)
    w = np.ones(n) if w is None else w
    oo = np.zeros(n) if off is None else off
    A = np.c_[X, np.ones(n)] if fit_int else X
    g, ginv, gp_ = link_fns(link, lp)
    mu = clamp(fam, ginv(oo + A @ beta))
    dev = (w * unit_dev(fam, y, mu, vp)).sum()
    rank = A.shape[1]
    dof = n - rank
    pear = (y - mu) * np.sqrt(w) / np.sqrt(variance(fam, mu, vp))
    disp = 1.0 if fam in ("binomial", "poisson") else (pear ** 2).sum() / dof
    if not fit_int:
        b_null = 0.0
    elif off is None:
        b_null = g((w * y).sum() / w.sum())
    else:
        b_null = ref_irls(np.zeros((n, 0)), y, w, off, fam, link, vp, lp, True, 0.0, 1e-13, 100)[0][0]
    null = (w * unit_dev(fam, y, clamp(fam, ginv(oo + b_null)), vp)).sum()
    if fam == "gaussian":
        ll = n * (np.log(dev / n * 2 * np.pi) + 1) + 2 - np.log(w).sum()
    elif fam == "binomial":
        ll = -2 * sst.binom.logpmf(np.round(y * w), np.round(w), mu).sum()
    elif fam == "poisson":
        ll = -2 * (w * sst.poisson.logpmf(y, mu)).sum()
    elif fam == "gamma":
        dd = dev / w.sum()
        ll = -2 * (w * sst.gamma.logpdf(y, 1 / dd, scale=mu * dd)).sum() + 2
    else:
        ll = np.nan
    se = np.sqrt(disp * np.diag(np.linalg.inv(M)))
    tv = beta / se
    pv = 2 * sst.norm.sf(np.abs(tv)) if fam in ("binomial", "poisson") else 2 * sst.t.sf(np.abs(tv), dof)
    res = {"deviance": np.sign(y - mu) * np.sqrt(np.maximum(w * unit_dev(fam, y, mu, vp), 0)), "pearson": pear,
           "working": (y - mu) * gp_(mu), "response": y - mu}
    return dict(deviance=dev, nullDeviance=null, dispersion=disp, aic=ll + 2 * rank, se=se, t=tv, p=pv, res=res,
                rank=rank, dof=dof)


@pytest.mark.parametrize("name", ["gaussian-identity", "binomial-logit", "poisson-weights", "poisson-exposure",
                                  "gamma-log", "gamma-log-weights-no-intercept", "tweedie-log"])
def test_summary_fields(spark, name):
    fam, link, vp, lp, X, y, w, off, fit_int, lam = case_data(name)
    m, df = fit(spark, X, y, w, off, fitIntercept=fit_int, **est_kw(fam, link, vp, lp))
    beta, it, M = ref_irls(X, y, w, off, fam, link, vp, lp, fit_int)
    r = ref_summary(fam, link, vp, lp, X, y, w, off, beta, M, fit_int)
    s = m.summary
    tol = dict(rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(s.deviance, r["deviance"], **tol)
    np.testing.assert_allclose(s.nullDeviance, r["nullDeviance"], **tol)
    np.testing.assert_allclose(s.dispersion, r["dispersion"], **tol)
    assert (s.rank, s.degreesOfFreedom, s.residualDegreeOfFreedom, s.numInstances) == (r["rank"], r["dof"],
                                                                                       r["dof"], N)
    assert s.residualDegreeOfFreedomNull == N - (1 if fit_int else 0) and s.numIterations == it
    if fam == "tweedie":
        with pytest.raises(RuntimeError):
            s.aic
    else:
        np.testing.assert_allclose(s.aic, r["aic"], **tol)
    np.testing.assert_allclose(s.coefficientStandardErrors, r["se"], **tol)
    np.testing.assert_allclose(s.tValues, r["t"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(s.pValues, r["p"], rtol=1e-6, atol=1e-300)
    for kind, want in r["res"].items():
        got = s.residuals(kind).toPandas()[kind + "Residuals"].to_numpy()
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-9, err_msg=kind)
    assert s.predictions.count() == N
    # evaluate(): the same statistics without the training fields
    e = m.evaluate(df)
    np.testing.assert_allclose([e.deviance, e.nullDeviance, e.dispersion], [s.deviance, s.nullDeviance, s.dispersion],
                               rtol=1e-12)
    assert not hasattr(e, "numIterations") and not hasattr(e, "coefficientStandardErrors")


def test_no_standard_errors_with_penalty(spark):
    fam, link, vp, lp, X, y, w, off, fit_int, lam = case_data("poisson-ridge")
    m, _ = fit(spark, X, y, regParam=lam, family="poisson")
    with pytest.raises(RuntimeError):
        m.summary.coefficientStandardErrors


def test_gaussian_identity_is_linear_regression(spark):
    from cdnaml.ml.regression import LinearRegression
    fam, link, vp, lp, X, y, *_ = case_data("gaussian-identity")
    m, df = fit(spark, X, y, family="gaussian")
    lr = LinearRegression().fit(df)
    np.testing.assert_allclose(got_vec(m), got_vec(lr), rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(m.summary.coefficientStandardErrors, lr.summary.coefficientStandardErrors, rtol=1e-8)
    assert m.summary.numIterations == 0


def test_binomial_logit_is_logistic_regression(spark):
    from cdnaml.ml.classification import LogisticRegression
    fam, link, vp, lp, X, y, *_ = case_data("binomial-logit")
    m, df = fit(spark, X, y, family="binomial")
    lo = LogisticRegression(regParam=0.0, tol=1e-12, maxIter=500).fit(df)
    np.testing.assert_allclose(got_vec(m), np.r_[lo.coefficients.toArray(), lo.intercept], rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------- other behaviour
def test_validation(spark):
    from cdnaml.ml.regression import GeneralizedLinearRegression as GLR
    from cdnaml.models.util import IllegalArgumentException as IAE
    X, y, _, _ = make_data("poisson", "log", 0, 40, 2, 0)
    for fam, link in [("gaussian", "logit"), ("binomial", "log"), ("poisson", "inverse"), ("gamma", "sqrt"),
                      ("poisson", "nope")]:
        with pytest.raises(IAE):
            GLR(family=fam, link=link).fit(frame(spark, X, y))
    with pytest.raises(IAE):
        GLR(family="cauchy").fit(frame(spark, X, y))
    with pytest.raises(IAE):
        GLR(family="tweedie", variancePower=0.5).fit(frame(spark, X, y))
    with pytest.raises(IAE):
        GLR(family="binomial").fit(frame(spark, X, y + 2.0))          # outside [0, 1]
    with pytest.raises(IAE):
        GLR(family="poisson").fit(frame(spark, X, y - 5.0))           # negative counts
    with pytest.raises(IAE):
        GLR(family="gamma").fit(frame(spark, X, y * 0.0))             # not positive
    with pytest.raises(TypeError):
        GLR(elasticNetParam=0.5)
    # a fit whose mean overflows is reported with its family and link, not returned: the starting fit has slope
    # ~3 on x0 (the outlying row's weight keeps it out of that fit), so that row's eta is ~3000 at iteration 1
    x0 = np.linspace(0.0, 2.0, 40)
    Xb = np.r_[np.c_[x0, X[:, 1]], [[1000.0, 0.0]]]
    yb = np.r_[np.round(np.exp(3.0 * x0)), 0.0]
    with pytest.raises(RuntimeError, match="poisson.*log"):
        GLR(family="poisson", link="log", weightCol="w").fit(frame(spark, Xb, yb, np.r_[np.ones(40), 1e-12]))


def test_defaults_and_params():
    from cdnaml.ml.regression import GeneralizedLinearRegression as GLR
    g = GLR()
    assert (g.getFamily(), g.getMaxIter(), g.getTol(), g.getRegParam(), g.getSolver(), g.getFitIntercept(),
            g.getVariancePower(), g.getAggregationDepth()) == ("gaussian", 25, 1e-6, 0.0, "irls", True, 0.0, 2)
    assert not g.isDefined("link") and not g.isDefined("linkPower")
    g2 = GLR(family="poisson", link="log", labelCol="y", featuresCol="f", predictionCol="p", weightCol="w",
             offsetCol="o", linkPredictionCol="lp", variancePower=1.2, linkPower=0.0, aggregationDepth=3)
    assert g2.setLink("sqrt").getLink() == "sqrt" and g2.getOffsetCol() == "o"


def test_link_prediction_col_and_predict(spark):
    fam, link, vp, lp, X, y, w, off, *_ = case_data("poisson-exposure")
    m, df = fit(spark, X, y, None, off, family="poisson", linkPredictionCol="eta")
    out = m.transform(df).select("prediction", "eta").toPandas()
    eta = off + X @ m.coefficients.toArray() + m.intercept
    np.testing.assert_allclose(out.eta.to_numpy(), eta, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out.prediction.to_numpy(), np.exp(eta), rtol=1e-12)
    m2, df2 = fit(spark, X, y, family="poisson")
    assert "eta" not in m2.transform(df2).columns
    from cdnaml.ml.linalg import Vectors
    np.testing.assert_allclose(m2.predict(Vectors.dense(X[0])),
                               np.exp(X[0] @ m2.coefficients.toArray() + m2.intercept), rtol=1e-12)


def test_persistence_round_trip(spark, tmp_path):
    from cdnaml.ml.regression import GeneralizedLinearRegression, GeneralizedLinearRegressionModel
    fam, link, vp, lp, X, y, *_ = case_data("gamma-log")
    m, df = fit(spark, X, y, family="gamma", link="log")
    p = str(tmp_path / "glm")
    m.write().overwrite().save(p)
    back = GeneralizedLinearRegressionModel.load(p)
    assert (back.getFamily(), back.getLink(), back.intercept) == ("gamma", "log", m.intercept)
    assert np.array_equal(back.coefficients.toArray(), m.coefficients.toArray()) and not back.hasSummary
    a = m.transform(df).select("prediction").toPandas().prediction.to_numpy()
    b = back.transform(df).select("prediction").toPandas().prediction.to_numpy()
    assert np.array_equal(a, b)
    est = GeneralizedLinearRegression(family="tweedie", variancePower=1.3, linkPower=0.0)
    est.write().overwrite().save(str(tmp_path / "est"))
    e2 = GeneralizedLinearRegression.load(str(tmp_path / "est"))
    assert (e2.getFamily(), e2.getVariancePower(), e2.getLinkPower()) == ("tweedie", 1.3, 0.0)


def test_pyspark_alias(spark):
    from cdnaml import compat
    compat.install()
    try:
        from pyspark.ml.regression import (GeneralizedLinearRegression, GeneralizedLinearRegressionModel,
                                           GeneralizedLinearRegressionTrainingSummary)
        fam, link, vp, lp, X, y, *_ = case_data("poisson-log")
        glr = GeneralizedLinearRegression(family="poisson", link="log", maxIter=10, regParam=0.0)
        model = glr.fit(frame(spark, X, y))
        assert isinstance(model, GeneralizedLinearRegressionModel)
        assert isinstance(model.summary, GeneralizedLinearRegressionTrainingSummary)
        assert model.summary.deviance < model.summary.nullDeviance
    finally:
        compat.uninstall()
