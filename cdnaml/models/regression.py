"""Regression algorithms.

LinearRegression: ONE pass of the fused MFMA Gram kernel (K1) per rank, one
RCCL all-reduce of the (d+2)² f64 statistics, then an exact host solve in the
standardized space (Cholesky / least squares for OLS & ridge, coordinate
descent for elastic net — all sufficient statistics are in the Gram, so no
further data passes are needed; cf. Labs/ML 02L:68-79 "matrix decomposition"
first, iterative fallback).

Tree regressors delegate to :mod:`cdnaml.models.tree.engine`.

FMRegressor (and FMClassifier in :mod:`.classification`): Spark's minibatch gradient descent on the host, every
iteration one pass of the fused K25 kernel (X [V | w], the fp64 top and the gradient on the fp32 MFMA) plus one
all-reduce of P + 2 doubles.

AFTSurvivalRegression: L-BFGS on the host, every evaluation one pass of the fused fp64 K26 kernel plus one all-reduce
of d + 4 doubles.
"""
from __future__ import annotations

import math
import weakref
import zlib
from typing import Optional

import numpy as np
import torch

from ..ops import kernels as K
from ..sql import types as T
from ..sql.batch import ColumnData
from ..sql.dataframe import MapPlan
from .base import Estimator, Model
from .linalg import DenseMatrix, DenseVector, SparseVector
from .param import NO_DEFAULT, TypeConverters as TC, keyword_init
from .tree.binning import make_binned
from .tree.engine import ForestTrainer, TreeParams
from .tree import forest as _forest_mod
from .tree.forest import FitBins, Forest
from .util import (IllegalArgumentException, categorical_info, feature_dtype, global_count, global_offset,
                   gram_fp64_auto, local_batch, local_xyw, require_vector, streamed_columns)

_PRED = {
    "featuresCol": ("features column name", "features", TC.toString),
    "labelCol": ("label column name", "label", TC.toString),
    "predictionCol": ("prediction column name", "prediction", TC.toString),
}


def _default_seed(cls) -> int:
    return zlib.crc32(cls.__name__.encode()) & 0x7FFFFFFF


# =============================================================== summaries
class _RegressionSummary:
    def __init__(self, predictions, labelCol, predictionCol, numFeatures=0):
        self.predictions = predictions
        self.labelCol = labelCol
        self.predictionCol = predictionCol
        self._acc = None
        self._numFeatures = numFeatures

    def _sums(self):
        if self._acc is None:
            from .evaluation import RegressionEvaluator
            b = local_batch(self.predictions, [self.labelCol, self.predictionCol])
            acc = K.reg_metrics(b.columns[self.labelCol].values, b.columns[self.predictionCol].values)
            self.predictions._session.comm.all_reduce(acc)
            self._acc = acc.cpu().numpy()
        return self._acc

    def _m(self, name):
        from .evaluation import _regression_metric
        return _regression_metric(name, self._sums())

    @property
    def rootMeanSquaredError(self):
        return self._m("rmse")

    @property
    def meanSquaredError(self):
        return self._m("mse")

    @property
    def meanAbsoluteError(self):
        return self._m("mae")

    @property
    def r2(self):
        return self._m("r2")

    @property
    def explainedVariance(self):
        return self._m("var")

    @property
    def numInstances(self):
        return int(self._sums()[0])

    @property
    def r2adj(self):
        n, p = self.numInstances, self._numFeatures
        return 1 - (1 - self.r2) * (n - 1) / max(n - p - 1, 1)

    @property
    def residuals(self):
        from ..sql import functions as F
        return self.predictions.select((F.col(self.labelCol) - F.col(self.predictionCol)).alias("residuals"))

    @property
    def degreesOfFreedom(self):
        return self.numInstances - self._numFeatures - 1


class LinearRegressionTrainingSummary(_RegressionSummary):
    def __init__(self, predictions, labelCol, predictionCol, numFeatures, objectiveHistory, totalIterations,
                 stderr=None, coef=None, intercept=None):
        super().__init__(predictions, labelCol, predictionCol, numFeatures)
        self.objectiveHistory = objectiveHistory
        self.totalIterations = totalIterations
        self._stderr = stderr
        self._coef = coef
        self._intercept = intercept

    @property
    def coefficientStandardErrors(self):
        if callable(self._stderr):
            self._stderr = self._stderr()
        if self._stderr is None:
            raise RuntimeError("No Std. Error of coefficients available for this LinearRegressionModel")
        return list(self._stderr)

    @property
    def tValues(self):
        se = self.coefficientStandardErrors
        vals = list(self._coef) + [self._intercept]
        return [v / s if s > 0 else float("nan") for v, s in zip(vals, se)]

    @property
    def pValues(self):
        from scipy import stats
        dof = max(self.degreesOfFreedom, 1)
        return [float(2 * stats.t.sf(abs(t), dof)) for t in self.tValues]


def _gram_fp64(prec: str, n: int, d: int) -> bool:
    """gramPrecision "auto" (util.gram_fp64_auto): course-sized problems take an fp64 library GEMM of the
    augmented matrix -- Spark's normal-equation solver works in fp64 and course-sized one-hot designs are
    ill-conditioned (condition ~1e4: the K1 kernel's fp32 block accumulation moved coefficients by ~2e-3
    relative); larger ones take K1 (fp32 MFMA, HBM-bound)."""
    if prec == "fp64":
        return True
    return prec == "auto" and gram_fp64_auto(n, d)


def _lr_shift(Xk: torch.Tensor, yk: torch.Tensor, comm, d: int) -> torch.Tensor:
    """[d + 1] fp64 common shift of the features and the label: the mean of every rank's leading rows (averaged
    over the ranks that have any).  It only conditions the f32 Gram; the solve un-shifts exactly with the host
    copy of the same values."""
    k = Xk.shape[0]
    if comm.distributed:
        sh = torch.cat([torch.mean(Xk, 0, dtype=torch.float64), yk.double().mean().reshape(1)]) if k else \
            torch.zeros(d + 1, dtype=torch.float64, device=Xk.device)
        cnt = torch.full((1,), 1.0 if k else 0.0, dtype=torch.float64, device=Xk.device)
        comm.all_reduce_many([sh, cnt])
        return sh / cnt.clamp_min(1.0)
    # one rank: fp64-accumulated column means of the fp32 rows (no fp64 copy of the block), no all-reduce
    return torch.cat([torch.mean(Xk, 0, dtype=torch.float64), yk.double().mean().reshape(1)]) if k else \
        torch.zeros(d + 1, dtype=torch.float64, device=Xk.device)


def _cho_factor(A):
    from scipy.linalg import cho_factor  # lazily: tree / xgboost imports of this module need no scipy
    return cho_factor(A, lower=True, check_finite=False)


def _cho_solve(cl, b):
    from scipy.linalg import cho_solve
    return cho_solve(cl, b, check_finite=False)


# =========================================================== LinearRegression
class LinearRegression(Estimator):
    _params = dict(_PRED, **{
        "maxIter": ("max number of iterations (>= 0)", 100, TC.toInt),
        "regParam": ("regularization parameter (>= 0)", 0.0, TC.toFloat),
        "elasticNetParam": ("the ElasticNet mixing parameter, in range [0, 1]", 0.0, TC.toFloat),
        "tol": ("the convergence tolerance for iterative algorithms (>= 0)", 1e-6, TC.toFloat),
        "fitIntercept": ("whether to fit an intercept term", True, TC.toBoolean),
        "standardization": ("whether to standardize the training features before fitting the model", True,
                            TC.toBoolean),
        "solver": ("the solver algorithm for optimization: auto, normal, l-bfgs", "auto", TC.toString),
        "weightCol": ("weight column name", None, TC.toString),
        "aggregationDepth": ("suggested depth for treeAggregate (>= 2)", 2, TC.toInt),
        "loss": ("the loss function to be optimized: squaredError, huber", "squaredError", TC.toString),
        "epsilon": ("the shape parameter to control the amount of robustness (huber)", 1.35, TC.toFloat),
        "gramPrecision": ("Gram precision: auto (fp64 library GEMM for small problems, else fp32), fp32 (K1 f32 MFMA "
                          "with fp32 block accumulation), bf16 (K1 bf16 MFMA) or fp64", "auto", TC.toString),
    })

    def __init__(self, featuresCol=None, labelCol=None, predictionCol=None, maxIter=None, regParam=None,
                 elasticNetParam=None, tol=None, fitIntercept=None, standardization=None, solver=None,
                 weightCol=None, aggregationDepth=None, loss=None, epsilon=None, gramPrecision=None):
        super().__init__()
        keyword_init(self, {k: v for k, v in locals().items() if k not in ("self", "__class__")})

    def _fit(self, dataset):
        fc, lc, wc = self.getFeaturesCol(), self.getLabelCol(), self.getWeightCol()
        require_vector(dataset, fc)
        from .util import require_numeric
        require_numeric(dataset, lc)
        src = streamed_columns(dataset, fc, [lc] + ([wc] if wc else []), head_rows=4096)
        if src is not None:
            return self._fit_streamed(dataset, src, lc, wc)
        X, y, w = local_xyw(dataset, fc, lc, wc, keep_f64=True)
        comm = dataset._session.comm
        d = X.shape[1]
        fit_int = self.getFitIntercept()
        # common shift (global mean of per-rank leading samples) keeps the f32 Gram well conditioned; it stays on
        # the device (the label shift is applied to y there), so the fit reads the host once, for the Gram
        bf16 = self.getGramPrecision() == "bf16"
        fp64 = _gram_fp64(self.getGramPrecision(), X.shape[0], d + (1 if w is not None else 0))
        sh = shift = None
        yc = y
        if fit_int:
            sh = _lr_shift(X[:4096], y[:4096], comm, d)
            shift = sh[:d].float()
            # y - mean in fp64, rounded to fp32, in one pass (the Gram reads the fp32 label)
            yc = K.shifted_f32(y, sh[d:]) if y.is_cuda else y - sh[d]
        if w is None:
            G = K.gram(X, yc, shift, 0.0, bf16=bf16, fp64=fp64) if X.shape[0] else \
                torch.zeros((d + 2, d + 2), dtype=torch.float64, device=X.device)
        else:
            # weighted Gram on K1 too: rows scaled by sqrt(w), with sqrt(w) itself as an extra feature column,
            # so [X' | sqrt(w) | 1 | y']^T [...] holds sum w x x^T, sum w x, sum w and the y blocks
            sw = torch.sqrt(w).float()[:, None]
            Xw = torch.cat([(X.float() - (shift if shift is not None else 0.0)) * sw, sw], 1)
            G3 = K.gram(Xw, (yc.float() * sw[:, 0]), None, 0.0, bf16=bf16, fp64=fp64) if X.shape[0] else \
                torch.zeros((d + 3, d + 3), dtype=torch.float64, device=X.device)
            keep = torch.tensor(list(range(d + 1)) + [d + 2], device=X.device)
            G = G3[keep][:, keep].contiguous()
        comm.all_reduce(G)
        host = torch.cat([G.reshape(-1), sh if sh is not None else G.new_zeros(d + 1)]).cpu().numpy()
        G = host[:(d + 2) * (d + 2)].reshape(d + 2, d + 2)
        yshift = float(host[-1]) if fit_int else 0.0
        # the f32 shift the Gram kernel subtracted, from the same host copy (no second device read)
        shift_h = host[(d + 2) * (d + 2):(d + 2) * (d + 2) + d].astype(np.float32).astype(np.float64) \
            if shift is not None else None
        coef, intercept, hist, iters, stderr = self._solve(G, d, shift_h, yshift)
        if X.dtype == torch.float64:
            coef, intercept = self._refine(X, y, w, comm, G, d, shift_h, yshift, coef, intercept)
        model = LinearRegressionModel(coef, intercept)
        model._post_fit(self)
        preds = model.transform(dataset)
        model.summary = LinearRegressionTrainingSummary(preds, lc, self.getPredictionCol(), d, hist, iters,
                                                        stderr, coef, intercept)
        return model

    def _fit_streamed(self, dataset, src, lc, wc):
        """Out-of-core fit: K1 Gram blocks accumulated chunk by chunk in fp64 (X never resident),
        the shift taken from the first chunk's leading rows, then the same solve as the materialised fit."""
        Xs, cd, _ = src
        comm = dataset._session.comm
        d = Xs.d
        y = cd[lc].values.double()
        w = cd[wc].values.double() if wc else None
        fit_int = self.getFitIntercept()
        bf16 = self.getGramPrecision() == "bf16"
        fp64 = _gram_fp64(self.getGramPrecision(), Xs.n, d + (1 if w is not None else 0))
        dev = Xs.device
        head = cd["__head__"]
        sh = _lr_shift(head, y[:head.shape[0]], comm, d) if fit_int else \
            torch.zeros(d + 1, dtype=torch.float64, device=dev)
        shift = sh[:d].float() if fit_int else None
        extra = 1 if w is not None else 0
        G = torch.zeros((d + 2 + extra, d + 2 + extra), dtype=torch.float64, device=dev)
        for r0, Xc in Xs:
            m = Xc.shape[0]
            yc_ = y[r0:r0 + m]
            ycc = yc_ - sh[d] if fit_int else yc_
            if m == 0:
                continue
            if w is None:
                G += K.gram(Xc, ycc, shift, 0.0, bf16=bf16, fp64=fp64)
            else:
                sw = torch.sqrt(w[r0:r0 + m]).float()[:, None]
                Xw = torch.cat([(Xc.float() - (shift if shift is not None else 0.0)) * sw, sw], 1)
                G += K.gram(Xw, ycc.float() * sw[:, 0], None, 0.0, bf16=bf16, fp64=fp64)
        if w is not None:
            keep = torch.tensor(list(range(d + 1)) + [d + 2], device=dev)
            G = G[keep][:, keep].contiguous()
        comm.all_reduce(G)
        host = torch.cat([G.reshape(-1), sh]).cpu().numpy()
        Gh = host[:(d + 2) * (d + 2)].reshape(d + 2, d + 2)
        yshift = float(host[-1]) if fit_int else 0.0
        shift_h = host[(d + 2) * (d + 2):(d + 2) * (d + 2) + d].astype(np.float32).astype(np.float64) \
            if fit_int else None
        coef, intercept, hist, iters, stderr = self._solve(Gh, d, shift_h, yshift)
        model = LinearRegressionModel(coef, intercept)
        model._post_fit(self)
        model.summary = LinearRegressionTrainingSummary(model.transform(dataset), lc, self.getPredictionCol(), d,
                                                        hist, iters, stderr, coef, intercept)
        return model

    def _solve(self, G, d, shift, yshift):
        n = G[d, d]
        if n <= 0:
            raise IllegalArgumentException("requirement failed: empty training dataset")
        sx, sy = G[:d, d], G[d + 1, d]
        Sxx, Sxy, Syy = G[:d, :d], G[:d, d + 1], G[d + 1, d + 1]
        fit_int = self.getFitIntercept()
        s = np.asarray(shift, dtype=np.float64) if shift is not None else np.zeros(d)
        mx = s + sx / n
        my = yshift + sy / n
        Cxx = Sxx - np.outer(sx, sx) / n
        Cxy = Sxy - sx * sy / n
        Cyy = Syy - sy * sy / n
        varx = np.clip(np.diag(Cxx) / n, 0, None)
        sdx = np.sqrt(varx)
        vary = max(Cyy / n, 0.0)
        sdy = math.sqrt(vary)
        lam, alpha = self.getRegParam(), self.getElasticNetParam()
        if fit_int and sdy > 0.0 and (lam == 0.0 or alpha == 0.0) and bool((sdx > 0).all()):
            fast = self._solve_ridge(sdx, sdy, lam, alpha, d, n, mx, my, Cxx, Cxy, Cyy)
            if fast is not None:
                return fast
        if fit_int:
            M, c, yy = Cxx / n, Cxy / n, Cyy / n
        else:
            # raw (uncentred) moments
            raw_xx = Sxx + np.outer(s, sx) + np.outer(sx, s) + n * np.outer(s, s)
            raw_xy = Sxy + s * sy + yshift * sx + n * s * yshift
            M, c = raw_xx / n, raw_xy / n
            yy = (Syy + 2 * yshift * sy + n * yshift ** 2) / n
        if sdy == 0.0 and fit_int:
            return np.zeros(d), float(my), [0.0], 0, None
        ystd = sdy if sdy > 0 else 1.0
        active = sdx > 0
        scale = np.where(active, sdx, 1.0)
        Ms = M / np.outer(scale, scale)
        cs = c / scale / ystd
        lam_eff = lam / ystd
        if self.getStandardization():
            p1, p2 = np.ones(d), np.ones(d)
        else:
            p1, p2 = 1.0 / scale, 1.0 / (scale * scale)
        idx = np.nonzero(active)[0]
        beta_s = np.zeros(d)
        hist, iters = [], 0
        stderr = None
        if len(idx):
            Ma, ca = Ms[np.ix_(idx, idx)], cs[idx]
            l1 = lam_eff * alpha * p1[idx]
            l2 = lam_eff * (1 - alpha) * p2[idx]
            if lam == 0.0 or alpha == 0.0:
                A = Ma + np.diag(l2)
                try:
                    # SPD: Cholesky (raises when not positive definite) + two triangular solves, in LAPACK
                    c_, low = _cho_factor(A)
                    b = _cho_solve((c_, low), ca)
                except np.linalg.LinAlgError:
                    b = np.linalg.lstsq(A, ca, rcond=None)[0]
                iters = 1
            else:
                b = np.zeros(len(idx))
                tol = max(self.getTol(), 1e-12)
                for it in range(max(self.getMaxIter(), 1) * 10):
                    mx_change = 0.0
                    for j in range(len(idx)):
                        r = ca[j] - Ma[j] @ b + Ma[j, j] * b[j]
                        nb = np.sign(r) * max(abs(r) - l1[j], 0.0) / (Ma[j, j] + l2[j])
                        mx_change = max(mx_change, abs(nb - b[j]))
                        b[j] = nb
                    iters = it + 1
                    obj = 0.5 * b @ Ma @ b - ca @ b + (l1 * np.abs(b)).sum() + 0.5 * (l2 * b * b).sum()
                    hist.append(float(obj + 0.5 * yy / (ystd * ystd)))
                    if mx_change < tol:
                        break
            beta_s[idx] = b
        coef = beta_s * ystd / scale
        coef[~active] = 0.0
        intercept = float(my - coef @ mx) if fit_int else 0.0
        if not hist:
            resid = yy / (ystd * ystd) - 2 * cs @ beta_s + beta_s @ Ms @ beta_s
            hist = [0.5 * float(resid)]
        if lam == 0.0 and fit_int and len(idx) == d:
            stderr = self._stderr_fn(coef, Cxx, Cxy, Cyy, n, d, mx)
        return coef, intercept, hist, iters, stderr

    def _refine(self, X, y, w, comm, G, d, shift, yshift, coef, intercept, steps: int = 3):
        """Iterative refinement of the closed-form solution on Double features (course scale): the normal
        equations square the design's condition number (the ML 03 one-hot Airbnb design: cond(X) ~4e6), so the
        Cholesky solution alone is good to ~cond(X)^2 eps ~1e-4.  Each step forms the exact gradient from the data
        -- g = sum w (x - mean) r with r = y - x.coef - b in fp64, one pass, all-reduced -- and solves the same
        system for the correction (corrected semi-normal equations): the coefficients converge to ~cond(X) eps,
        what a QR / SVD least-squares solve gives.  Only the closed-form case (intercept, L2 or no penalty, every
        feature varying) is refined; the other solvers are iterative already."""
        n = G[d, d]
        sx, sy = G[:d, d], G[d + 1, d]
        Cxx, Cyy = G[:d, :d] - np.outer(sx, sx) / n, G[d + 1, d + 1] - sy * sy / n
        sdx = np.sqrt(np.clip(np.diag(Cxx) / n, 0, None))
        sdy = math.sqrt(max(Cyy / n, 0.0))
        lam, alpha = self.getRegParam(), self.getElasticNetParam()
        if not (self.getFitIntercept() and sdy > 0.0 and (lam == 0.0 or alpha == 0.0) and bool((sdx > 0).all())):
            return coef, intercept
        A = Cxx.copy()
        if lam > 0.0:
            p2 = np.ones(d) if self.getStandardization() else 1.0 / (sdx * sdx)
            A += np.diag(n * (lam / sdy) * (1 - alpha) * p2 * sdx * sdx)
        try:
            cf = _cho_factor(A)
        except np.linalg.LinAlgError:
            return coef, intercept
        mx = (np.asarray(shift, np.float64) if shift is not None else 0.0) + sx / n
        pen = A - Cxx
        coef = np.asarray(coef, np.float64).copy()
        for _ in range(steps):
            cw = torch.tensor(coef, dtype=torch.float64, device=X.device)
            r = y - (X @ cw + intercept) if X.shape[0] else y
            if w is not None:
                r = r * w
            acc = torch.cat([X.T @ r, r.sum().reshape(1)]) if X.shape[0] else \
                torch.zeros(d + 1, dtype=torch.float64, device=X.device)
            comm.all_reduce(acc)
            a = acc.cpu().numpy()
            g = a[:d] - mx * a[d] - pen @ coef          # sum w (x - mean) r, less the ridge term
            delta = _cho_solve(cf, g)
            coef = coef + delta
            intercept = intercept + a[d] / n - float(mx @ delta)   # sum w r = 0 at the optimum
            if np.max(np.abs(delta)) <= 1e-15 * max(np.max(np.abs(coef)), 1e-300):
                break
        return coef, float(intercept)

    @staticmethod
    def _stderr_fn(coef, Cxx, Cxy, Cyy, n, d, mx):
        """Standard errors (unregularised normal-equation solution only), computed on first access: the d x d
        inverse cost ~1 ms of host BLAS per fit (half the fit time at 1e7 x 100 on MI355X) for a summary field
        most fits never read."""
        def stderr():
            try:
                sse = max(Cyy - 2 * coef @ Cxy + coef @ Cxx @ coef, 0.0)
                sigma2 = sse / max(n - d - 1, 1)
                inv = np.linalg.inv(Cxx)
                se_coef = np.sqrt(np.clip(np.diag(inv) * sigma2, 0, None))
                se_int = math.sqrt(max(sigma2 * (1.0 / n + mx @ inv @ mx), 0.0))
                return list(se_coef) + [se_int]
            except np.linalg.LinAlgError:
                return None
        return stderr

    def _solve_ridge(self, sdx, sdy, lam, alpha, d, n, mx, my, Cxx, Cxy, Cyy):
        """Fast path of _solve for the closed-form case (intercept, L2 or no penalty, every feature varying):
        the standardised system (D^-1 M D^-1 + L) b = D^-1 c / sd_y (M = Cxx / n, c = Cxy / n), coef =
        sd_y D^-1 b, has the same solution as (Cxx + n D L D) coef = Cxy -- one Cholesky of the unscaled
        covariance, no scaled copies (the general path's ~20 d x d numpy passes cost ~0.3 ms of host time per
        fit, a fifth of the fit at 1e7 x 100).  None when the system is not positive definite (the general
        path's least squares then)."""
        A = Cxx
        if lam > 0.0:
            p2 = np.ones(d) if self.getStandardization() else 1.0 / (sdx * sdx)
            A = Cxx + np.diag(n * (lam / sdy) * (1 - alpha) * p2 * sdx * sdx)
        try:
            coef = _cho_solve(_cho_factor(A), Cxy)
        except np.linalg.LinAlgError:
            return None
        intercept = float(my - coef @ mx)
        # the general path's objective history: 0.5 (yy - 2 c.coef + coef.M.coef) / sd_y^2, penalty not included
        obj = 0.5 * float(Cyy - 2 * Cxy @ coef + coef @ (Cxx @ coef)) / (n * sdy * sdy)
        stderr = self._stderr_fn(coef, Cxx, Cxy, Cyy, n, d, mx) if lam == 0.0 else None
        return coef, intercept, [obj], 1, stderr


class LinearRegressionModel(Model):
    _params = LinearRegression._params

    def __init__(self, coefficients=None, intercept=0.0):
        super().__init__()
        self._coef = np.asarray(coefficients if coefficients is not None else [], dtype=np.float64)
        self._intercept = float(intercept)
        self.summary = None

    @property
    def coefficients(self):
        return DenseVector(self._coef)

    @property
    def intercept(self):
        return self._intercept

    @property
    def numFeatures(self):
        return len(self._coef)

    @property
    def hasSummary(self):
        return self.summary is not None

    @property
    def scale(self):
        return 1.0

    def predict(self, features):
        x = features.toArray() if hasattr(features, "toArray") else np.asarray(features)
        return float(x @ self._coef + self._intercept)

    def _transform(self, dataset):
        fc, pc = self.getFeaturesCol(), self.getPredictionCol()
        require_vector(dataset, fc)
        coef = torch.tensor(self._coef, dtype=torch.float32)
        coef64 = torch.tensor(self._coef, dtype=torch.float64)
        icpt = self._intercept

        def fn(b, ctx):
            X = b.columns[fc].values
            if X.dtype == torch.float64:     # Double vectors: Spark's fp64 dot product
                p = X @ coef64.to(X.device) + icpt
            else:
                p = (X.float() @ coef.to(X.device)).double() + icpt if X.shape[0] else \
                    torch.zeros(0, dtype=torch.float64, device=X.device)
            return b.with_column(pc, ColumnData(p, T.DoubleType(), b.columns[fc].valid))
        return dataset._new(MapPlan(dataset._plan, f"LinearRegressionModel -> {pc}", fn))

    def evaluate(self, dataset):
        return _RegressionSummary(self.transform(dataset), self.getLabelCol(), self.getPredictionCol(),
                                  self.numFeatures)

    def _save_state(self):
        return {"intercept": self._intercept}, {"coefficients": torch.tensor(self._coef)}

    def _load_state(self, extra, tensors, stages):
        self._coef = tensors["coefficients"].numpy()
        self._intercept = float(extra["intercept"])
        self.summary = None

    def __repr__(self):
        return f"LinearRegressionModel: uid={self.uid}, numFeatures={self.numFeatures}"


# ================================================================ trees
_TREE = {
    "maxDepth": ("Maximum depth of the tree. (>= 0)", 5, TC.toInt),
    "maxBins": ("Max number of bins for discretizing continuous features. Must be >= 2 and >= number of "
                "categories for any categorical feature.", 32, TC.toInt),
    "minInstancesPerNode": ("Minimum number of instances each child must have after split.", 1, TC.toInt),
    "minWeightFractionPerNode": ("Minimum fraction of the weighted sample count that each child must have.",
                                 0.0, TC.toFloat),
    "minInfoGain": ("Minimum information gain for a split to be considered at a tree node.", 0.0, TC.toFloat),
    "maxMemoryInMB": ("Maximum memory in MB allocated to histogram aggregation.", 256, TC.toInt),
    "cacheNodeIds": ("If false, the algorithm will pass trees to executors to match instances with nodes.",
                     False, TC.toBoolean),
    "checkpointInterval": ("set checkpoint interval (>= 1) or disable checkpoint (-1).", 10, TC.toInt),
    "seed": ("random seed.", None, TC.toInt),
    "weightCol": ("weight column name.", None, TC.toString),
    "leafCol": ("Leaf indices column name.", "", TC.toString),
}
_RF = {
    "numTrees": ("Number of trees to train (>= 1).", 20, TC.toInt),
    "featureSubsetStrategy": ("The number of features to consider for splits at each tree node. Supported "
                              "options: 'auto', 'all', 'onethird', 'sqrt', 'log2', (0.0-1.0], [1-n].", "auto",
                              TC.toString),
    "subsamplingRate": ("Fraction of the training data used for learning each decision tree, in range (0, 1].",
                        1.0, TC.toFloat),
    "bootstrap": ("Whether bootstrap samples are used when building trees.", True, TC.toBoolean),
}


def resolve_subset(strategy: str, d: int, num_trees: int, classification: bool) -> Optional[int]:
    s = strategy.lower()
    if s == "auto":
        s = "all" if num_trees == 1 else ("sqrt" if classification else "onethird")
    if s == "all":
        return None
    if s == "sqrt":
        return max(1, int(math.ceil(math.sqrt(d))))
    if s == "log2":
        return max(1, int(math.ceil(math.log2(d))))
    if s == "onethird":
        return max(1, int(math.ceil(d / 3.0)))
    try:
        v = float(s)
    except ValueError:
        raise IllegalArgumentException(f"invalid featureSubsetStrategy {strategy}")
    if v.is_integer() and v >= 1 and "." not in s:
        return min(d, int(v))
    if 0 < v <= 1:
        return max(1, int(math.ceil(v * d)))
    raise IllegalArgumentException(f"invalid featureSubsetStrategy {strategy}")


def tree_fit_prepare(est, dataset, classification: bool, pre=None):
    """Common: device features/labels, categorical info, global row offset, binned data.

    pre(n_local, row_offset, seed, device, y): launched before the quantile sample is queued (the label's fp32
    copy and maximum, on a side stream); it may return a callable, run right before the binning is queued (the
    bootstrap draws: compute-bound, they overlap the memory-bound binning)."""
    fc, lc = est.getFeaturesCol(), est.getLabelCol()
    wc = est.getWeightCol() if est.hasParam("weightCol") else None
    require_vector(dataset, fc)
    session = dataset._session
    cols = [fc, lc] + ([wc] if wc else [])
    src = streamed_columns(dataset, fc, cols[1:])
    if src is not None:
        # out-of-core: X streamed chunk by chunk into the quantile sample and the bins, never resident
        X, cd, fmeta = src
        y = cd[lc].values.double()
        w = cd[wc].values.double() if wc else None
    else:
        b = local_batch(dataset, cols)
        fcol = b.columns[fc]
        fmeta = fcol.meta
        X = fcol.values.float()
        X = X if X.is_contiguous() else X.contiguous()
        y = b.columns[lc].values.double()
        w = b.columns[wc].values.double() if wc else None
    d = X.shape[1]
    cat = categorical_info(fmeta, d, fc)
    n = X.shape[0]
    n_global = global_count(session, n)
    off = global_offset(session, n)
    seed = est.getOrDefault("seed")
    if seed is None:
        seed = _default_seed(type(est))
    late = pre(n, off, seed, X.device, y) if pre is not None else None
    data = make_binned(session, X, cat, est.getMaxBins(), seed, off, n_global, before_binize=late)
    data.source_ref = weakref.ref(fcol.values) if src is None else None
    return session, data, y, w, seed, fmeta


def attach_fit_bins(forest: Forest, data) -> None:
    """Give a single-output forest the bins of its training tensor (``FitBins``): a transform of that same,
    unmodified tensor then predicts from the bins (REUSE_FIT_BINS; numeric features only)."""
    src = data.source_ref() if data.source_ref is not None else None
    if (_forest_mod.REUSE_FIT_BINS and src is not None and src.is_cuda and forest.K == 1 and not data.categorical
            and not data.missing_bin and data.bins is not None and data.bins.is_cuda):
        forest._fit_bins = FitBins(src, data.bins, data.thresholds, data.nthr, data.d, data.B)


def _num_classes(session, y: torch.Tensor, meta_label: Optional[dict]) -> int:
    if meta_label and meta_label.get("num_vals"):
        return int(meta_label["num_vals"])
    mx = torch.tensor([float(y.max()) if y.numel() else 0.0], dtype=torch.float64, device=session.comm.device)
    session.comm.all_reduce(mx, "max")
    return int(mx) + 1


class _TreeModelBase(Model):
    """Shared prediction + persistence for tree ensembles.

    ``contributionsCol`` (model-only output param, off by default): a vector column of numFeatures + 1 doubles per
    row, the exact path-dependent TreeSHAP contribution of every feature to the row's raw prediction (the margin
    of a GBTClassifier) and, last, the bias; a row's contributions sum to its raw prediction.  Single-output
    ensembles only: DecisionTree / RandomForest classification models raise NotImplementedError."""
    _params = {
        "contributionsCol": ("Per-feature TreeSHAP contributions (+ bias) column name; empty: not computed.", "",
                             TC.toString),
    }

    def __init__(self, forest: Optional[Forest] = None, numFeatures: int = 0, tree_weights=None):
        super().__init__()
        self._forest = forest
        self._numFeatures = numFeatures
        self._tree_w = np.asarray(tree_weights if tree_weights is not None else [], dtype=np.float64)

    @property
    def numFeatures(self):
        return self._numFeatures

    @property
    def featureImportances(self):
        imp = self._forest.feature_importances(self._numFeatures)
        nz = np.nonzero(imp)[0]
        return SparseVector(self._numFeatures, nz.tolist(), imp[nz].tolist())

    @property
    def getNumTrees(self):
        return len(self._forest.roots)

    @property
    def treeWeights(self):
        return list(self._tree_w)

    @property
    def totalNumNodes(self):
        return sum(len(self._forest.tree_nodes(t)) for t in range(len(self._forest.roots)))

    @property
    def numNodes(self):
        return self.totalNumNodes

    @property
    def depth(self):
        return int(self._forest.tree_depths().max()) if self._forest.roots else 0

    def toDebugString_tree(self, t, names=None):
        f = self._forest
        lines = []

        def rec(i, ind):
            pad = " " * ind
            if f.feat[i] < 0:
                v = f.value[i]
                lines.append(f"{pad}Predict: {float(v[0]) if len(v) == 1 else int(np.argmax(v)):g}")
                return
            fn = f"feature {f.feat[i]}"
            if f.is_cat[i]:
                cats = [c for c in range(256) if (int(f.catmask[i][c >> 5]) >> (c & 31)) & 1]
                lines.append(f"{pad}If ({fn} in {{{','.join(f'{c:.1f}' for c in cats)}}})")
                rec(f.left[i], ind + 1)
                lines.append(f"{pad}Else ({fn} not in {{{','.join(f'{c:.1f}' for c in cats)}}})")
            else:
                lines.append(f"{pad}If ({fn} <= {f.thr[i]})")
                rec(f.left[i], ind + 1)
                lines.append(f"{pad}Else ({fn} > {f.thr[i]})")
            rec(f.right[i], ind + 1)
        rec(f.roots[t], 1)
        return "\n".join(lines)

    @property
    def toDebugString(self):
        T_ = len(self._forest.roots)
        s = f"{type(self).__name__}: uid={self.uid}, depth={self.depth}, numNodes={self.totalNumNodes}, " \
            f"numFeatures={self._numFeatures}\n"
        if T_ == 1:
            return s + self.toDebugString_tree(0)
        return s + "\n".join(f"  Tree {t} (weight {self._tree_w[t] if t < len(self._tree_w) else 1.0}):\n" +
                             self.toDebugString_tree(t) for t in range(T_))

    def _save_state(self):
        return {"numFeatures": self._numFeatures, "K": self._forest.K}, dict(
            self._forest.state(), tree_w=torch.tensor(self._tree_w))

    def _load_state(self, extra, tensors, stages):
        self._forest = Forest.from_state(tensors)
        self._numFeatures = int(extra["numFeatures"])
        self._tree_w = tensors["tree_w"].numpy()

    def _leaf_col(self, b, out_cols):
        lc = self.getLeafCol() if self.hasParam("leafCol") else ""
        if lc:
            X = b.columns[self.getFeaturesCol()].values
            leaves = self._forest.predict_leaf_index(X).double().to(X.device)
            out_cols[lc] = ColumnData(leaves, T.VectorUDT())

    def _check_contributions(self) -> str:
        """The contributions column name ("": off); raises for ensembles TreeSHAP does not cover."""
        cc = self.getContributionsCol()
        if cc and self._forest.K != 1:
            raise NotImplementedError(
                f"{type(self).__name__}: contributionsCol needs a single-output ensemble (regression trees or GBT "
                f"margins); this model's leaves hold {self._forest.K} class outputs")
        return cc

    def _contrib_col(self, b, out_cols):
        cc = self.getContributionsCol()
        if cc:
            X = b.columns[self.getFeaturesCol()].values
            phi = self._forest.shap_values(X, self._tree_w, [getattr(self, "_base", 0.0)])
            out_cols[cc] = ColumnData(phi, T.VectorUDT())

    def featureContributions(self, dataset, contributionsCol: str = "contributions"):
        """``transform(dataset)`` with the TreeSHAP contributions column on (``contributionsCol`` as set on the
        model, else the given name)."""
        cc = self.getContributionsCol() or contributionsCol
        return self.copy({self.contributionsCol: cc}).transform(dataset)


class _TreeRegressorModel(_TreeModelBase):
    _base = 0.0

    def _transform(self, dataset):
        fc, pc = self.getFeaturesCol(), self.getPredictionCol()
        require_vector(dataset, fc)
        forest, tw, base = self._forest, self._tree_w, self._base
        self._check_contributions()

        from .inference import predictor_for
        predictor = predictor_for(self, "value", [base])  # forest uploaded once; recurring buffers graph-replayed

        def fn(b, ctx):
            X = b.columns[fc].values
            p = predictor(X, torch.float64)[:, 0] if X.shape[0] else \
                torch.zeros(0, dtype=torch.float64, device=X.device)
            out = {pc: ColumnData(p, T.DoubleType())}
            self._leaf_col(b, out)
            self._contrib_col(b, out)
            nb = b
            for k, v in out.items():
                nb = nb.with_column(k, v)
            return nb
        return dataset._new(MapPlan(dataset._plan, f"{type(self).__name__} -> {pc}", fn))

    def predict(self, features):
        x = torch.tensor(np.asarray(features.toArray() if hasattr(features, "toArray") else features),
                         dtype=torch.float32)[None, :]
        return float(self._forest.predict(x, self._tree_w, [self._base])[0, 0])

    def evaluate(self, dataset):
        return _RegressionSummary(self.transform(dataset), self.getLabelCol(), self.getPredictionCol(),
                                  self._numFeatures)


def _early_side_work(num_trees, bootstrap, rate, want_label_max=True, codes_ok=False):
    """(pre, early): ``pre`` for tree_fit_prepare queues the label's fp32 copy and max |label| on the side stream
    before the quantile sample, and returns the Poisson bootstrap draws (+ the largest weight) for
    tree_fit_prepare to queue on the side stream right before the binning; the first level reads the maxima
    without draining the queue.  ``early`` then holds "yf" (fp32 label) and "codes" (BootstrapCodes) or "w"
    (weights); call _join_early once the binning is queued."""
    early = {}

    def pre(n, off, seed_, dev, y_):
        if dev.type != "cuda":
            return None
        side = _side_stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        if want_label_max:
            early["yf"] = K.float_with_absmax(y_, stream=side)


        def draws():
            # queued right behind the quantile kernel, before the binning, on the MAIN stream (K.POISSON_STREAM
            # =side: the side stream).  Measured at 1e8 rows (profiles/r4/prologue_ab.md): beside the quantile sort
            # the draws kept its 1024-thread blocks off the CUs (2.1 ms for a 0.3 ms kernel); beside the binning --
            # itself ~60 % VALU-bound (6-step threshold search) -- they slowed it by more than their own 2.2 ms;
            # in series they cost exactly their 2.2 ms
            if bootstrap and num_trees > 1:
                if codes_ok and K.POISSON_CODES:
                    # the draws written straight as the engine's row codes + their max (no uint8 weights, no
                    # codes_init pass, no separate max reduction over T x n bytes); lazy: the trainer's level-0
                    # root histogram draws them itself when it can (K.POISSON_FUSED), else they run here on demand
                    with torch.cuda.stream(side if K.POISSON_STREAM == "side" else torch.cuda.current_stream(dev)):
                        early["codes"] = K.BootstrapCodes(num_trees, n, seed_, off, rate, dev,
                                                          lazy=K.POISSON_FUSED and K.POISSON_STREAM != "side")
                else:
                    early["w"] = _poisson_side(num_trees, n, seed_, off, rate, dev, join=False)
                    K.prefetch_max(early["w"], stream=side)
        return draws
    return pre, early


def _label_f32(early, y):
    """The fp32 label queued on the side stream (``early["yf"]``), else a cast of ``y`` (never both: a
    ``dict.get(k, y.float())`` default is evaluated eagerly -- a full extra cast of the label per fit, 0.27 ms at
    1e8 rows)."""
    yf = early.get("yf")
    return yf if yf is not None else y.float()


def _join_early(early, dev):
    for k in ("yf", "w"):
        if k in early:
            _join_side(early[k], dev)  # binning is queued: the trainer's first kernel waits for the side stream
    if "codes" in early:
        _join_side(early["codes"].codes, dev)


def _train_forest_regression(est, dataset, num_trees, subset, bootstrap, rate, impurity="variance"):
    pre, early = _early_side_work(num_trees, bootstrap, rate)
    session, data, y, w, seed, meta = tree_fit_prepare(est, dataset, classification=False, pre=pre)
    _join_early(early, data.bins.device)
    p = TreeParams(max_depth=est.getMaxDepth(), max_bins=est.getMaxBins(),
                   min_instances=float(est.getMinInstancesPerNode()), min_info_gain=est.getMinInfoGain(),
                   impurity=impurity, feature_subset=subset, bootstrap=bootstrap, subsampling_rate=rate, seed=seed)
    weights = early["w"] if "w" in early else _bag_weights(data, num_trees, bootstrap, rate, seed)
    if w is not None:
        weights = _combine_weights(weights, w, num_trees)
    trainer = ForestTrainer(session, data, p)
    forest = trainer.train(num_trees, {"v0": None, "v1": _label_f32(early, y)}, weights)
    attach_fit_bins(forest, data)
    return forest, data.d


_SIDE_STREAMS = {}


def _side_stream(dev):
    s = _SIDE_STREAMS.get(dev.index)
    if s is None:
        s = _SIDE_STREAMS[dev.index] = torch.cuda.Stream(device=dev)
    return s


def _poisson_side(T_, n, seed, row_offset, rate, dev, join: bool = True):
    """Compute-bound Philox Poisson draws on a side stream (they depend on nothing queued on the current one).
    join: the current stream waits for them before its next kernel (else call _join_side before using them)."""
    side = _side_stream(dev)
    with torch.cuda.stream(side):
        wts = K.poisson_weights(T_, n, seed, row_offset, rate, device=dev)
    if join:
        _join_side(wts, dev)
    return wts


def _join_side(wts, dev):
    main = torch.cuda.current_stream(dev)
    main.wait_stream(_side_stream(dev))
    wts.record_stream(main)


def _bag_weights(data, T_, bootstrap, rate, seed):
    n = data.n_local
    dev = data.bins.device
    if bootstrap and T_ > 1:
        if dev.type == "cuda":
            return _poisson_side(T_, n, seed, data.row_offset, rate, dev)
        return K.poisson_weights(T_, n, seed, data.row_offset, rate, device=dev)
    if rate < 1.0:
        u = torch.stack([K.uniform(n, seed, data.row_offset, 0x200 + t, device=dev) for t in range(T_)])
        return (u < rate).to(torch.uint8)
    return None


def _combine_weights(bag, w, T_):
    # instance weights must be small non-negative integers for the uint8 weight path
    wi = torch.round(w).clamp(0, 255).to(torch.uint8)
    if bag is None:
        return wi[None, :].expand(T_, -1).contiguous()
    return (bag.to(torch.int32) * wi.to(torch.int32)[None, :]).clamp(0, 255).to(torch.uint8)


class DecisionTreeRegressor(Estimator):
    _params = dict(_PRED, **_TREE, **{
        "impurity": ("Criterion used for information gain calculation. Supported: variance", "variance",
                     TC.toString),
        "varianceCol": ("column name for the biased sample variance of prediction", None, TC.toString),
    })

    def __init__(self, **kwargs):
        super().__init__()
        keyword_init(self, kwargs)

    def _fit(self, dataset):
        forest, d = _train_forest_regression(self, dataset, 1, None, False, 1.0)
        return DecisionTreeRegressionModel(forest, d, [1.0])


class DecisionTreeRegressionModel(_TreeRegressorModel):
    _params = DecisionTreeRegressor._params


class RandomForestRegressor(Estimator):
    """Bagged regression trees (ML 07:41; north-star benchmark model)."""
    _params = dict(_PRED, **_TREE, **_RF, **{
        "impurity": ("Criterion used for information gain calculation. Supported: variance", "variance",
                     TC.toString),
    })

    def __init__(self, **kwargs):
        super().__init__()
        keyword_init(self, kwargs)

    def _fit(self, dataset):
        T_ = self.getNumTrees()
        forest, dd = _train_rf_reg(self, dataset, T_)
        return RandomForestRegressionModel(forest, dd, np.full(T_, 1.0 / T_))


def _train_rf_reg(est, dataset, T_):
    pre, early = _early_side_work(T_, est.getBootstrap(), est.getSubsamplingRate(),
                                  codes_ok=not (est.hasParam("weightCol") and est.getWeightCol()))
    session, data, y, w, seed, meta = tree_fit_prepare(est, dataset, classification=False, pre=pre)
    _join_early(early, data.bins.device)
    subset = resolve_subset(est.getFeatureSubsetStrategy(), data.d, T_, False)
    p = TreeParams(max_depth=est.getMaxDepth(), max_bins=est.getMaxBins(),
                   min_instances=float(est.getMinInstancesPerNode()), min_info_gain=est.getMinInfoGain(),
                   impurity="variance", feature_subset=subset, bootstrap=est.getBootstrap(),
                   subsampling_rate=est.getSubsamplingRate(), seed=seed)
    bc = early.get("codes")
    if bc is not None:
        weights = None
    else:
        weights = early["w"] if "w" in early else \
            _bag_weights(data, T_, est.getBootstrap(), est.getSubsamplingRate(), seed)
    if w is not None:
        weights = _combine_weights(bc.weights() if bc is not None else weights, w, T_)
        bc = None
    forest = ForestTrainer(session, data, p).train(T_, {"v0": None, "v1": _label_f32(early, y)}, weights,
                                                   codes_pre=bc)
    attach_fit_bins(forest, data)
    return forest, data.d


class RandomForestRegressionModel(_TreeRegressorModel):
    _params = RandomForestRegressor._params

    @property
    def trees(self):
        out = []
        for t in range(len(self._forest.roots)):
            f = Forest(self._forest.K)
            sub = _subforest(self._forest, t)
            out.append(DecisionTreeRegressionModel(sub, self._numFeatures, [1.0]))
        return out


def _subforest(forest: Forest, t: int) -> Forest:
    idx = forest.tree_nodes(t)
    pos = {g: j for j, g in enumerate(idx)}
    f = Forest(forest.K)
    for g in idx:
        j = f.add(forest.value[g], forest.weight[g], forest.depth[g], forest.impurity[g])
        f.feat[j], f.thr[j], f.bin[j] = forest.feat[g], forest.thr[g], forest.bin[g]
        f.is_cat[j], f.catmask[j], f.gain[j] = forest.is_cat[g], forest.catmask[g], forest.gain[g]
    for g in idx:
        if forest.feat[g] >= 0:
            f.left[pos[g]], f.right[pos[g]] = pos[forest.left[g]], pos[forest.right[g]]
    f.roots = [0]
    return f


# ================================================================== GBT
_GBT = {
    "maxIter": ("max number of iterations (>= 0)", 20, TC.toInt),
    "stepSize": ("Step size (a.k.a. learning rate) in interval (0, 1] for shrinking the contribution of each "
                 "estimator.", 0.1, TC.toFloat),
    "subsamplingRate": ("Fraction of the training data used for learning each decision tree.", 1.0, TC.toFloat),
    "featureSubsetStrategy": ("The number of features to consider for splits at each tree node.", "all",
                              TC.toString),
    "validationIndicatorCol": ("name of the column that indicates whether each row is for training or for "
                               "validation.", None, TC.toString),
    "validationTol": ("Threshold for stopping early when fit with validation is used.", 0.01, TC.toFloat),
    "impurity": ("Criterion used for information gain calculation: variance", "variance", TC.toString),
}


def boost(session, data, y_target_fn, grad_fn, T_rounds, est, seed, init_margin, first_weight_one=True):
    """Generic gradient boosting on the shared binned data (variance-impurity trees on pseudo-residuals)."""
    dev = data.bins.device
    n = data.n_local
    subset = resolve_subset(est.getFeatureSubsetStrategy(), data.d, 1, False)
    p = TreeParams(max_depth=est.getMaxDepth(), max_bins=est.getMaxBins(),
                   min_instances=float(est.getMinInstancesPerNode()), min_info_gain=est.getMinInfoGain(),
                   impurity="variance", feature_subset=subset, seed=seed)
    trainer = ForestTrainer(session, data, p)
    forest = Forest(1)
    F = torch.full((n,), float(init_margin), dtype=torch.float32, device=dev)
    weights = []
    # checkpointInterval + SparkContext.setCheckpointDir: resume from the last saved round
    from .tree.checkpoint import RoundCheckpointer
    ck = RoundCheckpointer(session, est, data,
                           est.getCheckpointInterval() if est.hasParam("checkpointInterval") else None,
                           labels=y_target_fn(F))
    start = 0
    resumed = ck.load()
    if resumed is not None:
        start, forest, Fm, extra = resumed
        F = Fm.to(dev)
        weights = list(extra["weights"])
    for m in range(start, T_rounds):
        target = y_target_fn(F) if (m == 0 and first_weight_one) else grad_fn(F)
        bag = _bag_weights(data, 1, False, est.getSubsamplingRate(), seed + m)
        trainer.p.seed = seed + m
        trainer.train(1, {"v0": None, "v1": target.float()}, bag, forest)
        wgt = 1.0 if (m == 0 and first_weight_one) else est.getStepSize()
        nodes, vals, masks = forest.binned_arrays(dev, m)
        K.predict_binned_add(data.bins, nodes, 0, vals, masks, wgt, F)
        weights.append(wgt)
        ck.maybe_save(m + 1, forest, F, {"weights": weights})
    ck.finish()
    return forest, np.asarray(weights)


class GBTRegressor(Estimator):
    _params = dict(_PRED, **_TREE, **_GBT, **{
        "lossType": ("Loss function which GBT tries to minimize: squared, absolute", "squared", TC.toString),
    })

    def __init__(self, **kwargs):
        super().__init__()
        keyword_init(self, kwargs)

    def _fit(self, dataset):
        session, data, y, w, seed, meta = tree_fit_prepare(self, dataset, classification=False)
        yf = y.float()
        loss = self.getLossType()
        if loss == "squared":
            grad = lambda F: yf - F  # noqa: E731
        elif loss == "absolute":
            grad = lambda F: torch.sign(yf - F)  # noqa: E731
        else:
            raise IllegalArgumentException(f"unsupported lossType {loss}")
        forest, tw = boost(session, data, lambda F: yf, grad, self.getMaxIter(), self, seed, 0.0)
        return GBTRegressionModel(forest, data.d, tw)


class GBTRegressionModel(_TreeRegressorModel):
    _params = GBTRegressor._params

    @property
    def trees(self):
        return [DecisionTreeRegressionModel(_subforest(self._forest, t), self._numFeatures, [1.0])
                for t in range(len(self._forest.roots))]


class IsotonicRegression(Estimator):
    """Pool-adjacent-violators on the globally sorted (feature, label) pairs."""
    _params = dict(_PRED, **{
        "isotonic": ("whether the output sequence should be isotonic/increasing", True, TC.toBoolean),
        "featureIndex": ("index of the feature if featuresCol is a vector column", 0, TC.toInt),
        "weightCol": ("weight column name", None, TC.toString),
    })

    def __init__(self, **kwargs):
        super().__init__()
        keyword_init(self, kwargs)

    def _fit(self, dataset):
        pdf = dataset.select(self.getFeaturesCol(), self.getLabelCol()).toPandas()
        x = np.array([v[self.getFeatureIndex()] if hasattr(v, "toArray") else v
                      for v in pdf[self.getFeaturesCol()]], dtype=np.float64)
        yv = pdf[self.getLabelCol()].to_numpy(np.float64)
        sign = 1.0 if self.getIsotonic() else -1.0
        o = np.argsort(x, kind="stable")
        xs, ys = x[o], sign * yv[o]
        vals, wts, xs_b = [], [], []
        for xi, yi in zip(xs, ys):
            vals.append(yi)
            wts.append(1.0)
            xs_b.append([xi, xi])
            while len(vals) > 1 and vals[-2] > vals[-1]:
                v = (vals[-2] * wts[-2] + vals[-1] * wts[-1]) / (wts[-2] + wts[-1])
                wts[-2] += wts[-1]
                vals[-2] = v
                xs_b[-2][1] = xs_b[-1][1]
                vals.pop(); wts.pop(); xs_b.pop()
        bnd, pred = [], []
        for (a, b), v in zip(xs_b, vals):
            bnd += [a, b] if a != b else [a]
            pred += [sign * v] * (2 if a != b else 1)
        return IsotonicRegressionModel(np.array(bnd), np.array(pred))


class IsotonicRegressionModel(Model):
    _params = IsotonicRegression._params

    def __init__(self, boundaries=None, predictions=None):
        super().__init__()
        self._b = np.asarray(boundaries if boundaries is not None else [])
        self._p = np.asarray(predictions if predictions is not None else [])

    @property
    def boundaries(self):
        return DenseVector(self._b)

    @property
    def predictions(self):
        return DenseVector(self._p)

    def _transform(self, dataset):
        fc, pc, fi = self.getFeaturesCol(), self.getPredictionCol(), self.getFeatureIndex()
        bt, pt = torch.tensor(self._b), torch.tensor(self._p)

        def fn(b, ctx):
            v = b.columns[fc].values
            x = (v[:, fi] if v.dim() == 2 else v).double()
            out = torch.from_numpy(np.interp(x.cpu().numpy(), bt.numpy(), pt.numpy())).to(x.device)
            return b.with_column(pc, ColumnData(out, T.DoubleType()))
        return dataset._new(MapPlan(dataset._plan, "IsotonicRegressionModel", fn))

    def _save_state(self):
        return {}, {"b": torch.tensor(self._b), "p": torch.tensor(self._p)}

    def _load_state(self, extra, tensors, stages):
        self._b, self._p = tensors["b"].numpy(), tensors["p"].numpy()


# ================================================= GeneralizedLinearRegression
# family -> (canonical link, links Spark accepts)
_GLM_LINKS = {
    "gaussian": ("identity", ("identity", "log", "inverse")),
    "binomial": ("logit", ("logit", "probit", "cloglog")),
    "poisson": ("log", ("log", "identity", "sqrt")),
    "gamma": ("inverse", ("inverse", "identity", "log")),
}
_GLM_POWER_LINKS = {0.0: "log", 1.0: "identity", -1.0: "inverse", 0.5: "sqrt"}
_GLM_POWER_FAMILIES = {0.0: "gaussian", 1.0: "poisson", 2.0: "gamma"}

_GLM_PARAMS = dict(_PRED, **{
    "family": ("The name of family which is a description of the error distribution to be used in the model. "
               "Supported options: gaussian (default), binomial, poisson, gamma and tweedie.", "gaussian",
               TC.toString),
    "link": ("The name of link function which provides the relationship between the linear predictor and the "
             "mean of the distribution function. Supported options: identity, log, inverse, logit, probit, "
             "cloglog and sqrt.", NO_DEFAULT, TC.toString),
    "variancePower": ("The power in the variance function of the Tweedie distribution which characterizes the "
                      "relationship between the variance and mean of the distribution. Only applicable for the "
                      "Tweedie family. Supported values: 0 and [1, Inf).", 0.0, TC.toFloat),
    "linkPower": ("The index in the power link function. Only applicable to the Tweedie family.", NO_DEFAULT,
                  TC.toFloat),
    "fitIntercept": ("whether to fit an intercept term", True, TC.toBoolean),
    "maxIter": ("max number of iterations (>= 0)", 25, TC.toInt),
    "tol": ("the convergence tolerance for iterative algorithms (>= 0)", 1e-6, TC.toFloat),
    "regParam": ("regularization parameter (>= 0)", 0.0, TC.toFloat),
    "weightCol": ("weight column name", None, TC.toString),
    "offsetCol": ("The offset column name. If this is not set or empty, we treat all instance offsets as 0.0",
                  None, TC.toString),
    "linkPredictionCol": ("link prediction (linear predictor) column name", None, TC.toString),
    "solver": ("The solver algorithm for optimization. Supported options: irls.", "irls", TC.toString),
    "aggregationDepth": ("suggested depth for treeAggregate (>= 2)", 2, TC.toInt),
})


def _glm_family_link(p):
    """(family, link, variancePower, linkPower) of an estimator / model as the K22 op names them.  Tweedie with
    variancePower 0 / 1 / 2 is the gaussian / poisson / gamma family and its power link 0 / 1 / -1 / 0.5 the
    log / identity / inverse / sqrt link, as in Spark."""
    family = p.getFamily().lower()
    if p.getSolver().lower() != "irls":
        raise IllegalArgumentException(f"GeneralizedLinearRegression solver must be irls, got {p.getSolver()}")
    if family == "tweedie":
        vp = float(p.getVariancePower())
        if not (vp == 0.0 or vp >= 1.0):
            raise IllegalArgumentException(
                f"GeneralizedLinearRegression variancePower must be 0 or in [1, Inf), got {vp}")
        lp = float(p.getLinkPower()) if p.isDefined("linkPower") else 1.0 - vp
        return _GLM_POWER_FAMILIES.get(vp, "tweedie"), _GLM_POWER_LINKS.get(lp, "power"), vp, lp
    if family not in _GLM_LINKS:
        raise IllegalArgumentException(
            f"GeneralizedLinearRegression family must be one of gaussian, binomial, poisson, gamma, tweedie, "
            f"got {p.getFamily()}")
    canonical, allowed = _GLM_LINKS[family]
    link = p.getLink().lower() if p.isDefined("link") else canonical
    if link not in allowed:
        raise IllegalArgumentException(
            f"Generalized Linear Regression with {family} family does not support {link} link function.")
    return family, link, 0.0, 0.0


def _glm_local(dataset, fc, lc, wc, oc):
    """This rank's (X, y, w, offset): X fp32, or fp64 for course-sized Double vectors; the rest fp64 or None.
    It is util.local_xyw(..., keep_f64=True) with one more column: the offset has to pass through the same
    null-label filter as the weights, and local_xyw returns (X, y, w) only.  Keep the two in step."""
    require_vector(dataset, fc)
    from .util import feature_dtype, require_numeric
    cols = [fc] + [c for c in (lc, wc, oc) if c]
    for c in cols[1:]:
        require_numeric(dataset, c)
    b = local_batch(dataset, cols)
    X = b.columns[fc].values
    want = feature_dtype(X)
    X = X if X.dtype == want else X.to(want)
    y = b.columns[lc].values.to(torch.float64) if lc else None
    w = b.columns[wc].values.to(torch.float64) if wc else None
    off = b.columns[oc].values.to(torch.float64) if oc else None
    keep = b.columns[lc].valid if lc else None
    if keep is not None and not bool(keep.all()):
        X, y = X[keep], y[keep]
        w = None if w is None else w[keep]
        off = None if off is None else off[keep]
    return X, y, w, off


def _glm_check_labels(family, vp, y, comm):
    """Labels outside the family's domain, from one min / max pass."""
    mm = torch.stack([y.min(), -y.max()]) if y.numel() else \
        torch.full((2,), float("inf"), dtype=torch.float64, device=y.device)
    comm.all_reduce(mm, "min")
    lo, hi = float(mm[0]), -float(mm[1])
    if lo > hi:
        return
    if family == "binomial" and (lo < 0.0 or hi > 1.0):
        raise IllegalArgumentException(f"The binomial family requires labels in [0, 1], found [{lo}, {hi}]")
    if (family == "poisson" or (family == "tweedie" and vp < 2.0)) and lo < 0.0:
        raise IllegalArgumentException(f"The {family} family requires labels >= 0, found {lo}")
    if (family == "gamma" or (family == "tweedie" and vp >= 2.0)) and lo <= 0.0:
        raise IllegalArgumentException(f"The {family} family requires labels > 0, found {lo}")


class GeneralizedLinearRegressionSummary:
    """Fit statistics of a GLM on a dataset (``model.evaluate``), from small fp64 passes over (y, mu, w)."""

    def __init__(self, predictions, model, data, comm, stats=None):
        self.predictions = predictions
        self.predictionCol = model.getPredictionCol()
        self._model = model
        self._X, self._y, self._w, self._off = data
        self._comm = comm
        self._fl = _glm_family_link(model)
        self._stats = stats          # [deviance, sum w, sum w y] of the fit's final EVAL step, when there was one
        self._cache = {}

    # ------------------------------------------------------------ pieces
    def _rows(self):
        """(y, w, offset, eta, mu) of this rank's rows, fp64, computed once."""
        if "rows" not in self._cache:
            fam, link, _, lp = self._fl
            m = self._model
            y = self._y
            w = torch.ones_like(y) if self._w is None else self._w
            off = torch.zeros_like(y) if self._off is None else self._off
            eta = off + m._intercept + K.matvec64(self._X, torch.tensor(m._coef, dtype=torch.float64))
            mu = K.glm_clamp(fam, K.glm_unlink(link, eta, lp))
            self._cache["rows"] = (y, w, off, eta, mu)
            self._X = None
        return self._cache["rows"]

    def _sum(self, *ts):
        acc = torch.stack([t.sum() for t in ts]).double()
        self._comm.all_reduce(acc)
        return [float(v) for v in acc.cpu()]

    def _basic(self):
        """[deviance, sum w, sum w y]."""
        if self._stats is None:
            fam, _, vp, _ = self._fl
            y, w, _, _, mu = self._rows()
            self._stats = self._sum(w * K.glm_unit_deviance(fam, y, mu, vp), w, w * y)
        return self._stats

    # ------------------------------------------------------------ fields
    @property
    def numInstances(self):
        if "n" not in self._cache:
            self._cache["n"] = int(self._comm.all_reduce_scalar(float(self._y.numel())))
        return self._cache["n"]

    @property
    def rank(self):
        return self._model.numFeatures + (1 if self._model.getFitIntercept() else 0)

    @property
    def degreesOfFreedom(self):
        return self.numInstances - self.rank

    @property
    def residualDegreeOfFreedom(self):
        return self.degreesOfFreedom

    @property
    def residualDegreeOfFreedomNull(self):
        return self.numInstances - (1 if self._model.getFitIntercept() else 0)

    @property
    def deviance(self):
        return self._basic()[0]

    @property
    def nullDeviance(self):
        if "null" not in self._cache:
            fam, link, vp, lp = self._fl
            y, w, off, _, _ = self._rows()
            m = self._model
            one = torch.ones(1, dtype=torch.float64, device=y.device)
            if not m.getFitIntercept():
                b = 0.0
            elif self._off is None:
                _, sw, swy = self._basic()
                b = float(K.glm_link(link, one * (swy / sw), lp)[0])
            else:
                # intercept-only IRLS with the offset, on the host formulation's row terms
                b, mode = 0.0, K.GLM_INIT
                for _ in range(max(m.getMaxIter(), 1) + 1):
                    _, _, W, z, _ = K.glm_row_terms(y, w, off, b * one, fam, link, vp, lp, mode)
                    swz, sw = self._sum(W * z, W)
                    nb = swz / sw
                    done = mode != K.GLM_INIT and abs(nb - b) < m.getTol()
                    b, mode = nb, K.GLM_STEP
                    if done:
                        break
            mu0 = K.glm_clamp(fam, K.glm_unlink(link, off + b, lp))
            self._cache["null"] = self._sum(w * K.glm_unit_deviance(fam, y, mu0, vp))[0]
        return self._cache["null"]

    def _pearson(self):
        fam, _, vp, _ = self._fl
        y, w, _, _, mu = self._rows()
        return (y - mu) * torch.sqrt(w) / torch.sqrt(K.glm_variance(fam, mu, vp))

    @property
    def dispersion(self):
        if "disp" not in self._cache:
            if self._fl[0] in ("binomial", "poisson"):
                self._cache["disp"] = 1.0
            else:
                r = self._pearson()
                self._cache["disp"] = self._sum(r * r)[0] / self.degreesOfFreedom
        return self._cache["disp"]

    @property
    def aic(self):
        if "aic" not in self._cache:
            fam = self._fl[0]
            y, w, _, _, mu = self._rows()
            dev, sw, _ = self._basic()
            n = self.numInstances
            if fam == "gaussian":
                ll = n * (math.log(dev / n * 2.0 * math.pi) + 1.0) + 2.0 - self._sum(torch.log(w))[0]
            elif fam == "binomial":
                nn = torch.round(w)
                k = torch.round(y * w)
                lp = (torch.lgamma(nn + 1) - torch.lgamma(k + 1) - torch.lgamma(nn - k + 1)
                      + torch.xlogy(k, mu) + torch.xlogy(nn - k, 1.0 - mu))
                ll = -2.0 * self._sum(torch.where(nn == 0, torch.zeros_like(lp), lp))[0]
            elif fam == "poisson":
                ll = -2.0 * self._sum(w * (torch.xlogy(y, mu) - mu - torch.lgamma(y + 1)))[0]
            elif fam == "gamma":
                disp = dev / sw
                a, scale = 1.0 / disp, mu * disp
                lp = (a - 1.0) * torch.log(y) - y / scale - a * torch.log(scale) - math.lgamma(a)
                ll = -2.0 * self._sum(w * lp)[0] + 2.0
            else:
                raise RuntimeError("No AIC available for the tweedie family")
            self._cache["aic"] = ll + 2.0 * self.rank
        return self._cache["aic"]

    def residuals(self, residualsType="deviance"):
        fam, link, vp, lp = self._fl
        y, w, _, _, mu = self._rows()
        if residualsType == "deviance":
            r = torch.sign(y - mu) * torch.sqrt((w * K.glm_unit_deviance(fam, y, mu, vp)).clamp_min(0.0))
        elif residualsType == "pearson":
            r = self._pearson()
        elif residualsType == "working":
            r = (y - mu) * K.glm_dlink(link, mu, lp)
        elif residualsType == "response":
            r = y - mu
        else:
            raise IllegalArgumentException(
                f"The residuals type {residualsType} is not supported by Generalized Linear Regression.")
        return self.predictions._session.createDataFrameFromLocalTensors({residualsType + "Residuals": r})


class GeneralizedLinearRegressionTrainingSummary(GeneralizedLinearRegressionSummary):
    def __init__(self, predictions, model, data, comm, stats, numIterations, solver, cov=None):
        super().__init__(predictions, model, data, comm, stats)
        self.numIterations = numIterations
        self.solver = solver
        self._cov = cov   # diag((X^T W X)^-1) of the last weighted least squares, intercept last; None: regParam > 0

    @property
    def coefficientStandardErrors(self):
        if self._cov is None:
            raise RuntimeError("No Std. Error of coefficients available for this GeneralizedLinearRegressionModel")
        return [math.sqrt(max(self.dispersion * v, 0.0)) for v in self._cov]

    @property
    def tValues(self):
        m = self._model
        vals = list(m._coef) + ([m._intercept] if m.getFitIntercept() else [])
        return [v / s if s > 0 else float("nan") for v, s in zip(vals, self.coefficientStandardErrors)]

    @property
    def pValues(self):
        from scipy import stats
        if self._fl[0] in ("binomial", "poisson"):
            return [float(2.0 * stats.norm.sf(abs(t))) for t in self.tValues]
        return [float(2.0 * stats.t.sf(abs(t), self.degreesOfFreedom)) for t in self.tValues]


class GeneralizedLinearRegression(Estimator):
    """IRLS, one fused pass over the features per iteration (K22 ``glm_step``): the step's (d+2)^2 weighted Gram and
    its scalars are all-reduced in one buffer and the weighted least squares is solved on the host by the solver
    LinearRegression's normal-equation path uses (standardised, L2 ``regParam``)."""
    _params = _GLM_PARAMS

    def __init__(self, labelCol=None, featuresCol=None, predictionCol=None, family=None, link=None,
                 fitIntercept=None, maxIter=None, tol=None, regParam=None, weightCol=None, solver=None,
                 linkPredictionCol=None, variancePower=None, linkPower=None, offsetCol=None, aggregationDepth=None):
        super().__init__()
        keyword_init(self, {k: v for k, v in locals().items() if k not in ("self", "__class__")})

    def _fit(self, dataset):
        fam, link, vp, lp = _glm_family_link(self)
        fc, lc = self.getFeaturesCol(), self.getLabelCol()
        wc, oc = self.getWeightCol() or None, self.getOffsetCol() or None
        X, y, w, off = _glm_local(dataset, fc, lc, wc, oc)
        comm = dataset._session.comm
        d = X.shape[1]
        dev = X.device
        _glm_check_labels(fam, vp, y, comm)
        fit_int = self.getFitIntercept()
        shift = shift_h = None
        zshift = 0.0
        one = torch.ones(1, dtype=torch.float64)
        if fit_int:
            # the features' shift and a first centre of the working response, from the leading rows: they only
            # condition the fp32 Gram, the solve un-shifts exactly
            sh = _lr_shift(X[:4096], y[:4096], comm, d).cpu()
            shift = sh[:d].float().to(dev)
            shift_h = sh[:d].float().double().numpy()
            z0 = K.glm_link(link, K.glm_clamp(fam, K.glm_init_mu(fam, one * float(sh[d]), one)), lp)
            zshift = float(z0[0]) if bool(torch.isfinite(z0[0])) else 0.0
        wls = LinearRegression(regParam=self.getRegParam(), elasticNetParam=0.0, fitIntercept=fit_int,
                               standardization=True)
        nG = (d + 2) * (d + 2)

        def step(coef, b, zs, mode, it):
            beta = None if coef is None else torch.tensor(coef, dtype=torch.float64, device=dev)
            G, st = K.glm_step(X, y, w, off, beta, b, shift, zs, fam, link, vp, lp, mode)
            buf = torch.cat([G.reshape(-1), st])
            comm.all_reduce(buf)
            host = buf.cpu().numpy()
            if host[nG + 3] > 0:
                raise RuntimeError(
                    f"GeneralizedLinearRegression (family {fam}, link {link}): {int(host[nG + 3])} rows have a "
                    f"non-finite mean, working weight or working response at iteration {it}; the fit diverged")
            return host[:nG].reshape(d + 2, d + 2), host[nG:]

        def solve(G, zs):
            coef, b = wls._solve(G, d, shift_h, float(np.float32(zs)) if fit_int else 0.0)[:2]
            return np.asarray(coef, np.float64), float(b)

        def centre(G, zs):
            # the weighted mean of the working response: the next step's zshift
            return float(np.float32(zs)) + G[d + 1, d] / G[d, d] if fit_int and G[d, d] > 0 else 0.0

        zs = zshift
        G, _ = step(None, 0.0, zs, K.GLM_INIT, 0)
        coef, b = solve(G, zs)
        iters = 0
        if not (fam == "gaussian" and link == "identity"):
            tol, max_iter = self.getTol(), self.getMaxIter()
            while iters < max_iter:
                zs = centre(G, zs)
                G, _ = step(coef, b, zs, K.GLM_STEP, iters + 1)
                ncoef, nb = solve(G, zs)
                iters += 1
                delta = max(float(np.max(np.abs(ncoef - coef))) if d else 0.0, abs(nb - b))
                coef, b = ncoef, nb
                if delta < tol:
                    break
        _, st = step(coef, b, 0.0, K.GLM_EVAL, iters)
        model = GeneralizedLinearRegressionModel(coef, b)
        model._post_fit(self)
        cov = self._cov_diag(G, d, shift_h, fit_int) if self.getRegParam() == 0.0 else None
        model.summary = GeneralizedLinearRegressionTrainingSummary(
            model.transform(dataset), model, (X, y, w, off), comm, [float(v) for v in st[:3]], iters,
            self.getSolver(), cov)
        return model

    @staticmethod
    def _cov_diag(G, d, shift, fit_int):
        """diag((X^T W X)^-1) in uncentred coordinates (intercept last) from the shifted Gram: [x | 1] =
        [x - s | 1] T with T = [[I, 0], [s^T, 1]], so X^T W X = T^T G T."""
        k = d + 1 if fit_int else d
        M = np.array(G[:k, :k], dtype=np.float64)
        if fit_int and shift is not None:
            Tm = np.eye(k)
            Tm[d, :d] = shift
            M = Tm.T @ M @ Tm
        try:
            return list(np.diag(np.linalg.inv(M)))
        except np.linalg.LinAlgError:
            return None


class GeneralizedLinearRegressionModel(Model):
    _params = _GLM_PARAMS

    def __init__(self, coefficients=None, intercept=0.0):
        super().__init__()
        self._coef = np.asarray(coefficients if coefficients is not None else [], dtype=np.float64)
        self._intercept = float(intercept)
        self.summary = None

    @property
    def coefficients(self):
        return DenseVector(self._coef)

    @property
    def intercept(self):
        return self._intercept

    @property
    def numFeatures(self):
        return len(self._coef)

    @property
    def hasSummary(self):
        return self.summary is not None

    def predict(self, features):
        fam, link, _, lp = _glm_family_link(self)
        x = features.toArray() if hasattr(features, "toArray") else np.asarray(features)
        eta = torch.tensor([float(x @ self._coef + self._intercept)], dtype=torch.float64)
        return float(K.glm_clamp(fam, K.glm_unlink(link, eta, lp))[0])

    def _transform(self, dataset):
        fam, link, _, lp = _glm_family_link(self)
        fc, pc = self.getFeaturesCol(), self.getPredictionCol()
        lpc, oc = self.getLinkPredictionCol() or None, self.getOffsetCol() or None
        require_vector(dataset, fc)
        coef = torch.tensor(self._coef, dtype=torch.float64)
        icpt = self._intercept

        def fn(b, ctx):
            X = b.columns[fc].values
            eta = K.matvec64(X, coef) + icpt
            if oc:
                eta = eta + b.columns[oc].values.to(torch.float64)
            mu = K.glm_clamp(fam, K.glm_unlink(link, eta, lp))
            out = b.with_column(pc, ColumnData(mu, T.DoubleType(), b.columns[fc].valid))
            if lpc:
                out = out.with_column(lpc, ColumnData(eta, T.DoubleType(), b.columns[fc].valid))
            return out
        return dataset._new(MapPlan(dataset._plan, f"GeneralizedLinearRegressionModel -> {pc}", fn))

    def evaluate(self, dataset):
        data = _glm_local(dataset, self.getFeaturesCol(), self.getLabelCol(), self.getWeightCol() or None,
                          self.getOffsetCol() or None)
        return GeneralizedLinearRegressionSummary(self.transform(dataset), self, data, dataset._session.comm)

    def _save_state(self):
        return {"intercept": self._intercept}, {"coefficients": torch.tensor(self._coef)}

    def _load_state(self, extra, tensors, stages):
        self._coef = tensors["coefficients"].numpy()
        self._intercept = float(extra["intercept"])
        self.summary = None

    def __repr__(self):
        return f"GeneralizedLinearRegressionModel: uid={self.uid}, family={self.getFamily()}, " \
               f"numFeatures={self.numFeatures}"


# ============================================================ factorization machines
_FM_PARAMS = dict(_PRED, **{
    "factorSize": ("Dimensionality of the factor vectors, which are used to get pairwise interactions between "
                   "variables", 8, TC.toInt),
    "fitIntercept": ("whether to fit an intercept term", True, TC.toBoolean),
    "fitLinear": ("whether to fit linear term (aka 1-way term)", True, TC.toBoolean),
    "regParam": ("regularization parameter (>= 0)", 0.0, TC.toFloat),
    "miniBatchFraction": ("fraction of the input data set that should be used for one iteration of gradient "
                          "descent, in range (0, 1]", 1.0, TC.toFloat),
    "initStd": ("standard deviation of initial coefficients", 0.01, TC.toFloat),
    "maxIter": ("max number of iterations (>= 0)", 100, TC.toInt),
    "stepSize": ("Step size to be used for each iteration of optimization (>= 0).", 1.0, TC.toFloat),
    "tol": ("the convergence tolerance for iterative algorithms (>= 0)", 1e-6, TC.toFloat),
    "solver": ("The solver algorithm for optimization. Supported options: gd, adamW.", "adamW", TC.toString),
    "seed": ("random seed", None, TC.toInt),
})


def fm_initial_params(d: int, k: int, fit_linear: bool, fit_intercept: bool, init_std: float, seed: int) -> np.ndarray:
    """V ~ N(0, initStd^2), w = 0, b = 0 in Spark's flat layout.  The normals are numpy's, drawn on the host from the
    seed: the same on every device and number of ranks, but not the JVM's stream."""
    theta = np.zeros(K.fm_num_params(d, k, fit_linear, fit_intercept))
    theta[:d * k] = np.random.default_rng(int(seed) & 0xFFFFFFFFFFFFFFFF).normal(0.0, init_std, d * k)
    return theta


def fm_update_gd(theta, g, i: int, step_size: float, reg_param: float):
    """Spark's SquaredL2Updater at iteration i (from 1): eta = stepSize / sqrt(i)."""
    eta = step_size / math.sqrt(i)
    return theta * (1.0 - eta * reg_param) - eta * g


def fm_update_adamw(theta, g, state, i: int, step_size: float, reg_param: float):
    """Spark's AdamWUpdater at iteration i (from 1); ``state`` holds the two moment vectors and is updated."""
    b1, b2, eps = 0.9, 0.999, 1e-8
    state["m"] = b1 * state["m"] + (1.0 - b1) * g
    state["v"] = b2 * state["v"] + (1.0 - b2) * g * g
    mh = state["m"] / (1.0 - b1 ** i)
    vh = state["v"] / (1.0 - b2 ** i)
    return theta - (step_size * mh / (np.sqrt(vh) + eps) + reg_param * theta)


def fm_converged(prev, cur, tol: float) -> bool:
    """GradientDescent.isConverged: |prev - cur|_2 < tol max(|cur|_2, 1)."""
    return float(np.linalg.norm(prev - cur)) < tol * max(float(np.linalg.norm(cur)), 1.0)


def _fm_fit(est, dataset, loss: int, check_labels=None):
    """GradientDescent.runMiniBatchSGD on the host in fp64: every iteration is one ``K.fm_step`` over the local rows
    plus one all-reduce of P + 2 doubles.  Returns (theta, d, per-iteration [mean loss, selected count])."""
    solver, frac = est.getSolver(), est.getMiniBatchFraction()
    if solver not in ("gd", "adamW"):
        raise IllegalArgumentException(f"{type(est).__name__} solver must be gd or adamW, got {solver}")
    if not 0.0 < frac <= 1.0:
        raise IllegalArgumentException(f"{type(est).__name__} miniBatchFraction must be in (0, 1], got {frac}")
    k = est.getFactorSize()
    if k < 1:
        raise IllegalArgumentException(f"{type(est).__name__} factorSize must be >= 1, got {k}")
    lin, icpt = est.getFitLinear(), est.getFitIntercept()
    X, y, _ = local_xyw(dataset, est.getFeaturesCol(), est.getLabelCol(), None, keep_f64=True)
    session = dataset._session
    comm = session.comm
    n = X.shape[0]
    dd = torch.tensor([float(X.shape[1]) if n else 0.0], dtype=torch.float64, device=comm.device)
    comm.all_reduce(dd, "max")
    d = int(dd)
    if n == 0:
        X = torch.zeros((0, d), dtype=X.dtype, device=X.device)
    if check_labels is not None:
        check_labels(y, comm)          # global: every rank raises, or none does
    off = global_offset(session, n)
    seed = est.getSeed() if est.getSeed() is not None else _default_seed(type(est))
    theta = fm_initial_params(d, k, lin, icpt, est.getInitStd(), seed)
    P = len(theta)
    state = {"m": np.zeros(P), "v": np.zeros(P)}
    step, reg, tol = est.getStepSize(), est.getRegParam(), est.getTol()
    hist, updates = [], 0
    for i in range(1, est.getMaxIter() + 1):
        ls, g, cnt = K.fm_step(X, y, theta, k, loss, K.FM_STEP, lin, icpt,
                               sample=(seed + i, off, frac) if frac < 1.0 else None)
        acc = torch.cat([g, ls.reshape(1), cnt.reshape(1)])
        comm.all_reduce(acc)
        a = acc.cpu().numpy()
        c = float(a[P + 1])
        hist.append([a[P] / c if c > 0 else 0.0, c])
        if c == 0:
            continue
        gm = a[:P] / c
        new = fm_update_gd(theta, gm, i, step, reg) if solver == "gd" else \
            fm_update_adamw(theta, gm, state, i, step, reg)
        prev, theta = theta, new
        updates += 1
        if updates >= 2 and fm_converged(prev, theta, tol):
            break
    return theta, d, hist


class _FMModel(Model):
    """The parameters of a fitted factorization machine and its raw prediction."""

    def __init__(self, theta=None, numFeatures=0, factorSize=None, fitLinear=True, fitIntercept=True):
        super().__init__()
        self._theta = np.asarray(theta if theta is not None else np.zeros(0), dtype=np.float64).reshape(-1)
        self._d = int(numFeatures)
        self._shape = (int(factorSize) if factorSize is not None else 0, bool(fitLinear), bool(fitIntercept))
        self._prep = None
        self.fitHistory = []      # per iteration [mean loss over the selected rows, selected rows]

    @property
    def numFeatures(self):
        return self._d

    def _parts(self):
        k, lin, icpt = self._shape
        return K.fm_unpack(torch.from_numpy(self._theta), self._d, k, lin, icpt)

    @property
    def intercept(self):
        return float(self._parts()[2])

    @property
    def linear(self):
        return DenseVector(self._parts()[1].numpy().copy())

    @property
    def factors(self):
        return DenseMatrix(self._d, self._shape[0], self._parts()[0].numpy().reshape(-1).copy(), True)

    def _prepared(self):
        if self._prep is None:   # the device tables are built once per model, not per batch
            self._prep = K.FmPrepared(self._theta, self._d, *self._shape)
        return self._prep

    def _raw(self, X: torch.Tensor) -> torch.Tensor:
        k, lin, icpt = self._shape
        if X.shape[0] == 0:
            return torch.zeros(0, dtype=torch.float64, device=X.device)
        X = X if feature_dtype(X) == torch.float64 else X.float()
        return K.fm_step(X, None, self._theta, k, mode=K.FM_PREDICT, fit_linear=lin, fit_intercept=icpt,
                         prepared=self._prepared())

    def _raw_one(self, features) -> float:
        x = np.asarray(features.toArray() if hasattr(features, "toArray") else features, dtype=np.float64)
        return float(self._raw(torch.from_numpy(x.reshape(1, -1).copy()))[0])

    def _save_state(self):
        k, lin, icpt = self._shape
        return {"numFeatures": self._d, "factorSize": k, "fitLinear": lin, "fitIntercept": icpt}, \
            {"theta": torch.tensor(self._theta)}

    def _load_state(self, extra, tensors, stages):
        self._theta = tensors["theta"].numpy()
        self._d = int(extra["numFeatures"])
        self._shape = (int(extra["factorSize"]), bool(extra["fitLinear"]), bool(extra["fitIntercept"]))
        self._prep = None
        self.fitHistory = []


class FMRegressor(Estimator):
    """``pyspark.ml.regression.FMRegressor``: a factorization machine with the squared loss, fitted by Spark's
    minibatch gradient descent (``solver`` "gd" or "adamW").  Every iteration is one pass of the K25 ``fm_step`` op
    over the local rows plus one all-reduce of P + 2 doubles; ``miniBatchFraction`` selects rows by a Philox draw
    keyed by the global row id, so a fit does not depend on the number of ranks.  The initial factors follow Spark's
    N(0, initStd^2) but come from numpy's generator, not the JVM's.  There is no ``weightCol`` (Spark has none), and
    no training summary."""
    _params = _FM_PARAMS

    def __init__(self, **kwargs):
        super().__init__()
        keyword_init(self, kwargs)

    def _fit(self, dataset):
        theta, d, hist = _fm_fit(self, dataset, K.FM_SQUARED)
        model = FMRegressionModel(theta, d, self.getFactorSize(), self.getFitLinear(), self.getFitIntercept())
        model._post_fit(self)
        model.fitHistory = hist
        return model


class FMRegressionModel(_FMModel):
    _params = _FM_PARAMS

    def predict(self, features):
        return self._raw_one(features)

    def _transform(self, dataset):
        fc, pc = self.getFeaturesCol(), self.getPredictionCol()
        require_vector(dataset, fc)

        def fn(b, ctx):
            return b.with_column(pc, ColumnData(self._raw(b.columns[fc].values), T.DoubleType(),
                                                b.columns[fc].valid))
        return dataset._new(MapPlan(dataset._plan, f"FMRegressionModel -> {pc}", fn))

    def __repr__(self):
        return f"FMRegressionModel: uid={self.uid}, numFeatures={self.numFeatures}, factorSize={self._shape[0]}"


# ============================================================ AFT survival regression
_AFT_PARAMS = dict(_PRED, **{
    "censorCol": ("censor column name. The value of this column could be 0 or 1. If the value is 1, it means the "
                  "event has occurred i.e. uncensored; otherwise censored.", "censor", TC.toString),
    "quantileProbabilities": ("quantile probabilities array. Values of the quantile probabilities array should be "
                              "in the range (0, 1) and the array should be non-empty.",
                              [0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99], TC.toListFloat),
    "quantilesCol": ("quantiles column name. This column will output quantiles of corresponding "
                     "quantileProbabilities if it is set.", None, TC.toString),
    "fitIntercept": ("whether to fit an intercept term", True, TC.toBoolean),
    "maxIter": ("max number of iterations (>= 0)", 100, TC.toInt),
    "tol": ("the convergence tolerance for iterative algorithms (>= 0)", 1e-6, TC.toFloat),
    "aggregationDepth": ("suggested depth for treeAggregate (>= 2)", 2, TC.toInt),
    "maxBlockSizeInMB": ("maximum memory in MB for stacking input data into blocks", 0.0, TC.toFloat),
})


def _aft_probs(stage):
    """The stage's quantileProbabilities, checked: non-empty, every value in (0, 1)."""
    probs = [float(p) for p in stage.getQuantileProbabilities()]
    if not probs or not all(0.0 < p < 1.0 for p in probs):
        raise IllegalArgumentException(f"{type(stage).__name__} quantileProbabilities must be a non-empty array of "
                                       f"values in the range (0, 1), got {probs}")
    return probs


class AFTSurvivalRegression(Estimator):
    """``pyspark.ml.regression.AFTSurvivalRegression``: the Weibull accelerated failure time model, fitted as Spark
    fits it: no weights and no regularisation, the features scaled by their unbiased std (not centred) and the
    coefficients scaled back, L-BFGS from the all-zero point (``optim.minimize``).  Every evaluation is one pass of
    the K26 ``aft_step`` op over the local rows plus one all-reduce of d + 4 doubles.  The first evaluation also
    validates the rows: there e^eps = t, so a row the op reports as bad has a label that is not positive and finite,
    a censor other than 0 / 1 or a non-finite feature.  At a later point a bad row means e^eps overflowed: the
    evaluation is +inf and the line search shortens the step.  ``aggregationDepth`` and ``maxBlockSizeInMB`` are
    accepted and unused.  Spark has no training summary for this model, and there is none here."""
    _params = _AFT_PARAMS

    def __init__(self, **kwargs):
        super().__init__()
        keyword_init(self, kwargs)
        _aft_probs(self)

    def _fit(self, dataset):
        from .optim import minimize
        from .util import centered_gram
        _aft_probs(self)
        X, y, cens = local_xyw(dataset, self.getFeaturesCol(), self.getLabelCol(), self.getCensorCol(),
                               keep_f64=True)
        session = dataset._session
        comm = session.comm
        n_loc = X.shape[0]
        dd = torch.tensor([float(X.shape[1]) if n_loc else 0.0], dtype=torch.float64, device=comm.device)
        comm.all_reduce(dd, "max")
        d = int(dd)
        if n_loc == 0:
            X = torch.zeros((0, d), dtype=X.dtype, device=X.device)
        n = global_count(session, n_loc)
        if n == 0:
            raise IllegalArgumentException("AFTSurvivalRegression: the training frame has no rows")
        logt = torch.log(y)            # once per fit; t <= 0 or NaN gives a non-finite value: a bad row
        _, _, Cg = centered_gram(X, comm)
        sd = np.sqrt(np.clip(torch.diagonal(Cg).cpu().numpy(), 0, None) / max(n - 1, 1))
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(sd > 0, 1.0 / sd, 0.0)     # a zero-std feature takes no part, as in Spark
        fit_int = self.getFitIntercept()
        evals = [0]

        def fg(theta):
            b0 = theta[d] if fit_int else 0.0
            ls, g, bad = K.aft_step(X, logt, cens, theta[:d] * inv, b0, theta[d + 1])
            acc = torch.cat([g, ls.reshape(1), bad.reshape(1)])
            comm.all_reduce(acc)
            a = acc.cpu().numpy()
            evals[0] += 1
            if a[d + 3] > 0:
                if evals[0] == 1:
                    raise IllegalArgumentException(
                        f"AFTSurvivalRegression: {int(a[d + 3])} rows are invalid: the label must be positive and "
                        f"finite, the censor 0 or 1 and every feature finite")
                return float("inf"), np.zeros(d + 2)
            grad = a[:d + 2] / n
            grad[:d] *= inv
            if not fit_int:
                grad[d] = 0.0
            return a[d + 2] / n, grad

        theta, _, _ = minimize(fg, np.zeros(d + 2), self.getMaxIter(), self.getTol())
        model = AFTSurvivalRegressionModel(theta[:d] * inv, theta[d] if fit_int else 0.0, theta[d + 1])
        model._post_fit(self)
        return model


class AFTSurvivalRegressionModel(Model):
    _params = _AFT_PARAMS

    def __init__(self, coefficients=None, intercept=0.0, logScale=0.0):
        super().__init__()
        self._coef = np.asarray(coefficients if coefficients is not None else [], dtype=np.float64).reshape(-1)
        self._intercept = float(intercept)
        self._log_scale = float(logScale)

    @property
    def coefficients(self):
        return DenseVector(self._coef)

    @property
    def intercept(self):
        return self._intercept

    @property
    def scale(self):
        return math.exp(self._log_scale)

    @property
    def numFeatures(self):
        return len(self._coef)

    def predict(self, features):
        x = np.asarray(features.toArray() if hasattr(features, "toArray") else features, dtype=np.float64)
        return float(np.exp(x @ self._coef + self._intercept))

    def predictQuantiles(self, features):
        return DenseVector(self.predict(features) * K.aft_quantile_factors(_aft_probs(self), self._log_scale))

    def _transform(self, dataset):
        fc, pc, qc = self.getFeaturesCol(), self.getPredictionCol(), self.getQuantilesCol() or None
        require_vector(dataset, fc)
        probs = _aft_probs(self) if qc else None

        def fn(b, ctx):
            X = b.columns[fc].values
            X = X if feature_dtype(X) == torch.float64 else X.float()
            res = K.aft_step(X, None, None, self._coef, self._intercept, self._log_scale, K.AFT_PREDICT, probs)
            valid = b.columns[fc].valid
            if not qc:
                return b.with_column(pc, ColumnData(res, T.DoubleType(), valid))
            out = b.with_column(pc, ColumnData(res[0], T.DoubleType(), valid))
            return out.with_column(qc, ColumnData(res[1], T.VectorUDT(), valid))
        return dataset._new(MapPlan(dataset._plan, f"AFTSurvivalRegressionModel -> {pc}", fn))

    def _save_state(self):
        return {"intercept": self._intercept, "logScale": self._log_scale}, {"coefficients": torch.tensor(self._coef)}

    def _load_state(self, extra, tensors, stages):
        self._coef = tensors["coefficients"].numpy()
        self._intercept = float(extra["intercept"])
        self._log_scale = float(extra["logScale"])

    def __repr__(self):
        return f"AFTSurvivalRegressionModel: uid={self.uid}, numFeatures={self.numFeatures}"
