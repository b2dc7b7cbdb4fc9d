"""Clustering: distributed k-means and Gaussian mixtures.

Each Lloyd iteration = one pass of the K10 ``kmeans_step`` HIP kernel
(nearest-centre assignment + LDS-privatised per-centre sums) and one RCCL
all-reduce of k*(d+1) doubles — the map → reduce → communicate pattern of
MLE 02 - K-Means.py:178-204.  ``maxIter=0`` returns the initial centres
(MLE 02:46-68).  Initialisation: k-means++ over a global sample
("k-means||" default) or random points, both seeded.

``GaussianMixture`` is EM for a full-covariance mixture: each iteration is one pass of the K23 ``gmm_step`` op
(responsibilities and centred moment sums, both on the fp32 MFMA), one all-reduce of k (d+1)^2 + 3 doubles and an
M-step on the host in fp64.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K
from ..sql import types as T
from ..sql.batch import ColumnData
from ..sql.dataframe import MapPlan
from .base import Estimator, Model
from .linalg import DenseMatrix, DenseVector
from .param import NO_DEFAULT, TypeConverters as TC, keyword_init
from .regression import _default_seed
from .util import VECTOR_F64_MAX, IllegalArgumentException, global_count, global_offset, local_xyw, require_vector


class KMeans(Estimator):
    _params = {
        "featuresCol": ("features column name", "features", TC.toString),
        "predictionCol": ("prediction column name", "prediction", TC.toString),
        "k": ("The number of clusters to create. Must be > 1.", 2, TC.toInt),
        "initMode": ("The initialization algorithm: 'random' or 'k-means||'", "k-means||", TC.toString),
        "initSteps": ("The number of steps for k-means|| initialization mode. Must be > 0.", 2, TC.toInt),
        "tol": ("the convergence tolerance for iterative algorithms (>= 0)", 1e-4, TC.toFloat),
        "maxIter": ("max number of iterations (>= 0)", 20, TC.toInt),
        "seed": ("random seed", None, TC.toInt),
        "distanceMeasure": ("'euclidean' or 'cosine'", "euclidean", TC.toString),
        "weightCol": ("weight column name", None, TC.toString),
    }

    def __init__(self, **kwargs):
        super().__init__()
        keyword_init(self, kwargs)

    def _init_centres(self, session, X, k, seed):
        comm = session.comm
        n = X.shape[0]
        ng = global_count(session, n)
        off = global_offset(session, n)
        target = min(ng, max(20 * k, 10000))
        frac = min(1.0, target / max(ng, 1))
        u = K.uniform(n, seed, off, 21, device=X.device)
        samp = X[u < frac] if frac < 1 else X
        if comm.distributed:
            samp = torch.cat(comm.all_gather_varlen(samp.contiguous()))
        S = samp.double().cpu().numpy()
        rng = np.random.default_rng(seed)
        if len(S) == 0:
            return np.zeros((k, X.shape[1]))
        if self.getInitMode() == "random":
            idx = rng.choice(len(S), size=min(k, len(S)), replace=False)
            C = S[idx]
        else:  # k-means++ on the global sample (deterministic given seed)
            C = [S[rng.integers(len(S))]]
            d2 = ((S - C[0]) ** 2).sum(1)
            for _ in range(1, k):
                p = d2 / d2.sum() if d2.sum() > 0 else np.full(len(S), 1.0 / len(S))
                C.append(S[rng.choice(len(S), p=p)])
                d2 = np.minimum(d2, ((S - C[-1]) ** 2).sum(1))
            C = np.array(C)
        if len(C) < k:
            C = np.vstack([C, np.repeat(C[-1:], k - len(C), 0)])
        return C

    def _fit(self, dataset):
        fc = self.getFeaturesCol()
        X, _, w = local_xyw(dataset, fc, None, self.getWeightCol(), keep_f64=True)
        session = dataset._session
        comm = session.comm
        seed = self.getSeed() if self.getSeed() is not None else _default_seed(type(self))
        k = self.getK()
        cosine = self.getDistanceMeasure() == "cosine"
        if cosine:
            X = X / torch.linalg.vector_norm(X, dim=1, keepdim=True).clamp_min(1e-30)
        C = self._init_centres(session, X, k, seed)
        cost = float("nan")
        it = 0
        for it in range(self.getMaxIter()):
            Ct = torch.tensor(C, dtype=X.dtype, device=X.device)
            _, sums, counts, c = K.kmeans_step(X, Ct)
            acc = torch.cat([sums.reshape(-1), counts, c.reshape(1)])
            comm.all_reduce(acc)
            a = acc.cpu().numpy()
            S = a[: k * X.shape[1]].reshape(k, -1)
            N = a[k * X.shape[1]: k * X.shape[1] + k]
            newC = np.where(N[:, None] > 0, S / np.maximum(N, 1)[:, None], C)
            if cosine:
                newC = newC / np.maximum(np.linalg.norm(newC, axis=1, keepdims=True), 1e-30)
            moved = np.sqrt(((newC - C) ** 2).sum(1)).max()
            C = newC
            if moved <= self.getTol():
                it += 1
                break
        # final cost / sizes with the final centres
        Ct = torch.tensor(C, dtype=X.dtype, device=X.device)
        assign, _, counts, c = K.kmeans_step(X, Ct)
        acc = torch.cat([counts, c.reshape(1)])
        comm.all_reduce(acc)
        a = acc.cpu().numpy()
        model = KMeansModel(C)
        model._post_fit(self)
        model.summary = KMeansSummary(model, dataset, a[:k].astype(np.int64).tolist(), float(a[k]),
                                      self.getMaxIter() if self.getMaxIter() == 0 else it)
        return model


class KMeansSummary:
    def __init__(self, model, dataset, sizes, cost, iters):
        self._model = model
        self._dataset = dataset
        self.clusterSizes = sizes
        self.trainingCost = cost
        self.numIter = iters
        self.k = len(sizes)
        self.featuresCol = model.getFeaturesCol()
        self.predictionCol = model.getPredictionCol()

    @property
    def predictions(self):
        return self._model.transform(self._dataset)

    @property
    def cluster(self):
        return self.predictions.select(self.predictionCol)


class KMeansModel(Model):
    _params = KMeans._params

    def __init__(self, centers=None):
        super().__init__()
        self._C = np.asarray(centers if centers is not None else np.zeros((0, 0)), dtype=np.float64)
        self.summary = None

    def clusterCenters(self):
        return [c.copy() for c in self._C]

    @property
    def hasSummary(self):
        return self.summary is not None

    def predict(self, features):
        x = np.asarray(features.toArray() if hasattr(features, "toArray") else features)
        return int(np.argmin(((self._C - x) ** 2).sum(1)))

    def computeCost(self, dataset):
        X, _, _ = local_xyw(dataset, self.getFeaturesCol(), keep_f64=True)
        _, _, _, c = K.kmeans_step(X, torch.tensor(self._C, dtype=X.dtype, device=X.device), with_sums=False)
        t = torch.tensor([float(c)], dtype=torch.float64, device=dataset._session.comm.device)
        dataset._session.comm.all_reduce(t)
        return float(t)

    def _transform(self, dataset):
        fc, pc = self.getFeaturesCol(), self.getPredictionCol()
        require_vector(dataset, fc)
        Cd = torch.tensor(self._C, dtype=torch.float64)
        cosine = self.getDistanceMeasure() == "cosine"

        def fn(b, ctx):
            X = b.columns[fc].values
            X = X if X.dtype == torch.float64 else X.float()   # Double vectors: fp64 distances (kernel <double>)
            if cosine:
                X = X / torch.linalg.vector_norm(X, dim=1, keepdim=True).clamp_min(1e-30)
            if X.shape[0] == 0:
                a = torch.zeros(0, dtype=torch.int32, device=X.device)
            else:
                a, _, _, _ = K.kmeans_step(X, Cd.to(X.device, X.dtype), with_sums=False)
            return b.with_column(pc, ColumnData(a.to(torch.int32), T.IntegerType()))
        return dataset._new(MapPlan(dataset._plan, "KMeansModel", fn))

    def _save_state(self):
        return {}, {"centers": torch.tensor(self._C)}

    def _load_state(self, extra, tensors, stages):
        self._C = tensors["centers"].numpy()
        self.summary = None


class BisectingKMeans(KMeans):
    """Divisive k-means: repeatedly split the largest cluster with 2-means."""
    _params = dict(KMeans._params, minDivisibleClusterSize=("min points in a divisible cluster", 1.0, TC.toFloat))

    def _fit(self, dataset):
        fc = self.getFeaturesCol()
        X, _, _ = local_xyw(dataset, fc, keep_f64=True)
        session = dataset._session
        comm = session.comm
        seed = self.getSeed() if self.getSeed() is not None else _default_seed(type(self))
        centers = [None]
        mean = X.double().sum(0)
        cnt = torch.tensor([float(X.shape[0])], dtype=torch.float64, device=X.device)
        comm.all_reduce_many([mean, cnt])
        centers = [(mean / cnt).cpu().numpy()]
        rng = np.random.default_rng(seed)
        while len(centers) < self.getK():
            C = np.array(centers)
            assign, _, counts, _ = K.kmeans_step(X, torch.tensor(C, dtype=X.dtype, device=X.device))
            comm.all_reduce(counts)
            big = int(torch.argmax(counts))
            sub = X[assign.long() == big]
            base = centers[big]
            jitter = rng.normal(scale=1e-3, size=base.shape) * (np.abs(base) + 1)
            pair = np.stack([base + jitter, base - jitter])
            for _ in range(self.getMaxIter()):
                _, s2, c2, _ = K.kmeans_step(sub, torch.tensor(pair, dtype=X.dtype, device=X.device))
                acc = torch.cat([s2.reshape(-1), c2])
                comm.all_reduce(acc)
                a = acc.cpu().numpy()
                S2, N2 = a[: 2 * X.shape[1]].reshape(2, -1), a[2 * X.shape[1]:]
                newp = np.where(N2[:, None] > 0, S2 / np.maximum(N2, 1)[:, None], pair)
                if np.abs(newp - pair).max() < self.getTol():
                    pair = newp
                    break
                pair = newp
            centers = centers[:big] + [pair[0], pair[1]] + centers[big + 1:]
        model = KMeansModel(np.array(centers))
        model._post_fit(self)
        return model


# ======================================================================================= GaussianMixture
class MultivariateGaussian:
    """``pyspark.ml.stat.distribution.MultivariateGaussian``: a mean vector and a covariance matrix."""

    def __init__(self, mean, cov):
        self.mean = mean if isinstance(mean, DenseVector) else DenseVector(np.asarray(mean, dtype=np.float64))
        if not isinstance(cov, DenseMatrix):
            c = np.asarray(cov, dtype=np.float64)
            cov = DenseMatrix(c.shape[0], c.shape[1], c.T.reshape(-1))
        self.cov = cov

    def __repr__(self):
        return f"MultivariateGaussian(mean={self.mean!r}, cov={self.cov!r})"


def gmm_tables(weights, means, covs):
    """(A [k, d, d], logc [k]) of ``K.gmm_step`` from the mixture's parameters, numpy fp64: A_j = D^-1/2 U^T over
    the eigenpairs Spark's pseudo-inverse keeps (eigenvalue > eps d max eigenvalue; the dropped rows are zero),
    logc_j = log pi_j - (d log 2 pi + log pdet Sigma_j) / 2."""
    k, d = means.shape
    A = np.zeros((k, d, d))
    logc = np.zeros(k)
    for j in range(k):
        vals, vecs = np.linalg.eigh(covs[j])
        tol = K.GMM_EPS * d * vals.max()
        keep = vals > tol
        if not keep.any():
            raise ValueError(f"GaussianMixture: the covariance matrix of component {j} has no non-zero singular "
                             f"values")
        m = int(keep.sum())
        A[j, :m] = vecs[:, keep].T / np.sqrt(vals[keep])[:, None]
        with np.errstate(divide="ignore"):
            logc[j] = np.log(weights[j]) - 0.5 * (d * np.log(2.0 * np.pi) + np.log(vals[keep]).sum())
    return A, logc


def _gmm_call(X, w, weights, means, covs, mode):
    A, logc = gmm_tables(weights, means, covs)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return K.gmm_step(X, w, t(means), t(A), t(logc), mode)


_GMM_PARAMS = {
    "featuresCol": ("features column name", "features", TC.toString),
    "predictionCol": ("prediction column name", "prediction", TC.toString),
    "probabilityCol": ("Column name for predicted class conditional probabilities.", "probability", TC.toString),
    "k": ("Number of independent Gaussians in the mixture model. Must be > 1.", 2, TC.toInt),
    "maxIter": ("max number of iterations (>= 0)", 100, TC.toInt),
    "tol": ("the convergence tolerance for iterative algorithms (>= 0)", 0.01, TC.toFloat),
    "seed": ("random seed", None, TC.toInt),
    "aggregationDepth": ("suggested depth for treeAggregate (>= 2)", 2, TC.toInt),
    "weightCol": ("weight column name", None, TC.toString),
}


class GaussianMixture(Estimator):
    """EM for a mixture of full-covariance Gaussians (``pyspark.ml.clustering.GaussianMixture``): Spark's
    initialisation, densities (pseudo-inverse of a singular covariance, EPSILON added to every density) and
    stopping rule (absolute change of the total log-likelihood below ``tol``)."""
    _params = _GMM_PARAMS

    def __init__(self, featuresCol=None, predictionCol=None, k=None, probabilityCol=None, tol=None, maxIter=None,
                 seed=None, aggregationDepth=None, weightCol=None):
        super().__init__()
        keyword_init(self, {k_: v for k_, v in locals().items() if k_ not in ("self", "__class__")})

    def _init_state(self, session, X, k, seed):
        """Spark's scheme on a seeded global sample (made as KMeans._init_centres makes its sample, so it is the
        same at any rank count): 5 k rows drawn with replacement, component j gets the mean and the diagonal
        variance of its 5 rows and weight 1 / k."""
        comm = session.comm
        n = X.shape[0]
        ng = global_count(session, n)
        off = global_offset(session, n)
        if ng == 0:
            raise ValueError("GaussianMixture: the training dataset is empty")
        target = min(ng, max(20 * k, 10000))
        frac = min(1.0, target / ng)
        u = K.uniform(n, seed, off, 21, device=X.device)
        samp = X[u < frac] if frac < 1 else X
        if comm.distributed:
            samp = torch.cat(comm.all_gather_varlen(samp.contiguous()))
        S = samp.double().cpu().numpy()
        if len(S) == 0:
            raise ValueError("GaussianMixture: the initialisation sample is empty")
        rng = np.random.default_rng(seed)
        rows = S[rng.integers(len(S), size=5 * k)].reshape(k, 5, -1)
        means = rows.mean(1)
        covs = np.stack([np.diag(((rows[j] - means[j]) ** 2).mean(0)) for j in range(k)])
        return np.full(k, 1.0 / k), means, covs

    def _fit(self, dataset):
        k = self.getK()
        if k <= 1:
            raise IllegalArgumentException(f"GaussianMixture parameter k given invalid value {k}: must be > 1")
        X, _, w = local_xyw(dataset, self.getFeaturesCol(), None, self.getWeightCol() or None, keep_f64=True)
        session = dataset._session
        comm = session.comm
        seed = self.getSeed() if self.getSeed() is not None else _default_seed(type(self))
        d = X.shape[1]
        D = d + 1
        # before the initial state is drawn: a non-finite row among its 5 k draws would turn the initial means and
        # variances into NaN and surface as a singular covariance
        bad = (~torch.isfinite(X).all(1)).sum().double().reshape(1)
        comm.all_reduce(bad)
        if float(bad) > 0:
            raise ValueError(f"GaussianMixture: {int(bad)} rows of column {self.getFeaturesCol()} have non-finite "
                             f"values")
        weights, means, covs = self._init_state(session, X, k, seed)

        def sums(mode):
            out = _gmm_call(X, w, weights, means, covs, mode)
            S, st = out if mode == K.GMM_STEP else (None, out)
            buf = st if S is None else torch.cat([S.reshape(-1), st])
            comm.all_reduce(buf)
            host = buf.cpu().numpy()
            if host[-1] > 0:
                raise ValueError(f"GaussianMixture: {int(host[-1])} rows of column {self.getFeaturesCol()} have a "
                                 f"non-finite Mahalanobis distance (overflow)")
            return (None if S is None else host[:-3].reshape(k, D, D)), host[-3:]

        tol, max_iter = self.getTol(), self.getMaxIter()
        ll, ll_prev, it = -np.finfo(np.float64).max, 0.0, 0
        while it < max_iter and not abs(ll - ll_prev) < tol:
            S, st = sums(K.GMM_STEP)
            # the op centres component j at c_j: the mean it was given, rounded to fp32 for fp32 rows
            c = means.astype(np.float32).astype(np.float64) if X.dtype == torch.float32 else means
            N = S[:, d, d]
            delta = S[:, :d, d] / N[:, None]
            means = c + delta
            covs = S[:, :d, :d] / N[:, None, None] - delta[:, :, None] * delta[:, None, :]
            weights = N / N.sum()
            ll_prev, ll = ll, float(st[0])
            it += 1
        if it == 0:
            ll = float(sums(K.GMM_EVAL)[1][0])
        model = GaussianMixtureModel(weights, means, covs)
        model._post_fit(self)
        if X.shape[0]:
            assign = _gmm_call(X, None, weights, means, covs, K.GMM_PREDICT)[1]
            sizes = torch.bincount(assign.long(), minlength=k).double()
        else:
            sizes = torch.zeros(k, dtype=torch.float64, device=X.device)
        comm.all_reduce(sizes)
        model.summary = GaussianMixtureSummary(model, dataset, ll, it, sizes.cpu().numpy().astype(np.int64).tolist())
        return model


class GaussianMixtureSummary:
    def __init__(self, model, dataset, log_likelihood, iters, sizes):
        self._model = model
        self._dataset = dataset
        self.logLikelihood = log_likelihood
        self.numIter = iters
        self.clusterSizes = sizes
        self.k = len(sizes)
        self.featuresCol = model.getFeaturesCol()
        self.predictionCol = model.getPredictionCol()
        self.probabilityCol = model.getProbabilityCol()

    @property
    def predictions(self):
        return self._model.transform(self._dataset)

    @property
    def cluster(self):
        return self.predictions.select(self.predictionCol)

    @property
    def probability(self):
        return self.predictions.select(self.probabilityCol)


class GaussianMixtureModel(Model):
    _params = _GMM_PARAMS

    def __init__(self, weights=None, means=None, covs=None):
        super().__init__()
        self._w = np.asarray(weights if weights is not None else np.zeros(0), dtype=np.float64)
        self._mu = np.asarray(means if means is not None else np.zeros((0, 0)), dtype=np.float64)
        self._cov = np.asarray(covs if covs is not None else np.zeros((0, 0, 0)), dtype=np.float64)
        self.summary = None

    @property
    def weights(self):
        return [float(v) for v in self._w]

    @property
    def gaussians(self):
        return [MultivariateGaussian(m, c) for m, c in zip(self._mu, self._cov)]

    @property
    def hasSummary(self):
        return self.summary is not None

    def _responsibilities(self, features):
        x = np.asarray(features.toArray() if hasattr(features, "toArray") else features, dtype=np.float64)
        return _gmm_call(torch.from_numpy(x.reshape(1, -1).copy()), None, self._w, self._mu, self._cov,
                         K.GMM_PREDICT)

    def predict(self, features):
        return int(self._responsibilities(features)[1][0])

    def predictProbability(self, features):
        return DenseVector(self._responsibilities(features)[0][0].numpy())

    def _transform(self, dataset):
        fc, pc, prc = self.getFeaturesCol(), self.getPredictionCol(), self.getProbabilityCol()
        require_vector(dataset, fc)
        A, logc = gmm_tables(self._w, self._mu, self._cov)
        mu, A, logc = torch.tensor(self._mu), torch.tensor(A), torch.tensor(logc)
        prep = K.GmmPrepared(mu, A, logc)   # the device tables are built once, not per batch

        def fn(b, ctx):
            X = b.columns[fc].values
            X = X if X.dtype == torch.float64 and X.numel() <= VECTOR_F64_MAX else X.float()
            R, a, _ = K.gmm_step(X, None, mu, A, logc, K.GMM_PREDICT, prepared=prep)
            if pc:
                b = b.with_column(pc, ColumnData(a.to(torch.int32), T.IntegerType()))
            if prc:
                b = b.with_column(prc, ColumnData(R, T.VectorUDT()))
            return b
        return dataset._new(MapPlan(dataset._plan, "GaussianMixtureModel", fn))

    def _save_state(self):
        return {}, {"weights": torch.tensor(self._w), "means": torch.tensor(self._mu), "covs": torch.tensor(self._cov)}

    def _load_state(self, extra, tensors, stages):
        self._w = tensors["weights"].numpy()
        self._mu = tensors["means"].numpy()
        self._cov = tensors["covs"].numpy()
        self.summary = None
