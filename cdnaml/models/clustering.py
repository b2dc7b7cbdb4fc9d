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

    def _init_centres(self, session, X, k, seed, normalise=False):
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
        if normalise:   # the cosine measure on rows that were not normalised beforehand (the K30 route)
            S = S / np.maximum(np.linalg.norm(S, axis=1, keepdims=True), 1e-30)
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
        X, _, w = local_xyw(dataset, fc, None, self.getWeightCol() or None, keep_f64=True)
        session = dataset._session
        comm = session.comm
        seed = self.getSeed() if self.getSeed() is not None else _default_seed(type(self))
        k = self.getK()
        d = X.shape[1]
        cosine = self.getDistanceMeasure() == "cosine"
        # K30 cluster_step: fp32 rows on a GPU inside its range, and (its host formulation) every weighted fit;
        # everything else keeps K10 kmeans_step on rows normalised beforehand for the cosine measure
        k30 = w is not None or _takes_k30(X, k, cosine)
        if cosine and not k30:
            X = X / torch.linalg.vector_norm(X, dim=1, keepdim=True).clamp_min(1e-30)
        C = self._init_centres(session, X, k, seed, normalise=cosine and k30)
        # the kernel works on x - shift: the fp32 mean of the initial centres, fixed for the fit
        shift = None if cosine else C.mean(0).astype(np.float32)

        def step(C, sums=True):
            """(assign, centre sums, weight sums, cost) of the local rows at the centres C"""
            if k30:
                out = K.cluster_step(X, C, K.CLUSTER_STEP if sums else K.CLUSTER_PREDICT, w, cosine, shift)
                return (out[0], out[1], out[2], out[3]) if sums else (out[0], None, None, out[1])
            a, S, N, c = K.kmeans_step(X, torch.tensor(C, dtype=X.dtype, device=X.device))
            return a, S, N, c * 0.5 if cosine else c    # |x^ - c^|^2 = 2 (1 - cos)

        it = 0
        for it in range(self.getMaxIter()):
            _, sums, counts, c = step(C)
            acc = torch.cat([sums.reshape(-1), counts, c.reshape(1)])
            comm.all_reduce(acc)
            a = acc.cpu().numpy()
            S = a[: k * d].reshape(k, -1)
            N = a[k * d: k * d + k]
            newC = np.where(N[:, None] > 0, S / np.where(N > 0, N, 1.0)[:, None], C)
            if cosine:
                newC = newC / np.maximum(np.linalg.norm(newC, axis=1, keepdims=True), 1e-30)
            moved = np.sqrt(((newC - C) ** 2).sum(1)).max()
            C = newC
            if moved <= self.getTol():
                it += 1
                break
        # final cost / sizes with the final centres: the sizes are row counts, whatever the weights
        assign, _, counts, c = step(C, sums=not k30)
        if k30:
            counts = torch.bincount(assign.long(), minlength=k).double()
        acc = torch.cat([counts, c.reshape(1)])
        comm.all_reduce(acc)
        a = acc.cpu().numpy()
        model = KMeansModel(C)
        model._post_fit(self)
        model.summary = KMeansSummary(model, dataset, a[:k].astype(np.int64).tolist(), float(a[k]),
                                      self.getMaxIter() if self.getMaxIter() == 0 else it)
        return model


def _takes_k30(X, k, cosine):
    """fp32 rows on a GPU inside K30's range.  That includes the unweighted Euclidean case K10 serves in HIP as well:
    at 1e7 x 100 K30's step takes 3.9 ms against K10's 108 ms (profiles/r22/cluster.md)."""
    return K.cluster_plan(X, k)["path"] == "native"


def _assign_cost(X, C, cosine):
    """(assign, cost) of the rows X at the centres C (numpy [k, d]), Spark's cost: sum of |x - c|^2 or 1 - cos."""
    if X.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int32, device=X.device), torch.zeros((), dtype=torch.float64,
                                                                               device=X.device)
    if _takes_k30(X, C.shape[0], cosine):
        shift = None if cosine else C.mean(0).astype(np.float32)
        a, c, _ = K.cluster_step(X, C, K.CLUSTER_PREDICT, None, cosine, shift)
        return a, c
    if cosine:
        X = X / torch.linalg.vector_norm(X, dim=1, keepdim=True).clamp_min(1e-30)
    a, _, _, c = K.kmeans_step(X, torch.tensor(C, dtype=X.dtype, device=X.device), with_sums=False)
    return a, c * 0.5 if cosine else c


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
        _, c = _assign_cost(X, self._C, self.getDistanceMeasure() == "cosine")
        t = torch.tensor([float(c)], dtype=torch.float64, device=dataset._session.comm.device)
        dataset._session.comm.all_reduce(t)
        return float(t)

    def _transform(self, dataset):
        fc, pc = self.getFeaturesCol(), self.getPredictionCol()
        require_vector(dataset, fc)
        cosine = self.getDistanceMeasure() == "cosine"

        def fn(b, ctx):
            X = b.columns[fc].values
            X = X if X.dtype == torch.float64 else X.float()   # Double vectors: fp64 distances (kernel <double>)
            a, _ = _assign_cost(X, self._C, cosine)
            return b.with_column(pc, ColumnData(a.to(torch.int32), T.IntegerType()))
        return dataset._new(MapPlan(dataset._plan, "KMeansModel", fn))

    def _save_state(self):
        return {}, {"centers": torch.tensor(self._C)}

    def _load_state(self, extra, tensors, stages):
        self._C = tensors["centers"].numpy()
        self.summary = None


class BisectingKMeans(KMeans):
    """Spark's bisecting k-means (mllib's level-wise algorithm): a binary tree of clusters, node i with the children
    2 i and 2 i + 1.  Every level bisects all divisible leaves together (the largest by weight when more are divisible
    than leaves are still needed, ties to the lower index) with ``maxIter`` passes of the K33 ``bisect_step`` op --
    every row takes one side of the bisector of its leaf's two children -- each followed by one all-reduce of the
    children's (W, cnt, S, Q) sums, from which centre and cost of a cluster both come.  No row leaves its rank and no
    copy of the rows is made: a row carries the split entry of its leaf in an int32."""
    _params = dict(KMeans._params, minDivisibleClusterSize=("min points in a divisible cluster", 1.0, TC.toFloat))

    def _fit(self, dataset):
        X, _, w = local_xyw(dataset, self.getFeaturesCol(), None, self.getWeightCol() or None, keep_f64=True)
        comm = dataset._session.comm
        seed = self.getSeed() if self.getSeed() is not None else _default_seed(type(self))
        cosine = self.getDistanceMeasure() == "cosine"
        d = X.shape[1]
        node = torch.zeros(X.shape[0], dtype=torch.int32, device=X.device)
        shift = np.zeros(d, dtype=np.float32)

        def step(h, t):
            """the children's [L, 2] W and Q and [L, 2, d] S over all ranks: one all-reduce of 2 L (d + 3) doubles"""
            L = len(t)
            W, cnt, S, Q, bad = K.bisect_step(X, h, t, [-1] * L, [-1] * L, K.BISECT_STEP, node, w, cosine, shift)
            acc = torch.cat([W.reshape(-1), cnt.reshape(-1), Q.reshape(-1), S.reshape(-1), bad.reshape(1)])
            comm.all_reduce(acc)
            a = acc.cpu().numpy()
            if a[-1] > 0:
                raise ValueError(f"BisectingKMeans: {int(a[-1])} rows of column {self.getFeaturesCol()} have "
                                 f"non-finite or overflowing values")
            return a[:2 * L].reshape(L, 2), a[6 * L:-1].reshape(L, 2, d), a[4 * L:6 * L].reshape(L, 2)

        # the root: one everything-left entry; the Euclidean fit works in the frame of the fp32 global mean
        root = (np.zeros((1, d)), [np.inf])
        W, S, Q = step(*root)
        if not W[0, 0] > 0:
            raise ValueError("BisectingKMeans: the training dataset has no weight")
        if not cosine:
            shift = (S[0, 0] / W[0, 0]).astype(np.float32)
            W, S, Q = step(*root)
        info = {1: _cluster_summary(W[0, 0], S[0, 0], Q[0, 0], cosine)}
        mds = self.getMinDivisibleClusterSize()
        min_size = mds if mds >= 1.0 else mds * W[0, 0]
        rng = np.random.default_rng(seed)
        max_iter, need = self.getMaxIter(), self.getK() - 1

        def divisible(active):
            div = [i for i in active if info[i][0] >= min_size and info[i][2] > _BISECT_EPS * info[i][0]]
            return sorted(sorted(div, key=lambda i: (-info[i][0], i))[:max(need, 0)])

        div = divisible([1]) if max_iter > 0 else []
        while div:
            cen = {}
            for i in div:            # Spark's splitCenter
                c = info[i][1]
                noise = rng.random(d)
                level = 1e-4 * np.linalg.norm(c + shift.astype(np.float64))
                for child, sign in ((2 * i, -1.0), (2 * i + 1, 1.0)):
                    v = c + sign * level * noise
                    cen[child] = v / max(np.linalg.norm(v), 1e-30) if cosine else v
            for _ in range(max_iter):
                W, S, Q = step(*_split_table(div, cen, d))
                new = {}
                for e, i in enumerate(div):
                    for s in (0, 1):
                        if 2 * i + s in cen:
                            if W[e, s] > 0:
                                new[2 * i + s] = _cluster_summary(W[e, s], S[e, s], Q[e, s], cosine)
                                cen[2 * i + s] = new[2 * i + s][1]
                            else:          # an empty child drops out for good: its sibling takes every row
                                del cen[2 * i + s]
            info.update(new)
            need -= len(div)
            nxt = divisible(sorted(new))
            if nxt:                  # commit the level: every row moves on to its child's entry of the next level
                h, t = _split_table(div, cen, d)
                tg = [[nxt.index(2 * i + s) if 2 * i + s in nxt else -1 for i in div] for s in (0, 1)]
                K.bisect_step(X, h, t, tg[0], tg[1], K.BISECT_ASSIGN, node, None, cosine, shift)
            div = nxt
        index = np.array(sorted(info), dtype=np.int64)
        model = BisectingKMeansModel(index, np.array([info[i][1] for i in index]) + shift.astype(np.float64),
                                     np.array([info[i][2] for i in index]), np.array([info[i][0] for i in index]),
                                     shift)
        model._post_fit(self)
        tab = model._tables()
        leaf = model._descend(X, tab)[0]
        sizes = torch.bincount(leaf.long(), minlength=len(tab["leaves"])).double()
        comm.all_reduce(sizes)
        model.summary = BisectingKMeansSummary(model, dataset, sizes.cpu().numpy().astype(np.int64).tolist(),
                                               float(model._cost[tab["leaves"]].sum()), max_iter)
        return model


_BISECT_EPS = 2.220446049250313e-16


def _cluster_summary(W, S, Q, cosine):
    """(W, centre, cost) of a cluster from its sums: the weight, the sum of w x~ and the sum of w |x~|^2 (Euclidean:
    in the shifted frame, which the cost does not depend on)."""
    if cosine:
        norm = float(np.linalg.norm(S))
        return float(W), S / max(norm, 1e-30), max(float(W) - norm, 0.0)
    return float(W), S / W, max(float(Q) - float(S @ S) / float(W), 0.0)


def _split_entry(cl, cr, d):
    """(h, t) of the bisector of two centres; a missing child (None) is h = 0 and t = +-inf."""
    if cl is None or cr is None:
        return np.zeros(d), (-np.inf if cl is None and cr is not None else np.inf)
    return cr - cl, (float(cr @ cr) - float(cl @ cl)) / 2.0


def _split_table(div, cen, d):
    rows = [_split_entry(cen.get(2 * i), cen.get(2 * i + 1), d) for i in div]
    return np.array([r[0] for r in rows]), [r[1] for r in rows]


class BisectingKMeansSummary(KMeansSummary):
    """clusterSizes (row counts per predicted leaf), trainingCost (the sum of the leaves' costs), numIter (maxIter),
    k, predictions and cluster."""


class BisectingKMeansModel(Model):
    """The tree of a bisecting k-means fit: ``index`` (tree indices, ascending: the children of node i are 2 i and
    2 i + 1), per node the centre, the cost and the weight, and the fit's shift.  The leaves, numbered depth-first and
    left first, are the clusters; prediction descends the tree (at every node to the closer child), which is not the
    nearest leaf."""
    _params = BisectingKMeans._params

    def __init__(self, index=None, centers=None, costs=None, weights=None, shift=None):
        super().__init__()
        self._index = np.asarray(index if index is not None else np.zeros(0), dtype=np.int64)
        self._C = np.asarray(centers if centers is not None else np.zeros((0, 0)), dtype=np.float64)
        self._cost = np.asarray(costs if costs is not None else np.zeros(0), dtype=np.float64)
        self._W = np.asarray(weights if weights is not None else np.zeros(0), dtype=np.float64)
        self._shift = np.asarray(shift if shift is not None else np.zeros(self._C.shape[1:]), dtype=np.float32)
        self.summary = None

    def _tables(self):
        """The PREDICT table of the tree, entries in depth-first order (targets point forward): h, t, left, right,
        and ``leaves``: the positions in ``index`` of the leaves in cluster order."""
        pos = {int(i): j for j, i in enumerate(self._index)}
        cosine = self.getDistanceMeasure() == "cosine"
        Ct = self._C if cosine else self._C - self._shift.astype(np.float64)
        d = self._C.shape[1]
        ent, leaves = [], []

        def visit(i):
            kids = [c if c in pos else None for c in (2 * i, 2 * i + 1)]
            if kids == [None, None]:
                leaves.append(pos[i])
                return -len(leaves)
            e = len(ent)
            ent.append(None)
            tg = [None if c is None else visit(c) for c in kids]
            h, t = _split_entry(*(None if c is None else Ct[pos[c]] for c in kids), d)
            ent[e] = (h, t, tg[0] if tg[0] is not None else tg[1], tg[1] if tg[1] is not None else tg[0])
            return e
        if visit(1) < 0:             # the root is the only cluster
            ent.append((np.zeros(d), np.inf, -1, -1))
        return dict(h=np.array([e[0] for e in ent]), t=[e[1] for e in ent], left=[e[2] for e in ent],
                    right=[e[3] for e in ent], leaves=np.array(leaves, dtype=np.int64))

    def _descend(self, X, tab, w=None):
        """(leaf, cost, bad) of the rows X by tree descent"""
        if X.shape[0] == 0:
            z = torch.zeros((), dtype=torch.float64, device=X.device)
            return torch.zeros(0, dtype=torch.int32, device=X.device), z, z
        return K.bisect_step(X, tab["h"], tab["t"], tab["left"], tab["right"], K.BISECT_PREDICT, None, w,
                             self.getDistanceMeasure() == "cosine", self._shift, self._C[tab["leaves"]])

    def clusterCenters(self):
        return [c.copy() for c in self._C[self._tables()["leaves"]]]

    @property
    def hasSummary(self):
        return self.summary is not None

    def predict(self, features):
        x = np.asarray(features.toArray() if hasattr(features, "toArray") else features, dtype=np.float64)
        return int(self._descend(torch.from_numpy(x.reshape(1, -1).copy()), self._tables())[0][0])

    def computeCost(self, dataset):
        X, _, _ = local_xyw(dataset, self.getFeaturesCol(), keep_f64=True)
        comm = dataset._session.comm
        t = self._descend(X, self._tables())[1].reshape(1).to(comm.device)
        comm.all_reduce(t)
        return float(t)

    def _transform(self, dataset):
        fc, pc = self.getFeaturesCol(), self.getPredictionCol()
        require_vector(dataset, fc)
        tab = self._tables()

        def fn(b, ctx):
            X = b.columns[fc].values
            X = X if X.dtype == torch.float64 else X.float()   # Double vectors: the fp64 host formulation
            return b.with_column(pc, ColumnData(self._descend(X, tab)[0], T.IntegerType()))
        return dataset._new(MapPlan(dataset._plan, "BisectingKMeansModel", fn))

    def _save_state(self):
        return {}, {"index": torch.tensor(self._index), "centers": torch.tensor(self._C),
                    "costs": torch.tensor(self._cost), "weights": torch.tensor(self._W),
                    "shift": torch.tensor(self._shift)}

    def _load_state(self, extra, tensors, stages):
        self._index = tensors["index"].numpy()
        self._C = tensors["centers"].numpy()
        self._cost = tensors["costs"].numpy()
        self._W = tensors["weights"].numpy()
        self._shift = tensors["shift"].numpy()
        self.summary = None


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
