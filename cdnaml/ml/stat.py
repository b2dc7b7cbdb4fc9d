"""``pyspark.ml.stat``: Correlation, Summarizer and the univariate hypothesis tests (ChiSquareTest, ANOVATest,
FValueTest) over device feature matrices."""
import numpy as np
import pandas as pd
import torch

from ..models.linalg import DenseMatrix, DenseVector
from ..ops import kernels as K


class Correlation:
    @staticmethod
    def corr(dataset, column, method="pearson"):
        from ..models.util import local_xyw
        X, _, _ = local_xyw(dataset, column, keep_f64=True)
        if method == "spearman":
            X = torch.argsort(torch.argsort(X, 0), 0).float()
        from ..models.util import centered_gram
        _, _, C = centered_gram(X, dataset._session.comm)
        sd = torch.sqrt(torch.diagonal(C).clamp_min(1e-300))
        R = (C / torch.outer(sd, sd)).cpu().numpy()
        return _MatrixFrame(R, method, column)


class _MatrixFrame:
    """Tiny stand-in for the 1x1 DataFrame of a Matrix (head()[0] is the matrix)."""

    def __init__(self, R, method, column):
        self._m = DenseMatrix(R.shape[0], R.shape[1], R.T.reshape(-1))
        self.columns = [f"{method}({column})"]

    def head(self):
        return [self._m]

    def collect(self):
        return [[self._m]]


_METRICS = ("mean", "sum", "variance", "std", "count", "numNonZeros", "max", "min", "normL2", "normL1", "weightSum")


def _col_expr(col):
    from ..sql.column import ColRef, Column
    if isinstance(col, Column):
        return col._expr
    return ColRef(col)


class SummaryBuilder:
    """``Summarizer.metrics(...)``: ``summary(featuresCol, weightCol=None)`` is an aggregate Column whose value
    is a struct (Row) with one field per requested metric, in the requested order."""

    def __init__(self, names):
        bad = [m for m in names if m not in _METRICS]
        if bad or not names:
            raise ValueError(f"Summarizer metrics must be among {list(_METRICS)}, got {list(names)}")
        self.names = list(names)

    def summary(self, featuresCol, weightCol=None):
        from ..sql.column import Column
        from ..sql.functions import AggExpr
        x = _col_expr(featuresCol)
        w = None if weightCol is None else _col_expr(weightCol)
        disp = f"aggregate_metrics({x.name()}, {'1.0' if w is None else w.name()})"
        return Column(AggExpr("summarizer", x, param={"metrics": self.names, "weight": w, "single": False},
                              display=disp))


class Summarizer:
    """``pyspark.ml.stat.Summarizer``: vector-column statistics as aggregate expressions (usable in ``select``
    and ``groupBy().agg``).  Weighted semantics follow Spark's SummarizerBuffer: rows of weight 0 are skipped;
    ``count`` / ``numNonZeros`` count rows / non-zero entries, ``sum`` / ``mean`` / ``normL1`` / ``normL2`` are
    weighted, ``variance`` is the unbiased weighted variance (denominator W - sum(w^2) / W).  On the GPU the
    unweighted per-column moments come from K20 (``col_moments``: count, mean, M2, min, max in fp64)."""

    @staticmethod
    def metrics(*names):
        return SummaryBuilder(names)

    @staticmethod
    def _single(metric, col, weightCol=None):
        from ..sql.column import Column
        from ..sql.functions import AggExpr
        x = _col_expr(col)
        w = None if weightCol is None else _col_expr(weightCol)
        return Column(AggExpr("summarizer", x, param={"metrics": [metric], "weight": w, "single": True},
                              display=f"{metric}({x.name()})"))


for _m in _METRICS:
    setattr(Summarizer, _m, staticmethod(lambda col, weightCol=None, _m=_m: Summarizer._single(_m, col, weightCol)))


def _metric_values(X: torch.Tensor, w, metrics):
    """{metric: value} for one group's rows X [n, d] (fp64) and weights w [n] or None."""
    n, d = X.shape
    if w is not None:
        keep = w != 0
        X, w = X[keep], w[keep]
        n = X.shape[0]
    out = {}
    need_mom = any(m in metrics for m in ("mean", "variance", "std", "max", "min")) and w is None
    mom = K.col_moments(X) if need_mom else None  # K20 (count, mean, M2, min, max)
    W = float(n) if w is None else float(w.sum())
    for m in metrics:
        if m == "count":
            out[m] = int(n)
        elif m == "weightSum":
            out[m] = W
        elif m == "numNonZeros":
            out[m] = DenseVector((X != 0).sum(0).double().cpu().numpy())
        elif m in ("max", "min"):
            if n == 0:
                v = np.full(d, -np.inf if m == "max" else np.inf)
            elif mom is not None:
                v = mom[:, 4 if m == "max" else 3].cpu().numpy()
            else:
                v = (X.amax(0) if m == "max" else X.amin(0)).cpu().numpy()
            out[m] = DenseVector(v)
        elif m in ("sum", "mean", "normL1", "normL2"):
            ww = torch.ones(n, dtype=torch.float64, device=X.device) if w is None else w
            if m == "sum":
                v = (ww[:, None] * X).sum(0)
            elif m == "mean":
                v = mom[:, 1] if mom is not None else (ww[:, None] * X).sum(0) / (W if W > 0 else float("nan"))
            elif m == "normL1":
                v = (ww[:, None] * X.abs()).sum(0)
            else:
                v = torch.sqrt((ww[:, None] * X * X).sum(0))
            out[m] = DenseVector(v.cpu().numpy() if n else np.zeros(d))
        else:  # variance / std
            if w is None:
                v = (mom[:, 2] / (n - 1)) if n > 1 else torch.zeros(d, dtype=torch.float64)
            else:
                den = W - float((w * w).sum()) / W if W > 0 else 0.0
                mu = (w[:, None] * X).sum(0) / W if W > 0 else torch.zeros(d, dtype=torch.float64, device=X.device)
                v = (w[:, None] * (X - mu) ** 2).sum(0) / den if den > 0 else torch.zeros(d, dtype=torch.float64)
            v = v.clamp_min(0.0)
            out[m] = DenseVector((torch.sqrt(v) if m == "std" else v).cpu().numpy())
    return out


def summarize_groups(c, wcol, gid: torch.Tensor, G: int, param):
    """Group engine hook (relational._agg_one, kind "summarizer"): one struct Row (or, for a single metric, a
    vector / count column) per group."""
    from ..sql import types as T
    from ..sql.batch import ColumnData
    from ..sql.types import Row
    X = c.values
    if X.dim() == 1:
        X = X[:, None]
    X = X.to(torch.float64)
    if c.valid is not None:
        gid = gid[c.valid]
        X = X[c.valid]
    w = None if wcol is None else wcol.values.to(torch.float64)
    if w is not None and c.valid is not None:
        w = w[c.valid]
    metrics = param["metrics"]
    order = torch.argsort(gid, stable=True)
    counts = torch.bincount(gid, minlength=G).cpu().tolist() if gid.numel() else [0] * G
    Xs, ws = X[order], None if w is None else w[order]
    rows, r0 = [], 0
    for g in range(G):
        r1 = r0 + counts[g]
        rows.append(_metric_values(Xs[r0:r1], None if ws is None else ws[r0:r1], metrics))
        r0 = r1
    dev = c.values.device
    if param.get("single"):
        m = metrics[0]
        if m == "count":
            return ColumnData(torch.tensor([r[m] for r in rows], dtype=torch.int64, device=dev), T.LongType())
        if m == "weightSum":
            return ColumnData(torch.tensor([r[m] for r in rows], dtype=torch.float64, device=dev), T.DoubleType())
        d = X.shape[1]
        V = np.stack([r[m].toArray() for r in rows]) if rows else np.zeros((0, d))
        return ColumnData(torch.from_numpy(V).to(dev), T.VectorUDT())
    fields = [T.StructField(m, T.LongType() if m == "count" else T.DoubleType() if m == "weightSum"
                            else T.VectorUDT(), True) for m in metrics]
    structs = [Row(**{m: r[m] for m in metrics}) for r in rows]
    return ColumnData(torch.zeros(G, device=dev), T.StructType(fields), meta={"_py": structs})


# ============================================================ univariate tests (K27 label_stats)
MAX_CATEGORIES = 10000         # Spark's limit on the distinct values of a chi-square feature or label
COUNT_MAX_CELLS = 1 << 24      # a wider contingency table [d][K][C] is formed per feature from the distinct values


def _label_codes(y: torch.Tensor, comm):
    """(distinct label values over all ranks, ascending; this rank's rows as int32 ranks among them)."""
    from ..models.feature import SparkException
    loc = torch.unique(y).cpu().numpy() if y.numel() else np.zeros(0)
    vals = np.unique(np.concatenate([np.asarray(v, dtype=np.float64) for v in comm.all_gather_object(loc)]))
    if len(vals) > MAX_CATEGORIES:
        raise SparkException(f"Chi-square test expect factors (categorical values) but found more than "
                             f"{MAX_CATEGORIES} distinct label values.")
    codes = torch.searchsorted(torch.from_numpy(vals).to(y.device), y).to(torch.int32) if y.numel() else \
        torch.zeros(0, dtype=torch.int32, device=y.device)
    return vals, codes


def _shift(V: torch.Tensor, comm) -> torch.Tensor:
    """The shift of ``util.centered_gram`` for the columns of V (a vector of labels: one column), fp64; every rank
    gets the same one.  A mean that is not finite (the F tests report such values afterwards) becomes 0."""
    from ..models.util import lead_mean
    sh = lead_mean(V[:, None] if V.dim() == 1 else V, comm)
    return torch.where(torch.isfinite(sh), sh, torch.zeros_like(sh))


def _reduced(parts, comm) -> np.ndarray:
    """One all-reduce of the statistics' parts as fp64 (counts are exact below 2^53); the host copy, flat."""
    flat = torch.cat([p.reshape(-1).double() for p in parts])
    comm.all_reduce(flat)
    return flat.cpu().numpy()


def _chi2_of_table(O: np.ndarray):
    """(statistic, p-value, degrees of freedom) of a contingency table; categories and labels that do not occur
    are dropped (Spark's factors are the distinct values that occur)."""
    from scipy.stats import chi2
    O = np.asarray(O, dtype=np.float64)
    O = O[O.sum(1) > 0][:, O.sum(0) > 0]
    if O.shape[0] > MAX_CATEGORIES:
        from ..models.feature import SparkException
        raise SparkException(f"Chi-square test expect factors (categorical values) but found more than "
                             f"{MAX_CATEGORIES} distinct values.")
    df = (O.shape[0] - 1) * (O.shape[1] - 1) if O.size else 0
    if df <= 0:
        return 0.0, 1.0, 0
    E = np.outer(O.sum(1), O.sum(0)) / O.sum()
    stat = float(((O - E) ** 2 / E).sum())
    return stat, float(chi2.sf(stat, df)), int(df)


def _distinct_table(x: torch.Tensor, codes: torch.Tensor, C: int, comm) -> np.ndarray:
    """The contingency table of one feature from its distinct values (any doubles: the categories are their
    ranks), over all ranks."""
    from ..models.feature import SparkException
    xv = x.double().cpu().numpy()
    uv, inv = np.unique(xv, return_inverse=True)
    tab = np.zeros((len(uv), C), dtype=np.int64)
    np.add.at(tab, (inv.reshape(-1), codes.cpu().numpy().astype(np.int64)), 1)
    got = comm.all_gather_object((uv, tab))
    vals = np.unique(np.concatenate([g[0] for g in got]))
    if len(vals) > MAX_CATEGORIES:
        raise SparkException(f"Chi-square test expect factors (categorical values) but found more than "
                             f"{MAX_CATEGORIES} distinct values.")
    out = np.zeros((len(vals), C), dtype=np.int64)
    for u, t in got:
        if len(u):
            np.add.at(out, np.searchsorted(vals, u), t)
    return out


def chi_square_scores(dataset, featuresCol, labelCol):
    """(pValues, degreesOfFreedom, statistics) per feature, numpy: Pearson's chi-square test of independence of
    every feature against the label, both taken as categorical."""
    from ..models.util import categorical_info, local_xyw
    comm = dataset._session.comm
    X, y, _ = local_xyw(dataset, featuresCol, labelCol, keep_f64=True)
    n, d = X.shape
    vals, codes = _label_codes(y, comm)
    C = len(vals)
    if C == 0 or d == 0:
        return np.ones(d), np.zeros(d, dtype=np.int64), np.zeros(d)
    arity = categorical_info(dataset.schema[featuresCol].metadata, d, featuresCol)
    if len(arity) == d:
        Kc = max(arity.values())
    else:
        mx = float(torch.where(torch.isfinite(X), X, torch.zeros_like(X)).amax()) if n else 0.0
        Kc = int(min(max(comm.all_reduce_scalar(mx, "max"), 0.0), 2.0 ** 40)) + 1
    if d * Kc * C <= COUNT_MAX_CELLS:
        st = K.label_stats(X, codes, K.LABEL_COUNT, C=C, K=Kc)
        flat = _reduced([st["table"], st["bad"]], comm)
        table = np.rint(flat[:d * Kc * C]).astype(np.int64).reshape(d, Kc, C)
        bad = flat[d * Kc * C:] > 0
    else:
        table, bad = None, np.ones(d, dtype=bool)
    p, dof, stat = np.ones(d), np.zeros(d, dtype=np.int64), np.zeros(d)
    for j in range(d):
        # a feature with values that are not category indices below K: from its distinct values, as Spark does
        O = _distinct_table(X[:, j], codes, C, comm) if bad[j] else table[j]
        stat[j], p[j], dof[j] = _chi2_of_table(O)
    return p, dof, stat


def _require_clean(bad: np.ndarray, bad_label: float, what: str):
    from ..models.util import IllegalArgumentException
    if bad_label > 0:
        raise IllegalArgumentException(f"{what}: the label has {int(bad_label)} values that are not finite")
    if (bad > 0).any():
        j = int(np.argmax(bad > 0))
        raise IllegalArgumentException(f"{what}: feature {j} has {int(bad[j])} values that are not finite")


def anova_scores(dataset, featuresCol, labelCol):
    """(pValues, degreesOfFreedom, fValues) per feature, numpy: the one-way ANOVA F-test of every continuous
    feature against a categorical label (Spark's computeANOVA; sklearn's f_classif)."""
    from scipy.stats import f as f_dist
    from ..models.util import local_xyw
    comm = dataset._session.comm
    X, y, _ = local_xyw(dataset, featuresCol, labelCol, keep_f64=True)
    d = X.shape[1]
    vals, codes = _label_codes(y, comm)
    C = max(len(vals), 1)
    st = K.label_stats(X, codes, K.LABEL_CLASS, C=C, shift=_shift(X, comm))
    flat = _reduced([st["sums"], st["sq"], st["n"], st["bad"], st["bad_label"]], comm)
    sums, sq = flat[:C * d].reshape(C, d), flat[C * d:C * d + d]
    nc, bad, bad_label = flat[C * d + d:C * d + d + C], flat[C * d + d + C:C * d + 2 * d + C], flat[-1]
    _require_clean(bad, bad_label, "ANOVATest")
    keep = nc > 0
    sums, nc = sums[keep], nc[keep]
    n, Cn = nc.sum(), int(keep.sum())
    S = sums.sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        between = (sums ** 2 / nc[:, None]).sum(0) - S ** 2 / n
        within = (sq - S ** 2 / n) - between
        dfb, dfw = Cn - 1, n - Cn
        F = (between / dfb) / (within / dfw)
        p = f_dist.sf(F, dfb, dfw)
    return p, np.full(d, int(n) - 1, dtype=np.int64), F


def fvalue_scores(dataset, featuresCol, labelCol):
    """(pValues, degreesOfFreedom, fValues) per feature, numpy: the F-test of the Pearson correlation of every
    continuous feature with a continuous label (sklearn's f_regression)."""
    from scipy.stats import f as f_dist
    from ..models.util import local_xyw
    comm = dataset._session.comm
    X, y, _ = local_xyw(dataset, featuresCol, labelCol, keep_f64=True)
    d = X.shape[1]
    st = K.label_stats(X, y, K.LABEL_REGRESS, shift=_shift(X, comm), yshift=float(_shift(y, comm)[0]))
    flat = _reduced([st["sx"], st["sxx"], st["sxy"], st["bad"], st["sy"], st["syy"], st["n"], st["bad_label"]], comm)
    sx, sxx, sxy, bad = flat[:d], flat[d:2 * d], flat[2 * d:3 * d], flat[3 * d:4 * d]
    sy, syy, n, bad_label = flat[4 * d:]
    _require_clean(bad, bad_label, "FValueTest")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (sxy - sx * sy / n) / np.sqrt((sxx - sx ** 2 / n) * (syy - sy ** 2 / n))
        F = r ** 2 / (1.0 - r ** 2) * (n - 2)
        p = f_dist.sf(F, 1, n - 2)
    return p, np.full(d, int(n) - 2, dtype=np.int64), F


def _test_frame(dataset, p, dof, stat, stat_name, flatten, long_dof):
    """The tests' result as a DataFrame of the dataset's session: one row of vectors, or one row per feature."""
    from ..sql import types as T
    from ..sql.batch import Batch, ColumnData
    sess = dataset._session
    dev = sess.device
    it = T.LongType() if long_dof else T.IntegerType()
    tdt = torch.int64 if long_dof else torch.int32
    d = len(p)
    a, b = sess._rank_slice(d if flatten else 1)      # the rows are spread over the ranks like any local table
    if flatten:
        cols = {"featureIndex": ColumnData(torch.arange(a, b, dtype=torch.int32, device=dev), T.IntegerType()),
                "pValue": ColumnData(torch.from_numpy(p[a:b].astype(np.float64)).to(dev), T.DoubleType()),
                "degreesOfFreedom": ColumnData(torch.from_numpy(dof[a:b].astype(np.int64)).to(dev, tdt), it),
                stat_name: ColumnData(torch.from_numpy(stat[a:b].astype(np.float64)).to(dev), T.DoubleType())}
    else:
        k = b - a

        def vec(v):
            return ColumnData(torch.from_numpy(np.asarray(v, np.float64))[None, :].to(dev)[:k], T.VectorUDT())
        # the array of integers rides as host objects, like the group engine's struct rows
        cols = {"pValues": vec(p),
                "degreesOfFreedom": ColumnData(torch.zeros(k, device=dev), T.ArrayType(it),
                                               meta={"_py": [[int(v) for v in dof]] * k}),
                stat_name + "s": vec(stat)}                # statistics / fValues
    batch = Batch(cols, b - a, dev)
    return sess._from_local_batches("LocalTableScan", lambda: [batch], batch.schema())


class ChiSquareTest:
    """``pyspark.ml.stat.ChiSquareTest``: Pearson's independence test of every feature against the label.  The
    label's categories are its distinct values; a feature's are its values as category indices (the contingency
    tables of all features come from one pass of K27 ``label_stats``), and a feature with other values (not
    integers, negative) is recounted from its distinct values, as Spark does.  More than 10000 distinct values
    raise."""

    @staticmethod
    def test(dataset, featuresCol, labelCol, flatten=False):
        p, dof, stat = chi_square_scores(dataset, featuresCol, labelCol)
        return _test_frame(dataset, p, dof, stat, "statistic", flatten, long_dof=False)


class ANOVATest:
    """``pyspark.ml.stat.ANOVATest``: the one-way ANOVA F-test of every continuous feature against a categorical
    label.  A feature value that is not finite raises IllegalArgumentException naming the first such feature
    (Spark returns NaN there); AFTSurvivalRegression validates its rows the same way."""

    @staticmethod
    def test(dataset, featuresCol, labelCol, flatten=False):
        p, dof, stat = anova_scores(dataset, featuresCol, labelCol)
        return _test_frame(dataset, p, dof, stat, "fValue", flatten, long_dof=True)


class FValueTest:
    """``pyspark.ml.stat.FValueTest``: the F-test of every continuous feature's correlation with a continuous
    label.  A feature value or label that is not finite raises IllegalArgumentException naming the first such
    feature (Spark returns NaN there); AFTSurvivalRegression validates its rows the same way."""

    @staticmethod
    def test(dataset, featuresCol, labelCol, flatten=False):
        p, dof, stat = fvalue_scores(dataset, featuresCol, labelCol)
        return _test_frame(dataset, p, dof, stat, "fValue", flatten, long_dof=True)
