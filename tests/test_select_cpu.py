"""``K.label_stats``' host formulation, the univariate tests of ``pyspark.ml.stat`` and the feature selectors.

* the host formulation against ``tests/_select_refs.py`` at the shapes of the device tests: COUNT tables exactly, the
  CLASS and REGRESS sums under the criterion (at most M = 8 times the error of the plain numpy fp64 yardstick, floor
  4 fp64 ulps of the largest entry);
* ChiSquareTest, ANOVATest and FValueTest against the longdouble statistics, with scipy's and scikit-learn's results
  as the yardstick of the same criterion (p-values: on log p where p is tiny), and chi-square's semantics;
* the selection modes, the selectors end to end, transform, persistence, Pipeline and the pyspark aliases.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _select_refs as R
from tests.test_select_gpu import BAD_CELLS, CC, KC, SHAPES


def host(X, label, mode, **kw):
    st = K.label_stats(torch.tensor(X), torch.tensor(label), mode, native=False, **kw)
    return {k: v.numpy() for k, v in st.items()}


# ------------------------------------------------------------------------------------------------ host formulation
@pytest.mark.parametrize("d,n,vw", SHAPES)
def test_host_formulation_matches_the_references(d, n, vw):
    k, c = R.count_case(d, n, KC, CC), R.cont_case(d, n, CC)
    st = host(k["X"], k["codes"], K.LABEL_COUNT, C=CC, K=KC)
    assert st["table"].dtype == np.int64 and np.array_equal(st["table"], k["table"])
    assert not st["bad"].any() and st["bad_label"] == 0
    R.check_class(f"host class d={d} n={n}", host(c["X"], c["codes"], K.LABEL_CLASS, C=CC, shift=c["shift"]),
                  c["cls"], c["y_cls"])
    R.check_regress(f"host regress d={d} n={n}",
                    host(c["X"], c["y"], K.LABEL_REGRESS, shift=c["shift"], yshift=c["yshift"]), c["reg"], c["y_reg"])


def test_host_formulation_in_chunks(monkeypatch):
    d, n = 5, 130
    k, c = R.count_case(d, n, KC, CC), R.cont_case(d, n, CC)
    monkeypatch.setattr(K, "LABEL_HOST_CHUNK", 64)
    assert np.array_equal(host(k["X"], k["codes"], K.LABEL_COUNT, C=CC, K=KC)["table"], k["table"])
    R.check_class("host class, chunks", host(c["X"], c["codes"], K.LABEL_CLASS, C=CC, shift=c["shift"]),
                  c["cls"], c["y_cls"])
    R.check_regress("host regress, chunks",
                    host(c["X"], c["y"], K.LABEL_REGRESS, shift=c["shift"], yshift=c["yshift"]), c["reg"], c["y_reg"])


@pytest.mark.parametrize("C", [2, 33, 70])
def test_host_formulation_class_counts(C):
    """Both forms of the class sums: a one-hot product for few classes, an index add for many."""
    c = R.cont_case(9, 600, C)
    R.check_class(f"host class C={C}", host(c["X"], c["codes"], K.LABEL_CLASS, C=C, shift=c["shift"]),
                  c["cls"], c["y_cls"])


def test_host_formulation_bad_cells_and_labels():
    d, n = 5, 130
    k, c = R.count_case(d, n, KC, CC), R.cont_case(d, n, CC)
    X, codes = k["X"].copy(), k["codes"].copy()
    X[[0, 17, 63, 64, n - 1], 1] = BAD_CELLS
    codes[[5, 100]] = [-1, CC]
    table, bad, bad_label = R.count_table(X, codes, KC, CC)
    st = host(X, codes, K.LABEL_COUNT, C=CC, K=KC)
    assert np.array_equal(st["table"], table) and np.array_equal(st["bad"], bad) and st["bad_label"] == bad_label == 2
    assert bad.tolist() == [0, 5, 0, 0, 0]
    X, codes, y = c["X"].copy(), c["codes"].copy(), c["y"].copy()
    X[[0, 63, n - 1], 3] = [float("nan"), float("inf"), float("-inf")]
    codes[[5, 100]] = [-1, CC]
    y[[5, 100]] = [float("nan"), float("inf")]
    a = host(X, codes, K.LABEL_CLASS, C=CC, shift=c["shift"])
    r = host(X, y, K.LABEL_REGRESS, shift=c["shift"], yshift=c["yshift"])
    for st in (a, r):
        assert st["bad"].tolist() == [0, 0, 0, 3, 0] and st["bad_label"] == 2
    R.check_class("host class, bad cells", a, R.class_reference(X, codes, CC, c["shift"]),
                  R.class_yardstick(X, codes, CC, c["shift"]))
    R.check_regress("host regress, bad cells", r, R.regress_reference(X, y, c["shift"], c["yshift"]),
                    R.regress_yardstick(X, y, c["shift"], c["yshift"]))


def test_plan_on_the_cpu_is_the_host_formulation():
    assert K.label_stats_plan(torch.zeros((10, 4)), K.LABEL_COUNT, C=2, K=3) == {"path": "host"}
    with pytest.raises(ValueError):
        K.label_stats(torch.zeros((10, 4)), torch.zeros(9), K.LABEL_REGRESS)
    with pytest.raises(ValueError):
        K.label_stats(torch.zeros((10, 4)), torch.zeros(10), 3)


# ------------------------------------------------------------------------------------------------ frames
def frame(spark, X, label):
    """features (a Double vector of X's columns) and label."""
    from cdnaml.ml.feature import VectorAssembler
    names = [f"x{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(np.asarray(X, dtype=np.float64), columns=names)
    pdf["label"] = np.asarray(label, dtype=np.float64)
    return VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))


def one_row(df):
    r = df.head()
    return np.asarray(r[0].toArray()), list(r[1]), np.asarray(r[2].toArray())


def p_scale(p, ref):
    """p-values as the criterion takes them: log p where the reference's p is tiny."""
    p, ref = np.asarray(p, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(ref < 1e-8, np.log(p), p)


# ------------------------------------------------------------------------------------------------ third parties
def test_chi_square_against_scipy(spark):
    from scipy.stats import chi2, chi2_contingency
    from cdnaml.ml.stat import ChiSquareTest
    d, n = 6, 700
    X, codes = R.make_counts(d, n, KC, CC)
    df = frame(spark, X, codes)
    p, dof, stat = one_row(ChiSquareTest.test(df, "features", "label"))
    table = R.count_table(X, codes, KC, CC)[0]
    ref = [R.chi2_reference(table[j]) for j in range(d)]
    sc = [chi2_contingency(table[j][table[j].sum(1) > 0], correction=False) for j in range(d)]
    assert dof == [r[1] for r in ref] == [int(s[2]) for s in sc] and all(isinstance(v, int) for v in dof)
    ref_stat = np.array([r[0] for r in ref])
    ref_p = chi2.sf(ref_stat, dof)
    R.check("chi-square statistic", stat, ref_stat, [s[0] for s in sc])
    R.check("chi-square p", p_scale(p, ref_p), p_scale(ref_p, ref_p), p_scale([s[1] for s in sc], ref_p))
    flat = ChiSquareTest.test(df, "features", "label", flatten=True)
    assert flat.columns == ["featureIndex", "pValue", "degreesOfFreedom", "statistic"]
    pdf = flat.toPandas()
    assert pdf.featureIndex.tolist() == list(range(d)) and pdf.degreesOfFreedom.tolist() == dof
    assert np.array_equal(pdf.pValue.to_numpy(), p) and np.array_equal(pdf.statistic.to_numpy(), stat)
    assert ChiSquareTest.test(df, "features", "label").columns == ["pValues", "degreesOfFreedom", "statistics"]


def _narrow(n, rng):
    """A far-from-zero narrow column (the latitude of util.centered_gram): mean 37.8, sd 0.02."""
    return 37.8 + 0.02 * rng.normal(size=n)


def test_anova_against_sklearn_and_scipy(spark):
    from scipy.stats import f as f_dist, f_oneway
    from sklearn.feature_selection import f_classif
    from cdnaml.ml.stat import ANOVATest
    d, n = 6, 700
    X, codes, _ = R.make_continuous(d, n, CC, dtype=np.float64)
    X[:, 5] = _narrow(n, np.random.default_rng(5)) + 0.004 * codes
    df = frame(spark, X, codes)
    p, dof, F = one_row(ANOVATest.test(df, "features", "label"))
    assert dof == [n - 1] * d
    ref = R.anova_f_reference(X, codes)
    ref_p = f_dist.sf(ref, CC - 1, n - CC)
    sk_F, sk_p = f_classif(X, codes)
    one = f_oneway(*[X[codes == c] for c in range(CC)])
    R.check("anova F against f_classif", F, ref, sk_F)
    R.check("anova p against f_classif", p_scale(p, ref_p), p_scale(ref_p, ref_p), p_scale(sk_p, ref_p))
    R.check("anova F against f_oneway", F, ref, one.statistic)
    R.check("anova p against f_oneway", p_scale(p, ref_p), p_scale(ref_p, ref_p), p_scale(one.pvalue, ref_p))
    # the narrow column alone: the shift at work
    R.check("anova F, narrow column", F[5:], ref[5:], sk_F[5:])
    flat = ANOVATest.test(df, "features", "label", flatten=True)
    assert flat.columns == ["featureIndex", "pValue", "degreesOfFreedom", "fValue"]
    assert np.array_equal(flat.toPandas().fValue.to_numpy(), F)
    assert ANOVATest.test(df, "features", "label").columns == ["pValues", "degreesOfFreedom", "fValues"]


def test_fvalue_against_sklearn(spark):
    from scipy.stats import f as f_dist
    from sklearn.feature_selection import f_regression
    from cdnaml.ml.stat import FValueTest
    d, n = 6, 700
    X, _, y = R.make_continuous(d, n, CC, dtype=np.float64)
    X[:, 5] = _narrow(n, np.random.default_rng(6)) + 0.002 * (y - 5.0)
    df = frame(spark, X, y)
    p, dof, F = one_row(FValueTest.test(df, "features", "label"))
    assert dof == [n - 2] * d
    ref = R.fvalue_f_reference(X, y)
    ref_p = f_dist.sf(ref, 1, n - 2)
    sk_F, sk_p = f_regression(X, y)
    R.check("F-value against f_regression", F, ref, sk_F)
    R.check("F-value p against f_regression", p_scale(p, ref_p), p_scale(ref_p, ref_p), p_scale(sk_p, ref_p))
    R.check("F-value, narrow column", F[5:], ref[5:], sk_F[5:])
    flat = FValueTest.test(df, "features", "label", flatten=True).toPandas()
    assert np.array_equal(flat.fValue.to_numpy(), F) and flat.degreesOfFreedom.tolist() == dof


# ------------------------------------------------------------------------------------------------ chi-square semantics
def test_chi_square_semantics(spark):
    from cdnaml.ml.stat import ChiSquareTest
    n = 400
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 3, size=n)
    label = np.array([-1.0, 2.5, 7.0])[codes]             # labels that are not 0 .. C-1
    cat = (codes + (rng.random(n) < 0.4) * rng.integers(0, 3, size=n)) % 3
    X = np.stack([np.full(n, 4.0),                          # constant
                  np.array([0.0, 3.0, 5.0])[cat],           # categories 1, 2 and 4 do not occur
                  np.array([0.5, -3.0, 2.0])[cat],          # not category indices: the ranks of the values
                  np.array([1.0, 0.0, 2.0])[cat]], axis=1)  # -3.0 < 0.5 < 2.0: the rank codes of column 2
    p, dof, stat = one_row(ChiSquareTest.test(frame(spark, X, label), "features", "label"))
    assert (dof[0], stat[0], p[0]) == (0, 0.0, 1.0)
    assert dof[1:] == [4, 4, 4]
    want, _ = R.chi2_reference(R.count_table(X[:, 3:], codes, 3, 3)[0][0])
    assert stat[2] == stat[3] and p[2] == p[3]
    np.testing.assert_allclose(stat[1:], want, rtol=1e-13)
    # the same table whatever the label's values are
    p2, dof2, stat2 = one_row(ChiSquareTest.test(frame(spark, X, codes), "features", "label"))
    assert dof2 == dof and np.array_equal(stat2, stat) and np.array_equal(p2, p)


def test_chi_square_distinct_value_limit(spark):
    from cdnaml.ml.feature import SparkException
    from cdnaml.ml.stat import ChiSquareTest
    n = 10001
    X = np.stack([np.arange(n) + 0.5, np.arange(n) % 3], axis=1)
    with pytest.raises(SparkException):
        ChiSquareTest.test(frame(spark, X, np.arange(n) % 2), "features", "label").head()
    with pytest.raises(SparkException):
        ChiSquareTest.test(frame(spark, X[:, 1:], np.arange(n)), "features", "label").head()
    ok = one_row(ChiSquareTest.test(frame(spark, X[:10000], np.arange(10000) % 2), "features", "label"))
    assert ok[1] == [9999, 2]


def test_f_tests_raise_on_values_that_are_not_finite(spark):
    from cdnaml.ml.stat import ANOVATest, FValueTest
    from cdnaml.models.util import IllegalArgumentException
    X, codes, y = R.make_continuous(4, 100, CC, dtype=np.float64)
    X[7, 2] = float("inf")
    with pytest.raises(IllegalArgumentException, match="feature 2"):
        ANOVATest.test(frame(spark, X, codes), "features", "label")
    with pytest.raises(IllegalArgumentException, match="feature 2"):
        FValueTest.test(frame(spark, X, y), "features", "label")
    X[7, 2] = 0.0
    y[3] = float("inf")
    with pytest.raises(IllegalArgumentException, match="label"):
        FValueTest.test(frame(spark, X, y), "features", "label")


# ------------------------------------------------------------------------------------------------ selection modes
def test_selection_modes_on_hand_written_p_values():
    from cdnaml.models.feature import select_by_pvalues as sel
    p = [0.20, 0.01, 0.03, 0.01, 0.50, 0.03, 0.001, 0.04]
    assert sel(p, "numTopFeatures", 3) == [1, 3, 6]                 # the tie at 0.01 both fit
    assert sel(p, "numTopFeatures", 2) == [1, 6]                    # the tie goes to the lower index
    assert sel(p, "numTopFeatures", 4) == [1, 2, 3, 6]              # and the tie at 0.03
    assert sel(p, "numTopFeatures", 50) == list(range(8))
    assert sel(p, "percentile", 0.3) == [1, 6]                      # int(8 * 0.3) = 2
    assert sel(p, "percentile", 0.1) == []
    assert sel(p, "fpr", 0.03) == [1, 3, 6]                         # strictly below alpha
    assert sel(p, "fwe", 0.09) == [1, 3, 6]                         # p < 0.09 / 8 = 0.01125
    assert sel(p, "fwe", 0.08) == [6]                               # 0.01 is not below 0.01
    # Benjamini-Hochberg at alpha = 0.05, d = 5: levels 0.01 .. 0.05; the second sorted p-value fails its level and
    # the third meets its own, so three are selected
    q = [0.9, 0.028, 0.005, 0.2, 0.025]
    assert sel(q, "fdr", 0.05) == [1, 2, 4]
    assert sel([0.9, 0.5, 0.2], "fdr", 0.05) == []
    assert sel(p, "fdr", 0.05) == [1, 2, 3, 5, 6]     # 0.03 <= 0.05 * 5 / 8 = 0.03125, 0.04 > 0.05 * 6 / 8 = 0.0375
    rng = np.random.default_rng(0)
    for _ in range(50):
        v = np.round(rng.random(9) ** 3, 2)                          # ties are common
        for mode, thr in [("numTopFeatures", 4), ("percentile", 0.5), ("fpr", 0.1), ("fdr", 0.2), ("fwe", 0.5)]:
            assert sel(v, mode, thr) == R.select(v, mode, thr), (v, mode)
    from cdnaml.models.util import IllegalArgumentException
    with pytest.raises(IllegalArgumentException):
        sel(p, "best", 1)


def test_selector_params():
    from cdnaml.ml.feature import ChiSqSelector, UnivariateFeatureSelector, VarianceThresholdSelector
    u = UnivariateFeatureSelector()
    assert (u.getFeaturesCol(), u.getLabelCol(), u.getSelectionMode()) == ("features", "label", "numTopFeatures")
    assert not u.isDefined("featureType") and not u.isDefined("labelType")
    for mode, thr in [("numTopFeatures", 50), ("percentile", 0.1), ("fpr", 0.05), ("fdr", 0.05), ("fwe", 0.05)]:
        assert u.setSelectionMode(mode).getSelectionThreshold() == thr
    assert u.setSelectionThreshold(3).getSelectionThreshold() == 3
    c = ChiSqSelector()
    assert (c.getNumTopFeatures(), c.getSelectorType(), c.getPercentile()) == (50, "numTopFeatures", 0.1)
    assert (c.getFpr(), c.getFdr(), c.getFwe()) == (0.05, 0.05, 0.05)
    assert VarianceThresholdSelector().getVarianceThreshold() == 0.0


# ------------------------------------------------------------------------------------------------ end to end
def _gap(p, cut_pairs):
    """Every (selected side, other side) pair of p-values or levels differs by a factor of at least 2."""
    for lo, hi in cut_pairs:
        assert hi >= 2 * lo, (lo, hi, p)


def _top_k_gap(p, k):
    s = np.sort(p)
    _gap(p, [(s[k - 1], s[k])])


def graded(kind, d=10, n=1500):
    """(X, label, the reference's p-values): features whose signal falls with the index."""
    from scipy.stats import chi2, f as f_dist
    if kind == "chi2":
        X, codes = R.make_counts(d, n, KC, CC, seed=4)
        ref = [R.chi2_reference(t) for t in R.count_table(X, codes, KC, CC)[0]]
        return X, codes, chi2.sf([r[0] for r in ref], [r[1] for r in ref])
    X, codes, y = R.make_continuous(d, n, CC, seed=4, dtype=np.float64)
    if kind == "anova":
        return X, codes, f_dist.sf(R.anova_f_reference(X, codes), CC - 1, n - CC)
    return X, y, f_dist.sf(R.fvalue_f_reference(X, y), 1, n - 2)


@pytest.mark.parametrize("kind,ftype,ltype", [("chi2", "categorical", "categorical"),
                                              ("anova", "continuous", "categorical"),
                                              ("fvalue", "continuous", "continuous")])
def test_univariate_selector_selects_what_the_reference_selects(spark, kind, ftype, ltype):
    from cdnaml.ml.feature import UnivariateFeatureSelector
    X, label, p = graded(kind)
    d = len(p)
    df = frame(spark, X, label)
    est = UnivariateFeatureSelector(outputCol="sel").setFeatureType(ftype).setLabelType(ltype)
    k = 3
    _top_k_gap(p, k)
    m = est.setSelectionMode("numTopFeatures").setSelectionThreshold(k).fit(df)
    assert m.selectedFeatures == R.select(p, "numTopFeatures", k) and len(m.selectedFeatures) == k
    _top_k_gap(p, int(d * 0.5))
    assert est.setSelectionMode("percentile").setSelectionThreshold(0.5).fit(df).selectedFeatures == \
        R.select(p, "percentile", 0.5)
    # an alpha, and an alpha / d, in the widest gap of the sorted p-values: at least a factor 4 wide, so every p-value
    # is a factor 2 away from the cut
    s = np.sort(p)
    i = int(np.argmax(s[1:] / s[:-1]))
    assert s[i + 1] >= 4 * s[i]
    alpha = float(np.sqrt(s[i] * s[i + 1]))
    _gap(p, [(s[i], alpha), (alpha, s[i + 1])])
    assert est.setSelectionMode("fpr").setSelectionThreshold(alpha).fit(df).selectedFeatures == \
        R.select(p, "fpr", alpha) == sorted(np.argsort(p)[:i + 1].tolist())
    assert alpha * d < 1
    assert est.setSelectionMode("fwe").setSelectionThreshold(alpha * d).fit(df).selectedFeatures == \
        R.select(p, "fwe", alpha * d) == sorted(np.argsort(p)[:i + 1].tolist())
    # Benjamini-Hochberg: no sorted p-value within a factor 2 of its level
    a = 0.05
    levels = a * (np.arange(d) + 1) / d
    assert all(max(x, l) >= 2 * min(x, l) for x, l in zip(s, levels))
    assert est.setSelectionMode("fdr").setSelectionThreshold(a).fit(df).selectedFeatures == R.select(p, "fdr", a)


def test_unsupported_and_unset_types_raise(spark):
    from cdnaml.ml.feature import UnivariateFeatureSelector
    from cdnaml.models.util import IllegalArgumentException
    X, label, _ = graded("anova", d=4, n=200)
    df = frame(spark, X, label)
    with pytest.raises(IllegalArgumentException):
        UnivariateFeatureSelector(outputCol="s").setFeatureType("categorical").setLabelType("continuous").fit(df)
    with pytest.raises(IllegalArgumentException):
        UnivariateFeatureSelector(outputCol="s").setLabelType("categorical").fit(df)
    with pytest.raises(IllegalArgumentException):
        UnivariateFeatureSelector(outputCol="s").setFeatureType("continuous").fit(df)


def test_chisq_and_variance_selectors(spark):
    from cdnaml.ml.feature import ChiSqSelector, VarianceThresholdSelector
    X, codes, p = graded("chi2")
    df = frame(spark, X, codes)
    _top_k_gap(p, 3)
    assert ChiSqSelector(numTopFeatures=3, outputCol="s").fit(df).selectedFeatures == R.select(p, "numTopFeatures", 3)
    _top_k_gap(p, 5)
    assert ChiSqSelector(selectorType="percentile", percentile=0.5, outputCol="s").fit(df).selectedFeatures == \
        R.select(p, "percentile", 0.5)
    s = np.sort(p)
    alpha = float(np.sqrt(s[0] * s[1]))
    assert s[1] >= 4 * s[0]
    assert ChiSqSelector(selectorType="fpr", fpr=alpha, outputCol="s").fit(df).selectedFeatures == \
        [int(np.argmin(p))]
    Xv = np.random.default_rng(8).normal(size=(300, 6)) * np.array([0.5, 1.0, 2.0, 0.0, 3.0, 1.5]) + 4.0
    var = Xv.var(0, ddof=1)
    dfv = frame(spark, Xv, np.zeros(300))
    assert VarianceThresholdSelector(outputCol="s").fit(dfv).selectedFeatures == [0, 1, 2, 4, 5]
    thr = 1.5                                              # between 1.0^2 and 1.5^2: far from every variance
    assert all(abs(v - thr) > 0.3 for v in var)
    assert VarianceThresholdSelector(outputCol="s", varianceThreshold=thr).fit(dfv).selectedFeatures == \
        [int(i) for i in np.nonzero(var > thr)[0]]


# ------------------------------------------------------------------------------------------------ transform etc.
def cat_frame(spark, n=240):
    """A string column whose categories {a, c} -> 1 and {b, d} -> 0 (no ordered split separates them), a constant
    and two noise columns; features = [cat index (nominal, 4 values), constant, noise, noise]."""
    from cdnaml.ml.feature import StringIndexer, VectorAssembler
    rng = np.random.default_rng(2)
    cat = np.array(list("abcd"))[np.arange(n) % 4]
    pdf = pd.DataFrame({"cat": cat, "const": np.full(n, 2.0), "u": rng.normal(size=n), "v": rng.normal(size=n),
                        "label": np.isin(cat, ["a", "c"]).astype(np.float64)})
    df = StringIndexer(inputCol="cat", outputCol="cat_idx", stringOrderType="alphabetAsc").fit(
        spark.createDataFrame(pdf)).transform(spark.createDataFrame(pdf))
    return VectorAssembler(inputCols=["const", "u", "cat_idx", "v"], outputCol="features").transform(df), pdf


def test_transform_keeps_dtype_and_attributes_and_feeds_a_forest(spark):
    from cdnaml.ml.classification import RandomForestClassifier
    from cdnaml.ml.feature import ChiSqSelectorModel, VarianceThresholdSelector
    from cdnaml.models.util import categorical_info, local_batch
    df, pdf = cat_frame(spark)
    m = VarianceThresholdSelector(outputCol="sel").fit(df)
    assert m.selectedFeatures == [1, 2, 3]                  # the constant goes
    out = m.transform(df)
    col = local_batch(out, ["sel"]).columns["sel"]
    assert col.values.dtype == torch.float64
    want = np.stack([pdf.u.to_numpy(), (np.arange(len(pdf)) % 4).astype(np.float64), pdf.v.to_numpy()], axis=1)
    assert np.array_equal(col.values.cpu().numpy(), want)
    meta = out.schema["sel"].metadata
    attrs = meta["ml_attr"]["attrs"]
    assert [a["idx"] for a in attrs] == [0, 1, 2] and [a["name"] for a in attrs] == ["u", "cat_idx", "v"]
    assert categorical_info(meta, 3, "sel") == {1: 4}
    # behind the selector the forest still splits on category sets
    rf = RandomForestClassifier(featuresCol="sel", numTrees=1, maxDepth=1, featureSubsetStrategy="all",
                                bootstrap=False, seed=1).fit(out)
    assert " in {" in rf.toDebugString
    pred = rf.transform(out).select("prediction").toPandas().prediction.to_numpy()
    assert np.array_equal(pred, pdf.label.to_numpy())
    # a model made by hand slices in the order of the indices
    hand = ChiSqSelectorModel([2]).setFeaturesCol("features").setOutputCol("one")
    assert categorical_info(hand.transform(df).schema["one"].metadata, 1, "one") == {0: 4}


def test_persistence_and_pipeline(spark, tmp_path):
    from cdnaml.ml import Pipeline, PipelineModel
    from cdnaml.ml.feature import (ChiSqSelector, ChiSqSelectorModel, UnivariateFeatureSelector,
                                   UnivariateFeatureSelectorModel, VarianceThresholdSelector,
                                   VarianceThresholdSelectorModel, VectorAssembler)
    X, codes, _ = graded("chi2", d=6, n=300)
    df = frame(spark, X, codes)
    fits = [(UnivariateFeatureSelector(outputCol="o", selectionMode="numTopFeatures").setFeatureType("categorical")
             .setLabelType("categorical").setSelectionThreshold(2), UnivariateFeatureSelectorModel),
            (ChiSqSelector(numTopFeatures=2, outputCol="o"), ChiSqSelectorModel),
            (VarianceThresholdSelector(outputCol="o", varianceThreshold=0.1), VarianceThresholdSelectorModel)]
    for i, (est, cls) in enumerate(fits):
        m = est.fit(df)
        m.write().overwrite().save(str(tmp_path / f"m{i}"))
        back = cls.load(str(tmp_path / f"m{i}"))
        assert type(back) is cls and back.selectedFeatures == m.selectedFeatures and back.getOutputCol() == "o"
        a, b = (np.stack([v.toArray() for v in s.transform(df).select("o").toPandas().o]) for s in (m, back))
        assert np.array_equal(a, b) and np.array_equal(a, X[:, m.selectedFeatures].astype(np.float64))
    names = [f"x{i}" for i in range(6)]
    pdf = pd.DataFrame(X.astype(np.float64), columns=names)
    pdf["label"] = codes.astype(np.float64)
    raw = spark.createDataFrame(pdf)
    pm = Pipeline(stages=[VectorAssembler(inputCols=names, outputCol="features"), fits[0][0]]).fit(raw)
    pm.write().overwrite().save(str(tmp_path / "pipe"))
    pb = PipelineModel.load(str(tmp_path / "pipe"))
    assert isinstance(pb.stages[-1], UnivariateFeatureSelectorModel)
    assert pb.stages[-1].selectedFeatures == pm.stages[-1].selectedFeatures
    assert pb.transform(raw).select("o").head()[0] == pm.transform(raw).select("o").head()[0]


def test_pyspark_aliases():
    import cdnaml.compat
    cdnaml.compat.install()
    import pyspark.ml.feature as F
    import pyspark.ml.stat as S
    from cdnaml.ml import feature, stat
    for name in ("UnivariateFeatureSelector", "UnivariateFeatureSelectorModel", "ChiSqSelector", "ChiSqSelectorModel",
                 "VarianceThresholdSelector", "VarianceThresholdSelectorModel"):
        assert getattr(F, name) is getattr(feature, name)
    for name in ("ChiSquareTest", "ANOVATest", "FValueTest"):
        assert getattr(S, name) is getattr(stat, name)
