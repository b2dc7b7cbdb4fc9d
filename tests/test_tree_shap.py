"""TreeSHAP feature contributions (K21 tree_shap_kernel, K.tree_shap, Forest.shap_values, contributionsCol /
pred_contrib_col): exactness against brute-force Shapley enumeration, device = host, determinism, additivity
through the model API, persistence and the unsupported cases."""
import functools
import itertools
import math
import pickle

import numpy as np
import pandas as pd
import pytest
import torch

import cdnaml
from cdnaml.ml.classification import GBTClassifier, RandomForestClassifier
from cdnaml.ml.feature import VectorAssembler
from cdnaml.ml.regression import DecisionTreeRegressor, GBTRegressor, RandomForestRegressor
from cdnaml.ml.xgboost import XgboostClassifier, XgboostRegressor
from cdnaml.models.tree.forest import Forest
from cdnaml.models.util import local_batch
from cdnaml.ops import kernels as K

from tests.conftest import session_device

D = 6
CAT = 4  # the categorical feature of the hand-built trees


# ------------------------------------------------------------------ hand-built forests
def _leaf(v):
    return ("leaf", v)


def _num(f, thr, frac, left, right):
    return ("num", f, thr, frac, left, right)


def _cat(f, cats, frac, left, right):
    return ("cat", f, cats, frac, left, right)


def _tree_a():
    """Depth 6; feature 0 three times on one path; a categorical split; cover fractions 1e-3 and 0.999."""
    deep = _num(3, 1.0, 0.7, _num(0, -1.5, 0.2, _leaf(0.5), _leaf(1.5)), _leaf(3.0))
    left = _num(1, -0.25, 1e-3, _leaf(2.0),
                _num(0, -0.5, 0.3, _num(2, 0.0, 0.5, _leaf(-1.0), deep), _leaf(0.25)))
    right = _cat(CAT, (1, 3, 200), 0.4, _leaf(-2.0), _num(5, 2.0, 0.999, _leaf(1.0), _leaf(4.0)))
    return _num(0, 0.5, 0.6, left, right)


def _tree_b():
    return _cat(CAT, (0, 2, 255), 0.25, _num(1, 0.0, 0.5, _leaf(1.0), _leaf(-1.0)),
                _num(2, 0.0, 0.01, _leaf(5.0), _num(1, 0.75, 0.5, _leaf(-3.0), _leaf(2.0))))


def _mirror(spec):
    """The same tree with every cover fraction f replaced by 1 - f."""
    if spec[0] == "leaf":
        return spec
    kind, f, arg, frac, lt, rt = spec
    return (kind, f, arg, 1.0 - frac, _mirror(lt), _mirror(rt))


def _build(specs, root_cover=1000.0):
    forest = Forest(1)

    def add(spec, cover, depth):
        if spec[0] == "leaf":
            return forest.add([spec[1]], cover, depth)
        kind, f, arg, frac, lt, rt = spec
        i = forest.add([0.0], cover, depth)
        lc = cover * frac
        li, ri = add(lt, lc, depth + 1), add(rt, cover - lc, depth + 1)
        forest.feat[i], forest.left[i], forest.right[i] = f, li, ri
        if kind == "num":
            forest.thr[i] = arg
        else:
            m = np.zeros(8, dtype=np.uint32)
            for c in arg:
                m[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
            forest.is_cat[i] = True
            forest.catmask[i] = m
        return i
    for s in specs:
        forest.roots.append(add(s, root_cover, 0))
    return forest


@functools.lru_cache(maxsize=None)
def hand_forests():
    """[(forest, tree weights, base)]: 3 trees each, d = 6, depth <= 6, one single-leaf tree."""
    return [(_build([_tree_a(), _leaf(0.7), _tree_b()]), np.array([1.0, 0.5, -0.75]), 0.3),
            (_build([_leaf(-1.25), _mirror(_tree_b()), _mirror(_tree_a())], 37.0), np.array([0.1, 2.0, 1.0]), -2.0)]


@functools.lru_cache(maxsize=None)
def hand_rows():
    """200 rows: NaNs in numeric features, values exactly on thresholds, categories outside [0, 256), and NaN
    categories (every 9th row: _tree_b's mask has bit 0 set, so category 0 and NaN part there)."""
    rng = np.random.default_rng(7)
    X = rng.normal(size=(200, D)).astype(np.float32)
    X[:, CAT] = rng.choice([-3.0, 0.0, 1.0, 2.0, 2.7, 3.0, 200.0, 255.0, 256.0, 300.0, 1e10], size=200)
    X[::9, CAT] = np.nan
    thr = np.array([0.5, -0.25, -0.5, 0.0, 1.0, 2.0, 0.75, -1.5], dtype=np.float32)
    for f in (0, 1, 2, 3, 5):
        hit = rng.uniform(size=200) < 0.25
        X[hit, f] = rng.choice(thr, size=int(hit.sum()))
        X[rng.uniform(size=200) < 0.1, f] = np.nan
    return torch.from_numpy(X)


# ------------------------------------------------------------------ brute-force oracle
def _goes_left(forest, i, x):
    v = x[forest.feat[i]]
    if forest.is_cat[i]:
        if not (v == v) or not 0 <= v < 256:  # a NaN category goes right, like one outside [0, 256)
            return False
        c = int(v)
        return bool((int(forest.catmask[i][c >> 5]) >> (c & 31)) & 1)
    return bool(np.float32(v) <= np.float32(forest.thr[i]))  # NaN: False, goes right


def _cond_exp(forest, i, x, S):
    """E[tree | x_S]: follow x at splits on features in S, average the children by cover otherwise."""
    if forest.feat[i] < 0:
        return float(forest.value[i][0])
    lt, rt = forest.left[i], forest.right[i]
    if forest.feat[i] in S:
        return _cond_exp(forest, lt if _goes_left(forest, i, x) else rt, x, S)
    return (forest.weight[lt] * _cond_exp(forest, lt, x, S) + forest.weight[rt] * _cond_exp(forest, rt, x, S)) \
        / forest.weight[i]


def brute_shap(forest, tree_w, base, X):
    """Shapley values by subset enumeration over the features each tree uses (pure Python, fp64)."""
    X = X.numpy()
    n, d = X.shape
    phi = np.zeros((n, d + 1))
    phi[:, d] = base
    for t, root in enumerate(forest.roots):
        used = sorted({forest.feat[i] for i in forest.tree_nodes(t) if forest.feat[i] >= 0})
        u = len(used)
        subsets = [frozenset(c) for k in range(u + 1) for c in itertools.combinations(used, k)]
        for r in range(n):
            val = {S: _cond_exp(forest, root, X[r], S) for S in subsets}
            phi[r, d] += tree_w[t] * val[frozenset()]
            for f in used:
                for S in subsets:
                    if f not in S:
                        w = math.factorial(len(S)) * math.factorial(u - len(S) - 1) / math.factorial(u)
                        phi[r, f] += tree_w[t] * w * (val[S | {f}] - val[S])
    return phi


@functools.lru_cache(maxsize=None)
def hand_oracle(k):
    forest, tw, base = hand_forests()[k]
    return brute_shap(forest, tw, base, hand_rows())


def _scale(forest, tw):
    leaves = forest.value.array()[forest.feat.array() < 0, 0]
    return float(np.abs(tw).sum() * np.abs(leaves).max())


# Observed maximum error of the CPU path against the enumeration, relative to sum_t |w_t| * max |leaf|:
# 7.9e-17 (forest 0) and 3.44e-16 (forest 1).  Asserted at 100x the larger: the margin covers the 1 / z
# amplification at the 1e-3 cover fractions.
ORACLE_TOL = 100 * 3.44e-16
CROSS_TOL = 1e-12  # the project's cross-device tolerance for tree outputs (tests/parity/test_cross_device.py)


@pytest.mark.parametrize("k", [0, 1])
def test_cpu_path_matches_enumeration(k):
    forest, tw, base = hand_forests()[k]
    X = hand_rows()
    phi = forest.shap_values(X, tw, [base])
    assert phi.dtype == torch.float64 and tuple(phi.shape) == (200, D + 1)
    err = np.abs(phi.numpy() - hand_oracle(k)).max() / _scale(forest, tw)
    print(f"forest {k}: max error vs enumeration / scale = {err:.3e}")
    assert err <= ORACLE_TOL
    # every row sums to the raw prediction
    pred = forest.predict(X, tw, [base])[:, 0]
    assert float((phi.sum(1) - pred).abs().max()) <= CROSS_TOL * _scale(forest, tw)


@pytest.mark.gpu
@pytest.mark.parametrize("phi_mode", ["lds", "global"])
@pytest.mark.parametrize("k", [0, 1])
def test_gpu_kernel_matches_enumeration(gpu_device, k, phi_mode):
    forest, tw, base = hand_forests()[k]
    X = hand_rows()
    phi = forest.shap_values(X.to(gpu_device), tw, [base], phi=phi_mode).cpu()
    s = _scale(forest, tw)
    err = np.abs(phi.numpy() - hand_oracle(k)).max() / s
    print(f"forest {k} ({phi_mode}): max error vs enumeration / scale = {err:.3e}")
    assert err <= ORACLE_TOL
    assert float((phi - forest.shap_values(X, tw, [base])).abs().max()) <= CROSS_TOL * s


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("k", [0, 1])
def test_margin_of_the_same_pass_is_the_prediction(device, k):
    """with_margin: base + the weighted value of the leaf reached in every tree, summed in fp64 by the same pass,
    equals Forest.predict; the device gives the host path's bits."""
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no GPU")
    forest, tw, base = hand_forests()[k]
    X = hand_rows()
    phi, margin = forest.shap_values(X.to(device), tw, [base], with_margin=True)
    assert margin.dtype == torch.float64 and tuple(margin.shape) == (200,)
    assert torch.equal(phi, forest.shap_values(X.to(device), tw, [base]))
    s = _scale(forest, tw)
    assert float((margin - forest.predict(X.to(device), tw, [base])[:, 0]).abs().max()) <= CROSS_TOL * s
    assert float((phi.sum(1) - margin).abs().max()) <= CROSS_TOL * s
    if device == "cuda":
        assert torch.equal(margin.cpu(), forest.shap_values(X, tw, [base], with_margin=True)[1])
    e_phi, e_margin = forest.shap_values(X[:0].to(device), tw, [base], with_margin=True)
    assert tuple(e_phi.shape) == (0, D + 1) and tuple(e_margin.shape) == (0,)


def test_flattening_layout_and_cache():
    forest, tw, base = hand_forests()[0]
    sp = forest.shap_paths()
    assert forest.shap_paths() is sp                       # cached
    leaves = [i for t in range(3) for i in forest.tree_nodes(t) if forest.feat[i] < 0]
    assert sp["leaf"].tolist() == leaves                   # trees ascending, leaves in left-first DFS order
    assert sp["hdr"][:, 3].max() == sp["max_slots"] == 4   # f0 (x3), f1, f2, f3 merge into 4 slots
    single = sp["hdr"][sp["tree"] == 1]
    assert single.shape[0] == 1 and single[0, 1] == 0 and single[0, 3] == 0   # the single-leaf tree: m = 0
    # the deepest path of tree 0: feature 0 three times -> one slot with the product of its three fractions
    p = int(np.argmax(sp["hdr"][:, 1]))
    assert sp["hdr"][p, 1] == 6
    k0 = sp["hdr"][p, 2]
    assert sp["slot_feat"][k0] == 0 and sp["slot_z"][k0] == pytest.approx(0.6 * 0.3 * 0.2, rel=1e-12)
    assert "_shap" not in forest.__getstate__()            # never pickled
    clone = pickle.loads(pickle.dumps(forest))
    assert torch.equal(clone.shap_values(hand_rows(), tw, [base]), forest.shap_values(hand_rows(), tw, [base]))


# ------------------------------------------------------------------ fitted forests: GPU kernel = CPU path
def _frame(spark, n, d, seed):
    dev = spark.device
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((n, d), generator=g)
    w = torch.linspace(1.0, 2.0, d, dtype=torch.float32)
    y = ((X[:, : min(d, 24)] > 0.3).float() * w[: min(d, 24)]).sum(1) + X[:, 0] * X[:, 1] + 0.5 * X[:, d - 1]
    return spark.createDataFrameFromLocalTensors({"features": X.to(dev), "label": y.double().to(dev)}), X


@functools.lru_cache(maxsize=None)
def fitted(case, device="cuda"):
    """(forest, tree weights, fp32 rows) of the cross-device cases, fitted once (on the GPU by default)."""
    with session_device(device):
        spark = cdnaml.SparkSession.builder.getOrCreate()
        try:
            if case == "dt12":
                df, X = _frame(spark, 2000, 20, 5)
                m = DecisionTreeRegressor(maxDepth=12, seed=3).fit(df)
                return m._forest, m._tree_w, X[:193]
            d = {"rf100": 100, "rf7": 7, "rf300": 300}[case]
            df, X = _frame(spark, 4096, d, d)
            m = RandomForestRegressor(numTrees=20, maxDepth=5, seed=1).fit(df)
            return m._forest, m._tree_w, X[:193]
        finally:
            spark.stop()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rf100", "rf7", "rf300", "dt12"])
def test_gpu_kernel_equals_cpu_path(gpu_device, case):
    """n = 193 (a 1-row tile tail); d = 100 (float4 row loads), d = 7 (scalar row loads), d = 300 (the phi tile
    beyond LDS: the global arrangement), a depth-12 tree (more than 8 slots: the 16-slot instantiation)."""
    forest, tw, X = fitted(case)
    sp = forest.shap_paths()
    if case == "dt12":
        assert 8 < sp["max_slots"] <= 16
    if case == "rf300":
        L = cdnaml.ops._lib.lib()
        assert L.cdna_tree_shap_lds_bytes(300, 0) > L.cdna_tree_shap_lds_budget()
    ref = forest.shap_values(X, tw, [0.0])
    got = forest.shap_values(X.to(gpu_device), tw, [0.0])
    assert got.dtype == torch.float64 and tuple(got.shape) == (193, X.shape[1] + 1)
    s = _scale(forest, tw)
    err = float((got.cpu() - ref).abs().max()) / s
    print(f"{case}: max |gpu - cpu| / scale = {err:.3e}")
    assert err <= CROSS_TOL
    pred = forest.predict(X.to(gpu_device), tw, [0.0])[:, 0]
    assert float((got.sum(1) - pred).abs().max()) <= CROSS_TOL * s
    if case in ("rf100", "rf7"):  # the LDS arrangement of the phi tile gives the same bits as the global one
        alt = forest.shap_values(X.to(gpu_device), tw, [0.0], phi="lds")
        assert torch.equal(alt, got)


@pytest.mark.gpu
def test_gpu_empty_and_single_row(gpu_device):
    forest, tw, X = fitted("rf100")
    ref = forest.shap_values(X[:1], tw, [1.5])
    got = forest.shap_values(X[:1].to(gpu_device), tw, [1.5])
    assert float((got.cpu() - ref).abs().max()) <= CROSS_TOL * _scale(forest, tw)
    for dev in ("cpu", gpu_device):
        e = forest.shap_values(X[:0].to(dev), tw, [1.5])
        assert tuple(e.shape) == (0, 101) and e.dtype == torch.float64


def test_cpu_empty_and_single_row():
    forest, tw, base = hand_forests()[0]
    X = hand_rows()
    assert tuple(forest.shap_values(X[:0], tw, [base]).shape) == (0, D + 1)
    assert torch.equal(forest.shap_values(X[:1], tw, [base]), forest.shap_values(X, tw, [base])[:1])


@pytest.mark.gpu
def test_gpu_rows_do_not_depend_on_the_batch(gpu_device):
    """Rows 0..63 computed alone and inside the 193-row batch are bit-identical."""
    forest, tw, X = fitted("rf100")
    Xd = X.to(gpu_device)
    whole = forest.shap_values(Xd, tw, [0.0])
    alone = forest.shap_values(Xd[:64].contiguous(), tw, [0.0])
    assert torch.equal(alone, whole[:64])
    assert torch.equal(forest.shap_values(Xd, tw, [0.0]), whole)


# ------------------------------------------------------------------ the model API
def _assembled(spark, n=600, seed=0, with_missing=False, binary=False):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 5))
    if with_missing:
        X[rng.uniform(size=n) < 0.25, 0] = 0.0
        X[rng.uniform(size=n) < 0.1, 2] = np.nan
    x2 = np.nan_to_num(X[:, 2])
    y = np.where(X[:, 0] == 0, 3.0, 2 * X[:, 0]) + X[:, 1] ** 2 - x2 + 0.1 * rng.normal(size=n)
    pdf = pd.DataFrame(X, columns=list("abcde"))
    pdf["label"] = (y > np.median(y)).astype(float) if binary else y
    va = VectorAssembler(inputCols=list("abcde"), outputCol="features", handleInvalid="keep")
    return va.transform(spark.createDataFrame(pdf))


def _col(df, name):
    return local_batch(df, [name]).columns[name].values.double().cpu()


def _expected_bias(forest, tw, base):
    """base + sum_t w_t E_t from the node fields: E_t = sum over leaves of cover * value / cover(root)."""
    b = base
    for t, root in enumerate(forest.roots):
        e = sum(forest.weight[i] * float(forest.value[i][0]) for i in forest.tree_nodes(t) if forest.feat[i] < 0)
        b += tw[t] * e / forest.weight[root]
    return b


def _model_case(spark, name):
    """(fitted model, frame, name of the contributions param, margin of the transformed frame, weights, base)."""
    if name == "rf":
        df = _assembled(spark)
        m = RandomForestRegressor(numTrees=5, maxDepth=4, seed=2).fit(df)
    elif name == "gbt":
        df = _assembled(spark)
        m = GBTRegressor(maxIter=5, maxDepth=3, seed=2).fit(df)
    elif name == "gbtc":
        df = _assembled(spark, binary=True)
        m = GBTClassifier(maxIter=5, maxDepth=3, seed=2).fit(df)
    elif name == "xgb":
        df = _assembled(spark, with_missing=True)
        m = XgboostRegressor(n_estimators=6, max_depth=3, missing=0, random_state=1).fit(df)
    else:
        df = _assembled(spark, with_missing=True, binary=True)
        m = XgboostClassifier(n_estimators=6, max_depth=3, random_state=1).fit(df)
    return m, df


def _margin_and_weights(m, out, name):
    if name in ("rf", "gbt"):
        return _col(out, "prediction"), m._tree_w, 0.0
    if name == "gbtc":
        return _col(out, "rawPrediction")[:, 1], m._tree_w, 0.0
    tw = np.full(len(m._forest.roots), m.getLearning_rate())
    if name == "xgb":
        return _col(out, "prediction"), tw, m._base
    return _col(out, "rawPrediction")[:, 1], tw, m._base


def _check_additive(m, df, name):
    param = "contributionsCol" if name in ("rf", "gbt", "gbtc") else "pred_contrib_col"
    out = m.copy({m.getParam(param): "phi"}).transform(df)
    phi = _col(out, "phi")
    margin, tw, base = _margin_and_weights(m, out, name)
    assert tuple(phi.shape) == (margin.shape[0], 6)
    s = _scale(m._forest, tw)
    gap = float((phi.sum(1) - margin).abs().max())
    bias = _expected_bias(m._forest, tw, base)
    print(f"{name}: max |row sum - margin| / scale = {gap / s:.3e}; bias {float(phi[0, 5])!r} vs {bias!r}")
    assert float((phi[:, 5] - bias).abs().max()) <= CROSS_TOL * max(s, abs(bias))
    assert gap <= CROSS_TOL * s
    return phi


@pytest.mark.parametrize("name", ["rf", "gbt", "gbtc", "xgb", "xgbc"])
def test_contributions_are_additive_through_the_api(spark, tmp_path, name):
    """Row sums of the contributions column equal the raw prediction / margin column to 1e-12 relative, the
    last entry equals base + sum_t w_t E_t, and both hold after save / load.

    The XGBoost models report an fp32 margin (``_margins``); with ``pred_contrib_col`` set they report the fp64
    margin that the contributions' pass sums from the leaves themselves, so the two columns can agree to 1e-12
    (``test_xgb_contributions_sum_to_the_fp64_margin`` checks that margin against a walk written in the test and
    against the fp32 one)."""
    m, df = _model_case(spark, name)
    phi = _check_additive(m, df, name)
    path = str(tmp_path / name)
    m.write().overwrite().save(path)
    again = _check_additive(type(m).load(path), df, name)
    assert torch.equal(again, phi)


@pytest.mark.parametrize("binary", [False, True])
def test_xgb_contributions_sum_to_the_fp64_margin(spark, binary):
    """With pred_contrib_col set the XGBoost models report base + eta * sum_t leaf value summed in fp64: it and the
    contributions' row sums equal, to 1e-12 relative, that sum made here in fp64 over a walk of the model's own
    bins written in the test.  Against the fp32 margin the models report without the param they agree to its
    rounding: T + 1 fp32 additions and T leaf values rounded to fp32, each within 2^-24 of the running magnitude
    <= |base| + scale."""
    m, df = _model_case(spark, "xgbc" if binary else "xgb")
    name = "rawPrediction" if binary else "prediction"
    on, off = m.copy({m.pred_contrib_col: "phi"}).transform(df), m.transform(df)
    phi = _col(on, "phi")
    margin_on, margin32 = _col(on, name), _col(off, name)
    if binary:
        margin_on, margin32 = margin_on[:, 1], margin32[:, 1]
        assert torch.equal(_col(on, "prediction"), _col(off, "prediction"))
        assert float((_col(on, "probability") - _col(off, "probability")).abs().max()) < 1e-6
    X = local_batch(df, ["features"]).columns["features"].values
    assert torch.equal(margin32, m._margins(X)[:, 0].double().cpu())  # param unset: the fp32 predictor as before
    B = K.bins_to_matrix(m._bins(X), 5).cpu().tolist()
    f, eta = m._forest, m.getLearning_rate()
    margin64 = []
    for row in B:
        acc = m._base
        for root in f.roots:
            i = root
            while f.feat[i] >= 0:
                b = row[f.feat[i]]
                left = (int(f.catmask[i][b >> 5]) >> (b & 31)) & 1 if f.is_cat[i] else b <= f.bin[i]
                i = f.left[i] if left else f.right[i]
            acc += eta * float(f.value[i][0])
        margin64.append(acc)
    margin64 = torch.tensor(margin64, dtype=torch.float64)
    T_ = len(f.roots)
    s = _scale(f, np.full(T_, eta)) + abs(m._base)
    assert float((margin_on - margin64).abs().max()) <= CROSS_TOL * s
    assert float((phi.sum(1) - margin64).abs().max()) <= CROSS_TOL * s
    assert float((margin_on - margin32).abs().max()) <= (2 * T_ + 1) * 2.0 ** -24 * s


def test_feature_contributions_method(spark):
    df = _assembled(spark)
    m = DecisionTreeRegressor(maxDepth=3, seed=1).fit(df)
    out = m.featureContributions(df)
    assert "contributions" in out.columns and m.getContributionsCol() == ""
    phi = _col(out, "contributions")
    assert float((phi.sum(1) - _col(out, "prediction")).abs().max()) <= CROSS_TOL * _scale(m._forest, m._tree_w)


# ------------------------------------------------------------------ rejections and the unchanged default
def test_unsupported_models_raise(spark):
    df = _assembled(spark, n=300, binary=True)
    rfc = RandomForestClassifier(numTrees=3, maxDepth=3, seed=1).fit(df)
    with pytest.raises(NotImplementedError, match="single-output"):
        rfc.setContributionsCol("phi").transform(df)
    with pytest.raises(NotImplementedError, match="single-output"):
        rfc._forest.shap_values(torch.zeros((1, 5)), rfc._tree_w)
    pdf = df.toPandas()
    pdf["label"] = np.arange(len(pdf)) % 3
    df3 = spark.createDataFrame(pdf)
    xm = XgboostClassifier(n_estimators=2, max_depth=2).fit(df3)
    assert xm._n_out == 3
    with pytest.raises(NotImplementedError, match="multi:softprob"):
        xm.copy({xm.pred_contrib_col: "phi"}).transform(df3)


def test_zero_cover_child_and_too_many_slots_raise():
    forest = _build([_num(0, 0.0, 0.0, _leaf(1.0), _leaf(2.0))])  # the left child has cover 0
    with pytest.raises(ValueError, match=r"child 1 of node 0 .* zero cover"):
        forest.shap_values(torch.zeros((2, 1)), [1.0])
    chain = _leaf(1.0)
    for f in range(33):  # a path over 33 distinct features
        chain = _num(f, 0.0, 0.5, chain, _leaf(float(f)))
    deep = _build([chain])
    with pytest.raises(ValueError, match="at most 32"):
        deep.shap_values(torch.zeros((2, 33)), [1.0])
    ok = _build([chain[4]])  # 32 distinct features: the largest supported path
    phi = ok.shap_values(torch.zeros((2, 33)), [1.0])
    assert float((phi.sum(1) - ok.predict(torch.zeros((2, 33)), [1.0])[:, 0]).abs().max()) <= CROSS_TOL * 32.0


def test_default_transform_is_unchanged(spark):
    """With both new params unset the models emit the columns and values they emitted before."""
    df = _assembled(spark)
    rf = RandomForestRegressor(numTrees=3, maxDepth=3, seed=2).fit(df)
    assert rf.getContributionsCol() == ""
    out = rf.transform(df)
    assert out.columns == df.columns + ["prediction"]
    assert [f.dataType.simpleString() for f in out.schema.fields][-1] == "double"
    on = rf.copy({rf.contributionsCol: "phi"}).transform(df)
    assert on.columns == df.columns + ["prediction", "phi"]
    assert torch.equal(_col(on, "prediction"), _col(out, "prediction"))
    X = local_batch(df, ["features"]).columns["features"].values
    assert torch.equal(_col(out, "prediction"), rf._forest.predict(X, rf._tree_w, [0.0])[:, 0].cpu())
    xg = XgboostRegressor(n_estimators=3, max_depth=2).fit(df)
    assert xg.getOrDefault("pred_contrib_col") is None
    xo = xg.transform(df)
    assert xo.columns == df.columns + ["prediction"]
    xon = xg.copy({xg.pred_contrib_col: "phi"}).transform(df)
    assert xon.columns == df.columns + ["prediction", "phi"]
    assert torch.equal(_col(xo, "prediction"), xg._margins(X)[:, 0].double().cpu())
    # with the param set the margin is summed in fp64: the fp32 one to its rounding (3 trees)
    assert float((_col(xon, "prediction") - _col(xo, "prediction")).abs().max()) <= 7 * 2.0 ** -24 * (
        _scale(xg._forest, np.full(3, xg.getLearning_rate())) + abs(xg._base))
