"""K27 ``label_stats`` on the device against the references of ``tests/_select_refs.py``, and UnivariateFeatureSelector
fitted end to end on the GPU.

COUNT tables and bad counts must equal numpy's exactly.  The CLASS and REGRESS sums meet the criterion of the
host-formulation tests: the kernel's error against the longdouble reference may be M = 8 times the error of the plain
numpy fp64 yardstick, with a floor of 4 fp64 ulps (2^-53) of the largest entry.  Every case first asserts the plan, so
none silently tests the host formulation, and counts the native calls; the sums' cases print their kernel / yardstick
figures before they assert (``-s`` shows them; profiles/r17/select.md records a run).
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _select_refs as R
from tests.conftest import session_device
from tests.test_aft_gpu import Counting

pytestmark = pytest.mark.gpu

N2 = 1025           # the smallest n the plan gives two blocks (asserted)
KC, CC = 7, 3       # the shapes' categories and classes

# (d, n, load width): tile boundaries; d around the float4 loads and the 32-lane halves; the edge of the native range;
# two blocks
SHAPES = [(5, 1, 1), (5, 63, 1), (5, 64, 1), (5, 65, 1), (5, 130, 1),
          (1, 130, 1), (3, 130, 1), (4, 130, 4), (31, 130, 1), (32, 130, 4), (33, 130, 1),
          (127, 600, 1), (128, 600, 4), (100, N2, 4)]


def dev_np(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


def same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def assert_plan(Xd, mode, C, K_, vw, n):
    plan = K.label_stats_plan(Xd, mode, C=C, K=K_)
    assert (plan["path"], plan["vw"]) == ("native", vw), plan
    assert plan["nblk"] == (2 if n >= N2 else 1), plan
    if n == N2:
        assert K.label_stats_plan(Xd[:N2 - 1], mode, C=C, K=K_)["nblk"] == 1
    return plan


def count(Xd, cd, C=CC, K_=KC, **kw):
    return K.label_stats(Xd, cd, K.LABEL_COUNT, C=C, K=K_, **kw)


def assert_count(st, table, bad, bad_label):
    got = dev_np(st)
    assert got["table"].dtype == np.int64 and got["table"].shape == table.shape
    assert np.array_equal(got["table"], table)
    assert np.array_equal(got["bad"], bad) and int(got["bad_label"]) == bad_label


@pytest.mark.parametrize("d,n,vw", SHAPES)
def test_count_equals_numpy(gpu_device, d, n, vw):
    c = R.count_case(d, n, KC, CC)
    Xd, cd = torch.tensor(c["X"], device=gpu_device), torch.tensor(c["codes"], device=gpu_device)
    assert_plan(Xd, K.LABEL_COUNT, CC, KC, vw, n)
    with Counting() as calls:
        a = count(Xd, cd)
        b = count(Xd, cd)
    assert calls.count("cdna_label_stats") == 2, calls
    assert same_bits(a, b)
    assert_count(a, c["table"], c["bad"], c["bad_label"])
    assert int(a["table"].sum()) == n * d


@pytest.mark.parametrize("d,n,vw", SHAPES)
def test_class_and_regress_match_reference(gpu_device, d, n, vw):
    c = R.cont_case(d, n, CC)
    Xd = torch.tensor(c["X"], device=gpu_device)
    cd, yd = torch.tensor(c["codes"], device=gpu_device), torch.tensor(c["y"], device=gpu_device)
    assert np.abs(c["shift"]).max() > 0 and c["yshift"] != 0
    assert_plan(Xd, K.LABEL_CLASS, CC, 1, vw, n)
    assert_plan(Xd, K.LABEL_REGRESS, 1, 1, vw, n)
    with Counting() as calls:
        a = K.label_stats(Xd, cd, K.LABEL_CLASS, C=CC, shift=c["shift"])
        b = K.label_stats(Xd, cd, K.LABEL_CLASS, C=CC, shift=c["shift"])
        r = K.label_stats(Xd, yd, K.LABEL_REGRESS, shift=c["shift"], yshift=c["yshift"])
        s = K.label_stats(Xd, yd, K.LABEL_REGRESS, shift=c["shift"], yshift=c["yshift"])
    assert calls.count("cdna_label_stats") == 4, calls
    # no float atomics: the same bits twice
    assert same_bits(a, b) and same_bits(r, s)
    assert a["sums"].shape == (CC, d) and a["sums"].dtype == torch.float64
    R.check_class(f"class d={d} n={n}", dev_np(a), c["cls"], c["y_cls"])
    R.check_regress(f"regress d={d} n={n}", dev_np(r), c["reg"], c["y_reg"])
    for st in (a, r):
        assert float(st["bad"].sum()) == 0.0 and float(st["bad_label"]) == 0.0


# K = 1; C = 2, 3, 32; K C a multiple of 64, where a [column][category][label] table would put a wave in one bank
@pytest.mark.parametrize("K_,C", [(1, 3), (7, 2), (7, 3), (5, 32), (16, 4), (2, 32), (64, 2)])
def test_count_categories_and_labels(gpu_device, K_, C):
    d, n = 33, 600
    c = R.count_case(d, n, K_, C)
    Xd, cd = torch.tensor(c["X"], device=gpu_device), torch.tensor(c["codes"], device=gpu_device)
    assert K.label_stats_plan(Xd, K.LABEL_COUNT, C=C, K=K_)["path"] == "native"
    with Counting() as calls:
        st = count(Xd, cd, C, K_)
    assert calls.count("cdna_label_stats") == 1, calls
    assert_count(st, c["table"], c["bad"], 0)


def test_count_at_the_budget_and_the_first_table_past_it(gpu_device):
    """d = 128: the table's pitch is 129 cells, and the budget admits K C <= budget / (4 * 129)."""
    d, n = 128, 600
    budget = K.label_stats_plan(torch.zeros((4, 4), device=gpu_device), K.LABEL_COUNT)["count_budget"]
    assert budget == 96 * 1024
    top = budget // (4 * (d | 1))
    assert top % 2 == 0
    for K_, C in [(top, 1), (top // 2, 2)]:
        c = R.count_case(d, n, K_, C)
        Xd, cd = torch.tensor(c["X"], device=gpu_device), torch.tensor(c["codes"], device=gpu_device)
        plan = K.label_stats_plan(Xd, K.LABEL_COUNT, C=C, K=K_)
        assert (plan["path"], plan["vw"], plan["blocks_per_cu"]) == ("native", 4, 1), plan
        assert plan["lds"] <= 160 * 1024
        with Counting() as calls:
            st = count(Xd, cd, C, K_)
        assert calls.count("cdna_label_stats") == 1, calls
        assert_count(st, c["table"], c["bad"], 0)
    for K_, C in [(top + 1, 1), (top // 2 + 1, 2)]:
        c = R.count_case(d, n, K_, C)
        Xd, cd = torch.tensor(c["X"], device=gpu_device), torch.tensor(c["codes"], device=gpu_device)
        assert K.label_stats_plan(Xd, K.LABEL_COUNT, C=C, K=K_) == {"path": "host"}
        with Counting() as calls:
            st = count(Xd, cd, C, K_)
        assert "cdna_label_stats" not in calls, calls
        assert_count(st, c["table"], c["bad"], 0)


BAD_CELLS = [float("nan"), float("inf"), -1.0, 2.5, float(KC)]


@pytest.mark.parametrize("d,n", [(5, 130), (100, N2)])
def test_count_bad_cells_and_labels(gpu_device, d, n):
    """One bad cell of each kind in features 1 and d - 2, two bad labels: ``bad`` and ``bad_label`` are exact, the
    other features' tables are those of the rows with a good label."""
    c = R.count_case(d, n, KC, CC)
    X, codes = c["X"].copy(), c["codes"].copy()
    rows = [0, 17, 63, 64, n - 1]
    for j in (1, d - 2):
        X[rows, j] = BAD_CELLS
    codes[[5, 100]] = [-1, CC]
    table, bad, bad_label = R.count_table(X, codes, KC, CC)
    assert bad[1] == bad[d - 2] == len(rows) and bad.sum() == 2 * len(rows) and bad_label == 2
    keep = np.ones(n, dtype=bool)
    keep[[5, 100]] = False
    clean = R.count_table(c["X"][keep], c["codes"][keep], KC, CC)[0]
    Xd, cd = torch.tensor(X, device=gpu_device), torch.tensor(codes, device=gpu_device)
    assert K.label_stats_plan(Xd, K.LABEL_COUNT, C=CC, K=KC)["path"] == "native"
    with Counting() as calls:
        st = count(Xd, cd)
    assert calls.count("cdna_label_stats") == 1, calls
    assert_count(st, table, bad, bad_label)
    others = [j for j in range(d) if j not in (1, d - 2)]
    assert np.array_equal(st["table"].cpu().numpy()[others], clean[others])


def test_count_every_row_in_one_cell(gpu_device):
    """Every row has the same label and category, 3072 rows per block: all of a column's increments hit one cell."""
    d, K_, C, rows = 4, 4096, 1, 3072
    probe = K.label_stats_plan(torch.zeros((4, d), device=gpu_device), K.LABEL_COUNT, C=C, K=K_)
    assert (probe["path"], probe["blocks_per_cu"]) == ("native", 1), probe
    n = 256 * rows
    Xd = torch.full((n, d), 5.0, device=gpu_device)
    cd = torch.zeros(n, dtype=torch.int32, device=gpu_device)
    plan = K.label_stats_plan(Xd, K.LABEL_COUNT, C=C, K=K_)
    assert (plan["path"], plan["vw"], plan["nblk"], plan["rows_per_block"]) == ("native", 4, 256, rows), plan
    with Counting() as calls:
        st = count(Xd, cd, C, K_)
    assert calls.count("cdna_label_stats") == 1, calls
    t = st["table"]
    assert t[:, 5, 0].tolist() == [n] * d and int(t.sum()) == n * d
    assert int(st["bad"].sum()) == 0 and int(st["bad_label"]) == 0


@pytest.mark.parametrize("C", [2, 32])
def test_class_counts_of_classes(gpu_device, C):
    d, n = 33, 600
    c = R.cont_case(d, n, C)
    Xd, cd = torch.tensor(c["X"], device=gpu_device), torch.tensor(c["codes"], device=gpu_device)
    assert K.label_stats_plan(Xd, K.LABEL_CLASS, C=C)["path"] == "native"
    with Counting() as calls:
        st = K.label_stats(Xd, cd, K.LABEL_CLASS, C=C, shift=c["shift"])
    assert calls.count("cdna_label_stats") == 1, calls
    R.check_class(f"class C={C}", dev_np(st), c["cls"], c["y_cls"])


def test_class_with_an_empty_class(gpu_device):
    d, n, C = 33, 600, 4
    c = R.cont_case(d, n, 3)
    codes = np.where(c["codes"] == 2, 3, c["codes"]).astype(np.int32)       # no row of class 2
    ref, yard = R.class_reference(c["X"], codes, C, c["shift"]), R.class_yardstick(c["X"], codes, C, c["shift"])
    Xd, cd = torch.tensor(c["X"], device=gpu_device), torch.tensor(codes, device=gpu_device)
    assert K.label_stats_plan(Xd, K.LABEL_CLASS, C=C)["path"] == "native"
    with Counting() as calls:
        st = K.label_stats(Xd, cd, K.LABEL_CLASS, C=C, shift=c["shift"])
    assert calls.count("cdna_label_stats") == 1, calls
    R.check_class("class, one empty", dev_np(st), ref, yard)
    assert float(st["n"][2]) == 0.0 and float(st["sums"][2].abs().max()) == 0.0


@pytest.mark.parametrize("d,n", [(5, 130), (100, N2)])
def test_class_and_regress_bad_cells_and_labels(gpu_device, d, n):
    """NaN, inf and -inf cells in features 1 and d - 2, bad labels in two rows: exact bad counts, and the sums are
    the reference's over what is left."""
    c = R.cont_case(d, n, CC)
    X, codes, y = c["X"].copy(), c["codes"].copy(), c["y"].copy()
    rows = [0, 63, n - 1]
    for j in (1, d - 2):
        X[rows, j] = [float("nan"), float("inf"), float("-inf")]
    codes[[5, 100]] = [-1, CC]
    y[[5, 100]] = [float("nan"), float("inf")]
    want_bad = np.zeros(d)
    want_bad[[1, d - 2]] = len(rows)
    Xd = torch.tensor(X, device=gpu_device)
    assert K.label_stats_plan(Xd, K.LABEL_CLASS, C=CC)["path"] == "native"
    assert K.label_stats_plan(Xd, K.LABEL_REGRESS)["path"] == "native"
    with Counting() as calls:
        a = K.label_stats(Xd, torch.tensor(codes, device=gpu_device), K.LABEL_CLASS, C=CC, shift=c["shift"])
        r = K.label_stats(Xd, torch.tensor(y, device=gpu_device), K.LABEL_REGRESS, shift=c["shift"],
                          yshift=c["yshift"])
    assert calls.count("cdna_label_stats") == 2, calls
    for st in (a, r):
        assert np.array_equal(st["bad"].cpu().numpy(), want_bad) and float(st["bad_label"]) == 2.0
    R.check_class(f"class, bad cells d={d}", dev_np(a), R.class_reference(X, codes, CC, c["shift"]),
                  R.class_yardstick(X, codes, CC, c["shift"]))
    R.check_regress(f"regress, bad cells d={d}", dev_np(r), R.regress_reference(X, y, c["shift"], c["yshift"]),
                    R.regress_yardstick(X, y, c["shift"], c["yshift"]))


def run_mode(mode, Xd, c, k, dev):
    """One call of ``mode`` on Xd with the labels of the count case ``k`` or the continuous case ``c``."""
    if mode == K.LABEL_COUNT:
        return count(Xd, torch.tensor(k["codes"], device=dev))
    if mode == K.LABEL_CLASS:
        return K.label_stats(Xd, torch.tensor(c["codes"], device=dev), mode, C=CC, shift=c["shift"])
    return K.label_stats(Xd, torch.tensor(c["y"], device=dev), mode, shift=c["shift"], yshift=c["yshift"])


def test_strided_misaligned_rows_take_the_scalar_loads(gpu_device):
    """X as a column slice of a wider tensor: odd row stride, pointer off 16-byte alignment, d a multiple of 4."""
    d, n = 100, N2
    c, k = R.cont_case(d, n, CC), R.count_case(d, n, KC, CC)
    for case, mode in ((k, K.LABEL_COUNT), (c, K.LABEL_CLASS), (c, K.LABEL_REGRESS)):
        wide = torch.full((n, 103), float("nan"), device=gpu_device)
        Xs = wide[:, 1:101]
        Xs.copy_(torch.tensor(case["X"]))
        assert Xs.stride(0) == 103 and Xs.data_ptr() % 16 != 0
        plan = K.label_stats_plan(Xs, mode, C=CC, K=KC)
        assert (plan["path"], plan["vw"], plan["nblk"]) == ("native", 1, 2), plan
        with Counting() as calls:
            st = run_mode(mode, Xs, c, k, gpu_device)
        assert calls.count("cdna_label_stats") == 1, calls
        if mode == K.LABEL_COUNT:
            assert_count(st, k["table"], k["bad"], 0)
        elif mode == K.LABEL_CLASS:
            R.check_class("class, strided", dev_np(st), c["cls"], c["y_cls"])
        else:
            R.check_regress("regress, strided", dev_np(st), c["reg"], c["y_reg"])


@pytest.mark.parametrize("d,n", [(5, 65), (100, N2)])
def test_rows_past_the_end_are_neither_read_nor_counted(gpu_device, d, n):
    """The first n rows of a buffer whose other rows are NaN give the bits of a tight buffer, in every mode."""
    c, k = R.cont_case(d, n, CC), R.count_case(d, n, KC, CC)
    for case, mode in ((k, K.LABEL_COUNT), (c, K.LABEL_CLASS), (c, K.LABEL_REGRESS)):
        Xd = torch.tensor(case["X"], device=gpu_device)
        big = torch.full((n + 200, d), float("nan"), device=gpu_device)
        big[:n] = Xd
        assert K.label_stats_plan(big[:n], mode, C=CC, K=KC)["path"] == "native"
        with Counting() as calls:
            a = run_mode(mode, Xd, c, k, gpu_device)
            b = run_mode(mode, big[:n], c, k, gpu_device)
        assert calls.count("cdna_label_stats") == 2, calls
        assert same_bits(a, b)
        assert float(b["bad"].sum()) == 0 and all(bool(torch.isfinite(v.double()).all()) for v in b.values())


@pytest.mark.parametrize("what", ["d", "C", "f64"])
def test_outside_the_native_range_takes_the_host_formulation(gpu_device, what):
    d, n, C = (K.LABEL_MAX_D + 1 if what == "d" else 20), 300, (K.LABEL_MAX_C + 1 if what == "C" else CC)
    c = R.cont_case(d, n, C)
    Xd = torch.tensor(c["X"], device=gpu_device)
    Xd = Xd.double() if what == "f64" else Xd
    assert K.label_stats_plan(Xd, K.LABEL_CLASS, C=C) == {"path": "host"}
    with Counting() as calls:
        st = K.label_stats(Xd, torch.tensor(c["codes"], device=gpu_device), K.LABEL_CLASS, C=C, shift=c["shift"])
    assert "cdna_label_stats" not in calls, calls
    R.check_class(f"host on the device, {what}", dev_np(st), c["cls"], c["y_cls"])


# ------------------------------------------------------------------------------------------------ end to end
def _fit(device, tmp_path, pdf, names, ftype, ltype, k):
    import cdnaml
    from cdnaml.ml.feature import UnivariateFeatureSelector, VectorAssembler
    with session_device(device):
        spark = cdnaml.SparkSession.builder.config("cdnaml.warehouse.dir", str(tmp_path / f"wh_{device}")) \
            .getOrCreate()
        spark.conf.set("cdnaml.ml.vectorPrecision", "fp32")
        try:
            with Counting() as calls:
                df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))
                sel = UnivariateFeatureSelector(outputCol="sel").setFeatureType(ftype).setLabelType(ltype) \
                    .setSelectionThreshold(k)
                m = sel.fit(df)
                width = len(m.transform(df).select("sel").head()[0])
        finally:
            spark.conf.set("cdnaml.ml.vectorPrecision", "auto")
            spark.stop()
    return m.selectedFeatures, width, calls


@pytest.mark.parametrize("ftype,ltype", [("categorical", "categorical"), ("continuous", "categorical"),
                                         ("continuous", "continuous")])
def test_selector_on_the_device_matches_the_cpu_session(gpu_device, tmp_path, ftype, ltype):
    n, d, k = 3000, 12, 4
    names = [f"x{i}" for i in range(d)]
    if ftype == "categorical":
        X, codes = R.make_counts(d, n, KC, CC)
        label = codes.astype(np.float64)
    else:
        X, codes, y = R.make_continuous(d, n, CC)
        label = codes.astype(np.float64) if ltype == "categorical" else y
    pdf = pd.DataFrame(X, columns=names)
    pdf["label"] = label
    got, width, calls = _fit("cuda", tmp_path, pdf, names, ftype, ltype, k)
    want, _, ccalls = _fit("cpu", tmp_path, pdf, names, ftype, ltype, k)
    print(f"selector {ftype} / {ltype}: {got} on the device, {want} on the CPU")
    assert calls.count("cdna_label_stats") == 1 and "cdna_label_stats" not in ccalls, calls
    assert got == want and len(got) == k == width
