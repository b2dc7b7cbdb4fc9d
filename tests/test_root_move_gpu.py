"""The level-0 row partition inside the level-1 codes histogram (seg.hip RootMove, engine ROOT_MOVE): the fused
kernel against ``partition_codes`` + ``seg_hist_codes``, the op's refusals, and the forests it grows."""
import numpy as np
import pytest
import torch

from cdnaml.ops import _lib, kernels as K

pytestmark = pytest.mark.gpu

T, B = 7, 40


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()  # must load: no silent fallback on a GPU box
    return torch.device("cuda:0")


def _thresholds(X, maxb):
    d = X.shape[1]
    thr = torch.zeros(d, maxb - 1)
    nthr = torch.zeros(d, dtype=torch.int32)
    for f in range(d):
        q = torch.quantile(X[:2000, f], torch.linspace(0, 1, maxb + 1)[1:-1]).unique()
        thr[f, : len(q)] = q
        nthr[f] = len(q)
    return thr, nthr


def _level0_tables(d):
    """Level-0 decode tables of T = 7 roots (active node t = the root of tree t) and the local node each tree
    builds at level 1.  Trees 0-4 have two active children, tree 5 a leaf on the left, tree 6 a leaf on the right
    (the other child gets local node 0)."""
    sf = np.array([0, d - 1, 5, d - 1, 0, 17, 40], dtype=np.int32)
    sb = np.array([0, B - 2, 20, 0, B - 2, 19, 10], dtype=np.int32)
    built = np.array([0, 1, 0, 1, 1, 0, 0], dtype=np.int64)  # left, right, ... ; the only child of trees 5 and 6
    child = np.full(2 * T, -1, dtype=np.int32)
    tfn = np.zeros(T, dtype=np.int32)
    nxt = 0
    for t in range(T):
        tfn[t] = nxt
        for side in (0, 1):
            if (t, side) in ((5, 0), (6, 1)):
                continue
            child[2 * t + side] = nxt
            nxt += 1
    dec = {"split_feat": torch.from_numpy(sf), "split_bin": torch.from_numpy(sb),
           "cat_off": torch.full((T,), -1, dtype=torch.int32), "child": torch.from_numpy(child),
           "tfirst_next": torch.from_numpy(tfn)}
    # every case the kernel's move has to get right occurs in the tables
    assert 0 in sf and d - 1 in sf                      # first and last bins word (d = 100: word 12, d = 81: word 10)
    assert 0 in sb and B - 2 in sb
    two = (child[0::2] >= 0) & (child[1::2] >= 0)
    assert np.any(two & (built == 0)) and np.any(two & (built == 1))  # built child left / right
    assert np.sum(~two) == 2 and child[2 * 5] < 0 and child[2 * 6 + 1] < 0 and not np.any(built[~two])
    assert np.array_equal(child[child >= 0], np.arange(nxt))
    return dec, built


def _inputs(n, d, dev):
    """Level-0 state of T trees over n rows: codes weight << 8 | 0 (0xFF for weight 0), bins, labels."""
    rng = np.random.default_rng(1000 * d + n)
    w = rng.choice(4, size=(T, n), p=[1 / 3, 2 / 9, 2 / 9, 2 / 9])
    for t in range(T):
        assert set(np.unique(w[t])) == {0, 1, 2, 3}           # weights 0..3 in every tree
    assert 0.2 < np.mean(w == 0) < 0.45                       # ~1/3 of the codes are 0xFF and stay 0xFF
    codes = torch.from_numpy(((w << 8) | np.where(w == 0, 0xFF, 0)).astype(np.uint16).view(np.int16)).to(dev)
    g = torch.Generator().manual_seed(d + n)
    X = torch.randn(n, d, generator=g)
    thr, nthr = _thresholds(X, B)
    bins, s10 = K.binize(X.to(dev), thr.to(dev), nthr.to(dev), want_rm=True, rm_layout="s10")
    if s10 is None:  # rows the streaming binning kernel does not take (d = 81: unaligned): the layout in torch
        s10 = K.bins_seg10(bins, d)
    assert s10.shape == (n, 16, 8) and bins.shape == ((d + 7) // 8, n, 8)
    v1 = (torch.randn(n, generator=g) * 3).to(dev)
    return codes, bins, s10, v1, K.seg_scales(None, v1, 3, n)


@pytest.mark.parametrize("n", [37, 64, 100003])
@pytest.mark.parametrize("d", [100, 81])
def test_fused_move_equals_partition_then_histogram(dev, monkeypatch, d, n):
    """One seg_hist_codes(move=) call on the level-0 codes leaves exactly the codes of partition_codes
    (partition7) and the int64 histograms of seg_hist_codes on those moved codes: a partial window, exactly one
    window, several work items per tree with a ragged tail."""
    monkeypatch.setattr(K, "PARTITION7_MIN_T", 1)  # the pass the fused move replaces
    codes, bins, s10, v1, sc = _inputs(n, d, dev)
    dec, built = _level0_tables(d)
    zeros = lambda: torch.zeros((T, d, B, 2), dtype=torch.int64, device=dev)  # noqa: E731
    ref_codes = codes.clone()
    K.partition_codes(bins, ref_codes, torch.arange(T, dtype=torch.int32), dec["tfirst_next"], dec["split_feat"],
                      dec["split_bin"], dec["cat_off"], torch.zeros(0, dtype=torch.int32), dec["child"])
    ref = K.seg_hist_codes(s10, d, B, ref_codes, v1, sc[1], 3, np.arange(T), built, 0, T, zeros())
    got_codes = codes.clone()
    got = K.seg_hist_codes(s10, d, B, got_codes, v1, sc[1], 3, np.arange(T), built, 0, T, zeros(),
                           move=(dec, bins))
    rc = ref_codes.cpu().numpy().view(np.uint16)
    loc, w0 = rc & 0xFF, codes.cpu().numpy().view(np.uint16) >> 8
    assert np.array_equal(rc >> 8, w0) and np.all(loc[w0 == 0] == 0xFF)  # the reference itself: weights kept
    assert int(ref[..., 0].sum()) > 0
    if n > 1000:
        # both children of every root receive rows (a leaf child as 0xFF), so each compare direction is exercised
        for t in range(T):
            live = loc[t][w0[t] > 0]
            assert set(np.unique(live)) == ({0, 0xFF} if t >= 5 else {0, 1}), t
        assert np.all(ref[..., 0].sum((1, 2)).cpu().numpy() > 0)
    assert torch.equal(got_codes.cpu(), ref_codes.cpu())
    assert torch.equal(got.cpu(), ref.cpu())


def test_fused_move_refusals(dev):
    """move= needs one slot per tree over the whole slot range and numeric root splits."""
    n, d = 64, 100
    codes, bins, s10, v1, sc = _inputs(n, d, dev)
    dec, built = _level0_tables(d)
    out = lambda s: torch.zeros((s, d, B, 2), dtype=torch.int64, device=dev)  # noqa: E731
    before = codes.clone()
    with pytest.raises(AssertionError):  # a slot subrange
        K.seg_hist_codes(s10, d, B, codes, v1, sc[1], 3, np.arange(T), built, 1, T, out(T - 1), move=(dec, bins))
    with pytest.raises(AssertionError):  # S < T: tree T - 1 has no slot
        K.seg_hist_codes(s10, d, B, codes, v1, sc[1], 3, np.arange(T - 1), built[:T - 1], 0, T - 1, out(T - 1),
                         move=(dec, bins))
    cat = dict(dec, cat_off=dec["cat_off"].clone())
    cat["cat_off"][2] = 2
    with pytest.raises(AssertionError):  # a categorical root split
        K.seg_hist_codes(s10, d, B, codes, v1, sc[1], 3, np.arange(T), built, 0, T, out(T), move=(cat, bins))
    assert torch.equal(codes.cpu(), before.cpu())  # a refused call moves nothing


def _fit(df, **kw):
    from cdnaml.ml.regression import RandomForestRegressor
    from cdnaml.utils.synthetic import forest_digest
    m = RandomForestRegressor(numTrees=20, maxDepth=5, maxBins=40, seed=3, **kw).fit(df)
    pred = m.transform(df)._plan.execute()[0].columns["prediction"].values
    return m._forest, forest_digest(m._forest), pred.cpu()


def _spies(monkeypatch):
    calls = {"partition": 0, "move": 0}
    part, hist = K.partition_codes, K.seg_hist_codes

    def partition(*a, **k):
        calls["partition"] += 1
        return part(*a, **k)

    def codes_hist(*a, **k):
        calls["move"] += k.get("move") is not None
        return hist(*a, **k)
    monkeypatch.setattr(K, "partition_codes", partition)
    monkeypatch.setattr(K, "seg_hist_codes", codes_hist)
    return calls


def _features():
    g = torch.Generator().manual_seed(4)
    return torch.randn((300000, 100), generator=g)


def test_root_move_grows_the_same_forest(dev, monkeypatch):
    """RandomForestRegressor with the level-0 partition fused into the level-1 histogram: the same forest and
    predictions as with the partition pass, one partition_codes call fewer, one histogram call that moves."""
    import cdnaml
    from cdnaml.models.tree import engine as E
    spark = cdnaml.SparkSession.builder.getOrCreate()
    X = _features().to(dev)
    y = (X[:, 0] * 2 - X[:, 1] + torch.sin(3 * X[:, 2])).double()
    df = spark.createDataFrameFromLocalTensors({"features": X, "label": y})
    calls = _spies(monkeypatch)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(E, "ROOT_MOVE", on)
        calls.update(partition=0, move=0)
        _, dig, pred = _fit(df)
        res[on] = (dig, pred, dict(calls))
    assert res[True][0] == res[False][0] and torch.equal(res[True][1], res[False][1])
    assert res[False][2]["move"] == 0 and res[True][2]["move"] == 1
    assert res[True][2]["partition"] == res[False][2]["partition"] - 1


def test_root_move_falls_back_when_a_root_does_not_split(dev, monkeypatch):
    """A label that is constant but on two rows: a tree whose bootstrap draws weight 0 for both sees a constant
    label, its root does not split, and level 1 has fewer built nodes than trees -- the level-0 partition then
    runs late, from the kept decode tables, and the forest is the one the partition pass grows."""
    import cdnaml
    from cdnaml.models.tree import engine as E
    spark = cdnaml.SparkSession.builder.getOrCreate()
    X = _features()
    y = torch.zeros(X.shape[0], dtype=torch.float64)
    y[np.random.default_rng(11).choice(X.shape[0], 2, replace=False)] = 1.0
    df = spark.createDataFrameFromLocalTensors({"features": X.to(dev), "label": y.to(dev)})
    calls = _spies(monkeypatch)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(E, "ROOT_MOVE", on)
        calls.update(partition=0, move=0)
        forest, dig, pred = _fit(df, minInstancesPerNode=1)
        res[on] = (dig, pred, dict(calls))
        feat = np.asarray(forest.feat)
        roots = np.array([feat[r] for r in forest.roots])
        assert np.any(roots < 0) and np.any(roots >= 0), roots  # a root that did not split, and level 1 exists
    assert res[True][0] == res[False][0] and torch.equal(res[True][1], res[False][1])
    assert res[True][2]["move"] == 0 and res[False][2]["move"] == 0
    # the late partition replaces the queued one (and level 1 ran: it queued its own)
    assert res[True][2]["partition"] == res[False][2]["partition"] >= 2
