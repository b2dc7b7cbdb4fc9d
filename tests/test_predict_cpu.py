"""The host twins of the forest predict kernels against the independent references of tests/_predict_refs.py.

K.tree_predict, K.heap_predict_host, K.tree_predict_heap_binned, K.predict_binned_add and K.heap_last_level on cpu
tensors must return the references bit for bit, on the cases the GPU suite (tests/test_predict_gpu.py) runs; the
references' ordered sums are checked against exact sums.  This pins the references before they judge a kernel."""
import numpy as np
import pytest
import torch

from tests import _predict_refs as R
from cdnaml.ops import kernels as K


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _masks(c):
    return _t(c.masks.view(np.int32).reshape(-1)) if len(c.masks) else torch.zeros(8, dtype=torch.int32)


def _node_predict(c, X, base):
    return K.tree_predict(X, _t(c.nodes), _t(c.roots), _t(c.tw), _t(c.values), _masks(c), c.K,
                          _t(c.base) if base else None)


# ============================================================================================ references
@pytest.mark.parametrize("T", R.NODE_T)
@pytest.mark.parametrize("K_", [1, 3])
def test_ordered_sum_within_bound_of_exact_sum(T, K_):
    """|ordered - exact| <= T 2^-53 sum |tw v|: the T products are added by T - 1 roundings, each at most 2^-53 of a
    partial sum that the magnitudes bound.  With the base one more term joins the sum and the magnitudes."""
    c = R.case(T, 3, 12, K=K_, n=200, cats=R.CATS)
    rows = range(c.n)
    exact, mag = R.exact_sum(c.tw, c.vals_k, c.leaf, None, rows)
    err = np.abs(c.ref_nobase - exact)
    print(f"T={T} K={K_}: max err / bound = {(err / (T * 2.0 ** -53 * mag)).max():.3f}")
    assert (err <= T * 2.0 ** -53 * mag).all()
    exact_b, mag_b = R.exact_sum(c.tw, c.vals_k, c.leaf, c.base, rows)
    assert (np.abs(c.ref - exact_b) <= (T + 1) * 2.0 ** -53 * mag_b).all()


@pytest.mark.parametrize("T", [33, 35, 37, 64])
def test_trees_past_the_first_round_change_every_row(T):
    """What the T > 32 cases can see: a sum that leaves out the trees of the second round (t >= 32), or adds tree
    T - 1 once for each tree index a pass clamps to it, differs from the reference in every row."""
    c = R.case(T, 3, 12, n=200, cats=R.CATS) if T != 35 else R.case(T, 3, 9, n=200, bup=40)
    first = R.ordered_sum(c.tw[:32], c.vals_k[:32], c.leaf[:, :32], c.base)
    assert (first != c.ref).all()
    pad = 8 * 4 * 2 - T      # tree indices past T in the second pass of NT = 8
    if pad:
        twx = np.concatenate([c.tw, np.repeat(c.tw[-1:], pad)])
        vx = np.concatenate([c.vals_k, np.repeat(c.vals_k[-1:], pad, 0)])
        lx = np.concatenate([c.leaf, np.repeat(c.leaf[:, -1:], pad, 1)], 1)
        assert (R.ordered_sum(twx, vx, lx, c.base) != c.ref).all()


def test_rows_hold_the_edges():
    """The rows of a case hold thresholds exactly, both fp32 neighbours, +-inf, NaN, +-0.0 against a 0.0 threshold, and
    in categorical columns non-integers, values outside [0, 256) and NaN; the masks have bit 0 set, clear, bit 255."""
    c = R.case(5, 3, 12, n=200, cats=R.CATS)
    thr0 = [c.struct[t, s:s + 1, 1].view(np.float32)[0] for t in range(c.T) for s in R.reachable(c.struct[t])[0]
            if c.struct[t, s, 0] >= 0]
    feats = [c.struct[t, s, 0] for t in range(c.T) for s in R.reachable(c.struct[t])[0] if c.struct[t, s, 0] >= 0]
    on = sum(int((c.X[:, f] == v).sum()) for f, v in zip(feats, thr0))
    up = sum(int((c.X[:, f] == np.nextafter(v, np.float32(np.inf))).sum()) for f, v in zip(feats, thr0))
    dn = sum(int((c.X[:, f] == np.nextafter(v, np.float32(-np.inf))).sum()) for f, v in zip(feats, thr0))
    assert on and up and dn
    num = [f for f in range(c.d) if f not in R.CATS]
    assert np.isnan(c.X[:, num]).any() and np.isposinf(c.X[:, num]).any() and np.isneginf(c.X[:, num]).any()
    x0 = c.X[:, 0]
    assert ((x0 == 0) & np.signbit(x0)).any() and ((x0 == 0) & ~np.signbit(x0)).any()
    xc = c.X[:, R.CATS[0]]
    for v in R.CAT_ODD:
        assert (np.isnan(xc).any() if v != v else (xc == np.float32(v)).any()), v
    assert c.nan_cat_hits > 0
    assert (c.masks[:, 0] & 1).any() and not (c.masks[:, 0] & 1).all() and (c.masks[:, 7] >> 31).any()


# ============================================================================================ K.tree_predict
@pytest.mark.parametrize("K_", [1, 3])
@pytest.mark.parametrize("d", sorted({d for _, d, _ in R.NODE_STAGING}))
def test_tree_predict_host(d, K_):
    for n in R.SMALL_N:
        c = R.case(5, 3, d, K=K_, n=n, cats=R.CATS)
        assert torch.equal(_node_predict(c, _t(c.X), True), _t(c.ref))
        assert torch.equal(_node_predict(c, _t(c.X), False), _t(c.ref_nobase))


@pytest.mark.parametrize("T", R.NODE_T)
def test_tree_predict_host_trees(T):
    c = R.case(T, 3, 12, n=200, cats=R.CATS)
    assert torch.equal(_node_predict(c, _t(c.X), True), _t(c.ref))


@pytest.mark.parametrize("T,K_", [(24, 3), (40, 1)])
def test_tree_predict_host_large_forests(T, K_):
    c = R.case(T, 6, 12, K=K_, n=200, cats=R.CATS, complete=True)
    assert c.nodes.shape[0] == T * 127
    assert torch.equal(_node_predict(c, _t(c.X), True), _t(c.ref))


# ============================================================================================ heap walk
def _heap(c):
    return _t(K.pack_heap(c.struct, c.vals, c.depth))


@pytest.mark.parametrize("T", R.HEAP_T)
def test_heap_predict_host_trees(T):
    c = R.case(T, 3, 12, n=200)
    got = K.heap_predict_host(_t(c.X), _heap(c), c.depth, _t(c.tw), float(c.base[0]))
    assert torch.equal(got, _t(c.ref[:, 0]))


@pytest.mark.parametrize("depth,T", R.HEAP_DEPTHS + R.HEAP_OVER)
def test_heap_predict_host_depths(depth, T):
    c = R.case(T, depth, 12, n=200)
    got = K.heap_predict_host(_t(c.X), _heap(c), c.depth, _t(c.tw), float(c.base[0]))
    assert torch.equal(got, _t(c.ref[:, 0]))


def test_heap_predict_host_refuses_categorical_slots():
    c = R.case(5, 3, 12, n=64, cats=R.CATS)
    with pytest.raises(ValueError):
        K.heap_predict_host(_t(c.X), _heap(c), c.depth, _t(c.tw), 0.0)


# ============================================================================================ heap walk on bins
def _binned_case_list():
    cases = [(T, 3, 9, 40) for T in R.BINNED_T_ONE_PASS + R.BINNED_T_TWO_PASS]
    cases += [(5, 3, d, 40) for d, _, _ in R.BINNED_D]
    cases += [(5, depth, 9, 40) for depth in R.BINNED_DEPTHS]
    cases += [(5, 3, 9, bup) for bup in R.BINNED_BUP]
    return sorted(set(cases))


@pytest.mark.parametrize("T,depth,d,bup", _binned_case_list())
def test_heap_binned_host(T, depth, d, bup):
    for n in (65, 200):
        c = R.case(T, depth, d, n=n, bup=bup)
        got = K.tree_predict_heap_binned(_t(c.bins), _t(c.thr_up), d, _heap(c), depth, _t(c.tw), float(c.base[0]))
        assert got.dtype == torch.float64 and tuple(got.shape) == (n, 1)
        assert torch.equal(got, _t(c.ref))
        # the project's own table of upper edges is the reference's
        assert np.array_equal(K.bin_upper_edges(c.thr, c.nthr, bup), c.thr_up)


def test_binned_tables_hold_the_edges():
    c = R.case(5, 3, 9, n=200, bup=40)
    assert c.nthr[1] == 0 and c.nthr[2] == 1 and c.nthr[4] == 39
    assert c.thr[3, 0] == c.thr[3, 1] and c.nthr[3] >= 3
    b = c.bins.transpose(1, 0, 2).reshape(c.n, -1)
    assert (b[:, 1] == 0).all() and not (b[:, 3] == 1).any()      # no thresholds: bin 0; the duplicate's bin is empty
    assert (b[np.isnan(c.X[:, 0]), 0] == c.nthr[0]).all()
    assert int(b[:, 4].max()) == 39


# ============================================================================================ K.predict_binned_add
def _binned_add(c, out):
    for nodes, root, values in c.tables:
        K.predict_binned_add(_t(c.bins), _t(nodes), root, _t(values), _t(c.masks.view(np.int32).reshape(-1)),
                             c.scale, out)
    return out


@pytest.mark.parametrize("n,G", R.BINNED_ADD)
def test_predict_binned_add_host(n, G):
    c = R.binned_add_case(n, G)
    out = _binned_add(c, _t(c.out0.copy()))
    assert torch.equal(out, _t((c.out0.astype(np.float64) + c.picked.sum(1)).astype(np.float32)))


def test_predict_binned_add_host_scaled():
    c = R.binned_add_case(257, 2, T=1, exact=False)
    err, bound = R.binned_add_bound(c, _binned_add(c, _t(c.out0.copy())).numpy())
    assert (err <= bound).all()


# ============================================================================================ K.heap_last_level
@pytest.mark.parametrize("D,A,sw", R.LAST_LEVEL)
def test_heap_last_level_host(D, A, sw):
    c = R.last_level_case(D, A, sw)
    heap = _t(c.heap.copy())
    K.heap_last_level(_t(c.so), _t(c.a_tree), _t(c.a_key), _t(c.a_w), _t(c.thr), c.min_gain, c.min_w, heap, D)
    assert not np.array_equal(c.want, c.heap)
    assert torch.equal(heap, _t(c.want))


# ============================================================================================ K.binize, categorical
def test_binize_host_categorical_edges():
    """bin = clamp(int(x), 0, 255): NaN -> 0, +inf and values past the integers -> 255, -inf and negatives -> 0."""
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), 1e20, 3e9, -3.0, -0.5, 255.9, 256.0, 300.0, 7.0, 3.7])
    X = torch.stack([x, torch.zeros_like(x)], 1)
    got = K.binize(X, torch.zeros(2, 1), torch.tensor([-1, 0], dtype=torch.int32))
    assert got[0, :, 0].tolist() == [0, 255, 0, 255, 255, 0, 0, 255, 255, 255, 7, 3]
