"""The forest predict kernels of csrc/kernels/trees.hip on the GPU against the independent references of
tests/_predict_refs.py (pinned on the host by tests/test_predict_cpu.py).

Every case first asserts the path it reaches from the launchers' own host functions (K.tree_predict_plan,
K.tree_predict_heap_plan, K.tree_predict_heap_binned_plan), so a shape that stops reaching its staging mode, forest
placement or template instantiation fails instead of passing on another path; then the result must equal the
reference bit for bit."""
import numpy as np
import pytest
import torch

from tests import _predict_refs as R
from cdnaml.models.tree.forest import Forest
from cdnaml.ops import _lib, kernels as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()  # must load: no silent fallback on a GPU box
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _offset_copy(t, dev):
    """A device copy of ``t`` that starts one float into its storage (4 bytes past a 16-byte boundary)."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)[1:].view(t.shape)
    buf.copy_(t)
    assert buf.data_ptr() % 16 != 0 and buf.is_contiguous()
    return buf


def _rows(c, name, dev):
    """The case's rows on the device as the staging case ``name`` wants them."""
    X = torch.from_numpy(c.X)
    if name == "view":
        big = torch.full((c.n, 20), 7.0)
        big[:, 3:15] = X
        Xd = big.to(dev)[:, 3:15]
        assert Xd.stride(0) == 20 and Xd.stride(1) == 1
        return Xd
    if name == "offset":
        return _offset_copy(X, dev)
    Xd = X.to(dev)
    assert Xd.data_ptr() % 16 == 0
    return Xd


def _masks(c, dev):
    return _t(c.masks.view(np.int32).reshape(-1), dev) if len(c.masks) else torch.zeros(8, dtype=torch.int32,
                                                                                        device=dev)


def _node_plan(c, Xd):
    return K.tree_predict_plan(Xd, c.nodes.shape[0], c.T, c.K, c.values.size)


def _node_predict(c, Xd, dev, base=True):
    return K.tree_predict(Xd, _t(c.nodes, dev), _t(c.roots, dev), _t(c.tw, dev), _t(c.values, dev), _masks(c, dev),
                          c.K, _t(c.base, dev) if base else None)


def _node_lds(c, n_nodes, n_vals):
    """cdna_tree_predict's LDS bytes: the tile [64][d + 1] fp32, the partials [4][64][K] fp64, the forest copy."""
    vb = (((n_vals + 1) & ~1) + ((c.T + 1) & ~1)) * 8 + ((c.T + 3) & ~3) * 4 if n_vals else 0
    return 64 * (c.d + 1) * 4 + 4 * 64 * c.K * 8 + n_nodes * 16 + vb


def _assert_small_forest(c, plan):
    """Nodes and leaf values both in LDS."""
    assert plan["n_nodes_lds"] == c.nodes.shape[0] and plan["n_vals_lds"] == c.values.size, plan
    assert plan["lds_bytes"] == _node_lds(c, c.nodes.shape[0], c.values.size) <= 64 * 1024


# ============================================================================================ predict_kernel
@pytest.mark.parametrize("K_", [1, 3])
@pytest.mark.parametrize("name,d,staging", R.NODE_STAGING)
def test_tree_predict_staging(dev, name, d, staging, K_):
    for n in R.SMALL_N:
        c = R.case(5, 3, d, K=K_, n=n, cats=R.CATS)
        Xd = _rows(c, name, dev)
        plan = _node_plan(c, Xd)
        assert plan["staging"] == staging and plan["grid"] == -(-n // 64), plan
        _assert_small_forest(c, plan)
        assert torch.equal(_node_predict(c, Xd, dev).cpu(), torch.from_numpy(c.ref)), n
        assert torch.equal(_node_predict(c, Xd, dev, base=False).cpu(), torch.from_numpy(c.ref_nobase)), n


@pytest.mark.parametrize("T", R.NODE_T)
def test_tree_predict_trees(dev, T):
    """Tree lanes without a tree (T < 4), one tree per lane, and T > 32: the second round of 4 x 8 trees."""
    for n in (65, 200):
        c = R.case(T, 3, 12, n=n, cats=R.CATS)
        Xd = _rows(c, "d12", dev)
        plan = _node_plan(c, Xd)
        assert plan["staging"] == "float4+prefetch"
        _assert_small_forest(c, plan)
        assert torch.equal(_node_predict(c, Xd, dev).cpu(), torch.from_numpy(c.ref))


def test_tree_predict_nan_category_goes_right(dev):
    """Rows with a NaN in a categorical feature meet masks whose bit 0 is set (the reference counts the visits) and go
    right.  (int)NaN is 0 on the device: a kernel that tests the converted integer sends them left with category 0."""
    c = R.case(5, 3, 12, n=200, cats=R.CATS)
    assert c.nan_cat_hits > 0
    assert torch.equal(_node_predict(c, _rows(c, "d12", dev), dev).cpu(), torch.from_numpy(c.ref))


def test_tree_predict_values_in_global_memory(dev):
    """T = 24, depth 6, K = 3, d = 12: the 3048 nodes (48768 B) fit the 56064 B beside the tile and the partials, the
    36864 B of leaf values with them do not."""
    c = R.case(24, 6, 12, K=3, n=200, cats=R.CATS, complete=True)
    Xd = _rows(c, "d12", dev)
    plan = _node_plan(c, Xd)
    assert c.nodes.shape[0] == 3048 and c.values.size == 24 * 64 * 3
    assert plan["n_nodes_lds"] == 3048 and plan["n_vals_lds"] == 0 and plan["staging"] == "float4+prefetch", plan
    assert plan["lds_bytes"] == _node_lds(c, 3048, 0) == 9472 + 48768
    assert torch.equal(_node_predict(c, Xd, dev).cpu(), torch.from_numpy(c.ref))


def test_tree_predict_forest_in_global_memory(dev):
    """T = 40, depth 6, K = 1, d = 12: 5080 nodes, 3760 fit: the walk reads nodes and values from global memory."""
    c = R.case(40, 6, 12, K=1, n=200, cats=R.CATS, complete=True)
    Xd = _rows(c, "d12", dev)
    plan = _node_plan(c, Xd)
    assert c.nodes.shape[0] == 5080
    assert plan["n_nodes_lds"] == 0 and plan["n_vals_lds"] == 0 and plan["lds_bytes"] == _node_lds(c, 0, 0), plan
    assert torch.equal(_node_predict(c, Xd, dev).cpu(), torch.from_numpy(c.ref))


def test_tree_predict_second_trip(dev):
    """n = 8192 * 64 + 65: the grid is capped at 8192 blocks, block 0 and block 1 walk a second tile from the prefetch
    registers, the last tile has one row."""
    c = R.case(5, 3, 12, n=R.BIG_N, cats=R.CATS)
    Xd = _rows(c, "d12", dev)
    plan = _node_plan(c, Xd)
    assert plan["grid"] == 8192 < -(-c.n // 64) and plan["staging"] == "float4+prefetch", plan
    assert torch.equal(_node_predict(c, Xd, dev).cpu(), torch.from_numpy(c.ref))


# ============================================================================================ predict_heap_kernel
def _heap(c, dev):
    return _t(K.pack_heap(c.struct, c.vals, c.depth), dev)


def _heap_lds(c):
    """cdna_tree_predict_heap's LDS bytes: heap, tree weights, the tile [64][d + 1] fp32, the partials [4][64] fp64."""
    return c.T * ((4 << c.depth) - 2) * 4 + ((c.T + 1) & ~1) * 8 + 64 * (c.d + 1) * 4 + 2048


def _heap_check(c, Xd, dev, staging):
    """Plan, then both stores of K.tree_predict_heap against the reference."""
    plan = K.tree_predict_heap_plan(Xd, c.depth, c.T)
    assert plan["fits"] and plan["staging"] == staging and plan["lds_bytes"] == _heap_lds(c), plan
    assert plan["grid"] == min(-(-c.n // 64), 8192)
    heap, tw, mk = _heap(c, dev), _t(c.tw, dev), _masks(c, dev)
    got = K.tree_predict_heap(Xd, heap, c.depth, tw, mk, float(c.base[0]))
    assert got.dtype == torch.float64 and torch.equal(got.cpu(), torch.from_numpy(c.ref))
    got32 = K.tree_predict_heap(Xd, heap, c.depth, tw, mk, float(c.base[0]), dtype=torch.float32)
    assert got32.dtype == torch.float32 and torch.equal(got32.cpu(), torch.from_numpy(c.ref.astype(np.float32)))
    return plan


@pytest.mark.parametrize("name,d,staging", R.HEAP_STAGING)
def test_heap_staging(dev, name, d, staging):
    for n in R.SMALL_N:
        c = R.case(5, 3, d, n=n, cats=R.CATS)
        _heap_check(c, _rows(c, name, dev), dev, staging)


@pytest.mark.parametrize("T", R.HEAP_T)
def test_heap_trees(dev, T):
    for n in (65, 200):
        c = R.case(T, 3, 12, n=n, cats=R.CATS)
        _heap_check(c, _rows(c, "d12", dev), dev, "float4+prefetch")


def test_heap_nan_category_goes_right(dev):
    """As test_tree_predict_nan_category_goes_right, for the heap walk."""
    c = R.case(5, 3, 12, n=200, cats=R.CATS)
    assert c.nan_cat_hits > 0
    _heap_check(c, _rows(c, "d12", dev), dev, "float4+prefetch")


@pytest.mark.parametrize("depth,T", R.HEAP_DEPTHS)
def test_heap_depths(dev, depth, T):
    """Depth 1, depth 8, and depth 11 with one tree: 32760 + 16 + 3328 + 2048 B, the deepest heap that fits."""
    c = R.case(T, depth, 12, n=200)
    plan = _heap_check(c, _rows(c, "d12", dev), dev, "float4+prefetch")
    if depth == 11:
        assert plan["lds_bytes"] == 32760 + 16 + 3328 + 2048


def _forest_of(c):
    """The case's numeric trees as a Forest (its node lists)."""
    forest = Forest(1)

    def add(t, s, depth):
        code, pay = c.struct[t, s]
        i = forest.add([c.vals[t, s]], 1.0, depth)
        if code != -1:
            li, ri = add(t, 2 * s + 1, depth + 1), add(t, 2 * s + 2, depth + 1)
            forest.feat[i], forest.left[i], forest.right[i] = int(code), li, ri
            forest.thr[i] = float(c.struct[t, s:s + 1, 1].view(np.float32)[0])
        return i
    for t in range(c.T):
        forest.roots.append(add(t, 0, 0))
    return forest


@pytest.mark.parametrize("depth,T", R.HEAP_OVER)
def test_heap_over_the_lds_budget(dev, depth, T):
    """Two depth-11 trees (65520 B of heap) and any depth-12 tree (65528 B of heap alone: depth 12 never fits 64 KB)
    are over the budget: K.tree_predict_heap returns None, and Forest.predict gives the reference through the node
    kernel."""
    c = R.case(T, depth, 12, n=200)
    Xd = _rows(c, "d12", dev)
    plan = K.tree_predict_heap_plan(Xd, depth, T)
    assert not plan["fits"] and plan["lds_bytes"] == _heap_lds(c) > 64 * 1024 and plan["grid_resident"] == 0, plan
    assert K.tree_predict_heap(Xd, _heap(c, dev), depth, _t(c.tw, dev), _masks(c, dev), float(c.base[0])) is None
    got = _forest_of(c).predict(Xd, c.tw, c.base)
    assert torch.equal(got.cpu(), torch.from_numpy(c.ref))


def test_heap_resident_grid_second_trip(dev, monkeypatch):
    """n = 8192 * 64 + 65: with PREDICT_RESIDENT the grid is exactly the resident blocks (grid_mode 1) and every
    block walks many tiles; without it 8192 blocks, of which two walk a second tile.  Both equal the reference."""
    c = R.case(5, 3, 12, n=R.BIG_N, cats=R.CATS)
    Xd = _rows(c, "d12", dev)
    plan = K.tree_predict_heap_plan(Xd, c.depth, c.T)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert plan["fits"] and plan["grid"] == 8192 and plan["staging"] == "float4+prefetch", plan
    assert 0 < plan["grid_resident"] < 8192 and plan["grid_resident"] % cus == 0, plan
    heap, tw, mk = _heap(c, dev), _t(c.tw, dev), _masks(c, dev)
    plain = K.tree_predict_heap(Xd, heap, c.depth, tw, mk, float(c.base[0]))
    monkeypatch.setattr(K, "PREDICT_RESIDENT", True)
    resident = K.tree_predict_heap(Xd, heap, c.depth, tw, mk, float(c.base[0]))
    assert torch.equal(resident, plain)
    assert torch.equal(plain.cpu(), torch.from_numpy(c.ref))


# ===================================================================================== predict_heap_binned_kernel
def _binned_check(c, dev, nt, passes, prefetch, raw=True):
    plan = K.tree_predict_heap_binned_plan(c.n, c.G, c.d, c.depth, c.T)
    assert plan["fits"] and (plan["nt"], plan["passes"], plan["prefetch"]) == (nt, passes, prefetch), plan
    assert plan["grid"] == min(-(-c.n // 64), 8192)
    heap, tw = _heap(c, dev), _t(c.tw, dev)
    bins, up = _t(c.bins, dev), _t(c.thr_up, dev)
    got = K.tree_predict_heap_binned(bins, up, c.d, heap, c.depth, tw, float(c.base[0]))
    assert got.dtype == torch.float64 and torch.equal(got.cpu(), torch.from_numpy(c.ref))
    got32 = K.tree_predict_heap_binned(bins, up, c.d, heap, c.depth, tw, float(c.base[0]), dtype=torch.float32)
    assert torch.equal(got32.cpu(), torch.from_numpy(c.ref.astype(np.float32)))
    if raw:      # the fp32 kernel on the raw rows
        assert torch.equal(got, K.tree_predict_heap(_t(c.X, dev), heap, c.depth, tw, _masks(c, dev),
                                                    float(c.base[0])))


@pytest.mark.parametrize("T", R.BINNED_T_ONE_PASS)
def test_heap_binned_instantiations(dev, T):
    """NT = ceil(T / 4) = 1 .. 8 trees per wave in one pass."""
    for n in (65, 200):
        _binned_check(R.case(T, 3, 9, n=n, bup=40), dev, -(-T // 4), 1, True)


@pytest.mark.parametrize("T", R.BINNED_T_TWO_PASS)
def test_heap_binned_two_passes(dev, T):
    """T > 32: NT = 8 and a second pass, in which the tree indices past T walk tree T - 1 and must not be summed."""
    for n in (65, 200):
        _binned_check(R.case(T, 3, 9, n=n, bup=40), dev, 8, 2, True)


@pytest.mark.parametrize("d,G,prefetch", R.BINNED_D)
def test_heap_binned_word_groups(dev, d, G, prefetch):
    """G = 1, 2, 16 (64 G words = 4 per thread, the prefetch's limit) and 17 (staged without the prefetch)."""
    for n in R.SMALL_N:
        c = R.case(5, 3, d, n=n, bup=40)
        assert c.G == G
        _binned_check(c, dev, 2, 1, prefetch)


@pytest.mark.parametrize("depth", R.BINNED_DEPTHS)
def test_heap_binned_depths(dev, depth):
    _binned_check(R.case(5, depth, 9, n=200, bup=40), dev, 2, 1, True)


@pytest.mark.parametrize("bup", R.BINNED_BUP)
def test_heap_binned_table_widths(dev, bup):
    """Bup = 2 (one threshold at most), 40, 256 (a feature with 255 thresholds: bins up to 255)."""
    c = R.case(5, 3, 9, n=200, bup=bup)
    assert int(c.nthr.max()) == bup - 1
    _binned_check(c, dev, 2, 1, True)


def test_heap_binned_second_trip(dev):
    c = R.case(5, 3, 9, n=R.BIG_N, bup=40)
    assert c.G == 2
    _binned_check(c, dev, 2, 1, True)


# ============================================================================================ predict_binned_kernel
def _binned_add(c, dev):
    out = _t(c.out0.copy(), dev)
    bins, mk = _t(c.bins, dev), _t(c.masks.view(np.int32).reshape(-1), dev)
    for nodes, root, values in c.tables:
        K.predict_binned_add(bins, _t(nodes, dev), root, _t(values, dev), mk, c.scale, out)
    return out.cpu()


@pytest.mark.parametrize("n,G", R.BINNED_ADD + ((R.BIG_N_BINNED_ADD, 1),))
def test_predict_binned_add(dev, n, G):
    """Distinct small integer leaf values on integer margins with scale 1: the fp32 result is exact, a wrong leaf
    cannot hide.  n = 4096 * 256 + 257 (8 MB of bins) makes the first 257 threads walk a second row."""
    c = R.binned_add_case(n, G)
    want = (c.out0.astype(np.float64) + c.picked.sum(1)).astype(np.float32)
    assert torch.equal(_binned_add(c, dev), torch.from_numpy(want))


def test_predict_binned_add_scaled(dev):
    """Random fp32 leaf values and scale fp32(0.3): the device may fuse out + scale v."""
    c = R.binned_add_case(257, 2, T=1, exact=False)
    err, bound = R.binned_add_bound(c, _binned_add(c, dev).numpy())
    print(f"max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


# ============================================================================================ heap_last_level_kernel
@pytest.mark.parametrize("D,A,sw", R.LAST_LEVEL)
def test_heap_last_level(dev, D, A, sw):
    """Every word of the heap: the slots and leaves of the nodes that pass the split rule, the pattern elsewhere."""
    c = R.last_level_case(D, A, sw)
    heap = _t(c.heap.copy(), dev)
    K.heap_last_level(_t(c.so, dev), _t(c.a_tree, dev), _t(c.a_key, dev), _t(c.a_w, dev), _t(c.thr, dev),
                      c.min_gain, c.min_w, heap, D)
    assert torch.equal(heap.cpu(), torch.from_numpy(c.want))
