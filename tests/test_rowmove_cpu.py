"""The host paths of the row-movement operations (K.partition, K.partition_codes, K.seg_partition, K.codes_compact,
K.node_compact, K.decode_codes, K.codes_init_max, K.bins_row_major on CPU tensors) against the plain references of
tests/_rowmove_refs.py, on the small shapes of the cases tests/test_rowmove_gpu.py runs against the kernels.

The host paths and the references were written independently: this file is how the references are checked where
there is no GPU.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from tests import _rowmove_refs as R
from cdnaml.ops import kernels as K


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _codes_t(c):
    return _t(np.array(c, dtype=np.uint16).view(np.int16))  # a copy: partition_codes works in place


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _tab(tab):
    return [_t(x) for x in (tab.split_feat, tab.split_bin, tab.cat_off, tab.cat_mask, tab.child)]


def _partition_codes(bm, codes, tab):
    c = _codes_t(codes)
    K.partition_codes(_t(R.pack_bins(bm)), c, _t(tab.tfirst), _t(tab.tfirst_next), *_tab(tab))
    return _u16(c)


# ============================================================================================ the references
def test_go_left_reads_the_mask_words_unsigned():
    """Bit 31 of a word arrives as the sign of an int32: bins 31, 63, .., 255 of set 0 are in, bin 223 / 225 of set 1
    are out, 224 / 255 in."""
    tab = R.edge_table(np.random.default_rng(0), [9], 20)
    assert (tab.cat_mask[:8] < 0).all() and tab.cat_mask[15] < 0
    a0, a1 = np.full(8, 2), np.full(4, 3)
    assert tab.cat_off[2] == 0 and tab.cat_off[3] == 1
    assert R.go_left(np.arange(31, 256, 32), a0, tab).all()
    assert R.go_left(np.array([223, 224, 225, 255]), a1, tab).tolist() == [False, True, False, True]
    assert R.go_left(np.array([0, 1]), np.array([0, 0]), tab).tolist() == [True, False]       # ordered, bin 0
    assert R.go_left(np.array([254, 255]), np.array([1, 1]), tab).tolist() == [True, True]    # ordered, bin 255


def test_pack_bins_layout():
    bm = R.edge_bins(np.random.default_rng(1), 5, 19)
    b = R.pack_bins(bm)
    assert b.shape == (3, 5, 8) and b[2, 4, 2] == bm[4, 18] and b[0, 0, 7] == bm[0, 7] and not b[2, :, 3:].any()
    assert np.array_equal(K.bins_to_matrix(_t(b), 19).numpy(), bm)


# ================================================================================================ partition
@pytest.mark.parametrize("n", [1, 255, 257])
def test_partition_node_ids(n):
    rng = np.random.default_rng(10 + n)
    d, nloc = 20, [9, 5, 3]
    tab = R.edge_table(rng, nloc, d)
    bm = R.edge_bins(rng, n, d)
    node = (tab.tfirst[:, None] + (rng.random((3, n)) * np.array(nloc)[:, None]).astype(np.int32)).astype(np.int32)
    node[rng.random((3, n)) < 0.2] = -1
    got = _t(node.copy())
    K.partition(_t(R.pack_bins(bm)), got, *_tab(tab))
    assert np.array_equal(got.numpy(), R.ref_partition_nodes(bm, node, tab))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_partition_codes(n):
    rng = np.random.default_rng(20 + n)
    d, nloc = 20, [9, 12, 4]
    tab = R.edge_table(rng, nloc, d)
    bm = R.edge_bins(rng, n, d)
    codes = R.edge_codes(rng, nloc, n)
    assert np.array_equal(_partition_codes(bm, codes, tab), R.ref_partition_codes(bm, codes, tab.tfirst,
                                                                                 tab.tfirst_next, tab))


def test_partition_codes_255_local_nodes():
    """The table limit: 255 active nodes in one tree (local 254 in use), and 255 next-level nodes (child local 254)."""
    rng = np.random.default_rng(3)
    tab = R.edge_table(rng, [255, 3], 12, max_next=255)
    assert (tab.child[:510].max() - tab.tfirst_next[0]) == 254
    bm = R.edge_bins(rng, 3000, 12)
    codes = R.edge_codes(rng, [255, 3], 3000)
    codes[0, :255] = (codes[0, :255] & 0xFF00) | np.arange(255)  # every local node holds a row
    assert np.array_equal(_partition_codes(bm, codes, tab), R.ref_partition_codes(bm, codes, tab.tfirst,
                                                                                 tab.tfirst_next, tab))


def test_partition_codes_weight_byte_is_carried():
    """A live code with weight byte 0 moves like any other and keeps its weight byte; a done code keeps whatever
    weight byte it has.  (codes_init never writes a live weight-0 code; the kernels have always moved one.)"""
    rng = np.random.default_rng(4)
    nloc = [9, 6]
    tab = R.edge_table(rng, nloc, 20)
    bm = R.edge_bins(rng, 600, 20)
    codes = R.edge_codes(rng, nloc, 600, wzero=True)
    live0 = ((codes >> 8) == 0) & ((codes & 0xFF) != 0xFF)
    assert live0.sum() > 50
    got = _partition_codes(bm, codes, tab)
    assert np.array_equal(got, R.ref_partition_codes(bm, codes, tab.tfirst, tab.tfirst_next, tab))
    assert np.array_equal(got >> 8, codes >> 8)
    assert ((got[live0] & 0xFF) != 0xFF).sum() > 10  # some of them really moved to a child


def test_partition_codes_refuses_more_than_255_nodes():
    rng = np.random.default_rng(5)
    bm = R.edge_bins(rng, 10, 12)
    tab = R.edge_table(rng, [256], 12, max_next=10)
    with pytest.raises(ValueError, match="255"):
        _partition_codes(bm, R.edge_codes(rng, [3], 10), tab)
    tab = R.edge_table(rng, [200], 12, max_next=256)
    if tab.child.max() - tab.tfirst_next[0] >= 255:  # 256 children of one tree: local index 255 = the done byte
        with pytest.raises(ValueError, match="255"):
            _partition_codes(bm, R.edge_codes(rng, [3], 10), tab)
    else:  # pragma: no cover
        pytest.fail("the case must reach child local index 255")


# ========================================================================================== segment partition
def _assert_seg(got, ref, with_v0, with_w):
    np.testing.assert_array_equal(got[4], ref[4])
    assert np.array_equal(got[0].cpu().numpy().astype(np.int32), ref[0])  # the order, not only the content
    assert np.array_equal(got[2].cpu().numpy().view(np.int32), ref[2].view(np.int32))
    if with_v0:
        assert np.array_equal(got[1].cpu().numpy().view(np.int32), ref[1].view(np.int32))
    if with_w:
        assert np.array_equal(got[3].cpu().numpy(), ref[3])


@pytest.mark.parametrize("with_v0,with_w", [(False, False), (True, True)])
def test_seg_partition(with_v0, with_w):
    bm, perm, v0, v1, w, segs, tab, n_next = R.seg_case(np.random.default_rng(6), 20)
    v0, w = (v0 if with_v0 else None), (w if with_w else None)
    ref = R.ref_seg_partition(bm, perm, v0, v1, w, segs, tab, n_next)
    got = K.seg_partition(_t(R.pack_bins(bm)), _t(perm), None if v0 is None else _t(v0), _t(v1),
                          None if w is None else _t(w), segs, tab.split_feat, tab.split_bin, tab.cat_off,
                          tab.cat_mask, tab.child, n_next)
    _assert_seg(got, ref, with_v0, with_w)
    # the case is what it says: all left, all right, one-sided, dropped
    ln = ref[4][:, 1]
    c = tab.child
    assert ln[c[10]] == 8191 and ln[c[11]] == 0 and ln[c[12]] == 0 and ln[c[13]] == 8192
    assert c[14] == -1 and c[17] == -1 and c[18] == c[19] == -1 and 0 < ln[c[15]] < 8193 and 0 < ln[c[16]] < 16385


def test_seg_partition_implicit_level0():
    bm, v0, v1, w, segs, tab, n_next = R.seg_implicit_case(np.random.default_rng(7), 20)
    ref = R.ref_seg_partition(bm, None, v0, v1, w, segs, tab, n_next)
    got = K.seg_partition(_t(R.pack_bins(bm)), None, _t(v0), _t(v1), _t(w), segs, tab.split_feat, tab.split_bin,
                          tab.cat_off, tab.cat_mask, tab.child, n_next)
    _assert_seg(got, ref, True, True)
    assert ref[3].min() > 0 and ref[3].max() == 255 and ref[4][2, 1] == 0 and ref[4][3, 1] == 0  # tree 1: no rows


# ================================================================================================ compaction
@pytest.mark.parametrize("n", [1000, 1001])
@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16, 17])
def test_codes_compact(n, kb):
    rng = np.random.default_rng(30 + kb)
    codes, tfirst, bs, S = R.compact_case(rng, n, [kb, 0, max(kb // 2, 1)])
    v1 = R.rec_v1(rng, n)
    rows, w, segs = R.ref_compact(tfirst, bs, S, codes=codes)
    got = K.codes_compact(_codes_t(codes), _t(tfirst), bs, S, None, _t(v1))
    np.testing.assert_array_equal(got[4], segs)
    assert np.array_equal(got[0].numpy(), rows) and np.array_equal(got[3].numpy(), w)
    assert np.array_equal(got[2].numpy().view(np.int32), v1[rows].view(np.int32))
    rec = K.codes_compact(_codes_t(codes), _t(tfirst), bs, S, None, _t(v1), rec_scale=R.REC_SCALE)
    np.testing.assert_array_equal(rec[4], segs)
    assert np.array_equal(rec[0].numpy(), R.ref_records(rows, w, v1, R.REC_SCALE))


def test_codes_compact_no_slots_and_limit():
    rng = np.random.default_rng(8)
    codes, tfirst, bs, S = R.compact_case(rng, 100, [0, 0])
    got = K.codes_compact(_codes_t(codes), _t(tfirst), bs, 0, None, _t(R.rec_v1(rng, 100)))
    assert got[0].numel() == 0 and got[4].shape == (0, 2)
    with pytest.raises(ValueError, match="255"):
        K.codes_compact(_codes_t(codes), _t(np.array([0, 256], np.int32)), np.full(300, -1, np.int32), 0, None,
                        _t(R.rec_v1(rng, 100)))


def test_record_quantisation_edges():
    """clamp(rint(v1 * scale)) at +-2^23, past it, at the ties and at -0.0, as the reference states it."""
    q = (R.ref_records(np.arange(16), np.ones(16, np.int64), R.REC_EDGE_V1, R.REC_SCALE).view(np.uint64)
         >> np.uint64(39)).astype(np.int64) - (1 << 23)
    assert q.tolist() == [1 << 23, -(1 << 23), 1 << 23, -(1 << 23), 1 << 23, -(1 << 23), 0, 2, 2, 0, -2, -2,
                          4194304, -4194304, 0, 0]
    r, w, qq = K.rec_decode(_t(R.ref_records(np.arange(16), np.full(16, 255), R.REC_EDGE_V1, R.REC_SCALE)))
    assert r.tolist() == list(range(16)) and set(w.tolist()) == {255} and qq.tolist() == q.tolist()


@pytest.mark.parametrize("n", [1, 255, 2049])
@pytest.mark.parametrize("nloc", [[1, 256], [257, 1024, 3]], ids=["1-256", "257-1024-3"])
def test_node_compact(n, nloc):
    rng = np.random.default_rng(40 + n)
    node, w, tfirst, bs, S = R.node_case(rng, n, nloc)
    v1 = R.rec_v1(rng, n)
    rows, wts, segs = R.ref_compact(tfirst, bs, S, node=node, w=w)
    rec, sg = K.node_compact(_t(node), _t(w), tfirst, bs, S, _t(v1), R.REC_SCALE)
    np.testing.assert_array_equal(sg, segs)
    ref = R.ref_records(rows, wts, v1, R.REC_SCALE)
    assert np.array_equal(R.sort_segments(rec.numpy(), segs), R.sort_segments(ref, segs))


def test_node_compact_refuses_more_than_1024_nodes():
    rng = np.random.default_rng(9)
    node, w, tfirst, bs, S = R.node_case(rng, 10, [1025, 2])
    with pytest.raises(ValueError, match="1024"):
        K.node_compact(_t(node), _t(w), tfirst, bs, S, _t(R.rec_v1(rng, 10)), R.REC_SCALE)


def test_wave_scan_reference():
    off, tot = R.ref_wave_scan(np.array([[[1, 2], [3, 4], [5, 6]]]))
    assert off.tolist() == [[[0, 0], [1, 2], [4, 6]]] and tot.tolist() == [[9, 12]]


# ======================================================================================== layout changes
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_decode_codes_and_codes_init(n, T):
    rng = np.random.default_rng(50 + n + T)
    nloc = [7] * T
    codes = R.edge_codes(rng, nloc, n, wzero=True)
    tfirst = np.arange(T, dtype=np.int32) * 7
    ids, w = K.decode_codes(_codes_t(codes), _t(tfirst))
    rid, rw = R.ref_decode_codes(codes, tfirst)
    assert np.array_equal(ids.numpy(), rid) and np.array_equal(w.numpy(), rw)
    wts = rng.integers(0, 3, (T, n)).astype(np.uint8)
    wts[T - 1, n - 1] = 255  # the maximum sits in the last element
    c, wmax = K.codes_init_max(_t(wts), T, n, "cpu")
    rc, rmax = R.ref_codes_init(wts)
    assert np.array_equal(_u16(c), rc) and wmax == rmax == 255
    c, wmax = K.codes_init_max(_t(np.zeros((T, n), np.uint8)), T, n, "cpu")
    assert (_u16(c) == 0xFF).all() and wmax == 1
    c, wmax = K.codes_init_max(None, T, n, "cpu")
    assert (_u16(c) == 0x100).all() and wmax == 1


@pytest.mark.parametrize("G", [1, 13, 16, 17])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_bins_row_major(n, G):
    bins = R.pack_bins(R.edge_bins(np.random.default_rng(60 + G), n, G * 8 - 3))
    assert np.array_equal(K.bins_row_major(_t(bins)).numpy(), R.ref_bins_row_major(bins))
