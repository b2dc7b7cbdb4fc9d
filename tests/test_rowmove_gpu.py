"""The row partition and compaction kernels (hist5.hip partition5 / partition7, trees.hip partition, seg.hip
seg_count / seg_scatter, codes_compact, node_compact, codes_count_w -> wave_scan -> codes_scatter_w / codes_scatter_q,
codes_to_nodes, bins_row_major; misc.hip codes_init) on the GPU against the plain references of
tests/_rowmove_refs.py, which tests/test_rowmove_cpu.py pins on the host.

Every comparison is exact.  codes_compact_kernel and node_compact_kernel leave the order inside a segment
unspecified: their records are compared sorted per segment, and the segment table exactly.  Every other path is
stable and compared as it is.  Each case is the smallest shape that reaches the path its docstring names, with the
arithmetic; profiles/r20/rowmove_tests.md collects them."""
import numpy as np
import pytest
import torch

from tests import _rowmove_refs as R
from cdnaml.ops import _lib, kernels as K
from cdnaml.ops._base import _ptr, _stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch.device("cuda:0")


def _t(a, dev="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _codes_t(c, dev):
    return _t(np.array(c, dtype=np.uint16).view(np.int16), dev)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x).view(np.int32)


def _spy(monkeypatch, obj, name):
    """Record the calls of obj.name (and pass them on)."""
    real, calls = getattr(obj, name), []

    def f(*a, **k):
        calls.append(a)
        return real(*a, **k)
    monkeypatch.setattr(obj, name, f)
    return calls


def _partition_codes(dev, bm, codes, tab, G=None, margin=None, fm=False):
    bins = R.pack_bins(bm)
    G = bins.shape[0] if G is None else G
    assert bins.shape[0] == G
    c = _codes_t(codes, dev)
    m = None if margin is None else (_t(margin[0], dev), _t(margin[1], dev), margin[2])
    K.partition_codes(_t(bins, dev), c, _t(tab.tfirst), _t(tab.tfirst_next), _t(tab.split_feat), _t(tab.split_bin),
                      _t(tab.cat_off), _t(tab.cat_mask), _t(tab.child), margin=m,
                      bins_fm=_t(R.feature_major(bm, G), dev) if fm else None)
    return (_u16(c), m[0].cpu().numpy()) if m is not None else _u16(c)


def _ref_codes(bm, codes, tab, margin=None):
    return R.ref_partition_codes(bm, codes, tab.tfirst, tab.tfirst_next, tab, margin)


def _p5(monkeypatch):
    monkeypatch.setattr(K, "PARTITION7", False)
    return _spy(monkeypatch, _lib.lib(), "cdna_partition5")


def _p7(monkeypatch):
    monkeypatch.setattr(K, "PARTITION7", True)
    monkeypatch.setattr(K, "PARTITION7_MIN_T", 1)
    return _spy(monkeypatch, _lib.lib(), "cdna_partition7"), _spy(monkeypatch, _lib.lib(), "cdna_partition5")


# ============================================================================================= partition5
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 20001, 20002, 20003])
def test_partition5_tail_and_unaligned(dev, monkeypatch, n):
    """T = 3 trees over the shared split table.  n % 4 != 0 runs the tail loop of tree 0 (rows 4 (n / 4) ..); tree t
    starts t * n codes in, so for n odd (or n = 20002, t = 1: byte offset 40004) its codes are not 8-byte aligned
    and it takes the one-row loop.  The weight-0 codes move like the others."""
    calls = _p5(monkeypatch)
    rng = np.random.default_rng(100 + n)
    nloc = [9, 12, 4]
    tab = R.edge_table(rng, nloc, 20)
    bm = R.edge_bins(rng, n, 20)
    codes = R.edge_codes(rng, nloc, n, wzero=True)
    assert np.array_equal(_partition_codes(dev, bm, codes, tab), _ref_codes(bm, codes, tab))
    assert len(calls) == 1


def test_partition5_255_local_nodes(dev, monkeypatch):
    """One tree with 255 active nodes (the 256-entry table's last live index 254) and 255 children (local 254)."""
    _p5(monkeypatch)
    rng = np.random.default_rng(3)
    tab = R.edge_table(rng, [255, 3], 12, max_next=255)
    assert tab.child[:510].max() - tab.tfirst_next[0] == 254
    bm = R.edge_bins(rng, 3001, 12)
    codes = R.edge_codes(rng, [255, 3], 3001)
    codes[0, :255] = (codes[0, :255] & 0xFF00) | np.arange(255)
    assert np.array_equal(_partition_codes(dev, bm, codes, tab), _ref_codes(bm, codes, tab))


def test_partition_codes_refuses_256_local_nodes(dev, monkeypatch):
    _p5(monkeypatch)
    rng = np.random.default_rng(5)
    tab = R.edge_table(rng, [256], 12, max_next=10)
    with pytest.raises(ValueError, match="255"):
        _partition_codes(dev, R.edge_bins(rng, 10, 12), R.edge_codes(rng, [3], 10), tab)


@pytest.mark.parametrize("fm", [False, True], ids=["words", "feature_major"])
def test_partition5_feature_major_and_margin(dev, monkeypatch, fm):
    """The [G * 8][n] byte copy against the [G][n] words, without and with the boosting margin update (T = 1).
    eta = 3 / 16, lv = k / 64, F = k / 256: every product and sum is exact in fp32, so F is compared bit for bit.
    Some rows finish under a splitting node (child -1: lv[2 a + side]), some in a node that does not split
    (lv[2 A + a])."""
    _p5(monkeypatch)
    rng = np.random.default_rng(7)
    n, nloc = 20003, [12, 9, 4]
    tab = R.edge_table(rng, nloc, 20)
    bm = R.edge_bins(rng, n, 20)
    codes = R.edge_codes(rng, nloc, n)
    assert np.array_equal(_partition_codes(dev, bm, codes, tab, fm=fm), _ref_codes(bm, codes, tab))
    tab1 = R.edge_table(rng, [12], 20)
    c1 = R.edge_codes(rng, [12], n)
    A = 12
    F = (rng.integers(-512, 513, n) / 256.0).astype(np.float32)
    lv = (rng.integers(-64, 65, 3 * A) / 64.0).astype(np.float32)
    lv[lv == 0] = 0.5
    rc, rF = _ref_codes(bm, c1, tab1, margin=(F, lv, 0.1875))
    live = (c1[0] & 0xFF) != 0xFF
    leaf_node = live & (tab1.split_feat[np.minimum(c1[0] & 0xFF, A - 1)] < 0)
    fin = live & ((rc[0] & 0xFF) == 0xFF)
    assert leaf_node.sum() > 100 and (fin & ~leaf_node).sum() > 100 and (rF != F)[fin].all() and (rF == F)[~fin].all()
    gc, gF = _partition_codes(dev, bm, c1, tab1, margin=(F, lv, 0.1875), fm=fm)
    assert np.array_equal(gc, rc)
    assert np.array_equal(_bits(gF), _bits(rF))


@pytest.mark.parametrize("n", [1_300_003, 4_200_003])
def test_partition5_unrolled_slots_and_second_trip(dev, monkeypatch, n):
    """Tree 0's aligned loop: the grid is min(ceil((n / 4 + 1) / 256), 1024) = 1024 blocks, stride = 262144 words.

    n = 1 300 003: n4 = 325000 words; slot u covers words [u * stride, (u + 1) * stride): u = 0 all valid, u = 1 only
    q0 < 62856, u = 2, 3 guarded off; one trip.  n = 4 200 003: n4 = 1 050 000 > 4 * stride = 1 048 576: all four
    slots full, and a second trip for words 1 048 576 .. 1 049 999.  Both: 3 tail rows.  Tree 1 (n odd) takes the
    one-row loop over the same rows.  Rows are planted live at both ends of every slot's word range, in the second
    trip and in the tail, in a node whose two children have other local indices: a skipped slot leaves them
    unmoved."""
    _p5(monkeypatch)
    rng = np.random.default_rng(n)
    nloc = [9, 6]
    tab = R.edge_table(rng, nloc, 8)
    bm = R.edge_bins(rng, n, 8)
    codes = R.edge_codes(rng, nloc, n, done=0.7)
    stride, n4 = 262144, n // 4
    words = [q for u in range(5) for q in (u * stride, u * stride + 777, (u + 1) * stride - 1) if q < n4] + [n4 - 1]
    planted = np.array([4 * q + k for q in words for k in range(4)] + [n - 3, n - 2, n - 1])
    codes[:, planted] = 0x0301  # weight 3, local node 1 (ordered split at 255: children local 2 / 3 in tree 0)
    ref = _ref_codes(bm, codes, tab)
    assert (ref[0, planted] != codes[0, planted]).all() and (ref[1, planted] != codes[1, planted]).all()
    assert len(words) == {1_300_003: 6, 4_200_003: 15}[n]
    assert np.array_equal(_partition_codes(dev, bm, codes, tab), ref)


# ============================================================================================= partition7
def _p7_case(rng, n, G, T, per, feats=None, wzero=True):
    d = G * 8 - 3
    nloc = [per] * T
    tab = R.edge_table(rng, nloc, d, max_next=255, feats=feats)  # the node byte holds child local indices <= 254
    return R.edge_bins(rng, n, d), R.edge_codes(rng, nloc, n, wzero=wzero), tab


@pytest.mark.parametrize("G", [1, 8, 9, 13, 14, 16])
def test_partition7_row_widths(dev, monkeypatch, G):
    """The MAXG instantiations at their switch points: G <= 8 -> <8>, 9..13 -> <13>, 14..16 -> <16>."""
    p7, p5 = _p7(monkeypatch)
    bm, codes, tab = _p7_case(np.random.default_rng(200 + G), 1000, G, 3, 12)
    assert np.array_equal(_partition_codes(dev, bm, codes, tab, G=G), _ref_codes(bm, codes, tab))
    assert len(p7) == 1 and not p5


@pytest.mark.parametrize("groups", ["two", "every"])
def test_partition7_group_mask(dev, monkeypatch, groups):
    """G = 13.  two: every split reads group 0 or group 12, so the kernel skips the words of groups 1..11;
    every: each of the 13 groups is read by some split."""
    p7, _ = _p7(monkeypatch)
    rng = np.random.default_rng(17)
    G, d = 13, 101
    feats = np.r_[0:8, 96:101] if groups == "two" else None
    bm, codes, tab = _p7_case(rng, 1000, G, 4, 16, feats=feats)
    used = set((tab.split_feat[tab.split_feat >= 0] >> 3).tolist())
    if groups == "every":
        spare = [a for a in range(20, 64) if tab.split_feat[a] >= 0 and tab.cat_off[a] < 0][:13]
        tab.split_feat[spare] = np.arange(13) * 8 + 1
        used = set((tab.split_feat[tab.split_feat >= 0] >> 3).tolist())
    assert used == ({0, 12} if groups == "two" else set(range(13)))
    assert np.array_equal(_partition_codes(dev, bm, codes, tab, G=G), _ref_codes(bm, codes, tab))
    assert len(p7) == 1


@pytest.mark.parametrize("T", [1, 24, 25, 48, 49, 64])
def test_partition7_tree_blocks(dev, monkeypatch, T):
    """Trees move in blocks of kP7TB = 24: T = 25 / 48 take the reload branch t0 = 24, T = 49 / 64 also t0 = 48."""
    p7, _ = _p7(monkeypatch)
    bm, codes, tab = _p7_case(np.random.default_rng(300 + T), 300, 2, T, 3)
    assert np.array_equal(_partition_codes(dev, bm, codes, tab, G=2), _ref_codes(bm, codes, tab))
    assert len(p7) == 1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_partition7_row_counts(dev, monkeypatch, n):
    p7, _ = _p7(monkeypatch)
    bm, codes, tab = _p7_case(np.random.default_rng(400 + n), n, 3, 5, 9)
    assert np.array_equal(_partition_codes(dev, bm, codes, tab, G=3), _ref_codes(bm, codes, tab))
    assert len(p7) == 1


def test_partition7_1024_active_nodes(dev, monkeypatch):
    """A = 1024 = kP7MaxA: 8 trees of 128 nodes fill the LDS tables to their last entry."""
    p7, _ = _p7(monkeypatch)
    rng = np.random.default_rng(19)
    bm, codes, tab = _p7_case(rng, 3000, 2, 8, 128)
    assert len(tab.split_feat) == 1024
    codes[7, :128] = (codes[7, :128] & 0xFF00) | np.arange(128)
    assert np.array_equal(_partition_codes(dev, bm, codes, tab, G=2), _ref_codes(bm, codes, tab))
    assert len(p7) == 1


def test_partition7_second_trip(dev, monkeypatch):
    """n = 2 * 8 * 256 * CUs + 37 rows: the grid is at most per_cu * CUs blocks of 256 rows with per_cu <= 8 resident
    (launch bounds 4), so one trip covers at most 8 * 256 * CUs rows and every block runs the pipelined loop at
    least twice; the last 37 rows make a partial third trip for block 0."""
    p7, _ = _p7(monkeypatch)
    n = 2 * 8 * 256 * torch.cuda.get_device_properties(dev).multi_processor_count + 37
    bm, codes, tab = _p7_case(np.random.default_rng(23), n, 1, 2, 9, wzero=False)
    assert np.array_equal(_partition_codes(dev, bm, codes, tab, G=1), _ref_codes(bm, codes, tab))
    assert len(p7) == 1


@pytest.mark.parametrize("G,T,per", [(17, 3, 9), (2, 5, 205), (2, 65, 3)], ids=["G17", "A1025", "T65"])
def test_partition7_limits_fall_back_to_partition5(dev, monkeypatch, G, T, per):
    """One past each limit of partition7 (G 16, A 1024, T 64) the wrapper takes partition5, with the same result."""
    p7, p5 = _p7(monkeypatch)
    bm, codes, tab = _p7_case(np.random.default_rng(500 + G + T), 500, G, T, per)
    assert len(tab.split_feat) == T * per
    assert np.array_equal(_partition_codes(dev, bm, codes, tab, G=G), _ref_codes(bm, codes, tab))
    assert len(p5) == 1 and not p7


@pytest.mark.parametrize("variant", ["p5", "p7"])
def test_partition_codes_weight_byte_is_carried(dev, monkeypatch, variant):
    """Live codes with weight byte 0 move; done codes keep their weight byte (see K.partition_codes)."""
    _p5(monkeypatch) if variant == "p5" else _p7(monkeypatch)
    rng = np.random.default_rng(4)
    nloc = [9, 6]
    tab = R.edge_table(rng, nloc, 20)
    bm = R.edge_bins(rng, 600, 20)
    codes = R.edge_codes(rng, nloc, 600, wzero=True)
    got = _partition_codes(dev, bm, codes, tab)
    assert np.array_equal(got, _ref_codes(bm, codes, tab)) and np.array_equal(got >> 8, codes >> 8)


# ======================================================================================= partition (node ids)
@pytest.mark.parametrize("n", [1, 255, 257])
def test_partition_node_ids(dev, n):
    rng = np.random.default_rng(10 + n)
    d, nloc = 20, [9, 5, 3]
    tab = R.edge_table(rng, nloc, d)
    bm = R.edge_bins(rng, n, d)
    node = (tab.tfirst[:, None] + (rng.random((3, n)) * np.array(nloc)[:, None]).astype(np.int32)).astype(np.int32)
    node[rng.random((3, n)) < 0.2] = -1
    got = _t(node.copy(), dev)
    K.partition(_t(R.pack_bins(bm), dev), got, *[_t(x, dev) for x in (tab.split_feat, tab.split_bin, tab.cat_off,
                                                                       tab.cat_mask, tab.child)])
    assert np.array_equal(got.cpu().numpy(), R.ref_partition_nodes(bm, node, tab))


# ============================================================================================ seg_partition
def _assert_seg(got, ref, with_v0, with_w):
    np.testing.assert_array_equal(got[4], ref[4])
    assert np.array_equal(got[0].cpu().numpy(), ref[0])  # the order, not only the content
    assert np.array_equal(_bits(got[2]), _bits(ref[2]))
    if with_v0:
        assert np.array_equal(_bits(got[1]), _bits(ref[1]))
    if with_w:
        assert np.array_equal(got[3].cpu().numpy(), ref[3])


@pytest.mark.parametrize("with_v0,with_w", [(False, False), (True, True)])
def test_seg_partition(dev, with_v0, with_w):
    """Segment lengths 0 / 1 / 255 / 256 / 257 (the 256-row ballot round) and 8191 / 8192 / 8193 / 16385
    (SEG_PART_CHUNK = 8192: 1, 1, 2 and 3 chunks) in one call; see _rowmove_refs.seg_case for the split kinds."""
    bm, perm, v0, v1, w, segs, tab, n_next = R.seg_case(np.random.default_rng(6), 20)
    v0, w = (v0 if with_v0 else None), (w if with_w else None)
    ref = R.ref_seg_partition(bm, perm, v0, v1, w, segs, tab, n_next)
    got = K.seg_partition(_t(R.pack_bins(bm), dev), _t(perm, dev), None if v0 is None else _t(v0, dev), _t(v1, dev),
                          None if w is None else _t(w, dev), segs, tab.split_feat, tab.split_bin, tab.cat_off,
                          tab.cat_mask, tab.child, n_next)
    _assert_seg(got, ref, with_v0, with_w)


def test_seg_partition_implicit_level0(dev):
    """perm=None: 5 trees over 8200 rows (two chunks each); weight 0 at a tree's first and last row, a tree of
    weights 0 only, weight 255, a leaf tree, a tree keeping one child."""
    bm, v0, v1, w, segs, tab, n_next = R.seg_implicit_case(np.random.default_rng(7), 20)
    ref = R.ref_seg_partition(bm, None, v0, v1, w, segs, tab, n_next)
    got = K.seg_partition(_t(R.pack_bins(bm), dev), None, _t(v0, dev), _t(v1, dev), _t(w, dev), segs,
                          tab.split_feat, tab.split_bin, tab.cat_off, tab.cat_mask, tab.child, n_next)
    _assert_seg(got, ref, True, True)


# ============================================================================================ codes_compact
RANKS = [None, 0, 1, 2, 3]


def _set_rank(monkeypatch, rank, waves, defer=True):
    """The rank parametrisation of test_kernels_gpu.test_codes_compact: None = the atomic kernel, 0 / 1 = the
    wave-owned scatter by ballots / DPP scan, 2 / 3 = the queued scatter of records (3: loads a trip ahead)."""
    monkeypatch.setattr(K, "COMPACT_W", rank is not None)
    monkeypatch.setattr(K, "COMPACT_WAVES", waves)
    monkeypatch.setattr(K, "COMPACT_DEFER", defer)
    monkeypatch.setattr(K, "SCATTER_QUEUE", rank in (2, 3))
    monkeypatch.setattr(K, "SCATTER_PREFETCH", rank == 3)
    if rank is not None:
        monkeypatch.setattr(K, "SCATTER_RANK", min(rank, 1))
        monkeypatch.setattr(K, "SCATTER_SCAN_MIN_KB", 1)


def _check_compact(dev, codes, tfirst, bs, S, v1, stable, v0=None, plain=True):
    """Records first (with COMPACT_DEFER their buffer is sized by n * T, whatever the counts say), then the plain
    perm / v0 / v1 / w outputs."""
    rows, w, segs = R.ref_compact(tfirst, bs, S, codes=codes)
    c, v1d, tf = _codes_t(codes, dev), _t(v1, dev), _t(tfirst)
    out = K.codes_compact(c, tf, bs, S, None, v1d, rec_scale=R.REC_SCALE)
    np.testing.assert_array_equal(out[4], segs)
    got, ref = out[0].cpu().numpy(), R.ref_records(rows, w, v1, R.REC_SCALE)
    assert out[1] is None and got.dtype == np.int64
    if not stable:
        got, ref = R.sort_segments(got, segs), R.sort_segments(ref, segs)
    assert np.array_equal(got, ref)
    if not plain:
        return
    out = K.codes_compact(c, tf, bs, S, None if v0 is None else _t(v0, dev), v1d)
    np.testing.assert_array_equal(out[4], segs)
    perm, wp = out[0].cpu().numpy().astype(np.int64), out[3].cpu().numpy().astype(np.int64)
    assert np.array_equal(_bits(out[2]), _bits(v1[perm]))
    if v0 is not None:
        assert np.array_equal(_bits(out[1]), _bits(v0[perm]))
    key, rkey = perm << 8 | wp, rows << 8 | w
    if not stable:
        key, rkey = R.sort_segments(key, segs), R.sort_segments(rkey, segs)
    assert np.array_equal(key, rkey)


@pytest.mark.parametrize("n", [1000, 1001])
@pytest.mark.parametrize("kb", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("rank", RANKS)
def test_codes_compact_kb(dev, monkeypatch, rank, kb, n):
    """KB = 1 .. 16 built nodes per tree with a node at k = KB - 1, weights 1 and 255, a tree without built nodes;
    n % 4 = 1 takes the scalar code loads of the count and queue kernels.  per_wave = 256, Wv = 4."""
    _set_rank(monkeypatch, rank, 2048)
    rng = np.random.default_rng(30 + kb)
    codes, tfirst, bs, S = R.compact_case(rng, n, [kb, 0, max(kb // 2, 1)])
    _check_compact(dev, codes, tfirst, bs, S, R.rec_v1(rng, n), rank is not None,
                   v0=rng.random(n, dtype=np.float32) if kb == 8 else None)


@pytest.mark.parametrize("n", [40000, 40001])
@pytest.mark.parametrize("rank", [1, 3])
def test_codes_count_flush_and_saturation(dev, monkeypatch, rank, n):
    """COMPACT_WAVES = 1: per_wave = ceil(n / 256) * 256 = 40192 (<= 65536), one wave per tree, ceil(n / 512) = 79
    trips of 8 rows per lane: the 8-bit fields are flushed after trips 31 and 62 and at the end.  Tree 0: every row
    in built node k = 0 -- each lane's field reaches 31 * 8 = 248 before each flush (a flush one trip late would
    carry into field 1).  Tree 1: every row in k = KB - 1 = 7.  Tree 2: the 4 consecutive rows a lane owns share one
    node, k = lane % 8, so one field per lane saturates and the others stay 0."""
    _set_rank(monkeypatch, rank, 1)
    r = np.arange(n)
    codes, tfirst, bs, S = R.compact_case(np.random.default_rng(1), n, [8, 8, 8], unbuilt=0)
    assert bs.tolist() == list(range(24))
    codes[0], codes[1] = 0x0100, 0xFF07
    codes[2] = 0x0200 | (((r % 256) // 4) % 8)
    _check_compact(dev, codes, tfirst, bs, S, R.rec_v1(np.random.default_rng(2), n), True)


@pytest.mark.parametrize("n", [2148, 2149])
@pytest.mark.parametrize("rank", [2, 3])
def test_codes_scatter_queue_at_capacity(dev, monkeypatch, rank, n):
    """One wave (COMPACT_WAVES = 1, per_wave = 2304), trips of 512 rows.  Trip 0 holds 63 built rows: no full group,
    63 entries carry.  Trips 1..3 are 100 % built: the queue holds 63 + 512 = 575 of QCAP = 576 entries, drains 8
    groups and carries 63 again.  The last trip (100 or 101 rows) ends in a partial group.  KB = 16 with rows at
    k = 15 and weight 255 (the node field's and the weight field's last value)."""
    _set_rank(monkeypatch, rank, 1)
    rng = np.random.default_rng(n)
    codes, tfirst, bs, S = R.compact_case(rng, n, [16, 16], unbuilt=1, done=0.0)
    built_loc = [np.nonzero(bs[tfirst[t]:tfirst[t] + 17] >= 0)[0] for t in range(2)]
    for t in range(2):
        k = rng.integers(0, 16, n)
        k[600:700] = 15
        loc = built_loc[t][k]
        first = np.full(512, 0xFF)
        first[rng.permutation(512)[:63]] = built_loc[t][rng.integers(0, 16, 63)]
        loc[:512] = first
        codes[t] = (codes[t] & 0xFF00) | loc
    codes[:, 600:700] |= 0xFF00
    _check_compact(dev, codes, tfirst, bs, S, R.rec_v1(rng, n), True, plain=False)


@pytest.mark.parametrize("n,expect", [(65536, 3), (65537, 1)])
def test_codes_scatter_queue_cut(dev, monkeypatch, n, expect):
    """The queue packs a row's offset inside its wave into 16 bits.  One wave per tree: n = 65536 gives per_wave =
    65536, the last value _scatter_rank sends to the queue, with a built row at offset 65535 (weight 255, k = 15);
    n = 65537 gives per_wave = 65792 and the wave-owned scan (rank 1) instead."""
    _set_rank(monkeypatch, 3, 1)
    ranks = []
    real = K._scatter_rank
    monkeypatch.setattr(K, "_scatter_rank", lambda *a: ranks.append(real(*a)) or ranks[-1])
    rng = np.random.default_rng(n)
    codes, tfirst, bs, S = R.compact_case(rng, n, [16, 3], unbuilt=1, done=0.5)
    last = int(np.nonzero(bs[:17] >= 0)[0][-1])
    codes[0, 65535] = 0xFF00 | last
    codes[0, n - 1] = 0xFF00 | last
    _check_compact(dev, codes, tfirst, bs, S, R.rec_v1(rng, n), True, plain=False)
    assert ranks == [expect]


@pytest.mark.parametrize("rank", [1, 3])
def test_codes_compact_many_waves(dev, monkeypatch, rank):
    """COMPACT_WAVES = 2048, n = 70001: per_wave = 256, Wv = ceil(70001 / 256) = 274 > 256, so wave_scan's threads
    each own per = ceil(274 / 256) = 2 waves."""
    _set_rank(monkeypatch, rank, 2048)
    rng = np.random.default_rng(70001)
    codes, tfirst, bs, S = R.compact_case(rng, 70001, [5, 16, 1])
    _check_compact(dev, codes, tfirst, bs, S, R.rec_v1(rng, 70001), True)


@pytest.mark.parametrize("KB", [1, 4, 16])
@pytest.mark.parametrize("Wv", [1, 255, 256, 257, 1000])
def test_wave_scan(dev, Wv, KB):
    """cdna_wave_scan alone: per = ceil(Wv / 256) = 1, 1, 1, 2, 4 waves per thread."""
    cnt = np.random.default_rng(Wv + KB).integers(0, 700, (3, Wv, KB)).astype(np.int32)
    off, tot = R.ref_wave_scan(cnt)
    c = _t(cnt, dev)
    t = torch.empty((3, KB), dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().cdna_wave_scan(_ptr(c), 3, Wv, KB, _ptr(t), _stream(dev)), "cdna_wave_scan")
    assert np.array_equal(c.cpu().numpy(), off) and np.array_equal(t.cpu().numpy(), tot)


@pytest.mark.parametrize("defer", [True, False])
@pytest.mark.parametrize("rank", [1, 3])
def test_codes_compact_deferred_equals_direct(dev, monkeypatch, rank, defer):
    _set_rank(monkeypatch, rank, 4, defer=defer)
    rng = np.random.default_rng(77)
    codes, tfirst, bs, S = R.compact_case(rng, 5001, [8, 3, 0, 16])
    _check_compact(dev, codes, tfirst, bs, S, R.rec_v1(rng, 5001), True, plain=False)


def test_codes_compact_atomic_kernel(dev):
    """A tree with 17 built nodes leaves the wave-owned path (KB <= 16) for codes_compact_kernel, with COMPACT_W
    on.  Tree 1 has no built node; slots 3 and 20 receive no row."""
    rng = np.random.default_rng(17)
    n = 5001
    codes, tfirst, bs, S = R.compact_case(rng, n, [17, 0, 4])
    for s in (3, 20):
        a = int(np.nonzero(bs == s)[0][0])
        t = 0 if a < tfirst[1] else 2
        hit = (codes[t] & 0xFF) == a - tfirst[t]
        codes[t, hit] |= 0xFF
    _check_compact(dev, codes, tfirst, bs, S, R.rec_v1(rng, n), False, v0=rng.random(n, dtype=np.float32))
    segs = R.ref_compact(tfirst, bs, S, codes=codes)[2]
    assert segs[3, 1] == 0 and segs[20, 1] == 0 and S == 21


def test_codes_compact_atomic_kernel_empty_blocks(dev):
    """n = 2 100 001 > 512 * 4096: the grid caps at 512 blocks per tree of per = ceil(ceil(n / 512) / 256) * 256 =
    4352 rows, so blocks 483..511 (483 * 4352 > n) have an empty row range."""
    rng = np.random.default_rng(21)
    n = 2_100_001
    codes, tfirst, bs, S = R.compact_case(rng, n, [17, 0], done=0.8)
    _check_compact(dev, codes, tfirst, bs, S, R.rec_v1(rng, n), False, plain=False)


@pytest.mark.parametrize("rank", RANKS)
def test_codes_compact_no_slots(dev, monkeypatch, rank):
    """S = 0: no node of the level is built."""
    _set_rank(monkeypatch, rank, 2048)
    rng = np.random.default_rng(8)
    codes, tfirst, bs, S = R.compact_case(rng, 1000, [0, 0])
    out = K.codes_compact(_codes_t(codes, dev), _t(tfirst), bs, 0, None, _t(R.rec_v1(rng, 1000), dev),
                          rec_scale=R.REC_SCALE)
    assert out[0].numel() == 0 and out[4].shape == (0, 2)


@pytest.mark.parametrize("rank", RANKS)
def test_compact_record_quantisation(dev, monkeypatch, rank):
    """Every row built, so each REC_EDGE_V1 value (v1 * scale = +-2^23, one past, far past, the ties k + 0.5, -0.0)
    is quantised by each scatter kernel: clamp(rint(.)) in fp32, ties to even."""
    _set_rank(monkeypatch, rank, 2048)
    rng = np.random.default_rng(9)
    n = 333
    codes, tfirst, bs, S = R.compact_case(rng, n, [2, 1], unbuilt=0, done=0.0)
    v1 = R.rec_v1(rng, n)
    assert np.array_equal(v1[:16].view(np.int32), R.REC_EDGE_V1.view(np.int32))
    _check_compact(dev, codes, tfirst, bs, S, v1, rank is not None, plain=False)


# ============================================================================================= node_compact
@pytest.mark.parametrize("n", [1, 255, 2049])
@pytest.mark.parametrize("nloc", [[1, 256], [257, 1024, 3]], ids=["1-256", "257-1024-3"])
def test_node_compact(dev, n, nloc):
    """Trees with 1, 256, 257 and 1024 = kNodeCompactLoc active nodes (the last row of every tree sits in the tree's
    last node: local index 1023 of the table); ids -1 and ids of another tree's range do not count; built and
    unbuilt siblings; weights 1 and 255."""
    rng = np.random.default_rng(40 + n)
    node, w, tfirst, bs, S = R.node_case(rng, n, nloc)
    v1 = R.rec_v1(rng, n)
    rows, wts, segs = R.ref_compact(tfirst, bs, S, node=node, w=w)
    rec, sg = K.node_compact(_t(node, dev), _t(w, dev), tfirst, bs, S, _t(v1, dev), R.REC_SCALE)
    np.testing.assert_array_equal(sg, segs)
    assert np.array_equal(R.sort_segments(rec.cpu().numpy(), segs),
                          R.sort_segments(R.ref_records(rows, wts, v1, R.REC_SCALE), segs))


def test_node_compact_refuses_1025_nodes(dev):
    rng = np.random.default_rng(9)
    node, w, tfirst, bs, S = R.node_case(rng, 10, [1025, 2])
    with pytest.raises(ValueError, match="1024"):
        K.node_compact(_t(node, dev), _t(w, dev), tfirst, bs, S, _t(R.rec_v1(rng, 10), dev), R.REC_SCALE)


# ============================================================================================ layout changes
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_decode_codes_and_codes_init(dev, n, T):
    """codes_to_nodes (4 codes per thread when n % 4 == 0, else one) and codes_init (16 weights per thread, then the
    tail; the largest weight in the last element)."""
    rng = np.random.default_rng(50 + n + T)
    codes = R.edge_codes(rng, [7] * T, n, wzero=True)
    tfirst = np.arange(T, dtype=np.int32) * 7
    ids, w = K.decode_codes(_codes_t(codes, dev), _t(tfirst))
    rid, rw = R.ref_decode_codes(codes, tfirst)
    assert np.array_equal(ids.cpu().numpy(), rid) and np.array_equal(w.cpu().numpy(), rw)
    wts = rng.integers(0, 3, (T, n)).astype(np.uint8)
    wts[T - 1, n - 1] = 255
    c, wmax = K.codes_init_max(_t(wts, dev), T, n, dev)
    rc, rmax = R.ref_codes_init(wts)
    assert np.array_equal(_u16(c), rc) and wmax == rmax == 255
    c, wmax = K.codes_init_max(_t(np.zeros((T, n), np.uint8), dev), T, n, dev)
    assert (_u16(c) == 0xFF).all() and wmax == 1


@pytest.mark.parametrize("G", [1, 13, 16, 17])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_bins_row_major(dev, n, G):
    """Unpadded [n, G, 8] and padded to Gs = 16 words (G = 17 stays 17: no padding past 16)."""
    bins = R.pack_bins(R.edge_bins(np.random.default_rng(60 + G), n, G * 8 - 3))
    b = _t(bins, dev)
    assert np.array_equal(K.bins_row_major(b, pad=False).cpu().numpy(), R.ref_bins_row_major(bins))
    padded = K.bins_row_major(b, pad=True).cpu().numpy()
    assert np.array_equal(padded, R.ref_bins_row_major(bins, 16 if G <= 16 else G))
