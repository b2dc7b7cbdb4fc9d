"""Plain references of the row-movement operations of the tree engine (the partition, segment-partition and
compaction kernels of hist5.hip / seg.hip / trees.hip and their host paths in cdnaml/ops/kernels.py), and the edge
shaped cases tests/test_rowmove_cpu.py and tests/test_rowmove_gpu.py share.

numpy and Python integers only; nothing of cdnaml.ops.kernels but the format constants.  Every contract is stated
in a few lines:

* a row of active node ``a`` goes LEFT when ``go_left(bin of feature split_feat[a], a)``;
* a node with ``split_feat < 0`` is a leaf: its rows finish (node id -1, code byte 0xFF);
* a child index of -1 finishes the row as well;
* a row code is ``weight << 8 | local node``; the code is DONE when its node byte is 0xFF, whatever its weight
  byte holds, and the weight byte is never changed by a partition.

The bins of a case are a byte matrix ``bm [n, d]``; ``pack_bins`` lays it out as the [G, n, 8] words of the
kernels, so a case places bin 0 / 31 / 32 / 223 / 224 / 255 exactly where it wants them."""
from types import SimpleNamespace

import numpy as np

from cdnaml.ops.kernels import CODE_DONE, PACK_Q, REC_ROW_BITS, REC_W_BITS

EDGE_BINS = np.array([0, 31, 32, 223, 224, 255], dtype=np.uint8)


# ===================================================================================================== layouts
def pack_bins(bm):
    """bm uint8 [n, d] -> the kernels' words uint8 [G, n, 8], G = ceil(d / 8) (feature f = byte f % 8 of word f // 8;
    the bytes past d are 0)."""
    n, d = bm.shape
    G = (d + 7) // 8
    out = np.zeros((G, n, 8), dtype=np.uint8)
    for f in range(d):
        out[f >> 3, :, f & 7] = bm[:, f]
    return out


def ref_bins_row_major(bins, Gs=None):
    """[G, n, 8] -> [n, Gs, 8]: row r holds its G words in order, then zero words up to Gs."""
    G, n, _ = bins.shape
    Gs = G if Gs is None else Gs
    out = np.zeros((n, Gs, 8), dtype=np.uint8)
    for g in range(G):
        out[:, g, :] = bins[g]
    return out


def feature_major(bm, G):
    """bm [n, d] -> the feature-major byte copy [G * 8, n] (rows past d are 0)."""
    n, d = bm.shape
    out = np.zeros((G * 8, n), dtype=np.uint8)
    out[:d] = bm.T
    return out


# ================================================================================================= the split rule
def go_left(bins, node, tab):
    """Does a row whose split feature holds ``bins`` go left at active node ``node``?  (arrays of equal shape)

    ordered split: bin <= split_bin; bin-set split (cat_off >= 0): bit (bin & 31) of the UNSIGNED 32-bit word
    cat_off * 8 + (bin >> 5)."""
    b = np.asarray(bins, dtype=np.int64)
    a = np.asarray(node, dtype=np.int64)
    co = tab.cat_off.astype(np.int64)[a]
    words = np.asarray(tab.cat_mask).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    if words.size == 0:
        words = np.zeros(8, dtype=np.int64)
    in_set = ((words[np.maximum(co, 0) * 8 + (b >> 5)] >> (b & 31)) & 1) == 1
    return np.where(co >= 0, in_set, b <= tab.split_bin.astype(np.int64)[a])


def _next_of(bm, rows, a, tab):
    """(leaf, side, child) of rows ``rows`` sitting in active nodes ``a``: side 0 = left, 1 = right."""
    f = tab.split_feat.astype(np.int64)[a]
    leaf = f < 0
    side = np.where(go_left(bm[rows, np.maximum(f, 0)], a, tab), 0, 1)
    child = tab.child.astype(np.int64)[2 * a + side]
    return leaf, side, np.where(leaf, -1, child)


def ref_partition_nodes(bm, node, tab):
    """node int32 [T, n] of global active ids -> the next level's: -1 stays, a leaf gives -1, otherwise the child."""
    out = np.array(node, dtype=np.int32)
    for t in range(node.shape[0]):
        rows = np.nonzero(node[t] >= 0)[0]
        _, _, child = _next_of(bm, rows, node[t, rows].astype(np.int64), tab)
        out[t, rows] = child
    return out


def ref_partition_codes(bm, codes, tfirst, tfirst_next, tab, margin=None):
    """codes uint16 [T, n] -> the next level's codes (and the margins when ``margin = (F, lv, eta)``, T = 1).

    The weight byte is kept.  The node byte becomes child - tfirst_next[t], or 0xFF for a leaf, a -1 child or a code
    whose node byte is 0xFF already.  A row that finishes here adds eta * lv[e] to F[row] in fp32:
    e = 2 * a + side under a splitting node, 2 * A + a under a node that does not split."""
    codes = np.asarray(codes, dtype=np.uint16)
    T, n = codes.shape
    A = len(tab.split_feat)
    out = codes.copy()
    F = None
    if margin is not None:
        assert T == 1
        F = np.array(margin[0], dtype=np.float32)
        lv, eta = np.asarray(margin[1], dtype=np.float32), np.float32(margin[2])
    for t in range(T):
        loc = (codes[t] & 0xFF).astype(np.int64)
        rows = np.nonzero(loc != CODE_DONE)[0]
        a = int(tfirst[t]) + loc[rows]
        leaf, side, child = _next_of(bm, rows, a, tab)
        nl = np.where(child < 0, CODE_DONE, child - int(tfirst_next[t]))
        assert nl.min(initial=0) >= 0 and nl.max(initial=0) <= 0xFF
        out[t, rows] = (codes[t, rows] & 0xFF00) | nl.astype(np.uint16)
        if F is not None:
            fin = child < 0
            e = np.where(leaf, 2 * A + a, 2 * a + side)[fin]
            F[rows[fin]] = F[rows[fin]] + eta * lv[e]  # one rounded product, one rounded sum (exact on dyadic data)
    return out if F is None else (out, F)


def ref_decode_codes(codes, tfirst):
    """codes [T, n] -> (node ids int32, weights uint8): id = tfirst[t] + node byte; -1 where the node byte is 0xFF or
    the weight is 0 (a weight-0 row adds nothing to any histogram, so the node-id kernels skip it)."""
    c = np.asarray(codes, dtype=np.uint16).astype(np.int64)
    loc, w = c & 0xFF, c >> 8
    ids = np.asarray(tfirst, dtype=np.int64)[:, None] + loc
    return np.where((loc == CODE_DONE) | (w == 0), -1, ids).astype(np.int32), w.astype(np.uint8)


def ref_codes_init(w):
    """weights uint8 [T, n] -> (codes uint16: w << 8 at the root, 0xFF where w = 0; the largest weight, >= 1)."""
    w = np.asarray(w, dtype=np.uint8).astype(np.uint16)
    return (w << 8) | np.where(w == 0, CODE_DONE, 0).astype(np.uint16), max(1, int(w.max(initial=0)))


# ============================================================================================ segment partition
def ref_seg_partition(bm, perm, v0, v1, w, segs, tab, n_next):
    """Stable split of every segment into its children's segments; rows of leaves and of -1 children are dropped.

    perm [m] rows, v0 / v1 / w [m] permuted alike, segs [A, 2] {start, len}.  ``perm=None`` is the level-0 entry:
    segment a is tree a over rows 0..n-1, w is [T, n], v0 / v1 are per row, weight-0 rows are dropped.
    Returns (perm, v0, v1, w, segs_next): child c's rows in their segment order, children in index order."""
    n = bm.shape[0]
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 2)
    implicit = perm is None
    pieces = [np.zeros(0, dtype=np.int64) for _ in range(n_next)]
    wflat = None if w is None else np.asarray(w).reshape(-1)
    for a, (s, ln) in enumerate(segs):
        if tab.split_feat[a] < 0 or ln == 0:
            continue
        idx = np.arange(s, s + ln)
        if implicit:
            idx = idx[wflat[idx] > 0]
            rows = idx - a * n
        else:
            rows = np.asarray(perm, dtype=np.int64)[idx]
        _, _, child = _next_of(bm, rows, np.full(len(rows), a, dtype=np.int64), tab)
        for c in np.unique(child[child >= 0]):
            pieces[c] = np.concatenate([pieces[c], idx[child == c]])
    lens = np.array([len(p) for p in pieces], dtype=np.int64)
    starts = np.cumsum(lens) - lens
    src = np.concatenate(pieces) if n_next else np.zeros(0, dtype=np.int64)
    rows = src % n if implicit else np.asarray(perm, dtype=np.int64)[src]
    stat = rows if implicit else src
    return (rows.astype(np.int32), None if v0 is None else np.asarray(v0)[stat], np.asarray(v1)[stat],
            None if w is None else wflat[src], np.stack([starts, lens], 1))


# =================================================================================================== compaction
def _tree_of(tfirst, A):
    """Tree of every active node: tree t owns [tfirst[t], tfirst[t + 1]) (the last one up to A)."""
    ends = np.concatenate([np.asarray(tfirst, dtype=np.int64)[1:], [A]])
    out = np.full(A, -1, dtype=np.int64)
    for t, (lo, hi) in enumerate(zip(tfirst, ends)):
        out[int(lo):int(hi)] = t
    return out


def ref_compact(tfirst, build_slot, S, codes=None, node=None, w=None):
    """Rows of built nodes, one segment per slot: (rows, weights, segs [S, 2]).

    From codes uint16 [T, n], or from node ids int32 [T, n] + weights uint8 [T, n].  A row of tree t belongs to
    active node a when its code / id names a and a is one of tree t's nodes; slot build_slot[a] >= 0 lists its
    (row, weight) pairs in row order."""
    bs = np.asarray(build_slot, dtype=np.int64)
    A = len(bs)
    if codes is not None:
        c = np.asarray(codes, dtype=np.uint16).astype(np.int64)
        loc = c & 0xFF
        ids = np.where(loc == CODE_DONE, -1, np.asarray(tfirst, dtype=np.int64)[:, None] + loc)
        wts = c >> 8
    else:
        ids, wts = np.asarray(node, dtype=np.int64), np.asarray(w, dtype=np.int64)
    tree_of = _tree_of(tfirst, A)
    rows_o, w_o, lens = [], [], np.zeros(S, dtype=np.int64)
    node_of_slot = {int(s): a for a, s in enumerate(bs) if s >= 0}
    for s in range(S):
        a = node_of_slot.get(s)
        if a is None or tree_of[a] < 0:
            continue
        t = tree_of[a]
        r = np.nonzero(ids[t] == a)[0]
        rows_o.append(r)
        w_o.append(wts[t, r])
        lens[s] = len(r)
    cat = (lambda p: np.concatenate(p) if p else np.zeros(0, dtype=np.int64))
    return cat(rows_o), cat(w_o), np.stack([np.cumsum(lens) - lens, lens], 1)


def ref_records(rows, w, v1, scale):
    """Packed item records int64: row | w << 31 | (q + 2^23) << 39 with q = clamp(rint(fp32(v1) * fp32(scale)),
    +-2^23), the product and the round-half-even in fp32."""
    x = np.asarray(v1, dtype=np.float32)[rows] * np.float32(scale)
    assert x.dtype == np.float32
    q = np.clip(np.rint(x).astype(np.int64), -PACK_Q, PACK_Q)
    rec = (np.asarray(rows).astype(np.uint64) | (np.asarray(w).astype(np.uint64) << np.uint64(REC_ROW_BITS)) |
           ((q + PACK_Q).astype(np.uint64) << np.uint64(REC_ROW_BITS + REC_W_BITS)))
    return rec.view(np.int64)


def ref_wave_scan(cnt):
    """cnt int [T, Wv, KB] -> (exclusive prefix over the waves, totals [T, KB])."""
    c = np.asarray(cnt, dtype=np.int64)
    return np.cumsum(c, 1) - c, c.sum(1)


def sort_segments(x, segs):
    """x with every segment sorted (for the kernels whose order inside a segment is unspecified)."""
    out = np.array(x)
    for s, ln in np.asarray(segs, dtype=np.int64):
        out[s:s + ln] = np.sort(out[s:s + ln])
    return out


# ============================================================================================= the shared cases
def edge_bins(rng, n, d):
    """bm [n, d]: half the bytes from EDGE_BINS, half uniform; the first rows cycle through the edges in every
    feature so even n = 1 .. 6 see one."""
    bm = np.where(rng.random((n, d)) < 0.5, EDGE_BINS[rng.integers(0, 6, (n, d))],
                  rng.integers(0, 256, (n, d))).astype(np.uint8)
    k = min(n, 12)
    bm[:k] = EDGE_BINS[(np.arange(k)[:, None] + np.arange(d)[None, :]) % 6]
    return bm


def edge_masks(rng):
    """Three bin sets (24 int32 words): set 0 has bit 31 of every word set (negative as int32); set 1 holds bins 224
    and 255 (bits 0 and 31 of word 7) but not 223 or 225; set 2 is random."""
    m = rng.integers(0, 2 ** 32, 24, dtype=np.uint64)
    m[:8] |= 0x80000000
    m[8 + 7] = (m[8 + 7] | 0x80000001) & ~np.uint64(0x00000002)
    m[8 + 6] &= ~np.uint64(0x80000000)
    return m.astype(np.uint32).view(np.int32)


def edge_table(rng, nloc, d, max_next=None, feats=None):
    """A split table over trees with ``nloc[t]`` active nodes each.  The first nodes of the level are the edges the
    issue names -- ordered splits at bin 0 and 255, bin sets with bit 31 / word 7, a leaf, one-sided children, a
    node whose children are both -1, split features 0 / 7 / 8 / d - 1 -- the rest are random.  ``max_next``: at most
    that many children per tree (the others finish); ``feats``: the features random nodes draw from.
    Returns a namespace (split_feat, split_bin, cat_off, cat_mask, child, tfirst, tfirst_next, n_next)."""
    nloc = np.asarray(nloc, dtype=np.int64)
    A = int(nloc.sum())
    tfirst = np.cumsum(nloc) - nloc
    feats = np.arange(d) if feats is None else np.asarray(feats)
    sf = feats[rng.integers(0, len(feats), A)].astype(np.int32)
    sb = np.where(rng.random(A) < 0.5, EDGE_BINS[rng.integers(0, 6, A)], rng.integers(0, 256, A)).astype(np.int32)
    co = np.where(rng.random(A) < 0.3, rng.integers(0, 3, A), -1).astype(np.int32)
    kind = np.where(rng.random(A) < 0.15, 1, 0)  # 1: leaf
    keep = rng.random((A, 2)) < 0.8
    f_of = (lambda f: int(f) if f in feats else int(feats[0]))
    edges = [  # (feature, bin, cat_off, leaf, keep left, keep right)
        (0, 0, -1, 0, 1, 1), (min(7, d - 1), 255, -1, 0, 1, 1), (min(8, d - 1), 5, 0, 0, 1, 1),
        (d - 1, 5, 1, 0, 1, 1), (0, 0, -1, 1, 1, 1), (d - 1, 31, -1, 0, 0, 1), (0, 224, -1, 0, 1, 0),
        (min(7, d - 1), 32, -1, 0, 0, 0), (min(8, d - 1), 223, 2, 0, 1, 1)]
    for a, (f, b, c, lf, kl, kr) in enumerate(edges[:A]):
        sf[a], sb[a], co[a], kind[a], keep[a] = f_of(f), b, c, lf, (kl, kr)
    sf[kind == 1] = -1
    co[sf < 0] = -1
    child = np.full(2 * A, -1, dtype=np.int32)
    tfirst_next = np.zeros(len(nloc), dtype=np.int64)
    nxt = 0
    for t in range(len(nloc)):
        tfirst_next[t] = nxt
        for a in range(int(tfirst[t]), int(tfirst[t] + nloc[t])):
            for s in (0, 1):
                if sf[a] >= 0 and keep[a, s] and (max_next is None or nxt - tfirst_next[t] < max_next):
                    child[2 * a + s] = nxt
                    nxt += 1
    return SimpleNamespace(split_feat=sf, split_bin=sb, cat_off=co, cat_mask=edge_masks(rng), child=child,
                           tfirst=tfirst.astype(np.int32), tfirst_next=tfirst_next.astype(np.int32), n_next=nxt,
                           nloc=nloc)


def edge_codes(rng, nloc, n, done=0.1, wzero=False):
    """codes uint16 [T, n]: node bytes uniform over each tree's local nodes, ``done`` of them 0xFF; weights from
    {1, 2, 3, 254, 255}.  wzero: some LIVE codes with weight byte 0 and some done codes with weight byte 0 / 7."""
    T = len(nloc)
    loc = (rng.random((T, n)) * np.asarray(nloc)[:, None]).astype(np.int64)
    loc[rng.random((T, n)) < done] = CODE_DONE
    loc[np.asarray(nloc) == 0] = CODE_DONE
    w = np.array([1, 2, 3, 254, 255])[rng.integers(0, 5, (T, n))]
    if wzero:
        w[rng.random((T, n)) < 0.2] = 0
        w[(loc == CODE_DONE) & (rng.random((T, n)) < 0.5)] = 7
    return ((w << 8) | loc).astype(np.uint16)


ZERO_SET = 3  # edge_masks4: the empty bin set (every row goes right)


def edge_masks4(rng):
    """edge_masks plus a fourth, empty set."""
    return np.concatenate([edge_masks(rng), np.zeros(8, dtype=np.int32)])


SEG_LENS = (257, 0, 1, 255, 256, 8191, 8192, 8193, 16385, 300, 0, 64)


def seg_case(rng, d, lens=SEG_LENS):
    """The segment-partition case: one call whose segment lengths sit around the 256-row ballot round and the
    8192-row chunk, zero-length ones included.  Segment 3 is a leaf between split ones, 5 goes all left (ordered
    split at bin 255), 6 all right (empty bin set), 7 keeps only its right child and 8 only its left one (both
    longer than a chunk: the dropped side's base is -1 in every chunk), 9 loses both children, 10 is an empty leaf.
    Returns (bm, perm, v0, v1, w, segs, tab, n_next)."""
    lens = np.asarray(lens, dtype=np.int64)
    A, m = len(lens), int(lens.sum())
    n = m + m // 5 + 7
    bm = edge_bins(rng, n, d)
    perm = rng.permutation(n)[:m].astype(np.int32)
    sf = np.array([0, 3, min(8, d - 1), -1, d - 1, min(7, d - 1), 2, 1, d - 2, 4, -1, min(8, d - 1)], dtype=np.int32)
    sb = np.array([0, 9, 0, 0, 0, 255, 0, 100, 31, 32, 0, 0], dtype=np.int32)
    co = np.array([-1, -1, 0, -1, 1, -1, ZERO_SET, -1, -1, -1, -1, 2], dtype=np.int32)
    keep = np.ones((A, 2), dtype=bool)
    keep[7, 0] = keep[8, 1] = False
    keep[9] = False
    child = np.full(2 * A, -1, dtype=np.int32)
    nxt = 0
    for a in range(A):
        for s in (0, 1):
            if sf[a] >= 0 and keep[a, s]:
                child[2 * a + s] = nxt
                nxt += 1
    tab = SimpleNamespace(split_feat=sf, split_bin=sb, cat_off=co, cat_mask=edge_masks4(rng), child=child)
    w = np.array([1, 2, 3, 254, 255], dtype=np.uint8)[rng.integers(0, 5, m)]
    v0 = rng.random(m, dtype=np.float32)
    v1 = rng.standard_normal(m).astype(np.float32)
    return bm, perm, v0, v1, w, np.stack([np.cumsum(lens) - lens, lens], 1), tab, nxt


def seg_implicit_case(rng, d, n=8200):
    """The level-0 entry: 5 trees over n rows (n > 8192: two chunks per tree).  Tree 0 has weight 0 at its first
    and last row, tree 1 only weights 0, tree 2 weights 255 among zeros, tree 3 is a leaf, tree 4 keeps its right
    child only.  Returns (bm, v0, v1, w [T, n], segs, tab, n_next)."""
    T = 5
    bm = edge_bins(rng, n, d)
    w = rng.integers(0, 4, (T, n)).astype(np.uint8)
    w[0, 0] = w[0, n - 1] = 0
    w[0, 1] = w[0, n - 2] = 255
    w[1] = 0
    w[2] = np.where(rng.random(n) < 0.5, 255, 0)
    w[4, 0] = w[4, n - 1] = 1
    sf = np.array([0, 5, d - 1, -1, min(8, d - 1)], dtype=np.int32)
    sb = np.array([31, 100, 0, 0, 223], dtype=np.int32)
    co = np.array([-1, -1, 1, -1, -1], dtype=np.int32)
    child = np.array([0, 1, 2, 3, 4, 5, -1, -1, -1, 6], dtype=np.int32)
    tab = SimpleNamespace(split_feat=sf, split_bin=sb, cat_off=co, cat_mask=edge_masks4(rng), child=child)
    segs = np.stack([np.arange(T) * n, np.full(T, n)], 1)
    return bm, rng.random(n, dtype=np.float32), rng.standard_normal(n).astype(np.float32), w, segs, tab, 7


def compact_case(rng, n, kbs, unbuilt=2, done=0.2):
    """Row codes for a compaction: tree t has kbs[t] built nodes among kbs[t] + unbuilt active ones (built and unbuilt
    interleaved, the tree's LAST node built when it has one: k = kbs[t] - 1), slots numbered tree-major; weights 1
    and 255; ``done`` of the codes finished.  Returns (codes uint16 [T, n], tfirst, build_slot, S)."""
    kbs = np.asarray(kbs, dtype=np.int64)
    nloc = kbs + unbuilt
    tfirst = (np.cumsum(nloc) - nloc).astype(np.int32)
    bs = np.full(int(nloc.sum()), -1, dtype=np.int32)
    s = 0
    for t, kb in enumerate(kbs):
        pick = np.sort(rng.permutation(int(nloc[t]) - 1)[:max(int(kb) - 1, 0)])
        built = np.concatenate([pick, [nloc[t] - 1]]) if kb else pick
        bs[tfirst[t] + built] = s + np.arange(len(built))
        s += len(built)
    loc = (rng.random((len(kbs), n)) * nloc[:, None]).astype(np.int64)
    loc[rng.random(loc.shape) < done] = CODE_DONE
    w = np.where(rng.random(loc.shape) < 0.5, 1, 255)
    return ((w << 8) | loc).astype(np.uint16), tfirst, bs, s


REC_SCALE = 1024.0
# v1 * REC_SCALE at +-2^23 (the clamp's last value), one past it, far past it, at k + 0.5 (ties to even) and at -0.0
REC_EDGE_V1 = np.array([8192.0, -8192.0, 8192.0009765625, -8192.0009765625, 9000.0, -9000.0, 0.5 / 1024, 1.5 / 1024,
                        2.5 / 1024, -0.5 / 1024, -1.5 / 1024, -2.5 / 1024, 4194303.5 / 1024, -4194303.5 / 1024,
                        -0.0, 0.0], dtype=np.float32)


def rec_v1(rng, n):
    """Labels for a record compaction: REC_EDGE_V1 cycling through the first rows, then random."""
    v1 = (rng.standard_normal(n) * 3).astype(np.float32)
    k = min(n, 4 * len(REC_EDGE_V1))
    v1[:k] = np.resize(REC_EDGE_V1, k)
    return v1


def node_case(rng, n, nloc):
    """Node ids for node_compact: tree t owns nloc[t] nodes; ids are the tree's own nodes, -1, or (wrongly) another
    tree's node, which must not count; about half of the nodes are built (siblings 2k / 2k + 1 both ways); weights 1
    and 255.  Returns (node int32 [T, n], w uint8 [T, n], tfirst, build_slot, S)."""
    nloc = np.asarray(nloc, dtype=np.int64)
    T, A = len(nloc), int(nloc.sum())
    tfirst = np.cumsum(nloc) - nloc
    node = (tfirst[:, None] + (rng.random((T, n)) * nloc[:, None]).astype(np.int64))
    node[rng.random((T, n)) < 0.15] = -1
    foreign = rng.random((T, n)) < 0.15
    other = rng.integers(0, A, (T, n))
    own = (other >= tfirst[:, None]) & (other < (tfirst + nloc)[:, None])
    node = np.where(foreign & ~own, other, node)
    # the last node of every tree is used by the tree's last row (local index nloc - 1 at the table's end)
    node[:, n - 1] = tfirst + nloc - 1
    built = rng.random(A) < 0.5
    built[tfirst + nloc - 1] = True
    bs = np.full(A, -1, dtype=np.int32)
    bs[built] = np.arange(int(built.sum()))
    w = np.where(rng.random((T, n)) < 0.5, 1, 255).astype(np.uint8)
    return node.astype(np.int32), w, tfirst, bs, int(built.sum())
