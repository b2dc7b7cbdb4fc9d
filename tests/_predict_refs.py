"""Independent references, forests and rows for the forest predict kernels (csrc/kernels/trees.hip:
predict_kernel, predict_heap_kernel, heap_to_bins_kernel + predict_heap_binned_kernel, predict_binned_kernel,
heap_last_level_kernel).

Plain numpy on the CPU, nothing from ``cdnaml``.  A case is a random forest in the per-slot heap layout together with
rows made to sit on the kernels' edges, the leaf slot every (row, tree) reaches by this module's own walk, and the fp64
ensemble sum in the kernels' documented order, so device and host results are compared with ``torch.equal``.

Split rules (trees.hip's header):
* numeric: left iff fp32(x) <= fp32(thr); NaN goes right;
* categorical on raw features: the category is (int)x, truncated towards zero (3.7 -> 3, -0.5 -> 0); left iff x is
  not NaN, 0 <= (int)x < 256 and bit (int)x of the node's 256-bit mask is set; everything else goes right;
* on bins (predict_binned_kernel): numeric left iff bin <= node bin, categorical left iff mask bit ``bin`` is set.

Sum (the kernels' contract): tree lane q = t % 4 adds fl64(tw[t] * v) over its trees in ascending t starting from 0.0,
then ((((base + lane0) + lane1) + lane2) + lane3); every product and every sum is one rounded fp64 operation.

Every case asserts its coverage condition from the reference walk alone: each tree whose root is a split sends at
least one row to either side (n >= 2: one row cannot go both ways), and with n >= 4 * 2^depth at least half of every
tree's reachable leaves receive a row.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

F32 = np.float32
# what a categorical column holds besides the integers of [0, 256)
CAT_ODD = (3.7, -0.5, 255.9, -1.0, 256.0, 300.0, 3e9, 1e20, np.inf, -np.inf, np.nan)
BIG_N = 8192 * 64 + 65          # a second grid-stride trip of the 64-row kernels (grid cap 8192) and a 1-row last tile
BIG_N_BINNED_ADD = 4096 * 256 + 257   # the same for predict_binned_kernel (256 rows per block, grid cap 4096)
GROW_ROWS = 4096                # rows the generator looks at when it picks splits that divide them


# ------------------------------------------------------------------------------------------------ rows
def _numeric_column(rng, n, pool, with_zero):
    """Random values mixed with the pool's thresholds exactly, their fp32 neighbours on both sides, +-inf, NaN and
    (``with_zero``: the pool holds 0.0) +-0.0."""
    x = rng.normal(size=n).astype(F32)
    kind = rng.integers(0, 100, size=n)
    if len(pool):
        p = np.asarray(pool, dtype=F32)[rng.integers(0, len(pool), size=n)]
        x = np.where(kind < 15, p, x)
        x = np.where((kind >= 15) & (kind < 23), np.nextafter(p, F32(np.inf)), x)
        x = np.where((kind >= 23) & (kind < 31), np.nextafter(p, F32(-np.inf)), x)
    x = np.where((kind >= 31) & (kind < 34), F32(np.inf), x)
    x = np.where((kind >= 34) & (kind < 37), F32(-np.inf), x)
    x = np.where((kind >= 37) & (kind < 42), F32(np.nan), x)
    if with_zero:
        x = np.where((kind >= 42) & (kind < 46), F32(0.0), x)
        x = np.where((kind >= 46) & (kind < 50), F32(-0.0), x)
    return x.astype(F32)


def _cat_column(rng, n):
    x = rng.integers(0, 256, size=n).astype(F32)
    kind = rng.integers(0, 100, size=n)
    x = np.where(kind < 10, F32(0.0), x)
    x = np.where((kind >= 10) & (kind < 16), F32(255.0), x)
    x = np.where((kind >= 60) & (kind < 70), F32(np.nan), x)
    odd = np.asarray(CAT_ODD, dtype=F32)[rng.integers(0, len(CAT_ODD), size=n)]
    return np.where(kind >= 70, odd, x).astype(F32)


def _mask(rng, variant):
    """uint32[8]: random bits; variant 0 has bit 0 set, 1 has bit 0 clear, 2 has bit 255 set."""
    m = rng.integers(0, 1 << 32, size=8, dtype=np.uint64).astype(np.uint32)
    if variant % 3 == 0:
        m[0] |= np.uint32(1)
    elif variant % 3 == 1:
        m[0] &= np.uint32(0xFFFFFFFE)
    else:
        m[7] |= np.uint32(0x80000000)
    return m


# ------------------------------------------------------------------------------------------------ decisions
def _cat_left(x, words):
    """``x`` values (any real dtype), ``words`` int64 [..., 8] the mask of each value's node."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        xt = np.trunc(x)
        ok = (x == x) & (xt >= 0) & (xt < 256)
    c = np.where(ok, xt, 0.0).astype(np.int64)
    w = np.take_along_axis(words, (c >> 5)[..., None], axis=-1)[..., 0] if words.ndim > 1 else words[c >> 5]
    return ok & (((w >> (c & 31)) & 1) == 1)


def walk(struct, masks, depth, M, binned=False):
    """Leaf slot [n, T] (per-slot heap index) every row of ``M`` reaches in every tree.  ``M`` fp32 rows [n, d], or
    with ``binned`` integer bins [n, d].  Also the number of (row, node) visits of a NaN at a categorical node whose
    mask has bit 0 set."""
    T, n = struct.shape[0], M.shape[0]
    rows = np.arange(n)
    mk = masks.astype(np.int64).reshape(-1, 8) if len(masks) else np.zeros((1, 8), dtype=np.int64)
    leaf = np.zeros((n, T), dtype=np.int64)
    nan_hits = 0
    for t in range(T):
        idx = np.zeros(n, dtype=np.int64)
        for _ in range(depth):
            code = struct[t, idx, 0].astype(np.int64)
            pay = np.ascontiguousarray(struct[t, idx, 1])
            is_leaf = code == -1
            cat = code <= -2
            f = np.where(is_leaf, 0, np.where(cat, -code - 2, code))
            x = M[rows, f]
            with np.errstate(invalid="ignore"):
                num_left = (x <= pay) if binned else (x.astype(F32) <= pay.view(F32))
            words = mk[np.where(cat, pay, 0)]
            cat_left = _cat_left(x, words)
            if not binned:
                nan_hits += int((cat & (x != x) & ((words[:, 0] & 1) == 1)).sum())
            left = np.where(cat, cat_left, num_left)
            idx = np.where(is_leaf, idx, 2 * idx + np.where(left, 1, 2))
        leaf[:, t] = idx
    return leaf, nan_hits


def reachable(struct_t):
    """(split slots, leaf slots) reachable from the root of one tree's per-slot table."""
    splits, leaves, todo = [], [], [0]
    while todo:
        s = todo.pop()
        if struct_t[s, 0] == -1:
            leaves.append(s)
        else:
            splits.append(s)
            todo += [2 * s + 2, 2 * s + 1]
    return splits, leaves


def assert_coverage(struct, depth, leaf):
    n, T = leaf.shape
    for t in range(T):
        if struct[t, 0, 0] == -1:
            assert (leaf[:, t] == 0).all()
            continue
        s = leaf[:, t].copy()
        for _ in range(depth):
            s = np.where(s > 2, (s - 1) // 2, s)
        if n >= 2:
            assert (s == 1).any() and (s == 2).any(), f"tree {t}: every row goes to one side of the root"
        _, leaves = reachable(struct[t])
        got = np.unique(leaf[:, t])
        assert np.isin(got, leaves).all()
        if n >= 4 * 2 ** depth:
            assert 2 * len(got) >= len(leaves), f"tree {t}: {len(got)} of {len(leaves)} leaves receive a row"


# ------------------------------------------------------------------------------------------------ forests
def _grow(rng, T, depth, M, num_pools, cat_feats, complete, leaf_tree, binned, forced=None):
    """Per-slot forest: struct int32 [T, 2^(depth+1)-1, 2] ({feature | -1 leaf | -(f+2) categorical, fp32 threshold
    bits (bins: the node bin) | mask index}) and the masks uint32 [M, 8].  Tree 0 splits all along its leftmost path, so
    the forest's depth is ``depth``; elsewhere a node below the root is a leaf with probability 1/4 (``complete``:
    never); tree ``leaf_tree``'s root is a leaf.  A split is taken, where a few draws find one, such that the rows at
    the node go to both sides.  ``forced``: {(tree, slot): (feature, "num" | "cat")}."""
    S = 2 ** (depth + 1) - 1
    struct = np.zeros((T, S, 2), dtype=np.int32)
    struct[:, :, 0] = -1
    masks = []
    num_feats = [f for f in sorted(num_pools) if len(num_pools[f])]
    cat_feats = list(cat_feats)
    Mg = M[:GROW_ROWS]
    for t in range(T):
        if t == leaf_tree:
            continue
        todo = [(0, 0, np.arange(Mg.shape[0]))]
        while todo:
            slot, lvl, rows = todo.pop()
            if lvl == depth:
                continue
            spine = t == 0 and slot == 2 ** lvl - 1
            want = (forced or {}).get((t, slot))
            if not complete and not spine and not want and lvl > 0 and rng.random() < 0.25:
                continue
            best = None
            for _ in range(12):
                use_cat = (want[1] == "cat") if want else (bool(cat_feats) and (not num_feats or rng.random() < 0.4))
                if use_cat:
                    f = want[0] if want else cat_feats[rng.integers(len(cat_feats))]
                    m = _mask(rng, len(masks))
                    left = _cat_left(Mg[rows, f], m.astype(np.int64))
                    cand = (f, None, m, left)
                else:
                    f = want[0] if want else num_feats[rng.integers(len(num_feats))]
                    thr = num_pools[f][rng.integers(len(num_pools[f]))]
                    with np.errstate(invalid="ignore"):
                        left = Mg[rows, f] <= thr
                    cand = (f, thr, None, left)
                best = best or cand
                if len(rows) < 2 or (left.any() and not left.all()):
                    best = cand
                    break
            f, thr, m, left = best
            if m is not None:
                struct[t, slot] = (-(f + 2), len(masks))
                masks.append(m)
            else:
                struct[t, slot] = (f, int(thr) if binned else int(F32(thr).view(np.int32)))
            todo.append((2 * slot + 2, lvl + 1, rows[~left]))
            todo.append((2 * slot + 1, lvl + 1, rows[left]))
    masks = np.stack(masks).astype(np.uint32) if masks else np.zeros((0, 8), dtype=np.uint32)
    return struct, masks


def node_table(struct, vals_k, rng):
    """The int4 node table of cdna_tree_predict from the per-slot layout: nodes int32 [N, 4] (numeric {f, thr bits,
    left, right}, categorical {-(f+2), mask index, left, right}, leaf {-1, value offset, 0, 0}), roots int32 [T] and
    values fp64 [leaves * K].  Node ids and leaf value offsets are shuffled over the whole forest, so children are not
    at 2i + 1 and the trees interleave."""
    T, K = struct.shape[0], vals_k.shape[2]
    reach = [(t, s) for t in range(T) for part in reachable(struct[t]) for s in part]
    ids = rng.permutation(len(reach))
    id_of = {ts: int(i) for ts, i in zip(reach, ids)}
    leaves = [ts for ts in reach if struct[ts[0], ts[1], 0] == -1]
    off_of = {ts: int(i) * K for ts, i in zip(leaves, rng.permutation(len(leaves)))}
    nodes = np.zeros((len(reach), 4), dtype=np.int32)
    values = np.zeros(len(leaves) * K, dtype=np.float64)
    for (t, s), i in id_of.items():
        code, pay = struct[t, s]
        if code == -1:
            nodes[i] = (-1, off_of[(t, s)], 0, 0)
            values[off_of[(t, s)]:off_of[(t, s)] + K] = vals_k[t, s]
        else:
            nodes[i] = (code, pay, id_of[(t, 2 * s + 1)], id_of[(t, 2 * s + 2)])
    roots = np.array([id_of[(t, 0)] for t in range(T)], dtype=np.int32)
    return nodes, roots, values


def binned_node_table(struct_t, vals_t, rng):
    """One tree's table for predict_binned_add: nodes int32 [N, 4] with local shuffled ids (numeric {f, bin, l, r}),
    the root's id and the fp32 leaf values."""
    nodes, roots, values = node_table(struct_t[None], vals_t[None, :, None], rng)
    return nodes, int(roots[0]), values.astype(F32)


# ------------------------------------------------------------------------------------------------ sums
def ordered_sum(tw, vals_k, leaf, base):
    """[n, K] fp64 in the kernels' order; ``base`` fp64 [K] or None (0.0)."""
    n, T = leaf.shape
    K = vals_k.shape[2]
    lanes = [np.zeros((n, K), dtype=np.float64) for _ in range(4)]
    for t in range(T):
        prod = np.multiply(np.float64(tw[t]), vals_k[t, leaf[:, t], :])
        lanes[t % 4] = np.add(lanes[t % 4], prod)
    out = np.zeros((n, K), dtype=np.float64) if base is None else np.tile(np.asarray(base, np.float64), (n, 1))
    for q in range(4):
        out = np.add(out, lanes[q])
    return out


def exact_sum(tw, vals_k, leaf, base, rows):
    """(sum, sum of magnitudes) [len(rows), K] of the same terms -- base and the rounded products fl64(tw[t] * v) --
    added exactly (math.fsum)."""
    T, K = leaf.shape[1], vals_k.shape[2]
    out = np.zeros((len(rows), K))
    mag = np.zeros((len(rows), K))
    for i, r in enumerate(rows):
        for k in range(K):
            terms = [float(np.float64(tw[t]) * vals_k[t, leaf[r, t], k]) for t in range(T)]
            if base is not None:
                terms.append(float(base[k]))
            out[i, k] = math.fsum(terms)
            mag[i, k] = math.fsum(abs(v) for v in terms)
    return out, mag


# ------------------------------------------------------------------------------------------------ cases
def _thresholds(rng, d, bup):
    """Sorted fp32 threshold table [d, tmax] and nthr [d] of a binned case: feature 0 regular with 0.0 among its
    thresholds, then by feature index a table of none, of one, one with a duplicated threshold, a full one
    (nthr = Bup - 1), the rest of random lengths."""
    tmax = bup - 1
    thr = np.zeros((d, max(tmax, 1)), dtype=F32)
    nthr = np.zeros(d, dtype=np.int32)
    for f in range(d):
        k = [min(7, tmax), 0, 1, min(5, tmax), tmax][f] if f < 5 else int(rng.integers(1, min(9, tmax) + 1))
        v = rng.permutation(np.unique(rng.normal(size=4 * k + 4).astype(F32)))[:k]
        if f == 0:
            v[0] = 0.0
        if f == 3 and k >= 2:
            v[1] = v[0]
        thr[f, :k] = np.sort(v)
        nthr[f] = k
    return thr, nthr


@functools.lru_cache(maxsize=None)
def case(T, depth, d, K=1, seed=0, n=200, cats=(), complete=False, bup=0):
    """One forest with its rows, leaf slots and expected sums.  ``cats``: the categorical features.  ``bup`` > 0: a
    numeric forest over binned features -- thresholds [d, bup - 1] / nthr, the rows' bins [G, n, 8] and thr_up
    [d, bup]; every split threshold is one of its feature's thresholds."""
    rng = np.random.default_rng([seed, T, depth, d, K, n, bup])
    if bup:
        assert not cats
        thr, nthr = _thresholds(rng, d, bup)
        pools = {f: thr[f, :nthr[f]] for f in range(d)}
    else:
        pools = {f: np.unique(np.append(rng.normal(size=6).astype(F32), F32(0.0))[:7 if f == 0 else 6])
                 for f in range(d) if f not in cats}
    X = np.empty((n, d), dtype=F32)
    for f in range(d):
        X[:, f] = _cat_column(rng, n) if f in cats else _numeric_column(rng, n, pools[f], f == 0)
    leaf_tree = 1 if (T >= 3 and depth >= 1 and not complete) else -1
    # with categorical features tree 0's root tests the first of them against mask 0, whose bit 0 is set: every NaN
    # category meets it
    forced = {(0, 0): (cats[0], "cat")} if cats and depth >= 1 else None
    struct, masks = _grow(rng, T, depth, X, pools, cats, complete, leaf_tree, False, forced)
    S = struct.shape[1]
    vals_k = rng.normal(size=(T, S, K))
    tw = rng.uniform(0.5, 1.5, size=T)
    base = rng.normal(size=K)
    leaf, nan_hits = walk(struct, masks, depth, X)
    assert_coverage(struct, depth, leaf)
    assert max(len(reachable(struct[t])[0]) for t in range(T)) >= depth      # tree 0 is as deep as the heap
    c = SimpleNamespace(T=T, depth=depth, d=d, K=K, n=n, X=X, struct=struct, masks=masks, vals_k=vals_k,
                        vals=np.ascontiguousarray(vals_k[:, :, 0]), tw=tw, base=base, leaf=leaf,
                        nan_cat_hits=nan_hits, seed=seed)
    c.ref = ordered_sum(tw, vals_k, leaf, base)
    c.ref_nobase = ordered_sum(tw, vals_k, leaf, None)
    c.nodes, c.roots, c.values = node_table(struct, vals_k, rng)
    if cats:
        assert nan_hits > 0 or n < 64, "no NaN category meets a mask with bit 0 set"
    if bup:
        for t in range(T):       # the binned kernel's precondition
            for s in reachable(struct[t])[0]:
                f = struct[t, s, 0]
                assert struct[t, s:s + 1, 1].view(F32)[0] in thr[f, :nthr[f]]
        G = (d + 7) // 8
        b = np.zeros((n, 8 * G), dtype=np.uint8)
        for f in range(d):
            cnt = np.searchsorted(thr[f, :nthr[f]], X[:, f], side="left")     # #{t_j < x}
            b[:, f] = np.where(np.isnan(X[:, f]), nthr[f], cnt)
        c.bins = np.ascontiguousarray(b.reshape(n, G, 8).transpose(1, 0, 2))
        c.thr_up = np.full((d, bup), np.inf, dtype=F32)
        for f in range(d):
            c.thr_up[f, :nthr[f]] = thr[f, :nthr[f]]
        c.thr, c.nthr, c.G, c.bup = thr, nthr, G, bup
    return c


@functools.lru_cache(maxsize=None)
def binned_add_case(n, G, seed=0, T=3, depth=4, exact=True):
    """Trees that split on bins, for predict_binned_add: bins uint8 [G, n, 8] over all of 0..255, numeric and
    categorical splits (with G >= 2 on features 7 and 8: the last byte of a word and the first of the next), per-tree
    node tables, ``out0`` and the expected ``out``.  ``exact``: distinct small integer leaf values, integer out0 and
    scale 1, so the fp32 result is exact; else random fp32 values and scale fp32(0.3) with the result in fp64."""
    rng = np.random.default_rng([seed, n, G, T, depth, int(exact)])
    d = 8 * G
    b = rng.integers(0, 256, size=(n, d), dtype=np.int64)
    kind = rng.integers(0, 10, size=(n, d))
    b = np.where(kind == 0, 0, np.where(kind == 1, 255, b))
    pools = {f: np.unique(b[:GROW_ROWS, f])[:-1] if len(np.unique(b[:GROW_ROWS, f])) > 1 else b[:1, f]
             for f in range(d)}
    forced = {}
    if G >= 2:
        forced = {(0, 0): (7, "num"), (0, 1): (8, "cat"), (0, 2): (8, "num"),
                  (2, 0): (7, "cat"), (2, 1): (8, "num"), (2, 2): (8, "cat")}
    struct, masks = _grow(rng, T, depth, b, pools, range(d), False, -1, True, forced)
    S = struct.shape[1]
    if exact:
        vals = (np.arange(T * S, dtype=np.float64).reshape(T, S) % 4001) + 1.0     # distinct within a tree
        out0 = rng.integers(-50, 50, size=n).astype(F32)
        scale = 1.0
    else:
        vals = rng.normal(size=(T, S)).astype(F32).astype(np.float64)
        out0 = rng.normal(size=n).astype(F32)
        scale = float(F32(0.3))
    leaf, _ = walk(struct, masks, depth, b, binned=True)
    assert_coverage(struct, depth, leaf)
    c = SimpleNamespace(n=n, G=G, T=T, depth=depth, struct=struct, masks=masks, vals=vals, out0=out0, scale=scale,
                        leaf=leaf, bins=np.ascontiguousarray(b.astype(np.uint8).reshape(n, G, 8).transpose(1, 0, 2)))
    c.tables = [binned_node_table(struct[t], vals[t], rng) for t in range(T)]
    c.picked = np.stack([vals[t, leaf[:, t]] for t in range(T)], 1)      # [n, T] the leaf value of each tree
    used = {int(f if f >= 0 else -f - 2) for t in range(T) for f in struct[t, reachable(struct[t])[0], 0]}
    if G >= 2:
        assert {7, 8} <= used
    return c


def binned_add_bound(c, got):
    """|got - fl64(out0 + scale v)| <= 2^-24 (|scale v| + |result|): the rounding of the product and of the sum, or
    the one rounding of a fused multiply-add."""
    sv = np.float64(c.scale) * c.picked[:, 0]
    want = c.out0.astype(np.float64) + sv
    return np.abs(got.astype(np.float64) - want), 2.0 ** -24 * (np.abs(sv) + np.abs(want))


def gains(min_gain):
    return (min_gain, np.nan, np.inf, -np.inf, 0.0, -1.0, np.nextafter(min_gain, 0.0), 1e6)


def node_weights(min_w):
    return (min_w, np.nextafter(min_w, 0.0), 1e3)


@functools.lru_cache(maxsize=None)
def last_level_case(D, A, sw, seed=0, min_gain=0.25, min_w=2.0):
    """Inputs of heap_last_level and the heap it must leave.  The A active nodes are distinct (tree, key) pairs of the
    level 2^(D-1) <= key < 2^D, its first and its last key among them.  Gains cycle through gains(), node weights
    through node_weights(): 8 x 3 combinations; node 0 has gain == min_gain and weight == min_w and splits.  Either
    child's W is 0 for some nodes.  The heap holds a recognisable pattern.  The rule of trees.hip: a node splits iff
    its gain is finite, > 0 and >= min_gain and its weight >= min_w; it then gets slot key - 1 = (feature, fp32
    threshold bits) and the leaves S / W (0.0 when W <= 0) at 2 key - 2^D and 2 key + 1 - 2^D."""
    rng = np.random.default_rng([seed, D, A, sw])
    lo, hi = 1 << (D - 1), 1 << D
    T = -(-A // (hi - lo)) + 1
    d, Bt = 9, 17
    NI = hi - 1
    pairs = [(t, k) for t in range(T) for k in range(lo, hi)]
    pick = [pairs[i] for i in rng.permutation(len(pairs))[:A]]
    if A >= 2:
        pick[0], pick[-1] = (0, lo), (T - 1, hi - 1)
        pick = list(dict.fromkeys(pick))
        while len(pick) < A:                      # a replaced pair was drawn twice: refill with unused pairs
            pick.append(next(p for p in pairs if p not in pick))
    a_tree = np.array([p[0] for p in pick], dtype=np.int32)
    a_key = np.array([p[1] for p in pick], dtype=np.int32)
    gs, ws = gains(min_gain), node_weights(min_w)
    so = rng.normal(size=(A, sw)) * 5
    so[:, 0] = [gs[i % 8] for i in range(A)]
    so[:, 1] = rng.integers(0, d, size=A)
    so[:, 2] = rng.integers(0, Bt, size=A)
    so[:, 3] = [(3.0, 0.0, 2.5, 1.0, 7.0)[i % 5] for i in range(A)]
    so[:, 5] = [(4.0, 1.5, 6.0, 0.0, 2.0, 9.0, 0.5)[i % 7] for i in range(A)]
    a_w = np.array([ws[i % 3] for i in range(A)], dtype=np.float64)
    thr = rng.normal(size=(d, Bt)).astype(F32)
    heap = (np.arange(T * (4 * NI + 2), dtype=np.int64) * 7919 + 12345).astype(np.int32).reshape(T, 4 * NI + 2)
    want = heap.copy()
    n_split = 0
    for a in range(A):
        g = so[a, 0]
        if not (np.isfinite(g) and g > 0.0 and g >= min_gain and a_w[a] >= min_w):
            continue
        n_split += 1
        t, k = int(a_tree[a]), int(a_key[a])
        f, b = int(so[a, 1]), int(so[a, 2])
        want[t, 2 * (k - 1)] = f
        want[t, 2 * (k - 1) + 1] = thr[f, b:b + 1].view(np.int32)[0]
        for side in (0, 1):
            W, S_ = so[a, 3 + 2 * side], so[a, 4 + 2 * side]
            v = np.array([np.float64(S_) / np.float64(W) if W > 0.0 else 0.0], dtype=np.float64)
            j = 2 * NI + 2 * (2 * k + side - hi)
            want[t, j:j + 2] = v.view(np.int32)
    assert n_split > 0
    return SimpleNamespace(D=D, A=A, sw=sw, T=T, so=so, a_tree=a_tree, a_key=a_key, a_w=a_w, thr=thr, heap=heap,
                           want=want, min_gain=min_gain, min_w=min_w, n_split=n_split)


# ------------------------------------------------------------------------------------------------ shape tables
SMALL_N = (1, 63, 64, 65, 200)       # one row, a tile less one, a tile, a tile and one row, four tiles with a tail
CATS = (2, 5)                        # the categorical features of the raw-feature cases (d >= 12)
# predict_kernel: (name, d, staging K.tree_predict_plan must report).  "view": columns 3..14 of a 20-column matrix
# (ldx != d); "offset": a contiguous matrix that starts 4 bytes past a 16-byte boundary
NODE_STAGING = (("d12", 12, "float4+prefetch"), ("d128", 128, "float4+prefetch"), ("d132", 132, "float4"),
                ("d17", 17, "scalar"), ("view", 12, "scalar"), ("offset", 12, "scalar"))
# predict_heap_kernel has no float4 loop without the prefetch: d = 132 stages by scalars
HEAP_STAGING = (("d12", 12, "float4+prefetch"), ("d17", 17, "scalar"), ("d132", 132, "scalar"),
                ("view", 12, "scalar"), ("offset", 12, "scalar"))
NODE_T = (1, 3, 4, 5, 33, 37)        # lanes without a tree, one tree per lane, a second round of 32 (tb += 4 W)
HEAP_T = (1, 3, 5, 33, 64)
HEAP_DEPTHS = ((1, 5), (8, 9), (11, 1))             # (depth, T) that fit the LDS budget
HEAP_OVER = ((11, 2), (12, 1))                      # (depth, T) over it
BINNED_T_ONE_PASS = (1, 4, 5, 9, 13, 17, 21, 25, 29)    # NT = ceil(T / 4) = 1, 1, 2 .. 8
BINNED_T_TWO_PASS = (33, 35, 64)                    # NT = 8, two passes, tree indices past T clamped to T - 1
BINNED_D = ((1, 1, True), (8, 1, True), (9, 2, True), (128, 16, True), (130, 17, False))   # (d, G, prefetch)
BINNED_DEPTHS = (1, 5, 8)
BINNED_BUP = (2, 40, 256)
BINNED_ADD = ((1, 1), (257, 1), (257, 2))           # (n, G); BIG_N_BINNED_ADD with G = 1 on the GPU only
LAST_LEVEL = tuple((D, A, sw) for D in (1, 5) for A in (1, 256, 257, 600) for sw in (7, 12))
