"""Exact references for the level histograms (hist4.hip node ids, hist5.hip row codes; tests/test_hist_block_*.py).

The method of the Gram tests: labels, v0 and weights are small integers (|v1| <= 1000, v0 in 0..15, weights 0..3 with
a few rows at 255), so every fixed-point scale the wrappers pick is a power of two >= 1, quantisation is lossless and
every kernel must return the int64 sums of ``ref_hist`` bit for bit.  ``ref_hist`` is a numpy loop over (tree, feature)
with ``np.add.at`` over the rows; it shares nothing with ``K.hist_moments`` / ``K.hist_classes``.

A level is built once per (shape, T, per, wide) and shared, unchanged, by every test that uses it."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

# (n, d, B): three row trips of a 512-thread block plus a partial one, last feature group with 5 valid features |
# one feature group, 256 bins | two trips of a 1024-thread block plus a partial one, 13 feature groups
SHAPES = {"a": (1543, 21, 40), "b": (1031, 5, 256), "c": (2055, 100, 40)}
C = 3
NT_BUCKETS = (1, 2, 4, 8, 16)


@functools.lru_cache(maxsize=None)
def level(shape: str, T: int, per: int, wide: bool = False):
    """One tree level: T trees of ``per`` active nodes each (tree-major ids), as node ids + weights (hist4) and as
    row codes (hist5).  Every (tree, row) is done (-1 / 0xFF) with probability 0.1; weight-0 rows keep a valid node
    id (the node-id kernels must skip them) and are done in the codes (as ``codes_init`` makes them).  ``wide``: most
    ids are not built (few slots over a long id range; node ids only, per may pass 255)."""
    n, d, B = SHAPES[shape]
    rng = np.random.default_rng(1000 * T + per + (7 if wide else 0) + n)
    G = (d + 7) // 8
    binm = rng.integers(0, B, (n, d), dtype=np.int64)
    bins = np.zeros((G, n, 8), dtype=np.uint8)
    for f in range(d):
        bins[f // 8, :, f % 8] = binm[:, f]
    A = T * per
    if wide:
        built = np.arange(A) % (A // 8) == 3
    else:
        built = rng.random(A) < 0.6
        built[rng.integers(0, per, T) + np.arange(T) * per] = True  # every tree builds a node
    build = np.where(built, np.cumsum(built) - 1, -1).astype(np.int32)
    id_tree = (np.arange(A) // per).astype(np.int32)
    slot_tree = id_tree[built]
    if wide:  # half of the rows sit on a built id
        bid = np.flatnonzero(built).reshape(T, -1) - (np.arange(T) * per)[:, None]
        loc = np.where(rng.random((T, n)) < 0.5, bid[np.arange(T)[:, None], rng.integers(0, bid.shape[1], (T, n))],
                       rng.integers(0, per, (T, n)))
    else:
        loc = rng.integers(0, per, (T, n))
    done = rng.random((T, n)) < 0.1
    w = rng.integers(0, 4, (T, n))
    w[rng.random((T, n)) < 0.01] = 255
    ids = loc + (np.arange(T) * per)[:, None]
    node = np.where(done, -1, ids).astype(np.int32)
    lv = SimpleNamespace(shape=shape, wide=wide, n=n, d=d, B=B, T=T, per=per, A=A, S=int(built.sum()), binm=binm,
                         bins=torch.from_numpy(bins), build=torch.from_numpy(build), slot_tree=slot_tree,
                         id_tree=id_tree, node=torch.from_numpy(node), weight=torch.from_numpy(w.astype(np.uint8)),
                         tfirst=torch.arange(T, dtype=torch.int32) * per)
    lv.ids, lv.w, lv.live = ids, w, ~done & (w > 0)
    if per < 255:
        code = (w << 8) | np.where(done | (w == 0), 0xFF, loc)
        lv.codes = torch.from_numpy(code.astype(np.uint16).view(np.int16)).contiguous()
    lv.v1 = torch.from_numpy(rng.integers(-1000, 1001, n).astype(np.float32))
    lv.v0 = torch.from_numpy(rng.integers(0, 16, n).astype(np.float32))
    lv.label = torch.from_numpy(rng.integers(-1, C + 1, n).astype(np.int32))  # -1 and C: rows without a class
    mw = (d + 31) // 32
    lv.fmask = torch.from_numpy(rng.integers(0, 2 ** 32, (lv.S, mw), dtype=np.uint64).astype(np.uint32).view(np.int32))
    return lv


@functools.lru_cache(maxsize=None)
def _ref(shape, T, per, wide, kind, masked):
    lv = level(shape, T, per, wide)
    K_ = C if kind == "classes" else 2
    out = np.zeros((lv.S, lv.d, lv.B, K_), dtype=np.int64)
    build = lv.build.numpy()
    fm = lv.fmask.numpy().view(np.uint32)
    v0 = lv.v0.numpy().astype(np.int64) if kind == "v0" else np.ones(lv.n, dtype=np.int64)
    v1 = lv.v1.numpy().astype(np.int64)
    lab = lv.label.numpy()
    for t in range(lv.T):
        slot = build[lv.ids[t]]
        ok = lv.live[t] & (slot >= 0)
        if kind == "classes":
            ok &= (lab >= 0) & (lab < C)
        w = lv.w[t].astype(np.int64)
        for f in range(lv.d):
            m = ok.copy()
            if masked:
                m[ok] = ((fm[slot[ok], f // 32] >> np.uint32(f % 32)) & 1).astype(bool)
            s, b = slot[m], lv.binm[m, f]
            if kind == "classes":
                np.add.at(out, (s, f, b, lab[m]), w[m])
            else:
                np.add.at(out, (s, f, b, 0), w[m] * v0[m])
                np.add.at(out, (s, f, b, 1), w[m] * v1[m])
    return torch.from_numpy(out).double()


def ref_hist(lv, kind: str, masked: bool) -> torch.Tensor:
    """The level's histogram [S, d, B, K] as float64 of exact int64 sums.  kind: "moments" (count, sum w v1), "v0"
    (sum w v0, sum w v1) or "classes" (K = C weighted class counts).  Shared: do not modify."""
    return _ref(lv.shape, lv.T, lv.per, lv.wide, kind, masked)


def bytes_per_bin(kind: str) -> int:
    """LDS bytes per (slot, feature, bin) the planners count: u32 count + u64 sum, two u64 sums, or C u32 counts."""
    return {"moments": 12, "v0": 16, "classes": 4 * C}[kind]


def brute_groups(slot_tree, id_tree, SB, max_trees=None):
    """Slot groups by brute force: a group takes slots one by one while it holds fewer than SB and the slot's tree is
    within max_trees of the group's first; its id range is every id of the group's first to last tree."""
    rows, a, S = [], 0, len(slot_tree)
    while a < S:
        b = a
        while b < S and b - a < SB and (max_trees is None or slot_tree[b] - slot_tree[a] < max_trees):
            b += 1
        t0, t1 = int(slot_tree[a]), int(slot_tree[b - 1])
        inside = [i for i, t in enumerate(id_tree) if t0 <= t <= t1]
        rows.append((a, t0, t1, inside[0], inside[-1] + 1))
        a = b
    return rows


def code_plan(K, lv, kind: str, budget: int, packed: bool, maxt: int = 16):
    """(SB, rows, largest trees per group, its bucket, 1024-thread blocks) of K.hist_codes for this level: the
    wrapper's planning from the documented LDS sizes, through K.slot_groups."""
    per_slot = 8 * lv.B * bytes_per_bin(kind)
    SB = max(1, min(lv.S, min(budget, 16384 * 8) // per_slot if packed else budget // per_slot))
    rows = K.slot_groups(lv.slot_tree, lv.id_tree, SB, maxt)
    SB = max((rows[i + 1][0] if i + 1 < len(rows) else lv.S) - rows[i][0] for i in range(len(rows)))
    nt = max(r[2] - r[1] + 1 for r in rows)
    return SB, rows, nt, next(b for b in NT_BUCKETS if nt <= b), packed and SB * per_slot > 8192 * 8
