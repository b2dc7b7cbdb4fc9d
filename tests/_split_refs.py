"""Independent references and cases for the split-search and split-decode kernels (csrc/kernels/split.hip:
split_scan_kernel, split_scan_wave_kernel, split_scan_ex_kernel, split_decode_kernel).

Plain numpy on the CPU, nothing from ``cdnaml``.  The references restate the contract of split.hip's comments in fp64,
one rounded operation per arithmetic step and in the documented order, so a kernel is compared with ``==``:

* node totals: the per-bin sequential sum of the first feature with the largest weight;
* candidates in key order -- every (feature, bin) with the missing rows (bin 0) on the left, then every (feature,
  bin >= 1) with them on the right -- and the first strictly larger finite gain wins, i.e. ties go to the lowest key
  ``f * B + b`` (+ ``d * B`` for missing-right), torch.argmax's order over the concatenated gains;
* variance gain ``(SL^2 / WL + SR^2 / WR - St^2 / Wt) / Wt`` with every weight clamped at 1e-300, legal when both sides
  weigh at least ``max(min_inst, 1e-12)``; XGBoost gain ``0.5 (GL^2 / (HL + lam) + GR^2 / (HR + lam) - Gt^2 /
  (Ht + lam)) - gamma``, legal when both hessians are positive and at least ``min_child_weight``;
* Gini / entropy gain ``imp(t) - WL / Wt imp(l) - WR / Wt imp(r)`` on class counts, classes added left to right and
  every product rounded before it is added;
* categorical features (``nthr < 0``): bins ordered stably by centroid (mean label, P(class 1) for two classes, the
  bin's impurity for more; empty bins last), positions ``j < (#non-empty) - 1``, left set = the first ``j + 1``
  categories, returned as a 256-bit mask;
* the decode of a level's decisions into partition tables (split.hip's split_decode comment block).

``case_hist`` builds histograms from synthetic rows -- every row of a node falls into one bin of every feature, so every
feature of a node has the same totals -- with integer weights and sums that are integers times 2^-14: every partial
sum is exact, as the histograms of every record / codes path are.
"""
import functools
from types import SimpleNamespace

import numpy as np

INF = float("inf")
Q14 = 2.0 ** -14
KINDS_EX = {"variance": 0, "gini": 2, "entropy": 3}


def nthr_edges(B):
    """Threshold counts at the edges: no legal threshold (-1, 0), one, all but the last bin, every bin, past the end."""
    return (-1, 0, 1, B - 1, B, B + 5)


# ------------------------------------------------------------------------------------------------ small helpers
def mask_words(bits):
    """bool [A, d] -> uint32 [A, ceil(d / 32)] feature-subset words (bit f & 31 of word f >> 5)."""
    A, d = bits.shape
    w = np.zeros((A, (d + 31) // 32), dtype=np.uint32)
    for f in range(d):
        w[:, f >> 5] |= bits[:, f].astype(np.uint32) << np.uint32(f & 31)
    return w


def mask_bit(mask, a, f):
    return mask is None or bool((int(mask[a, f >> 5]) >> (f & 31)) & 1)


def bin_set(bins):
    """uint32[8]: the 256-bit set of ``bins``."""
    m = np.zeros(8, dtype=np.uint32)
    for b in bins:
        m[int(b) >> 5] |= np.uint32(1) << np.uint32(int(b) & 31)
    return m


def _seq_sum(x):
    """Left-to-right sum of a 1-d array from 0.0, one rounding per add."""
    return float(np.cumsum(x)[-1]) if len(x) else 0.0


# ------------------------------------------------------------------------------------------------ histograms
def _roles(A, masked):
    """Special nodes of a case: one without rows, one with all rows in one bin, one whose mask leaves only features
    without a legal threshold."""
    zero = A - 1 if A >= 3 else -1
    onebin = A - 2 if A >= 4 else -1
    illegal = A - 3 if (A >= 5 and masked) else -1
    return zero, onebin, illegal


def cat_order(hf, K, kind):
    """Stable centroid order of a categorical feature's bins hf [B, K] -> (order, number of non-empty bins)."""
    with np.errstate(all="ignore"):
        if kind == 0:
            W = hf[:, 0].copy()
            c = hf[:, 1] / np.maximum(W, 1e-300)
        else:
            W = np.zeros(hf.shape[0])
            for i in range(K):
                W = W + hf[:, i]
            c = hf[:, 1] / np.maximum(W, 1e-300) if K == 2 else impurity(hf, kind)
    cent = np.where(W > 0, c, INF)
    return np.argsort(cent, kind="stable"), int((cent != INF).sum()), cent


def case_hist(A, d, B, K=0, seed=0, rows=None, empty=0.3, missing=False, masked=False, cats=None, twin_cat=None,
              general=False, ex=False):
    """Histograms of ``A`` nodes from synthetic rows.

    K = 0: two statistics (weight or hessian: integers 1..3 per row; sum or gradient: integers times 2^-14);
    K >= 2: class counts.  ``ex``: the layout split_scan_ex reads (K = 0 means variance with two statistics).
    Features: 1 is copied to 2 and to 129 (a tie across the serial kernel's threads and inside one thread's walk);
    ``missing``: odd nodes have no row in bin 0 (every missing-right candidate ties its left twin), and feature 128 is
    feature 0 with its bin-0 rows moved to the last bin (its missing-left candidates tie feature 0's missing-right
    ones); ``cats`` {feature: cardinality}: categorical features (nthr -1); ``twin_cat`` (fc, fn): numeric feature fn
    holds categorical fc's bins in centroid order, so position j of fc and bin j of fn have equal gains.
    Even nodes' labels follow feature 0 (``twin_cat``: the categorical fc), odd nodes' feature 1.
    ``masked``: feature-subset words; half of the masked-off features are zeroed as a forest's histograms are.
    ``general``: every cell times a random factor -- inexact sums, features with different totals.
    """
    rng = np.random.default_rng(seed)
    cats = dict(cats or {})
    ks = K if K else 2
    zero, onebin, illegal = _roles(A, masked)
    # legal thresholds
    nthr = rng.integers(max(1, B // 2), B + 1, size=d).astype(np.int32)
    nthr[0] = min(B, (B // 2 + 1) | 1)           # odd: cuts inside a lane's bin group of the wave kernel
    if d > 1:
        nthr[1] = max(1, B - 1)
    if d >= 8:
        edges = [e for e in nthr_edges(B) if not (ex and e < 0)]   # (split_scan_ex: -1 means categorical)
        for f in range(4, d, 5):
            nthr[f] = edges[(f // 5) % len(edges)]
    for f in cats:
        nthr[f] = -1
    dups = [(1, t) for t in (2, 129) if t < d]
    for s, t in dups:
        nthr[t] = nthr[s]
    twin_miss = (0, 128) if (missing and d > 128) else None
    if twin_miss:
        nthr[128] = nthr[0] = B - 1
    if twin_cat:
        nthr[twin_cat[1]] = B
    Hi = np.zeros((A, d, B, ks), dtype=np.int64)
    for a in range(A):
        if a == zero:
            continue
        n = int(rows) if rows else int(rng.integers(B + 2, 4 * B + 8))
        bins = np.zeros((n, d), dtype=np.int64)
        for f in range(d):
            hi = cats.get(f, B)
            ok = rng.random(hi) >= empty
            if missing and f not in cats:
                ok[0] = a % 2 == 0
            allowed = np.nonzero(ok)[0]
            if a == onebin:
                allowed = np.array([int(rng.integers(0, hi))])
            elif len(allowed) < min(2, hi):
                allowed = np.arange(min(2, hi))
            bins[:, f] = allowed[rng.integers(0, len(allowed), size=n)]
        pf = (twin_cat[0] if twin_cat else 0) if a % 2 == 0 else min(1, d - 1)
        pb = bins[:, pf]
        if pf in cats:
            side = rng.permutation(B)[pb] % 4          # a category's level: unrelated to its index
        else:
            side = (pb > B // 2).astype(np.int64) * 3
            if missing and pf == 0:
                side = np.where(pb == 0, 3, side)       # missing rows behave like the high bins: missing-right wins
        if K:
            cls = np.where(rng.random(n) < 0.75, side * max(1, K // 4) % K, rng.integers(0, K, size=n))
            for f in range(d):
                np.add.at(Hi[a, f], (bins[:, f], cls), 1)
        else:
            w = rng.integers(1, 4, size=n)
            few = a % 4 >= 2                             # few label levels: tied category centroids
            noise = rng.integers(-2, 3, size=n) << 13 if few else rng.integers(-(1 << 15), 1 << 15, size=n)
            v = ((side - 1) << 16) + noise
            for f in range(d):
                np.add.at(Hi[a, f, :, 0], bins[:, f], w)
                np.add.at(Hi[a, f, :, 1], bins[:, f], v)
    for s, t in dups:
        Hi[:, t] = Hi[:, s]
    if twin_miss:
        s, t = twin_miss
        Hi[:, t] = Hi[:, s]
        Hi[:, t, B - 1] += Hi[:, s, 0]
        Hi[:, t, 0] = 0
    H = Hi.astype(np.float64)
    if not K:
        H[..., 1] *= Q14
    if twin_cat:
        fc, fn = twin_cat
        for a in range(A):
            order = cat_order(H[a, fc], ks, KINDS_EX[ex] if ex else 0)[0]
            H[a, fn] = H[a, fc][order]
    mask = None
    if masked:
        bits = rng.random((A, d)) < 0.5
        bits[0, [f for f in (0, 1, 128) if f < d]] = True
        if cats:
            bits[0, max(cats)] = False                    # a categorical feature that is masked off, content kept
        if illegal >= 0:
            bits[illegal] = nthr <= 0
            assert bits[illegal].any()
        mask = mask_words(bits)
        off = ~bits & (rng.random((A, d)) < 0.5)
        H[off] = 0.0
    if general:
        H = H * (1.0 + rng.random(H.shape))
    return SimpleNamespace(A=A, d=d, B=B, K=K, H=np.ascontiguousarray(H), nthr=nthr, mask=mask, cats=cats,
                           dups=dups, twin_miss=twin_miss, twin_cat=twin_cat, zero=zero, onebin=onebin,
                           illegal=illegal, missing=missing, general=general)


# ------------------------------------------------------------------------------------------------ K6 (two statistics)
def _totals2(Hn):
    """Node totals of Hn [d, B, 2]: the bins of the first feature with the largest weight, added left to right."""
    best, t = None, (0.0, 0.0)
    for f in range(Hn.shape[0]):
        w = _seq_sum(Hn[f, :, 0])
        if best is None or w > best:
            best, t = w, (w, _seq_sum(Hn[f, :, 1]))
    return t


def _gain2(kind, l0, l1, t0, t1, min_inst, lam, gamma, mcw):
    """(gain, legal) of the left statistics l0 / l1 (arrays over a feature's bins); right = total - left."""
    r0, r1 = t0 - l0, t1 - l1
    t0, t1 = np.float64(t0), np.float64(t1)
    if kind == 0:
        lo = max(min_inst, 1e-12)
        ok = (l0 >= lo) & (r0 >= lo)
        wt = max(t0, 1e-300)
        g = (l1 * l1 / np.maximum(l0, 1e-300) + r1 * r1 / np.maximum(r0, 1e-300) - t1 * t1 / wt) / wt
    else:
        ok = (l0 >= mcw) & (r0 >= mcw) & (l0 > 0.0) & (r0 > 0.0)
        g = 0.5 * (l1 * l1 / (l0 + lam) + r1 * r1 / (r0 + lam) - t1 * t1 / (t0 + lam)) - gamma
    return g, ok & np.isfinite(g)


def ref_split_scan(H, nthr, mask, kind, missing_bin=False, min_inst=1.0, lam=1.0, gamma=0.0, mcw=1.0):
    """-> out [A, 8] (gain, feature, bin, left0, left1, right0, right1, missing-right), tot [A, 2]."""
    A, d, B, _ = H.shape
    out, tot = np.zeros((A, 8)), np.zeros((A, 2))
    with np.errstate(all="ignore"):
        for a in range(A):
            t0, t1 = _totals2(H[a])
            tot[a] = t0, t1
            best, win = -INF, None
            for side in ((0, 1) if missing_bin else (0,)):
                for f in range(d):
                    lim = min(max(int(nthr[f]), 0), B)
                    if lim == 0 or not mask_bit(mask, a, f):
                        continue
                    l0, l1 = np.cumsum(H[a, f, :lim, 0]), np.cumsum(H[a, f, :lim, 1])
                    if side:
                        l0, l1 = l0 - H[a, f, 0, 0], l1 - H[a, f, 0, 1]
                    g, ok = _gain2(kind, l0, l1, t0, t1, min_inst, lam, gamma, mcw)
                    gl, okl = g.tolist(), ok.tolist()
                    for b in range(side, lim):
                        if okl[b] and gl[b] > best:
                            best, win = gl[b], (f, b, l0[b], l1[b], side)
            if win is None:
                out[a] = -INF, 0, 0, 0, 0, t0, t1, 0
            else:
                f, b, w0, w1, side = win
                out[a] = best, f, b, w0, w1, t0 - w0, t1 - w1, side
    return out, tot


# ------------------------------------------------------------------------------------------------ K6 (classes, categories)
def impurity(c, kind):
    """Gini (2) / entropy (3) of class counts c [n, K]: classes left to right, every product rounded first."""
    n, K = c.shape
    W = np.zeros(n)
    for i in range(K):
        W = W + c[:, i]
    Wc = np.maximum(W, 1e-300)
    s = np.zeros(n)
    for i in range(K):
        p = c[:, i] / Wc
        if kind == 2:
            s = s + p * p
        else:
            s = s + p * np.where(p > 0.0, np.log2(np.maximum(p, 1e-300)), 0.0)
    return 1.0 - s if kind == 2 else -s


def _gain_ex(kind, L, t, imp_t, min_inst):
    """(gain, legal) of left statistics L [n, K] against the node totals t [K]."""
    R = t[None, :] - L
    lo = max(min_inst, 1e-12)
    if kind == 0:
        g, ok = _gain2(0, L[:, 0], L[:, 1], t[0], t[1], min_inst, 0.0, 0.0, 0.0)
        return g, ok
    K = len(t)
    WL, WR, Wt = np.zeros(len(L)), np.zeros(len(L)), np.float64(0.0)
    for i in range(K):
        WL, WR, Wt = WL + L[:, i], WR + R[:, i], Wt + t[i]
    g = imp_t - WL / Wt * impurity(L, kind) - WR / Wt * impurity(R, kind)
    return g, (WL >= lo) & (WR >= lo) & np.isfinite(g)


def ref_split_scan_ex(H, nthr, mask, kind, min_inst=1.0, gaps=None):
    """-> out [A, 4 + 2K] (gain, feature, position, 0, left[K], right[K]), tot [A, K], cat uint32 [A, 8].
    ``gaps`` (a list): per node, best gain minus the next distinct legal gain (inf with fewer than two)."""
    kd = KINDS_EX[kind]
    A, d, B, K = H.shape
    out, tot, cat = np.zeros((A, 4 + 2 * K)), np.zeros((A, K)), np.zeros((A, 8), dtype=np.uint32)
    with np.errstate(all="ignore"):
        for a in range(A):
            bw, tf = None, 0
            for f in range(d):
                if kd == 0:
                    w = _seq_sum(H[a, f, :, 0])
                else:
                    wb = np.zeros(B)
                    for i in range(K):
                        wb = wb + H[a, f, :, i]
                    w = _seq_sum(wb)
                if bw is None or w > bw:
                    bw, tf = w, f
            t = np.array([_seq_sum(H[a, tf, :, i]) for i in range(K)])
            tot[a] = t
            imp_t = 0.0 if kd == 0 else impurity(t[None, :], kd)[0]
            best, win, seen = -INF, None, []
            for f in range(d):
                if not mask_bit(mask, a, f):
                    continue
                if nthr[f] < 0:
                    order, ncnt, _ = cat_order(H[a, f], K, kd)
                    lim = max(min(B, ncnt - 1), 0)
                else:
                    order, lim = np.arange(B), min(int(nthr[f]), B)
                if lim == 0:
                    continue
                L = np.cumsum(H[a, f][order[:lim]], axis=0)
                g, ok = _gain_ex(kd, L, t, imp_t, min_inst)
                gl, okl = g.tolist(), ok.tolist()
                for j in range(lim):
                    if okl[j]:
                        seen.append(gl[j])
                        if gl[j] > best:
                            best, win = gl[j], (f, j, L[j], order)
            if gaps is not None:
                u = sorted(set(seen))
                gaps.append(u[-1] - u[-2] if len(u) >= 2 else INF)
            if win is None:
                out[a, 0] = -INF
                out[a, 4 + K:] = t
            else:
                f, j, L, order = win
                out[a, :3] = best, f, j
                out[a, 4:4 + K], out[a, 4 + K:] = L, t - L
                if nthr[f] < 0:
                    cat[a] = bin_set(order[:j + 1])
    return out, tot, cat


# ------------------------------------------------------------------------------------------------ decode
def ref_split_decode(so, tot, a_tree, T, min_inst, min_gain, can_level, leaf_children, missing_bin=False,
                     leaf_values=None, catm=None, nthr=None):
    """The partition tables of a level's decisions so [A, >= 7] (gain, feature, bin, left weight, left sum, right
    weight, right sum, missing-right) and node totals tot [A, >= 1] (weight, sum); nodes are ordered by tree.

    can = the level may split, gain finite, > 0 and >= min_gain, node weight >= 2 min_inst.  split_feat = feature or
    -1; split_bin = bin of a plain numeric split, else 0; cat_off = a for missing-right winners (masks[a] = bins
    1..b) and categorical winners (masks[a] = catm[a]), else -1.  A child of a splitting node is active unless its
    weight is below 2 min_inst or the next level is the last; child[2a + s] numbers the active children in (node,
    side) order, -1 otherwise.  tfirst_next[t] = active children of the trees before t.  lv [3A] fp32: lv[2a + s] the
    value of child s when it is a leaf, lv[2A + a] the value of a node that does not split, 0 elsewhere; a value is
    -S / (W + lam) (xgb) or S / W (0 when W = 0) in fp64, then cast."""
    A = so.shape[0]
    sw = so.shape[1]
    sf, sb, co = np.full(A, -1, np.int32), np.zeros(A, np.int32), np.full(A, -1, np.int32)
    masks = np.zeros((A, 8), dtype=np.uint32)
    child = np.full(2 * A, -1, np.int32)
    lv = np.zeros(3 * A, dtype=np.float32) if leaf_values is not None else None

    def value(W, S):
        with np.errstate(all="ignore"):
            if leaf_values[0] == "xgb":
                return np.float32(-np.float64(S) / (np.float64(W) + leaf_values[1]))
            return np.float32(np.float64(S) / np.float64(W) if W > 0.0 else 0.0)
    per_tree = np.zeros(T + 1, dtype=np.int64)
    n = 0
    for a in range(A):
        g, W = float(so[a, 0]), float(tot[a, 0])
        can = bool(can_level) and np.isfinite(g) and g > 0.0 and g >= min_gain and W >= 2.0 * min_inst
        if can:
            f, b = int(so[a, 1]), int(so[a, 2])
            sf[a] = f
            if catm is not None and nthr is not None and nthr[f] < 0:
                co[a] = a
                masks[a] = np.asarray(catm[a]).view(np.uint32)
            elif missing_bin and sw >= 8 and so[a, 7] > 0.5:
                co[a] = a
                masks[a] = bin_set(range(1, min(b, 255) + 1))
            else:
                sb[a] = b
            for s in (0, 1):
                cw = float(so[a, 3 + 2 * s])
                if not (cw < 2.0 * min_inst) and not leaf_children:
                    child[2 * a + s] = n
                    n += 1
                    per_tree[int(a_tree[a]) + 1] += 1
                elif lv is not None:
                    lv[2 * a + s] = value(cw, so[a, 4 + 2 * s])
        elif lv is not None:
            lv[2 * A + a] = value(W, tot[a, 1])
    return {"split_feat": sf, "split_bin": sb, "cat_off": co, "masks": masks, "child": child,
            "tfirst_next": np.cumsum(per_tree)[:T].astype(np.int32), "lv": lv}


def case_decode(A, seed=0, sw=8, missing_bin=False, cats=False, min_inst=1.5, min_gain=0.25):
    """Hand-built decisions of ``A`` nodes in 7 trees (trees 0, 3 and 6 without a node where A allows): gains from
    {NaN, +-inf, 0, -1, min_gain and its neighbours, larger ones}, node and child weights at 2 min_inst, one ulp
    below, 0 and above, missing-right bins at the mask words' edges, categorical winners with random bitmasks."""
    rng = np.random.default_rng(seed)
    T, d = 7, 9
    occ = np.array([1, 2, 4, 5])[:max(1, min(A, 4))]
    a_tree = np.sort(occ[rng.integers(0, len(occ), size=A)]).astype(np.int32)
    two = 2.0 * min_inst
    gpool = np.array([np.nan, INF, -INF, 0.0, -1.0, min_gain, np.nextafter(min_gain, -INF),
                      np.nextafter(min_gain, INF), 3.5, 17.0])
    wpool = np.array([two, np.nextafter(two, -INF), 0.0, np.nextafter(two, INF), 40.0])
    so = np.zeros((A, sw))
    pick = rng.integers(0, len(gpool), size=A)
    so[:, 0] = np.where(rng.random(A) < 0.55, rng.random(A) + 1.0, gpool[pick])
    so[:, 1] = rng.integers(0, d, size=A)
    bpool = np.array([1, 31, 32, 255, 0, 7, 63, 64, 224])
    so[:, 2] = bpool[rng.integers(0, len(bpool), size=A)]
    for c in (3, 5):
        so[:, c] = np.where(rng.random(A) < 0.5, rng.random(A) * 30 + two, wpool[rng.integers(0, len(wpool), size=A)])
    so[:, 4], so[:, 6] = rng.normal(size=A) * 9, rng.normal(size=A) * 9
    if sw >= 8:
        so[:, 7] = rng.integers(0, 2, size=A)
    tot = np.zeros((A, 2))
    tot[:, 0] = np.where(rng.random(A) < 0.6, rng.random(A) * 60 + two, wpool[rng.integers(0, len(wpool), size=A)])
    tot[:, 1] = rng.normal(size=A) * 20
    so[-1, 0], so[-1, 3], so[-1, 5], tot[-1, 0] = 2.0, 40.0, 41.0, 81.0   # the last node splits into active children
    nthr = catm = None
    if cats:
        nthr = np.full(d, 30, dtype=np.int32)
        nthr[[2, 5, 8]] = -1
        catm = rng.integers(0, 1 << 32, size=(A, 8), dtype=np.uint64).astype(np.uint32).view(np.int32)
    return SimpleNamespace(A=A, T=T, d=d, so=so, tot=tot, a_tree=a_tree, min_inst=min_inst, min_gain=min_gain,
                           missing_bin=missing_bin, nthr=nthr, catm=catm, sw=sw)


# ------------------------------------------------------------------------------------------------ the suites' cases
# (A, d, B, masked): split_scan, serial kernel
SCAN_SHAPES = [(1, 1, 1, False), (3, 1, 2, False), (5, 37, 17, False), (5, 37, 17, True), (4, 130, 40, False),
               (4, 130, 40, True), (2, 257, 64, False)]
# (A, d, B, masked): split_scan(exact=True) -- B > 64 the wave kernel (R = 2 up to 128 bins, R = 4 beyond), else and
# beyond 4096 features the serial one
WAVE_SHAPES = [(1, 1, 65, False), (6, 17, 65, False),(6, 16, 128, True), (6, 17, 129, False), (1, 130, 255, True), (6, 130, 256, False),
               (6, 17, 255, True), (1, 16, 256, False), (6, 17, 64, False), (6, 16, 40, True), (1, 4097, 65, False)]
# (kind, K, A, d, B, min_inst): split_scan_ex
EX_CASES = [(kind, K, A, d, B, mi)
            for kind, K in (("variance", 2), ("gini", 2), ("gini", 5), ("gini", 32), ("entropy", 3), ("entropy", 32))
            for A, d, B, mi in ((8, 12, 40, 1.0), (4, 130, 40, 5.0), (6, 6, 129, 5.0), (6, 6, 256, 1.0))]
# (A, can_level, leaf_children, sw, missing_bin, cats, leaf values)
DECODE_CASES = [(1, 1, 0, 8, True, False, ("xgb", 1.0)), (2, 1, 0, 7, False, False, ("variance", 0.0)),
                (2, 1, 1, 8, False, True, None), (511, 1, 0, 8, True, False, ("variance", 0.0)),
                (513, 1, 0, 7, False, True, ("variance", 0.0)), (513, 0, 0, 8, True, False, ("xgb", 1.0)),
                (1025, 1, 0, 8, True, False, ("xgb", 1.0)), (1025, 1, 1, 8, False, True, ("xgb", 1.0)),
                (1025, 1, 0, 7, False, True, None)]


@functools.lru_cache(maxsize=None)
def scan_case(A, d, B, masked, kind, missing, general):
    """A split_scan case with its parameter sets and references (shared by the CPU and the GPU suite).  The second
    parameter set puts min_inst (variance) / min_child_weight (XGBoost, lambda 0) at the lighter child's weight of a
    winner, so that winner sits exactly on the threshold, and gamma at the median best gain, so that some nodes
    report a negative best gain."""
    c = case_hist(A, d, B, seed=A * 1000 + d * 10 + B + kind + 2 * missing, missing=missing, masked=masked,
                  general=general)
    base = ref_split_scan(c.H, c.nthr, c.mask, kind, missing, 1.0, 0.0, 0.0, 1.0)[0]
    fin = base[np.isfinite(base[:, 0])]
    # the lighter child of the first node's winner: as a threshold that winner stays legal, exactly at >=
    at = float(min(fin[0, 3], fin[0, 5])) if len(fin) else 1.0
    gmid = float(np.median(fin[:, 0])) if len(fin) else 1.0
    if kind == 0:
        params = [dict(min_inst=1.0), dict(min_inst=at)]
    else:
        params = [dict(min_inst=1.0, lam=1.5, gamma=0.0, mcw=1.0), dict(min_inst=1.0, lam=0.0, gamma=gmid, mcw=at)]
    c.params = [dict(dict(min_inst=1.0, lam=1.0, gamma=0.0, mcw=1.0), **p) for p in params]
    c.kind = kind
    c.refs = [ref_split_scan(c.H, c.nthr, c.mask, kind, missing, **p) for p in c.params]
    c.at = at
    return c


def ex_layout(d, B):
    """Categorical features of an (d, B) split_scan_ex case and its (categorical, numeric) twin pair."""
    if d >= 12:
        return {3: min(7, B), 7: min(33, B), 9: B}, (9, 10)
    if B > 200:
        return {3: min(7, B), 4: B}, (4, 5)       # the categorical twin has the lower key: its set wins
    return {3: min(7, B), 5: B}, (5, 4)


@functools.lru_cache(maxsize=None)
def ex_case(kind, K, A, d, B, min_inst):
    cats, twin = ex_layout(d, B)
    seed = 7 * K + d + B + len(kind)
    for _ in range(16):
        c = case_hist(A, d, B, K=0 if kind == "variance" else K, seed=seed, masked=d in (12, 130), cats=cats,
                      twin_cat=twin, ex=kind, empty=0.15)
        c.kind, c.min_inst, c.gaps = kind, min_inst, []
        c.ref = ref_split_scan_ex(c.H, c.nthr, c.mask, kind, min_inst, gaps=c.gaps)
        if kind != "entropy" or min(c.gaps) > 1e-9:
            return c
        seed += 1000      # a near-tie of entropy gains: another seed (the gap is asserted by the CPU suite)
    raise AssertionError("no tie-safe entropy case")


@functools.lru_cache(maxsize=None)
def decode_case(i):
    """Case ``i`` of DECODE_CASES with its reference tables."""
    A, can_level, leaf_children, sw, mb, cats, lvk = DECODE_CASES[i]
    c = case_decode(A, seed=i, sw=sw, missing_bin=mb, cats=cats, min_inst=1.5 if i % 2 == 0 else 1.0,
                    min_gain=0.25 if i % 3 else 0.0)
    c.can_level, c.leaf_children, c.leaf_values = can_level, leaf_children, lvk
    c.ref = ref_split_decode(c.so, c.tot, c.a_tree, c.T, c.min_inst, c.min_gain, can_level, leaf_children, mb, lvk,
                             c.catm, c.nthr)
    return c


def entropy_bound(K):
    """Absolute bound on an entropy gain's difference between two correctly rounded evaluations whose log2 differ
    in the last place: three weighted impurities of at most log2 K, K terms each (a divide, a log2, a multiply),
    and the adds."""
    return (3 * K + 8) * 2.0 ** -52 * max(1.0, float(np.log2(K)))
