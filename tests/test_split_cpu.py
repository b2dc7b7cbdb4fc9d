"""The references of tests/_split_refs.py pinned on the host before they judge a kernel (tests/test_split_gpu.py).

On the GPU suite's own cases the torch split chain (ForestTrainer._node_stats / _best_splits on cpu tensors) must
return the references' winners bit for bit -- finiteness, feature, bin, gain, child statistics, the missing-right flag
and the category sets; entropy gains within the stated bound -- and ``ref_split_decode`` must pass the checked build's
ForestTrainer._check_decode against a host decode written the way ForestTrainer._level_advance computes it.  The
cases' coverage conditions (ties, thresholds met exactly, negative best gains, category sets in all eight mask
words, tie-safe entropy cases) are asserted from the references alone."""
import numpy as np
import pytest
import torch

from tests import _split_refs as R
from cdnaml.models.tree.engine import ForestTrainer, TreeParams

SCAN = [(s, kind, missing) for s in R.SCAN_SHAPES for kind, missing in ((0, False), (1, False), (1, True))]
WAVE = [(s, kind, missing) for s in R.WAVE_SHAPES for kind, missing in ((0, False), (1, False), (1, True))]


def _trainer(kind, C, nthr, categorical, min_inst=1.0, missing=False, lam=1.0, gamma=0.0, mcw=1.0):
    tr = object.__new__(ForestTrainer)
    tr.p = TreeParams(impurity=kind, num_classes=C, min_instances=min_inst, reg_lambda=lam, gamma=gamma,
                      min_child_weight=mcw)
    tr.classification = kind in ("gini", "entropy")
    tr.C = C if tr.classification else 0
    tr.stats_k = C if tr.classification else 2

    class _D:
        pass
    tr.data = _D()
    tr.data.nthr = nthr
    tr.data.categorical = categorical
    tr.data.missing_bin = missing
    return tr


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def _torch_scan(c, kind, missing, p):
    tr = _trainer("xgb" if kind else "variance", 0, c.nthr, {}, p["min_inst"], missing, p["lam"], p["gamma"],
                  p["mcw"])
    H = torch.from_numpy(c.H)
    mk = None if c.mask is None else torch.from_numpy(c.mask.view(np.int32))
    tot = tr._node_stats(H, None)
    gain, bf, bb, lst, rst, _, _, mr = tr._best_splits(H, tot, mk)
    mr = np.zeros(c.A, dtype=bool) if mr is None else mr.numpy()
    return tot.numpy(), gain.numpy(), bf.numpy(), bb.numpy(), lst.numpy(), rst.numpy(), mr


# ============================================================================================ split_scan
@pytest.mark.parametrize("shape,kind,missing", SCAN + WAVE)
def test_ref_split_scan_equals_torch_chain_on_exact_histograms(shape, kind, missing):
    c = R.scan_case(*shape, kind, missing, False)
    for p, (out, tot) in zip(c.params, c.refs):
        ttot, gain, bf, bb, lst, rst, mr = _torch_scan(c, kind, missing, p)
        assert np.array_equal(_bits(tot), _bits(ttot))
        ok = np.isfinite(gain)
        assert np.array_equal(ok, np.isfinite(out[:, 0]))
        assert np.array_equal(bf[ok], out[ok, 1]) and np.array_equal(bb[ok], out[ok, 2]), (bf, bb, out[:, 1:3])
        assert np.array_equal(_bits(gain[ok]), _bits(out[ok, 0]))
        assert np.array_equal(_bits(lst[ok]), _bits(out[ok, 3:5])) and np.array_equal(_bits(rst[ok]),
                                                                                      _bits(out[ok, 5:7]))
        assert np.array_equal(mr[ok], out[ok, 7] > 0.5)
        # nodes without a legal split: -inf, zeros, the totals on the right
        assert (out[~ok, 1:5] == 0).all() and np.array_equal(out[~ok, 5:7], tot[~ok]) and (out[~ok, 7] == 0).all()


@pytest.mark.parametrize("shape,kind,missing", SCAN)
def test_ref_split_scan_winners_equal_torch_chain_on_general_histograms(shape, kind, missing):
    """Inexact sums: torch adds pairwise, the reference (and the serial kernel) left to right, so totals and gains
    differ in the last places; the decisions agree."""
    c = R.scan_case(*shape, kind, missing, True)
    out, _ = c.refs[0]
    _, gain, bf, bb, _, _, mr = _torch_scan(c, kind, missing, c.params[0])
    ok = np.isfinite(gain)
    assert np.array_equal(ok, np.isfinite(out[:, 0]))
    assert np.array_equal(bf[ok], out[ok, 1]) and np.array_equal(bb[ok], out[ok, 2])
    assert np.array_equal(mr[ok], out[ok, 7] > 0.5)


def test_scan_cases_reach_their_edges():
    """What the cases are built for, read from the references: a winner on the copied feature (lowest key of a tie),
    a missing-left winner on feature 128 whose gain feature 0's missing-right candidate ties, negative best gains,
    nodes without a legal split, a threshold that a candidate's weight meets exactly."""
    dup = twin = neg = none = thr = 0
    for shape, kind, missing in SCAN + WAVE:
        c = R.scan_case(*shape, kind, missing, False)
        for p, (out, _) in zip(c.params, c.refs):
            fin = np.isfinite(out[:, 0])
            neg += int((out[fin, 0] < 0).sum())
            none += int((~fin).sum())
            for a in np.nonzero(fin)[0]:
                f = int(out[a, 1])
                if f == 1 and c.dups and np.array_equal(c.H[a, 1], c.H[a, 2]) and R.mask_bit(c.mask, a, 2):
                    dup += 1
                if c.twin_miss and f == 128 and out[a, 7] == 0 and c.H[a, 0, 0, 0] > 0:
                    nthr = c.nthr.copy()
                    nthr[128] = 0
                    o2, _ = R.ref_split_scan(c.H[a:a + 1], nthr, None if c.mask is None else c.mask[a:a + 1], kind,
                                             missing, **p)
                    twin += int(o2[0, 7] == 1 and o2[0, 1] == 0 and o2[0, 0] == out[a, 0] and o2[0, 2] == out[a, 2])
        # the second parameter set: a winner whose lighter child weighs exactly the threshold
        out = c.refs[1][0]
        fin = np.isfinite(out[:, 0])
        thr += int((np.minimum(out[fin, 3], out[fin, 5]) == c.params[1]["mcw" if kind else "min_inst"]).sum())
    assert min(dup, twin, neg, none) > 0 and thr >= len(SCAN + WAVE) // 2, (dup, twin, neg, none, thr)


def test_threshold_at_an_attained_weight_is_inclusive():
    """min_inst (variance) / min_child_weight (XGBoost) equal to a left weight: that candidate is legal, and one ulp
    more makes it illegal -- the references' comparison is >=, as gain_of's."""
    H = np.zeros((1, 1, 4, 2))
    H[0, 0, :, 0] = [3, 0, 0, 5]
    H[0, 0, :, 1] = [1.5, 0, 0, -2.25]
    nthr = np.array([3], dtype=np.int32)
    for kind in (0, 1):
        out, _ = R.ref_split_scan(H, nthr, None, kind, False, 3.0, 1.0, 0.0, 3.0)
        assert np.isfinite(out[0, 0]) and out[0, 2] == 0 and out[0, 3] == 3.0 and out[0, 5] == 5.0
        up = float(np.nextafter(3.0, np.inf))
        out, _ = R.ref_split_scan(H, nthr, None, kind, False, up, 1.0, 0.0, up)
        assert out[0, 0] == -np.inf


# ============================================================================================ split_scan_ex
def _torch_ex(c):
    C = c.H.shape[-1]
    tr = _trainer(c.kind, C, c.nthr, c.cats, c.min_inst)
    H = torch.from_numpy(c.H)
    mk = None if c.mask is None else torch.from_numpy(c.mask.view(np.int32))
    tot = tr._node_stats(H, None)
    gain, bf, bb, lst, rst, order, cat_feats, _ = tr._best_splits(H, tot, mk)
    return tot.numpy(), gain.numpy(), bf.numpy(), bb.numpy(), lst.numpy(), rst.numpy(), order.numpy(), cat_feats


@pytest.mark.parametrize("case", R.EX_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_ref_split_scan_ex_equals_torch_chain(case):
    c = R.ex_case(*case)
    K = c.H.shape[-1]
    out, tot, cat = c.ref
    ttot, gain, bf, bb, lst, rst, order, cat_feats = _torch_ex(c)
    assert np.array_equal(_bits(tot), _bits(ttot))
    ok = np.isfinite(gain)
    assert np.array_equal(ok, np.isfinite(out[:, 0]))
    assert np.array_equal(bf[ok], out[ok, 1]) and np.array_equal(bb[ok], out[ok, 2]), (bf, bb, out[:, 1:3])
    if c.kind == "entropy":
        diff = np.abs(gain[ok] - out[ok, 0]).max() if ok.any() else 0.0
        print(f"{case}: entropy gain, torch vs reference: {diff / R.entropy_bound(K):.3f} of the bound")
        assert diff <= R.entropy_bound(K)
    else:
        assert np.array_equal(_bits(gain[ok]), _bits(out[ok, 0]))
    assert np.array_equal(_bits(lst[ok]), _bits(out[ok, 4:4 + K]))
    assert np.array_equal(_bits(rst[ok]), _bits(out[ok, 4 + K:]))
    assert (out[:, 3] == 0).all() and (out[~ok, 1:4 + K] == 0).all() and np.array_equal(out[~ok, 4 + K:], tot[~ok])
    for a in range(c.A):
        f, b = int(out[a, 1]), int(out[a, 2])
        if ok[a] and f in c.cats:
            assert np.array_equal(R.bin_set(order[a, cat_feats.index(f), :b + 1]), cat[a]), (a, f, b)
        else:
            assert not cat[a].any()


def test_entropy_cases_are_tie_safe():
    """Every node of every entropy case: the best gain and the next distinct one differ by more than 1e-9, far above
    the entropy bound, so a device log2 that differs in the last place cannot change a winner."""
    worst = np.inf
    for case in R.EX_CASES:
        if case[0] == "entropy":
            c = R.ex_case(*case)
            assert len(c.gaps) == c.A
            worst = min(worst, min(c.gaps))
    print(f"smallest gap between an entropy winner and the next distinct gain: {worst:.3e}")
    assert worst > 1e-9


def test_ex_cases_reach_their_edges():
    """A categorical winner with bits in all eight mask words, tied centroids inside a categorical feature, features
    with one and with no non-empty category, a masked-off categorical feature, a categorical candidate and a numeric
    one with equal best gains on either side of the key order, numeric and categorical winners."""
    words8 = tied = one = zero = off = cat_first = num_first = numw = catw = 0
    for case in R.EX_CASES:
        c = R.ex_case(*case)
        kd, K = R.KINDS_EX[c.kind], c.H.shape[-1]
        out, _, cat = c.ref
        fc, fn = c.twin_cat
        for a in range(c.A):
            for f in c.cats:
                _, ncnt, cent = R.cat_order(c.H[a, f], K, kd)
                fin = cent[cent != np.inf]
                tied += int(len(np.unique(fin)) < len(fin))
                one += int(ncnt == 1)
                zero += int(ncnt == 0)
                off += int(not R.mask_bit(c.mask, a, f) and c.H[a, f].any())
            if not np.isfinite(out[a, 0]):
                continue
            f = int(out[a, 1])
            catw += int(f in c.cats)
            numw += int(f not in c.cats)
            words8 += int(cat[a].all())
            if f in (fc, fn) and R.mask_bit(c.mask, a, fc) and R.mask_bit(c.mask, a, fn) and \
                    np.array_equal(c.H[a, fn], c.H[a, fc][R.cat_order(c.H[a, fc], K, kd)[0]]):
                assert f == min(fc, fn)      # equal content, equal gains: the lower key
                cat_first += int(fc < fn)
                num_first += int(fn < fc)
    assert min(words8, tied, one, zero, off, cat_first, num_first, numw, catw) > 0, \
        (words8, tied, one, zero, off, cat_first, num_first, numw, catw)


# ============================================================================================ split_decode
def _host_decode(c):
    """The decode of ForestTrainer._level_advance: can, the bin sets in dense numbering, leaf and child."""
    A, so = c.A, c.so
    gain, W = so[:, 0], c.tot[:, 0]
    with np.errstate(invalid="ignore"):
        can = np.isfinite(gain) & (gain > 0) & (gain >= c.min_gain) & (W >= 2 * c.min_inst)
    if not c.can_level:
        can[:] = False
    sp = np.nonzero(can)[0]
    split_feat, split_bin = np.full(A, -1, dtype=np.int32), np.zeros(A, dtype=np.int32)
    cat_off, cat_masks, child = np.full(A, -1, dtype=np.int32), [], np.full(2 * A, -1, dtype=np.int32)
    f_sp, b_sp = so[sp, 1].astype(np.int64), so[sp, 2].astype(np.int64)
    plain = np.ones(len(sp), dtype=bool)
    for j, a in enumerate(sp.tolist()):
        f, b = int(f_sp[j]), int(b_sp[j])
        if c.nthr is not None and c.nthr[f] < 0:
            m = c.catm[a].view(np.uint32).copy()
        elif c.missing_bin and so[a, 7] > 0.5:
            m = np.zeros(8, dtype=np.uint32)
            for q in range(1, b + 1):
                m[q >> 5] |= np.uint32(1) << np.uint32(q & 31)
        else:
            continue
        plain[j] = False
        cat_off[a] = len(cat_masks)
        cat_masks.append(m)
    split_bin[sp[plain]] = b_sp[plain]
    split_feat[sp] = f_sp
    cw = np.stack([so[sp, 3], so[sp, 5]], 1).reshape(-1)
    leaf = (cw < 2 * c.min_inst) | bool(c.leaf_children)
    nl = np.nonzero(~leaf)[0]
    ch_par = np.repeat(sp, 2)
    child[2 * ch_par[nl] + (nl & 1)] = np.arange(len(nl), dtype=np.int32)
    return can, split_feat, split_bin, cat_off, cat_masks, child, c.a_tree[ch_par[nl]], leaf, sp


@pytest.mark.parametrize("i", range(len(R.DECODE_CASES)), ids=lambda i: "-".join(str(x) for x in R.DECODE_CASES[i]))
def test_ref_split_decode_passes_the_checked_builds_comparison(i):
    c = R.decode_case(i)
    can, split_feat, split_bin, cat_off, cat_masks, child, n_tree, leaf, sp = _host_decode(c)
    dec = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v) for k, v in c.ref.items()
           if v is not None}
    ForestTrainer._check_decode(dec, split_feat, split_bin, cat_off, cat_masks, child, n_tree, c.T)
    assert np.array_equal(c.ref["split_bin"], split_bin)
    if c.leaf_values is not None:
        # the host forest's values of the same nodes (ForestTrainer._leaf_values_v, fp64, then one cast)
        tr = _trainer(c.leaf_values[0], 0, None, {}, lam=c.leaf_values[1])
        lv = np.zeros(3 * c.A, dtype=np.float32)
        ch = np.stack([c.so[sp][:, 3:5], c.so[sp][:, 5:7]], 1).reshape(-1, 2)
        idx = (2 * np.repeat(sp, 2) + np.tile([0, 1], len(sp)))[leaf]
        lv[idx] = tr._leaf_values_v(ch[leaf])[:, 0].astype(np.float32)
        lv[2 * c.A + np.nonzero(~can)[0]] = tr._leaf_values_v(c.tot[~can])[:, 0].astype(np.float32)
        assert np.array_equal(lv.view(np.int32), c.ref["lv"].view(np.int32))


def test_decode_cases_reach_their_edges():
    """Trees without an active node before, between and after the others; gains on either side of min_gain; node and
    child weights at 2 min_inst and one ulp below; missing-right winners at bins 1, 31, 32 and 255; categorical
    winners; splitting nodes in every 1024-entry chunk of the scan."""
    bins, cat, chunks = set(), 0, set()
    for i, spec in enumerate(R.DECODE_CASES):
        c = R.decode_case(i)
        assert set(c.a_tree.tolist()) <= {1, 2, 4, 5}
        can = c.ref["split_feat"] >= 0
        tfn = c.ref["tfirst_next"]
        assert tfn[0] == 0 and tfn[3] == tfn[4] and tfn[6] == (c.ref["child"] >= 0).sum()
        mr = can & (c.ref["cat_off"] >= 0) & (c.nthr is None)
        bins |= set(c.so[mr, 2].astype(int).tolist())
        cat += int((can & (c.ref["cat_off"] >= 0)).sum()) if c.nthr is not None else 0
        if c.A >= 511 and c.can_level:
            two = 2.0 * c.min_inst
            g = c.so[:, 0]
            for v in (c.min_gain, np.nextafter(c.min_gain, -np.inf)):
                assert (g == v).any()
            assert np.isnan(g).any() and np.isinf(g).any()
            for col in (c.tot[:, 0], c.so[:, 3], c.so[:, 5]):
                assert (col == two).any() and (col == np.nextafter(two, -np.inf)).any() and (col == 0).any()
            if not c.leaf_children:
                chunks |= {(c.A, int(e) // 1024) for e in np.nonzero(c.ref["child"] >= 0)[0]}
    assert {1, 31, 32, 255} <= bins and cat > 0
    assert {(511, 0), (513, 0), (513, 1), (1025, 0), (1025, 1), (1025, 2)} <= chunks
