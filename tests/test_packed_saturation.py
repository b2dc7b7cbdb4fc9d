"""The packed histogram kernels (seg.hip, hist5.hip) at saturation, against exact integer sums.

A histogram cell's count and label sum share one 64-bit LDS word (csrc/kernels/packed.h): bits 44..63 the count,
bits 0..43 the sum of w * (q + 2^23).  Nothing in the kernels stops a carry between the fields; the host planning
keeps items x max weight below 2^20 per cell between clears (K.pack_rows_cap chunks, K._root_work row ranges, the
drain interval of cdna_hist5).  These tests fill that budget: chunks of exactly ``CAP`` items of weight 255 in ONE
cell, at q = +2^23 (count and sum fields both at their maximum, record bit 63 set) and at q = -2^23 (sum field zero).

The inputs are built so that the reference needs no floating point: bins are a uint8 matrix written directly, labels
are j * 2^-10 with integer |j| <= 2^23 (so the packed scale is 1024 and the quantised label is j itself), weights
are bytes.  The reference is numpy int64 ``np.add.at`` per (slot, feature) and calls nothing of cdnaml; every case
compares a kernel with it, never one kernel with another.  The ``cpu`` variants prove the reference and the inputs
(the CPU paths emulate the same integers), the ``cuda`` variants are the point."""
import functools

import numpy as np
import pytest
import torch

from cdnaml.ops import kernels as K

COUNT_BITS = 20                      # packed.h: the cell's count field
CAP = (1 << COUNT_BITS) // 256       # items of weight <= 255 one count field holds: what K.pack_rows_cap(255) must be
QMAX = 1 << 23                       # packed.h: |quantised label| <= 2^23
SCALE = 1024.0                       # labels are j / 1024
# one record buffer, carved into segments by the test: lengths around the cap, an empty one, and a last one that is
# one item past a whole six-items-per-wave trip (16 waves x 6 items x 16) after two full chunks and ends at the
# buffer's last record, so the kernels' unconditional record over-read lands in the buffer's REC_PAD tail
SEG_LENS = [1, CAP - 1, CAP, CAP + 1, 0, 2 * CAP + 16 * 6 * 16 + 1]
SEG_SLOT = [3, 0, 5, 1, 4, 2]        # out of order
I_MAX, I_MIN, I_LONG = 2, 3, 5       # the segments at (w 255, j +2^23), at (w 255, j -2^23), and the long one
S_REC = len(SEG_LENS)


def _devices():
    return ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


def _device(device):
    if device == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        from cdnaml.ops import _lib
        _lib.lib()  # must load: no silent fallback on a GPU box
        return torch.device("cuda:0")
    return torch.device("cpu")


# ---------------------------------------------------------------------------------------------- inputs
def _segs():
    lens = np.array(SEG_LENS, dtype=np.int64)
    return np.stack([np.cumsum(lens) - lens, lens, np.array(SEG_SLOT, dtype=np.int64)], 1)


@functools.lru_cache(maxsize=None)
def _items(cls3):
    """Per record position: weight, and the integer label j (regression) or the class 0 / 1 / 2 (cls3)."""
    rng = np.random.default_rng(11 + int(cls3))
    segs = _segs()
    n = int(segs[:, 1].sum())
    pos = lambda i: slice(int(segs[i, 0]), int(segs[i, 0] + segs[i, 1]))  # noqa: E731
    w = rng.integers(1, 256, n)
    # the long segment's weights are random in [192, 255]: any 5462 of its items outweigh the count field, so a
    # planner that let a chunk grow to twice the cap would carry out of it whatever the draw
    w[pos(I_LONG)] = rng.integers(192, 256, SEG_LENS[I_LONG])
    w[pos(I_MAX)] = 255
    w[pos(I_MIN)] = 255
    if cls3:
        lab = rng.integers(0, 3, n)
        lab[pos(I_MAX)] = 2  # a full chunk of class 2 at weight 255: the largest W2
        lab[pos(I_MIN)] = 1  # a full chunk of class 1 at weight 255: the largest W1 (below the 2^22 split)
    else:
        lab = rng.integers(-QMAX, QMAX + 1, n)
        lab[pos(I_MAX)] = QMAX
        lab[pos(I_MIN)] = -QMAX
    return w.astype(np.int64), lab.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _matrix(n, d, B, seed=0):
    """uint8 bins [n, d]: constant at the top bin in feature 0, feature d - 1 and either side of the kernels'
    feature-block boundary (128 features for B <= 80, 64 above), constant at bin 0 in feature 2, uniform elsewhere."""
    rng = np.random.default_rng(1000 * d + B + seed)
    M = rng.integers(0, B, (n, d), dtype=np.int64).astype(np.uint8)
    blk = 128 if B <= 80 else 64
    for f in (0, d - 1, blk - 1, blk):
        if 0 <= f < d:
            M[:, f] = B - 1
    M[:, 2] = 0
    M.setflags(write=False)
    return M


def _bins(M, dev):
    """The [G, n, 8] feature-group-major layout of M, written directly (not through binize)."""
    n, d = M.shape
    G = (d + 7) // 8
    P = np.zeros((n, 8 * G), dtype=np.uint8)
    P[:, :d] = M
    bins = torch.from_numpy(np.ascontiguousarray(P.reshape(n, G, 8).transpose(1, 0, 2))).to(dev)
    assert np.array_equal(K.bins_to_matrix(bins, d).cpu().numpy(), M)
    return bins


def _labels(j):
    v1 = torch.from_numpy((j.astype(np.float64) / SCALE).astype(np.float32))
    assert np.array_equal(v1.double().numpy() * SCALE, j)  # j / 1024 is exact in fp32
    return v1


def _encode(rows, w, q):
    """The item record written out (packed.h): row | w << 31 | (q + 2^23) << 39; q = +2^23 sets bit 63."""
    u = np.uint64
    return (rows.astype(u) | (w.astype(u) << u(31)) | ((q + QMAX).astype(u) << u(39))).view(np.int64)


def _records(dev, cls3):
    """(rec, w, lab): the record buffer of one tree with every row in local node 0, from K.codes_compact on the
    device under test, checked word for word against the test's own encoding."""
    w, lab = _items(cls3)
    n = len(w)
    codes = torch.from_numpy((w << 8).astype(np.uint16).view(np.int16)).reshape(1, n).to(dev)
    if cls3:
        q, scale = np.where(lab == 2, K.CLS3_CODE, lab), 1.0
        v1 = torch.from_numpy(q.astype(np.float32))
    else:
        q, scale = lab, SCALE
        v1 = _labels(lab)
        assert int(lab.max()) == QMAX and int(lab.min()) == -QMAX and float(v1.abs().max()) == 2.0 ** 13
        assert K.seg_scales(None, v1.to(dev), 255, n)[1] == SCALE
    rec, _, _, _, sg = K.codes_compact(codes, torch.zeros(1, dtype=torch.int32), np.zeros(1, dtype=np.int32), 1,
                                       None, v1.to(dev), rec_scale=scale)
    assert rec.dtype == torch.int64 and np.array_equal(np.asarray(sg), [[0, n]])
    # position = row: the compaction of one node is stable
    want = _encode(np.arange(n), w, q)
    assert cls3 or (want < 0).any()  # the top label value makes the word negative as int64
    assert np.array_equal(rec.cpu().numpy(), want)
    return rec, w, lab


# ---------------------------------------------------------------------------------------------- reference
def _add_cells(out, M, rows, cols):
    """out [d, B, k] += the integer columns ``cols`` of the items at bins rows ``rows``: np.add.at per feature."""
    for f in range(M.shape[1]):
        b = M[rows, f]
        for k, c in enumerate(cols):
            np.add.at(out[f, :, k], b, c)


def _reference(M, B, rows, cols, segs, S):
    """int64 [S, d, B, len(cols)]: segment {start, len, slot} adds its items' columns into its slot."""
    out = np.zeros((S, M.shape[1], B, len(cols)), dtype=np.int64)
    for start, ln, slot in np.asarray(segs).tolist():
        _add_cells(out[slot], M, rows[start:start + ln], [c[start:start + ln] for c in cols])
    return out


def _columns(w, lab, cls3):
    """The reference columns: (sum w, sum w * j), or (sum w, sum w[y == 1], sum w[y == 2]) for 3-class records."""
    return [w, w * (lab == 1), w * (lab == 2)] if cls3 else [w, w * lab]


@functools.lru_cache(maxsize=None)
def _record_reference(d, B, cls3):
    w, lab = _items(cls3)
    ref = _reference(_matrix(len(w), d, B), B, np.arange(len(w)), _columns(w, lab, cls3), _segs(), S_REC)
    ref.setflags(write=False)
    return ref


# ---------------------------------------------------------------------------------------------- the host plan
def _watch_plan(monkeypatch):
    """Collect the (chunk, work list) pairs the host planners hand the segment kernels."""
    seen = []
    plan, work = K._seg_plan, K._seg_work

    def plan_(*a, **k):
        c, wk = plan(*a, **k)
        seen.append((int(c), np.array(wk)))
        return c, wk

    def work_(segs, chunk, *a, **k):
        wk = work(segs, chunk, *a, **k)
        seen.append((int(chunk), np.array(wk)))
        return wk
    monkeypatch.setattr(K, "_seg_plan", plan_)
    monkeypatch.setattr(K, "_seg_work", work_)
    return seen


def _the_plan(seen, segs, B, wm):
    """The plan of the launch just made; the CPU paths plan nothing, there the numpy planner is asked."""
    if not seen:
        chunk = K._fill_chunk(segs, min(K.SEG_HIST_CHUNK, K.pack_rows_cap(wm)), B)
        return int(chunk), K._seg_work(segs, chunk)
    assert len(seen) == 1
    return seen[0]


def _assert_saturating(plan, w):
    """The premise of a saturating case: no chunk above the cap, and some work item of exactly ``CAP`` items, all of
    weight 255 (they share one cell in every constant column)."""
    chunk, work = plan
    assert chunk <= CAP and int(work[:, 1].max()) == CAP
    full = work[work[:, 1] == CAP]
    assert any(bool((w[s:s + CAP] == 255).all()) for s in full[:, 0].tolist())


def _record_hist(device, monkeypatch, d, B, cls3=False, s10=False):
    """A record histogram of the shared buffer on ``device`` and its reference."""
    dev = _device(device)
    rec, w, lab = _records(dev, cls3)
    M = _matrix(len(w), d, B)
    assert int(M[:, 0].min()) == B - 1 and int(M[:, d - 1].min()) == B - 1 and int(M[:, 2].max()) == 0 and B - 1 != 0
    bins = _bins(M, dev)
    rm = K.bins_seg10(bins, d) if s10 else K.bins_row_major(bins)
    seen = _watch_plan(monkeypatch)
    got = K.seg_hist(bins, d, B, rec, None, None, None, _segs(), S_REC, 255, (1.0, 1.0 if cls3 else SCALE),
                     bins_rm=rm, rec=True, raw=True, rm_s10=s10, cls3=cls3)
    _assert_saturating(_the_plan(seen, _segs(), B, 255), w)
    assert got.dtype == torch.int64
    return got.cpu().numpy(), _record_reference(d, B, cls3)


# ---------------------------------------------------------------------------------------------- 1. perm path
@pytest.mark.parametrize("device", _devices())
@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("row_major", [None, "rm", "pad"])
@pytest.mark.parametrize("d,B", [(21, 40), (100, 256)])
def test_perm_path(device, d, B, row_major, weights, monkeypatch):
    """K.seg_hist(raw=True) without v0 on perm / v1p / wp: seg_hist_kernel (no row-major copy) and
    seg_hist_flat_kernel (row-major rows of G and of 16 words).  Without ``wp`` every weight is 1 and the cap is 2^19
    items, far above the buffer: that variant runs unsaturated and checks the sums only."""
    dev = _device(device)
    w, j = _items(False)
    n = len(w)
    if not weights:
        w = np.ones(n, dtype=np.int64)
    M = _matrix(n, d, B)
    perm = np.random.default_rng(5).permutation(n)  # the items' rows: any order, the statistics go by position
    bins = _bins(M, dev)
    rm = None if row_major is None else K.bins_row_major(bins, pad=row_major == "pad")
    if rm is not None and device == "cuda":
        assert rm.shape[1] == (16 if row_major == "pad" else (d + 7) // 8)
    seen = _watch_plan(monkeypatch)
    got = K.seg_hist(bins, d, B, torch.from_numpy(perm.astype(np.int32)).to(dev), None, _labels(j).to(dev),
                     torch.from_numpy(w.astype(np.uint8)).to(dev) if weights else None, _segs(), S_REC,
                     255 if weights else 1, bins_rm=rm, raw=True)
    plan = _the_plan(seen, _segs(), B, 255 if weights else 1)
    if weights:
        _assert_saturating(plan, w)
    else:
        assert plan[0] <= (1 << COUNT_BITS) // 2
    ref = _perm_reference(d, B, weights)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), ref)


@functools.lru_cache(maxsize=None)
def _perm_reference(d, B, weights):
    w, j = _items(False)
    n = len(w)
    if not weights:
        w = np.ones(n, dtype=np.int64)
    return _reference(_matrix(n, d, B), B, np.random.default_rng(5).permutation(n), [w, w * j], _segs(), S_REC)


# ---------------------------------------------------------------------------------------------- 2. records, flat
@pytest.mark.parametrize("device", _devices())
@pytest.mark.parametrize("d,B", [(130, 40), (70, 256)])
def test_records_flat(device, d, B, monkeypatch):
    """The (row, group)-pair record kernel (seg_hist_flat_kernel<REC>, SEG_LANE off): one cell copy, so the full
    chunks bring a cell to count 2^20 - 4096 and offset sum 2^44 - 2^36."""
    monkeypatch.setattr(K, "SEG_LANE", False)
    got, ref = _record_hist(device, monkeypatch, d, B)
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------------------------- 3. records, lane
@pytest.mark.parametrize("device", _devices())
@pytest.mark.parametrize("B", [2, 32, 33, 40, 41, 64, 65, 80, 81, 128, 129, 256])
def test_records_lane(device, B, monkeypatch):
    """The lane-feature record kernels either side of every B at which the kernel or its plane changes: lane8
    <32> / <40> / <64> (B <= 64), lane <80> (B <= 80), lane4 <128> / <256>.  d = 130 is two blocks of 128 features
    (the second partial), d = 70 two blocks of 64."""
    monkeypatch.setattr(K, "SEG_LANE", True)
    got, ref = _record_hist(device, monkeypatch, 130 if B <= 80 else 70, B)
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------------------------- 4. seg10 records
@pytest.mark.parametrize("device", _devices())
@pytest.mark.parametrize("d,B", [(100, 40), (100, 32), (100, 33), (81, 17)])
def test_records_seg10(device, d, B, monkeypatch):
    """The six-items-per-wave kernel on seg10 rows; on the GPU its chunks come from the native planner with round
    fitting (ncu > 0), which may grow a chunk -- never past the cap (_assert_saturating checks the chunk)."""
    got, ref = _record_hist(device, monkeypatch, d, B, s10=True)
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------------------------- 5. codes path
N_CODES = 35011


@functools.lru_cache(maxsize=None)
def _codes_items(cls3):
    """T = 2 over N_CODES rows at weight 255: tree 0 has every row in its root, tree 1 has the first 6 CAP rows and
    three quarters of the rest in local node 1 (the others in node 2 or done).  Labels: the first 3 CAP rows at
    j = +2^23 (cls3: class 2, the next 3 CAP rows class 1), the rest random."""
    rng = np.random.default_rng(23 + int(cls3))
    n = N_CODES
    loc = np.zeros((2, n), dtype=np.int64)
    loc[1] = rng.choice([1, 1, 1, 1, 1, 1, 2, 0xFF], n)
    loc[1, :6 * CAP] = 1
    if cls3:
        lab = rng.integers(0, 3, n)
        lab[:3 * CAP] = 2
        lab[3 * CAP:6 * CAP] = 1
    else:
        lab = rng.integers(-QMAX, QMAX + 1, n)
        lab[:3 * CAP] = QMAX
        lab[-1] = -QMAX
    return loc, lab.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _codes_reference(d, B, cls3):
    loc, lab = _codes_items(cls3)
    n = N_CODES
    M = _matrix(n, d, B, seed=1)
    w = np.full(n, 255, dtype=np.int64)
    cols = _columns(w, lab, cls3)
    out = np.zeros((2, d, B, len(cols)), dtype=np.int64)
    for t, node in enumerate((0, 1)):
        rows = np.nonzero(loc[t] == node)[0]
        _add_cells(out[t], M, rows, [c[rows] for c in cols])
    return out


def _codes_hist(device, monkeypatch, d, B, cls3=False):
    """K.seg_hist_codes over all slots and over a slot-range slice, with the planner emitting the chunks it emits at
    the headline size (one CU: no spreading of a small input over the chip) -> [(got, reference)]."""
    dev = _device(device)
    wide = B > 80
    monkeypatch.setattr(K, "_num_cus", lambda _dev: 1)
    monkeypatch.setattr(K, "_ROOT_WORK", {})
    loc, lab = _codes_items(cls3)
    n = N_CODES
    M = _matrix(n, d, B, seed=1)
    bins = _bins(M, dev)
    rows = K.bins_row_major(bins) if wide else K.bins_seg10(bins, d)
    codes = torch.from_numpy(((255 << 8) | loc).astype(np.uint16).view(np.int16)).to(dev)
    if cls3:
        v1, scale = torch.from_numpy(np.where(lab == 2, K.CLS3_CODE, lab).astype(np.float32)).to(dev), 1.0
    else:
        v1, scale = _labels(lab).to(dev), SCALE
    kc = 3 if cls3 else 2
    ref = _codes_reference(d, B, cls3)
    out = []
    for s0, s1 in [(0, 2), (1, 2)]:
        # the premise: some block takes the most rows the count field allows, all of them in one cell at weight 255
        work = K._root_work(n, d, wide, 255, s0, s1, dev)
        top = CAP - 64 if wide else 3 * CAP - 1024
        assert int(work[:, 1].max()) == top
        assert any(r0 + ln <= 3 * CAP for r0, ln, _ in work[work[:, 1] == top].tolist())
        if device == "cuda":
            got = K.seg_hist_codes(rows, d, B, codes, v1, scale, 255, np.array([0, 1]), np.array([0, 1]), s0, s1,
                                   torch.zeros((s1 - s0, d, B, kc), dtype=torch.int64, device=dev), cls3=cls3)
        else:
            # the kernel is GPU-only; its contract is the sums of codes_compact records + the record histogram
            slot_of = np.array([0, -1, 1, -1], dtype=np.int32)  # tree 0: its root; tree 1: local node 1 of 0..2
            rec, _, _, _, sg = K.codes_compact(codes, torch.tensor([0, 1], dtype=torch.int32), slot_of, 2, None, v1,
                                               rec_scale=scale)
            sb = np.concatenate([sg, np.arange(2)[:, None]], 1)
            got = K.seg_hist(bins, d, B, rec, None, None, None, sb, 2, 255, (1.0, scale), rec=True, raw=True,
                             cls3=cls3)[s0:s1]
        assert got.dtype == torch.int64
        out.append((got.cpu().numpy(), ref[s0:s1]))
    return out


@pytest.mark.parametrize("device", _devices())
@pytest.mark.parametrize("d,B", [(100, 40), (100, 33), (100, 81), (37, 256)])
def test_codes_path(device, d, B, monkeypatch):
    """The root kernels (seg_hist_lane10_root_kernel, B <= 40; seg_hist_lane4_root_kernel, 80 < B <= 256) at the
    full-size row chunks of the headline shape: 3 CAP - 1024 rows over three cell copies, CAP - 64 rows over one."""
    for got, ref in _codes_hist(device, monkeypatch, d, B):
        assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------------------------- 6. hist_codes
N_H5, D_H5, B_H5 = 30000, 21, 256


@functools.lru_cache(maxsize=None)
def _h5_items():
    """T = 2 trees x 3 local nodes, all built; the first 8192 rows sit in one node per tree at j = +2^23."""
    rng = np.random.default_rng(31)
    loc = rng.integers(0, 3, (2, N_H5))
    loc[0, :2 * CAP] = 0
    loc[1, :2 * CAP] = 1
    j = rng.integers(-QMAX, QMAX + 1, N_H5)
    j[:2 * CAP] = QMAX
    j[-1] = -QMAX
    return loc, j.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _h5_reference(wmax):
    loc, j = _h5_items()
    M = _matrix(N_H5, D_H5, B_H5, seed=2)
    w = np.full(N_H5, wmax, dtype=np.int64)
    out = np.zeros((6, D_H5, B_H5, 2), dtype=np.int64)
    for t in range(2):
        for node in range(3):
            rows = np.nonzero(loc[t] == node)[0]
            _add_cells(out[3 * t + node], M, rows, [w[rows], (w * j)[rows]])
    return out


@pytest.mark.parametrize("device", _devices())
@pytest.mark.parametrize("wmax", [255, 254])
@pytest.mark.parametrize("lds_kb", [16, 128])
@pytest.mark.parametrize("compact", [0, 2])
def test_hist_codes_packed(device, compact, lds_kb, wmax, monkeypatch):
    """K.hist_codes' packed kernels (hist5p lane-per-row, hist5q wave-compacted) between register drains: 16 KB of
    LDS holds one slot (512-thread hist5p blocks, a drain every 8 iterations), 128 KB five (1024 threads, every
    4); 8192 consecutive rows of weight ``wmax`` share one cell per tree, so every drain interval inside them ends
    with the cell at 4096 x wmax.  wmax = 254 allows 4112 rows per interval, no multiple of the block size."""
    dev = _device(device)
    monkeypatch.setattr(K, "HIST5_PACKED", True)
    monkeypatch.setattr(K, "HIST5_COMPACT", compact)
    loc, j = _h5_items()
    M = _matrix(N_H5, D_H5, B_H5, seed=2)
    bins = _bins(M, dev)
    codes = torch.from_numpy(((wmax << 8) | loc).astype(np.uint16).view(np.int16)).to(dev)
    v1 = _labels(j)
    assert float(v1.abs().max()) == 2.0 ** 13  # so hist_codes' own packed scale is 1024
    tree = np.repeat(np.arange(2), 3)
    out = K.hist_codes(0, bins, D_H5, codes, torch.tensor([0, 3], dtype=torch.int32), None, v1.to(dev), None, 0,
                       torch.arange(6, dtype=torch.int32).to(dev), tree.astype(np.int32), tree, None, B_H5,
                       lds_budget=lds_kb * 1024, wmax=wmax).cpu().numpy()
    ref = _h5_reference(wmax)
    # float64 moments of integers below 2^53 and a power-of-two scale: exact
    assert int(np.abs(ref).max()) < 1 << 53
    assert np.array_equal(out[..., 0], ref[..., 0].astype(np.float64))
    assert np.array_equal(out[..., 1] * SCALE, ref[..., 1].astype(np.float64))


# ---------------------------------------------------------------------------------------------- 7. 3-class records
def _assert_cls3(got, ref, w, lab, slot):
    assert np.array_equal(got, ref)
    counts = K.cls3_expand(torch.from_numpy(got)).numpy()
    # feature 2 is constant at bin 0: that cell holds the whole slot
    assert counts[slot, 2, 0].tolist() == [int(w[lab == c].sum()) for c in range(3)]


@pytest.mark.parametrize("device", _devices())
@pytest.mark.parametrize("kernel,d,B", [("flat", 130, 40), ("lane8", 130, 40), ("lane4", 70, 129),
                                        ("lane10", 100, 40)])
def test_cls3_records(device, kernel, d, B, monkeypatch):
    """3-class records (label codes 0 / 1 / 2^22, scale 1) through the record kernels: the flush splits a block's
    sum W1 + 2^22 W2 into two columns; a full chunk of class 2 and a full chunk of class 1 at weight 255."""
    monkeypatch.setattr(K, "SEG_LANE", kernel != "flat")
    got, ref = _record_hist(device, monkeypatch, d, B, cls3=True, s10=kernel == "lane10")
    w, lab = _items(True)
    segs = _segs()
    for i in (I_MAX, I_MIN, I_LONG):
        p = slice(int(segs[i, 0]), int(segs[i, 0] + segs[i, 1]))
        _assert_cls3(got, ref, w[p], lab[p], SEG_SLOT[i])


@pytest.mark.parametrize("device", _devices())
@pytest.mark.parametrize("d,B", [(100, 40), (37, 256)])
def test_cls3_codes_path(device, d, B, monkeypatch):
    """3-class sums straight from the row codes (both root kernels): the first 3 CAP rows class 2, the next 3 CAP
    class 1, all at weight 255, so the seg10 kernel's full blocks hold W1 or W2 = 11264 x 255 (below 2^22)."""
    loc, lab = _codes_items(True)
    w = np.full(N_CODES, 255, dtype=np.int64)
    for (got, ref), s0 in zip(_codes_hist(device, monkeypatch, d, B, cls3=True), (0, 1)):
        for s in range(s0, 2):
            rows = loc[s] == s
            _assert_cls3(got, ref, w[rows], lab[rows], s - s0)
