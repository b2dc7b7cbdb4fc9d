"""The relational references (tests/_relops_refs.py) against brute force, the hash replicas against values a
stand-alone host build of hashagg.hip's three helpers printed, and the portable aggregation path
(``relational.aggregate`` on CPU batches) against ``ref_groups`` where it used to disagree with the K16 tables:
NaN in min / max, long min / max above 2^53, all-null groups, first / last."""
import math

import numpy as np
import pytest
import torch

from tests import _relops_refs as RR
from cdnaml.sql import relational, types as T
from cdnaml.sql.batch import Batch, ColumnData
from cdnaml.sql.column import ColRef
from cdnaml.sql.functions import AggExpr

I64_MIN, I64_MAX = RR.I64_MIN, RR.I64_MAX

# (key, mix64, part_of(., 5), part_of(., 9), part_of(., 14), pos_of(., 64), pos_of(., 4094), pos_of(., 65535))
# printed by a host program compiled from the mix64 / part_of / pos_of of hashagg.hip
HOST_HASHES = [
    (0, 0xE220A8397B1DCDAF, 28, 452, 14472, 30, 1968, 31517),
    (1, 0x910A2DEC89025CC1, 18, 290, 9282, 34, 2191, 35073),
    (-1, 0xE4D971771B652C20, 28, 457, 14646, 6, 438, 7013),
    (I64_MIN, 0x481EC0A212A9F3DB, 9, 144, 4615, 4, 298, 4777),
    (I64_MAX, 0x2A67D7552E039EA7, 5, 84, 2713, 11, 735, 11779),
    (7919, 0x436D6B84A3314152, 8, 134, 4315, 40, 2609, 41776),
    (-(1 << 40), 0x7EC2F3D2E3AE3E6B, 15, 253, 8112, 56, 3641, 58285),
    (0x0123456789ABCDEF, 0x157A3807A48FAA9D, 2, 42, 1374, 41, 2631, 42127),
]


def test_hash_replicas_equal_the_host_build():
    keys = np.array([h[0] for h in HOST_HASHES], dtype=np.int64)
    h = RR.mix64(keys)
    assert h.dtype == np.uint64
    assert [int(x) for x in h] == [r[1] for r in HOST_HASHES]
    assert [RR.mix64_int(int(k)) for k in keys] == [r[1] for r in HOST_HASHES]
    assert RR.part_of(h, 0).tolist() == [0] * len(keys)
    for col, pbits in ((2, 5), (3, 9), (4, 14)):
        assert RR.part_of(h, pbits).tolist() == [r[col] for r in HOST_HASHES]
    for col, S in ((5, 64), (6, 4094), (7, 65535)):
        assert RR.pos_of(h, S).tolist() == [r[col] for r in HOST_HASHES]


def test_hash_replicas_python_integers_random():
    rng = np.random.default_rng(0)
    keys = rng.integers(I64_MIN, I64_MAX, 2000, dtype=np.int64, endpoint=True)
    h = RR.mix64(keys)
    for k, x in zip(keys.tolist(), h.tolist()):
        m = RR.mix64_int(k)
        assert x == m
    hs = [RR.mix64_int(k) for k in keys.tolist()]
    assert RR.part_of(h, 9).tolist() == [x >> 55 for x in hs]
    assert RR.pos_of(h, 64).tolist() == [((x & 0xFFFFFFFF) * 64) >> 32 for x in hs]
    assert RR.pos_of(h, 8190).tolist() == [((x & 0xFFFFFFFF) * 8190) >> 32 for x in hs]
    assert int(RR.pos_of(h, 64).max()) == 63 and int(RR.pos_of(h, 64).min()) == 0


def test_feasibility_of_the_two_pass_shape():
    """10 000 keys arange * 7919 - 2^40 over 512 partitions: the fullest holds 34 keys, within a cap of 56."""
    keys = np.arange(10_000, dtype=np.int64) * 7919 - (1 << 40)
    d = RR.distinct_per_partition(keys, 9)
    assert d.sum() == 10_000 and d.max() == 34
    assert RR.distinct_per_partition(np.array([I64_MIN, 5, 5], dtype=np.int64), 0).tolist() == [1]
    assert RR.distinct_per_chunk(np.array([1, 1, 2, I64_MIN, 3, 3, 3, 3, 9]), 4) == [2, 1, 1]


def test_same_value_rules():
    nan = float("nan")
    assert RR.same_value(None, None) and not RR.same_value(None, 0.0) and not RR.same_value(0.0, None)
    assert RR.same_value(nan, nan) and not RR.same_value(nan, 1.0) and not RR.same_value(math.inf, nan)
    assert RR.same_value(-0.0, 0.0) and RR.same_value(5e-324, 5e-324) and not RR.same_value(5e-324, 0.0)
    assert not RR.same_value(1.0, 1.0 + 2 ** -52) and RR.same_value(3, 3) and not RR.same_value(3, 4)
    assert RR.same_value(np.float64(2.5), 2.5) and RR.same_value((1 << 53) + 1, (1 << 53) + 1)
    assert not RR.same_value((1 << 53) + 1, 1 << 53)


def _brute(keys, v, m):
    """A different formulation of the group rules: numpy masks per key instead of the row dictionary."""
    out = {}
    for k in np.unique(keys):
        sel = keys == k
        rows = np.nonzero(sel)[0]
        ok = sel if m is None else sel & m
        x = np.asarray(v, dtype=np.float64)[ok]
        if len(x) == 0:
            s = lo = hi = None
        else:
            with np.errstate(invalid="ignore"):
                s = float(np.sum(x))
            fin = x[~np.isnan(x)]
            lo = float(fin.min()) if len(fin) else float("nan")
            hi = float("nan") if len(fin) < len(x) else float(fin.max())
        out[int(k)] = (len(rows), int(rows[0]), int(rows[-1]), len(x), s, lo, hi)
    return out


@pytest.mark.parametrize("masked", [False, True])
def test_ref_groups_against_brute_force(masked):
    rng = np.random.default_rng(1 + masked)
    n = 400
    keys = rng.choice(np.array([I64_MIN, I64_MAX, -1, 0, 1, 77, 1 << 40], dtype=np.int64), n)
    v = RR.exact_values(rng, n, np.float64)
    v[keys == 77] = np.nan                          # only NaN
    v[(keys == 1) & (rng.random(n) < 0.3)] = np.nan  # NaN among numbers
    v[keys == 0] = np.where(rng.random((keys == 0).sum()) < 0.5, np.inf, -np.inf)
    m = None
    if masked:
        m = rng.random(n) < 0.7
        m[keys == -1] = False                       # an all-null group
    got = RR.ref_groups(keys, [(v, m)], [("sum", 0), ("min", 0), ("max", 0), ("count", 0), ("last", 0)])
    ref = _brute(keys, v, m)
    assert sorted(got) == sorted(ref)
    for k, (cnt, first, last, nn, s, lo, hi) in ref.items():
        g = got[k]
        assert (g["cnt"], g["first"], g["last"]) == (cnt, first, last)
        assert g["acc"][3] == nn and g["acc"][4] == last
        for a, b in zip(g["acc"][:3], (s, lo, hi)):
            assert RR.same_value(a, b), (k, a, b)
    if masked:
        assert got[-1]["acc"][:3] == [None, None, None] and got[-1]["acc"][3] == 0
    assert math.isnan(got[77]["acc"][1]) and math.isnan(got[77]["acc"][2])
    assert not math.isnan(got[1]["acc"][1]) and math.isnan(got[1]["acc"][2])


def test_ref_groups_sum_is_exact_and_order_free():
    rng = np.random.default_rng(3)
    n = 5000
    keys = rng.integers(0, 7, n)
    for dt in (np.float64, np.float32, np.int64, np.int32, np.int16, np.int8, np.uint8, np.bool_):
        v = RR.exact_values(rng, n, dt)
        assert v.dtype == np.dtype(dt)
        a = RR.ref_groups(keys, [(v, None)], [("sum", 0)])
        p = rng.permutation(n)
        b = RR.ref_groups(keys[p], [(v[p], None)], [("sum", 0)])
        for k in a:
            s = a[k]["acc"][0]
            assert s == b[k]["acc"][0]
            assert s == float(np.sum(v[keys == k].astype(np.float64)))   # fp64 accumulation is exact here
            assert (s * 1024).is_integer() and abs(s) < 2.0 ** 53 / 1024
    assert abs(RR.exact_values(rng, 100_000, np.float64)).max() <= 1024.0
    assert RR.ref_groups([1, 1], [([1 << 62, 1], None)], [("sum", 0)])[1]["acc"][0] == float((1 << 62) + 1)


def test_ref_join_against_brute_force():
    rng = np.random.default_rng(4)
    bk = rng.integers(-5, 6, 60)
    bv = rng.random(60) < 0.8
    pk = np.concatenate([rng.integers(-8, 9, 200), [I64_MIN, I64_MAX]])
    pv = rng.random(202) < 0.8
    for bvalid, pvalid in ((None, None), (bv, None), (None, pv), (bv, pv)):
        ri, cnt = RR.ref_join(bk, bvalid, pk, pvalid)
        for r in range(len(pk)):
            rows = [j for j in range(60) if bk[j] == pk[r] and (bvalid is None or bvalid[j])]
            if pvalid is not None and not pvalid[r]:
                rows = []
            assert ri[r] == (rows[0] if rows else -1) and cnt[r] == len(rows)


def test_ref_pack_order_is_tuple_order_nulls_first():
    rng = np.random.default_rng(5)
    n = 300
    cols, tuples = [], [[] for _ in range(n)]
    for lo, hi in ((-3, 3), (0, 1), (100, 104), (-128, 127)):
        v = rng.integers(lo, hi + 1, n)
        m = rng.random(n) < 0.8
        cols.append((v, m, lo, hi - lo + 2))
        for r in range(n):
            tuples[r].append((1, int(v[r])) if m[r] else (0, 0))     # a null sorts before every value
    cols.append((np.zeros(n, np.int64), np.zeros(n, bool), 0, 2))    # an all-null column
    w = RR.ref_pack(cols)
    order_w = sorted(range(n), key=lambda r: (w[r], r))
    order_t = sorted(range(n), key=lambda r: (tuples[r], r))
    assert order_w == order_t
    for a in range(0, n, 7):
        for b in range(n):
            assert (w[a] == w[b]) == (tuples[a] == tuples[b])
    assert min(w) >= 0 and max(w) < 8 * 3 * 6 * 257 * 2
    # nine columns of radix 2^7 exceed 2^62: Python integers, no wrap
    wide = RR.ref_pack([(np.array([126]), None, 0, 128)] * 9)
    assert wide[0] == sum(127 * 128 ** j for j in range(9))


def test_ref_bucket_compact_is_a_stable_grouping():
    rng = np.random.default_rng(6)
    keep = rng.integers(0, 6, 500).astype(np.uint8)
    idx, counts = RR.ref_bucket_compact(keep, 5)
    order = np.argsort(keep[keep > 0], kind="stable")
    assert np.array_equal(idx, np.nonzero(keep > 0)[0][order])
    assert counts.tolist() == [int((keep == b + 1).sum()) for b in range(5)]
    idx, counts = RR.ref_bucket_compact(np.zeros(9, np.uint8), 3)
    assert idx.size == 0 and counts.tolist() == [0, 0, 0]


def test_ordered_to_float_inverts_the_ordered_image():
    import struct
    vals = [-math.inf, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.5, math.inf, float("nan")]
    img = []
    for v in vals:
        b = struct.unpack("<Q", struct.pack("<d", v))[0]
        img.append((~b) & ((1 << 64) - 1) if b >> 63 else b | (1 << 63))
    assert img == sorted(img) and len(set(img)) == len(img)       # NaN above +inf, -0.0 below 0.0
    for v, u in zip(vals, img):
        assert RR.same_value(RR.ordered_to_float(u), v) and 0 < u < (1 << 64) - 1   # never a sentinel


# ------------------------------------------------------------------------------ the portable aggregation path
def _col(v, m=None):
    t = torch.from_numpy(np.ascontiguousarray(v))
    dt = {torch.float64: T.DoubleType(), torch.float32: T.FloatType(), torch.int64: T.LongType(),
          torch.int32: T.IntegerType()}[t.dtype]
    return ColumnData(t, dt, None if m is None else torch.from_numpy(np.ascontiguousarray(m)))


def _aggregate(keys, v, m, kinds):
    batch = Batch({"k": _col(keys), "v": _col(v, m)})
    out = relational.aggregate(batch, ["k"], [(kd, AggExpr(kd, ColRef("v"))) for kd in kinds])
    ks = out.columns["k"].values.tolist()
    res = {}
    for kd in kinds:
        c = out.columns[kd]
        vals = c.values.tolist()
        ok = [True] * len(vals) if c.valid is None else c.valid.tolist()
        res[kd] = {k: (x if o else None) for k, x, o in zip(ks, vals, ok)}
    return ks, res, out


def _check(keys, v, m, kinds):
    ks, res, out = _aggregate(keys, v, m, kinds)
    ops = [kd for kd in kinds if kd in ("sum", "min", "max", "count", "last")]
    ref = RR.ref_groups(keys, [(v, m)], [(o, 0) for o in ops])
    assert ks == sorted(ref)                         # groups in key order
    for k, g in ref.items():
        for kd in kinds:
            got = res[kd][k]
            if kd == "first":
                want = v[g["first"]] if m is None or m[g["first"]] else None
            elif kd == "last":
                want = v[g["last"]] if m is None or m[g["last"]] else None
            else:
                want = g["acc"][ops.index(kd)]
            if kd == "sum" and want is not None and np.asarray(v).dtype.kind in "iu":
                want = int(want)
            assert RR.same_value(got, None if want is None else RR._py(want)), (kd, k, got, want)
    return out


def test_portable_min_max_order_nan_as_spark_does():
    """min skips NaN unless every non-null value of the group is NaN; max is NaN as soon as one value is."""
    nan = float("nan")
    keys = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3, 3, 4, 4, 5], dtype=np.int64)
    v = np.array([1.0, nan, -2.5, nan, nan, np.inf, nan, 7.0, 3.0, 5.0, -np.inf, nan, nan])
    _check(keys, v, None, ["min", "max", "count"])
    _, res, _ = _aggregate(keys, v, None, ["min", "max"])
    assert res["min"][0] == -2.5 and math.isnan(res["max"][0])
    assert math.isnan(res["min"][1]) and math.isnan(res["max"][1])
    assert res["min"][2] == math.inf and res["min"][4] == -math.inf and res["max"][3] == 7.0
    # a null NaN is no value: group 5's only row is null -> no value; group 0's NaN is null -> max is finite
    m = np.ones(len(v), bool)
    m[[1, 12]] = False
    _check(keys, v, m, ["min", "max", "count"])
    _check(keys, v.astype(np.float32), m, ["min", "max"])


def test_portable_long_min_max_are_exact_above_2_53():
    big = 1 << 60
    keys = np.array([0, 0, 0, 1, 1, 2, 2, 3], dtype=np.int64)
    v = np.array([big + 1, big + 3, big + 2, -big - 1, -big - 2, I64_MAX, I64_MAX - 1, I64_MIN], dtype=np.int64)
    assert len(set(v.astype(np.float64)[:3])) == 1       # fp64 cannot tell them apart
    out = _check(keys, v, None, ["min", "max", "first", "last"])
    assert out.columns["min"].values.dtype == torch.int64
    assert out.columns["min"].values.tolist() == [big + 1, -big - 2, I64_MAX - 1, I64_MIN]
    assert out.columns["max"].values.tolist() == [big + 3, -big - 1, I64_MAX, I64_MIN]
    m = np.array([1, 0, 1, 1, 0, 0, 0, 1], bool)         # nulls carry the extreme values; group 2 is all null
    _check(keys, v, m, ["min", "max", "count"])
    _check(keys, (v >> 40).astype(np.int32), m, ["min", "max", "sum"])


def test_portable_all_null_groups_first_last_and_exact_sums():
    rng = np.random.default_rng(7)
    n = 3000
    keys = rng.choice(np.array([I64_MIN, I64_MAX, -1, 0, 1, 12345], dtype=np.int64), n)
    for dt in (np.float64, np.float32, np.int64, np.int32):
        v = RR.exact_values(rng, n, dt)
        m = rng.random(n) < 0.6
        m[keys == -1] = False
        v[~m] = 1 << 20                                  # a null's payload must not leak
        out = _check(keys, v, m, ["sum", "min", "max", "count", "first", "last"])
        assert out.columns["sum"].valid.tolist() == [True, False, True, True, True, True]
        _check(keys, v, None, ["sum", "min", "max", "count", "first", "last"])
