"""The relational hash kernels (K16 hashagg.hip / hash.hip, K19 bucket_compact) at their table and key edges,
against the plain references of tests/_relops_refs.py.  Every comparison is exact: values come from
``exact_values`` (fp64 sums exact in any order), min / max are decoded from the ordered-u64 image the way
``_aggregate_native`` does, and zeros compare by value.

Table shapes are forced through ``R._hp_shape``: (64, 56, pbits) is the smallest table the kernels accept, so 56
keys fill a partition to its cap, probe chains wrap from slot 63 to slot 0, and pbits = 9 takes the two-pass radix
partition (n = 70 001 gives 18 source blocks: two pass-1 groups; and four row chunks on the low-cardinality path).
Before every kernel call the host replicas of the kernel's hash count the distinct keys of every partition, so a
``None`` (overflow) where the input fits is a failure, never a skip."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import _relops_refs as RR
from cdnaml.ops import _lib, kernels as K, relops as R

pytestmark = pytest.mark.gpu

N = 70_001
I64_MIN, I64_MAX = RR.I64_MIN, RR.I64_MAX
SPECIALS = np.array([I64_MAX, -1, 0, 1], dtype=np.int64)      # INT64_MIN is placed by row
SMALL = (64, 56)
SHAPES = {"default": None, "one": SMALL + (0,), "p5": SMALL + (5,), "p9": SMALL + (9,)}
DISTINCT = {"default": 2000, "one": 50, "p5": 800, "p9": 10_000}
NP_DT = {torch.float64: np.float64, torch.float32: np.float32, torch.int64: np.int64, torch.int32: np.int32,
         torch.uint8: np.uint8, torch.bool: np.bool_, torch.int16: np.int16, torch.int8: np.int8}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch.device("cuda")


@pytest.fixture(scope="module")
def spark(dev):
    import cdnaml
    return cdnaml.SparkSession.builder.getOrCreate()


_real_shape = R._hp_shape


def _force(monkeypatch, shape):
    """(S, cap, pbits) hash_groups will use for n rows / na accumulators; forced unless shape is 'default'."""
    if SHAPES[shape] is not None:
        monkeypatch.setattr(R, "_hp_shape", lambda n, na: SHAPES[shape])
        return lambda n, na: SHAPES[shape]
    return _real_shape


@pytest.fixture
def la_seen(monkeypatch):
    """Records what the low-cardinality path returned (None: it reported overflow and the partitions ran)."""
    seen = []
    la = R._la_groups

    def spy(*a, **k):
        r = la(*a, **k)
        seen.append(r is not None)
        return r
    monkeypatch.setattr(R, "_la_groups", spy)
    return seen


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _vals(values, dev):
    return [(_t(v, dev), None if m is None else _t(m, dev)) for v, m in values]


def _chunk_rows(n):
    nblk = max(1, min(1024, n // 16384))
    return -(-n // nblk)


def _pick_keys(nd, pbits, cap):
    """nd distinct keys (the specials, then arange * 7919 - 2^40), taken greedily so that no partition of
    2^pbits gets more than cap of them."""
    cand = np.concatenate([SPECIALS, np.arange(4 * nd + 4096, dtype=np.int64) * 7919 - (1 << 40)])
    part = RR.part_of(RR.mix64(cand), pbits)
    fill = np.zeros(1 << pbits, dtype=np.int64)
    out = []
    for k, p in zip(cand.tolist(), part.tolist()):
        if fill[p] < cap:
            fill[p] += 1
            out.append(k)
            if len(out) == nd:
                break
    assert len(out) == nd
    return np.array(out, dtype=np.int64)


def _rows_of(rng, distinct, n, min_at=None):
    """n rows over the distinct keys, every key at least once when n allows; INT64_MIN once at row min_at."""
    idx = rng.integers(0, len(distinct), n)
    m = min(n, len(distinct))
    idx[:m] = rng.permutation(len(distinct))[:m]
    keys = distinct[idx]
    if min_at is not None:
        keys[min_at] = I64_MIN
    return keys


def _fits(keys, shape_of, na):
    """Asserts the partitioned path must succeed on these keys; returns whether the low-cardinality path must."""
    S, cap, pbits = shape_of(len(keys), na)
    per = RR.distinct_per_partition(keys, pbits)
    assert per.max() <= cap, (int(per.max()), cap)
    chunks = RR.distinct_per_chunk(keys, _chunk_rows(len(keys)))
    total = len(set(keys.tolist()) - {I64_MIN})
    return max(chunks) <= cap and total <= S - 1


def _check_groups(res, ref, accs):
    """Mode 0 / 2 result against ref_groups: key, cnt, first and every accumulator, through pos."""
    assert res is not None, "overflow reported for an input that fits"
    G = res["G"]
    assert G == len(ref)
    pos = res["pos"].long()
    assert pos.numel() == G and torch.unique(pos).numel() == G
    k = res["key"][pos].cpu().tolist()
    assert len(set(k)) == G and set(k) == set(ref)
    want = [ref[x] for x in k]
    assert res["cnt"][pos].cpu().tolist() == [w["cnt"] for w in want]
    assert res["first"][pos].cpu().tolist() == [w["first"] for w in want]
    for i, (op, _) in enumerate(accs):
        raw = res["acc"][i][pos].contiguous()
        exp = [w["acc"][i] for w in want]
        if op in ("count", "last"):
            assert raw.cpu().tolist() == exp, op
        elif op == "sum":
            got = raw.view(torch.float64).cpu().tolist()
            bad = [(kk, g, e) for kk, g, e in zip(k, got, exp) if not RR.same_value(g, 0.0 if e is None else e)]
            assert not bad, (op, i, bad[:5])
        else:
            has = (raw != (-1 if op == "min" else 0)).cpu().tolist()       # the two sentinels: no value
            val = K.ordered_to_double(raw).cpu().tolist()
            bad = [(kk, h, v, e) for kk, h, v, e in zip(k, has, val, exp)
                   if h != (e is not None) or (h and not RR.same_value(v, e))]
            assert not bad, (op, i, bad[:5])


_REFS = {}


def _ref(tag, keys, values, accs):
    key = (tag, tuple(accs))
    if key not in _REFS:
        _REFS[key] = RR.ref_groups(keys, values, accs)
    return _REFS[key]


ACCS_A = [("sum", 0), ("min", 0), ("max", 0), ("count", 0)]
ACCS_B = [("last", 0), ("min", 1), ("sum", 1), ("count", 1)]


def _two_columns(rng, n):
    """An fp64 column with nulls (payload 1e300) and an int32 column without."""
    v0 = RR.exact_values(rng, n, np.float64)
    m0 = rng.random(n) < 0.8
    v0[~m0] = 1e300
    return [(v0, m0), (RR.exact_values(rng, n, np.int32), None)]


# ------------------------------------------------------------------------------------------- hash_groups
@pytest.mark.parametrize("local", [True, False], ids=["local", "partitioned"])
@pytest.mark.parametrize("min_at", [0, 40_000], ids=["min_row0", "min_chunk2"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_hash_groups_shapes(dev, monkeypatch, la_seen, shape, min_at, local):
    """Every table shape on both paths: INT64_MIN (the special slot) once, as row 0 or inside one chunk only."""
    monkeypatch.setattr(R, "LOCAL_FIRST", local)
    shape_of = _force(monkeypatch, shape)
    rng = np.random.default_rng(11)
    S, cap, pbits = shape_of(N, 4)
    keys = _rows_of(rng, _pick_keys(DISTINCT[shape], pbits, cap), N, min_at)
    values = _two_columns(rng, N)
    la_fits = _fits(keys, shape_of, 4)
    kd, vd = _t(keys, dev), _vals(values, dev)
    for accs in (ACCS_A, ACCS_B):
        la_seen.clear()
        res = K.hash_groups(kd, vd, accs, mode=0)
        assert la_seen == ([la_fits] if local else [])
        _check_groups(res, _ref(("shapes", shape, min_at), keys, values, accs), accs)
    res = K.hash_groups(kd, vd, ACCS_A, mode=2)
    _check_groups(res, _ref(("shapes", shape, min_at), keys, values, ACCS_A), ACCS_A)
    assert torch.equal(res["key"][res["gpos"].long()], kd)


@pytest.mark.parametrize("local", [True, False], ids=["local", "partitioned"])
@pytest.mark.parametrize("shape", ["default", "p9"])
@pytest.mark.parametrize("n", [1, 255, 4097])
def test_hash_groups_tiny_inputs(dev, monkeypatch, shape, n, local):
    monkeypatch.setattr(R, "LOCAL_FIRST", local)
    shape_of = _force(monkeypatch, shape)
    rng = np.random.default_rng(n)
    S, cap, pbits = shape_of(n, 4)
    for min_at in (0, None):
        keys = _rows_of(rng, _pick_keys(min(n, 40), pbits, cap), n, min_at)
        values = _two_columns(rng, n)
        _fits(keys, shape_of, 4)
        ref = RR.ref_groups(keys, values, ACCS_A)
        kd, vd = _t(keys, dev), _vals(values, dev)
        _check_groups(K.hash_groups(kd, vd, ACCS_A, mode=0), ref, ACCS_A)
        res = K.hash_groups(kd, vd, ACCS_A, mode=2)
        _check_groups(res, ref, ACCS_A)
        assert torch.equal(res["key"][res["gpos"].long()], kd)
        keep = K.hash_groups(kd, mode=1, pout=7)
        first = np.zeros(n, bool)
        first[[g["first"] for g in ref.values()]] = True
        assert np.array_equal(keep.cpu().numpy() != 0, first)


def _search(pred, count, start=0):
    """The first ``count`` keys of arange * 7919 - 2^40 (from index start) that satisfy pred(hash)."""
    out = np.zeros(0, dtype=np.int64)
    while len(out) < count:
        cand = np.arange(start, start + (1 << 16), dtype=np.int64) * 7919 - (1 << 40)
        out = np.concatenate([out, cand[pred(RR.mix64(cand))]])
        start += 1 << 16
    return out[:count]


@pytest.mark.parametrize("local", [True, False], ids=["local", "partitioned"])
def test_probe_chains_wrap_at_the_table_end(dev, monkeypatch, la_seen, local):
    """56 keys (the cap: 87 % of 64 slots) whose home slot is 62 or 63: every chain wraps from slot 63 to 0."""
    monkeypatch.setattr(R, "LOCAL_FIRST", local)
    shape_of = _force(monkeypatch, "one")
    distinct = _search(lambda h: RR.pos_of(h, 64) >= 62, 56)
    assert set(RR.pos_of(RR.mix64(distinct), 64).tolist()) == {62, 63}
    rng = np.random.default_rng(12)
    keys = _rows_of(rng, distinct, N, 5)
    values = _two_columns(rng, N)
    assert _fits(keys, shape_of, 4)
    kd, vd = _t(keys, dev), _vals(values, dev)
    for accs in (ACCS_A, ACCS_B):
        res = K.hash_groups(kd, vd, accs, mode=2)
        _check_groups(res, _ref("wrap", keys, values, accs), accs)
        assert torch.equal(res["key"][res["gpos"].long()], kd)
    assert la_seen == ([True, True] if local else [])


@pytest.mark.parametrize("part", [0, 300, 511])
def test_one_full_partition_among_empty_ones(dev, monkeypatch, part):
    """All 56 keys in one of 512 partitions (the other 511 are empty): pos still indexes the groups."""
    monkeypatch.setattr(R, "LOCAL_FIRST", False)
    shape_of = _force(monkeypatch, "p9")
    distinct = _search(lambda h: RR.part_of(h, 9) == part, 56)
    rng = np.random.default_rng(13)
    keys = _rows_of(rng, distinct, N)
    values = _two_columns(rng, N)
    _fits(keys, shape_of, 4)
    per = RR.distinct_per_partition(keys, 9)
    assert per[part] == 56 and per.sum() == 56
    kd = _t(keys, dev)
    res = K.hash_groups(kd, _vals(values, dev), ACCS_A, mode=2)
    _check_groups(res, RR.ref_groups(keys, values, ACCS_A), ACCS_A)
    assert torch.equal(res["key"][res["gpos"].long()], kd)


@pytest.mark.parametrize("shape", ["p5", "p9"])
def test_partition_capacity_is_exact(dev, monkeypatch, shape):
    """Exactly cap distinct keys in one partition (and others half full, and empty ones) give groups; one more
    key in that partition reports overflow (None), in every mode."""
    monkeypatch.setattr(R, "LOCAL_FIRST", False)
    shape_of = _force(monkeypatch, shape)
    pbits = SHAPES[shape][2]
    P = 1 << pbits
    full = _search(lambda h: RR.part_of(h, pbits) == 7, 57)
    rest = np.concatenate([_search(lambda h, p=p: RR.part_of(h, pbits) == p, 28) for p in (0, 8, P - 1)])
    rng = np.random.default_rng(14)
    keys = _rows_of(rng, np.concatenate([full[:56], rest]), N, 123)
    per = RR.distinct_per_partition(keys, pbits)
    assert per[7] == 56 and per.max() == 56 and (per == 0).sum() == P - 4
    values = _two_columns(rng, N)
    kd, vd = _t(keys, dev), _vals(values, dev)
    ref = RR.ref_groups(keys, values, ACCS_A)
    _check_groups(K.hash_groups(kd, vd, ACCS_A, mode=0), ref, ACCS_A)
    keep = K.hash_groups(kd, mode=1, pout=3)
    assert keep is not None and int((keep != 0).sum()) == len(ref)
    over = keys.copy()
    over[N // 2] = full[56]
    assert RR.distinct_per_partition(over, pbits)[7] == 57
    od = _t(over, dev)
    assert K.hash_groups(od, vd, ACCS_A, mode=0) is None
    assert K.hash_groups(od, vd, ACCS_A, mode=2) is None
    assert K.hash_groups(od, mode=1, pout=3) is None


def test_chunk_and_merge_capacity(dev, monkeypatch):
    """R._la_groups directly, S = 64 / cap = 56: 56 distinct keys in every chunk give groups, 57 in one chunk give
    None; the merged table holds S - 1 = 63 keys: four chunks of 16 + 16 + 16 + 15 disjoint keys give groups,
    four chunks of 20 give None."""
    shape_of = _force(monkeypatch, "one")
    rng = np.random.default_rng(15)
    rpc = _chunk_rows(N)
    assert -(-N // rpc) == 4
    distinct = _pick_keys(100, 0, 100)
    values = _two_columns(rng, N)
    vd = _vals(values, dev)

    def chunked(per_chunk):
        keys = np.empty(N, dtype=np.int64)
        for c, ks in enumerate(per_chunk):
            r0, r1 = c * rpc, min(N, (c + 1) * rpc)
            keys[r0:r1] = _rows_of(rng, ks, r1 - r0)
        return keys

    keys = chunked([distinct[:56]] * 4)
    keys[3] = I64_MIN                               # the special slot is no table key
    assert RR.distinct_per_chunk(keys, rpc) == [56] * 4
    _check_groups(R._la_groups(_t(keys, dev), vd, ACCS_A, 0, 1), RR.ref_groups(keys, values, ACCS_A), ACCS_A)
    keys = chunked([distinct[:56], distinct[:57], distinct[:56], distinct[:56]])
    assert RR.distinct_per_chunk(keys, rpc) == [56, 57, 56, 56]
    assert R._la_groups(_t(keys, dev), vd, ACCS_A, 0, 1) is None
    assert R._la_groups(_t(keys, dev), (), (), 1, 5) is None
    keys = chunked([distinct[0:16], distinct[16:32], distinct[32:48], distinct[48:63]])
    assert len(set(keys.tolist())) == 63
    _check_groups(R._la_groups(_t(keys, dev), vd, ACCS_B, 0, 1), RR.ref_groups(keys, values, ACCS_B), ACCS_B)
    keys = chunked([distinct[0:20], distinct[20:40], distinct[40:60], distinct[60:80]])
    assert RR.distinct_per_chunk(keys, rpc) == [20] * 4 and len(set(keys.tolist())) == 80
    assert R._la_groups(_t(keys, dev), vd, ACCS_A, 0, 1) is None


@pytest.mark.parametrize("local", [True, False], ids=["local", "partitioned"])
@pytest.mark.parametrize("shape", ["default", "p9"])
def test_one_key_holds_ninety_percent_of_the_rows(dev, monkeypatch, shape, local):
    monkeypatch.setattr(R, "LOCAL_FIRST", local)
    shape_of = _force(monkeypatch, shape)
    rng = np.random.default_rng(16)
    S, cap, pbits = shape_of(N, 4)
    keys = _rows_of(rng, _pick_keys(DISTINCT[shape], pbits, cap), N, 9)
    hot = rng.random(N) < 0.9
    hot[9] = False
    keys[hot] = 424242
    values = _two_columns(rng, N)
    _fits(keys, shape_of, 4)
    kd, vd = _t(keys, dev), _vals(values, dev)
    for accs in (ACCS_A, ACCS_B):
        res = K.hash_groups(kd, vd, accs, mode=2)
        _check_groups(res, _ref(("skew", shape), keys, values, accs), accs)
        assert torch.equal(res["key"][res["gpos"].long()], kd)


@pytest.mark.parametrize("pout", [1, 7, 255])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dedup_marks_first_rows_with_their_output_partition(dev, monkeypatch, la_seen, shape, pout):
    """Mode 1: keep is non-zero exactly at every key's first row, holds 1 + the kernel's output partition
    (uint32)(mix64(k) >> 16) % pout there, and is the same on both paths."""
    shape_of = _force(monkeypatch, shape)
    rng = np.random.default_rng(17)
    S, cap, pbits = shape_of(N, 0)
    keys = _rows_of(rng, _pick_keys(DISTINCT[shape], pbits, cap), N, 40_000)
    la_fits = _fits(keys, shape_of, 0)
    first = {}
    for r, k in enumerate(keys.tolist()):
        first.setdefault(k, r)
    want = np.zeros(N, dtype=np.uint8)
    rows = np.array(list(first.values()))
    want[rows] = 1 + RR.dedup_bucket(keys[rows], pout)
    kd = _t(keys, dev)
    got = {}
    for local in (True, False):
        monkeypatch.setattr(R, "LOCAL_FIRST", local)
        la_seen.clear()
        keep = K.hash_groups(kd, mode=1, pout=pout)
        assert keep is not None and la_seen == ([la_fits] if local else [])
        got[local] = keep.cpu().numpy()
        assert np.array_equal(got[local], want)
    assert np.array_equal(got[True], got[False])


def _designated(rng, dtype, n, masked):
    """Keys, one value column of dtype and its mask: 50 keys in all, INT64_MIN among them, with designated groups
    9000.. (only nulls / +inf with finite / +inf with -inf / NaN with finite / only NaN / -0.0 with 0.0 / a
    denormal among zeros for the float types; only nulls / the type's extremes / its maximum alone for the integer
    types).  Null rows carry a real, large value."""
    npdt = NP_DT[dtype]
    keys = _rows_of(rng, _pick_keys(42, 5, 56), n, 40_000)
    v = RR.exact_values(rng, n, npdt)
    m = (rng.random(n) < 0.7) if masked else None
    free = np.setdiff1d(np.arange(n), [40_000])
    rows = rng.choice(free, (7, 40), replace=False)
    for j in range(7):
        keys[rows[j]] = 9000 + j
    must = []                                   # rows whose value makes the case: never null
    if np.dtype(npdt).kind == "f":
        big = npdt(1e300) if npdt == np.float64 else npdt(1e38)
        denorm = npdt(5e-324) if npdt == np.float64 else npdt(1e-45)
        assert 0 < float(denorm) < 1e-40
        v[rows[1, :3]] = np.inf
        v[rows[2, :3]] = np.inf
        v[rows[2, 3:6]] = -np.inf
        v[rows[3, 0:8:2]] = np.nan
        v[rows[4]] = np.nan
        v[rows[5, 0::2]] = 0.0
        v[rows[5, 1::2]] = -0.0
        v[rows[6]] = 0.0
        v[rows[6, 0]] = denorm
        must = [rows[1, :8], rows[2, :8], rows[3, :8], rows[4, :4], rows[5, :4], rows[6, :4]]
    else:
        if npdt == np.bool_:
            lo, hi, big = False, True, True
        elif npdt == np.int64:
            lo, hi, big = -(1 << 53), 1 << 53, I64_MAX      # fp64 holds these exactly; above, see the README
        else:
            lo, hi = np.iinfo(npdt).min, np.iinfo(npdt).max
            big = hi
        v[rows[1]] = 0
        v[rows[1, 0]] = lo
        v[rows[1, 1]] = hi
        v[rows[2]] = hi
        must = [rows[1, :4], rows[2, :4]]
    if masked:
        for r in must:
            m[r] = True
        m[rows[0]] = False                # only nulls
        v[~m] = big
    return keys, v, m


@pytest.mark.parametrize("local", [True, False], ids=["local", "partitioned"])
@pytest.mark.parametrize("masked", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("dtype", list(R._VAL_DT), ids=lambda d: str(d).replace("torch.", ""))
def test_accumulators_over_every_value_type(dev, monkeypatch, la_seen, dtype, masked, local):
    """sum / min / max / count / last over every value dtype of R._VAL_DT, with and without nulls, on 32 small
    partitions and on the chunk tables (50 keys fit both)."""
    monkeypatch.setattr(R, "LOCAL_FIRST", local)
    shape_of = _force(monkeypatch, "p5")
    rng = np.random.default_rng(18)
    keys, v, m = _designated(rng, dtype, N, masked)
    other = RR.exact_values(rng, N, np.float32 if dtype != torch.float32 else np.int16)
    values = [(v, m), (other, None if not masked else rng.random(N) < 0.5)]
    assert _fits(keys, shape_of, 4)
    kd, vd = _t(keys, dev), _vals(values, dev)
    assert vd[0][0].dtype == dtype
    for accs in (ACCS_A, [("last", 1), ("max", 1), ("sum", 0), ("count", 1)]):
        res = K.hash_groups(kd, vd, accs, mode=0)
        _check_groups(res, _ref(("types", dtype, masked), keys, values, accs), accs)
    assert la_seen == ([True, True] if local else [])
    ref = _ref(("types", dtype, masked), keys, values, ACCS_A)
    if masked:
        assert ref[9000]["acc"] == [None, None, None, 0]
    if dtype.is_floating_point:
        s, lo, hi, _ = ref[9002]["acc"]
        assert s != s and lo == -np.inf and hi == np.inf
        s, lo, hi, _ = ref[9003]["acc"]
        assert s != s and lo == lo and hi != hi
        s, lo, hi, _ = ref[9004]["acc"]
        assert lo != lo and hi != hi
        assert 0 < ref[9006]["acc"][0] == ref[9006]["acc"][2] < 1e-40


def test_aggregate_table_and_portable_paths_agree(dev, monkeypatch):
    """relational.aggregate on device batches, below HASH_MIN_ROWS (portable) and above (K16 tables): NaN in
    min / max, long min / max above 2^53 (the generic step of the table path) and an all-null group."""
    from cdnaml.sql import relational, types as T
    from cdnaml.sql.batch import Batch, ColumnData
    from cdnaml.sql.column import ColRef
    from cdnaml.sql.functions import AggExpr
    calls = []
    hg = K.hash_groups
    monkeypatch.setattr(K, "hash_groups", lambda *a, **k: calls.append(k.get("mode")) or hg(*a, **k))
    for n in (2_000, 20_000):
        rng = np.random.default_rng(n)
        keys = rng.integers(-3, 4, n)
        v = RR.exact_values(rng, n, np.float64)
        v[(keys == 0) & (rng.random(n) < 0.3)] = np.nan
        v[keys == 1] = np.nan
        m = rng.random(n) < 0.8
        m[keys == 2] = False
        big = (1 << 60) + rng.integers(0, 1000, n)
        big[keys < 0] *= -1
        small = RR.exact_values(rng, n, np.int64)
        batch = Batch({"k": ColumnData(_t(keys, dev), T.LongType()),
                       "v": ColumnData(_t(v, dev), T.DoubleType(), _t(m, dev)),
                       "b": ColumnData(_t(big, dev), T.LongType()),
                       "s": ColumnData(_t(small, dev), T.LongType(), _t(m, dev))})
        aggs = [("v", "min"), ("v", "max"), ("b", "min"), ("b", "max"), ("s", "min"), ("s", "max"), ("s", "sum")]
        for c0 in (0, 4):      # four accumulators per table call
            part = aggs[c0:c0 + 4]
            calls.clear()
            out = relational.aggregate(batch, ["k"], [(f"{kd}_{c}", AggExpr(kd, ColRef(c))) for c, kd in part])
            assert calls == ([] if n < R.HASH_MIN_ROWS else [2 if c0 == 0 else 0])
            ref = RR.ref_groups(keys, [(v, m), (big, None), (small, m)],
                                [(kd, "vbs".index(c)) for c, kd in part])
            ks = out.columns["k"].values.cpu().tolist()
            assert ks == sorted(ref)
            for i, (c, kd) in enumerate(part):
                col = out.columns[f"{kd}_{c}"]
                vals = col.values.cpu().tolist()
                ok = [True] * len(ks) if col.valid is None else col.valid.cpu().tolist()
                for k_, x, o in zip(ks, vals, ok):
                    e = ref[k_]["acc"][i]
                    if e is not None and c != "v":
                        e = int(e) if kd == "sum" else e
                    assert RR.same_value(x if o else None, e), (n, c, kd, k_, x, o, e)


# -------------------------------------------------------------------------------------------------- joins
def _wrap(x):
    return (int(x) + (1 << 63)) % (1 << 64) - (1 << 63)


def _build_side(rng, kind, case):
    """(keys, valid or None) of a build side; kind 'dense': a small key range, 'sparse': keys 2^40 apart."""
    scale = 1 if kind == "dense" else 1 << 40
    base = rng.integers(-300, 300, 2000) * scale
    if case == "one_row":
        return np.array([-17 * scale], dtype=np.int64), None
    if case == "all_null":
        return base, np.zeros(len(base), bool)
    if case == "repeat1000":
        keys = np.concatenate([base, np.full(1000, 5 * scale)])
        return keys[rng.permutation(len(keys))], None
    if case == "min_valid":
        off = rng.integers(0, 500, 2000) * scale
        keys = I64_MIN + off
        at = rng.choice(2000, 3, replace=False)
        keys[at] = I64_MIN
        valid = rng.random(2000) < 0.9
        valid[at] = True
        return keys, valid
    assert case == "null_shadow"
    valid = rng.random(len(base)) < 0.5
    keys = base.copy()
    keys[~valid] = np.where(rng.random((~valid).sum()) < 0.5, keys[valid][0], 100_000 * scale)   # real / absent
    return keys, valid


def _probe_side(rng, bkeys, bvalid, n):
    live = bkeys if bvalid is None else bkeys[bvalid]
    lo, hi = (int(live.min()), int(live.max())) if len(live) else (0, 0)
    edges = [lo, hi, _wrap(lo - 1), _wrap(hi + 1), I64_MIN, I64_MAX]
    pool = np.concatenate([bkeys, bkeys + 1, rng.integers(lo // 2, hi // 2 + 2, 64)]) if lo != I64_MIN else \
        np.concatenate([bkeys, bkeys + 1])
    keys = np.concatenate([np.array(edges, dtype=np.int64), pool[rng.integers(0, len(pool), max(n, 6))]])[:n]
    valid = np.ones(n, bool)
    if n > 6:
        null = 6 + rng.choice(n - 6, (n - 6) // 10, replace=False)
        valid[null] = False
        keys[null[::2]] = live[0] if len(live) else 0          # null rows holding a matching key
    return keys, valid


@pytest.mark.parametrize("case", ["one_row", "all_null", "repeat1000", "min_valid", "null_shadow"])
@pytest.mark.parametrize("kind", ["dense", "sparse", "dense_off"])
def test_join_table_and_probe(dev, monkeypatch, kind, case):
    """join_table + join_probe(want_cnt, want_slot) against ref_join: the direct-addressed kind, the hash kind
    through sparse keys and through DENSE_JOIN_MAX = 0; probes of 1 / 3 / 1025 / 70 001 rows with keys at and
    just outside the build range (where the difference from lo wraps), nulls on both sides."""
    if kind == "dense_off":
        monkeypatch.setattr(R, "DENSE_JOIN_MAX", 0)
    rng = np.random.default_rng(19)
    bkeys, bvalid = _build_side(rng, "sparse" if kind == "sparse" else "dense", case)
    tab = K.join_table(_t(bkeys, dev), None if bvalid is None else _t(bvalid, dev))
    dense = (kind == "dense" and case != "all_null") or (kind == "sparse" and case == "one_row")   # range of 1
    assert tab.kind == ("dense" if dense else "hash")
    assert int(tab.ovf[0]) == 0
    for n in (1, 3, 1025, N):
        pkeys, pvalid = _probe_side(rng, bkeys, bvalid, n)
        for use_valid in (True, False):
            pv = pvalid if use_valid else None
            ri, cnt, slot = K.join_probe(_t(pkeys, dev), None if pv is None else _t(pv, dev), tab, want_cnt=True,
                                         want_slot=True)
            eri, ecnt = RR.ref_join(bkeys, bvalid, pkeys, pv)
            assert np.array_equal(ri.cpu().numpy(), eri)
            assert np.array_equal(cnt.cpu().numpy(), ecnt)
            s = slot.cpu().numpy()
            hit = eri >= 0
            assert (s[~hit] == -1).all() and (s[hit] >= 0).all() and (s[hit] < tab.nslots).all()
            if hit.any():                                   # slots are equal exactly when keys are
                pairs = np.unique(np.stack([s[hit], pkeys[hit]], 1), axis=0)
                assert len(pairs) == len(np.unique(s[hit])) == len(np.unique(pkeys[hit]))
            assert np.array_equal(tab.bcnt[slot[_t(hit, dev)]].cpu().numpy(), ecnt[hit])
            ri2, cnt2, slot2 = K.join_probe(_t(pkeys, dev), None if pv is None else _t(pv, dev), tab)
            assert torch.equal(ri2, ri) and cnt2 is None and slot2 is None


# ---------------------------------------------------------------------------------------------- pack_keys
PACK_DT = [np.uint8, np.bool_, np.int16, np.int32, np.int64, np.int8]


def _pack_columns(rng, ncols, n, first_dt):
    cols = []
    for j in range(ncols):
        dt = PACK_DT[(first_dt + j) % len(PACK_DT)]
        if dt == np.bool_:
            lo, hi = 0, 1
        elif dt == np.uint8:
            lo, hi = 200, 255
        elif dt == np.int64:
            lo, hi = -(1 << 40) - 7, -(1 << 40) + 90
        elif dt == np.int32:
            lo, hi = -(1 << 31), -(1 << 31) + 60
        else:
            lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).min) + 100
        v = rng.integers(lo, hi + 1, n).astype(dt)
        m = None if j % 3 == 0 else rng.random(n) < 0.8
        if j == 4:
            m = np.zeros(n, bool)                  # an all-null column
        cols.append((v, m, lo, hi - lo + 2))
    return cols


@pytest.mark.parametrize("first_dt", [0, 3])
@pytest.mark.parametrize("ncols", range(1, 9))
def test_pack_keys_matches_the_mixed_radix_reference(dev, ncols, first_dt):
    rng = np.random.default_rng(20 + ncols)
    for n in (1, 4099):
        cols = _pack_columns(rng, ncols, n, first_dt)
        prod = 1
        for c in cols:
            prod *= c[3]
        assert prod < (1 << 62)
        got = K.pack_keys([(_t(v, dev), None if m is None else _t(m, dev), lo, rdx) for v, m, lo, rdx in cols], n, dev)
        assert got.cpu().tolist() == RR.ref_pack(cols)


@pytest.mark.parametrize("ncols", [9, 12, 17])
def test_pack_keys_packs_more_than_eight_columns_in_stages(dev, ncols):
    rng = np.random.default_rng(21)
    n = 4099
    cols = []
    for j in range(ncols):
        v = rng.integers(-2, 3, n).astype(PACK_DT[2 + j % 4])
        cols.append((v, None if j % 2 else rng.random(n) < 0.8, -2, 6))
    assert 6 ** ncols < (1 << 62)
    got = K.pack_keys([(_t(v, dev), None if m is None else _t(m, dev), lo, rdx) for v, m, lo, rdx in cols], n, dev)
    assert got.cpu().tolist() == RR.ref_pack(cols)


def test_nine_key_columns_on_the_frame_level(spark, monkeypatch):
    """groupBy().count(), dropDuplicates() and an inner join over nine small-integer key columns at 20 000 rows
    (above HASH_MIN_ROWS) equal pandas, and run in the hash tables."""
    seen = {"groups": 0, "join": 0}
    hg, jt = K.hash_groups, K.join_table

    def hash_groups(*a, **k):
        seen["groups"] += 1
        return hg(*a, **k)

    def join_table(*a, **k):
        seen["join"] += 1
        return jt(*a, **k)
    monkeypatch.setattr(K, "hash_groups", hash_groups)
    monkeypatch.setattr(K, "join_table", join_table)
    rng = np.random.default_rng(22)
    n = 20_000
    names = [f"c{j}" for j in range(9)]
    pdf = pd.DataFrame({c: rng.integers(0, 3, n).astype(np.int32 if j % 2 else np.int64)
                        for j, c in enumerate(names)})
    df = spark.createDataFrame(pdf)
    got = df.groupBy(*names).count().toPandas()
    assert seen["groups"] == 1
    ref = pdf.groupby(names).size().reset_index(name="count")
    assert got[names].values.tolist() == ref[names].values.tolist()         # tuple order
    assert got["count"].tolist() == ref["count"].tolist()
    dd = df.dropDuplicates().toPandas()
    assert seen["groups"] == 2
    assert sorted(map(tuple, dd[names].values.tolist())) == \
        sorted(map(tuple, pdf.drop_duplicates().values.tolist()))
    left = pdf.assign(a=np.arange(n))
    right = pdf.iloc[: n // 2].drop_duplicates().assign(b=lambda d: np.arange(len(d)))
    j = spark.createDataFrame(left).join(spark.createDataFrame(right), on=names).toPandas()
    assert seen["join"] == 1
    rj = left.merge(right, on=names).sort_values(["a", "b"])
    assert j["a"].tolist() == rj["a"].tolist() and j["b"].tolist() == rj["b"].tolist()


# ------------------------------------------------------------------------------- group_sum / group_first
@pytest.mark.parametrize("G", [1, 50, 8192])
@pytest.mark.parametrize("n", [16_384, N])
def test_grouped_reduce_matches_numpy(dev, n, G):
    rng = np.random.default_rng(23)
    used = np.arange(G) if G == 1 else np.setdiff1d(np.arange(G), np.arange(1, G, 5))   # every fifth group empty
    for hot in (False, True):
        gid = used[rng.integers(0, len(used), n)]
        if hot:
            gid[rng.random(n) < 0.9] = used[-1]
        vals = RR.exact_values(rng, n, np.float64)
        gd, vd = _t(gid, dev), _t(vals, dev)
        esum = np.zeros(G)
        np.add.at(esum, gid, vals)                      # exact: any order gives these bits
        ecnt = np.bincount(gid, minlength=G).astype(np.float64)
        efirst = np.full(G, n, dtype=np.int64)
        np.minimum.at(efirst, gid, np.arange(n))
        assert G == 1 or (efirst == n).any()
        for got, exp in ((R._grouped(0, vd, gd, G), esum), (R._grouped(0, None, gd, G), ecnt),
                         (R._grouped(1, None, gd, G), efirst)):
            assert isinstance(got, torch.Tensor), "the grouped kernel did not run"
            assert got.dtype == (torch.float64 if exp.dtype == np.float64 else torch.int64)
            assert np.array_equal(got.cpu().numpy(), exp)
        assert np.array_equal(K.group_sum(vd, gd, G).cpu().numpy(), esum)
        assert np.array_equal(K.group_sum(None, gd, G).cpu().numpy(), ecnt)
        assert np.array_equal(K.group_first(gd, G).cpu().numpy(), efirst)


# ----------------------------------------------------------------------------------------- bucket_compact
@pytest.mark.parametrize("n", [1, 63, 64, 65, N])
@pytest.mark.parametrize("nb", [1, 16, 17, 64, 255])
def test_bucket_compact_every_bucket_count(dev, nb, n):
    """Both bucket paths (counters in registers up to 16 buckets, per-wave election above) at wave-size edges."""
    rng = np.random.default_rng(24)
    random = rng.integers(0, nb + 1, n)
    random[rng.random(n) < 0.3] = 0
    cases = {"random": random, "none": np.zeros(n, np.int64), "one": np.full(n, 1 + nb // 2),
             "last": np.where(rng.random(n) < 0.5, nb, 0)}
    for name, keep in cases.items():
        keep = keep.astype(np.uint8)
        idx, counts = K.bucket_compact(_t(keep, dev), nb)
        eidx, ecounts = RR.ref_bucket_compact(keep, nb)
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), eidx), name
        assert counts.cpu().tolist() == ecounts.tolist(), name


# -------------------------------------------------------------------------------------------- dict_encode
def _encode_check(vals, dev):
    import pyarrow as pa
    arr = pa.array(vals, type=pa.string())
    codes, valid, dic = K.dict_encode(arr, dev)
    ok = np.array([v is not None for v in vals], dtype=bool)
    present = sorted(set(v for v in vals if v is not None))
    assert dic.tolist() == present
    c = codes.cpu().numpy()
    assert c.dtype == np.int32 and (c[~ok] == -1).all()
    assert [dic[i] for i in c[ok]] == [v for v in vals if v is not None]
    if ok.all():
        assert valid is None
    else:
        assert np.array_equal(valid.cpu().numpy(), ok)


def test_dict_encode_edges(dev):
    _encode_check(["solo"], dev)
    _encode_check([""], dev)
    _encode_check([None], dev)
    _encode_check([None] * 300, dev)
    _encode_check(["same"] * 5000, dev)
    _encode_check(["", None, "", None, "a", ""] * 50, dev)
    prefix = "p" * 40
    tails = [chr(0x30 + i) for i in range(70)] + [chr(0x100 + i) for i in range(1930)]   # 1- and 2-byte tails
    strs = [prefix + t for t in tails]
    assert len(set(strs)) == 2000 and all(s.encode()[:40] == prefix.encode() for s in strs)
    rng = np.random.default_rng(25)
    _encode_check([strs[i] for i in rng.integers(0, 2000, 30_000)] + strs, dev)
