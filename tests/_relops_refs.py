"""Plain numpy / Python references for the relational kernels (K16 hashagg.hip / hash.hip and the K19 helpers).

``mix64`` / ``part_of`` / ``pos_of`` replicate the three hash helpers of hashagg.hip bit for bit, so a test can
build keys that land in a chosen partition or table position and count every partition's distinct keys on the
host.  The other references are dictionaries and loops over the rows: slow, obvious, and independent of torch.

Value rules are Spark's: nulls are skipped, a group without a non-null value has "no value" (``None``), NaN is the
greatest value, and -0.0 == 0.0 (``same_value`` compares zeros by value and everything else by bits)."""
import math
import struct

import numpy as np

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
_M64 = (1 << 64) - 1


# ----------------------------------------------------------------------------------------------- hash replicas
def _u64(keys) -> np.ndarray:
    a = np.asarray(keys)
    if a.dtype == np.uint64:
        return a
    return a.astype(np.int64).view(np.uint64)


def mix64(keys) -> np.ndarray:
    """hashagg.hip mix64 (splitmix64 finalizer) of int64 / uint64 keys, as uint64."""
    z = _u64(keys).copy()
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def part_of(h, pbits: int) -> np.ndarray:
    """Partition of a hash: its top ``pbits`` bits (0 partitions bits -> partition 0)."""
    h = np.asarray(h, dtype=np.uint64)
    if pbits == 0:
        return np.zeros(h.shape, dtype=np.int64)
    return (h >> np.uint64(64 - pbits)).astype(np.int64)


def pos_of(h, S: int) -> np.ndarray:
    """Home slot in [0, S) from the low 32 hash bits."""
    h = np.asarray(h, dtype=np.uint64)
    return (((h & np.uint64(0xFFFFFFFF)) * np.uint64(S)) >> np.uint64(32)).astype(np.int64)


def dedup_bucket(keys, pout: int) -> np.ndarray:
    """Output partition of a key in dedup mode: (mix64(k) >> 16) % pout on the low 32 bits of the shifted hash
    (the kernel narrows to uint32 before the modulo)."""
    h = (mix64(keys) >> np.uint64(16)) & np.uint64(0xFFFFFFFF)
    return (h % np.uint64(pout)).astype(np.uint8)


def mix64_int(k: int) -> int:
    """mix64 of one key in Python integers (an independent check of the numpy replica)."""
    z = (k + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def distinct_per_partition(keys, pbits: int) -> np.ndarray:
    """Distinct keys of every partition [2^pbits] (what a partition's table has to hold).  INT64_MIN lives in the
    special slot and does not count."""
    u = np.unique(np.asarray(keys, dtype=np.int64))
    u = u[u != I64_MIN]
    return np.bincount(part_of(mix64(u), pbits), minlength=1 << pbits)


def distinct_per_chunk(keys, rows_per_chunk: int) -> list:
    """Distinct keys (INT64_MIN excluded) of every contiguous chunk of ``rows_per_chunk`` rows."""
    keys = np.asarray(keys, dtype=np.int64)
    out = []
    for r0 in range(0, len(keys), rows_per_chunk):
        u = np.unique(keys[r0:r0 + rows_per_chunk])
        out.append(int((u != I64_MIN).sum()))
    return out


# ------------------------------------------------------------------------------------------------------ values
def _bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def same_value(a, b) -> bool:
    """Equality of two results: None only equals None, NaN equals NaN, zeros compare by value (-0.0 == 0.0),
    every other float by its bits, integers by value."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer)):
        return int(a) == int(b)
    a, b = float(a), float(b)
    if a != a or b != b:
        return a != a and b != b
    if a == 0.0 and b == 0.0:
        return True
    return _bits(a) == _bits(b)


def _sum(vals):
    """Exactly rounded sum; non-finite terms follow IEEE addition (inf - inf and NaN give NaN)."""
    if all(isinstance(v, int) for v in vals):
        return float(sum(vals))
    if any(v != v for v in vals):
        return float("nan")
    pinf, ninf = any(v == math.inf for v in vals), any(v == -math.inf for v in vals)
    if pinf and ninf:
        return float("nan")
    if pinf or ninf:
        return math.inf if pinf else -math.inf
    return math.fsum(vals)


def _spark_key(v):
    return (v != v, v)         # NaN above everything, +inf included


def _py(v):
    if isinstance(v, (np.bool_, bool)):
        return int(v)
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    return v


def ref_groups(keys, values=(), accs=()):
    """{key: dict(cnt, first, last, acc)} for every distinct int64 key.

    values: [(array, valid bool array or None)]; accs: [(op, value index)] with op in sum / min / max / count /
    last.  acc[i] is the i-th accumulator's result: count -> non-null count, last -> the last row (the value index
    is ignored), sum / min / max -> a Python number, or None when the group has no non-null value.  Sums are exact
    (``math.fsum`` / Python integers, returned as float); min / max order NaN above +inf."""
    keys = np.asarray(keys, dtype=np.int64)
    rows = {}
    for r, k in enumerate(keys.tolist()):
        rows.setdefault(k, []).append(r)
    out = {}
    for k, rr in rows.items():
        res = []
        for op, j in accs:
            if op == "last":
                res.append(rr[-1])
                continue
            v, m = values[j]
            nn = [_py(v[r]) for r in rr if m is None or m[r]]
            if op == "count":
                res.append(len(nn))
            elif not nn:
                res.append(None)
            elif op == "sum":
                res.append(_sum(nn))
            elif op == "min":
                res.append(min(nn, key=_spark_key))
            elif op == "max":
                res.append(max(nn, key=_spark_key))
            else:
                raise ValueError(op)
        out[k] = {"cnt": len(rr), "first": rr[0], "last": rr[-1], "acc": res}
    return out


def ref_join(build_keys, build_valid, probe_keys, probe_valid):
    """(first build row, build rows) per probe row; a miss or a null on either side gives (-1, 0)."""
    first, count = {}, {}
    bk = np.asarray(build_keys, dtype=np.int64).tolist()
    for r, k in enumerate(bk):
        if build_valid is not None and not build_valid[r]:
            continue
        first.setdefault(k, r)
        count[k] = count.get(k, 0) + 1
    pk = np.asarray(probe_keys, dtype=np.int64).tolist()
    ri = np.full(len(pk), -1, dtype=np.int64)
    cnt = np.zeros(len(pk), dtype=np.int64)
    for r, k in enumerate(pk):
        if probe_valid is not None and not probe_valid[r]:
            continue
        if k in first:
            ri[r], cnt[r] = first[k], count[k]
    return ri, cnt


def ref_pack(cols):
    """Mixed-radix key word per row in Python integers: cols = [(values, valid or None, lo, radix)], code 0 for a
    null and value - lo + 1 otherwise, the first column most significant."""
    n = len(cols[0][0])
    out = []
    for r in range(n):
        w = 0
        for v, m, lo, radix in cols:
            code = 0 if (m is not None and not m[r]) else int(v[r]) - int(lo) + 1
            assert 0 <= code < radix
            w = w * int(radix) + code
        out.append(w)
    return out


def ref_bucket_compact(keep, nb: int):
    """(row ids grouped by bucket keep - 1, in row order within a bucket; rows per bucket)."""
    keep = np.asarray(keep).astype(np.int64)
    idx = [np.nonzero(keep == b + 1)[0] for b in range(nb)]
    return (np.concatenate(idx) if idx else np.zeros(0, np.int64)).astype(np.int64), \
        np.array([len(i) for i in idx], dtype=np.int64)


def exact_values(rng, n: int, dtype) -> np.ndarray:
    """Values whose fp64 sums are exact in any order: integers of [-2^20, 2^20] (cut to the type's own range for
    the narrow integer types), scaled by 2^-10 for the float types.  Every value is a multiple of 2^-10 below
    2^20 in magnitude, so a sum of n of them needs n * 2^30 < 2^53: exact for n < 2^23 rows."""
    dtype = np.dtype(dtype)
    lo, hi = -(1 << 20), 1 << 20
    if dtype == np.bool_:
        return rng.integers(0, 2, n).astype(np.bool_)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return rng.integers(max(lo, info.min), min(hi, info.max) + 1, n).astype(dtype)
    return (rng.integers(lo, hi + 1, n).astype(np.float64) / 1024.0).astype(dtype)


def ordered_to_float(u: int) -> float:
    """Inverse of hashagg.hip ord_of for one u64 (given as a Python int in [0, 2^64))."""
    b = (~u) & _M64 if not (u >> 63) else u & 0x7FFFFFFFFFFFFFFF
    return struct.unpack("<d", struct.pack("<Q", b))[0]
