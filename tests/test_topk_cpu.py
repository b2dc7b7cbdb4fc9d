"""K35 ``als_topk``'s host formulation and ``ALSModel.recommendFor*`` against ``tests/_topk_refs.py``."""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ml.recommendation import ALSModel
from cdnaml.ops import kernels as K
from tests import _topk_refs as R


def rows_on(dev, X, layout="plain"):
    """X on the device; "strided": a column slice of a wider NaN-filled tensor (odd row stride, the pointer off 16-byte
    alignment); "f4": the leading columns of one with four more."""
    Xd = torch.tensor(X, device=dev)
    if layout == "plain":
        return Xd
    lead, extra = (1, 3) if layout == "strided" else (0, 4)
    wide = torch.full((X.shape[0], X.shape[1] + extra), float("nan"), device=dev)
    wide[:, lead:lead + X.shape[1]] = Xd
    return wide[:, lead:lead + X.shape[1]]


def exact_case(dev, ns, nd, r, k, layout, native):
    """Integer factors: values and positions equal the reference, and two calls return the same bits."""
    S, D = R.integer_factors(ns, nd, r)
    args = (rows_on(dev, S, layout), rows_on(dev, D, layout), k)
    (val, idx), again = (K.als_topk(*args, native=native) for _ in range(2))
    assert (val.dtype, idx.dtype, val.device.type) == (torch.float32, torch.int32, torch.device(dev).type)
    rv, ri = R.topk(S, D, k)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy(), rv.astype(np.float32))
    assert torch.equal(val, again[0]) and torch.equal(idx, again[1])


def nan_case(dev, native):
    """A NaN in one destination row: its position is never returned, every other position competes as before."""
    S, D = R.integer_factors(33, 65, 5)
    D[7, 2] = np.nan
    val, idx = K.als_topk(rows_on(dev, S), rows_on(dev, D), 64, native=native)
    rv, ri = R.topk(S, D, 64)
    assert not (ri == 7).any() and (ri[:, -1] >= 0).all()
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy(), rv.astype(np.float32))
    # every destination NaN: nothing qualifies
    val, idx = K.als_topk(rows_on(dev, S), rows_on(dev, np.full_like(D, np.nan)), 3, native=native)
    assert (idx == -1).all() and (val == -np.inf).all()


@pytest.mark.parametrize("ns,nd,r,k,layout", R.EXACT)
def test_host_formulation_is_exact(ns, nd, r, k, layout):
    exact_case("cpu", ns, nd, r, k, layout, True)


def test_host_formulation_chunks_nan_and_range(monkeypatch):
    monkeypatch.setattr(K, "TOPK_HOST_ELEMS", 65 * 8)      # 33 source rows in five passes
    exact_case("cpu", 33, 65, 12, 10, "plain", True)
    nan_case("cpu", True)
    S, D = (torch.zeros((4, 200)), torch.zeros((9, 200)))
    assert K.als_topk_plan(S, D, 100) == {"path": "host"}
    val, idx = K.als_topk(S.double(), D.double(), 100)     # r > 128, k > 64, fp64 factors
    assert idx[:, :9].tolist() == [list(range(9))] * 4 and (idx[:, 9:] == -1).all() and (val[:, 9:] == -np.inf).all()


def test_model_recommendations(spark):
    """Integer factors, ids that are not 0 .. n - 1: ids and ratings in the reference's order (ties to the lower
    position), the subsets equal to the full calls' rows, unknown ids dropped, no -1 id when fewer items exist."""
    uid, iid = np.array([3, 10, 11, 40, 41, 97]), np.array([5, 6, 20, 21, 22, 50, 70, 71])
    U, V = R.integer_factors(len(uid), len(iid), 4, seed=3)
    model = ALSModel(uid, U, iid, V)

    def want(src, S, dst, Dm, k):
        val, idx = R.topk(S, Dm, k)
        return {int(s): [(int(dst[j]), float(v)) for j, v in zip(ri, rv) if j >= 0]
                for s, ri, rv in zip(src, idx, val)}

    def got(df, src_name, dst_name):
        ids = [row[0] for row in df.select(src_name).collect()]
        assert df.columns == [src_name, "recommendations"] and len(ids) == len(df._recs)
        return {int(s): [(rec[dst_name], rec["rating"]) for rec in recs] for s, recs in zip(ids, df._recs)}

    users, items = want(uid, U, iid, V, 3), want(iid, V, uid, U, 2)
    assert got(model.recommendForAllUsers(3), "user", "item") == users
    assert got(model.recommendForAllItems(2), "item", "user") == items
    some_u = spark.createDataFrame(pd.DataFrame({"user": [41, 3, 41, 12]}))
    some_i = spark.createDataFrame(pd.DataFrame({"item": [71, 4, 20]}))
    assert got(model.recommendForUserSubset(some_u, 3), "user", "item") == {u: users[u] for u in (3, 41)}
    assert got(model.recommendForItemSubset(some_i, 2), "item", "user") == {i: items[i] for i in (20, 71)}
    every = got(model.recommendForAllUsers(20), "user", "item")
    assert every == want(uid, U, iid, V, 20) and all(len(v) == len(iid) for v in every.values())
