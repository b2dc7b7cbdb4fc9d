"""``K.linear_step``'s host formulation against ``tests/_linear_refs.py``, its bad-row rule, and ``K.linear_plan`` on
CPU tensors: every shape is "host" there, so the limits of the range themselves are tested on the device only."""
import numpy as np
import pytest
import torch

from cdnaml.ops import kernels as K
from tests import _linear_refs as R


def step(c, X=None, y=None, w=None, **kw):
    binomial = c["W"].shape[0] == 1
    t = [None if a is None else torch.tensor(a) for a in (c["X"] if X is None else X, c["y"] if y is None else y,
                                                          c["w"] if w is None else w)]
    return K.linear_step(t[0], t[1], c["W"][0] if binomial else c["W"], c["b"], t[2], binomial=binomial, **kw)


@pytest.mark.parametrize("d,n,Kn,weighted", [(5, 130, 1, 1), (5, 65, 3, 0), (17, 130, 17, 1), (100, 1025, 3, 1)])
def test_host_matches_reference(d, n, Kn, weighted):
    c = R.case(d, n, Kn, bool(weighted))
    out, pr = step(c), step(c, mode=K.LINEAR_PREDICT)
    R.check_all(f"host d={d} n={n} K={Kn}", c, [t.numpy() for t in out], [t.numpy() for t in pr])


def plant(c):   # one bad row of each kind in (X, y, w); wc: those rows at weight 0 instead
    X, y, w, wc = c["X"].copy(), c["y"].copy(), c["w"].copy(), c["w"].copy()
    X[0, 2], X[17, 4], y[63], y[64], w[129] = np.nan, np.inf, max(c["W"].shape[0], 2), 0.5, np.nan
    wc[[0, 17, 63, 64, 129]] = 0.0
    return X, y, w, wc


@pytest.mark.parametrize("Kn", [1, 3])
def test_host_bad_rows_are_counted_and_add_nothing(Kn):
    c = R.case(5, 130, Kn, True)
    X, y, w, wc = plant(c)
    bad, clean = step(c, X, y, w), step(c, w=wc)
    assert float(bad[3]) == 5 and float(clean[3]) == 0.0
    assert all(torch.equal(u, v) for u, v in zip(bad[:3], clean[:3])) and torch.isfinite(bad[1]).all()


@pytest.mark.parametrize("d,Kn,dt", [(20, 3, "float32"), (20, 3, "float64"), (129, 3, "float32"), (20, 33, "float32")])
def test_plan_reports_host_for_cpu_tensors(d, Kn, dt):
    assert K.linear_plan(torch.zeros((300, d), dtype=getattr(torch, dt)), Kn) == {"path": "host"}
