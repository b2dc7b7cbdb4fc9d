"""CPU half of the level-histogram tests: K.slot_groups against a brute-force grouping, and the host formulation of
K.hist_moments / K.hist_classes / K.hist_codes against the exact references of tests/_hist_refs.py, bit for bit."""
import pytest
import torch

from tests import _hist_refs as R
from cdnaml.ops import kernels as K

# (shape, T, nodes per tree)
LEVELS = [("a", 17, 3), ("b", 1, 2), ("c", 9, 5)]


@pytest.mark.parametrize("max_trees", [None, 1, 3, 8, 16])
@pytest.mark.parametrize("SB", [1, 2, 5, 17, 100])
@pytest.mark.parametrize("shape,T,per", LEVELS + [("a", 16, 1), ("a", 5, 8)])
def test_slot_groups(shape, T, per, SB, max_trees):
    lv = R.level(shape, T, per)
    rows = K.slot_groups(lv.slot_tree, lv.id_tree, SB, max_trees)
    assert rows == R.brute_groups(lv.slot_tree, lv.id_tree, SB, max_trees)
    # the groups tile the slots, none larger than SB slots or max_trees trees
    assert rows[0][0] == 0 and all(a[0] < b[0] <= a[0] + SB for a, b in zip(rows, rows[1:]))
    assert lv.S - rows[-1][0] <= SB
    assert max_trees is None or all(r[2] - r[1] < max_trees for r in rows)


def test_slot_groups_empty():
    assert K.slot_groups([], [], 4) == []


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", ["moments", "v0", "classes"])
@pytest.mark.parametrize("shape,T,per", LEVELS)
def test_host_node_ids(shape, T, per, kind, masked):
    lv = R.level(shape, T, per)
    fm = lv.fmask if masked else None
    if kind == "classes":
        out = K.hist_classes(lv.bins, lv.d, lv.node, lv.weight, lv.label, R.C, lv.build, lv.slot_tree, fm, lv.B)
    else:
        out = K.hist_moments(lv.bins, lv.d, lv.node, lv.weight, lv.v0 if kind == "v0" else None, lv.v1, lv.build,
                             lv.slot_tree, fm, lv.B)
    assert torch.equal(out, R.ref_hist(lv, kind, masked))


@pytest.mark.parametrize("kind,masked", [("moments", True), ("v0", False), ("classes", True)])
@pytest.mark.parametrize("shape,T,per", LEVELS)
def test_host_row_codes(shape, T, per, kind, masked):
    lv = R.level(shape, T, per)
    out = K.hist_codes(1 if kind == "classes" else 0, lv.bins, lv.d, lv.codes, lv.tfirst,
                       lv.v0 if kind == "v0" else None, lv.v1, lv.label, R.C, lv.build, lv.slot_tree, lv.id_tree,
                       lv.fmask if masked else None, lv.B)
    assert torch.equal(out, R.ref_hist(lv, kind, masked))


def test_host_wide_ids():
    """Few slots over 20000 active ids (the level of the GPU test of hist4_kernel's global slot table)."""
    lv = R.level("a", 2, 10000, True)
    out = K.hist_moments(lv.bins, lv.d, lv.node, lv.weight, None, lv.v1, lv.build, lv.slot_tree, lv.fmask, lv.B)
    assert lv.S == 8 and torch.equal(out, R.ref_hist(lv, "moments", True))
    assert float(out[..., 0].sum()) > 0
