"""The node-id (hist4.hip) and row-code (hist5.hip) level histograms on the GPU against tests/_hist_refs.py.

Every case first asserts its plan -- the slot groups of K.slot_groups for the SB the wrapper uses, hence the
trees-per-group bucket and the block size its launch instantiates -- then compares with the exact int64 reference
bit for bit.  Every level has done rows (-1 / 0xFF), weight-0 rows and a few rows of weight 255; the last slot group
is partial wherever S is no multiple of SB, and with d = 21 or 100 the last feature group ends inside a mask word."""
import numpy as np
import pytest
import torch

from tests import _hist_refs as R
from cdnaml.ops import _lib, kernels as K

pytestmark = pytest.mark.gpu

KB = 1024
MASKS = [False, True]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()  # must load: no silent fallback on a GPU box
    return torch.device("cuda:0")


def _codes(dev, lv, kind, masked, budget):
    fm = lv.fmask.to(dev) if masked else None
    out = K.hist_codes(1 if kind == "classes" else 0, lv.bins.to(dev), lv.d, lv.codes.to(dev), lv.tfirst,
                       lv.v0.to(dev) if kind == "v0" else None, lv.v1.to(dev), lv.label.to(dev), R.C,
                       lv.build.to(dev), lv.slot_tree, lv.id_tree, fm, lv.B, lds_budget=budget, wmax=255)
    assert out.dtype == torch.float64
    assert torch.equal(out.cpu(), R.ref_hist(lv, kind, masked))


def _nodes(dev, lv, kind, masked, budget):
    fm = lv.fmask.to(dev) if masked else None
    args = (lv.build.to(dev), lv.slot_tree, fm, lv.B)
    if kind == "classes":
        out = K.hist_classes(lv.bins.to(dev), lv.d, lv.node.to(dev), lv.weight.to(dev), lv.label.to(dev), R.C, *args,
                             lds_budget=budget, id_tree=lv.id_tree)
    else:
        out = K.hist_moments(lv.bins.to(dev), lv.d, lv.node.to(dev), lv.weight.to(dev),
                             lv.v0.to(dev) if kind == "v0" else None, lv.v1.to(dev), *args, lds_budget=budget,
                             id_tree=lv.id_tree)
    assert torch.equal(out.cpu(), R.ref_hist(lv, kind, masked))


# ================================================================================================ hist5_kernel
# (shape, T, per, largest trees per group at 12 bytes per bin, at 16 (v0), slot groups at 12): every bucket, through
# 1, 2, 3, 5, 9 and 16 trees per group; T = 17 must split
UNPACKED = [("a", 1, 5, 1, 1, 1), ("a", 2, 3, 2, 2, 1), ("a", 3, 3, 3, 3, 1), ("a", 5, 3, 5, 5, 1),
            ("a", 9, 2, 9, 8, 1), ("a", 16, 1, 16, 12, 1), ("a", 17, 1, 16, 12, 2), ("b", 2, 3, 2, 2, 2),
            ("c", 5, 3, 5, 5, 1)]


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("kind", ["moments", "v0", "classes"])
@pytest.mark.parametrize("shape,T,per,nt12,nt16,ng12", UNPACKED)
def test_hist5_unpacked(dev, monkeypatch, shape, T, per, nt12, nt16, ng12, kind, masked):
    monkeypatch.setattr(K, "HIST5_PACKED", False)
    lv = R.level(shape, T, per)
    SB, rows, nt, bucket, big = R.code_plan(K, lv, kind, 64 * KB, False)
    assert nt == (nt16 if kind == "v0" else nt12) and not big
    if kind != "v0":
        assert len(rows) == ng12
    _codes(dev, lv, kind, masked, 64 * KB)


# ================================================================================================ hist5p / hist5q
# (shape, T, per, budget KB, largest trees per group, 1024-thread blocks): buckets 1, 2, 4, 8 at both block sizes
PACKED = [("a", 1, 5, 64, 1, False), ("a", 2, 3, 64, 2, False), ("a", 3, 3, 64, 3, False), ("a", 5, 3, 64, 5, False),
          ("a", 9, 2, 64, 8, False), ("c", 5, 3, 64, 5, False),
          ("a", 1, 40, 128, 1, True), ("a", 2, 20, 128, 2, True), ("a", 3, 12, 128, 3, True), ("a", 5, 8, 128, 5, True),
          ("b", 1, 5, 128, 1, True), ("c", 8, 4, 128, 8, True)]


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("shape,T,per,budget,nt_want,big_want", PACKED)
def test_hist5p(dev, monkeypatch, shape, T, per, budget, nt_want, big_want, masked):
    monkeypatch.setattr(K, "HIST5_PACKED", True)
    monkeypatch.setattr(K, "HIST5_COMPACT", 0)
    lv = R.level(shape, T, per)
    SB, rows, nt, bucket, big = R.code_plan(K, lv, "moments", budget * KB, True, K.HIST5_PACKED_MAXT)
    assert (nt, big) == (nt_want, big_want)
    _codes(dev, lv, "moments", masked, budget * KB)


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("shape,T,per,budget,nt_want", [("a", 1, 5, 64, 1), ("a", 2, 3, 64, 2), ("a", 3, 3, 64, 3),
                                                        ("a", 5, 3, 64, 5), ("a", 9, 2, 64, 8), ("a", 5, 8, 128, 5),
                                                        ("b", 3, 3, 128, 3), ("c", 8, 4, 128, 8)])
def test_hist5q(dev, monkeypatch, shape, T, per, budget, nt_want, masked):
    monkeypatch.setattr(K, "HIST5_PACKED", True)
    monkeypatch.setattr(K, "HIST5_COMPACT", 2)  # the wave-compacted kernel whatever the plan
    lv = R.level(shape, T, per)
    nt = R.code_plan(K, lv, "moments", budget * KB, True, K.HIST5_PACKED_MAXT)[2]
    assert nt == nt_want
    _codes(dev, lv, "moments", masked, budget * KB)


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("compact", [0, 2])
def test_hist5_packed_16_trees(dev, monkeypatch, compact, masked):
    """The NT = 16 instantiations of hist5p (1024 threads here) and hist5q: only HIST5_PACKED_MAXT = 16 reaches them."""
    monkeypatch.setattr(K, "HIST5_PACKED", True)
    monkeypatch.setattr(K, "HIST5_COMPACT", compact)
    monkeypatch.setattr(K, "HIST5_PACKED_MAXT", 16)
    lv = R.level("a", 16, 2)
    SB, rows, nt, bucket, big = R.code_plan(K, lv, "moments", 128 * KB, True, 16)
    assert (len(rows), nt, bucket, big) == (1, 16, 16, True)
    _codes(dev, lv, "moments", masked, 128 * KB)


# ================================================================================================ hist4 / hist4f
def _node_plan(lv, kind, budget):
    per_slot = 8 * lv.B * R.bytes_per_bin(kind)
    SB = max(1, min(lv.S, budget // per_slot))
    rows = K.slot_groups(lv.slot_tree, lv.id_tree, SB)
    assert len(rows) == -(-lv.S // SB)
    return SB * per_slot, rows, max(r[4] - r[3] for r in rows)


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("lane_map,kind", [(2, "moments"), (2, "v0"), (2, "classes"), (5, "moments"), (5, "classes")])
@pytest.mark.parametrize("shape,T,per", [("a", 3, 3), ("b", 2, 3), ("c", 5, 3)])
def test_hist4(dev, monkeypatch, shape, T, per, lane_map, kind, masked):
    """hist4_kernel (map 2) and hist4f_kernel (map 5, whose LDS slot table holds every group's id span)."""
    monkeypatch.setattr(K, "HIST_MAP", lane_map)
    lv = R.level(shape, T, per)
    planes, rows, span = _node_plan(lv, kind, 8 * KB)
    assert len(rows) > 1 and span <= 16384
    _nodes(dev, lv, kind, masked, 8 * KB)


@pytest.mark.parametrize("masked", MASKS)
def test_hist4_global_slot_table(dev, monkeypatch, masked):
    """20000 active ids in one slot group: more than the 16384-entry LDS slot table, so hist4_kernel reads build_slot
    from global memory (and the fast kernel, which needs the table, is not taken)."""
    monkeypatch.setattr(K, "HIST_MAP", 5)
    lv = R.level("a", 2, 10000, True)
    planes, rows, span = _node_plan(lv, "moments", 64 * KB)
    assert lv.S == 8 and len(rows) == 1 and span == 20000 > 16384
    _nodes(dev, lv, "moments", masked, 64 * KB)


# ================================================================================================ above 64 KB of LDS
def test_hist4f_128k(dev, monkeypatch):
    """25 slots of 3840 bytes in one group: the fast node-id kernel launched with 96000 bytes of planes."""
    monkeypatch.setattr(K, "HIST_MAP", 5)
    lv = R.level("a", 5, 8)
    planes, rows, span = _node_plan(lv, "moments", 128 * KB)
    assert planes > 64 * KB and len(rows) == 1 and span <= 16384
    _nodes(dev, lv, "moments", True, 128 * KB)


def test_hist5_unpacked_128k(dev, monkeypatch):
    """The same level through the unpacked row-code kernel, 96000 bytes of planes."""
    monkeypatch.setattr(K, "HIST5_PACKED", False)
    lv = R.level("a", 5, 8)
    SB, rows, nt, bucket, big = R.code_plan(K, lv, "moments", 128 * KB, False)
    assert SB * 8 * lv.B * 12 > 64 * KB and (len(rows), nt) == (1, 5)
    _codes(dev, lv, "moments", True, 128 * KB)
