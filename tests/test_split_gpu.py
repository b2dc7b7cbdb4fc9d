"""The split-search and split-decode kernels of csrc/kernels/split.hip on the GPU against the independent references
of tests/_split_refs.py (pinned on the host by tests/test_split_cpu.py).

K.split_scan (serial and wave-parallel kernels), K.split_scan_ex and K.split_decode must return the references bit
for bit: inputs are exact or the summation order is fixed, and the references use the kernels' documented operation
order.  The one exception is the entropy gain, whose device log2 need not return numpy's bits: it stays within
``_split_refs.entropy_bound`` and the largest observed fraction of that bound is printed."""
import numpy as np
import pytest
import torch

from tests import _split_refs as R
from cdnaml.ops import _lib, kernels as K

pytestmark = pytest.mark.gpu

KINDS = ((0, False), (1, False), (1, True))
_ratio = {"max": 0.0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def _mask(c, dev):
    return None if c.mask is None else _t(c.mask.view(np.int32), dev)


def _scan(c, p, dev, exact):
    so, tot = K.split_scan(_t(c.H, dev), _t(c.nthr, dev), _mask(c, dev), c.kind, p["min_inst"], p["lam"], p["gamma"],
                           p["mcw"], missing_bin=c.missing, exact=exact)
    return so.cpu().numpy(), tot.cpu().numpy()


def _assert_scan(got, ref, what):
    (so, tot), (out, rtot) = got, ref
    assert np.array_equal(_bits(tot), _bits(rtot)), what
    assert np.array_equal(so[:, 1:3], out[:, 1:3]) and np.array_equal(so[:, 7], out[:, 7]), \
        (what, so[:, [1, 2, 7]], out[:, [1, 2, 7]])
    assert np.array_equal(_bits(so), _bits(out)), (what, so, out)


# ============================================================================================ split_scan
@pytest.mark.parametrize("general", [False, True], ids=["exact", "general"])
@pytest.mark.parametrize("kind,missing", KINDS)
@pytest.mark.parametrize("shape", R.SCAN_SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_split_scan_serial_equals_reference(dev, shape, kind, missing, general):
    """split_scan_kernel: every column of out and tot, nodes without a legal split included.  General fp64
    histograms too: the kernel's sums are sequential, as the reference's."""
    c = R.scan_case(*shape, kind, missing, general)
    for p, ref in zip(c.params, c.refs):
        _assert_scan(_scan(c, p, dev, False), ref, p)


@pytest.mark.parametrize("kind,missing", KINDS)
@pytest.mark.parametrize("shape", R.WAVE_SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_split_scan_exact_equals_reference(dev, shape, kind, missing, monkeypatch):
    """split_scan(exact=True): split_scan_wave_kernel<2> (65..128 bins) and <4> (129..256 bins) with ragged last
    lanes, and the serial kernel for B <= 64 and d > 4096; the serial kernel returns the same bits."""
    monkeypatch.setattr(K, "SPLIT_WAVE", True)
    c = R.scan_case(*shape, kind, missing, False)
    for p, ref in zip(c.params, c.refs):
        got = _scan(c, p, dev, True)
        _assert_scan(got, ref, p)
        ser = _scan(c, p, dev, False)
        assert np.array_equal(_bits(ser[0]), _bits(got[0])) and np.array_equal(_bits(ser[1]), _bits(got[1]))


def test_assembled_level_scans_like_the_built_histograms(dev, monkeypatch):
    """hist_assemble -> split_scan(exact=True): a level of built nodes (int64 fixed point) and parent-minus-sibling
    nodes decides as the reference does on the directly built histograms."""
    monkeypatch.setattr(K, "SPLIT_WAVE", True)
    c = R.scan_case(6, 17, 65, False, 1, True, False)
    # siblings 0/1 (0 built), siblings 2/3 (3 built), 4 and 5 built without a sibling
    slot = np.array([0, -1, -1, 1, 2, 3], dtype=np.int64)
    parent = np.array([0, 0, 1, 1, -1, -1], dtype=np.int64)
    sib = np.array([1, 0, 3, 2, -1, -1], dtype=np.int64)
    raw = c.H.copy()
    raw[..., 1] *= 2.0 ** 14
    assert np.array_equal(raw, np.round(raw))
    Hb = torch.from_numpy(raw[[0, 3, 4, 5]].astype(np.int64))
    prev = torch.from_numpy(np.stack([c.H[0] + c.H[1], c.H[2] + c.H[3]]))
    H = K.hist_assemble(Hb.to(dev), 2.0 ** 14, prev.to(dev), slot, parent, sib)
    assert np.array_equal(_bits(H.cpu().numpy()), _bits(c.H))
    for p, ref in zip(c.params, c.refs):
        so, tot = K.split_scan(H, _t(c.nthr, dev), None, 1, p["min_inst"], p["lam"], p["gamma"], p["mcw"],
                               missing_bin=True, exact=True)
        _assert_scan((so.cpu().numpy(), tot.cpu().numpy()), ref, p)


# ============================================================================================ split_scan_ex
@pytest.mark.parametrize("case", R.EX_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_split_scan_ex_equals_reference(dev, case):
    """split_scan_ex_kernel: feature, position, child counts, totals and category words equal; the gain bit-equal for
    variance and Gini, within the entropy bound for entropy."""
    c = R.ex_case(*case)
    Kc = c.H.shape[-1]
    out, rtot, cat = c.ref
    so, tot, cm = K.split_scan_ex(_t(c.H, dev), _t(c.nthr, dev), _mask(c, dev), c.kind, c.min_inst)
    so, tot = so.cpu().numpy(), tot.cpu().numpy()
    cm = np.ascontiguousarray(cm.cpu().numpy()).view(np.uint32)
    assert np.array_equal(_bits(tot), _bits(rtot))
    assert np.array_equal(so[:, 1:3], out[:, 1:3]), (so[:, :3], out[:, :3])
    assert np.array_equal(_bits(so[:, 1:]), _bits(out[:, 1:]))
    assert np.array_equal(cm, cat)
    fin = np.isfinite(out[:, 0])
    assert np.array_equal(fin, np.isfinite(so[:, 0])) and (so[~fin, 0] == -np.inf).all()
    if c.kind == "entropy":
        diff = float(np.abs(so[fin, 0] - out[fin, 0]).max()) if fin.any() else 0.0
        frac = diff / R.entropy_bound(Kc)
        _ratio["max"] = max(_ratio["max"], frac)
        print(f"{case}: entropy gain |device - reference| = {diff:.3e} = {frac:.3f} of the bound "
              f"(largest so far {_ratio['max']:.3f})")
        assert diff <= R.entropy_bound(Kc), (case, diff, R.entropy_bound(Kc))
    else:
        assert np.array_equal(_bits(so[:, 0]), _bits(out[:, 0])), (so[:, 0], out[:, 0])


def test_invalid_arguments_raise(dev):
    """More than 256 bins or 32 classes, variance with three statistics, a missing bin with the variance gain: the
    launchers refuse (no kernel runs on a shape its shared arrays do not hold)."""
    nthr = torch.ones(2, dtype=torch.int32, device=dev)
    for shape, kind in (((1, 2, 257, 2), "gini"), ((1, 2, 4, 33), "gini"), ((1, 2, 4, 3), "variance")):
        with pytest.raises(RuntimeError, match="cdna_split_scan_ex"):
            K.split_scan_ex(torch.ones(shape, dtype=torch.float64, device=dev), nthr, None, kind, 1.0)
    with pytest.raises(RuntimeError, match="cdna_split_scan"):
        K.split_scan(torch.ones((1, 2, 4, 2), dtype=torch.float64, device=dev), nthr, None, 0, 1.0, missing_bin=True)
    torch.cuda.synchronize()


# ============================================================================================ split_decode
@pytest.mark.parametrize("i", range(len(R.DECODE_CASES)), ids=lambda i: "-".join(str(x) for x in R.DECODE_CASES[i]))
def test_split_decode_equals_reference(dev, i):
    """split_decode_kernel on hand-built decisions: one, two and three 1024-entry scan chunks with a ragged last one,
    trees without active nodes, thresholds at equality, missing-right bin sets, categorical winners, leaf values.
    ``masks`` rows are compared where cat_off >= 0: the others are never written."""
    c = R.decode_case(i)
    dec = K.split_decode(_t(c.so, dev), _t(c.tot, dev), _t(c.a_tree, dev), c.T, c.min_inst, c.min_gain,
                         bool(c.can_level), bool(c.leaf_children), missing_bin=c.missing_bin,
                         leaf_values=c.leaf_values, catm=None if c.catm is None else _t(c.catm, dev),
                         nthr=None if c.nthr is None else _t(c.nthr, dev))
    got = {k: v.cpu().numpy() for k, v in dec.items() if v is not None}
    ref = c.ref
    for k in ("split_feat", "split_bin", "cat_off", "child", "tfirst_next"):
        assert np.array_equal(got[k], ref[k]), k
    rows = ref["cat_off"] >= 0
    assert np.array_equal(np.ascontiguousarray(got["masks"]).view(np.uint32)[rows], ref["masks"][rows])
    if c.leaf_values is None:
        assert dec["lv"] is None
    else:
        assert np.array_equal(got["lv"].view(np.int32), ref["lv"].view(np.int32))
