"""CPU pre-checks of the K1 gram references (tests/_gram_refs.py): the exact cases keep their 2^24 precondition, the
host formulations of K.gram agree with the references, and the bf16 rounding is torch's."""
import numpy as np
import pytest
import torch

from tests import _gram_refs as R
from cdnaml.ops import kernels as K

# every (n, d, ldx) of the GPU tables
_TABLES = {
    "direct": [(n, d, d) for n in R.DIRECT_N for d in R.DIRECT_D],
    "stream": [(n, d, ldx) for n in R.STREAM_N for d, ldx in R.STREAM_DL],
    "tiled": [(n, d, ldx) for n in R.TILED_N for d, ldx, _ in R.TILED_CASES],
    "f32": [(n, d, ldx) for n in R.F32_N for d, ldx in R.F32_DL],
}


@pytest.mark.parametrize("table", sorted(_TABLES))
def test_exact_cases_keep_their_precondition(table):
    """exact_case asserts max_ij sum_r |a_ri a_rj| < 2^24 for every variant itself; here it runs for the tables."""
    for n, d, ldx in sorted(set(_TABLES[table])):
        case = R.exact_case(n, d, ldx)
        assert case.X.shape == (n, ldx) and case.X.dtype == torch.float32
        assert case.X.abs().max() <= 3 and case.shift.abs().max() <= 1 and case.y.abs().max() <= 2


@pytest.mark.parametrize("cus", [256, 304])
def test_direct_capped_case_keeps_its_precondition(cus):
    n = R.direct_capped_n(cus)
    assert n > 10 ** 6
    case = R.exact_case(n, 4)
    assert set(case.X.unique().tolist()) == {-1.0, 0.0, 1.0, 2.0}
    assert float(R.exact_ref(case).diagonal().max()) < R.EXACT_LIMIT


@pytest.mark.parametrize("n,d,ldx", [(1, 1, 1), (65, 7, 9), (193, 30, 30), (1000, 100, 104)])
def test_exact_ref_algebra(n, d, ldx):
    """The moment-matrix form of the reference equals the integer matmul of the augmented matrix itself."""
    case = R.exact_case(n, d, ldx)
    for v in R.VARIANTS:
        assert torch.equal(R.exact_ref(case, *v), R.exact_ref_direct(case, *v))
    g = R.exact_ref(case)
    assert g[d, d] == n and torch.equal(g, g.T)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n,d,ldx", [(1, 4, 4), (65, 7, 9), (4097, 100, 104), (8193, 159, 159), (1000, 511, 511)])
def test_host_gram_equals_exact_reference(n, d, ldx, bf16):
    case = R.exact_case(n, d, ldx)
    for v in R.VARIANTS:
        y, sh, ys = R.variant_args(case, *v)
        assert torch.equal(K.gram(case.X[:, :d], y, sh, ys, bf16=bf16), R.exact_ref(case, *v))


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n,d,ldx", [(257, 158, 158), (4096, 101, 101), (257, 108, 112)])
def test_host_gram_within_real_bound(n, d, ldx, bf16):
    """The host formulation rounds a = x - s once to fp32 (and to bf16) like the kernels and multiplies in fp64."""
    case = R.real_case(n, d, ldx, bf16=bf16)
    out = K.gram(case.X[:, :d], case.y, case.shift, case.yshift, bf16=bf16)
    assert R.check_real(case, out, n) < 1e-3     # fp64 products and sums: far inside an fp32 bound


def test_real_bound_sees_a_lost_row():
    """Dropping the last row moves some entry past the bound (the check the bound exists for)."""
    n, d = 4096, 28
    case = R.real_case(n, d, bf16=False)
    out = K.gram(case.X[:n - 1, :d], case.y[:n - 1], case.shift, case.yshift)
    with pytest.raises(AssertionError):
        R.check_real(case, out, n)


def test_bf16_round_matches_torch():
    g = torch.Generator().manual_seed(5)
    bits = torch.randint(0, 2 ** 32, (100000,), generator=g, dtype=torch.int64)
    # exact ties (low half 0x8000) on even and odd kept bits, just below and above a tie, subnormals, signed zeros,
    # the largest finite values (they round to infinity)
    tie = torch.randint(0, 2 ** 16, (2000,), generator=g, dtype=torch.int64) << 16
    sub = torch.randint(0, 2 ** 23, (2000,), generator=g, dtype=torch.int64)
    extra = torch.cat([tie | 0x8000, tie | 0x7FFF, tie | 0x8001, sub, sub | 0x80000000,
                       torch.tensor([0, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x00008000, 0x00018000])])
    u = torch.cat([bits, extra]).numpy().astype(np.uint32)
    a = u.view(np.float32)
    a = a[np.isfinite(a)]
    assert a.size >= 100000
    want = torch.from_numpy(a.copy()).to(torch.bfloat16).float().numpy()
    got = R.bf16_round(a)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
