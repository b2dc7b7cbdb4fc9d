"""Independent references, inputs and shape tables for K1 gram (csrc/kernels/gram.hip).

Plain numpy on the CPU, nothing from ``cdnaml.ops.kernels``.  Two kinds of input:

* ``exact_case``: small integers, exact in bf16 and fp32, with an integer reference.  As long as no entry's sum of
  absolute products reaches 2^24 every fp32 partial sum is an integer below 2^24 in whatever order the kernel adds,
  so the kernel must return the reference bit for bit: a lost, doubled or misplaced row or column cannot hide in a
  tolerance.
* ``real_case``: normal data with a wide (``np.longdouble``) reference and a derived entrywise bound.

D = d + 2 columns [X - shift | 1 | y - yshift], T = ceil(D / 32) tiles, k = T (T + 1) / 2 tile pairs.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

LD = np.longdouble
EXACT_LIMIT = 1 << 24

# ------------------------------------------------------------------------------------------------ shape tables
# direct kernel (bf16, ldx == d, d % 4 == 0, d <= 108): both sides of every CPW step and the last direct width
DIRECT_D = [4, 28, 32, 44, 48, 60, 64, 76, 80, 92, 96, 108]
# fewer tiles than ring stages, multiples of the 64-row tile and +-1, the 5-stage ring wrapping, two blocks
DIRECT_N = [1, 63, 64, 65, 191, 192, 193, 64 * 6 + 1, 4096, 4097]
# stream kernel: (d, ldx); PW 1..4 and both NI
STREAM_DL = [(8, 12), (60, 64), (92, 96), (108, 112), (112, 112), (124, 124), (128, 128), (132, 132), (156, 156)]
STREAM_N = [1, 64, 65, 4097, 262145]      # the last: 65 blocks, the final one holds a single row
# tiled bf16 kernel: (d, ldx, misaligned operand)
TILED_D = [1, 7, 30, 31, 62, 63, 94, 101, 159, 200, 510]
TILED_CASES = [(d, d, None) for d in TILED_D] + [(100, 101, None), (100, 100, "X"), (100, 100, "shift")]
TILED_N = [1, 63, 65, 8193]
# f32 kernel: d = 158 is T = 5, 15 pairs in 2 groups of 8 (one padded pair); (d, ldx)
F32_D = [1, 30, 31, 62, 94, 126, 158, 190, 222, 510]
F32_DL = [(d, d) for d in F32_D] + [(30, 33), (158, 161)]
F32_N = [1, 3, 4, 5, 1000, 8193, 32769]


def tiles(d):
    T = (d + 2 + 31) // 32
    return T, T * (T + 1) // 2


def expected_plan(kernel, d):
    """(kernel, p, q) as K.gram_plan reports them, from the dispatch rules in the issue's path table."""
    T, k = tiles(d)
    if kernel == "direct":
        return kernel, -(-k // 4), max(2, -(-(d // 4 + 1) // 4))
    if kernel == "stream":
        return kernel, -(-k // 4), 2 if d >= 132 else 1
    groups = -(-k // (4 if kernel == "tiled" else 8))
    return kernel, -(-k // groups), 0


def direct_capped_n(cu_count):
    """More 4096-row units than CUs with an odd tail: the block count is capped and rows_per_unit rounded up."""
    return 4096 * cu_count + 4097


# ------------------------------------------------------------------------------------------------ bf16
def bf16_round(a):
    """fp32 array -> the fp32 value of its bf16 rounding (round to nearest even on the bit pattern; finite input)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------ exact cases
ExactCase = namedtuple("ExactCase", "X d shift y yshift M")


def _int_gram(Z):
    """Z^T Z in int64 for an integer-valued array Z [n, D] with |Z| <= 8.  The products of a chunk of 2^16 rows are
    summed by the fp64 GEMM -- every partial sum of a chunk is an integer below 2^22, exact in fp64 in any order --
    and the chunks are added in int64."""
    D = Z.shape[1]
    G = np.zeros((D, D), dtype=np.int64)
    for r0 in range(0, Z.shape[0], 1 << 16):
        Zc = Z[r0:r0 + (1 << 16)].astype(np.float64)
        G += np.rint(Zc.T @ Zc).astype(np.int64)
    return G


def exact_case(n, d, ldx=None, seed=0, small=None):
    """Integer inputs for an n x d problem stored with row stride ldx: X in [-3, 3] ({-1, 0, 1, 2} when ``small``,
    the default past 10^6 rows), column c offset by c (r mod 5) before the wrap so no two rows or columns are alike;
    shift in [-1, 1]; y in [-2, 2]; yshift = 1.  M is the int64 moment matrix of the raw [X | 1 | y], from which
    ``exact_ref`` derives every shifted variant.  Asserts the 2^24 precondition of every variant in VARIANTS."""
    ldx = d if ldx is None else ldx
    small = n > 10 ** 6 if small is None else small
    rng = np.random.default_rng(100003 * seed + 7919 * (n % 10007) + 31 * d + ldx)
    span, low = (4, -1) if small else (7, -3)
    X = rng.integers(0, span, size=(n, ldx), dtype=np.int8)
    X += (np.arange(ldx, dtype=np.int16)[None, :] * (np.arange(n) % 5).astype(np.int16)[:, None] % span).astype(np.int8)
    X = (X % span + low).astype(np.float32)
    shift = rng.integers(-1, 2, size=d).astype(np.float32)
    y = rng.integers(-2, 3, size=n).astype(np.float32)
    Z = np.concatenate([X[:, :d], np.ones((n, 1), np.float32), y[:, None]], axis=1)
    case = ExactCase(torch.from_numpy(X), d, torch.from_numpy(shift), torch.from_numpy(y), 1.0, _int_gram(Z))
    for v in VARIANTS:
        exact_ref(case, *v)
    return case


def exact_ref(case, use_y=True, use_shift=True, use_yshift=True):
    """The Gram of [X - shift | 1 | y - yshift] as an fp64 tensor, from int64 arithmetic alone.  With t the column
    offsets (-shift, 0, -yshift), A = Z + 1 t^T, so G = M + m1 t^T + t m1^T + n t t^T for m1 = Z^T 1 (the ones
    column of M); without y the last row and column are zero.  Asserts max_ij sum_r |a_ri a_rj| < 2^24: by
    Cauchy-Schwarz that maximum sits on the diagonal, where it is G_ii itself."""
    d, M = case.d, case.M
    t = np.zeros(d + 2, dtype=np.int64)
    if use_shift:
        t[:d] = -case.shift.numpy().astype(np.int64)
    if use_y and use_yshift:
        t[d + 1] = -int(case.yshift)
    m1, n = M[:, d], int(M[d, d])
    G = M + np.outer(m1, t) + np.outer(t, m1) + n * np.outer(t, t)
    if not use_y:
        G[d + 1, :] = 0
        G[:, d + 1] = 0
    assert int(np.diag(G).max()) < EXACT_LIMIT, (n, d, int(np.diag(G).max()))
    return torch.from_numpy(G.astype(np.float64))


def exact_ref_direct(case, use_y=True, use_shift=True, use_yshift=True):
    """The same Gram by forming the integer augmented matrix and multiplying it in int64 (small cases: the integer
    matmul is slow).  Checks ``exact_ref``'s algebra."""
    d = case.d
    X = case.X.numpy()[:, :d].astype(np.int64)
    n = X.shape[0]
    A = np.zeros((n, d + 2), dtype=np.int64)
    A[:, :d] = X - (case.shift.numpy().astype(np.int64)[None, :] if use_shift else 0)
    A[:, d] = 1
    if use_y:
        A[:, d + 1] = case.y.numpy().astype(np.int64) - (int(case.yshift) if use_yshift else 0)
    return torch.from_numpy((A.T @ A).astype(np.float64))


# the (y, shift, yshift) variants every exact test runs: all present; no y; no shift; neither; y with yshift = 0
VARIANTS = [(True, True, True), (False, True, False), (True, False, True), (False, False, False), (True, True, False)]


def variant_args(case, use_y, use_shift, use_yshift, to=lambda t: t):
    """(y, shift, yshift) arguments of K.gram for one variant; ``to`` moves the tensors to the device."""
    return (to(case.y) if use_y else None, to(case.shift) if use_shift else None,
            case.yshift if (use_y and use_yshift) else 0.0)


# ------------------------------------------------------------------------------------------------ real cases
RealCase = namedtuple("RealCase", "X d shift y yshift ref bound sum_abs")


def real_data(n, d, ldx=None, seed=0):
    """X[:, c] = randn (1 + c / d) + 0.5 (fp32, row stride ldx), shift = the fp32 mean of the first 64 rows,
    y = fp32 randn, yshift = 0.25."""
    ldx = d if ldx is None else ldx
    g = torch.Generator().manual_seed(9000 * seed + 17 * (n % 10007) + d + 3 * ldx)
    X = (torch.randn(n, ldx, generator=g, dtype=torch.float64) *
         (1.0 + torch.arange(ldx, dtype=torch.float64) / d) + 0.5).float()
    shift = X[:64, :d].double().mean(0).float()
    y = torch.randn(n, generator=g, dtype=torch.float64).float()
    return X, shift, y, 0.25


@functools.lru_cache(maxsize=16)
def real_case(n, d, ldx=None, seed=0, bf16=False):
    """Inputs, reference and bound of one real-valued case (n <= 4096).

    Reference: a = x - s in fp32 (one rounding, as the kernel does), rounded to bf16 for the bf16 kernels; products
    and sums in np.longdouble, rounded once to fp64.  bound_ij = (n + 8) 2^-24 sum_r |a_ri a_rj|: a product of fp32
    values is rounded once inside the MFMA (a product of bf16 values is exact in fp32), at most n terms are added in
    fp32 in an unknown order (n u sum|ab| to first order, u = 2^-24), then at most 4 fold adds; the fp64 slab sum is
    negligible.  It holds whichever rows a wave owns.

    The tests also require bound < 0.5 / n sum|ab| (half of what one lost row moves an entry by on average), which
    (n + 8) 2^-24 only meets up to n = 2892.  Beyond, the bound is capped at 0.4 / n sum|ab| -- at n = 4096 that
    is 1638 roundings' worth instead of 4104: tighter than the worst case of a 4096-term fp32 chain, which only
    errors that all point the same way would reach."""
    assert n <= 4096
    X, shift, y, yshift = real_data(n, d, ldx, seed)
    A = np.empty((n, d + 2), dtype=np.float32)
    A[:, :d] = X.numpy()[:, :d] - shift.numpy()[None, :]
    A[:, d] = 1.0
    A[:, d + 1] = y.numpy() - np.float32(yshift)
    if bf16:
        A = bf16_round(A)
    Al = A.astype(LD)
    Ab = np.abs(Al)
    D = d + 2
    ref = np.empty((D, D), dtype=np.float64)
    sab = np.empty((D, D), dtype=np.float64)
    for i in range(D):
        ref[i] = (Al[:, i:i + 1] * Al).sum(axis=0).astype(np.float64)
        sab[i] = (Ab[:, i:i + 1] * Ab).sum(axis=0).astype(np.float64)
    bound = min((n + 8) * 2.0 ** -24, 0.4 / n) * sab
    return RealCase(X, d, shift, y, yshift, ref, bound, sab)


def check_real(case, out, n):
    """|out - ref| <= bound entrywise, and the bound is tight enough to see a lost row: below 0.5 / n of sum|ab|."""
    assert (case.bound < 0.5 / n * case.sum_abs)[case.sum_abs > 0].all()
    o = out.detach().cpu().numpy()
    assert o.shape == case.ref.shape and np.isfinite(o).all()
    err = np.abs(o - case.ref)
    worst = float((err / np.maximum(case.bound, 1e-300)).max())
    assert (err <= case.bound).all(), worst
    return worst
