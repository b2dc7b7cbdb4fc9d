"""K1 gram on the GPU against the independent references of tests/_gram_refs.py.

Every case first asserts the kernel and template instantiation K.gram_plan reports for its operands (the dispatch's
own host function), so a shape that stops reaching its instantiation fails instead of passing on another path.  The
exact cases are small integers whose Gram every kernel must return bit for bit (see _gram_refs.exact_case)."""
import numpy as np
import pytest
import torch

from tests import _gram_refs as R
from cdnaml.ops import _lib, kernels as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()  # must load: no silent fallback on a GPU box
    return torch.device("cuda:0")


def _offset_copy(t, dev):
    """A device copy of ``t`` that starts one float into its storage (4 bytes past a 16-byte boundary)."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)[1:].view(t.shape)
    buf.copy_(t)
    assert buf.data_ptr() % 16 != 0 and buf.is_contiguous()
    return buf


def _assert_plan(Xd, sh, bf16, kernel, d):
    plan = K.gram_plan(Xd, sh, bf16)
    assert (plan["kernel"], plan["p"], plan["q"]) == R.expected_plan(kernel, d), plan
    assert plan["npairs"] == R.tiles(d)[1]
    return plan


def _exact(dev, case, kernel, bf16, misaligned=None):
    """Every variant of one exact case through K.gram: the expected plan, then the reference bit for bit.  Returns the
    plan of the full variant."""
    d = case.d
    Xd = _offset_copy(case.X, dev) if misaligned == "X" else case.X.to(dev)[:, :d]
    shd = _offset_copy(case.shift, dev) if misaligned == "shift" else case.shift.to(dev)
    yd = case.y.to(dev)
    full = None
    for use_y, use_shift, use_yshift in R.VARIANTS:
        if misaligned == "shift" and not use_shift:
            continue        # without the shift the call is aligned and takes the direct kernel
        sh = shd if use_shift else None
        plan = _assert_plan(Xd, sh, bf16, kernel, d)
        full = full or plan
        out = K.gram(Xd, yd if use_y else None, sh, case.yshift if (use_y and use_yshift) else 0.0, bf16=bf16)
        assert out.dtype == torch.float64 and out.shape == (d + 2, d + 2)
        assert torch.equal(out.cpu(), R.exact_ref(case, use_y, use_shift, use_yshift)), (use_y, use_shift, use_yshift)
    return full


# ============================================================================================ exact, per kernel
@pytest.mark.parametrize("n", R.DIRECT_N)
@pytest.mark.parametrize("d", R.DIRECT_D)
def test_direct_exact(dev, d, n):
    plan = _exact(dev, R.exact_case(n, d), "direct", True)
    assert plan["nblk"] == -(-n // 4096) and plan["nblk"] * plan["rows_per_unit"] >= n


def test_direct_exact_capped_blocks(dev):
    """More 4096-row units than CUs: one block per CU, rows_per_unit rounded up to whole 64-row tiles."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n = R.direct_capped_n(cus)
    plan = _exact(dev, R.exact_case(n, 4), "direct", True)
    assert plan["nblk"] == cus
    assert plan["rows_per_unit"] == -(-(-(-n // cus)) // 64) * 64 and plan["rows_per_unit"] > 4096


@pytest.mark.parametrize("n", R.STREAM_N)
@pytest.mark.parametrize("d,ldx", R.STREAM_DL)
def test_stream_exact(dev, d, ldx, n):
    plan = _exact(dev, R.exact_case(n, d, ldx), "stream", True)
    assert plan["nblk"] == -(-n // 4096)
    if n == 262145:
        assert plan["rows_per_unit"] == 4096        # 64 full blocks and one block of a single row


@pytest.mark.parametrize("n", R.TILED_N)
@pytest.mark.parametrize("d,ldx,misaligned", R.TILED_CASES)
def test_tiled_exact(dev, d, ldx, misaligned, n):
    plan = _exact(dev, R.exact_case(n, d, ldx), "tiled", True, misaligned)
    assert plan["nblk"] == -(-n // 8192) and plan["ngroups"] * plan["p"] >= plan["npairs"]


@pytest.mark.parametrize("n", R.F32_N)
@pytest.mark.parametrize("d,ldx", R.F32_DL)
def test_f32_exact(dev, d, ldx, n):
    plan = _exact(dev, R.exact_case(n, d, ldx), "f32", False)
    assert plan["nblk"] == -(-n // 8192) and plan["nblk"] * 4 * plan["rows_per_unit"] >= n
    if d == 158:
        assert (plan["ngroups"], plan["p"], plan["npairs"]) == (2, 8, 15)      # the last group's 8th pair is padding


# ============================================================================================ limits
@pytest.mark.parametrize("bf16", [False, True])
def test_width_past_the_kernel_limit_takes_the_host_formulation(dev, bf16):
    n, d = 65, 511                                   # d + 2 = 513
    case = R.exact_case(n, d)
    Xd = case.X.to(dev)
    assert K.gram_plan(Xd, case.shift.to(dev), bf16) == {"kernel": "host"}
    assert K.gram_plan(Xd[:, :510], case.shift.to(dev)[:510], bf16)["kernel"] in ("tiled", "f32")    # 512: native
    out = K.gram(Xd, case.y.to(dev), case.shift.to(dev), case.yshift, bf16=bf16)
    assert torch.equal(out.cpu(), R.exact_ref(case))


@pytest.mark.parametrize("bf16", [0, 1])
def test_native_entry_rejects_a_width_past_its_tables(dev, bf16):
    """d + 2 = 545 (more than 17 tiles): hipErrorInvalidValue, and neither the output nor the workspace is touched."""
    n, d = 8, 543
    L = _lib.lib()
    X = torch.zeros(n, d, device=dev)
    out = torch.full((d + 2, d + 2), -7.0, dtype=torch.float64, device=dev)
    ws = torch.full((153 * 1024,), float("nan"), device=dev)
    torch.cuda.synchronize()
    rc = L.cdna_gram(X.data_ptr(), n, d, d, None, None, 0.0, out.data_ptr(), ws.data_ptr(), bf16, None)
    assert rc == 1                                   # hipErrorInvalidValue
    plan = np.full(7, -1, dtype=np.int32)
    assert L.cdna_gram_plan(X.data_ptr(), n, d, d, None, bf16, plan.ctypes.data) == 1 and (plan == -1).all()
    torch.cuda.synchronize()
    assert (out == -7.0).all() and ws.isnan().all()


# ============================================================================================ coverage of the dispatch
def test_tables_reach_every_reachable_instantiation(dev):
    """The plan query over every width, row stride, operand alignment and type (it only looks at the addresses):
    the instantiations a call can reach are exactly those the tables above run.  The other 24 of the 44 that
    cdna_gram's switches name cannot be reached: direct PW and CPW both follow from d (PW 1 with CPW 2..4, PW 2 with
    5..6, PW 3 with 7; never PW 4), stream NI = 2 needs d >= 132 where PW = 4, tiled P = 2 and f32 P = 2, 4 divide
    no pair count."""
    L = _lib.lib()
    out = np.zeros(7, dtype=np.int32)

    def plan(x, n, d, ldx, sh, bf16):
        assert L.cdna_gram_plan(x, n, d, ldx, sh, bf16, out.ctypes.data) == 0
        return K.GRAM_KERNELS[out[0]], int(out[1]), int(out[2])

    reach = {plan(x, n, d, ldx, sh, bf16) for d in range(1, 511) for ldx in (d, d + 1, d + 4)
             for x in (0x10000, 0x10004) for sh in (None, 0x20000, 0x20004) for bf16 in (0, 1) for n in (1, 100000)}
    tables = {R.expected_plan("direct", d) for d in R.DIRECT_D} | {R.expected_plan("stream", d) for d, _ in R.STREAM_DL}
    tables |= {R.expected_plan("tiled", d) for d, _, _ in R.TILED_CASES}
    tables |= {R.expected_plan("f32", d) for d, _ in R.F32_DL}
    assert reach == tables
    assert reach == ({("direct", 1, 2), ("direct", 1, 3), ("direct", 1, 4), ("direct", 2, 5), ("direct", 2, 6),
                      ("direct", 3, 7)} | {("stream", pw, 1) for pw in (1, 2, 3, 4)} | {("stream", 4, 2)} |
                     {("tiled", p, 0) for p in (1, 3, 4)} | {("f32", p, 0) for p in (1, 3, 5, 6, 7, 8)})


# ============================================================================================ path independence
def test_four_paths_agree_bit_for_bit(dev):
    n, d = 4097, 100
    case = R.exact_case(n, d, 104)
    yd, shd = case.y.to(dev), case.shift.to(dev)
    wide = case.X.to(dev)
    operands = {"direct": (wide[:, :d].contiguous(), True), "stream": (wide[:, :d], True),
                "tiled": (_offset_copy(case.X[:, :d].contiguous(), dev), True), "f32": (wide[:, :d], False)}
    outs = {}
    for kernel, (Xd, bf16) in operands.items():
        _assert_plan(Xd, shd, bf16, kernel, d)
        outs[kernel] = K.gram(Xd, yd, shd, case.yshift, bf16=bf16)
    for kernel in ("stream", "tiled", "f32"):
        assert torch.equal(outs[kernel], outs["direct"]), kernel
    assert torch.equal(outs["direct"].cpu(), R.exact_ref(case))


# ============================================================================================ real-valued accuracy
# the widest instantiation of each kernel: (kernel, d, ldx, bf16)
WIDEST = [("direct", 108, 108, True), ("stream", 156, 156, True), ("tiled", 101, 101, True), ("f32", 158, 158, False)]


@pytest.mark.parametrize("n", [257, 4096])
@pytest.mark.parametrize("kernel,d,ldx,bf16", WIDEST)
def test_real_valued_within_derived_bound(dev, kernel, d, ldx, bf16, n):
    """|out - ref| <= bound entrywise against the np.longdouble reference; check_real also asserts that the bound is
    below 0.5 / n of sum|ab|, so a lost row could not pass."""
    case = R.real_case(n, d, ldx, bf16=bf16)
    Xd, shd = case.X.to(dev)[:, :d], case.shift.to(dev)
    _assert_plan(Xd, shd, bf16, kernel, d)
    out = K.gram(Xd, case.y.to(dev), shd, case.yshift, bf16=bf16)
    worst = R.check_real(case, out, n)
    print(f"gram {kernel} n={n} d={d}: largest error / bound = {worst:.4f}")


# ============================================================================================ workspace
# an n whose last unit (block; wave for f32) is short: (kernel, n, d, ldx, bf16)
SHORT_LAST = [("direct", 4097, 100, 100, True), ("stream", 4097, 100, 104, True), ("tiled", 8193, 101, 101, True),
              ("f32", 8193, 158, 158, False)]


@pytest.mark.parametrize("kernel,n,d,ldx,bf16", SHORT_LAST)
def test_poisoned_workspace(dev, monkeypatch, kernel, n, d, ldx, bf16):
    """The workspace arrives full of NaN with a NaN guard band behind it: every slab the reduction reads has been
    written (the result is exact), nothing past the plan's nblk x npairs slabs is written."""
    case = R.exact_case(n, d, ldx)
    Xd, yd, shd = case.X.to(dev)[:, :d], case.y.to(dev), case.shift.to(dev)
    plan = _assert_plan(Xd, shd, bf16, kernel, d)
    ws_n = _lib.lib().cdna_gram_workspace(n, d, int(bf16))
    used = plan["nblk"] * plan["npairs"] * 1024
    assert used <= ws_n
    guard = 4096
    real_empty = torch.empty
    poisoned = []

    def nan_empty(*a, **kw):
        if kw.get("dtype") == torch.float32 and len(a) == 1 and a[0] == ws_n:
            t = real_empty(ws_n + guard, **kw)
            t.fill_(float("nan"))
            poisoned.append(t)
            return t[:ws_n]
        return real_empty(*a, **kw)

    monkeypatch.setattr(K.torch, "empty", nan_empty)
    out = K.gram(Xd, yd, shd, case.yshift, bf16=bf16)
    monkeypatch.undo()
    assert len(poisoned) == 1
    o = out.cpu()
    assert o.isfinite().all() and torch.equal(o, R.exact_ref(case))
    ws = poisoned[0].cpu()
    assert not ws[:used].isnan().any()               # whole slabs are written, padding rows and columns included
    assert ws[used:].isnan().all()                   # the unused tail of the workspace and the guard band


# ============================================================================================ reruns
# real-valued, several blocks: (kernel, n, d, ldx, bf16)
RERUN = [("direct", 20001, 108, 108, True), ("stream", 20001, 156, 156, True), ("tiled", 20001, 101, 101, True),
         ("f32", 20001, 158, 158, False)]


@pytest.mark.parametrize("kernel,n,d,ldx,bf16", RERUN)
def test_rerun_is_bit_identical(dev, kernel, n, d, ldx, bf16):
    X, shift, y, yshift = R.real_data(n, d, ldx)
    Xd, yd, shd = X.to(dev)[:, :d], y.to(dev), shift.to(dev)
    plan = _assert_plan(Xd, shd, bf16, kernel, d)
    assert plan["nblk"] > 1
    first = K.gram(Xd, yd, shd, yshift, bf16=bf16)
    second = K.gram(Xd, yd, shd, yshift, bf16=bf16)
    assert first.isfinite().all() and torch.equal(first, second)
