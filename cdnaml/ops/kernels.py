"""Tensor-level entry points for every native kernel (SURVEY §2.10 K1–K15).

Each op dispatches on the device of its inputs:

* device tensors (ROCm/HIP) -> the hand-written gfx950 kernel in
  ``csrc/kernels`` via :mod:`cdnaml.ops._lib` (fails loudly if the library
  cannot be built/loaded);
* CPU tensors -> a plain PyTorch reference implementation of the same op.
  These references define the semantics and are the oracles of the GPU
  numerics tests (tests/test_kernels_gpu.py).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from . import philox as _philox


from ._base import _TORCH_DT, _native, _ptr, _stream, upload  # noqa: F401


# --------------------------------------------------------------------- K1
def _gram_operands(X: torch.Tensor, shift: Optional[torch.Tensor]):
    """The fp32 X (unit column stride) and shift tensors whose pointers K1 is called with."""
    if X.dtype != torch.float32:
        X = X.float()
    X = X if X.stride(1) == 1 else X.contiguous()
    return X, None if shift is None else shift.float().contiguous()


GRAM_KERNELS = ("direct", "stream", "tiled", "f32")


def gram_plan(X: torch.Tensor, shift: Optional[torch.Tensor] = None, bf16: bool = False) -> Dict[str, object]:
    """What :func:`gram` runs for these operands, from the dispatch's own host function (nothing is launched):
    ``kernel`` (one of GRAM_KERNELS, or "host" where gram takes the library GEMM), ``p`` (tile pairs per wave of the
    direct and stream kernels, per block of the tiled and f32 ones), ``q`` (DMA chunks per wave of the direct kernel,
    load items per thread of the stream kernel, else 0), ``nblk``, ``ngroups``, ``rows_per_unit`` (rows per block;
    per wave for f32) and ``npairs``."""
    n, d = X.shape
    if X.dtype == torch.float64 or not _native(X) or d + 2 > 512:
        return {"kernel": "host"}
    X, sh = _gram_operands(X, shift)
    out = np.zeros(7, dtype=np.int32)
    _lib.check(_lib.lib().cdna_gram_plan(_ptr(X), n, d, X.stride(0), _ptr(sh), int(bf16), out.ctypes.data),
               "cdna_gram_plan")
    kern, p, q, nblk, ngroups, rpu, npairs = (int(v) for v in out)
    return {"kernel": GRAM_KERNELS[kern], "p": p, "q": q, "nblk": nblk, "ngroups": ngroups, "rows_per_unit": rpu,
            "npairs": npairs}


def gram(X: torch.Tensor, y: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
         yshift: float = 0.0, bf16: bool = False, fp64: bool = False) -> torch.Tensor:
    """Return A^T A (float64, (d+2)x(d+2)) for A = [X - shift | 1 | y - yshift].

    Column d is the intercept column of ones; column d+1 is y (zeros if None).
    fp64: the fp32 augmented matrix multiplied in fp64 by the library GEMM (the CPU path's arithmetic) instead of
    the K1 MFMA kernel.
    """
    n, d = X.shape
    if X.dtype == torch.float64:
        # Spark's Double vectors (course scale): the augmented matrix is formed and multiplied in fp64 as is --
        # no fp32 rounding of the features (the shift is the caller's fp32-rounded value, used exactly)
        A = torch.empty((n, d + 2), dtype=torch.float64, device=X.device)
        A[:, :d] = X if shift is None else X - shift.double()
        A[:, d] = 1.0
        A[:, d + 1] = 0.0 if y is None else (y.double() - yshift)
        return A.T @ A
    if X.dtype != torch.float32:
        X = X.float()
    if _native(X) and d + 2 <= 512 and not fp64:
        X, sh = _gram_operands(X, shift)
        y32 = None if y is None else y.float().contiguous()
        L = _lib.lib()
        ws_n = L.cdna_gram_workspace(n, d, int(bf16))
        ws = torch.empty(max(ws_n, 1), dtype=torch.float32, device=X.device)
        out = torch.zeros((d + 2, d + 2), dtype=torch.float64, device=X.device)
        _lib.check(L.cdna_gram(_ptr(X), n, d, X.stride(0), _ptr(y32), _ptr(sh), float(yshift), _ptr(out), _ptr(ws),
                               int(bf16), _stream(X.device)), "cdna_gram")
        return out
    A = torch.empty((n, d + 2), dtype=torch.float32, device=X.device)
    A[:, :d] = X if shift is None else X - shift.float()
    A[:, d] = 1.0
    A[:, d + 1] = 0.0 if y is None else (y.float() - yshift)
    if bf16:
        A = A.to(torch.bfloat16)
    A = A.double()
    return A.T @ A


# -------------------------------------------------------------------- K15
def uniform(n: int, seed: int, offset: int = 0, stream: int = 0, device=None) -> torch.Tensor:
    """Philox uniform doubles keyed by (seed, offset+i, stream)."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if device.type == "cuda":
        out = torch.empty(n, dtype=torch.float64, device=device)
        _lib.check(_lib.lib().cdna_uniform(_ptr(out), n, seed, int(offset), int(stream) & 0xFFFFFFFF,
                                           _stream(device)), "cdna_uniform")
        return out
    return torch.from_numpy(_philox.uniform(n, seed, int(offset), int(stream)))


def normal32_(out: torch.Tensor, seed: int, offset: int = 0, stream: int = 0) -> torch.Tensor:
    """Fill the contiguous fp32 tensor ``out`` with standard normals for global elements offset..offset+numel-1
    (Philox quads, Box-Muller; ``normal_f32_kernel``).  CPU: the numpy oracle ``philox.normal32``."""
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("normal32_ needs a contiguous float32 tensor")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if out.is_cuda:
        _lib.check(_lib.lib().cdna_normal_f32(_ptr(out), out.numel(), seed, int(offset), int(stream) & 0xFFFFFFFF,
                                              _stream(out.device)), "cdna_normal_f32")
        return out
    out.view(-1).copy_(torch.from_numpy(_philox.normal32(out.numel(), seed, int(offset), int(stream))))
    return out


def poisson_weights(T: int, n: int, seed: int, offset: int, rate: float, device=None) -> torch.Tensor:
    """uint8 [T, n] Poisson(rate) bootstrap multiplicities, tree t on stream 0x100+t."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if device.type == "cuda":
        out = torch.empty((T, n), dtype=torch.uint8, device=device)
        _lib.check(_lib.lib().cdna_poisson(_ptr(out), T, n, seed, int(offset), float(rate), None, None, 0,
                                           _stream(device)), "cdna_poisson")
        return out
    return torch.from_numpy(_philox.poisson(T, n, seed, int(offset), float(rate)))


POISSON_CODES = True


# where the forest's bootstrap draws run when the level-0 root histogram cannot draw them itself (POISSON_FUSED):
# "main" -- in series before the binning, "side" -- on the side stream at the same point (profiles/r4/prologue_ab.md).
# (An "auto" placement that started small shards' draws on the side stream with the fit measured 17.6 vs 17.5 ms at
# the 8-GPU point's per-rank shape against the fused draws, and was removed.)
POISSON_STREAM = "main"


def poisson_max_draw(rate: float) -> int:
    """The largest bootstrap weight the tabulated Poisson draws can produce at ``rate`` (-1: no static bound)."""
    return int(_lib.lib().cdna_poisson_max_draw(float(rate)))


# level 0 of a bootstrapped forest draws its Poisson weights inside the root histogram kernel (seg.hip RootDraw)
# instead of a draws kernel in series ahead of it
POISSON_FUSED = True


class BootstrapCodes:
    """Poisson bootstrap draws written straight as the tree engine's row codes (GPU): ``codes`` [T, n] int16
    (weight << 8 | 0, 0xFF for weight 0 -- codes_init's format) and the largest weight, copied to the host behind
    the kernel (``wmax()`` waits for that copy only).  ``weights()`` derives the uint8 multiplicities for the
    paths that need them (bit-identical to poisson_weights).

    lazy: nothing is launched yet when the draws have a static bound (``poisson_max_draw``): the trainer's level-0
    root histogram draws and writes the codes itself (``draw_args`` / ``mark_drawn``), any other first reader calls
    ``materialize`` (the draws kernel); ``wmax()`` is then the static bound."""

    def __init__(self, T: int, n: int, seed: int, offset: int, rate: float, device, grid_blocks: int = 0,
                 lazy: bool = False):
        dev = torch.device(device)
        self.T, self.n, self.seed, self.offset, self.rate, self.dev = T, n, int(seed), int(offset), float(rate), dev
        self.codes = torch.empty((T, n), dtype=torch.int16, device=dev)
        self._bound = poisson_max_draw(rate) if lazy else -1
        self.pending = self._bound >= 1
        self._wmax = None
        if not self.pending:
            self._launch(grid_blocks)

    def _launch(self, grid_blocks: int = 0) -> None:
        wm = torch.zeros(1, dtype=torch.int32, device=self.dev)
        _lib.check(_lib.lib().cdna_poisson(None, self.T, self.n, self.seed & 0xFFFFFFFFFFFFFFFF, self.offset,
                                           self.rate, _ptr(self.codes), _ptr(wm), int(grid_blocks),
                                           _stream(self.dev)), "cdna_poisson(codes)")
        self._wmax = _PendingScalar(wm, torch.cuda.current_stream(self.dev))

    def draw_args(self):
        """(seed, row offset, rate) for a kernel that draws the pending codes itself, else None."""
        return (self.seed, self.offset, self.rate) if self.pending else None

    def mark_drawn(self) -> None:
        self.pending = False

    def materialize(self) -> None:
        if self.pending:
            self._launch()
            self.pending = False

    def wmax(self) -> int:
        if self._bound >= 1:
            return self._bound
        return max(1, int(self._wmax.get()))

    def weights(self) -> torch.Tensor:
        self.materialize()
        return ((self.codes.to(torch.int32) >> 8) & 0xFF).to(torch.uint8)


# ------------------------------------------------------- level histogram assembly
def assemble_table(slot: np.ndarray, parent: np.ndarray, sib: np.ndarray) -> np.ndarray:
    """hist_assemble's device table: int32 [A, 3] (slot, parent, sibling), flattened."""
    return np.stack([slot, parent, sib], 1).astype(np.int32).reshape(-1)


def hist_assemble(Hb: torch.Tensor, raw_scale, prev: Optional[torch.Tensor], slot: np.ndarray,
                  parent: np.ndarray, sib: np.ndarray, table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 histograms [A, d, B, K] of a level's active nodes in one launch (split.hip): built node a copies
    Hb[slot[a]] (int64 fixed point when ``raw_scale`` is given: a float divides stat 1, a pair (s0, s1)
    divides stats 0 and 1); a derived node (slot -1) is prev[parent[a]] - (its sibling's built histogram).
    ``table``: assemble_table(slot, parent, sib) already on the device (uploaded with the level's other tables)."""
    A = len(slot)
    nb, d, B, Kc = Hb.shape
    dev = Hb.device
    s0, s1 = raw_scales(raw_scale)
    raw = raw_scale is not None
    if not _native(Hb):
        src = Hb.double()
        if raw:
            src = src.clone()
            src[..., 0] /= s0
            src[..., 1] /= s1
        H = torch.empty((A, d, B, Kc), dtype=torch.float64, device=dev)
        sl = torch.from_numpy(np.asarray(slot, dtype=np.int64))
        built = sl >= 0
        if bool(built.any()):
            H[built] = src[sl[built]]
        der = torch.nonzero(~built).flatten()
        if der.numel():
            par = torch.from_numpy(np.asarray(parent, dtype=np.int64))[der]
            sib_ = torch.from_numpy(np.asarray(sib, dtype=np.int64))[der]
            H[der] = prev[par] - src[sl[sib_]]
        return H
    H = torch.empty((A, d, B, Kc), dtype=torch.float64, device=dev)
    m = table if table is not None else upload(dev, assemble_table(slot, parent, sib))[0]
    src = Hb.contiguous() if raw else Hb.double().contiguous()
    if raw:
        assert Hb.dtype == torch.int64
    pv = None if prev is None else prev.contiguous()
    _lib.check(_lib.lib().cdna_hist_assemble(_ptr(src), int(raw), float(s0), float(s1), _ptr(pv),
                                             _ptr(m), A, d * B * Kc, Kc, _ptr(H), _stream(dev)),
               "cdna_hist_assemble")
    return H


def raw_scales(raw_scale):
    """(scale of stat 0, scale of stat 1) of an int64 fixed-point histogram (1.0 = unscaled)."""
    if raw_scale is None:
        return 1.0, 1.0
    if isinstance(raw_scale, (tuple, list)):
        return float(raw_scale[0]), float(raw_scale[1])
    return 1.0, float(raw_scale)


# --------------------------------------------------------------------- K9
GRAD_HESS_OBJ = {"reg:squarederror": 0, "reg:linear": 0, "reg:absoluteerror": 1, "reg:pseudohubererror": 2,
                 "count:poisson": 3, "binary:logistic": 4, "multi:softprob": 5}


def grad_hess(F: torch.Tensor, y: torch.Tensor, w: Optional[torch.Tensor], obj: int):
    """K9: gradient and hessian [n, K] of objective code ``obj`` (GRAD_HESS_OBJ) at margin F [n, K] (GPU).
    y: float labels (class index for softmax); w: optional float row weights.  max |g| is computed in the same
    pass and attached to g as a pending scalar (``prefetch_max``'s attribute: packed_scale_global reads it)."""
    n, Kc = F.shape
    F = F.float().contiguous()
    y = y.float().contiguous()
    w = None if w is None else w.float().contiguous()
    g = torch.empty_like(F)
    h = torch.empty_like(F)
    bits = torch.empty(1, dtype=torch.int32, device=F.device)
    st = torch.cuda.current_stream(F.device)
    _lib.check(_lib.lib().cdna_grad_hess(_ptr(F), _ptr(y), _ptr(w), n, Kc, int(obj), _ptr(g), _ptr(h), _ptr(bits),
                                         st.cuda_stream), "cdna_grad_hess")
    setattr(g, "_cdna_absmax", _PendingScalar(bits.view(torch.float32), st))
    return g, h


# --------------------------------------------------------------------- K3
QUANTILE_MAX_S = 16384  # sample rows a quantile block sorts in LDS (fp64)


def quantile_thresholds(samp: torch.Tensor, max_bins: int):
    """K3 on the GPU: per-feature quantile split candidates of a [s, d] sample in one kernel (quantile.hip).

    Returns host arrays (thr [d, max_bins-1], nthr [d], kdist [d]) and the device tensor of sorted columns
    [d, s] (NaN last), or None when the kernel does not apply (CPU tensor, s > QUANTILE_MAX_S, max_bins < 2).
    Features with kdist <= max_bins (and categorical ones) need the host path on their sorted column."""
    s, d = samp.shape
    if not _native(samp) or s == 0 or s > QUANTILE_MAX_S or not (2 <= max_bins <= 257):
        return None
    samp = samp.double().contiguous()
    dev = samp.device
    sorted_ = torch.empty((d, s), dtype=torch.float64, device=dev)
    thr = torch.empty((d, max_bins - 1), dtype=torch.float64, device=dev)
    ints = torch.empty((2, d), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().cdna_quantile_thresholds(_ptr(samp), s, d, max_bins, _ptr(sorted_), _ptr(thr),
                                                   _ptr(ints[0]), _ptr(ints[1]), None, _stream(dev)),
               "cdna_quantile_thresholds")
    ih = ints.cpu().numpy()
    return thr.cpu().numpy(), ih[0].copy(), ih[1].copy(), sorted_


class _HostCopies:
    """Device tensors copied to pinned host buffers behind the work already queued; ``get()`` waits for them."""

    def __init__(self, *ts: torch.Tensor):
        self.h = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in ts]
        for hb, t in zip(self.h, ts):
            hb.copy_(t, non_blocking=True)
        self.ev = torch.cuda.Event()
        self.ev.record(torch.cuda.current_stream(ts[0].device))

    def get(self):
        self.ev.synchronize()
        return [hb.numpy() for hb in self.h]


def quantile_thresholds_dev(samp: torch.Tensor, max_bins: int):
    """K3 without a host round trip: (thr [d, max_bins-1] fp32, nthr [d] int32 -- both device tensors, the fp32
    thresholds written by the kernel itself for the binning --, pending host copies of (thr fp64, nthr, kdist)), or
    None where :func:`quantile_thresholds` does not apply.  The binning can be queued on the device thresholds at
    once; they equal the host path's only where every feature has more than ``max_bins`` distinct values (kdist),
    which the caller checks on the host copy once it has queued the binning."""
    s, d = samp.shape
    if not _native(samp) or s == 0 or s > QUANTILE_MAX_S or not (2 <= max_bins <= 257):
        return None
    samp = samp.double().contiguous()
    dev = samp.device
    sorted_ = torch.empty((d, s), dtype=torch.float64, device=dev)
    thr = torch.empty((d, max_bins - 1), dtype=torch.float64, device=dev)
    ints = torch.empty((2, d), dtype=torch.int32, device=dev)
    thr32 = torch.empty((d, max_bins - 1), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().cdna_quantile_thresholds(_ptr(samp), s, d, max_bins, _ptr(sorted_), _ptr(thr),
                                                   _ptr(ints[0]), _ptr(ints[1]), _ptr(thr32), _stream(dev)),
               "cdna_quantile_thresholds")
    return thr32, ints[0], _HostCopies(thr, ints)


# --------------------------------------------------------------------- K4
# binize v6: the per-feature uniform-grid LUT narrows the threshold search to the few thresholds of the value's cell
# (trees.hip binize5_kernel<C>): cells per feature, 64 or 256; 0 = the 6-step LDS binary search of v5
BINIZE_LUT = 256


def binize(X: torch.Tensor, thr: torch.Tensor, nthr: torch.Tensor, missing: Optional[float] = None,
           want_rm: bool = False, rm_layout: str = "std", out_full=None, row0: int = 0):
    """Raw features -> uint8 bins in feature-group-major layout [G, n, 8].

    want_rm: return ``(bins, rm)`` where ``rm`` is the row-major copy of ``bins_row_major`` written by the
    same kernel (GPU search kernel only; otherwise None and the caller transposes lazily).
    rm_layout "s10" (d <= 100): ``rm`` [n, 16, 8] is in the seg10 layout of :func:`bins_seg10` instead (the
    six-items-per-wave record histogram's rows); None when the kernel that ran cannot write it.

    Continuous feature f: bin = #{thr[f, :nthr[f]] < x}; NaN -> nthr[f].
    Categorical feature (nthr[f] < 0): bin = clamp(int(x), 0, 255).
    missing (XGBoost): values that are NaN or equal ``missing`` are binned as -inf (bin 0 when the
    thresholds start at -FLT_MAX), without materialising a masked copy of X.

    out_full (streamed fits, chunk by chunk): ``(bins [G, N, 8], rm [N, Gs, 8] or None)`` of the whole table;
    this chunk's rows are written to rows [row0, row0 + n) of both, and ``(bins, rm)`` views of them returned.
    """
    n, d = X.shape
    G = (d + 7) // 8
    tmax = thr.shape[1] if thr.dim() == 2 else 0
    if _native(X):
        X = X.float()
        X = X if X.stride(1) == 1 else X.contiguous()
        thr = thr.float().contiguous()
        nthr = nthr.int().contiguous()
        s10 = want_rm and rm_layout == "s10"
        if s10 and d > 100:
            raise ValueError("seg10 rows hold at most 100 features")
        Gs = 16 if (s10 or (BINS_RM_PAD and G <= 16)) else G
        if out_full is not None:
            full, rm_full = out_full
            assert full.shape[0] == G and full.is_contiguous() and row0 + n <= full.shape[1]
            out = full[:, row0:row0 + n]
            ldo, optr = full.shape[1], full.data_ptr() + row0 * 8
            rm = None
            if want_rm:
                assert rm_full is not None and rm_full.shape[1] == Gs and rm_full.is_contiguous()
                rm = rm_full[row0:row0 + n]
        else:
            out = torch.empty((G, n, 8), dtype=torch.uint8, device=X.device)
            ldo, optr = 0, _ptr(out)
            rm = torch.empty((n, Gs, 8), dtype=torch.uint8, device=X.device) if want_rm else None
        miss_on = missing is not None
        miss_val = float("nan") if (missing is None or math.isnan(missing)) else float(missing)
        if n:
            rc = _lib.lib().cdna_binize(_ptr(X), n, d, X.stride(0), _ptr(thr), _ptr(nthr), tmax, int(miss_on),
                                        miss_val, optr, _ptr(rm) if rm is not None else None,
                                        -10 if s10 else Gs, ldo, int(BINIZE_LUT), int(BINIZE_RESIDENT),
                                        _stream(X.device))
            if rc == 2:  # the fallback kernel ran: no row-major copy
                rm = None
            else:
                _lib.check(rc, "cdna_binize")
        return (out, rm) if want_rm else out
    out = torch.zeros((G, n, 8), dtype=torch.uint8) if out_full is None else out_full[0][:, row0:row0 + n]
    if out_full is not None:
        out.zero_()
    Xf = X.float()
    if missing is not None:
        miss = torch.isnan(Xf) if math.isnan(missing) else (torch.isnan(Xf) | (Xf == float(missing)))
        Xf = torch.where(miss, torch.full_like(Xf, float("-inf")), Xf)
    for f in range(d):
        nt = int(nthr[f])
        x = Xf[:, f]
        if nt < 0:
            # clamped in float first: the conversion of NaN, +-inf and values past int64 is not defined
            b = torch.clamp(torch.nan_to_num(x, nan=0.0), 0.0, 255.0).to(torch.int64)
        else:
            b = torch.searchsorted(thr[f, :nt].float().contiguous(), x.contiguous(), right=False)
            b = torch.where(torch.isnan(x), torch.full_like(b, nt), b)
        out[f // 8, :, f % 8] = b.to(torch.uint8)
    return (out, None) if want_rm else out


def bins_seg10(bins: torch.Tensor, d: int) -> torch.Tensor:
    """[G, n, 8] bins -> the seg10 row layout [n, 16, 8] (torch; reference of binize's ``rm_layout="s10"``):
    byte 12 s + p of a row holds feature 10 s + p (s < 10, p < 10), every other byte is 0."""
    G, n, _ = bins.shape
    if d > 100:
        raise ValueError("seg10 rows hold at most 100 features")
    flat = bins.permute(1, 0, 2).reshape(n, G * 8)[:, :d]
    out = torch.zeros((n, 128), dtype=torch.uint8, device=bins.device)
    f = torch.arange(d, device=bins.device)
    out[:, 12 * (f // 10) + f % 10] = flat
    return out.view(n, 16, 8)


def bins_to_matrix(bins: torch.Tensor, d: int) -> torch.Tensor:
    """[G, n, 8] -> [n, d] (int64) view helper for reference code."""
    G, n, _ = bins.shape
    return bins.permute(1, 0, 2).reshape(n, G * 8)[:, :d].to(torch.int64)


# --------------------------------------------------------------------- K5
HIST_LDS_BUDGET = 64 * 1024
# lane mapping: 2 = lane per row (hist4_kernel); 5 = rotated features with the per-update VALU work hoisted
# (hist4f_kernel, when its LDS slot table holds the level's id span)
HIST_MAP = 5
# hist v5 (row records): packed single-atomic regression histograms, trees per block group when packed
HIST5_PACKED = True
HIST5_PACKED_MAXT = 8
HIST5_PACKED_LDS = 128 * 1024
# wave-compacted packed kernel (hist5q): full-wave LDS atomic rounds over sparse (row, tree) work
# 0 off, 1 where it pays (deep levels), 2 always (tests)
HIST5_COMPACT = 1


def _absmax(v: torch.Tensor) -> float:
    """max |v| (NaN if v holds one) in one reduction kernel: the inf-norm reduces |v| inside the reduction, where
    ``v.abs().max()`` first wrote |v| in a full elementwise pass (0.14 ms of a 1e8-row boosting round)."""
    if v.is_floating_point():
        return float(torch.linalg.vector_norm(v.reshape(-1), float("inf")).item())
    return float(v.abs().max().item())


def _fixed_scale(v: Optional[torch.Tensor], n: int, wmax: int, qmax_bits: int = 62) -> float:
    """Power-of-two fixed-point scale so that sum_r w_r * |round(v_r * s)| < 2^62 over n rows
    (and |round(v_r * s)| < 2^qmax_bits for kernels that quantise in 32 bits)."""
    if v is None or v.numel() == 0:
        return 1.0
    m = _absmax(v)
    if not math.isfinite(m):
        raise ValueError("histogram statistic contains NaN/Inf")
    if m == 0.0:
        return 1.0
    e = 62 - math.ceil(math.log2(max(1, n) * max(1, wmax) * m)) - 1
    e = min(e, qmax_bits - math.ceil(math.log2(m)) - 1)
    return float(2.0 ** max(-120, min(100, e)))


# Maxima the host needs before a fit's first level (the label's max |v| for the fixed-point scale, the largest
# bootstrap weight) are reduced on a side stream right after their inputs exist and copied to pinned memory;
# the fit reads them later without draining the device queue (each .item() there idled the GPU ~0.1 ms).
class _PendingScalar:
    def __init__(self, t: torch.Tensor, stream):
        self.host = torch.empty(1, dtype=t.dtype, pin_memory=True)
        self.host.copy_(t.reshape(1), non_blocking=True)
        self.ev = torch.cuda.Event()
        self.ev.record(stream)

    def get(self) -> float:
        self.ev.synchronize()
        return float(self.host[0])


def float_with_absmax(t: torch.Tensor, stream=None) -> torch.Tensor:
    """``t.float()`` of a contiguous fp64 device column with max |t| queued alongside (as prefetch_max(absval)
    attaches it): one pass of misc.hip cast_absmax_kernel instead of cast + abs + max."""
    st = stream if stream is not None else torch.cuda.current_stream(t.device)
    if not (_native(t) and t.dtype == torch.float64 and t.dim() == 1 and t.is_contiguous() and t.numel()):
        with torch.cuda.stream(st):
            out = t.float()
        prefetch_max(out, absval=True, stream=st)
        return out
    with torch.cuda.stream(st):
        out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
        bits = torch.empty(1, dtype=torch.int32, device=t.device)
        rc = _lib.lib().cdna_cast_absmax(_ptr(t), t.numel(), _ptr(out), _ptr(bits), None, st.cuda_stream)
        if rc == 1:  # misaligned view: the torch passes
            out = t.float()
            prefetch_max(out, absval=True, stream=st)
            return out
        _lib.check(rc, "cdna_cast_absmax")
        setattr(out, "_cdna_absmax", _PendingScalar(bits.view(torch.float32), st))
    return out


def shifted_f32(t: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """``(t - shift).float()`` of a contiguous fp64 device column, ``shift`` a one-element fp64 device tensor: one
    pass (misc.hip cast_absmax_kernel with its shift operand), the subtraction in fp64 before the rounding."""
    if not (_native(t) and t.dtype == torch.float64 and t.dim() == 1 and t.is_contiguous() and t.numel()):
        return (t - shift.double()).float()
    sd = shift.double().reshape(1).contiguous()
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    rc = _lib.lib().cdna_cast_absmax(_ptr(t), t.numel(), _ptr(out), None, _ptr(sd), _stream(t.device))
    if rc == 1:  # misaligned view
        return (t - sd).float()
    _lib.check(rc, "cdna_cast_absmax(shift)")
    return out


def sample_rows(n: int, seed: int, offset: int, stream: int, frac: float, device,
                ordered: bool = True) -> Optional[torch.Tensor]:
    """int64 ids of the rows r < n with ``uniform(n, seed, offset, stream)[r] < frac`` (one fused kernel; the set
    of compact_mask(uniform(...) < frac), in arbitrary order unless ``ordered``).  None when the count passes the
    capacity sized from the expected count (the caller then takes the materialised path)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    exp_ = n * frac
    cap = int(exp_ + 12.0 * math.sqrt(exp_ + 1.0) + 1024)
    idx = torch.empty(cap, dtype=torch.int64, device=device)
    cnt = torch.empty(1, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().cdna_sample_rows(n, seed, int(offset), int(stream) & 0xFFFFFFFF, float(frac), _ptr(idx),
                                           cap, _ptr(cnt), _stream(torch.device(device))), "cdna_sample_rows")
    c = int(cnt.item())
    if c > cap:
        return None
    return torch.sort(idx[:c]).values if ordered else idx[:c]


def sample_gather(X: torch.Tensor, seed: int, offset: int, stream: int, frac: float):
    """``X[sample_rows(...)]`` as an fp64 [cap, d] sample without a host round trip: the rows of the Philox sample
    (arbitrary order) then NaN rows up to the capacity (misc.hip sample_gather_kernel).  -> (samp, ok) where
    ``ok()`` (call it once the work behind the sample is queued) tells whether every sampled row fitted the capacity
    (else the caller redoes the exact path); None where the kernels do not apply."""
    n, d = X.shape
    if not _native(X) or n == 0 or X.dtype != torch.float32 or X.stride(1) != 1:
        return None
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    exp_ = n * frac
    cap = int(exp_ + 12.0 * math.sqrt(exp_ + 1.0) + 1024)
    dev = X.device
    idx = torch.empty(8 * cap, dtype=torch.int64, device=dev)  # 8 regions of cap ids (misc.hip)
    cnt = torch.empty(8, dtype=torch.int32, device=dev)
    samp = torch.empty((cap, d), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().cdna_sample_gather(_ptr(X), n, X.stride(0), d, seed, int(offset) & 0xFFFFFFFFFFFFFFFF,
                                             int(stream) & 0xFFFFFFFF, float(frac), _ptr(idx), _ptr(cnt), cap,
                                             _ptr(samp), _stream(dev)), "cdna_sample_gather")
    host = torch.empty(8, dtype=torch.int32, pin_memory=True)
    host.copy_(cnt, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))

    def ok() -> bool:
        ev.synchronize()
        return int(host.to(torch.int64).sum()) <= cap
    return samp, ok


def prefetch_max(t: torch.Tensor, absval: bool = False, stream=None) -> None:
    """Queue max(t) (max |t|) on ``stream`` (default: current) and attach it to the tensor object itself (never
    keyed by address: a recycled allocation must not inherit a stale value) for packed_scale_global /
    codes_init_max, which then read it instead of syncing."""
    if not t.is_cuda or t.numel() == 0:
        return
    st = stream if stream is not None else torch.cuda.current_stream(t.device)
    with torch.cuda.stream(st):
        m = (t.abs() if absval else t).max()
        setattr(t, "_cdna_absmax" if absval else "_cdna_max", _PendingScalar(m, st))


def _prefetched(t: torch.Tensor, absval: bool) -> Optional[float]:
    p = getattr(t, "_cdna_absmax" if absval else "_cdna_max", None)
    return None if p is None else p.get()


def packed_scale_global(v: torch.Tensor, comm) -> float:
    """Power-of-two scale with |round(v * s)| <= 2^23 (packed count|sum LDS words), from the max |v| over all
    ranks of ``comm`` (None: this one): every rank quantises identically, so integer histograms all-reduce to the
    same sums whatever the number of GPUs."""
    m = _prefetched(v, True) if v.numel() else 0.0
    if m is None:
        m = _absmax(v)
    m = comm.all_reduce_scalar(m, "max") if comm is not None else m
    if not math.isfinite(m):
        raise ValueError("histogram statistic contains NaN/Inf")
    if m == 0.0:
        return 1.0
    e = math.floor(math.log2((2 ** 23) / m))
    return float(2.0 ** max(-120, min(100, e)))


def _packed_scale(v: torch.Tensor) -> float:
    """``packed_scale_global`` on this rank alone.  Like it, reads a max |v| that ``prefetch_max`` attached to ``v``
    instead of reducing again (the same value as long as ``v`` has not been written since)."""
    return packed_scale_global(v, None)


def slot_groups(slot_tree, id_tree, SB: int, max_trees: Optional[int] = None) -> list:
    """The slot groups of a level histogram launch, one per pass of a block over the rows: rows
    ``(s0, t0, t1, i0, i1)`` = first slot, first and last tree of the group's (at most ``SB``) slots, and the
    range of active ids of those trees.  ``slot_tree`` / ``id_tree``: the tree of every build slot / active id,
    ascending.  ``max_trees`` caps the trees of a group (the row-code kernels prefetch one code per tree)."""
    slot_tree = np.asarray(slot_tree)
    id_tree = np.asarray(id_tree)
    S = len(slot_tree)
    rows = []
    a = 0
    while a < S:
        b = min(S, a + SB)
        t0 = int(slot_tree[a])
        if max_trees is not None:
            b = min(b, int(np.searchsorted(slot_tree, t0 + max_trees, side="left")))
        t1 = int(slot_tree[b - 1])
        i0 = int(np.searchsorted(id_tree, t0, side="left"))
        i1 = int(np.searchsorted(id_tree, t1, side="right"))
        rows.append((a, t0, t1, i0, i1))
        a = b
    return rows


HIST5_NT_BUCKETS = (1, 2, 4, 8, 16)  # trees per group the row-code kernels are instantiated for (histblock.h)


def _nt_bucket(nt: int) -> int:
    return next(b for b in HIST5_NT_BUCKETS if nt <= b)


def _hist_per_slot(kbits: int, C: int, B: int) -> int:
    """LDS bytes of one slot's [8][B] block over all planes."""
    per_slot = 8 * B * int(_lib.lib().cdna_hist4_bytes_per_bin(kbits, int(C)))
    if per_slot > 150 * 1024:
        raise ValueError("histogram too large for LDS (classes x bins)")
    return per_slot


def _hist_launch(name: str, kbits: int, bins, d, T, rows_of, v0, v1, label, C, build_slot, feat_mask, S, B, SB,
                 rows, target, table, scales, tail, out):
    """The common tail of the two level-histogram wrappers: chunk count, operand casts, the int64 launch of
    ``cdna_<name>`` and the un-scaling into ``out``.  ``rows_of``: the kernel's two row-state pointers (node ids
    and weights, or codes and tfirst); ``table``: its table-size argument; ``scales(v0, v1)`` -> (qs0, qs1) from
    the cast operands; ``tail``: arguments between qs1 and the output."""
    G, n, _ = bins.shape
    ng = len(rows)
    grp, = upload(bins.device, np.asarray(rows, dtype=np.int32).reshape(-1))
    # enough chunks to fill 256 CUs; u32 LDS counts: rows/chunk * 255 < 2^32
    nchunk = int(max(1, min((target + G * ng - 1) // (G * ng), (n + 8191) // 8192)))
    nchunk = max(nchunk, -(-n // (1 << 23)))
    mw = 0 if feat_mask is None else feat_mask.shape[1]
    fm = None if feat_mask is None else feat_mask.int().contiguous()
    v0 = None if v0 is None else v0.float().contiguous()
    v1 = None if v1 is None else v1.float().contiguous()
    label = None if label is None else label.int().contiguous()
    bs = build_slot.int().contiguous()
    qs0, qs1 = scales(v0, v1)
    iout = torch.zeros(out.shape, dtype=torch.int64, device=bins.device)
    _lib.check(getattr(_lib.lib(), "cdna_" + name)(
        kbits, _ptr(bins), n, d, T, *rows_of, _ptr(v0), _ptr(v1), _ptr(label), int(C), _ptr(bs), _ptr(fm), mw, S, B,
        SB, _ptr(grp), ng, nchunk, table, qs0, qs1, *tail, _ptr(iout), _stream(bins.device)), "cdna_" + name)
    out.copy_(iout)
    if not kbits & 1:
        if v0 is not None:
            out[..., 0] /= qs0
        out[..., 1] /= qs1
    return out


def _hist2(mode: int, bins, d, node, weight, v0, v1, label, C, build_slot, slot_tree, id_tree, feat_mask, B,
           lds_budget, out):
    """Launch the LDS integer histogram kernel on node ids (hist4.hip)."""
    S = len(slot_tree)
    n = bins.shape[1]
    kbits = mode | (4 if (mode == 0 and v0 is not None) else 0)
    per_slot = _hist_per_slot(kbits, C, B)
    SB = max(1, min(S, lds_budget // per_slot))
    rows = slot_groups(slot_tree, id_tree, SB)
    span = max(r[4] - r[3] for r in rows)
    lds_left = 150 * 1024 - ((SB * per_slot + 15) // 16) * 16 - SB - 16
    id_span_max = int(min(span, max(0, lds_left // 4), 16384))
    # fast rotated kernel: its LDS slot table must hold the whole id span
    vmode = 32 if HIST_MAP == 5 and v0 is None and id_span_max >= span else 0
    wmax = 255 if weight is not None else 1
    node = node.int().contiguous()
    weight = None if weight is None else weight.to(torch.uint8).contiguous()

    def scales(v0, v1):
        return _fixed_scale(v0, n, wmax), _fixed_scale(v1, n, wmax, qmax_bits=30 if vmode == 32 else 62)
    # 2 x 512-thread blocks per CU when LDS allows
    return _hist_launch("hist4", kbits | vmode, bins, d, node.shape[0], (_ptr(node), _ptr(weight)), v0, v1, label,
                        C, build_slot, feat_mask, S, B, SB, rows, 1024, id_span_max, scales, (), out)


def _hist_host(bins, d, node, weight, build_slot, feat_mask, B, row_ok, stride, offset, addends, flat) -> None:
    """Host formulation of the level histograms: every (tree, row) whose node maps to a build slot adds, for each
    enabled feature f, ``w * addends[k]`` (None: 1) to ``flat[cell * stride + offset, k]``, cell = (slot, f, bin)."""
    bm = bins_to_matrix(bins, d)
    n = bm.shape[0]
    fr = torch.arange(d)
    bs = build_slot.long()
    for t in range(node.shape[0]):
        ids = node[t].long()
        ok = ids >= 0
        slot = torch.full_like(ids, -1)
        slot[ok] = bs[ids[ok]]
        w = torch.ones(n, dtype=torch.float64) if weight is None else weight[t].double()
        ok = (slot >= 0) & (w != 0)
        if row_ok is not None:
            ok = ok & row_ok
        if not ok.any():
            continue
        rs = slot[ok]
        idx = (rs[:, None] * d + fr[None, :]) * B + bm[ok]
        if offset is not None:
            idx = idx * stride + offset[ok][:, None]
        msk = torch.ones_like(idx, dtype=torch.bool)
        if feat_mask is not None:
            words = feat_mask.long()[rs]  # [m, MW]
            msk = ((words[:, fr // 32] >> (fr % 32)) & 1).bool()
        for k, a in enumerate(addends):
            wx = (w[ok] if a is None else w[ok] * a[ok])[:, None].expand_as(idx)
            flat[:, k] += torch.bincount(idx[msk], weights=wx[msk], minlength=flat.shape[0])


def hist_moments(bins: torch.Tensor, d: int, node: torch.Tensor, weight: Optional[torch.Tensor],
                 v0: Optional[torch.Tensor], v1: torch.Tensor, build_slot: torch.Tensor, slot_tree: np.ndarray,
                 feat_mask: Optional[torch.Tensor], B: int, lds_budget: Optional[int] = None,
                 id_tree: Optional[np.ndarray] = None) -> torch.Tensor:
    """Per-slot (feature, bin) weighted moments: out[S, d, B, 2] (float64).

    out[s, f, b, 0] = sum w_t(r) * v0(r), out[s, f, b, 1] = sum w_t(r) * v1(r) over
    rows r whose active node in tree t maps to build slot s and bin_f(r) == b,
    restricted to features enabled in feat_mask[s] (bit f).
    """
    S = len(slot_tree)
    n = bins.shape[1]
    out = torch.zeros((S, d, B, 2), dtype=torch.float64, device=bins.device)
    if S == 0 or n == 0:
        return out
    if _native(bins):
        assert id_tree is not None, "the GPU node-id histograms need id_tree (the tree of every active node)"
        return _hist2(0, bins, d, node, weight, v0, v1, None, 0, build_slot, slot_tree, id_tree, feat_mask, B,
                      lds_budget or HIST_LDS_BUDGET, out)
    _hist_host(bins, d, node, weight, build_slot, feat_mask, B, None, 1, None,
               (None if v0 is None else v0.double(), v1.double()), out.view(-1, 2))
    return out


def hist_classes(bins: torch.Tensor, d: int, node: torch.Tensor, weight: Optional[torch.Tensor],
                 label: torch.Tensor, C: int, build_slot: torch.Tensor, slot_tree: np.ndarray,
                 feat_mask: Optional[torch.Tensor], B: int, lds_budget: Optional[int] = None,
                 id_tree: Optional[np.ndarray] = None) -> torch.Tensor:
    """Per-slot (feature, bin) weighted class counts: out[S, d, B, C] (float64)."""
    S = len(slot_tree)
    n = bins.shape[1]
    out = torch.zeros((S, d, B, C), dtype=torch.float64, device=bins.device)
    if S == 0 or n == 0:
        return out
    if _native(bins):
        assert id_tree is not None, "the GPU node-id histograms need id_tree (the tree of every active node)"
        return _hist2(1, bins, d, node, weight, None, None, label, C, build_slot, slot_tree, id_tree, feat_mask, B,
                      lds_budget or HIST_LDS_BUDGET, out)
    lab = label.long()
    _hist_host(bins, d, node, weight, build_slot, feat_mask, B, (lab >= 0) & (lab < C), C, lab, (None,),
               out.view(-1, 1))
    return out


# ------------------------------------------------------------ K5/K7 on row records
CODE_DONE = 0xFF
CODES_MAX_LOC = 255  # local nodes 0..254 of a tree fit the node byte next to CODE_DONE (the kernels' LDS tables)


def _check_codes_level(tfirst: np.ndarray, A: int, tfirst_next: Optional[np.ndarray] = None,
                       child: Optional[np.ndarray] = None) -> None:
    """The row codes' limit: at most CODES_MAX_LOC active nodes per tree, at this level and (given the children) at
    the next.  ValueError otherwise -- the codes kernels index 256-entry tables with the node byte."""
    tf = np.asarray(tfirst, dtype=np.int64).reshape(-1)
    if tf.size == 0:
        return
    ends = np.concatenate([tf[1:], [A]])
    if int((ends - tf).max()) > CODES_MAX_LOC:
        raise ValueError(f"row codes hold at most {CODES_MAX_LOC} active nodes per tree, got {int((ends - tf).max())}")
    if child is None or A == 0:
        return
    ch = np.asarray(child, dtype=np.int64).reshape(-1, 2)
    tree_of = np.searchsorted(tf, np.arange(A), side="right") - 1
    loc = ch - np.asarray(tfirst_next, dtype=np.int64).reshape(-1)[tree_of][:, None]
    bad = (ch >= 0) & ((loc < 0) | (loc >= CODES_MAX_LOC))
    if bad.any():
        raise ValueError(f"row codes hold at most {CODES_MAX_LOC} next-level nodes per tree "
                         f"(child local index {int(loc[bad].max())})")


def codes_init(weights: Optional[torch.Tensor], T: int, n: int, device) -> torch.Tensor:
    """Row records for level 0: code[r, t] = weight << 8 | local (0 = the root, 255 = done).

    Returned as int16 [T, n] holding the uint16 bit patterns (hist5.hip)."""
    return codes_init_max(weights, T, n, device)[0]


def codes_init_max(weights: Optional[torch.Tensor], T: int, n: int, device):
    """(codes, largest weight).  On the GPU one kernel writes the codes and reduces the max."""
    if weights is not None and _native(weights) and weights.dtype == torch.uint8 and weights.is_contiguous() \
            and weights.data_ptr() % 16 == 0:
        codes = torch.empty((T, n), dtype=torch.int16, device=weights.device)
        wm = torch.zeros(1, dtype=torch.int32, device=weights.device)
        pre = _prefetched(weights, False)
        _lib.check(_lib.lib().cdna_codes_init(_ptr(weights), T * n, _ptr(codes), _ptr(wm), _stream(weights.device)),
                   "cdna_codes_init")
        return codes, max(1, int(pre if pre is not None else wm.item()))
    if weights is None:
        # every row in every tree with weight 1 at the root (local node 0): one fill, no elementwise chain
        return torch.full((T, n), 1 << 8, dtype=torch.int16, device=device), 1
    else:
        w = weights.to(device=device).to(torch.int32)
    c = (w << 8) | torch.where(w == 0, torch.full_like(w, CODE_DONE), torch.zeros_like(w))
    wmax = int(w.max().item()) if w.numel() else 1
    return c.to(torch.int16).contiguous(), max(1, wmax)


FEATURE_MASKS_MAX_D = 2048


def feature_masks(base: np.ndarray, d: int, k: int, device, base_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-node feature-subset bit words int32 [A, ceil(d/32)] on the GPU (misc.hip feature_masks_kernel): node a
    keeps the k features with the smallest splitmix64(base[a] + f * 0xD6E8FEB86659FD93) -- the words of
    ForestTrainer._feature_masks for the same per-node base.  d <= FEATURE_MASKS_MAX_D."""
    A = len(base)
    W = (d + 31) // 32
    out = torch.empty((A, W), dtype=torch.int32, device=device)
    if A == 0:
        return out
    b = base_dev if base_dev is not None else upload(device, np.ascontiguousarray(base, dtype=np.uint64).view(np.int64))[0]
    _lib.check(_lib.lib().cdna_feature_masks(_ptr(b), A, d, k, _ptr(out), _stream(out.device)), "cdna_feature_masks")
    return out


def decode_codes(codes: torch.Tensor, tfirst: torch.Tensor):
    """codes [T, n] -> (node ids int32 [T, n] with -1 = done, weights uint8 [T, n]).  GPU: one pass
    (seg.hip codes_to_nodes_kernel).

    Besides the done codes (node byte 255) a code of weight 0 decodes to -1, on the host and in the kernel: the
    node-id histograms and partitions that follow would carry such a row for nothing (it adds 0 to every cell, as it
    does in the row-code histograms).  This is the histograms' reading only; ``partition_codes`` looks at the node
    byte alone."""
    if _native(codes) and codes.dim() == 2 and codes.dtype in (torch.uint16, torch.int16):
        T, n = codes.shape
        c = codes.contiguous()
        tf, = upload(codes.device, tfirst.cpu().numpy().astype(np.int32))
        node = torch.empty((T, n), dtype=torch.int32, device=codes.device)
        w = torch.empty((T, n), dtype=torch.uint8, device=codes.device)
        _lib.check(_lib.lib().cdna_codes_to_nodes(_ptr(c), n, T, _ptr(tf), _ptr(node), _ptr(w), _stream(codes.device)),
                   "cdna_codes_to_nodes")
        return node, w
    c = codes.to(torch.int32) & 0xFFFF
    loc = c & 0xFF
    w = (c >> 8).to(torch.uint8)
    ids = tfirst.to(c.device).to(torch.int32)[:, None] + loc
    ids = torch.where((loc == CODE_DONE) | (w == 0), torch.full_like(ids, -1), ids)
    return ids.contiguous(), w.contiguous()


def hist_codes(mode: int, bins: torch.Tensor, d: int, codes: torch.Tensor, tfirst: torch.Tensor,
               v0: Optional[torch.Tensor], v1: Optional[torch.Tensor], label: Optional[torch.Tensor], C: int,
               build_slot: torch.Tensor, slot_tree: np.ndarray, id_tree: np.ndarray,
               feat_mask: Optional[torch.Tensor], B: int, lds_budget: Optional[int] = None,
               wmax: int = 255) -> torch.Tensor:
    """Histograms from row records (hist5.hip).  mode 0: moments [S, d, B, 2]; 1: classes [S, d, B, C].

    ``wmax``: largest row weight in ``codes`` (bounds the packed kernel's drain interval)."""
    S = len(slot_tree)
    G, n, _ = bins.shape
    T = codes.shape[0] if codes.dim() == 2 else 0
    K_ = 2 if mode == 0 else C
    out = torch.zeros((S, d, B, K_), dtype=torch.float64, device=bins.device)
    if S == 0 or n == 0:
        return out
    if not _native(bins):
        node, w = decode_codes(codes, tfirst)
        if mode == 0:
            return hist_moments(bins, d, node, w, v0, v1, build_slot, slot_tree, feat_mask, B)
        return hist_classes(bins, d, node, w, label, C, build_slot, slot_tree, feat_mask, B)
    maxt = int(_lib.lib().cdna_hist5_max_trees())
    packed = HIST5_PACKED and mode == 0 and v0 is None
    compact = packed and HIST5_COMPACT
    kbits = mode | (4 if (mode == 0 and v0 is not None) else 0) | (16 if packed else 0) | (64 if compact else 0)
    per_slot = _hist_per_slot(kbits, C, B)
    budget = lds_budget or HIST_LDS_BUDGET
    if packed:
        # register drain holds <= 16 cells per thread: 512 threads -> 64 KB, 1024 threads -> 128 KB
        budget = min(HIST5_PACKED_LDS if lds_budget is None else lds_budget, 16384 * 8)
        maxt = min(maxt, HIST5_PACKED_MAXT)
    SB = max(1, min(S, budget // per_slot))
    # at most `maxt` trees per group (prefetched row record)
    rows = slot_groups(slot_tree, id_tree, SB, maxt)
    ng = len(rows)
    # the tree cap can leave groups smaller than the LDS budget allows: size LDS to the largest group
    SB = max(min(SB, (rows[i + 1][0] if i + 1 < ng else S) - rows[i][0]) for i in range(ng))
    max_nt = max(r[2] - r[1] + 1 for r in rows)
    big = packed and SB * per_slot > 8192 * 8  # 1024-thread blocks: 1 per CU
    # wave compaction pays once the plane needs 1024-thread blocks and several trees share
    # a pass (measured per level: profiles/hist_micro_1e8_compact.txt); below that the
    # lane-per-row kernel's fewer LDS instructions win
    compact = compact and (HIST5_COMPACT >= 2 or (big and max_nt >= 2))
    kbits = kbits if compact else (kbits & ~64)
    rbuf = 16 * 128 * 12 if compact else 0
    lds_used = ((SB * per_slot + 15) // 16) * 16 + rbuf + _nt_bucket(max_nt) * 512 + SB + 16
    if lds_used > 160 * 1024:
        raise ValueError("local-node tables do not fit in LDS next to the histogram")
    wmax = int(max(1, min(255, wmax)))
    assert codes.dtype == torch.int16 and codes.is_contiguous() and codes.shape[1] == n
    tf = (upload(bins.device, tfirst.numpy().astype(np.int32))[0] if not tfirst.is_cuda else
          tfirst.to(dtype=torch.int32).contiguous())

    def scales(v0, v1):
        return (_fixed_scale(v0, n, wmax, qmax_bits=30),
                _packed_scale(v1) if packed else _fixed_scale(v1, n, wmax, qmax_bits=30))
    return _hist_launch("hist5", kbits, bins, d, T, (_ptr(codes), _ptr(tf)), v0, v1, label, C, build_slot,
                        feat_mask, S, B, SB, rows, 512 if big else 1024, max_nt, scales, (wmax,), out)


# persistent partition (tables staged once per block, coalesced bins words, all trees' codes in flight)
PARTITION7 = True
PARTITION7_MIN_T = 16



# boosting partitions (partition5 with margins) gather each row's split byte from a feature-major [d][n] byte copy
# of the bins (BinnedData.feature_major_bins, built once per fit) instead of the [G][n] 8-feature words
PART_FEATURE_MAJOR = True


def partition_codes(bins: torch.Tensor, codes: torch.Tensor, tfirst: torch.Tensor, tfirst_next: torch.Tensor,
                    split_feat: torch.Tensor, split_bin: torch.Tensor, cat_off: torch.Tensor,
                    cat_mask: torch.Tensor, child: torch.Tensor, margin: Optional[tuple] = None,
                    bins_fm: Optional[torch.Tensor] = None) -> None:
    """In place: every row's code moves to the chosen child's local index (255 = done).

    A code is done when its NODE byte is 255, and only then: the weight byte plays no part in the move and is
    carried untouched, so a live code whose weight byte is 0 moves like any other (``codes_init`` writes weight-0
    rows as done from the start, and ``decode_codes`` / the histograms skip weight 0 on their own).  The host path
    and the partition5 / partition7 kernels agree on this bit for bit.

    A tree holds at most ``CODES_MAX_LOC`` active nodes at this level and at the next (the node byte; checked when
    the tables are host tensors -- device tables come from ``split_decode`` of a forest whose depth bounds them).

    margin (GPU, partition5): ``(F [n] fp32, lv [3A] fp32 from split_decode, eta)`` -- rows that finish at this
    level add ``eta * leaf value`` to F (boosting margin update without a tree walk).
    bins_fm (partition5): the feature-major byte copy [G * 8, n] of ``bins`` the row bytes are gathered from."""
    G, n, _ = bins.shape
    T = codes.shape[0]
    if n == 0 or T == 0:
        return
    if _native(bins):
        if not cat_mask.numel():
            cat_mask = torch.zeros(8, dtype=torch.int32)
        srcs = (tfirst, tfirst_next, split_feat, split_bin, cat_off, child, cat_mask)
        if all(not t.is_cuda for t in srcs):
            _check_codes_level(tfirst.numpy(), int(split_feat.numel()), tfirst_next.numpy(), child.numpy())
            # one async host->device copy for the seven small tables (seven synchronous copies were ~0.13 ms
            # of launch gaps per level)
            args = upload(bins.device, *[t.numpy().astype(np.int32).reshape(-1) for t in srcs])
        else:
            args = [t.to(device=bins.device, dtype=torch.int32).contiguous() for t in srcs]
        cm = args[6]
        A = int(split_feat.numel())
        # partition7 streams every bins word of every row once per level (10 GB at 1e8 x 100): it pays when
        # many trees share that pass; for few trees partition5's per-(row, tree) byte gathers move less (GBDT,
        # T = 1: 57.9 vs 40.6 ms per boosting round with partition7; CV grid with 5 / 10 trees: 2.18 vs 1.34 s)
        # (its table packs a bin set's offset into 15 bits: larger mask tables take partition5 as well)
        if margin is None and PARTITION7 and T >= PARTITION7_MIN_T and G <= 16 and A <= 1024 and T <= 64 \
                and cat_mask.numel() <= 8 << 15:
            _lib.check(_lib.lib().cdna_partition7(
                _ptr(bins), n, G, T, A, _ptr(codes), _ptr(args[0]), _ptr(args[1]), _ptr(args[2]), _ptr(args[3]),
                _ptr(args[4]), _ptr(cm), _ptr(args[5]), _stream(bins.device)), "cdna_partition7")
            return
        F, lv, eta = margin if margin is not None else (None, None, 0.0)
        if margin is not None:
            assert F.dtype == torch.float32 and F.is_contiguous() and F.numel() == n and lv.numel() == 3 * A
        fm = bins_fm is not None
        if fm:
            assert bins_fm.shape == (G * 8, n) and bins_fm.dtype == torch.uint8 and bins_fm.is_contiguous()
        _lib.check(_lib.lib().cdna_partition5(_ptr(bins_fm if fm else bins), n, T, A, _ptr(codes), _ptr(args[0]),
                                              _ptr(args[1]), _ptr(args[2]), _ptr(args[3]), _ptr(args[4]), _ptr(cm),
                                              _ptr(args[5]), -1 if fm else 0, _ptr(lv), float(eta), _ptr(F),
                                              _stream(bins.device)), "cdna_partition5")
        return
    assert margin is None, "margin updates run in the GPU partition only"
    _check_codes_level(tfirst.numpy(), int(split_feat.numel()), tfirst_next.numpy(), child.numpy())
    # not decode_codes: that drops weight-0 rows (histograms), a partition moves them like any other row
    c = codes.to(torch.int32) & 0xFFFF
    loc = c & 0xFF
    node = torch.where(loc == CODE_DONE, torch.full_like(loc, -1), tfirst.to(torch.int32)[:, None] + loc).contiguous()
    partition(bins, node, split_feat, split_bin, cat_off, cat_mask, child)
    tn = tfirst_next.to(torch.int32)[:, None]
    loc = torch.where(node >= 0, node - tn, torch.full_like(node, CODE_DONE))
    codes.copy_(((c & 0xFF00) | loc).to(torch.int16))


# --------------------------------------------------------------------- K7
def partition(bins: torch.Tensor, node: torch.Tensor, split_feat: torch.Tensor, split_bin: torch.Tensor,
              cat_off: torch.Tensor, cat_mask: torch.Tensor, child: torch.Tensor) -> None:
    """In-place: move each row of each tree from its active node to the chosen child."""
    G, n, _ = bins.shape
    T = node.shape[0]
    if n == 0 or T == 0:
        return
    if _native(bins):
        cm = cat_mask.int().contiguous() if cat_mask.numel() else torch.zeros(8, dtype=torch.int32,
                                                                                 device=bins.device)
        assert node.dtype == torch.int32 and node.is_contiguous()
        split_feat, split_bin = split_feat.int().contiguous(), split_bin.int().contiguous()
        cat_off, child = cat_off.int().contiguous(), child.int().contiguous()
        _lib.check(_lib.lib().cdna_partition(_ptr(bins), n, T, _ptr(node), _ptr(split_feat), _ptr(split_bin),
                                             _ptr(cat_off), _ptr(cm), _ptr(child), _stream(bins.device)),
                   "cdna_partition")
        return
    d = G * 8
    bm = bins_to_matrix(bins, d)
    sf = split_feat.long()
    sb = split_bin.long()
    co = cat_off.long()
    cm = cat_mask.long() & 0xFFFFFFFF
    ch = child.long().view(-1, 2)
    rows = torch.arange(n)
    for t in range(T):
        ids = node[t].long()
        ok = ids >= 0
        if not ok.any():
            continue
        i = ids[ok]
        f = sf[i]
        leaf = f < 0
        fb = bm[rows[ok], f.clamp(min=0)]
        cat = co[i] >= 0
        words = cm[(co[i].clamp(min=0) * 8 + (fb >> 5))] if cm.numel() else torch.zeros_like(fb)
        left = torch.where(cat, ((words >> (fb & 31)) & 1).bool(), fb <= sb[i])
        nxt = torch.where(left, ch[i, 0], ch[i, 1])
        nxt = torch.where(leaf, torch.full_like(nxt, -1), nxt)
        new = ids.clone()
        new[ok] = nxt
        node[t] = new.to(node.dtype)


# --------------------------------------------------------------------- K8
def pack_heap(struct: np.ndarray, vals: np.ndarray, depth: int) -> np.ndarray:
    """Predict-heap table (trees.hip predict_heap_kernel) from a per-slot forest layout.

    ``struct`` int32 [T, 2^(D+1)-1, 2]: per heap slot {feature | -1 leaf/unreachable | -(f+2) categorical,
    threshold bits | mask offset}; ``vals`` float64 [T, 2^(D+1)-1]: the slot's leaf value.  Returns int32
    [T, 2^(D+2)-2]: the 2^D-1 internal slots (leaf slots become pass-through-left), then the 2^D depth-D leaf
    values as fp64, a shallower leaf's value at its leftmost depth-D descendant."""
    T = struct.shape[0]
    NI = (1 << depth) - 1
    out = np.empty((T, 4 * NI + 2), dtype=np.int32)
    out[:, :2 * NI] = struct[:, :NI].reshape(T, 2 * NI)
    leaf = np.zeros((T, NI + 1), dtype=np.float64)
    for k in range(depth, -1, -1):  # shallow last: a reachable leaf overwrites the unreachable slots below it
        s0, s1 = (1 << k) - 1, (1 << (k + 1)) - 1
        tt, ss = np.nonzero(struct[:, s0:s1, 0] == -1)
        if len(tt):
            leaf[tt, (s0 + ss + 1) * (1 << (depth - k)) - 1 - NI] = vals[tt, s0 + ss]
    out[:, 2 * NI:] = leaf.view(np.int32)
    return out


def heap_last_level(so: torch.Tensor, a_tree: torch.Tensor, a_key: torch.Tensor, a_w: torch.Tensor,
                    thr: torch.Tensor, min_gain: float, min_w: float, heap: torch.Tensor, depth: int) -> None:
    """Write a regression forest's last split level into its packed predict heap in place (``pack_heap`` layout
    of depth ``depth``; trees.hip heap_last_level_kernel): for each active node a whose K6 row ``so[a]`` (gain,
    feature, bin, left W, left S, right W, right S, ...) passes the host's split rule (finite gain > 0, >=
    min_gain; node weight a_w[a] >= min_w), the internal slot a_key[a] - 1 gets (feature, fp32 threshold bits of
    thr[feature, bin]) and its two depth-``depth`` leaves S / W (0 for an empty child).  a_tree / a_key int32,
    a_w f64, thr f32 [d, Bt], heap int32 [T, 2^(depth+2)-2]."""
    A = so.shape[0]
    if A == 0:
        return
    T = heap.shape[0]
    NI = (1 << depth) - 1
    assert heap.shape[1] == 4 * NI + 2 and so.dtype == torch.float64
    if _native(so):
        d, Bt = thr.shape
        _lib.check(_lib.lib().cdna_heap_last_level(_ptr(so), so.shape[1], A, _ptr(a_tree), _ptr(a_key), _ptr(a_w),
                                                   _ptr(thr), Bt, d, float(min_gain), float(min_w), _ptr(heap),
                                                   depth, T, _stream(so.device)), "cdna_heap_last_level")
        return
    gain = so[:, 0]
    ok = torch.isfinite(gain) & (gain > 0) & (gain >= min_gain) & (a_w >= min_w)
    idx = torch.nonzero(ok).flatten()
    if not len(idx):
        return
    f, b = so[idx, 1].long(), so[idx, 2].long()
    t, k = a_tree[idx].long(), a_key[idx].long()
    heap[t, 2 * (k - 1)] = f.to(torch.int32)
    heap[t, 2 * (k - 1) + 1] = thr[f, b].float().view(torch.int32)
    leaf = heap[:, 2 * NI:].view(torch.float64)  # [T, 2^depth] (a view: writes land in heap)
    for side in (0, 1):
        W, S = so[idx, 3 + 2 * side], so[idx, 4 + 2 * side]
        leaf[t, 2 * k + side - (1 << depth)] = torch.where(W > 0, S / torch.where(W > 0, W, torch.ones_like(W)),
                                                           torch.zeros_like(W))


def ordered_tree_sum(contribs, T: int, n: int, K: int, base=None) -> torch.Tensor:
    """The fp64 ensemble sum in the device kernels' order (trees.hip predict_kernel): lane q = t % 4 adds
    ``contribs(t)`` (tree_w[t] * leaf value, already a rounded product) for its trees in ascending order, then
    base + lane 0 + lane 1 + lane 2 + lane 3.  The cpu predictions therefore equal the GPU's bit for bit."""
    lanes = [torch.zeros((n, K), dtype=torch.float64) for _ in range(4)]
    for t in range(T):
        lanes[t & 3] += contribs(t)
    out = torch.zeros((n, K), dtype=torch.float64)
    if base is not None:
        out += base.double().cpu()[None, :]
    for q in range(4):
        out += lanes[q]
    return out


# persistent one-round grids (exactly the resident blocks) for the streaming kernels -- binize v5 and the heap
# predict -- instead of fixed caps of 1024 / 8192 blocks (per-block setup and the uneven last trips are what made
# them 8-9 % slower per row at the 8-GPU shard size: VERDICT r5 weak #2)
# (A/B round 6, profiles/r6/headline_ab.md: one persistent round was 0.4 ms SLOWER at the headline and within noise
# at the 8-GPU shard size, so both stay off)
BINIZE_RESIDENT = False
PREDICT_RESIDENT = False


PREDICT_STAGING = ("scalar", "float4", "float4+prefetch")  # trees.hip kStage*: how a 64-row X tile reaches LDS


def _predict_rows(X: torch.Tensor) -> torch.Tensor:
    """The fp32 rows (unit column stride) whose pointer the raw-feature predict kernels are called with."""
    X = X.float()
    return X if X.stride(1) == 1 else X.contiguous()


def tree_predict_plan(X: torch.Tensor, n_nodes: int, T: int, K: int, n_values: int) -> Dict[str, object]:
    """What :func:`tree_predict` launches for these device rows and a forest of ``n_nodes`` nodes, ``T`` trees and
    ``n_values`` leaf values, from the launcher's own host function (nothing is launched): ``staging`` (one of
    PREDICT_STAGING), ``n_nodes_lds`` / ``n_vals_lds`` (nodes / leaf values copied into LDS; 0: read from global
    memory), ``grid`` and ``lds_bytes``."""
    assert _native(X)
    X = _predict_rows(X)
    n, d = X.shape
    out = np.zeros(5, dtype=np.int32)
    _lib.check(_lib.lib().cdna_tree_predict_plan(_ptr(X), n, d, X.stride(0), int(n_nodes), int(T), int(K),
                                                 int(n_values), out.ctypes.data), "cdna_tree_predict_plan")
    stage, nn, nv, grid, lds = (int(v) for v in out)
    return {"staging": PREDICT_STAGING[stage], "n_nodes_lds": nn, "n_vals_lds": nv, "grid": grid, "lds_bytes": lds}


def tree_predict_heap_plan(X: torch.Tensor, depth: int, T: int) -> Dict[str, object]:
    """What :func:`tree_predict_heap` launches for these device rows and ``T`` trees of depth ``depth`` (the
    launcher's own host function; nothing is launched): ``fits`` (False: over the LDS budget, the call returns
    None), ``lds_bytes``, ``staging``, ``grid`` and ``grid_resident`` (the blocks with PREDICT_RESIDENT off / on;
    the latter 0 when the forest does not fit)."""
    assert _native(X)
    X = _predict_rows(X)
    n, d = X.shape
    out = np.zeros(8, dtype=np.int32)
    _lib.check(_lib.lib().cdna_tree_predict_heap_plan(_ptr(X), n, d, X.stride(0), int(depth), int(T), 0,
                                                      out.ctypes.data), "cdna_tree_predict_heap_plan")
    return {"fits": bool(out[0]), "lds_bytes": int(out[1]), "staging": PREDICT_STAGING[int(out[2])],
            "grid": int(out[3]), "grid_resident": int(out[4])}


def tree_predict_heap_binned_plan(n: int, G: int, d: int, depth: int, T: int) -> Dict[str, object]:
    """What :func:`tree_predict_heap_binned` launches on a device (the launcher's own host function; nothing is
    launched): ``fits``, ``lds_bytes``, ``nt`` (trees per wave and pass: the kernel's template argument),
    ``passes`` (over a wave's trees), ``prefetch`` (the next tile's words held in registers) and ``grid``."""
    out = np.zeros(8, dtype=np.int32)
    _lib.check(_lib.lib().cdna_tree_predict_heap_plan(None, int(n), int(d), 0, int(depth), int(T), int(G),
                                                      out.ctypes.data), "cdna_tree_predict_heap_plan")
    return {"fits": bool(out[0]), "lds_bytes": int(out[1]), "nt": int(out[5]), "passes": int(out[6]),
            "prefetch": bool(out[2]), "grid": int(out[3])}


def tree_predict_heap(X: torch.Tensor, heap: torch.Tensor, depth: int, tree_w: torch.Tensor,
                      masks: torch.Tensor, base: float = 0.0, dtype=torch.float64) -> Optional[torch.Tensor]:
    """Single-output ensemble prediction over a packed heap forest (int32 [T, 2^(depth+2)-2], ``pack_heap``):
    fp64 leaves, weights and sums (Spark's Double predictions), stored as ``dtype``.  Returns None when the forest
    does not fit the kernel's LDS budget (use ``tree_predict``)."""
    n, d = X.shape
    T = heap.shape[0]
    if not _native(X):
        return None
    assert heap.dtype == torch.int32 and heap.dim() == 2 and heap.shape[1] == (4 << depth) - 2, \
        (tuple(heap.shape), depth)
    X = _predict_rows(X)
    out = torch.empty((n, 1), dtype=dtype, device=X.device)
    if n == 0:
        return out
    m = masks.int().contiguous() if masks.numel() else torch.zeros(8, dtype=torch.int32, device=X.device)
    f64 = dtype == torch.float64
    assert tree_w.numel() == T
    rc = _lib.lib().cdna_tree_predict_heap(_ptr(X), n, d, X.stride(0), _ptr(heap.contiguous()), depth,
                                           _ptr(tree_w.double().contiguous()), T, _ptr(m), float(base),
                                           None if f64 else _ptr(out), _ptr(out) if f64 else None,
                                           int(PREDICT_RESIDENT), _stream(X.device))
    if rc == 1:  # hipErrorInvalidValue: over the LDS budget
        return None
    _lib.check(rc, "cdna_tree_predict_heap")
    return out


def bin_upper_edges(thresholds: np.ndarray, nthr: np.ndarray, B: int) -> np.ndarray:
    """[d, B] fp32: feature f's bin b -> the fp32 threshold t_b the bins were cut with (binize: bin(x) = #{t_j <
    x}), +inf for b >= nthr[f] (the last bin and NaN).  ``tree_predict_heap_binned``'s dequantisation table."""
    d = thresholds.shape[0]
    up = np.full((d, B), np.inf, dtype=np.float32)
    for f in range(d):
        k = int(min(max(nthr[f], 0), B, thresholds.shape[1]))
        up[f, :k] = thresholds[f, :k].astype(np.float32)
    return up


def heap_predict_host(Xf: torch.Tensor, heap: torch.Tensor, depth: int, tree_w: torch.Tensor,
                      base: float = 0.0) -> torch.Tensor:
    """Host walk of a packed predict heap (numeric and pass-through slots) on fp32 rows -> [n] fp64, summed in the
    device kernels' order (``ordered_tree_sum``): the cpu twin of ``tree_predict_heap`` and, on dequantised bins
    (``bin_upper_edges``), of ``tree_predict_heap_binned``."""
    Xf = Xf.float().cpu()
    h = heap.cpu()
    n, T = Xf.shape[0], h.shape[0]
    NI = (1 << depth) - 1
    tw = tree_w.double().cpu()
    rows = torch.arange(n)

    def contrib(t):
        slots = h[t, :2 * NI].reshape(max(NI, 0), 2)
        leaf = h[t, 2 * NI:].contiguous().view(torch.float64)
        idx = torch.zeros(n, dtype=torch.long)
        for _ in range(depth):
            nd = slots[idx]
            f = nd[:, 0].long()
            if bool((f < -1).any()):
                raise ValueError("heap_predict_host: categorical slots are not supported")
            thr = nd[:, 1].contiguous().view(torch.float32)
            x = Xf[rows, f.clamp(min=0)]
            go_left = (f < 0) | (x <= thr)
            idx = 2 * idx + torch.where(go_left, 1, 2)
        return (tw[t] * leaf[idx - NI])[:, None]
    out = ordered_tree_sum(contrib, T, n, 1, torch.tensor([float(base)], dtype=torch.float64))
    return out[:, 0]


def tree_predict_heap_binned(bins: torch.Tensor, thr_up: torch.Tensor, d: int, heap: torch.Tensor, depth: int,
                             tree_w: torch.Tensor, base: float = 0.0, dtype=torch.float64) -> Optional[torch.Tensor]:
    """``tree_predict_heap`` over the uint8 bins the features were cut into (trees.hip predict_heap_binned_kernel):
    bins [G, n, 8] (binize's column groups), thr_up fp32 [d, B] (``bin_upper_edges``).  x <= v <=> t_bin(x) <= v
    for every threshold v of the binning, so the predictions equal ``tree_predict_heap`` on the fp32 rows bit for
    bit.  [n, 1] ``dtype``; None when over the kernel's LDS budget.  Numeric / pass-through heap slots only."""
    G, n, _ = bins.shape
    T = heap.shape[0]
    assert heap.dtype == torch.int32 and heap.dim() == 2 and heap.shape[1] == (4 << depth) - 2, \
        (tuple(heap.shape), depth)
    assert thr_up.dtype == torch.float32 and thr_up.dim() == 2 and thr_up.shape[0] == d and d <= 8 * G
    assert tree_w.numel() == T
    if not _native(bins):
        b = bins_to_matrix(bins, d).cpu().clamp(max=thr_up.shape[1] - 1)
        Xq = thr_up.cpu().gather(1, b.t().contiguous()).t()   # [n, d]: each bin's upper edge
        return heap_predict_host(Xq, heap, depth, tree_w, base).to(dtype)[:, None].to(bins.device)
    out = torch.empty((n, 1), dtype=dtype, device=bins.device)
    if n == 0:
        return out
    f64 = dtype == torch.float64
    heap = heap.contiguous()
    heap_b = torch.empty_like(heap)  # the slots as bin counts (trees.hip heap_to_bins_kernel)
    rc = _lib.lib().cdna_tree_predict_heap_binned(_ptr(bins.contiguous()), n, G, d, _ptr(thr_up.contiguous()),
                                                  thr_up.shape[1], _ptr(heap), depth,
                                                  _ptr(tree_w.double().contiguous()), T, float(base), _ptr(heap_b),
                                                  None if f64 else _ptr(out), _ptr(out) if f64 else None,
                                                  _stream(bins.device))
    if rc == 1:
        return None
    _lib.check(rc, "cdna_tree_predict_heap_binned")
    return out


def tree_predict(X: torch.Tensor, nodes: torch.Tensor, roots: torch.Tensor, tree_w: torch.Tensor,
                 values: torch.Tensor, masks: torch.Tensor, K: int, base: Optional[torch.Tensor] = None
                 ) -> torch.Tensor:
    """Ensemble prediction on raw features -> float64 [n, K] (fp64 leaf values, weights and sums; the cpu path
    sums in the kernel's order: ``ordered_tree_sum``).

    nodes: int32 [N, 4] packed as documented in trees.hip.
    """
    n, d = X.shape
    T = roots.numel()
    if _native(X):
        X = _predict_rows(X)
        out = torch.empty((n, K), dtype=torch.float64, device=X.device)
        if n:
            m = masks.int().contiguous() if masks.numel() else torch.zeros(8, dtype=torch.int32, device=X.device)
            nodes, roots = nodes.int().contiguous(), roots.int().contiguous()
            tree_w, values = tree_w.double().contiguous(), values.double().contiguous()
            base = None if base is None else base.double().contiguous()
            _lib.check(_lib.lib().cdna_tree_predict(_ptr(X), n, d, X.stride(0), _ptr(nodes), int(nodes.shape[0]),
                                                    _ptr(roots),
                                                    _ptr(tree_w), T, _ptr(values), _ptr(m), K, _ptr(base), _ptr(out),
                                                    int(values.numel()), _stream(X.device)), "cdna_tree_predict")
        return out
    Xf = X.float().cpu()
    nd = nodes.long().cpu()
    vals = values.double().cpu()
    tw = tree_w.double().cpu()
    mk = masks.long().cpu() & 0xFFFFFFFF

    def contrib(t):
        cur = _walk_to_leaf(Xf, nd, mk, int(roots[t]))
        off = nd[cur][:, 1]
        idx = off[:, None] + torch.arange(K)[None, :]
        return vals[idx] * tw[t]
    return ordered_tree_sum(contrib, T, n, K, base).to(X.device)


def _raw_left(x: torch.Tensor, f: torch.Tensor, payload: torch.Tensor, mk: torch.Tensor) -> torch.Tensor:
    """The predictors' decision on raw fp32 values ``x`` for packed node codes ``f`` (trees.hip): numeric (f >= 0)
    left iff x <= the fp32 threshold whose bits are ``payload`` (NaN goes right); categorical (f <= -2) left iff
    the bit (int)x of the mask at offset ``payload`` is set; (int)x out of [0, 256) and NaN go right."""
    cont = f >= 0
    thr = payload.to(torch.int32).view(torch.float32)
    okc = (x > -1) & (x < 256)  # (int)x in [0, 256), decided in float: false for NaN, +-inf and huge values
    cc = torch.where(okc, x, torch.zeros_like(x)).to(torch.int64)
    moff = torch.where(f <= -2, payload, torch.zeros_like(payload)).clamp(min=0)
    words = mk[(moff * 8 + (cc >> 5))] if mk.numel() else torch.zeros_like(cc)
    catleft = okc & ((words >> (cc & 31)) & 1).bool()
    return torch.where(cont, x <= thr, catleft)


def _walk_to_leaf(Xf: torch.Tensor, nd: torch.Tensor, mk: torch.Tensor, root: int) -> torch.Tensor:
    """Node id [n] (int64) each fp32 row of ``Xf`` reaches from ``root`` in the packed int64 node table ``nd``."""
    n = Xf.shape[0]
    rows = torch.arange(n)
    cur = torch.full((n,), root, dtype=torch.long)
    for _ in range(64):
        nv = nd[cur]
        internal = nv[:, 0] != -1
        if not internal.any():
            break
        f = nv[:, 0]
        fi = torch.where(f >= 0, f, -f - 2).clamp(min=0)
        left = _raw_left(Xf[rows, fi], f, nv[:, 1], mk)
        nxt = torch.where(left, nv[:, 2], nv[:, 3])
        cur = torch.where(internal, nxt, cur)
    return cur


# -------------------------------------------------------------------- K21
def tree_leaf_index(X: torch.Tensor, nodes: torch.Tensor, roots: torch.Tensor, masks: torch.Tensor) -> torch.Tensor:
    """int32 [n, T]: the global node id of the leaf each row reaches in each tree, with ``tree_predict``'s node
    table and split decisions (shap.hip tree_leaf_index_kernel; on cpu ``tree_predict``'s walk)."""
    n, d = X.shape
    T = roots.numel()
    if _native(X):
        X = X.float()
        X = X if X.stride(1) == 1 else X.contiguous()
        out = torch.empty((n, T), dtype=torch.int32, device=X.device)
        if n and T:
            m = masks.int().contiguous() if masks.numel() else torch.zeros(8, dtype=torch.int32, device=X.device)
            _lib.check(_lib.lib().cdna_tree_leaf_index(_ptr(X), n, d, X.stride(0), _ptr(nodes.int().contiguous()),
                                                       _ptr(roots.int().contiguous()), T, _ptr(m), _ptr(out),
                                                       _stream(X.device)), "cdna_tree_leaf_index")
        return out
    Xf = X.float().cpu()
    nd = nodes.long().cpu()
    mk = masks.long().cpu() & 0xFFFFFFFF
    out = torch.empty((n, T), dtype=torch.int32)
    for t in range(T):
        out[:, t] = _walk_to_leaf(Xf, nd, mk, int(roots[t])).int()
    return out.to(X.device)


SHAP_MAX_SLOTS = 32
# Where a wave's phi tile accumulates: "global" (a [d][65] fp64 tile of scratch per block) or "lds" (while the tile
# fits the CU's LDS, else global).  Measured at 1e6 x 100 (profiles/r7/tree_shap.md): the LDS tile allows 2-3 waves
# per CU and the path loops are latency-bound, so the global tile with 16 blocks per CU is 2.2-2.6x faster.
SHAP_PHI = "global"
SHAP_GRID_LDS = 8192     # blocks (one wave each, grid-stride over 64-row tiles)
SHAP_GRID_GLOBAL = 4096  # 16 per CU; 8192 measured the same, 1024 1.3-2.1x slower
SHAP_SCRATCH_BYTES = 256 << 20  # cap of the global arrangement's scratch (fewer blocks at large d)


def tree_shap(X: torch.Tensor, paths: Dict[str, torch.Tensor], pv: torch.Tensor, bias: float, d: int,
              max_slots: int, binned: bool = False, phi: str = "auto", margin_base: Optional[float] = None):
    """Exact path-dependent TreeSHAP (Lundberg et al. 2018, Algorithm 2, per leaf path) -> fp64 [n, d + 1].

    With ``margin_base`` the result is (phi, margin): margin fp64 [n] = margin_base + the ``pv`` of the leaf the row
    reaches in every tree, added in path order -- the ensemble's raw prediction in fp64 from the same decisions,
    summed independently of the contributions.

    ``paths``: the tables of ``Forest.shap_paths`` on X's device (hdr, steps, slot_feat, slot_z, slot_rz, masks);
    ``pv`` fp64 [P]: tree weight * leaf value per path; column d of the result is ``bias``.  ``X``: fp32 rows
    [n, d], or with ``binned`` the uint8 bins [G, n, 8] of ``binize`` tested against node bins.  Every row's sums
    are made in (path, slot) order with each product rounded before it is added, on the device (shap.hip
    tree_shap_kernel) as in the cpu path below, which is vectorised over the rows."""
    if max_slots > SHAP_MAX_SLOTS:
        raise ValueError(f"TreeSHAP: {max_slots} distinct features on one path; at most {SHAP_MAX_SLOTS}")
    if binned:
        G, n, _ = X.shape
        assert X.dtype == torch.uint8 and d <= 8 * G, (X.dtype, d, G)
    else:
        n = X.shape[0]
        assert X.shape[1] == d, (tuple(X.shape), d)
    hdr, steps = paths["hdr"], paths["steps"]
    P = hdr.shape[0]
    if _native(X):
        out = torch.empty((n, d + 1), dtype=torch.float64, device=X.device)
        margin = None if margin_base is None else torch.empty(n, dtype=torch.float64, device=X.device)
        if n == 0:
            return out if margin is None else (out, margin)
        if not binned:
            X = X.float()
            X = X if X.stride(1) == 1 else X.contiguous()
        else:
            X = X.contiguous()
        L = _lib.lib()
        mode = SHAP_PHI if phi == "auto" else phi
        assert mode in ("lds", "global"), mode
        if mode == "lds" and L.cdna_tree_shap_lds_bytes(d, int(binned)) > L.cdna_tree_shap_lds_budget():
            mode = "global"  # any d: beyond what LDS holds the same kernel accumulates in its global tile
        tiles = (n + 63) // 64
        grid = min(tiles, SHAP_GRID_LDS) if mode == "lds" else \
            min(tiles, SHAP_GRID_GLOBAL, max(256, SHAP_SCRATCH_BYTES // (d * 65 * 8)))
        scratch = None if mode == "lds" else torch.empty(grid * d * 65, dtype=torch.float64, device=X.device)
        _lib.check(L.cdna_tree_shap(_ptr(X), int(binned), n, d, 0 if binned else X.stride(0), _ptr(hdr), P,
                                    _ptr(steps), _ptr(paths["slot_feat"]), _ptr(paths["slot_z"]),
                                    _ptr(paths["slot_rz"]), _ptr(pv), _ptr(paths["masks"]), float(bias),
                                    int(max_slots), int(mode == "lds"), _ptr(scratch), grid, _ptr(out),
                                    0.0 if margin is None else float(margin_base), _ptr(margin),
                                    _stream(X.device)), "cdna_tree_shap")
        return out if margin is None else (out, margin)
    out = torch.zeros((n, d + 1), dtype=torch.float64)
    out[:, d] = float(bias)
    margin = torch.full((n,), 0.0 if margin_base is None else float(margin_base), dtype=torch.float64)

    def result():
        return out.to(X.device) if margin_base is None else (out.to(X.device), margin.to(X.device))
    if n == 0:
        return result()
    Xv = bins_to_matrix(X, d).long() if binned else X.float().cpu()
    mk = paths["masks"].long() & 0xFFFFFFFF
    hd, stp = hdr.tolist(), steps.long()
    sfeat, sz, srz, pvl = paths["slot_feat"].tolist(), paths["slot_z"].double(), paths["slot_rz"].double(), \
        pv.double().tolist()
    inv = [0.0] + [1.0 / i for i in range(1, SHAP_MAX_SLOTS + 2)]
    for p, (s0, ns, k0, m) in enumerate(hd):
        if m == 0:
            margin += pvl[p]  # a single-leaf tree: every row reaches it
            continue
        on = torch.ones((m, n), dtype=torch.bool)
        for s in range(s0, s0 + ns):
            code, pay, go_left, slot = stp[s].tolist()
            f = code if code >= 0 else -code - 2
            if binned:
                b = Xv[:, f]
                left = (b <= pay) if code >= 0 else ((mk[pay * 8 + (b >> 5)] >> (b & 31)) & 1).bool()
            else:
                left = _raw_left(Xv[:, f], torch.full((n,), code), torch.full((n,), pay), mk)
            on[slot] &= left == bool(go_left)
        margin += on.all(0).double() * pvl[p]  # the rows that reach this path's leaf
        o = on.double()
        z = sz[k0:k0 + m]
        pw = torch.zeros((m + 1, n), dtype=torch.float64)
        pw[0] = 1.0
        for k in range(m):  # extend by slot k: elementwise the device loop j = l-1 .. 0
            l_ = k + 1
            rl = inv[l_ + 1]
            c1 = torch.tensor([(j + 1) * rl for j in range(l_)], dtype=torch.float64)[:, None]
            c2 = torch.tensor([(l_ - j) * rl for j in range(l_)], dtype=torch.float64)[:, None]
            old = pw[:l_].clone()
            pw[:l_] = (z[k] * old) * c2
            pw[1:l_ + 1] = pw[1:l_ + 1] + (o[k] * old) * c1
        mp1, rm1 = float(m + 1), inv[m + 1]
        zc = z[:, None]
        nxt = pw[m].expand(m, n).clone()
        tot1 = torch.zeros((m, n), dtype=torch.float64)
        tot0 = torch.zeros((m, n), dtype=torch.float64)
        for j in range(m - 1, -1, -1):  # the unwound sums of all m slots at once
            tmp = nxt * (mp1 * inv[j + 1])
            tot1 = tot1 + tmp
            nxt = pw[j] - (tmp * zc) * ((m - j) * rm1)
            tot0 = tot0 + pw[j] * (mp1 * inv[m - j])
        tot0 = tot0 * srz[k0:k0 + m, None]
        c = (torch.where(on, tot1, tot0) * (o - zc)) * pvl[p]
        for k in range(m):
            out[:, sfeat[k0 + k]] += c[k]
    return result()


def predict_binned_add(bins: torch.Tensor, nodes: torch.Tensor, root: int, values: torch.Tensor,
                       masks: torch.Tensor, scale: float, out: torch.Tensor) -> None:
    """out[r] += scale * leaf value of a bin-threshold tree (GBDT margin update).

    (A/B, profiles/r4/gbdt_predict_ab.md: the tree in LDS with four walks per thread measured 3.16 ms and a
    row-major walk 14 ms against this kernel's 2.37 ms per round at 1e8 rows; both dropped.)"""
    G, n, _ = bins.shape
    if n == 0:
        return
    if _native(bins):
        m = masks.int().contiguous() if masks.numel() else torch.zeros(8, dtype=torch.int32, device=bins.device)
        nodes, values = nodes.int().contiguous(), values.float().contiguous()
        assert out.dtype == torch.float32 and out.is_contiguous()
        _lib.check(_lib.lib().cdna_predict_binned_add(_ptr(bins), n, _ptr(nodes), int(root), _ptr(values), _ptr(m),
                                                      float(scale), _ptr(out), _stream(bins.device)),
                   "cdna_predict_binned_add")
        return
    bm = bins_to_matrix(bins, G * 8)
    nd = nodes.long()
    mk = masks.long() & 0xFFFFFFFF
    rows = torch.arange(n)
    cur = torch.full((n,), int(root), dtype=torch.long)
    for _ in range(64):
        nv = nd[cur]
        internal = nv[:, 0] != -1
        if not internal.any():
            break
        f = nv[:, 0]
        cont = f >= 0
        fi = torch.where(cont, f, -f - 2).clamp(min=0)
        b = bm[rows, fi]
        moff = torch.where(f <= -2, nv[:, 1], torch.zeros_like(f)).clamp(min=0)
        words = mk[(moff * 8 + (b >> 5))] if mk.numel() else torch.zeros_like(b)
        left = torch.where(cont, b <= nv[:, 1], ((words >> (b & 31)) & 1).bool())
        cur = torch.where(internal, torch.where(left, nv[:, 2], nv[:, 3]), cur)
    out += scale * values.float()[nd[cur][:, 1]]


def predict_binned_forest_host(bins: torch.Tensor, trees, scale: float, F: torch.Tensor) -> None:
    """Host twin of ``predict_binned_add`` over a WHOLE forest: every tree walks at once (one [T*n] cursor),
    so a 100-tree margin costs ~depth vector steps instead of 100 x depth.  ``trees[t] = (nodes, values,
    masks)`` as ``Forest.binned_arrays``; tree t adds to column ``t % F.shape[1]``, summed tree by tree in
    float32 like the per-tree path (identical results)."""
    G, n, _ = bins.shape
    T = len(trees)
    if n == 0 or T == 0:
        return
    bm = bins_to_matrix(bins, G * 8)
    nodes, vals, masks, roots = [], [], [], []
    no = vo = mo = 0
    for nd_t, v_t, m_t in trees:
        nd_t = nd_t.long().clone()
        leaf = nd_t[:, 0] == -1
        cat = nd_t[:, 0] <= -2
        nd_t[~leaf, 2:] += no
        nd_t[leaf, 1] += vo
        nd_t[cat, 1] += mo
        roots.append(no)
        nodes.append(nd_t)
        vals.append(v_t.float().reshape(-1))
        m_t = m_t.long().reshape(-1) & 0xFFFFFFFF
        masks.append(m_t)
        no += nd_t.shape[0]
        vo += vals[-1].numel()
        mo += m_t.numel() // 8
    nd = torch.cat(nodes)
    mk = torch.cat(masks)
    vv = torch.cat(vals)
    rows = torch.arange(n).repeat(T)
    cur = torch.tensor(roots, dtype=torch.long).repeat_interleave(n)
    for _ in range(64):
        nv = nd[cur]
        internal = nv[:, 0] != -1
        if not internal.any():
            break
        f = nv[:, 0]
        cont = f >= 0
        fi = torch.where(cont, f, -f - 2).clamp(min=0)
        b = bm[rows, fi]
        moff = torch.where(f <= -2, nv[:, 1], torch.zeros_like(f)).clamp(min=0)
        words = mk[(moff * 8 + (b >> 5))]
        left = torch.where(cont, b <= nv[:, 1], ((words >> (b & 31)) & 1).bool())
        cur = torch.where(internal, torch.where(left, nv[:, 2], nv[:, 3]), cur)
    leafv = vv[nd[cur][:, 1]].view(T, n)
    K = F.shape[1]
    for t in range(T):
        F[:, t % K] += scale * leafv[t]


# -------------------------------------------------------------------- K13
def reg_metrics(y: torch.Tensor, p: torch.Tensor, w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[Σw, Σw e², Σw|e|, Σw y, Σw y², Σw p, Σw p², Σw y p] as float64[8] (local)."""
    y = y.double().contiguous()
    p = p.double().contiguous()
    w = None if w is None else w.double().contiguous()
    if _native(y):
        acc = torch.zeros(8, dtype=torch.float64, device=y.device)
        part = torch.empty(8 * 1024, dtype=torch.float64, device=y.device)  # per-block partials (fixed-order sum)
        _lib.check(_lib.lib().cdna_reg_metrics(_ptr(y), _ptr(p), _ptr(w), y.numel(), _ptr(part), _ptr(acc),
                                               _stream(y.device)), "cdna_reg_metrics")
        return acc
    ww = torch.ones_like(y) if w is None else w
    e = y - p
    return torch.stack([ww.sum(), (ww * e * e).sum(), (ww * e.abs()).sum(), (ww * y).sum(), (ww * y * y).sum(),
                        (ww * p).sum(), (ww * p * p).sum(), (ww * y * p).sum()])


# -------------------------------------------------------------------- K14
def score_hist(score: torch.Tensor, label: torch.Tensor, lo: float, hi: float, nb: int) -> torch.Tensor:
    score = score.double().contiguous()
    label = label.double().contiguous()
    if _native(score):
        h = torch.zeros((nb, 2), dtype=torch.float64, device=score.device)
        _lib.check(_lib.lib().cdna_score_hist(_ptr(score), _ptr(label), score.numel(), float(lo), float(hi), nb,
                                              _ptr(h), _stream(score.device)), "cdna_score_hist")
        return h
    scale = nb / (hi - lo) if hi > lo else 0.0
    # clamped before the conversion, as in the kernel: +inf -> the last bucket, -inf and NaN -> bucket 0
    t = (score - lo) * scale
    b = torch.where(t.isnan(), torch.zeros_like(t), t).clamp(0, nb - 1).long()
    pos = (label > 0.5).long()
    h = torch.zeros(nb * 2, dtype=torch.float64)
    h.index_add_(0, b * 2 + pos, torch.ones_like(score))
    return h.view(nb, 2)


# -------------------------------------------------------------------- K10
def kmeans_step(X: torch.Tensor, C: torch.Tensor, with_sums: bool = True):
    """Assign rows to nearest centre; return (assign, sums[k,d], counts[k], cost) (local)."""
    n, d = X.shape
    k = C.shape[0]
    f64 = X.dtype == torch.float64   # Spark's Double vectors at course scale: the fp64 kernel instantiation
    if _native(X) and (2 * k * d + k) * (8 if f64 else 4) <= 64 * 1024:
        X = X if f64 else X.float()
        X = X if X.stride(1) == 1 else X.contiguous()
        Cf = C.to(X.dtype).contiguous()
        assign = torch.empty(n, dtype=torch.int32, device=X.device)
        sums = torch.zeros((k, d), dtype=torch.float64, device=X.device)
        counts = torch.zeros(k, dtype=torch.float64, device=X.device)
        cost = torch.zeros(1, dtype=torch.float64, device=X.device)
        if n:
            _lib.check(_lib.lib().cdna_kmeans_step(_ptr(X), n, d, X.stride(0), _ptr(Cf), k, _ptr(assign),
                                                   _ptr(sums) if with_sums else None,
                                                   _ptr(counts) if with_sums else None, _ptr(cost), int(f64),
                                                   _stream(X.device)), "cdna_kmeans_step")
        return assign, sums, counts, cost[0]
    Xf = X if f64 else X.float()
    dist = ((Xf[:, None, :] - C.to(Xf.dtype)[None, :, :]) ** 2).sum(2) if f64 else torch.cdist(Xf, C.float()) ** 2
    best, assign = dist.min(dim=1)
    sums = torch.zeros((k, d), dtype=torch.float64, device=X.device)
    sums.index_add_(0, assign, Xf.double())
    counts = torch.bincount(assign, minlength=k).double()
    return assign.int(), sums, counts, best.double().sum()


# -------------------------------------------------------------------- K11
def logistic_grad(X: torch.Tensor, y: torch.Tensor, w: torch.Tensor, b: float,
                  wt: Optional[torch.Tensor] = None):
    """Binary logistic loss and gradient (local sums): returns (grad[d+1], loss)."""
    n, d = X.shape
    y = y.double().contiguous()
    wt = None if wt is None else wt.double().contiguous()
    if _native(X) and d <= 512:
        f64 = X.dtype == torch.float64   # Double vectors (course scale): the fp64 instantiation reads them as is
        X = X if f64 else X.float()
        X = X if X.stride(1) == 1 else X.contiguous()
        wd = w.double().contiguous()
        grad = torch.zeros(d + 1, dtype=torch.float64, device=X.device)
        loss = torch.zeros(1, dtype=torch.float64, device=X.device)
        if n:
            _lib.check(_lib.lib().cdna_logistic_grad(_ptr(X), n, d, X.stride(0), _ptr(y), _ptr(wt), _ptr(wd),
                                                     float(b), _ptr(grad), _ptr(loss), int(f64), _stream(X.device)),
                       "cdna_logistic_grad")
        return grad, loss[0]
    Xd = X.double()
    m = Xd @ w.double() + b
    p = torch.sigmoid(m)
    ww = torch.ones_like(y) if wt is None else wt
    res = ww * (p - y)
    g = torch.empty(d + 1, dtype=torch.float64, device=X.device)
    g[:d] = Xd.T @ res
    g[d] = res.sum()
    loss = (ww * (torch.nn.functional.softplus(m) - y * m)).sum()
    return g, loss


# -------------------------------------------------------------------- K22
GLM_FAMILY = {"gaussian": 0, "binomial": 1, "poisson": 2, "gamma": 3, "tweedie": 4}
GLM_LINK = {"identity": 0, "log": 1, "inverse": 2, "logit": 3, "probit": 4, "cloglog": 5, "sqrt": 6, "power": 7}
GLM_STEP, GLM_INIT, GLM_EVAL = 0, 1, 2
GLM_EPS = 1e-16      # Spark's clamp of the mean (binomial into [eps, 1 - eps], poisson / gamma / tweedie >= eps)
GLM_MAX_D = 126      # the fused kernel's range: d + 2 <= 128
_SQRT_2PI = 2.5066282746310002


def glm_link(link: str, mu: torch.Tensor, lp: float = 0.0) -> torch.Tensor:
    """eta = g(mu) (fp64 tensors; ``lp`` is the exponent of the "power" link)."""
    if link == "identity":
        return mu
    if link == "log":
        return torch.log(mu)
    if link == "inverse":
        return 1.0 / mu
    if link == "logit":
        return torch.log(mu / (1.0 - mu))
    if link == "probit":
        return torch.special.ndtri(mu)
    if link == "cloglog":
        return torch.log(-torch.log(1.0 - mu))
    if link == "sqrt":
        return torch.sqrt(mu)
    return torch.pow(mu, lp)


def glm_unlink(link: str, eta: torch.Tensor, lp: float = 0.0) -> torch.Tensor:
    """mu = g^-1(eta), before the family's clamp."""
    if link == "identity":
        return eta
    if link == "log":
        return torch.exp(eta)
    if link == "inverse":
        return 1.0 / eta
    if link == "logit":
        return 1.0 / (1.0 + torch.exp(-eta))
    if link == "probit":
        return torch.special.ndtr(eta)
    if link == "cloglog":
        return 1.0 - torch.exp(-torch.exp(eta))
    if link == "sqrt":
        return eta * eta
    return torch.pow(eta, 1.0 / lp)


def glm_dlink(link: str, mu: torch.Tensor, lp: float = 0.0) -> torch.Tensor:
    """g'(mu)."""
    if link == "identity":
        return torch.ones_like(mu)
    if link == "log":
        return 1.0 / mu
    if link == "inverse":
        return -1.0 / (mu * mu)
    if link == "logit":
        return 1.0 / (mu * (1.0 - mu))
    if link == "probit":
        q = torch.special.ndtri(mu)
        return _SQRT_2PI * torch.exp(0.5 * q * q)
    if link == "cloglog":
        return 1.0 / ((mu - 1.0) * torch.log(1.0 - mu))
    if link == "sqrt":
        return 0.5 / torch.sqrt(mu)
    return lp * torch.pow(mu, lp - 1.0)


def glm_clamp(family: str, mu: torch.Tensor) -> torch.Tensor:
    # NaN stays NaN (torch.where, not clamp): the step counts such rows instead of hiding them
    if family == "binomial":
        mu = torch.where(mu < GLM_EPS, torch.full_like(mu, GLM_EPS), mu)
        return torch.where(mu > 1.0 - GLM_EPS, torch.full_like(mu, 1.0 - GLM_EPS), mu)
    if family == "gaussian":
        return mu
    return torch.where(mu < GLM_EPS, torch.full_like(mu, GLM_EPS), mu)


def glm_variance(family: str, mu: torch.Tensor, vp: float = 0.0) -> torch.Tensor:
    if family == "gaussian":
        return torch.ones_like(mu)
    if family == "binomial":
        return mu * (1.0 - mu)
    if family == "poisson":
        return mu
    if family == "gamma":
        return mu * mu
    return torch.pow(mu, vp)


def _ylogy(y: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
    return torch.where(y == 0, torch.zeros_like(y), y * torch.log(y / mu))


def _tw_yp(y, mu, p: float):
    return torch.log(y / mu) if p == 0.0 else (torch.pow(y, p) - torch.pow(mu, p)) / p


def glm_unit_deviance(family: str, y: torch.Tensor, mu: torch.Tensor, vp: float = 0.0) -> torch.Tensor:
    """d(y, mu); a row's deviance is its weight times this."""
    if family == "gaussian":
        return (y - mu) * (y - mu)
    if family == "binomial":
        return 2.0 * (_ylogy(y, mu) + _ylogy(1.0 - y, 1.0 - mu))
    if family == "poisson":
        return 2.0 * (_ylogy(y, mu) - (y - mu))
    if family == "gamma":
        return -2.0 * (torch.log(y / mu) - (y - mu) / mu)
    y1 = y.clamp_min(0.1) if 1.0 <= vp < 2.0 else y
    return 2.0 * (y * _tw_yp(y1, mu, 1.0 - vp) - _tw_yp(y, mu, 2.0 - vp))


def glm_init_mu(family: str, y: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The family's starting mean (R / Spark)."""
    if family == "binomial":
        return (w * y + 0.5) / (w + 1.0)
    if family in ("poisson", "tweedie"):
        return y.clamp_min(0.1)
    return y


def matvec64(X: torch.Tensor, beta: torch.Tensor, chunk: int = 1 << 20) -> torch.Tensor:
    """X @ beta in fp64 without an fp64 copy of a large fp32 X."""
    b = beta.double().to(X.device)
    if X.dtype == torch.float64 or X.shape[0] <= chunk:
        return X.double() @ b
    return torch.cat([X[i:i + chunk].double() @ b for i in range(0, X.shape[0], chunk)])


def glm_row_terms(y, w, offset, lin, family: str, link: str, vp: float, lp: float, mode: int):
    """(eta, mu, W, z, finite) of every row, fp64: ``lin`` is b + x.beta (ignored in INIT mode)."""
    if mode == GLM_INIT:
        mu = glm_clamp(family, glm_init_mu(family, y, w))
        eta = glm_link(link, mu, lp)
    else:
        eta = offset + lin
        mu = glm_clamp(family, glm_unlink(link, eta, lp))
    gp = glm_dlink(link, mu, lp)
    W = w / (glm_variance(family, mu, vp) * gp * gp)
    z = eta - offset + (y - mu) * gp
    fin = torch.isfinite(mu) & torch.isfinite(W) & torch.isfinite(z)
    return eta, mu, W, z, fin


def glm_step(X: torch.Tensor, y: torch.Tensor, w: Optional[torch.Tensor], offset: Optional[torch.Tensor],
             beta: Optional[torch.Tensor], intercept: float, shift: Optional[torch.Tensor], zshift: float,
             family: str, link: str, var_power: float = 0.0, link_power: float = 0.0, mode: int = GLM_STEP):
    """One IRLS pass of a generalized linear model (local sums): returns (G[d+2, d+2], stats[4]), both fp64.

    Per row, in fp64: eta = offset + intercept + x.beta, mu = g^-1(eta) clamped as Spark's families clamp it,
    gp = g'(mu), working weight W = w / (V(mu) gp^2), working response z = eta - offset + (y - mu) gp.
    G is the Gram of sqrt(W) [x - shift | 1 | z - zshift] in K.gram's layout (sum W x~x~^T, sum W x~, sum W,
    sum W x~ z~, sum W z~, sum W z~^2); stats = [sum w d(y, mu), sum w, sum w y, rows whose mu, W or z is not
    finite].  Such rows are left out of G and of the sums: their augmented row is zeroed, so an inf / NaN feature
    that makes eta non-finite does not reach G (in INIT mode the features do not enter eta, and a non-finite
    feature goes into G as it is).  ``zshift`` is used as its fp32 rounding.
    mode GLM_INIT: eta = g(mu0) with the family's starting mean from the label, beta unused.
    mode GLM_EVAL: stats only, G is zeros.
    family / link are names (GLM_FAMILY, GLM_LINK); "power" takes ``link_power``, "tweedie" ``var_power``.

    fp32 X on a GPU with d + 2 <= 128 (any n >= 1, row stride and alignment) runs the fused K22 kernel: one
    launch that reads X once, exact-fp32 MFMA Gram with the augmented row rounded to fp32, partial sums reduced
    in a fixed order: two calls on the same input return the same bits.  Bit-identical reruns of G are part of
    the contract inside this range only: past the cap G comes from torch elementwise ops and K.gram's fp32 path
    (itself bit-identical on reruns, tests/test_gram_gpu.py).  Everything else takes the host formulation, the
    same formulas as torch fp64 ops: fp64 X entirely in fp64; fp32 X past the cap on a GPU through a scaled copy and
    K.gram(fp64=False).
    """
    n, d = X.shape
    dev = X.device
    fam_id, link_id = GLM_FAMILY[family], GLM_LINK[link]
    zs = float(np.float32(zshift))
    yd = y.double().contiguous()
    wd = None if w is None else w.double().contiguous()
    od = None if offset is None else offset.double().contiguous()
    if X.dtype not in (torch.float32, torch.float64):
        X = X.float()
    if _native(X) and X.dtype == torch.float32 and 1 <= d <= GLM_MAX_D and n >= 1:
        X = X if X.stride(1) == 1 and X.stride(0) >= d else X.contiguous()
        bd = None if beta is None else beta.double().to(dev).contiguous()
        sh = None if shift is None else shift.float().to(dev).contiguous()
        L = _lib.lib()
        ws = torch.empty(max(L.cdna_glm_step_workspace(n, d), 1), dtype=torch.float32, device=dev)
        sws = torch.empty(4 * L.cdna_glm_step_blocks(n), dtype=torch.float64, device=dev)
        G = torch.zeros((d + 2, d + 2), dtype=torch.float64, device=dev)
        stats = torch.zeros(4, dtype=torch.float64, device=dev)
        _lib.check(L.cdna_glm_step(_ptr(X), n, d, X.stride(0), _ptr(yd), _ptr(wd), _ptr(od), _ptr(bd),
                                   float(intercept), _ptr(sh), zs, fam_id, link_id, float(var_power),
                                   float(link_power), int(mode), _ptr(G), _ptr(stats), _ptr(ws), _ptr(sws),
                                   _stream(dev)), "cdna_glm_step")
        return G, stats
    # host formulation
    ww = torch.ones_like(yd) if wd is None else wd
    oo = torch.zeros_like(yd) if od is None else od
    lin = None
    if mode != GLM_INIT:
        lin = float(intercept) + (matvec64(X, beta) if beta is not None else torch.zeros_like(yd))
    _, mu, W, z, fin = glm_row_terms(yd, ww, oo, lin, family, link, var_power, link_power, mode)
    zero = torch.zeros_like(yd)
    wf = torch.where(fin, ww, zero)
    stats = torch.stack([torch.where(fin, ww * glm_unit_deviance(family, yd, mu, var_power), zero).sum(),
                         wf.sum(), (wf * yd).sum(), (~fin).sum().double()])
    if mode == GLM_EVAL:
        return torch.zeros((d + 2, d + 2), dtype=torch.float64, device=dev), stats
    sw = torch.sqrt(torch.where(fin, W, zero))
    zt = sw * (torch.where(fin, z, zero) - zs)
    if X.dtype == torch.float32 and _native(X) and d + 3 <= 512:
        # past the fused kernel's range: a sqrt(W)-scaled copy with sqrt(W) itself as an extra feature, then K1
        sw32 = sw.float()[:, None]
        Xw = torch.cat([(X - (shift.float().to(dev) if shift is not None else 0.0)) * sw32, sw32], 1)
        Xw = torch.where(fin[:, None], Xw, torch.zeros_like(Xw))
        G3 = gram(Xw, zt.float(), None, 0.0, fp64=False) if n else \
            torch.zeros((d + 3, d + 3), dtype=torch.float64, device=dev)
        keep = torch.tensor(list(range(d + 1)) + [d + 2], device=dev)
        return G3[keep][:, keep].contiguous(), stats
    A = torch.empty((n, d + 2), dtype=torch.float64, device=dev)
    if X.dtype == torch.float64:
        A[:, :d] = (X if shift is None else X - shift.double().to(dev)) * sw[:, None]
    else:   # the kernel's arithmetic: x - shift and its scaling in fp32
        A[:, :d] = (X if shift is None else X - shift.float().to(dev)) * sw.float()[:, None]
    A[:, d] = sw
    A[:, d + 1] = zt
    A = torch.where(fin[:, None], A, torch.zeros_like(A))   # a left-out row is zeroed, not scaled by 0
    if X.dtype == torch.float32:
        A = A.float().double()   # the augmented row rounded to fp32, as the kernel feeds it to the MFMA
    return A.T @ A, stats


# ------------------------------------------------------------ K23 gmm_step (gmm.hip)
GMM_STEP, GMM_PREDICT, GMM_EVAL = 0, 1, 2
GMM_EPS = 2.0 ** -52   # Spark's EPSILON: added to every component density
GMM_MAX_D = 127        # the fused kernels' range: d + 1 <= 128
GMM_MAX_K = 32         # and 2 <= k <= 32
GMM_HOST_CHUNK = 1 << 18   # rows per pass of the host formulation (bounds its [rows, d] intermediates)


def gmm_centres(mu: torch.Tensor, A: torch.Tensor, f32: bool):
    """(c, A', corr) of the op's definition, fp64 tensors: the centres, the matrices as the products use them
    and the constant A'_j (mu_j - c_j).  For fp32 X the centres and the matrices are rounded to fp32."""
    mu, A = mu.double(), A.double()
    if not f32:
        return mu, A, torch.zeros(mu.shape, dtype=torch.float64, device=mu.device)
    c, Ar = mu.float().double(), A.float().double()
    return c, Ar, torch.einsum("jab,jb->ja", Ar, mu - c)


class GmmPrepared:
    """The parameters of one mixture as ``gmm_step`` consumes them, prepared once per (device, row dtype, path)
    and reused by every call that is given this object: a model's transform goes through the op once per batch."""

    def __init__(self, mu: torch.Tensor, A: torch.Tensor, logc: torch.Tensor):
        self.mu, self.A, self.logc = mu.double(), A.double(), logc.double()
        self._made = {}

    def on(self, dev, f32: bool, native: bool):
        """(c, A', corr, logc) on ``dev``; for the native path (cf, AT, corr, logc): the kernels' zero-padded
        fp32 centres [k, dk], transposed matrices [k, dk, dc] and fp64 constants [k, dc]."""
        key = (str(dev), f32, native)
        if key not in self._made:
            c, Ar, corr = gmm_centres(self.mu.to(dev), self.A.to(dev), f32)
            lc = self.logc.to(dev).contiguous()
            if native:
                k, d = c.shape
                L = _lib.lib()
                dk, dc = L.cdna_gmm_dk(d), L.cdna_gmm_dc(d)
                cf = torch.zeros((k, dk), dtype=torch.float32, device=dev)
                cf[:, :d] = c
                AT = torch.zeros((k, dk, dc), dtype=torch.float32, device=dev)
                AT[:, :d, :d] = Ar.transpose(1, 2)
                cr = torch.zeros((k, dc), dtype=torch.float64, device=dev)
                cr[:, :d] = corr
                self._made[key] = (cf, AT, cr, lc)
            else:
                self._made[key] = (c, Ar, corr, lc)
        return self._made[key]


def gmm_step(X: torch.Tensor, w: Optional[torch.Tensor], mu: torch.Tensor, A: torch.Tensor, logc: torch.Tensor,
             mode: int = GMM_STEP, native: bool = True, prepared: Optional[GmmPrepared] = None):
    """One EM pass of a full-covariance Gaussian mixture over the local rows.

    X [n, d] fp32 or fp64, w [n] fp64 row weights or None, mu [k, d], A [k, d, d] with q_j(x) = |A_j (x - mu_j)|^2,
    logc [k] = log pi_j - (d log 2 pi + log pdet Sigma_j) / 2; all fp64.  Per row, in fp64 (Spark's formulas):
    p_j = GMM_EPS + exp(logc_j - q_j / 2), s = sum_j p_j, r_j = p_j / s; a row that underflows under every
    component gets uniform responsibilities.

    GMM_STEP returns (S [k, d+1, d+1], stats [3]): S_j = sum_rows w r_j [t | 1][t | 1]^T with t = x - c_j, c_j the
    centre the op uses (mu_j rounded to fp32 for fp32 X, mu_j itself for fp64 X), so new mean = c_j + S_j[:d, d] /
    N_j and new covariance = S_j[:d, :d] / N_j - delta delta^T with a small delta; stats = [sum w log s, sum w,
    rows whose q is not finite].  Such rows are left out of S and of the sums.
    GMM_PREDICT returns (R [n, k] fp64, assign [n] int32, stats): assign is the argmax of R, lowest index among
    equals; a left-out row has NaN responsibilities and assign 0.  GMM_EVAL returns stats.

    fp32 X is defined with this rounding, on the device and in the host formulation alike: t is the fp32
    difference, A_j is rounded to fp32, the constant A_j (mu_j - c_j) is subtracted from A_j t (the density is that
    of the fp64 mean), the row scaled by fp32 sqrt(w r_j) is rounded to fp32 before the moment product, and
    everything from q on is fp64.  fp64 X is fp64 throughout.

    fp32 X on a GPU with d <= GMM_MAX_D and 2 <= k <= GMM_MAX_K (any n >= 1, row stride and alignment) runs the
    K23 kernels: both products on the exact-fp32 MFMA, partial sums reduced in a fixed order, so two calls on the
    same input return the same bits; N_j = S_j[d, d] is summed there in fp64 from the unrounded w r_j.  Everything
    else takes the host formulation: the same formulas as torch ops (``native=False`` asks for it inside the range
    too: bench/gmm_micro.py times the two side by side).  ``prepared``: a GmmPrepared of the same (mu, A, logc),
    so that repeated calls with one mixture build its device tables once.
    """
    n, d = X.shape
    k = mu.shape[0]
    dev = X.device
    if X.dtype not in (torch.float32, torch.float64):
        X = X.float()
    f32 = X.dtype == torch.float32
    wd = None if w is None else w.double().to(dev).contiguous()
    prep = prepared if prepared is not None else GmmPrepared(mu, A, logc)
    if native and _native(X) and f32 and 1 <= d <= GMM_MAX_D and 2 <= k <= GMM_MAX_K and n >= 1:
        X = X if X.stride(1) == 1 and X.stride(0) >= d else X.contiguous()
        L = _lib.lib()
        cf, AT, cr, lc = prep.on(dev, True, True)
        # every entry of S and of stats is written by the reduction
        sws = torch.empty((3 + k) * L.cdna_gmm_step_blocks(n), dtype=torch.float64, device=dev)
        stats = torch.empty(3, dtype=torch.float64, device=dev)
        S = R = assign = ws = None
        if mode == GMM_STEP:
            S = torch.empty((k, d + 1, d + 1), dtype=torch.float64, device=dev)
            ws = torch.empty(L.cdna_gmm_step_workspace(n, d, k), dtype=torch.float32, device=dev)
        elif mode == GMM_PREDICT:
            R = torch.empty((n, k), dtype=torch.float64, device=dev)
            assign = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(L.cdna_gmm_step(_ptr(X), n, d, X.stride(0), _ptr(wd), _ptr(cf), _ptr(AT), _ptr(cr), _ptr(lc), k,
                                   int(mode), _ptr(S), _ptr(R), _ptr(assign), _ptr(stats), _ptr(ws), _ptr(sws),
                                   _stream(dev)), "cdna_gmm_step")
        return (S, stats) if mode == GMM_STEP else ((R, assign, stats) if mode == GMM_PREDICT else stats)
    # host formulation, GMM_HOST_CHUNK rows at a time
    c, Ar, corr, lc = prep.on(dev, f32, False)
    S = torch.zeros((k, d + 1, d + 1), dtype=torch.float64, device=dev)
    stats = torch.zeros(3, dtype=torch.float64, device=dev)
    Rs, As = [], []
    cx = c.to(X.dtype)
    Ax = Ar.to(X.dtype)
    for i0 in range(0, n, GMM_HOST_CHUNK):
        Xc = X[i0:i0 + GMM_HOST_CHUNK]
        wc = torch.ones(Xc.shape[0], dtype=torch.float64, device=dev) if wd is None else wd[i0:i0 + GMM_HOST_CHUNK]
        q = torch.stack([(((Xc - cx[j]) @ Ax[j].T).double() - corr[j]).square().sum(1) for j in range(k)], 1)
        bad = ~torch.isfinite(q).all(1)
        p = GMM_EPS + torch.exp(lc - 0.5 * q)
        s = p.sum(1)
        r = p / s[:, None]
        zero = torch.zeros_like(s)
        stats += torch.stack([torch.where(bad, zero, wc * torch.log(s)).sum(), torch.where(bad, zero, wc).sum(),
                              bad.sum().double()])
        if mode == GMM_PREDICT:
            Rs.append(torch.where(bad[:, None], torch.full_like(r, float("nan")), r))
            As.append(torch.where(bad, torch.zeros_like(bad, dtype=torch.int64), torch.argmax(r, 1)).to(torch.int32))
        elif mode == GMM_STEP:
            sr = torch.sqrt(torch.where(bad[:, None], torch.zeros_like(r), wc[:, None] * r)).to(X.dtype)
            for j in range(k):
                sj = sr[:, j:j + 1]
                Z = torch.cat([torch.where(sj != 0, (Xc - cx[j]) * sj, torch.zeros_like(Xc)), sj], 1).double()
                S[j] += Z.T @ Z
    if mode == GMM_STEP:
        return S, stats
    if mode == GMM_PREDICT:
        if not Rs:
            return (torch.zeros((0, k), dtype=torch.float64, device=dev),
                    torch.zeros(0, dtype=torch.int32, device=dev), stats)
        return torch.cat(Rs), torch.cat(As), stats
    return stats


# ------------------------------------------------------------ K24 mlp_step (mlp.hip)
MLP_STEP, MLP_PREDICT = 0, 1
MLP_MAX_WIDTH = 128        # the fused kernel's range: every layer width, the input's d included, <= 128
MLP_MAX_LAYERS = 3         # at most 3 affine layers (two hidden), i.e. len(layers) <= 4; and 2 <= classes
MLP_HOST_CHUNK = 1 << 18   # rows per pass of the host formulation (bounds its [rows, width] intermediates)


def mlp_num_params(layers) -> int:
    return sum(o * i + o for i, o in zip(layers[:-1], layers[1:]))


def mlp_unpack(theta: torch.Tensor, layers):
    """[(W [out, in], b [out])] per affine layer from Spark's flat vector: per layer W column-major (entry (o, i) at
    off + o + i * out), then the out biases."""
    out, off = [], 0
    for i, o in zip(layers[:-1], layers[1:]):
        out.append((theta[off:off + o * i].reshape(i, o).T, theta[off + o * i:off + o * i + o]))
        off += o * i + o
    return out


class MlpPrepared:
    """The weights of one net as ``mlp_step`` consumes them, prepared once per (device, row dtype, path) and reused
    by every call that is given this object: an objective evaluation's STEP, a model's PREDICT per batch."""

    def __init__(self, theta, layers):
        self.layers = [int(v) for v in layers]
        self.theta = torch.as_tensor(theta, dtype=torch.float64).reshape(-1).cpu()
        if self.theta.numel() != mlp_num_params(self.layers):
            raise ValueError(f"mlp_step: {self.theta.numel()} weights for layers {self.layers}, expected "
                             f"{mlp_num_params(self.layers)}")
        self._made = {}

    def on(self, dev, f32: bool, native: bool):
        """[(W, b)] fp64 on ``dev`` (the weights rounded to fp32 first for fp32 rows); for the native path the
        kernel's table: per layer the zero-padded fp32 W^T [in up to 2][out up to 32], W [out up to 2][in up to 32]
        and b [out up to 32]."""
        key = (str(dev), f32, native)
        if key not in self._made:
            th = self.theta.float().double() if f32 else self.theta
            Wb = mlp_unpack(th, self.layers)
            if native:
                L = _lib.lib()
                lay = np.asarray(self.layers, dtype=np.int32)
                plan = np.zeros(8, dtype=np.int64)
                off = np.zeros(3 * (len(lay) - 1), dtype=np.int64)
                _lib.check(L.cdna_mlp_plan(None, 1, int(lay[0]), lay.ctypes.data, len(lay), plan.ctypes.data),
                           "cdna_mlp_plan")
                _lib.check(L.cdna_mlp_table_offsets(lay.ctypes.data, len(lay), off.ctypes.data),
                           "cdna_mlp_table_offsets")
                tab = np.zeros(int(plan[7]), dtype=np.float32)
                r2, r32 = (lambda v: (v + 1) // 2 * 2), (lambda v: (v + 31) // 32 * 32)
                for l, (W, b) in enumerate(Wb):
                    o, i = W.shape
                    W32 = W.numpy().astype(np.float32)
                    tab[off[3 * l]:off[3 * l] + r2(i) * r32(o)].reshape(r2(i), r32(o))[:i, :o] = W32.T
                    tab[off[3 * l + 1]:off[3 * l + 1] + r2(o) * r32(i)].reshape(r2(o), r32(i))[:o, :i] = W32
                    tab[off[3 * l + 2]:off[3 * l + 2] + o] = b.numpy().astype(np.float32)
                self._made[key] = upload(dev, tab)[0]
            else:
                self._made[key] = [(W.to(dev).contiguous(), b.to(dev)) for W, b in Wb]
        return self._made[key]


def _row_plan(X: torch.Tensor, fn_name: str, nout: int, *args):
    """The answer of a row-streaming kernel's plan function ``fn_name(X, n, ldx, *args, out[nout])`` for these
    operands (None: the host formulation) and X as the kernel takes it: fp32 rows of unit stride."""
    if not _native(X) or X.dtype != torch.float32 or X.dim() != 2:
        return None, X
    X = X if X.stride(1) == 1 and X.stride(0) >= X.shape[1] else X.contiguous()
    out = np.zeros(nout, dtype=np.int64)
    _lib.check(getattr(_lib.lib(), fn_name)(_ptr(X), X.shape[0], X.stride(0), *args, out.ctypes.data), fn_name)
    return (out if out[0] else None), X


def _mlp_native_plan(X: torch.Tensor, layers):
    if X.dim() != 2 or X.shape[1] != layers[0]:
        return None, X
    lay = np.asarray(layers, dtype=np.int32)
    return _row_plan(X, "cdna_mlp_plan", 8, lay.ctypes.data, len(lay))


def mlp_plan(X: torch.Tensor, layers) -> Dict[str, object]:
    """What :func:`mlp_step` runs for these operands, from the dispatch's own host function (nothing is launched):
    ``path`` "native" or "host"; for the native path ``slots`` (gradient tiles per wave of the STEP instantiation:
    1, 3, 6 or 12), ``vw`` (4: float4 row loads, 1: scalar loads), ``nblk``, ``rows_per_block``, ``tiles`` (32 x 32
    gradient tiles over all layers) and ``lds`` (bytes per block)."""
    layers = [int(v) for v in layers]
    out, _ = _mlp_native_plan(X, layers)
    if out is None:
        return {"path": "host"}
    return {"path": "native", "slots": int(out[1]), "vw": int(out[2]), "nblk": int(out[3]),
            "rows_per_block": int(out[4]), "tiles": int(out[5]), "lds": int(out[6])}


def _first_argmax(Z: torch.Tensor) -> torch.Tensor:
    """argmax over dim 1, the lowest index among equals, int32."""
    C = Z.shape[1]
    idx = torch.arange(C, device=Z.device).expand_as(Z)
    return torch.where(Z == Z.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values \
        .clamp_max(C - 1).to(torch.int32)


def mlp_step(X: torch.Tensor, y: Optional[torch.Tensor], theta32, layers, mode: int = MLP_STEP, native: bool = True,
             prepared: Optional[MlpPrepared] = None):
    """Loss and gradient sums, or the predictions, of a multilayer perceptron over the local rows.

    X [n, layers[0]] fp32 or fp64, y [n] integer labels in [0, layers[-1]) (STEP only), ``theta32`` the flat weight
    vector in Spark's layout (see ``mlp_unpack``).  The net: one affine layer per consecutive pair of ``layers``,
    sigmoid after every layer but the last, softmax with cross-entropy on top.

    MLP_STEP returns (loss_sum fp64 scalar, grad_sum fp64 [P]): the sums over the rows of logsumexp(z) - z[label]
    and of its gradient in the flat layout, un-normalised.  MLP_PREDICT returns (raw [n, C] fp64, prob [n, C] fp64,
    pred [n] int32): the last affine layer's output, its softmax and the argmax of raw, the lowest index among
    equals.

    For fp32 X the op is defined at the weights rounded to fp32, on the device and in the host formulation alike;
    fp64 X uses them as they are.  fp32 X on a GPU with every width <= MLP_MAX_WIDTH, at most MLP_MAX_LAYERS affine
    layers and at least 2 classes (any n >= 1, row stride and alignment) runs the K24 kernel: every matmul on the
    exact-fp32 MFMA, fp32 sigmoid, the softmax, the loss and the delta of the top layer in fp64, per-block partial
    sums reduced in a fixed order (two calls on the same input return the same bits).  Everything else takes the
    host formulation: a plain forward / explicit backward in fp64 torch ops, MLP_HOST_CHUNK rows at a time
    (``native=False`` asks for it inside the range too: bench/mlp_micro.py times the two side by side).
    ``prepared``: a MlpPrepared of the same weights, so that repeated calls build the device tables once.
    """
    layers = [int(v) for v in layers]
    n = X.shape[0]
    C = layers[-1]
    dev = X.device
    if X.dim() != 2 or X.shape[1] != layers[0]:
        raise ValueError(f"mlp_step: X has {X.shape[1]} columns, layers[0] is {layers[0]}")
    if X.dtype not in (torch.float32, torch.float64):
        X = X.float()
    f32 = X.dtype == torch.float32
    prep = prepared if prepared is not None else MlpPrepared(theta32, layers)
    if prep.layers != layers:
        raise ValueError(f"mlp_step: prepared for layers {prep.layers}, called with {layers}")
    P = prep.theta.numel()
    plan, Xn = _mlp_native_plan(X, layers) if native else (None, X)
    if plan is not None:
        L = _lib.lib()
        lay = np.asarray(layers, dtype=np.int32)
        tab = prep.on(dev, True, True)
        out = ws = raw = prob = pred = yi = None
        if mode == MLP_STEP:
            yi = y.to(device=dev, dtype=torch.int32).contiguous()
            # every entry of out is written by the reduction, every workspace entry it reads by the step kernel
            out = torch.empty(P + 1, dtype=torch.float64, device=dev)
            ws = torch.empty(L.cdna_mlp_step_workspace(n, lay.ctypes.data, len(lay)), dtype=torch.float64, device=dev)
        else:
            raw = torch.empty((n, C), dtype=torch.float64, device=dev)
            prob = torch.empty((n, C), dtype=torch.float64, device=dev)
            pred = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(L.cdna_mlp_step(_ptr(Xn), n, Xn.stride(0), _ptr(yi), _ptr(tab), lay.ctypes.data, len(lay),
                                   int(mode), _ptr(out), _ptr(ws), _ptr(raw), _ptr(prob), _ptr(pred), _stream(dev)),
                   "cdna_mlp_step")
        return (out[P], out[:P]) if mode == MLP_STEP else (raw, prob, pred)
    # host formulation, MLP_HOST_CHUNK rows at a time
    Wb = prep.on(dev, f32, False)
    nl = len(Wb)
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    gW = [torch.zeros_like(W) for W, _ in Wb]
    gb = [torch.zeros_like(b) for _, b in Wb]
    raws, probs, preds = [], [], []
    yl = None if y is None else y.to(device=dev, dtype=torch.int64)
    for i0 in range(0, n, MLP_HOST_CHUNK):
        acts = [X[i0:i0 + MLP_HOST_CHUNK].double()]
        for l, (W, b) in enumerate(Wb):
            Z = acts[-1] @ W.T + b
            acts.append(torch.sigmoid(Z) if l < nl - 1 else Z)
        Z = acts[-1]
        lse = torch.logsumexp(Z, 1)
        Pm = torch.exp(Z - lse[:, None])
        if mode == MLP_PREDICT:
            raws.append(Z)
            probs.append(Pm)
            preds.append(_first_argmax(Z))
            continue
        yc = yl[i0:i0 + MLP_HOST_CHUNK]
        loss += (lse - Z.gather(1, yc[:, None])[:, 0]).sum()
        D = Pm
        D.scatter_add_(1, yc[:, None], torch.full((yc.shape[0], 1), -1.0, dtype=torch.float64, device=dev))
        for l in range(nl - 1, -1, -1):
            gW[l] += D.T @ acts[l]
            gb[l] += D.sum(0)
            if l > 0:
                D = (D @ Wb[l][0]) * (acts[l] * (1.0 - acts[l]))
    if mode == MLP_PREDICT:
        if not raws:
            z = torch.zeros((0, C), dtype=torch.float64, device=dev)
            return z, z.clone(), torch.zeros(0, dtype=torch.int32, device=dev)
        return torch.cat(raws), torch.cat(probs), torch.cat(preds)
    return loss, torch.cat([t for W, b in zip(gW, gb) for t in (W.T.reshape(-1), b)])


# ------------------------------------------------------------ K25 fm_step (fm.hip)
FM_STEP, FM_PREDICT = 0, 1
FM_SQUARED, FM_LOGISTIC = 0, 1
FM_MAX_D = 128             # the fused kernel's range: d <= 128 and factorSize <= 32
FM_MAX_K = 32
FM_STREAM = 25             # Philox stream of the miniBatchFraction row selection
FM_HOST_CHUNK = 1 << 18    # rows per pass of the host formulation


def fm_num_params(d: int, k: int, fit_linear: bool = True, fit_intercept: bool = True) -> int:
    return d * k + (d if fit_linear else 0) + (1 if fit_intercept else 0)


def fm_unpack(theta, d: int, k: int, fit_linear: bool = True, fit_intercept: bool = True):
    """(V [d, k], w [d], b) from Spark's flat vector: the factors row-major (entry (i, f) at i * k + f), then the d
    linear weights if ``fit_linear``, then the intercept if ``fit_intercept`` (zeros for what is not fitted)."""
    V = theta[:d * k].reshape(d, k)
    w = theta[d * k:d * k + d] if fit_linear else theta.new_zeros(d)
    b = theta[-1] if fit_intercept else theta.new_zeros(())
    return V, w, b


class FmPrepared:
    """The parameters of one factorization machine as ``fm_step`` consumes them, prepared once per (device, row
    dtype, path) and reused by every call that is given this object."""

    def __init__(self, theta, d: int, k: int, fit_linear: bool = True, fit_intercept: bool = True):
        self.shape = (int(d), int(k), bool(fit_linear), bool(fit_intercept))
        self.theta = torch.as_tensor(theta, dtype=torch.float64).reshape(-1).cpu()
        if self.theta.numel() != fm_num_params(*self.shape):
            raise ValueError(f"fm_step: {self.theta.numel()} parameters for d = {d}, factorSize = {k}, fitLinear = "
                             f"{fit_linear}, fitIntercept = {fit_intercept}, expected {fm_num_params(*self.shape)}")
        self._made = {}

    def on(self, dev, f32: bool, native: bool):
        """(V, w, b) fp64 on ``dev`` (the parameters rounded to fp32 first for fp32 rows); for the native path the
        kernel's operands instead: the zero-padded fp32 table [d up to 2][(k + 1) up to 32] whose row i is v_i, then
        w_i with linear weights; u [128] fp64 with u_i = sum_f v_if^2; and the intercept."""
        key = (str(dev), f32, native)
        if key not in self._made:
            d, k, lin, icpt = self.shape
            th = self.theta.float().double() if f32 else self.theta
            V, w, b = fm_unpack(th, d, k, lin, icpt)
            if native:
                plan = np.zeros(10, dtype=np.int64)
                _lib.check(_lib.lib().cdna_fm_plan(None, 1, d, d, k, int(lin), plan.ctypes.data), "cdna_fm_plan")
                ldw = int(plan[8])
                tab = np.zeros((int(plan[7]) // ldw, ldw), dtype=np.float32)
                tab[:d, :k] = V.numpy()
                if lin:
                    tab[:d, k] = w.numpy()
                u = np.zeros(FM_MAX_D)
                u[:d] = (V.numpy() ** 2).sum(1)
                tab_d, u_d = upload(dev, tab.reshape(-1), u)
                self._made[key] = (tab_d, u_d, float(b))
            else:
                self._made[key] = (V.to(dev).contiguous(), w.to(dev), b.to(dev))
        return self._made[key]


def _fm_native_plan(X: torch.Tensor, k: int, fit_linear: bool):
    return _row_plan(X, "cdna_fm_plan", 10, X.shape[-1], int(k), int(fit_linear))


def fm_plan(X: torch.Tensor, k: int, fit_linear: bool = True) -> Dict[str, object]:
    """What :func:`fm_step` runs for these operands, from the dispatch's own host function (nothing is launched):
    ``path`` "native" or "host"; for the native path ``slots`` (gradient tiles per wave of the STEP instantiation: 1
    or 2), ``vw`` (4: float4 row loads, 1: scalar loads), ``nblk``, ``rows_per_block``, ``tiles`` (32 x 32 gradient
    tiles), ``lds`` (bytes per block) and ``fold_rows`` (rows a block accumulates in fp32 between folds into its
    fp64 slab)."""
    out, _ = _fm_native_plan(X, k, fit_linear)
    if out is None:
        return {"path": "host"}
    return {"path": "native", "slots": int(out[1]), "vw": int(out[2]), "nblk": int(out[3]),
            "rows_per_block": int(out[4]), "tiles": int(out[5]), "lds": int(out[6]), "fold_rows": int(out[9])}


def fm_step(X: torch.Tensor, y: Optional[torch.Tensor], theta, k: int, loss: int = FM_SQUARED, mode: int = FM_STEP,
            fit_linear: bool = True, fit_intercept: bool = True, sample=None, native: bool = True,
            prepared: Optional[FmPrepared] = None):
    """Loss and gradient sums, or the raw predictions, of a factorization machine over the local rows.

    X [n, d] fp32 or fp64, y [n] (STEP only; 0 / 1 for the logistic loss), ``theta`` the flat parameter vector in
    Spark's layout (see ``fm_unpack``), ``k`` the factor size.  Per row s_f = sum_i v_if x_i and
    raw = b + w.x + 1/2 sum_f (s_f^2 - sum_i v_if^2 x_i^2).  FM_SQUARED: loss (raw - y)^2, m = 2 (raw - y).
    FM_LOGISTIC: loss log1p(exp(-raw)) for y > 0 and log1p(exp(raw)) otherwise, m = sigmoid(raw) - y.  The gradient
    is db = m, dw_i = m x_i, dv_if = m (s_f x_i - v_if x_i^2) (Spark's MSE / LogisticFactorizationMachinesGradient).

    FM_STEP returns (loss_sum fp64 scalar, grad_sum fp64 [P], count fp64 scalar): un-normalised sums over the
    selected rows and their number.  ``sample = (seed, row_offset, frac)`` selects row r when
    ``uniform(seed, row_offset + r, FM_STREAM) < frac`` (the Philox of :func:`uniform`, keyed by the global row id,
    so the selection does not depend on how the rows are sharded); ``frac >= 1`` or ``sample=None`` selects every row
    without a draw.  FM_PREDICT returns raw [n] fp64.

    For fp32 X the op is defined at the parameters rounded to fp32, on the device and in the host formulation alike;
    fp64 X uses them as they are.  fp32 X on a GPU with d <= FM_MAX_D and k <= FM_MAX_K (any n >= 1, row stride and
    alignment) runs the K25 kernel: X [V | w] and the gradient X^T (m s | m) on the exact-fp32 MFMA, the rest of raw,
    the loss term and m in fp64, the selection drawn in the kernel, per-block partial sums reduced in a fixed order
    (two calls on the same input return the same bits).  Everything else takes the host formulation: plain fp64
    torch ops, FM_HOST_CHUNK rows at a time, the mask from :func:`uniform` (``native=False`` asks for it inside the
    range too: bench/fm_micro.py times the two side by side).  ``prepared``: a FmPrepared of the same parameters, so
    that repeated calls build the device tables once.
    """
    if X.dim() != 2:
        raise ValueError("fm_step: X must be [n, d]")
    n, d = X.shape
    k = int(k)
    dev = X.device
    if loss not in (FM_SQUARED, FM_LOGISTIC) or mode not in (FM_STEP, FM_PREDICT):
        raise ValueError(f"fm_step: loss {loss} / mode {mode}")
    if X.dtype not in (torch.float32, torch.float64):
        X = X.float()
    f32 = X.dtype == torch.float32
    shape = (int(d), k, bool(fit_linear), bool(fit_intercept))
    prep = prepared if prepared is not None else FmPrepared(theta, *shape)
    if prep.shape != shape:
        raise ValueError(f"fm_step: prepared for {prep.shape}, called with {shape}")
    P = prep.theta.numel()
    seed, row_offset, frac = sample if sample is not None else (0, 0, 1.0)
    draw = mode == FM_STEP and float(frac) < 1.0
    plan, Xn = _fm_native_plan(X, k, fit_linear) if native else (None, X)
    if plan is not None:
        L = _lib.lib()
        tab, u, b0 = prep.on(dev, True, True)
        out = ws = raw = yd = None
        if mode == FM_STEP:
            yd = y.to(device=dev, dtype=torch.float64).contiguous()
            # every entry of out is written by the reduction, every workspace entry it reads by the step kernel
            out = torch.empty(P + 2, dtype=torch.float64, device=dev)
            ws = torch.empty(L.cdna_fm_step_workspace(n, d, k, int(fit_linear)), dtype=torch.float64, device=dev)
        else:
            raw = torch.empty(n, dtype=torch.float64, device=dev)
        _lib.check(L.cdna_fm_step(_ptr(Xn), n, Xn.stride(0), _ptr(yd), _ptr(tab), _ptr(u), b0, d, k, int(fit_linear),
                                  int(fit_intercept), int(loss), int(mode), int(draw),
                                  int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_offset), float(frac), FM_STREAM, _ptr(out),
                                  _ptr(ws), _ptr(raw), _stream(dev)), "cdna_fm_step")
        return (out[P], out[:P], out[P + 1]) if mode == FM_STEP else raw
    # host formulation, FM_HOST_CHUNK rows at a time
    V, w, b = prep.on(dev, f32, False)
    V2 = V * V
    lsum = torch.zeros((), dtype=torch.float64, device=dev)
    cnt = torch.zeros((), dtype=torch.float64, device=dev)
    gV, gw, gb = torch.zeros_like(V), torch.zeros_like(w), torch.zeros_like(b)
    raws = []
    yl = None if y is None else y.to(device=dev, dtype=torch.float64)
    for i0 in range(0, n, FM_HOST_CHUNK):
        Xc = X[i0:i0 + FM_HOST_CHUNK].double()
        X2 = Xc * Xc
        S = Xc @ V
        r = b + Xc @ w + 0.5 * ((S * S).sum(1) - (X2 @ V2).sum(1))
        if mode == FM_PREDICT:
            raws.append(r)
            continue
        yc = yl[i0:i0 + FM_HOST_CHUNK]
        if loss == FM_SQUARED:
            l, m = (r - yc) ** 2, 2.0 * (r - yc)
        else:
            z = torch.where(yc > 0, -r, r)
            l = z.clamp_min(0.0) + torch.log1p(torch.exp(-z.abs()))
            m = torch.sigmoid(r) - yc
        if draw:
            sel = uniform(Xc.shape[0], seed, int(row_offset) + i0, FM_STREAM, device=dev) < float(frac)
            l, m = torch.where(sel, l, torch.zeros_like(l)), torch.where(sel, m, torch.zeros_like(m))
            cnt += sel.sum()
        else:
            cnt += Xc.shape[0]
        lsum += l.sum()
        gb += m.sum()
        gw += Xc.T @ m
        gV += Xc.T @ (S * m[:, None]) - V * (X2.T @ m)[:, None]
    if mode == FM_PREDICT:
        return torch.cat(raws) if raws else torch.zeros(0, dtype=torch.float64, device=dev)
    parts = [gV.reshape(-1)] + ([gw] if fit_linear else []) + ([gb.reshape(1)] if fit_intercept else [])
    return lsum, torch.cat(parts), cnt


# ------------------------------------------------------------ K26 aft_step (aft.hip)
AFT_STEP, AFT_PREDICT = 0, 1
AFT_MAX_D = 128            # the fused kernel's range: fp32 rows with d <= 128
AFT_MAX_Q = 16             # quantiles written by the PREDICT pass itself; more take one outer product on top
AFT_HOST_CHUNK = 1 << 18   # rows per pass of the host formulation


def aft_quantile_factors(probs, log_sigma: float) -> np.ndarray:
    """exp(sigma log(-log(1 - p))) per quantile probability: the Weibull quantile over the prediction."""
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    return np.exp(math.exp(float(log_sigma)) * np.log(-np.log1p(-p)))


def _aft_native_plan(X: torch.Tensor):
    return _row_plan(X, "cdna_aft_plan", 6, X.shape[-1])


def aft_plan(X: torch.Tensor) -> Dict[str, object]:
    """What :func:`aft_step` runs for these operands, from the dispatch's own host function (nothing is launched):
    ``path`` "native" or "host"; for the native path ``vw`` (4: float4 row loads, 1: scalar loads), ``nblk``,
    ``rows_per_block``, ``lds`` (bytes per block) and ``slot`` (workspace doubles per block)."""
    out, _ = _aft_native_plan(X)
    if out is None:
        return {"path": "host"}
    return {"path": "native", "vw": int(out[1]), "nblk": int(out[2]), "rows_per_block": int(out[3]),
            "lds": int(out[4]), "slot": int(out[5])}


def aft_step(X: torch.Tensor, logt: Optional[torch.Tensor], censor: Optional[torch.Tensor], coef, intercept: float,
             log_sigma: float, mode: int = AFT_STEP, probs=None, native: bool = True):
    """Loss and gradient sums, or the predictions and quantiles, of Spark's AFTSurvivalRegression (a Weibull
    accelerated failure time model) over the local rows.

    X [n, d] fp32 or fp64, ``logt`` [n] the log of the survival times, ``censor`` [n] (1: the event occurred, 0:
    censored), ``coef`` [d] fp64 for the rows as they are, sigma = exp(``log_sigma``).  Per row
    eps = (log t - x.coef - intercept) / sigma, the loss term is delta log sigma - delta eps + e^eps,
    m = (delta - e^eps) / sigma, and the gradient terms are m x (coef), m (intercept) and
    delta + (delta - e^eps) eps (log sigma).

    AFT_STEP returns (loss_sum fp64 scalar, grad_sums fp64 [d + 2] = [coef | intercept | log sigma], bad fp64
    scalar): un-normalised sums, and the number of bad rows.  A row is bad when it has a non-finite feature or
    log t (t <= 0 or NaN), a censor that is neither 0 nor 1, or a loss, m or log-sigma term that is not finite
    (e^eps overflowed); a bad row adds exactly nothing to the other sums.  AFT_PREDICT returns exp(x.coef +
    intercept) [n] fp64, and with ``probs`` also the quantiles [n, Q] = prediction * exp(sigma log(-log(1 - p))).

    fp32 X on a GPU with d <= AFT_MAX_D (any n >= 1, row stride and alignment) runs the K26 kernel: one pass, all
    arithmetic in fp64, per-block partial sums reduced in a fixed order (two calls on the same input return the same
    bits); up to AFT_MAX_Q quantiles are written by the same pass.  Everything else takes the host formulation: plain
    fp64 torch ops, AFT_HOST_CHUNK rows at a time (``native=False`` asks for it inside the range too:
    bench/aft_micro.py times the two side by side).
    """
    if X.dim() != 2:
        raise ValueError("aft_step: X must be [n, d]")
    if mode not in (AFT_STEP, AFT_PREDICT):
        raise ValueError(f"aft_step: mode {mode}")
    n, d = X.shape
    dev = X.device
    if X.dtype not in (torch.float32, torch.float64):
        X = X.float()
    cf = np.asarray(coef.detach().cpu().numpy() if isinstance(coef, torch.Tensor) else coef,
                    dtype=np.float64).reshape(-1)
    if cf.shape[0] != d:
        raise ValueError(f"aft_step: {cf.shape[0]} coefficients for d = {d}")
    b0, ls = float(intercept), float(log_sigma)
    sigma = math.exp(ls)
    qf = None if probs is None or mode != AFT_PREDICT else aft_quantile_factors(probs, ls)
    Q = 0 if qf is None else int(qf.shape[0])
    if mode == AFT_STEP:
        logt = logt.to(device=dev, dtype=torch.float64).contiguous()
        censor = censor.to(device=dev, dtype=torch.float64).contiguous()
        if logt.shape != (n,) or censor.shape != (n,):
            raise ValueError("aft_step: logt and censor must be [n]")
    plan, Xn = _aft_native_plan(X) if native else (None, X)
    if plan is not None:
        L = _lib.lib()
        inner = qf is not None and 0 < Q <= AFT_MAX_Q
        if inner:
            cf_d, qf_d = upload(dev, cf, qf)
        else:
            cf_d, qf_d = upload(dev, cf)[0], None
        out = ws = pred = quant = None
        if mode == AFT_STEP:
            # every entry of out is written by the reduction, every workspace entry it reads by the step kernel
            out = torch.empty(d + 4, dtype=torch.float64, device=dev)
            ws = torch.empty(L.cdna_aft_step_workspace(n, d), dtype=torch.float64, device=dev)
        else:
            pred = torch.empty(n, dtype=torch.float64, device=dev)
            quant = torch.empty((n, Q), dtype=torch.float64, device=dev) if inner else None
        _lib.check(L.cdna_aft_step(_ptr(Xn), n, Xn.stride(0), _ptr(logt), _ptr(censor), _ptr(cf_d), b0, sigma, ls, d,
                                   int(mode), Q if inner else 0, _ptr(qf_d), _ptr(out), _ptr(ws), _ptr(pred),
                                   _ptr(quant), _stream(dev)), "cdna_aft_step")
        if mode == AFT_STEP:
            return out[d + 2], out[:d + 2], out[d + 3]
        if qf is None:
            return pred
        return pred, (quant if inner else torch.outer(pred, upload(dev, qf)[0]))
    # host formulation, AFT_HOST_CHUNK rows at a time
    cf_t = torch.from_numpy(cf).to(dev)
    acc = torch.zeros(d + 4, dtype=torch.float64, device=dev)
    preds = []
    for i0 in range(0, n, AFT_HOST_CHUNK):
        Xc = X[i0:i0 + AFT_HOST_CHUNK].double()
        dot = Xc @ cf_t
        if mode == AFT_PREDICT:
            preds.append(torch.exp(dot + b0))
            continue
        lt, dl = logt[i0:i0 + AFT_HOST_CHUNK], censor[i0:i0 + AFT_HOST_CHUNK]
        eps = (lt - dot - b0) / sigma
        ee = torch.exp(eps)
        loss = dl * ls - dl * eps + ee
        mm = (dl - ee) / sigma
        ss = dl + (dl - ee) * eps
        ok = torch.isfinite(Xc).all(1) & torch.isfinite(lt) & ((dl == 0) | (dl == 1)) & torch.isfinite(loss) & \
            torch.isfinite(mm) & torch.isfinite(ss)
        zero = torch.zeros_like(loss)
        mm = torch.where(ok, mm, zero)
        acc[:d] += torch.where(ok[:, None], Xc, zero[:, None]).T @ mm      # predicated: never a NaN times zero
        acc[d] += mm.sum()
        acc[d + 1] += torch.where(ok, ss, zero).sum()
        acc[d + 2] += torch.where(ok, loss, zero).sum()
        acc[d + 3] += (~ok).sum()
    if mode == AFT_STEP:
        return acc[d + 2], acc[:d + 2], acc[d + 3]
    pred = torch.cat(preds) if preds else torch.zeros(0, dtype=torch.float64, device=dev)
    if qf is None:
        return pred
    return pred, torch.outer(pred, torch.from_numpy(qf).to(dev))


# ------------------------------------------------------------ K27 label_stats (select.hip)
LABEL_COUNT, LABEL_CLASS, LABEL_REGRESS = 0, 1, 2
LABEL_MAX_D = 128              # the fused kernel's range: fp32 rows with d <= 128
LABEL_MAX_C = 32               # CLASS: classes of the kernel's LDS table
LABEL_HOST_CHUNK = 1 << 18     # rows per pass of the host formulation


def _label_native_plan(X: torch.Tensor, mode: int, C: int, K: int):
    return _row_plan(X, "cdna_label_stats_plan", 8, X.shape[-1], int(mode), min(int(C), 1 << 30),
                     min(int(K), 1 << 30))


def label_stats_plan(X: torch.Tensor, mode: int, C: int = 1, K: int = 1) -> Dict[str, object]:
    """What :func:`label_stats` runs for these operands, from the dispatch's own host function (nothing is
    launched): ``path`` "native" or "host"; for the native path ``vw`` (4: float4 row loads, 1: scalar loads),
    ``nblk``, ``rows_per_block``, ``lds`` (bytes per block), ``slot`` (workspace doubles per block),
    ``count_budget`` (the LDS bytes a COUNT table may take) and ``blocks_per_cu`` (by LDS)."""
    out, _ = _label_native_plan(X, mode, C, K)
    if out is None:
        return {"path": "host"}
    return {"path": "native", "vw": int(out[1]), "nblk": int(out[2]), "rows_per_block": int(out[3]),
            "lds": int(out[4]), "slot": int(out[5]), "count_budget": int(out[6]), "blocks_per_cu": int(out[7])}


def label_stats(X: torch.Tensor, label: torch.Tensor, mode: int, C: int = 1, K: int = 1, shift=None,
                yshift: float = 0.0, native: bool = True) -> Dict[str, torch.Tensor]:
    """The per-feature statistics of X [n, d] against a label that the univariate tests need, over the local rows.

    LABEL_COUNT (chi-square): ``label`` holds codes in 0 .. C-1; returns ``table`` int64 [d, K, C], the exact
    counts of the cells (feature, int(x), code).  A cell is bad when x is non-finite, not integer-valued, < 0
    or >= K.
    LABEL_CLASS (ANOVA): codes in 0 .. C-1 and ``shift`` [d] fp64; returns ``sums`` [C, d] = sum (x - shift) per
    (class, feature), ``sq`` [d] = sum (x - shift)^2 and ``n`` [C], the rows per class, all fp64 and formed from
    (double)x - shift.  A cell is bad when x is non-finite.
    LABEL_REGRESS (F-value): ``label`` is y fp64, with ``shift`` and ``yshift``; returns ``sx``, ``sxx``, ``sxy``
    [d] = sum (x - shift), its square and (x - shift)(y - yshift), and ``sy``, ``syy``, ``n``: sum (y - yshift), its
    square and the number of rows.  A cell is bad when x is non-finite.
    Every mode returns ``bad`` [d], the bad cells per feature -- a bad cell adds nothing to its feature's
    statistics -- and ``bad_label``: the rows whose label is bad (a code outside 0 .. C-1, a non-finite y), which are
    never accumulated.  The counts are int64 in LABEL_COUNT and fp64 (exact) in the other modes.

    fp32 X on a GPU with d <= LABEL_MAX_D (any n >= 1, row stride and alignment) runs the K27 kernel: one pass;
    LABEL_CLASS with 2 <= C <= LABEL_MAX_C, LABEL_COUNT while the block's table of K C cells per feature fits the
    kernel's LDS budget (:func:`label_stats_plan` reports it).  Sums are fp64 per-block partials reduced in a
    fixed order and the counts go through integer atomics: two calls on the same input return the same bits.
    Everything else takes the host formulation: plain fp64 torch ops, LABEL_HOST_CHUNK rows at a time
    (``native=False`` asks for it inside the range too: bench/select_micro.py times the two side by side).
    """
    if X.dim() != 2:
        raise ValueError("label_stats: X must be [n, d]")
    if mode not in (LABEL_COUNT, LABEL_CLASS, LABEL_REGRESS):
        raise ValueError(f"label_stats: mode {mode}")
    n, d = X.shape
    dev = X.device
    if X.dtype not in (torch.float32, torch.float64):
        X = X.float()
    C, K = (1, 1) if mode == LABEL_REGRESS else (int(C), int(K) if mode == LABEL_COUNT else 1)
    if C < 1 or K < 1:
        raise ValueError(f"label_stats: C = {C}, K = {K}")
    if label.shape != (n,):
        raise ValueError("label_stats: the label must be [n]")
    if mode == LABEL_REGRESS:
        label = label.to(device=dev, dtype=torch.float64).contiguous()
    else:
        label = label.to(device=dev, dtype=torch.int32).contiguous()
    sh = None
    if mode != LABEL_COUNT:
        sh = np.zeros(d) if shift is None else np.asarray(
            shift.detach().cpu().numpy() if isinstance(shift, torch.Tensor) else shift, dtype=np.float64).reshape(-1)
        if sh.shape[0] != d:
            raise ValueError(f"label_stats: {sh.shape[0]} shifts for d = {d}")
    ys = float(yshift)
    plan, Xn = _label_native_plan(X, mode, C, K) if native else (None, X)
    if plan is not None:
        L = _lib.lib()
        if mode == LABEL_COUNT:
            # cleared by the call itself
            out = torch.empty(d * K * C + d + 1, dtype=torch.int64, device=dev)
            _lib.check(L.cdna_label_stats(_ptr(Xn), n, Xn.stride(0), _ptr(label), None, None, 0.0, d, int(mode), C, K,
                                          _ptr(out), None, _stream(dev)), "cdna_label_stats")
            return {"table": out[:d * K * C].view(d, K, C), "bad": out[d * K * C:d * K * C + d],
                    "bad_label": out[d * K * C + d]}
        sh_d = upload(dev, sh)[0]
        slot = int(plan[5])
        # every entry of out is written by the reduction, every workspace entry it reads by the pass
        out = torch.empty(slot, dtype=torch.float64, device=dev)
        ws = torch.empty(L.cdna_label_stats_workspace(n, d, int(mode), C, K), dtype=torch.float64, device=dev)
        is_y = mode == LABEL_REGRESS
        _lib.check(L.cdna_label_stats(_ptr(Xn), n, Xn.stride(0), None if is_y else _ptr(label),
                                      _ptr(label) if is_y else None, _ptr(sh_d), ys, d, int(mode), C, K, _ptr(out),
                                      _ptr(ws), _stream(dev)), "cdna_label_stats")
        D = LABEL_MAX_D
        if mode == LABEL_CLASS:
            return {"sums": out[:C * D].view(C, D)[:, :d], "sq": out[C * D:C * D + d],
                    "bad": out[C * D + D:C * D + D + d], "n": out[C * D + 2 * D:C * D + 2 * D + C],
                    "bad_label": out[C * D + 2 * D + C]}
        return {"sx": out[:d], "sxx": out[D:D + d], "sxy": out[2 * D:2 * D + d], "bad": out[3 * D:3 * D + d],
                "sy": out[4 * D], "syy": out[4 * D + 1], "n": out[4 * D + 2], "bad_label": out[4 * D + 3]}
    # host formulation, LABEL_HOST_CHUNK rows at a time
    f64 = dict(dtype=torch.float64, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    if mode == LABEL_COUNT:
        table = torch.zeros(d * K * C, **i64)
        bad, bad_label = torch.zeros(d, **i64), torch.zeros((), **i64)
        cols = torch.arange(d, device=dev)[None, :]
        for i0 in range(0, n, LABEL_HOST_CHUNK):
            Xc = X[i0:i0 + LABEL_HOST_CHUNK].double()
            yl = label[i0:i0 + LABEL_HOST_CHUNK].long()
            ok = (yl >= 0) & (yl < C)
            good = torch.isfinite(Xc) & (Xc >= 0) & (Xc < K) & (Xc == torch.floor(Xc)) & ok[:, None]
            k = torch.where(good, Xc, torch.zeros_like(Xc)).long()
            idx = (cols * K + k) * C + torch.where(ok, yl, torch.zeros_like(yl))[:, None]
            table += torch.bincount(idx[good], minlength=d * K * C)
            bad += (~good & ok[:, None]).sum(0)
            bad_label += (~ok).sum()
        return {"table": table.view(d, K, C), "bad": bad, "bad_label": bad_label}
    sh_t = torch.from_numpy(sh).to(dev)
    bad, bad_label = torch.zeros(d, **f64), torch.zeros((), **f64)
    if mode == LABEL_CLASS:
        sums, sq, cnt = torch.zeros((C, d), **f64), torch.zeros(d, **f64), torch.zeros(C, **f64)
        for i0 in range(0, n, LABEL_HOST_CHUNK):
            Xc = X[i0:i0 + LABEL_HOST_CHUNK].double()
            yl = label[i0:i0 + LABEL_HOST_CHUNK].long()
            ok = (yl >= 0) & (yl < C)
            yz = torch.where(ok, yl, torch.zeros_like(yl))
            fin = torch.isfinite(Xc)
            V = torch.where(fin & ok[:, None], Xc - sh_t, torch.zeros_like(Xc))   # predicated: never a NaN times zero
            if C <= 64:    # a one-hot product: index_add_'s fp64 atomics on a few rows serialise on a GPU
                sums += torch.nn.functional.one_hot(yz, C).double().T @ V
            else:
                sums.index_add_(0, yz, V)
            sq += (V * V).sum(0)
            cnt += torch.bincount(yl[ok], minlength=C).double()
            bad += (~fin & ok[:, None]).sum(0)
            bad_label += (~ok).sum()
        return {"sums": sums, "sq": sq, "n": cnt, "bad": bad, "bad_label": bad_label}
    sx, sxx, sxy = torch.zeros(d, **f64), torch.zeros(d, **f64), torch.zeros(d, **f64)
    sy, syy, cnt = torch.zeros((), **f64), torch.zeros((), **f64), torch.zeros((), **f64)
    for i0 in range(0, n, LABEL_HOST_CHUNK):
        Xc = X[i0:i0 + LABEL_HOST_CHUNK].double()
        yc = label[i0:i0 + LABEL_HOST_CHUNK]
        ok = torch.isfinite(yc)
        yy = torch.where(ok, yc - ys, torch.zeros_like(yc))
        fin = torch.isfinite(Xc)
        V = torch.where(fin & ok[:, None], Xc - sh_t, torch.zeros_like(Xc))
        sx += V.sum(0)
        sxx += (V * V).sum(0)
        sxy += V.T @ yy
        sy += yy.sum()
        syy += (yy * yy).sum()
        cnt += ok.sum()
        bad += (~fin & ok[:, None]).sum(0)
        bad_label += (~ok).sum()
    return {"sx": sx, "sxx": sxx, "sxy": sxy, "sy": sy, "syy": syy, "n": cnt, "bad": bad, "bad_label": bad_label}


# ------------------------------------------------------------ K28 col_digit_hist / col_select (quantile_select.hip)
COLQ_MAX_D = 128               # the kernel's range: fp32 rows with d <= 128 and at most COLQ_MAX_Q targets
COLQ_MAX_Q = 8
COLQ_MAX_BITS = 8              # the widest digit of a pass
COLQ_BUDGET = 96 * 1024        # LDS bytes of a block's digit table
_I64_MIN = -(1 << 63)


def col_quantile_widths(d: int, Q: int) -> list:
    """The digit widths of the passes of a native quantile call for Q targets over d columns: a pure-Python mirror
    of the kernel's plan function, which is the source of the widths wherever the library loads
    (:func:`col_quantiles_plan`).  B(Q') is the widest b <= 8 with Q' 2^b (d | 1) 4 <= COLQ_BUDGET; pass 0 takes B(1)
    bits and every later pass min(B(Q), bits left)."""
    def B(q):
        b = COLQ_MAX_BITS
        while b > 0 and (q << b) * (d | 1) * 4 > COLQ_BUDGET:
            b -= 1
        return b
    widths, left = [B(1)], 32 - B(1)
    while left > 0:
        widths.append(min(B(Q), left))
        left -= widths[-1]
    return widths


def _colq_native_plan(X: torch.Tensor, Q: int):
    return _row_plan(X, "cdna_col_quantiles_plan", 40, X.shape[-1], min(int(Q), 1 << 30))


def col_quantiles_plan(X: torch.Tensor, Q: int) -> Dict[str, object]:
    """What :func:`col_quantiles` runs for X and Q probabilities, from the dispatch's own host function (nothing is
    launched): ``path`` "native" or "host" and ``widths``, the digit widths of the passes; for the native path
    ``vw`` (4: float4 row loads, 1: scalar loads), ``nblk``, ``rows_per_block``, ``lds`` (bytes per block at the
    widest pass) and ``max_bits`` = (B(1), B(Q)), the widest digit of a FIRST and of a NEXT pass."""
    out, _ = _colq_native_plan(X, Q)
    if out is None:
        return {"path": "host", "widths": [8] * (8 if X.dtype == torch.float64 else 4)}
    return {"path": "native", "vw": int(out[1]), "nblk": int(out[2]), "rows_per_block": int(out[3]),
            "lds": int(out[4]), "max_bits": (int(out[5]), int(out[6])),
            "widths": [int(v) for v in out[8:8 + int(out[7])]]}


def _colq_keys(X: torch.Tensor):
    """(keys int64, not NaN) of fp32 / fp64 values.  The keys' signed order is numeric order (-0.0 just below +0.0,
    +-inf at the ends): the unsigned 32-bit key u ^ (sign ? 0xFFFFFFFF : 0x80000000) of an fp32 value, held in
    int64; for fp64 the int64 bits with the magnitude bits of negative values flipped."""
    ok = ~torch.isnan(X)
    if X.dtype == torch.float32:
        u = X.contiguous().view(torch.int32).long() & 0xFFFFFFFF
        return u ^ torch.where(u >> 31 != 0, 0xFFFFFFFF, 0x80000000), ok
    b = X.contiguous().view(torch.int64)
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF), ok


def _colq_values(keys: torch.Tensor, dtype) -> torch.Tensor:
    """The values of keys (the inverse of :func:`_colq_keys`)."""
    if dtype == torch.float32:
        u = keys ^ torch.where(keys >> 31 != 0, 0x80000000, 0xFFFFFFFF)
        return torch.where(u >> 31 != 0, u - (1 << 32), u).to(torch.int32).view(torch.float32)
    return (keys ^ ((keys >> 63) & 0x7FFFFFFFFFFFFFFF)).view(torch.float64)


def _colq_pattern(keys: torch.Tensor, kb: int) -> torch.Tensor:
    """The keys as kb-bit unsigned patterns whose digits the passes take (in int64; kb = 64: the sign bit flipped)."""
    return keys if kb == 32 else keys ^ _I64_MIN


def _colq_extrema(kmin: torch.Tensor, kmax: torch.Tensor, dtype):
    """(min, max) values of the columns' extreme keys; NaN for a column without a value (kmin > kmax)."""
    nan = torch.full(kmin.shape, float("nan"), dtype=dtype, device=kmin.device)
    none = kmin > kmax
    return torch.where(none, nan, _colq_values(kmin, dtype)), torch.where(none, nan, _colq_values(kmax, dtype))


def _digit_hist_native(Xn: torch.Tensor, Q: int, bits: int, shift: int, prefix: Optional[torch.Tensor]):
    """One native pass of a call for Q targets; prefix: int32 [d, Q] holding the u32 prefixes, None: FIRST."""
    n, d = Xn.shape
    dev = Xn.device
    first = prefix is None
    cells = d * (1 if first else Q) << bits
    out = torch.empty(cells + (2 * d if first else 0), dtype=torch.int64, device=dev)   # cleared by the call itself
    _lib.check(_lib.lib().cdna_col_digit_hist(_ptr(Xn), n, Xn.stride(0), d, Q, bits, shift, _ptr(prefix), _ptr(out),
                                              _stream(dev)), "cdna_col_digit_hist")
    res = {"hist": out[:cells].view(d, 1 if first else Q, 1 << bits)}
    if first:
        km = out[cells + d:].view(torch.int32).long() & 0xFFFFFFFF
        res.update(nan=out[cells:cells + d], kmin=km[:d], kmax=km[d:])
    return res


def _digit_hist_host(X: torch.Tensor, bits: int, shift: int, prefix: Optional[torch.Tensor]):
    """One pass in plain torch ops, LABEL_HOST_CHUNK rows at a time; prefix: int64 [d, Q] patterns, None: FIRST."""
    n, d = X.shape
    dev = X.device
    kb = 64 if X.dtype == torch.float64 else 32
    first = prefix is None
    Q = 1 if first else prefix.shape[1]
    nd = 1 << bits
    i64 = dict(dtype=torch.int64, device=dev)
    hist = torch.zeros(d * Q * nd, **i64)
    nan = torch.zeros(d, **i64)
    kmin = torch.full((d,), (1 << (kb - 1)) - 1 if kb == 64 else (1 << 32) - 1, **i64)
    kmax = torch.full((d,), _I64_MIN if kb == 64 else 0, **i64)
    cols = torch.arange(d, device=dev)[None, :]
    for i0 in range(0, n, LABEL_HOST_CHUNK):
        keys, ok = _colq_keys(X[i0:i0 + LABEL_HOST_CHUNK])
        pat = _colq_pattern(keys, kb)
        digit = (pat >> shift) & (nd - 1)
        if first:
            hist += torch.bincount((cols * nd + digit)[ok], minlength=d * nd)
            nan += (~ok).sum(0)
            kmin = torch.minimum(kmin, torch.where(ok, keys, kmin[None, :]).amin(0))
            kmax = torch.maximum(kmax, torch.where(ok, keys, kmax[None, :]).amax(0))
            continue
        # shift + bits < kb here: the shift is never by the key's whole width
        hi = (pat >> (shift + bits)) & ((1 << (kb - shift - bits)) - 1)
        for t in range(Q):
            hit = ok & (hi == prefix[None, :, t])
            hist += torch.bincount(((cols * Q + t) * nd + digit)[hit], minlength=d * Q * nd)
    res = {"hist": hist.view(d, Q, nd)}
    if first:
        res.update(nan=nan, kmin=kmin, kmax=kmax)
    return res


def col_digit_hist(X: torch.Tensor, bits: int, shift: int, prefix: Optional[torch.Tensor] = None,
                   native: bool = True) -> Dict[str, torch.Tensor]:
    """One pass of the radix select over the local rows of X [n, d]: the counts of the key digit
    ``(key >> shift) & (2^bits - 1)`` per column.

    FIRST (``prefix`` None; ``shift + bits`` must be the key width, 32 for fp32 and 64 for fp64): every non-NaN
    value counts; returns ``hist`` int64 [d, 1, 2^bits], ``nan`` int64 [d] and ``kmin`` / ``kmax`` int64 [d], the
    columns' extreme keys (for fp32 2^32 - 1 / 0 for a column without a value).
    NEXT (``prefix`` integer [d, Q], ``shift + bits`` below the key width): a value counts for every target t with
    ``key >> (shift + bits) == prefix[c, t]``; returns ``hist`` int64 [d, Q, 2^bits].  Targets that share a prefix
    get identical counts.
    The key of an fp32 value is u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000), u its bits: unsigned key order is numeric
    order.  A NaN has no key.

    fp32 X on a GPU with d <= COLQ_MAX_D, Q <= COLQ_MAX_Q and ``bits`` within the plan's ``max_bits`` runs the K28
    kernel (LDS integer atomics, 64-bit integer atomics on the table: exact, the same bits on every call); n = 0
    launches nothing.  Everything else, and ``native=False``, takes the host formulation: the same counts from
    ``bincount``, LABEL_HOST_CHUNK rows at a time."""
    if X.dim() != 2:
        raise ValueError("col_digit_hist: X must be [n, d]")
    if X.dtype not in (torch.float32, torch.float64):
        X = X.float()
    d = X.shape[1]
    kb = 64 if X.dtype == torch.float64 else 32
    bits, shift = int(bits), int(shift)
    first = prefix is None
    if bits < 1 or bits > COLQ_MAX_BITS or shift < 0 or (shift + bits != kb if first else shift + bits >= kb):
        raise ValueError(f"col_digit_hist: bits = {bits}, shift = {shift} for {kb}-bit keys")
    if not first and (prefix.dim() != 2 or prefix.shape[0] != d or prefix.shape[1] < 1):
        raise ValueError("col_digit_hist: prefix must be [d, Q]")
    Q = 1 if first else prefix.shape[1]
    plan, Xn = _colq_native_plan(X, Q) if native else (None, X)
    if plan is not None and bits <= int(plan[5 if first else 6]):
        p32 = None
        if not first:   # the u32 prefixes in int32 storage
            p = prefix.to(device=X.device, dtype=torch.int64) & 0xFFFFFFFF
            p32 = torch.where(p >> 31 != 0, p - (1 << 32), p).to(torch.int32).contiguous()
        return _digit_hist_native(Xn, Q, bits, shift, p32)
    if not first:
        prefix = prefix.to(device=X.device, dtype=torch.int64)
        prefix = prefix & 0xFFFFFFFF if kb == 32 else prefix
    return _digit_hist_host(X, bits, shift, prefix)


def _colq_select(hist: torch.Tensor, rank: torch.Tensor, prefix: Optional[torch.Tensor], bits: int):
    """The select step of a pass in torch ops: hist int64 [d, Q', 2^bits], rank int64 [d, Q] -> (prefix, rank)."""
    cum = hist.cumsum(-1)
    lt = cum < rank[:, :, None]            # the digits before the rank's digit
    g = lt.sum(-1)
    below = (hist * lt).sum(-1)
    return (g if prefix is None else (prefix << bits) | g), rank - below


def _colq_probs(probs) -> np.ndarray:
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    if p.size < 1 or not bool(np.all((p >= 0) & (p <= 1))):
        raise ValueError(f"col_quantiles: probabilities must lie in [0, 1], got {probs}")
    return p


def _colq_reduce_first(st, comm):
    if comm is not None and comm.distributed:
        comm.all_reduce(st["hist"])
        comm.all_reduce(st["nan"])
        comm.all_reduce(st["kmin"], "min")
        comm.all_reduce(st["kmax"], "max")


def col_quantiles(X: torch.Tensor, probs, comm=None, native: bool = True) -> Dict[str, torch.Tensor]:
    """Exact quantiles of every column of X [n, d] over the rows of all ranks, by an MSB-first radix select.

    With m non-NaN values in a column, the quantile for probability q is the value of 1-based rank
    min(max(ceil(q m), 1), m) in key order (the product in fp64; -0.0 sorts just below +0.0, +-inf are ordinary
    values): q = 0 gives the minimum, q = 1 the maximum, m = 0 NaN.  NaN values are counted and otherwise ignored.
    Returns ``q`` [Q, d] in X's dtype, ``count`` and ``nan`` int64 [d] (the non-NaN and the NaN values) and ``min``
    / ``max`` [d] (NaN for a column without a value).

    Every pass is one :func:`col_digit_hist` over the local rows, an all-reduce of its int64 table when ``comm`` is
    distributed (pass 0 also reduces ``nan``, ``kmin`` and ``kmax``) and a select step that extends the targets'
    key prefixes by one digit: the result is exact, the same on every call and at every number of ranks, and no
    row leaves its rank.  fp32 X on a GPU with d <= COLQ_MAX_D and at most COLQ_MAX_Q probabilities runs the K28
    kernels with the widths of :func:`col_quantiles_plan`; prefixes and ranks stay on the device and a single-GPU
    call does not synchronise with the host.  Everything else (the CPU, fp64 rows with 64-bit keys, wider inputs,
    ``native=False``) takes the host formulation: the same algorithm in torch ops with 8-bit digits, the same bits.
    """
    if X.dim() != 2:
        raise ValueError("col_quantiles: X must be [n, d]")
    if X.dtype not in (torch.float32, torch.float64):
        X = X.float()
    p = _colq_probs(probs)
    n, d = X.shape
    Q = p.size
    dev = X.device
    plan, Xn = _colq_native_plan(X, Q) if native else (None, X)
    if plan is not None:
        L = _lib.lib()
        widths = [int(v) for v in plan[8:8 + int(plan[7])]]
        probs_d = upload(dev, p)[0]
        prefix = torch.empty((d, Q), dtype=torch.int32, device=dev)     # written by the first select
        rank = torch.empty((d, Q), dtype=torch.int64, device=dev)
        count = torch.empty(d, dtype=torch.int64, device=dev)
        q = torch.empty((Q, d), dtype=torch.float32, device=dev)
        shift = 32
        for i, b in enumerate(widths):
            shift -= b
            st = _digit_hist_native(Xn, Q, b, shift, None if i == 0 else prefix)
            if i == 0:
                first = st
                _colq_reduce_first(st, comm)
            elif comm is not None and comm.distributed:
                comm.all_reduce(st["hist"])
            _lib.check(L.cdna_col_select(_ptr(st["hist"]), d, Q, b, int(i == 0), int(shift == 0), _ptr(probs_d),
                                         _ptr(prefix), _ptr(rank), _ptr(count), _ptr(q), _stream(dev)),
                       "cdna_col_select")
        lo, hi = _colq_extrema(first["kmin"], first["kmax"], torch.float32)
        return {"q": q, "count": count, "nan": first["nan"], "min": lo, "max": hi}
    # host formulation
    kb = 64 if X.dtype == torch.float64 else 32
    first = _digit_hist_host(X, 8, kb - 8, None)
    _colq_reduce_first(first, comm)
    count = first["hist"].sum((1, 2))
    pt = torch.from_numpy(p).to(dev)
    rank = torch.ceil(pt[None, :] * count.double()[:, None]).long()
    rank = torch.minimum(rank.clamp_min(1), count[:, None])
    prefix, rank = _colq_select(first["hist"], rank, None, 8)
    for shift in range(kb - 16, -1, -8):
        hist = _digit_hist_host(X, 8, shift, prefix)["hist"]
        if comm is not None and comm.distributed:
            comm.all_reduce(hist)
        prefix, rank = _colq_select(hist, rank, prefix, 8)
    keys = prefix if kb == 32 else prefix ^ _I64_MIN
    vals = _colq_values(keys, X.dtype)
    nanv = torch.full_like(vals, float("nan"))
    lo, hi = _colq_extrema(first["kmin"], first["kmax"], X.dtype)
    return {"q": torch.where(count[:, None] > 0, vals, nanv).T.contiguous(), "count": count, "nan": first["nan"],
            "min": lo, "max": hi}


def col_extrema(X: torch.Tensor, comm=None) -> Dict[str, torch.Tensor]:
    """Pass 0 of :func:`col_quantiles` alone: ``min`` and ``max`` [d] of the non-NaN values of every column over
    the rows of all ranks (NaN for a column without one), ``count`` and ``nan`` int64 [d]."""
    if X.dim() != 2:
        raise ValueError("col_extrema: X must be [n, d]")
    if X.dtype not in (torch.float32, torch.float64):
        X = X.float()
    plan, Xn = _colq_native_plan(X, 1)
    if plan is not None:
        b = int(plan[5])
        st = _digit_hist_native(Xn, 1, b, 32 - b, None)
    else:
        kb = 64 if X.dtype == torch.float64 else 32
        st = _digit_hist_host(X, 8, kb - 8, None)
    _colq_reduce_first(st, comm)
    lo, hi = _colq_extrema(st["kmin"], st["kmax"], X.dtype)
    return {"min": lo, "max": hi, "count": st["hist"].sum((1, 2)), "nan": st["nan"]}


# ------------------------------------------------------------ segment mode (seg.hip)
SEG_HIST_CHUNK = 262144
# lane10 record chunks (levels 2-4 of the headline): at most this many records per block.  The records of a slot
# are in row order and the work list interleaves the slots by relative position, so smaller chunks keep the ~256
# concurrently running blocks on a narrower row window (each row line is gathered by ~6.3 slots at the headline:
# scripts/level_records.py); 16384 blocks per level measured -0.7 ms at 1e8 rows, and the per-rank shape keeps its
# ~37K-record chunks (SEG_MIN_BLOCKS) -- profiles/r6/headline_ab.md
LANE10_CHUNK_MAX = 40960
# row-major bins copy for segment histograms (one cache line per row instead of one per 8-feature group)
SEG_ROW_MAJOR = True
SEG_PART_CHUNK = 8192


def seg_scales(v0p: Optional[torch.Tensor], v1p: torch.Tensor, wmax: int, n_global: int, comm=None):
    """Fixed-point scales for one tree's statistics (packed when there is no v0).

    With ``comm`` the max |v|, the max weight and ``n_global`` are agreed over every rank first: all ranks
    then quantise identically and their int64 histograms all-reduce to the same sums on 1 or N GPUs."""
    if v0p is None:
        return 1.0, packed_scale_global(v1p, comm)
    if comm is None or not comm.distributed:
        return (_fixed_scale(v0p, n_global, wmax, qmax_bits=30), _fixed_scale(v1p, n_global, wmax, qmax_bits=30))
    m = torch.tensor([_absmax(v0p) if v0p.numel() else 0.0,
                      _absmax(v1p) if v1p.numel() else 0.0, float(wmax)], dtype=torch.float64)
    comm.all_reduce(m, "max")
    w = int(m[2])
    return (_fixed_scale(m[0:1], n_global, w, qmax_bits=30), _fixed_scale(m[1:2], n_global, w, qmax_bits=30))


SEG_MIN_BLOCKS = 2048
# wide-bin (80 < B <= 256, boosting) record levels: work items per level (x ceil(d / 64) feature blocks).  Every block
# clears and flushes 64 features x B bins of LDS cells into the level histogram with global atomics, so at deep
# boosting levels (fewer rows, the same number of blocks) the flush -- not the rows -- sets the level time.
# bench_configs.py gbdt (1e8 x 100, 256 bins), 3 interleaved reps: 1024 -> 28.05-28.23, 768 -> 27.83-27.85,
# 512 -> 27.78-27.83 ms per tree (profiles/r4/gbdt_min_blocks_ab.txt)
SEG_MIN_BLOCKS_WIDE = 512
# record histograms through the lane-feature kernel (seg_hist_lane_kernel: lanes own features, bin-major
# conflict-free LDS planes, one v_perm per cell address); B <= 80 (4 planes <= 80 KB of LDS), 80 < B <= 256:
# seg_hist_lane4_kernel (64 features per block, a quarter-wave per item; SEG_LANE=False keeps the flat kernel)
SEG_LANE = True
# seg10 rows + the six-items-per-wave record histogram for 80 < d <= 100, B <= 40 (SEG10=False: lane8 rows)
SEG10 = True
SEG_LANE_MAX_B = 256
# records buffers carry REC_PAD readable entries past their end: the lane kernel's record loads are unconditional
REC_PAD = 128


# the record histograms' host planning (_fill_chunk + _seg_work) in the native library (csrc/kernels/plan.hip): ~250 us
# of numpy per level -> a few us, off the GPU's critical path at the 8-GPU shard size
def _seg_plan(segs: np.ndarray, chunk: int, B: int, ncu: int, interleave: bool):
    """(chunk, work) = (_fill_chunk(segs, chunk, B, ncu), _seg_work(segs, that chunk, interleave)), natively."""
    segs = np.ascontiguousarray(np.asarray(segs, dtype=np.int64).reshape(-1, 3))
    k = len(segs)
    mb = SEG_MIN_BLOCKS if B <= 64 else min(SEG_MIN_BLOCKS, SEG_MIN_BLOCKS_WIDE)
    L = _lib.lib()
    lens = np.ascontiguousarray(segs[:, 1])
    c = int(L.cdna_fill_chunk(lens.ctypes.data, k, int(chunk), int(B), int(ncu), int(mb)))
    total = int(lens.clip(min=0).sum())
    cap = total // max(1, c) + k + 1
    out = np.empty((cap, 3), dtype=np.int32)
    m = int(L.cdna_seg_work(segs.ctypes.data, k, c, int(bool(interleave)), out.ctypes.data, cap))
    assert m >= 0, (m, cap)
    return c, out[:m]


def _fill_chunk(segs: np.ndarray, chunk: int, B: int = 0, ncu: int = 0) -> int:
    """Shrink the rows-per-block chunk so a level with few rows still launches ~SEG_MIN_BLOCKS blocks
    (at 1.25e7 rows per GPU a level's 95K-row chunks made only ~100 blocks for 256 CUs).  With 2048 instead of
    1024 the per-rank shape of the 8-GPU point ran 22.6 -> 21.2 ms (the last round of blocks no longer idles
    half the chip); wide-bin levels (B > 64: 128 KB LDS planes to clear and flush per block) keep 1024.

    ncu > 0 (one block per CU, B <= 64): when the per-segment rounding leaves a last round of blocks less than
    half full (2048 target blocks + one partial chunk per segment = 8 rounds + a sliver), the chunk grows -- up to
    ``chunk`` -- just enough for the blocks to fit the whole rounds before it."""
    lens = np.asarray(segs, dtype=np.int64).reshape(-1, 3)[:, 1].clip(min=0)
    total = int(lens.sum())
    mb = SEG_MIN_BLOCKS if B <= 64 else min(SEG_MIN_BLOCKS, SEG_MIN_BLOCKS_WIDE)
    c0 = int(min(chunk, max(8192, -(-total // max(1, mb)))))
    if ncu <= 0 or B > 64 or c0 >= chunk:
        return c0
    lens = lens[lens > 0]
    blocks = int(((lens + c0 - 1) // c0).sum())
    R, rem = divmod(blocks, ncu)
    if R < 1 or rem == 0 or rem > ncu // 2:
        return c0
    lo, hi = c0, int(chunk)
    if int(((lens + hi - 1) // hi).sum()) > R * ncu:
        return c0
    # the answer c satisfies total / c <= sum ceil(len / c) <= R * ncu and sum ceil(len / c) <= total / c + k:
    # it lies in [total / (R ncu), total / (R ncu - k)] (a few bisection steps, not ~17 over [c0, chunk])
    cap = R * ncu
    lo = max(lo, -(-total // cap))
    if cap > len(lens):
        hi = min(hi, -(-total // (cap - len(lens))))
    while lo < hi:  # smallest chunk whose blocks fit R rounds
        mid = (lo + hi) // 2
        if int(((lens + mid - 1) // mid).sum()) <= R * ncu:
            hi = mid
        else:
            lo = mid + 1
    return lo


def _seg_work(segs: np.ndarray, chunk: int, interleave: bool = False) -> np.ndarray:
    """segs [k, 3] {start, len, tag} -> work items [m, 3] of at most `chunk` rows each.

    interleave: ordered by relative position inside the segment, so that concurrently running blocks gather nearby
    rows (chunk j of every segment covers about the same fraction of the row ids; placing rounds of chunks on one
    XCD for L2 sharing measured no better and was dropped), built in the same pass: the
    position is bucketed to a uint16 key (chunk j of a k-chunk segment -> j * kmax // k), whose stable argsort is a
    radix sort -- the float key's merge sort plus a second pass cost ~60-70 us of host time per level at the
    per-rank shape, while the GPU waited.  Any order gives the same histograms (exact fixed-point sums)."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 3)
    segs = segs[segs[:, 1] > 0]
    if len(segs) == 0:
        return np.zeros((0, 3), dtype=np.int32)
    k = (segs[:, 1] + chunk - 1) // chunk
    rep = np.repeat(np.arange(len(segs)), k)
    j = np.arange(len(rep)) - (np.cumsum(k) - k)[rep]
    if interleave and len(segs) > 1:
        kmax = int(k.max())
        key = j * kmax // k[rep]
        if kmax < 1 << 16:
            key = key.astype(np.uint16)
        o = np.argsort(key, kind="stable")
        rep, j = rep[o], j[o]
    out = np.empty((len(rep), 3), dtype=np.int32)
    out[:, 0] = segs[rep, 0] + j * chunk
    out[:, 1] = np.minimum(chunk, segs[rep, 1] - j * chunk)
    out[:, 2] = segs[rep, 2]
    return out


def seg_hist(bins: torch.Tensor, d: int, B: int, perm: torch.Tensor, v0p: Optional[torch.Tensor],
             v1p: torch.Tensor, wp: Optional[torch.Tensor], segs: np.ndarray, S: int, wmax: int,
             scales=None, bins_rm: Optional[torch.Tensor] = None, interleave: bool = False,
             rec: bool = False, raw: bool = False, out: Optional[torch.Tensor] = None,
             rm_s10: bool = False, cls3: bool = False) -> torch.Tensor:
    """Moments [S, d, B, 2] of node segments of ``perm`` (row ids grouped by node).

    rm_s10 (rec): ``bins_rm`` is in the seg10 layout (:func:`bins_seg10`): the six-items-per-wave kernel.

    cls3 (rec + raw): 3-class records (label codes 0 / 1 / ``CLS3_CODE``, scale 1): the sums are [S, d, B, 3]
    (W, W1, W2) (:func:`cls3_expand` turns them into class counts).

    out (rec + raw): a zeroed int64 [S, d, B, 2] tensor (e.g. a slot-range slice of a level's buffer) the sums
    are accumulated into and returned -- lets the engine all-reduce one slot chunk while the next is built.

    rec: ``perm`` holds packed int64 item records from ``codes_compact(rec_scale=scales[1])`` (v1p/wp unused;
    GPU with ``bins_rm`` only).  raw (with rec): return the exact int64 fixed-point sums (count, sum * scales[1])
    instead of fp64 moments, so ranks can all-reduce integers (also without rec: (sum w*q0 | count, sum w*q1)).
    CPU: the same fixed-point integers as the HIP kernels (fp32 quantisation, int64 sums), so CPU ranks
    traverse the exact arithmetic of the GPU path."""
    if out is not None:
        assert rec and raw and out.dtype == torch.int64 and out.is_contiguous()
    if rec:
        return _seg_hist_rec(bins, d, B, perm, segs, S, wmax, scales, bins_rm, interleave, raw, out, rm_s10, cls3)
    assert not rm_s10
    return _seg_hist(bins, d, B, perm, v0p, v1p, wp, segs, S, wmax, scales, bins_rm, interleave, raw)


def _seg_flat_index(bins: torch.Tensor, d: int, B: int, rows: torch.Tensor, slot: torch.Tensor) -> torch.Tensor:
    """CPU: flat cell index slot * d * B + f * B + bin(row, f) of every (row, feature) pair, [m, d]."""
    G, n, _ = bins.shape
    flat = bins.permute(1, 0, 2).reshape(n, G * 8)[:, :d].long()
    return slot[:, None] * (d * B) + torch.arange(d)[None, :] * B + flat[rows]


def _int_hist_cpu(bins, d, B, S, rows, slot, *cols) -> torch.Tensor:
    """CPU: exact int64 sums of per-item integers (a0, a1[, a2]) into cells [S, d, B, len(cols)]."""
    k = len(cols)
    out = torch.zeros(S * d * B * k, dtype=torch.int64)
    if rows.numel():
        idx = _seg_flat_index(bins, d, B, rows, slot) * k
        for j, a in enumerate(cols):
            out.index_add_(0, idx.reshape(-1) + j, a[:, None].expand(-1, d).reshape(-1))
    return out.view(S, d, B, k)


def _seg_items(segs: np.ndarray):
    """segs [k, 3] {start, len, slot} -> (item positions, item slots) as int64 tensors."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 3)
    segs = segs[segs[:, 1] > 0]
    if len(segs) == 0:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    ln = segs[:, 1]
    pos = np.repeat(segs[:, 0], ln) + (np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln))
    return torch.from_numpy(pos), torch.from_numpy(np.repeat(segs[:, 2], ln))


def _quant(v: torch.Tensor, scale: float, clamp: bool) -> torch.Tensor:
    """The kernels' fixed-point quantisation: rintf(v * scale) in fp32 (clamped to +-2^23 when packed)."""
    q = torch.round(v.float() * torch.tensor(scale, dtype=torch.float32)).to(torch.int64)
    return q.clamp(-PACK_Q, PACK_Q) if clamp else q


# 3-class packed records (packed.h kClsSplit): class c's label code is 0 / 1 / CLS3_CODE, so a histogram block's
# sum w * q is W1 + 2^22 W2 (W1 < 2^22 inside a block); the kernels' flush splits it into two int64 columns, so the
# level histograms are [S, d, B, 3] (W, W1, W2) and their global sums have no size bound (round 5 packed
# W1 + 2^32 W2 in one column: n_global * 255 < 2^32 rows at most)
CLS3_CODE = 1 << 22


def hist_cols(cls3: bool) -> int:
    """Int64 columns per cell of a record histogram: (count, sum), or (W, W1, W2) for 3-class records."""
    return 3 if cls3 else 2


def cls3_expand(Hb: torch.Tensor) -> torch.Tensor:
    """3-class record sums [..., 3] (W, W1, W2) -> exact int64 class counts [..., 3] (W0, W1, W2)."""
    W, W1, W2 = Hb[..., 0], Hb[..., 1], Hb[..., 2]
    return torch.stack([W - W1 - W2, W1, W2], -1)


# the packed item record and LDS cell formats: csrc/kernels/packed.h describes the layouts, these name its numbers
PACK_SHIFT = 44                  # cell: count << PACK_SHIFT | sum of w * (q + PACK_Q)
PACK_Q = 1 << 23                 # |q| <= PACK_Q; stored offset by it
PACK_COUNT_BITS = 64 - PACK_SHIFT
REC_ROW_BITS = 31                # record: row | w << REC_ROW_BITS | (q + PACK_Q) << (REC_ROW_BITS + REC_W_BITS)
REC_W_BITS = 8
_REC_Q_SHIFT = REC_ROW_BITS + REC_W_BITS


# cdna_seg_hist mode bits (csrc/kernels/seg.hip SegHistMode)
SEG_MODE_PACKED = 1        # no v0: count | sum in one packed cell
SEG_MODE_HAS_W = 2         # per-row weights
SEG_MODE_ROW_MAJOR = 4     # bins are the row-major copy
SEG_MODE_FORCE_RM = 8      # seg_hist_rm_kernel even where the flat kernel fits
SEG_MODE_REC = 16          # perm holds packed item records
SEG_MODE_LANE = 128        # lane-feature record kernels
SEG_MODE_ROWS10 = 256      # seg10 rows: the six-items-per-wave kernel
SEG_MODE_CLS3 = 512        # 3-class records


def pack_rows_cap(wm: int) -> int:
    """Items of weight <= ``wm`` that one packed cell's count field can hold."""
    return (1 << PACK_COUNT_BITS) // (wm + 1)


def rec_decode(rec: torch.Tensor):
    """Packed item records -> (row, weight, quantised label) int64 tensors."""
    r = rec.to(torch.int64)
    return (r & ((1 << REC_ROW_BITS) - 1), (r >> REC_ROW_BITS) & ((1 << REC_W_BITS) - 1),
            ((r >> _REC_Q_SHIFT) & ((1 << (64 - _REC_Q_SHIFT)) - 1)) - PACK_Q)


def rec_encode(rows: torch.Tensor, w: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    return rows.to(torch.int64) | (w.to(torch.int64) << REC_ROW_BITS) | ((q.to(torch.int64) + PACK_Q) << _REC_Q_SHIFT)


def _seg_hist_rec(bins, d, B, rec, segs, S, wmax, scales, bins_rm, interleave, raw=False, out=None, rm_s10=False,
                  cls3=False):
    G, n, _ = bins.shape
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 3)
    kc = hist_cols(cls3)
    if S == 0 or len(segs) == 0:
        if out is not None:
            return out
        return torch.zeros((S, d, B, kc), dtype=torch.int64 if raw else torch.float64, device=bins.device)
    qs1 = float(scales[1])
    if not _native(bins):
        pos, slot = _seg_items(segs)
        rows, w, q = rec_decode(rec[pos])
        if cls3:
            iout = _int_hist_cpu(bins, d, B, S, rows, slot, w, w * (q & (CLS3_CODE - 1)), w * (q >> 22))
        else:
            iout = _int_hist_cpu(bins, d, B, S, rows, slot, w, w * q)
        if out is not None:
            iout = out.copy_(iout)
    else:
        assert bins_rm is not None and rec.dtype == torch.int64
        wm = int(max(1, min(255, wmax)))
        # one count field per chunk, also for the six-items-per-wave kernel, whose three cell copies could hold
        # three times the rows: such chunks measured 145.1 vs 139.8 ms per headline step (fewer, longer blocks)
        cap = pack_rows_cap(wm)
        top = SEG_HIST_CHUNK
        if rm_s10 and int(segs[:, 1].sum()) > 2 * LANE10_CHUNK_MAX * SEG_MIN_BLOCKS:
            # large levels only: the smaller levels of a shard keep _fill_chunk's round fitting (its chunks grow
            # to drop a sliver round; capping them cost +0.25 ms at 1.25e7 rows)
            top = min(top, LANE10_CHUNK_MAX)
        # seg10 levels fit their chunks to whole rounds of blocks (_fill_chunk, ncu > 0): without it 19.0 / 19.1
        # vs 18.6 / 18.7 ms per step at 1.25e7 rows (profiles/r4/round_fill_ab.md)
        ncu = _num_cus(bins.device) if (rm_s10 and bins.is_cuda) else 0
        chunk, work = _seg_plan(segs, min(top, cap), B, ncu, interleave)
        if len(work) == 0:
            if out is not None:
                return out
            return torch.zeros((S, d, B, kc), dtype=torch.int64 if raw else torch.float64, device=bins.device)
        wt, = upload(bins.device, work.reshape(-1))
        iout = out if out is not None else torch.zeros((S, d, B, kc), dtype=torch.int64, device=bins.device)
        assert iout.shape == (S, d, B, kc)
        assert bins_rm.shape[0] == n and bins_rm.shape[1] >= G and bins_rm.is_contiguous()
        mode = (SEG_MODE_PACKED | SEG_MODE_ROW_MAJOR | SEG_MODE_REC |
                (SEG_MODE_LANE if (SEG_LANE and B <= SEG_LANE_MAX_B) else 0) | (SEG_MODE_CLS3 if cls3 else 0))
        if rm_s10:
            assert d <= 100 and B <= 40 and bins_rm.shape[1] == 16
            mode |= SEG_MODE_LANE | SEG_MODE_ROWS10
        _lib.check(_lib.lib().cdna_seg_hist(mode, _ptr(bins_rm), n, d, B, _ptr(rec), None, None, None,
                                            _ptr(wt), len(work), 1.0, qs1, _ptr(iout), bins_rm.shape[1],
                                            _stream(bins.device)), "cdna_seg_hist(rec)")
    if raw:
        return iout
    out = iout.double()
    out[..., 1] /= qs1
    return out


_NCU = {}


def _num_cus(dev) -> int:
    if dev.index not in _NCU:
        _NCU[dev.index] = int(torch.cuda.get_device_properties(dev).multi_processor_count)
    return _NCU[dev.index]


def seg_hist_codes(bins_s10: torch.Tensor, d: int, B: int, codes: torch.Tensor, v1: torch.Tensor, qs1: float,
                   wmax: int, slot_tree: np.ndarray, slot_node: np.ndarray, s0: int, s1: int,
                   out: torch.Tensor, draw: Optional[tuple] = None, cls3: bool = False,
                   move: Optional[tuple] = None) -> torch.Tensor:
    """Record histograms of slots [s0, s1) straight from the row codes (GPU, seg10 rows), for levels with at most
    one built node per tree: slot s is local node ``slot_node[s]`` of tree ``slot_tree[s]`` (level 0: every root,
    node 0).  Adds the exact int64 sums (count, sum w * q) into ``out`` [s1 - s0, d, B, 2] (zeroed by the caller)
    -- the same integers as ``codes_compact(rec_scale=qs1)`` + ``seg_hist(rec=True, raw=True)``, without
    materialising the level's 8-byte records.

    draw (level 0 of a bootstrapped forest, B <= 40): ``(seed, row offset, rate)`` -- the kernel draws every row's
    Poisson weight itself and WRITES ``codes`` (the lazy :class:`BootstrapCodes`); ``wmax`` must then be the draws'
    static bound (``poisson_max_draw``).

    move (level 1, B <= 40, slots [0, T): one per tree): ``(dec, bins[, numeric])`` -- ``codes`` still hold level 0
    (the row partition was not run): the kernel moves them to level 1 in place, as ``partition_codes`` with
    ``split_decode``'s level-0 tables ``dec`` and the column-major ``bins`` [G, n, 8] would have, and builds the
    histograms of the moved codes.  Numeric splits only (``numeric``: the caller vouches, no device read)."""
    T, n = codes.shape
    wide = 80 < B <= 256
    # B <= 40: seg10 rows, six-items-per-wave kernel; 80 < B <= 256 (boosting): standard row-major rows, lane4
    assert _native(codes) and ((d <= 100 and B <= 40 and bins_s10.shape == (n, 16, 8)) or
                               (wide and bins_s10.shape[0] == n and bins_s10.shape[1] * 8 >= d and
                                bins_s10.is_contiguous()))
    assert out.dtype == torch.int64 and out.is_contiguous() and out.shape == (s1 - s0, d, B, hist_cols(cls3))
    st = np.asarray(slot_tree, dtype=np.int64)
    sn = np.asarray(slot_node, dtype=np.int64)
    assert len(st) == len(sn) and np.all((st >= 0) & (st < T)) and np.all((sn >= 0) & (sn < 0xFF))
    assert len(np.unique(st[s0:s1])) == s1 - s0  # one built node per tree
    if move is not None:
        dec, bins_cm = move[0], move[1]
        G = bins_cm.shape[0]
        tabs = [dec[k].to(device=codes.device, dtype=torch.int32).contiguous()
                for k in ("split_feat", "split_bin", "cat_off", "child", "tfirst_next")]
        assert draw is None and not wide and d <= 100 and B <= 40, "the fused move runs on seg10 rows, drawn codes"
        assert s0 == 0 and s1 - s0 == T, "the fused move needs one slot per tree (else a tree's codes stay unmoved)"
        assert _native(bins_cm) and bins_cm.dtype == torch.uint8 and bins_cm.is_contiguous() and \
            bins_cm.shape == (G, n, 8) and G * 8 >= d
        assert [t.numel() for t in tabs] == [T, T, T, 2 * T, T], "level-0 tables: one active node per tree"
        # (the trainer knows from the host that its splits are numeric; any other caller pays one device read)
        assert (len(move) > 2 and move[2]) or not bool((tabs[2] >= 0).any()), "categorical / bin-set root split"
    if n == 0 or s1 <= s0:
        return out
    wm = int(max(1, min(255, wmax)))
    sinfo = np.stack([st, sn], 1).astype(np.int32).reshape(-1)
    v1c = v1.float().contiguous()
    key = (n, d, B, wm, s0, s1, wide, str(codes.device))
    work = _ROOT_WORK.get(key)
    if work is None:
        work = _root_work(n, d, wide, wm, s0, s1, codes.device)
        if len(_ROOT_WORK) > 64:
            _ROOT_WORK.clear()
        _ROOT_WORK[key] = work
    if wide:
        wt, si = upload(codes.device, work.reshape(-1), sinfo)
        _lib.check(_lib.lib().cdna_seg_hist_root_wide(_ptr(bins_s10), n, d, B, bins_s10.shape[1] * 8, _ptr(codes),
                                                      _ptr(v1c), float(qs1), _ptr(wt), len(work), _ptr(si), s0,
                                                      _ptr(out), int(cls3), _stream(codes.device)),
                   "cdna_seg_hist_root_wide")
        return out
    wt, si = upload(codes.device, work.reshape(-1), sinfo)
    if move is not None:
        _lib.check(_lib.lib().cdna_seg_hist_root_move(_ptr(bins_s10), n, d, B, _ptr(codes), _ptr(v1c), float(qs1),
                                                      _ptr(wt), len(work), _ptr(si), s0, _ptr(out), _ptr(bins_cm), G,
                                                      T, *[_ptr(t) for t in tabs], int(cls3),
                                                      _stream(codes.device)),
                   "cdna_seg_hist_root_move")
        return out
    if draw is not None:
        assert np.array_equal(np.sort(st[s0:s1]), np.arange(T)) and not np.any(sn[s0:s1]), "draws need every root"
    seed, off, rate = draw if draw is not None else (0, 0, 1.0)
    _lib.check(_lib.lib().cdna_seg_hist_root(_ptr(bins_s10), n, d, B, _ptr(codes), _ptr(v1c), float(qs1), _ptr(wt),
                                             len(work), _ptr(si), s0, _ptr(out), int(draw is not None),
                                             int(seed) & 0xFFFFFFFFFFFFFFFF, int(off), float(rate), int(cls3),
                                             _stream(codes.device)),
               "cdna_seg_hist_root")
    return out


# (shape, slot range, device) -> the root / codes histogram work list: the same for every fit of a shard, so its
# host planning (~100 us of numpy per level, on the critical path between a level's decisions and the next level's
# first launch at the per-rank shape) runs once
_ROOT_WORK: Dict[tuple, np.ndarray] = {}


def _root_work(n: int, d: int, wide: bool, wm: int, s0: int, s1: int, device) -> np.ndarray:
    """Work items [m, 3] {row start, rows, slot} of a codes histogram over slots [s0, s1) (see seg_hist_codes)."""
    # each LDS cell copy takes every third item of a wave's stream: rows x wmax / 3 (+ a partial trip per
    # wave) stays below the count field (the wide kernel has one copy: rows x wmax).  The largest chunks the field
    # allows: shrinking them toward 4096 blocks ran 21.0-21.3 vs 20.0-20.1 ms per step at the per-rank 1.25e7
    # shape (the per-block LDS clear + flush of 100 KB outweighs the emptier last round)
    rows = max(64, min(n, pack_rows_cap(wm) - 64 if wide else 3 * pack_rows_cap(wm) - 16 * 64))
    S_l = max(1, s1 - s0)
    rows = (rows + 63) // 64 * 64
    C = (n + rows - 1) // rows
    bpc = S_l * (-(-d // 64) if wide else 1)  # blocks per row chunk (the wide kernel: one per 64 features)
    if device.type == "cuda":
        # at least two rounds of blocks (one block per CU) while blocks keep >= 4096 rows: a boosting level of
        # 1.25e7 rows in 524k-row chunks would run 48 blocks on 256 CUs
        C_min = min(-(-2 * _num_cus(device) // bpc), max(1, n // 4096))
        if C < C_min:
            C = C_min
            rows = (-(-n // C) + 63) // 64 * 64
            C = (n + rows - 1) // rows
    if C * bpc < 64 * _num_cus(device):
        # one block per CU: spread the rows over as many chunks as the rounds of blocks already needed can hold,
        # so the last round is full instead of a fraction of the chip (1.25e7 rows x 20 trees: 640 blocks in 2.5
        # rounds -> 760 in 2.97, 19.2 -> 18.9 ms per step; an exact multiple of the CUs, 1280 blocks in 5
        # rounds, pays each block's 100 KB LDS clear + flush twice as often)
        ncu = _num_cus(device)
        rounds = -(-(C * bpc) // ncu)
        C2 = max(C, (rounds * ncu) // bpc)
        if C2 > C:
            rows = (-(-n // C2) + 63) // 64 * 64
            C = (n + rows - 1) // rows
    # XCD-aware order: block b runs on XCD b % 8; the slots (trees) of row chunk c are consecutive blocks of
    # XCD c % 8, so their row-line gathers and label reads share that XCD's L2
    nq = (C + 7) // 8
    cq, sl, x = np.meshgrid(np.arange(nq), np.arange(s0, s1), np.arange(8), indexing="ij")  # (cq, slot, x) order
    c = (cq * 8 + x).reshape(-1)
    keep = c < C
    c, sl = c[keep], sl.reshape(-1)[keep]
    r0 = c * rows
    work = np.stack([r0, np.minimum(rows, n - r0), sl], 1).astype(np.int32)
    if wide:
        # the kernel pairs the feature blocks of each item on one XCD itself: items in (chunk, slot) order
        work = work[np.lexsort((work[:, 2], work[:, 0]))]
    return work


def seg_hist_root(bins_s10: torch.Tensor, d: int, B: int, codes: torch.Tensor, v1: torch.Tensor, qs1: float,
                  wmax: int, t0: int, t1: int, out: torch.Tensor) -> torch.Tensor:
    """Level 0: :func:`seg_hist_codes` with slot t = the root (local node 0) of tree t, slots [t0, t1)."""
    T = codes.shape[0]
    return seg_hist_codes(bins_s10, d, B, codes, v1, qs1, wmax, np.arange(T), np.zeros(T, np.int64), t0, t1, out)


def _seg_hist(bins: torch.Tensor, d: int, B: int, perm: torch.Tensor, v0p: Optional[torch.Tensor],
              v1p: torch.Tensor, wp: Optional[torch.Tensor], segs: np.ndarray, S: int, wmax: int,
              scales=None, bins_rm: Optional[torch.Tensor] = None, interleave: bool = False,
              raw: bool = False) -> torch.Tensor:
    """Moments [S, d, B, 2] of node segments of ``perm`` (row ids grouped by node).

    segs: [k, 3] {start, len, slot}.  [..., 0] = sum w*v0 (or sum w when v0p is None), [..., 1] = sum w*v1.
    interleave: order the work items by their relative position inside their segment, so that segments
    of different trees (whose rows are all sorted by row id) gather the same region of the bins at the
    same time and share it through L2 / MALL.
    raw: return the int64 fixed-point sums (stat k scaled by ``scales[k]``; stat 0 unscaled when packed).
    """
    G, n, _ = bins.shape
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 3)
    packed = v0p is None
    wm = int(max(1, min(255, wmax)))
    zero = lambda: torch.zeros((S, d, B, 2), dtype=torch.int64 if raw else torch.float64,  # noqa: E731
                               device=bins.device)
    if S == 0 or len(segs) == 0:
        return zero()
    qs0, qs1 = scales if scales is not None else seg_scales(v0p, v1p, wm, n)
    if not _native(bins):
        pos, slot = _seg_items(segs)
        rows = perm[pos].long()
        w = torch.ones(len(pos), dtype=torch.int64) if wp is None else wp[pos].to(torch.int64)
        if packed:
            a0, a1 = w, w * _quant(v1p[pos], qs1, True)
        else:
            a0, a1 = w * _quant(v0p[pos], qs0, False), w * _quant(v1p[pos], qs1, False)
        iout = _int_hist_cpu(bins, d, B, S, rows, slot, a0, a1)
    else:
        chunk = SEG_HIST_CHUNK if not packed else min(SEG_HIST_CHUNK, pack_rows_cap(wm))
        chunk = _fill_chunk(segs, chunk, B)
        work = _seg_work(segs, chunk, interleave)
        if len(work) == 0:
            return zero()
        wt, = upload(bins.device, work.reshape(-1))
        iout = torch.zeros((S, d, B, 2), dtype=torch.int64, device=bins.device)
        mode = ((SEG_MODE_PACKED if packed else 0) | (SEG_MODE_HAS_W if wp is not None else 0) |
                (SEG_MODE_ROW_MAJOR if bins_rm is not None else 0))
        if bins_rm is not None:
            assert bins_rm.shape[0] == n and bins_rm.shape[1] >= G and bins_rm.is_contiguous()
        src = bins if bins_rm is None else bins_rm
        _lib.check(_lib.lib().cdna_seg_hist(mode, _ptr(src), n, d, B, _ptr(perm), _ptr(v0p), _ptr(v1p), _ptr(wp),
                                            _ptr(wt), len(work), float(qs0), float(qs1), _ptr(iout),
                                            0 if bins_rm is None else bins_rm.shape[1], _stream(bins.device)),
                   "cdna_seg_hist")
    if raw:
        return iout
    out = iout.double()
    if not packed:
        out[..., 0] /= qs0
    out[..., 1] /= qs1
    return out


def seg_partition(bins: torch.Tensor, perm: Optional[torch.Tensor], v0p: Optional[torch.Tensor], v1p: torch.Tensor,
                  wp: Optional[torch.Tensor], segs: np.ndarray, split_feat: np.ndarray, split_bin: np.ndarray,
                  cat_off: np.ndarray, cat_mask: np.ndarray, child: np.ndarray, n_next: int):
    """Stable split of every node segment into its children's segments (rows of leaves dropped).

    segs [A, 2] {start, len} of the active nodes (in active order); child [2A] next-level node index
    or -1; n_next = number of next-level nodes.  Returns (perm, v0p, v1p, wp, segs_next [n_next, 2]).

    ``perm=None`` is the level-0 entry of multi-tree segment mode: active node a is the root of tree
    a over all n rows, ``wp`` is the [T, n] bootstrap weight matrix, ``v0p``/``v1p`` are the unpermuted
    per-row statistics, and rows whose weight in that tree is 0 are dropped.
    """
    G, n, _ = bins.shape
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 2)
    A = len(segs)
    dev = v1p.device
    sf = np.asarray(split_feat, dtype=np.int32)
    implicit = perm is None
    if implicit:
        assert wp is not None and wp.shape == (A, n) and wp.is_contiguous(), "implicit entry needs [T, n] weights"
        assert np.array_equal(segs[:, 0], np.arange(A) * n) and np.all(segs[:, 1] == n)
        assert A * n < 2 ** 31, "multi-tree segment mode indexes rows with int32"
    if not _native(bins):
        flat = bins.permute(1, 0, 2).reshape(n, G * 8)
        pieces = [[] for _ in range(max(n_next, 0))]
        for a in range(A):
            s, ln = segs[a]
            if ln == 0 or sf[a] < 0:
                continue
            idx = torch.arange(int(s), int(s + ln))
            if implicit:
                rows = idx - a * n
                keep = wp[a].cpu() > 0
                idx, rows = idx[keep], rows[keep]
            else:
                rows = perm[idx].long()
            bv = flat[rows, int(sf[a])].long()
            if cat_off[a] >= 0:
                m = torch.from_numpy(np.asarray(cat_mask, dtype=np.int64).reshape(-1, 8)[cat_off[a]] & 0xFFFFFFFF)
                left = ((m[bv >> 5] >> (bv & 31)) & 1).bool()
            else:
                left = bv <= int(split_bin[a])
            for side, sel in ((0, left), (1, ~left)):
                c = int(child[2 * a + side])
                if c >= 0:
                    pieces[c].append(idx[sel])
        order = [torch.cat(p) if p else torch.zeros(0, dtype=torch.long) for p in pieces]
        lens = np.array([len(o) for o in order], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) if n_next else np.zeros(0, np.int64)
        cat = torch.cat(order) if order else torch.zeros(0, dtype=torch.long)
        if implicit:
            rows = cat % n
            return (rows.to(torch.int32).contiguous(), None if v0p is None else v0p[rows].contiguous(),
                    v1p[rows].contiguous(), wp.reshape(-1)[cat].contiguous(), np.stack([starts, lens], 1))
        return (perm[cat].contiguous(), None if v0p is None else v0p[cat].contiguous(), v1p[cat].contiguous(),
                None if wp is None else wp[cat].contiguous(), np.stack([starts, lens], 1))
    # native: pass 1 counts left/right rows per chunk, host computes output offsets, pass 2 scatters
    tags = np.arange(A, dtype=np.int64)
    work = _seg_work(np.concatenate([segs, tags[:, None]], 1), SEG_PART_CHUNK)
    nw = len(work)
    L = _lib.lib()
    cm = np.asarray(cat_mask, dtype=np.int32).reshape(-1)
    sf_t, sb_t, co_t, cm_t, wt = upload(dev, sf, np.asarray(split_bin, dtype=np.int32),
                                        np.asarray(cat_off, dtype=np.int32), cm if cm.size else np.zeros(8, np.int32),
                                        work.reshape(-1))
    lrc = torch.zeros((2, max(nw, 1)), dtype=torch.int32, device=dev)
    impl_n = n if implicit else 0
    if nw:
        _lib.check(L.cdna_seg_partition(1, _ptr(bins), n, _ptr(perm), None, None, _ptr(wp) if implicit else None,
                                        _ptr(wt), nw, _ptr(sf_t), _ptr(sb_t), _ptr(co_t), _ptr(cm_t), None, None,
                                        _ptr(lrc[0]), None, None, None, None, impl_n, _ptr(lrc[1]), _stream(dev)),
                   "cdna_seg_partition(count)")
    lrc_h = lrc.cpu().numpy()[:, :nw].astype(np.int64)
    lc_h, rc_h = lrc_h[0], lrc_h[1]
    wseg = work[:, 2].astype(np.int64)
    child = np.asarray(child, dtype=np.int64)
    # child sizes
    lens = np.zeros(n_next, dtype=np.int64)
    cl, cr = child[2 * wseg], child[2 * wseg + 1]
    splits = sf[wseg] >= 0
    np.add.at(lens, cl[splits & (cl >= 0)], lc_h[splits & (cl >= 0)])
    np.add.at(lens, cr[splits & (cr >= 0)], rc_h[splits & (cr >= 0)])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) if n_next else np.zeros(0, np.int64)
    # per-chunk offsets: child start + rows of the same child in earlier chunks of the segment
    # (work items are in segment order: exclusive scans restart at each segment's first chunk)
    first = np.searchsorted(wseg, wseg, side="left")
    ex_l = np.cumsum(lc_h) - lc_h
    ex_r = np.cumsum(rc_h) - rc_h
    off_l = ex_l - ex_l[first]
    off_r = ex_r - ex_r[first]
    lb = np.where(splits & (cl >= 0), starts[np.maximum(cl, 0)] + off_l, -1) if n_next else np.full(nw, -1)
    rb = np.where(splits & (cr >= 0), starts[np.maximum(cr, 0)] + off_r, -1) if n_next else np.full(nw, -1)
    total = int(lens.sum())
    assert total < 2 ** 31
    perm_o = torch.empty(total, dtype=torch.int32, device=dev)
    v1_o = torch.empty(total, dtype=torch.float32, device=dev)
    v0_o = None if v0p is None else torch.empty(total, dtype=torch.float32, device=dev)
    w_o = None if wp is None else torch.empty(total, dtype=torch.uint8, device=dev)
    if nw and total:
        lb_t, rb_t = upload(dev, lb.astype(np.int32), rb.astype(np.int32))
        _lib.check(L.cdna_seg_partition(2, _ptr(bins), n, _ptr(perm), _ptr(v0p), _ptr(v1p), _ptr(wp), _ptr(wt), nw,
                                        _ptr(sf_t), _ptr(sb_t), _ptr(co_t), _ptr(cm_t), _ptr(lb_t), _ptr(rb_t),
                                        None, _ptr(perm_o), _ptr(v0_o), _ptr(v1_o), _ptr(w_o), impl_n, None,
                                        _stream(dev)), "cdna_seg_partition(scatter)")
    return perm_o, v0_o, v1_o, w_o, np.stack([starts, lens], 1)


def codes_compact(codes: torch.Tensor, tfirst: torch.Tensor, build_slot: np.ndarray, S: int,
                  v0: Optional[torch.Tensor], v1: torch.Tensor, rec_scale: Optional[float] = None):
    """Rows of the nodes a level builds, gathered into one segment per histogram slot.

    codes [T, n] row records (weight << 8 | local node); tfirst [T] first active index per tree;
    build_slot [A] slot of active node a (-1: not built).  Returns (perm int32, v0p, v1p, wp uint8,
    segs [S, 2] {start, len}).  Row order inside a segment is unspecified (the segment histograms
    are exact fixed-point sums, so it does not change any result).

    rec_scale (GPU, no v0, wave-owned path only): return packed int64 item records instead, as
    (rec, None, None, None, segs) with rec = :func:`rec_encode` of (row, w, clamp(rint(v1 * rec_scale), +-PACK_Q)).
    """
    T, n = codes.shape
    dev = codes.device
    A = len(build_slot)
    bs = np.asarray(build_slot, dtype=np.int32)
    _check_codes_level(tfirst.cpu().numpy(), A)
    if not _native(codes):
        c = codes.to(torch.int32) & 0xFFFF
        loc = c & 0xFF
        ids = tfirst.to(torch.int64).to(dev)[:, None] + loc.long()
        slot_t = torch.from_numpy(np.concatenate([bs, [-1]])).to(dev)
        ids = torch.where(loc == CODE_DONE, torch.full_like(ids, A), ids).clamp_max(A)
        slot = slot_t[ids]  # [T, n]
        flat = slot.reshape(-1)
        keep = torch.nonzero(flat >= 0).flatten()
        order = keep[torch.argsort(flat[keep], stable=True)]
        rows = order % n
        lens = np.bincount(flat[keep].numpy(), minlength=S)[:S].astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) if S else np.zeros(0, np.int64)
        wts = c.reshape(-1)[order] >> 8
        if rec_scale is not None and v0 is None and n < 2 ** 31:
            # the packed item records of the HIP compaction (same fp32 quantisation)
            return rec_encode(rows, wts, _quant(v1[rows], rec_scale, True)), None, None, None, \
                np.stack([starts, lens], 1)
        return (rows.to(torch.int32), None if v0 is None else v0[rows].float(), v1[rows].float(),
                wts.to(torch.uint8), np.stack([starts, lens], 1))
    L = _lib.lib()
    assert tfirst.numel() == T
    # built nodes per tree -> wave-owned kernel when few (stable, no atomics)
    tf_h = tfirst.cpu().numpy().astype(np.int64)
    tree_of = np.searchsorted(tf_h, np.arange(A), side="right") - 1
    built = bs >= 0
    nb_t = np.bincount(tree_of[built], minlength=T) if A else np.zeros(T, np.int64)
    kb_need = int(nb_t.max()) if T else 0
    if 0 < kb_need <= 16 and COMPACT_W:
        return _codes_compact_w(codes, tf_h.astype(np.int32), bs, tree_of, built, nb_t, kb_need, S, v0, v1,
                                rec_scale if (v0 is None and n < 2 ** 31) else None)
    tf, bs_t = upload(dev, tf_h.astype(np.int32), bs)
    v1c = v1.float().contiguous()
    v0c = None if v0 is None else v0.float().contiguous()
    cnt = torch.zeros(max(S, 1), dtype=torch.int32, device=dev)
    _lib.check(L.cdna_codes_compact(1, _ptr(codes), n, T, A, _ptr(tf), _ptr(bs_t), _ptr(v0c), _ptr(v1c), _ptr(cnt),
                                    None, None, None, None, None, 0.0, _stream(dev)), "cdna_codes_compact(count)")
    lens = cnt.cpu().numpy()[:S].astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) if S else np.zeros(0, np.int64)
    total = int(lens.sum())
    assert total < 2 ** 31
    rec = rec_scale is not None and v0 is None and n < 2 ** 31
    if rec:
        perm = torch.empty(total + REC_PAD, dtype=torch.int64, device=dev)[:total]  # readable tail
        v1p = v0p = wp = None
    else:
        perm = torch.empty(total, dtype=torch.int32, device=dev)
        v1p = torch.empty(total, dtype=torch.float32, device=dev)
        v0p = None if v0 is None else torch.empty(total, dtype=torch.float32, device=dev)
        wp = torch.empty(total, dtype=torch.uint8, device=dev)
    if total:
        cur, = upload(dev, np.concatenate([starts, [0]]).astype(np.int32))
        _lib.check(L.cdna_codes_compact(2, _ptr(codes), n, T, A, _ptr(tf), _ptr(bs_t), _ptr(v0c), _ptr(v1c),
                                        _ptr(cur), None if rec else _ptr(perm), _ptr(v0p), _ptr(v1p), _ptr(wp),
                                        _ptr(perm) if rec else None, float(rec_scale) if rec else 0.0,
                                        _stream(dev)), "cdna_codes_compact(scatter)")
    return perm, v0p, v1p, wp, np.stack([starts, lens], 1)


def node_compact(node: torch.Tensor, w: torch.Tensor, tfirst: np.ndarray, build_slot: np.ndarray, S: int,
                 v1: torch.Tensor, rec_scale: float):
    """The packed item records of the rows of a level's built nodes from node ids (the levels below the u16
    codes: node [T, n] int32 global active index, -1 = done; w [T, n] uint8), one segment per slot ->
    (rec int64, segs [S, 2] {start, len}) -- codes_compact(rec_scale=...)'s output for these rows (the order
    inside a segment is unspecified; the fixed-point histograms do not depend on it)."""
    T, n = node.shape
    dev = node.device
    A = len(build_slot)
    bs = np.asarray(build_slot, dtype=np.int32)
    tf_h = np.asarray(tfirst, dtype=np.int64)
    nloc = np.diff(np.concatenate([tf_h, [A]])) if T else np.zeros(0, np.int64)
    max_loc = int(nloc.max()) if T else 0
    if max_loc > NODE_COMPACT_MAX_LOC:
        raise ValueError(f"node_compact holds at most {NODE_COMPACT_MAX_LOC} active nodes per tree, got {max_loc}")
    if not _native(node):
        slot_t = torch.from_numpy(np.concatenate([bs, [-1]]).astype(np.int64))
        # a row of tree t counts when its id is one of tree t's nodes (the kernel's table holds only those)
        lo = torch.from_numpy(tf_h)[:, None]
        own = (node >= lo) & (node < lo + torch.from_numpy(nloc)[:, None])
        ids = torch.where(own, node.long(), torch.full_like(node, A, dtype=torch.int64))
        slot = slot_t[ids]
        flat = slot.reshape(-1)
        keep = torch.nonzero(flat >= 0).flatten()
        order = keep[torch.argsort(flat[keep], stable=True)]
        rows = order % n
        lens = np.bincount(flat[keep].numpy(), minlength=S)[:S].astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) if S else np.zeros(0, np.int64)
        wts = w.reshape(-1)[order].to(torch.int64)
        return rec_encode(rows, wts, _quant(v1[rows], rec_scale, True)), np.stack([starts, lens], 1)
    L = _lib.lib()
    tf, bs_t = upload(dev, tf_h.astype(np.int32), bs)
    v1c = v1.float().contiguous()
    cnt = torch.zeros(max(S, 1), dtype=torch.int32, device=dev)
    _lib.check(L.cdna_node_compact(1, _ptr(node), _ptr(w), n, T, A, _ptr(tf), _ptr(bs_t), _ptr(v1c), _ptr(cnt), None,
                                   float(rec_scale), max_loc, _stream(dev)), "cdna_node_compact(count)")
    lens = cnt.cpu().numpy()[:S].astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) if S else np.zeros(0, np.int64)
    total = int(lens.sum())
    assert total < 2 ** 31
    rec = torch.empty(total + REC_PAD, dtype=torch.int64, device=dev)[:total]  # readable tail
    if total:
        cur, = upload(dev, np.concatenate([starts, [0]]).astype(np.int32))
        _lib.check(L.cdna_node_compact(2, _ptr(node), _ptr(w), n, T, A, _ptr(tf), _ptr(bs_t), _ptr(v1c), _ptr(cur),
                                       _ptr(rec), float(rec_scale), max_loc, _stream(dev)), "cdna_node_compact(scatter)")
    return rec, np.stack([starts, lens], 1)


NODE_COMPACT_MAX_LOC = 1024  # seg.hip kNodeCompactLoc
COMPACT_W = True
# record compaction without a host round trip before the scatter (device segment starts, totals copied back
# behind the scatter kernel)
COMPACT_DEFER = True


# how codes_scatter_w ranks the lanes of one node (seg.hip codes_scatter_w_kernel): 0 = a ballot per node,
# 1 = one DPP prefix scan per 4 nodes (from SCATTER_SCAN_MIN_KB built nodes per tree; KB = 8: 3.54 vs 3.85 ms)
SCATTER_RANK = 1
SCATTER_SCAN_MIN_KB = 4


# waves per tree of the wave-owned compaction (each owns a contiguous row range: per-wave counts, then offsets).
# A/B (round 5): 512 / 1024 / 2048 -> 17.7 / 17.6 / 17.5-17.6 ms at the per-rank shape, 131.2-131.5 vs 129.7-129.8
# ms at the headline for 512 vs 2048
COMPACT_WAVES = 2048
# rows per wave at least (a multiple of 256): small shards keep fewer, longer waves (the per-block node table and
# the per-wave count flush are fixed costs; the queued scatter carries its queue across the wave's trips)
COMPACT_MIN_PER_WAVE = 256


# queued scatter (seg.hip codes_scatter_q_kernel, rank 2): the built row slots queued per wave in LDS and ranked /
# stored in dense groups of 64 (packed records, per_wave <= 65536); identical records to ranks 0 / 1
SCATTER_QUEUE = True
# the queued scatter with its code / label loads one trip ahead (two register sets; rank 3): 120.9 / 120.9 vs
# 121.6 / 121.6 ms per headline step, scatter 7.7 vs ~8.2 ms (profiles/r6/headline_ab.md)
SCATTER_PREFETCH = True


def _scatter_rank(KB: int, rec: bool = False, per_wave: int = 0) -> int:
    if SCATTER_QUEUE and rec and per_wave <= 65536:
        return 3 if SCATTER_PREFETCH else 2
    return 0 if (SCATTER_RANK == 1 and KB < SCATTER_SCAN_MIN_KB) else SCATTER_RANK


def _codes_compact_w(codes, tf_h, bs, tree_of, built, nb_t, kb_need, S, v0, v1, rec_scale=None):
    T, n = codes.shape
    dev = codes.device
    A = len(bs)
    KB = 1
    while KB < kb_need:
        KB *= 2
    # k of each built node inside its tree (slots are numbered tree-major, so slot = first slot of tree + k)
    kmap = np.full(A, -1, dtype=np.int32)
    first_slot = np.zeros(T, dtype=np.int64)
    first_slot[1:] = np.cumsum(nb_t)[:-1]
    kmap[built] = bs[built] - first_slot[tree_of[built]]
    assert np.all(kmap[built] >= 0) and np.all(kmap[built] < KB)
    per_wave = max(COMPACT_MIN_PER_WAVE, -(-n // (COMPACT_WAVES * 256)) * 256)
    Wv = -(-n // per_wave)
    L = _lib.lib()
    tf, kmap_t = upload(dev, tf_h, kmap)
    v1c = v1.float().contiguous()
    v0c = None if v0 is None else v0.float().contiguous()
    wcnt = torch.empty((T, Wv, KB), dtype=torch.int32, device=dev)
    _lib.check(L.cdna_codes_compact_w(1, KB, _ptr(codes), n, T, A, _ptr(tf), _ptr(kmap_t), _ptr(v0c), _ptr(v1c),
                                      per_wave, Wv, _ptr(wcnt), None, None, None, None, None, None, 0.0, None, 0,
                                      _stream(dev)), "cdna_codes_compact_w(count)")
    # per-(tree, node) exclusive scan over the waves in place + node totals, one launch
    tot = torch.empty((T, KB), dtype=torch.int64, device=dev)
    _lib.check(L.cdna_wave_scan(_ptr(wcnt), T, Wv, KB, _ptr(tot), _stream(dev)), "cdna_wave_scan")
    sl = (first_slot[:, None] + np.arange(KB)[None, :])        # slot of (t, k)
    valid = np.arange(KB)[None, :] < nb_t[:, None]
    rec = rec_scale is not None
    if rec and COMPACT_DEFER and n * T < 2 ** 31:
        # No host round trip before the scatter: slots are numbered tree-major with k inside the tree and
        # (t, k) pairs that are not built count 0, so the segment starts are the exclusive prefix of the
        # [T][KB] totals in place -- computed on the device.  The records buffer is sized by the n * T bound
        # (one item per (row, tree)); the totals come back through pinned memory while the scatter runs, and the
        # host builds the segment table (and the caller its histogram work list) behind it instead of idling
        # the GPU for the D2H copy + host work + H2D copy of every level.
        flat = tot.view(-1)
        kstart_t = torch.cumsum(flat, 0) - flat
        tot_p = torch.empty((T, KB), dtype=torch.int64, pin_memory=True)
        tot_p.copy_(tot, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        perm = torch.empty(n * T + REC_PAD, dtype=torch.int64, device=dev)
        _lib.check(L.cdna_codes_compact_w(2, KB, _ptr(codes), n, T, A, _ptr(tf), _ptr(kmap_t), _ptr(v0c), _ptr(v1c),
                                          per_wave, Wv, None, _ptr(wcnt), None, None, None, None, _ptr(perm),
                                          float(rec_scale), _ptr(kstart_t), _scatter_rank(KB, True, per_wave),
                                          _stream(dev)),
                   "cdna_codes_compact_w(scatter)")
        ev.synchronize()
        tot_h = tot_p.numpy()
        lens = np.zeros(S, dtype=np.int64)
        lens[sl[valid]] = tot_h[valid]
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) if S else np.zeros(0, np.int64)
        total = int(lens.sum())
        return perm[:total], None, None, None, np.stack([starts, lens], 1)
    tot_h = tot.cpu().numpy()
    lens = np.zeros(S, dtype=np.int64)
    lens[sl[valid]] = tot_h[valid]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) if S else np.zeros(0, np.int64)
    total = int(lens.sum())
    assert total < 2 ** 31
    if rec:
        perm = torch.empty(total + REC_PAD, dtype=torch.int64, device=dev)[:total]  # readable tail
        v1p = v0p = wp = None
    else:
        perm = torch.empty(total, dtype=torch.int32, device=dev)
        v1p = torch.empty(total, dtype=torch.float32, device=dev)
        v0p = None if v0 is None else torch.empty(total, dtype=torch.float32, device=dev)
        wp = torch.empty(total, dtype=torch.uint8, device=dev)
    if total:
        kstart = np.zeros((T, KB), dtype=np.int64)
        kstart[valid] = starts[sl[valid]]
        kstart_t, = upload(dev, kstart)
        # wcnt now holds the per-wave exclusive offsets; the scatter pass adds each node's segment start
        _lib.check(L.cdna_codes_compact_w(2, KB, _ptr(codes), n, T, A, _ptr(tf), _ptr(kmap_t), _ptr(v0c), _ptr(v1c),
                                          per_wave, Wv, None, _ptr(wcnt), None if rec else _ptr(perm), _ptr(v0p),
                                          _ptr(v1p), _ptr(wp), _ptr(perm) if rec else None,
                                          float(rec_scale) if rec else 0.0, _ptr(kstart_t),
                                          _scatter_rank(KB, rec, per_wave),
                                          _stream(dev)),
                   "cdna_codes_compact_w(scatter)")
    return perm, v0p, v1p, wp, np.stack([starts, lens], 1)


BINS_RM_PAD = True


def bins_row_major(bins: torch.Tensor, pad: Optional[bool] = None) -> torch.Tensor:
    """[G, n, 8] feature-group-major bins -> row-major [n, Gs, 8] copy.

    pad (default on the GPU when G <= 16): Gs = 16, zero-filled, so every row is one aligned 128-byte line
    (a gathered 104-byte row at d = 100 touched ~1.8 lines)."""
    G, n, _ = bins.shape
    if not _native(bins):
        return bins.permute(1, 0, 2).contiguous()
    pad = BINS_RM_PAD if pad is None else pad
    Gs = 16 if (pad and G <= 16) else G
    out = torch.empty((n, Gs, 8), dtype=torch.uint8, device=bins.device)
    _lib.check(_lib.lib().cdna_bins_row_major(_ptr(bins), n, G, Gs, _ptr(out), _stream(bins.device)),
               "cdna_bins_row_major")
    return out


# ------------------------------------------------------------ K6 (split.hip)
# K6 over exact histograms (split_scan(exact=True)) in the wave-parallel kernel: a wave per feature instead of a
# thread walking every bin, the same winner bit for bit (split.hip split_scan_wave_kernel)
SPLIT_WAVE = True


def split_scan(H: torch.Tensor, nthr: torch.Tensor, masks: Optional[torch.Tensor], kind: int, min_inst: float,
               reg_lambda: float = 1.0, gamma: float = 0.0, min_child_weight: float = 1.0,
               missing_bin: bool = False, exact: bool = False):
    """Best split per node of level histograms H [A, d, B, 2] (fp64) -> (out [A, 8], tot [A, 2]).

    out = (gain, feature, bin, left0, left1, right0, right1, missing-goes-right); gain -inf when no legal split.
    kind 0: variance gain on (weight, sum); kind 1: XGBoost gain on (hess, grad).
    exact: every prefix sum of H is exact in fp64 (int64 fixed point at power-of-two scales below 2^53), so the
    wave-parallel kernel's summation order gives the serial kernel's bits (``SPLIT_WAVE``)."""
    A, d, B, k = H.shape
    assert k == 2 and H.dtype == torch.float64 and _native(H)
    Hc = H.contiguous()
    out = torch.empty((A, 8), dtype=torch.float64, device=H.device)
    tot = torch.empty((A, 2), dtype=torch.float64, device=H.device)
    nt = nthr.to(device=H.device, dtype=torch.int32).contiguous()
    m = None if masks is None else masks.to(device=H.device, dtype=torch.int32).contiguous()
    mw = 0 if m is None else m.shape[1]
    kw = kind | (0x100 if (exact and SPLIT_WAVE) else 0)
    _lib.check(_lib.lib().cdna_split_scan(_ptr(Hc), _ptr(nt), _ptr(m), mw, A, d, B, kw, int(missing_bin),
                                          float(min_inst),
                                          float(reg_lambda), float(gamma), float(min_child_weight), _ptr(out),
                                          _ptr(tot), _stream(H.device)), "cdna_split_scan")
    return out, tot


def split_decode(so: torch.Tensor, tot: torch.Tensor, a_tree: torch.Tensor, T: int, min_inst: float,
                 min_gain: float, can_level: bool, leaf_children: bool, missing_bin: bool = False,
                 leaf_values: Optional[tuple] = None, catm: Optional[torch.Tensor] = None,
                 nthr: Optional[torch.Tensor] = None):
    """K6 decisions [A, >= 7] + node totals -> partition tables on the device (split.hip split_decode_kernel):
    split_feat / split_bin / cat_off [A], masks [A, 8] (bin sets of missing-right splits, cat_off[a] = a),
    child [2A], tfirst_next [T] (int32), the host decode's exact twin.

    leaf_values ("xgb" | "variance", lambda): also "lv" [3A] fp32, the leaf values of the rows' destinations at
    this level (children that are leaves, active nodes that do not split) for the partition's margin update.
    catm [A, 8] int32 + nthr [d] int32 (split_scan_ex): winners on categorical features (nthr < 0) split by the
    node's category bitmask (cat_off[a] = a)."""
    A = so.shape[0]
    dev = so.device
    out = torch.empty(15 * A + T, dtype=torch.int32, device=dev)
    sf, sb, co = out[:A], out[A:2 * A], out[2 * A:3 * A]
    child, pref, tfn = out[3 * A:5 * A], out[5 * A:7 * A], out[7 * A:7 * A + T]
    masks = out[7 * A + T:15 * A + T]
    sc, tc = so.contiguous(), tot.contiguous()
    lv = torch.empty(3 * A, dtype=torch.float32, device=dev) if leaf_values is not None else None
    vk, lam = (1 if leaf_values[0] == "xgb" else 0, float(leaf_values[1])) if leaf_values is not None else (0, 0.0)
    _lib.check(_lib.lib().cdna_split_decode(_ptr(sc), sc.shape[1], _ptr(tc), tc.shape[1], _ptr(a_tree), A, T,
                                            float(min_inst), float(min_gain), int(bool(can_level)),
                                            int(bool(leaf_children)), int(bool(missing_bin)), _ptr(sf), _ptr(sb),
                                            _ptr(co), _ptr(masks), _ptr(child), _ptr(pref), _ptr(tfn), _ptr(lv), vk,
                                            lam, _ptr(None if catm is None else catm.contiguous()),
                                            _ptr(None if nthr is None else nthr.contiguous()), _stream(dev)),
               "cdna_split_decode")
    return {"split_feat": sf, "split_bin": sb, "cat_off": co, "masks": masks.view(A, 8), "child": child,
            "tfirst_next": tfn, "lv": lv}


def split_scan_ex(H: torch.Tensor, nthr: torch.Tensor, masks: Optional[torch.Tensor], kind: str, min_inst: float):
    """K6 for classification impurities and categorical features (split.hip split_scan_ex_kernel).

    H [A, d, B, K] fp64; nthr [d] (< 0: categorical); kind 'variance' (K = 2) / 'gini' / 'entropy'.
    Returns (out [A, 4 + 2K] = gain, feature, position, 0, left[K], right[K]; tot [A, K]; catmask [A, 8] int32 =
    the left categories of a categorical winner)."""
    A, d, B, Kc = H.shape
    assert H.dtype == torch.float64 and _native(H)
    out = torch.empty((A, 4 + 2 * Kc), dtype=torch.float64, device=H.device)
    tot = torch.empty((A, Kc), dtype=torch.float64, device=H.device)
    cm = torch.empty((A, 8), dtype=torch.int32, device=H.device)
    nt = nthr.to(device=H.device, dtype=torch.int32).contiguous()
    m = None if masks is None else masks.to(device=H.device, dtype=torch.int32).contiguous()
    mw = 0 if m is None else m.shape[1]
    kd = {"variance": 0, "gini": 2, "entropy": 3}[kind]
    _lib.check(_lib.lib().cdna_split_scan_ex(_ptr(H.contiguous()), _ptr(nt), _ptr(m), mw, A, d, B, Kc, kd,
                                             float(min_inst), _ptr(out), _ptr(tot), _ptr(cm), _stream(H.device)),
               "cdna_split_scan_ex")
    return out, tot, cm


from .relops import (  # noqa: E402,F401  (the relational ops, also reachable as K.<name>)
    _merge_moments, col_moments, partition_dest, compact_mask, gather_cols, bucket_compact, _key_bits,
    _bits_values, hash_dense_ids, dense_ids, dict_encode, HP_OPS, _ptr_array, pack_keys, _excl_scan_n, _hp_shape,
    hash_groups, _la_groups, ordered_to_double, JoinTable, join_table, join_probe, _grouped, group_sum,
    group_first)

from . import tune as _tune  # noqa: E402  (CDNAML_TUNE overrides of the constants above)
_tune.apply(__import__(__name__, fromlist=["_"]))
