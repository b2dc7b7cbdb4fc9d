"""Plain numpy references for ``K.gmm_step`` (K23) and for the whole EM loop of ``GaussianMixture``, the derived
error bounds of the fp32 path, and the makers of the inputs the CPU and GPU tests share.

Nothing here imports ``cdnaml.ops.kernels``: the references work from the exact stored inputs and from the op's
written definition (Spark's formulas; for fp32 rows: centres and matrices rounded to fp32, t the fp32 difference,
the constant A_j (mu_j - c_j) subtracted, the scaled row rounded to fp32 before the moment product).

Arithmetic of the references: the two matrix products run in fp64 BLAS (every product of two fp32 values is exact in
fp64 and the length-d sums carry d 2^-53, nine orders below the fp32 bounds; a ``np.longdouble`` matmul has no BLAS
and would take minutes at 70001 x 126); everything per row from q on (exp, sums over the components, log, the
division) runs in ``np.longdouble`` where the platform has one wider than fp64.

Bounds (``Ref.dlogp``, ``Ref.dr``, ``Ref.dstats0``, ``Ref.moments``), all computed from the inputs, none chosen by
looking at an implementation's error.  The only difference between an implementation of the fp32 definition and
this reference is the fp32 ``fmaf`` chain of the two products (the MFMA is bitwise an fmaf chain; a host sgemm obeys
the same bound):
    |dy|     <= gamma_d (|T| |A_j|^T),  gamma_d = d u / (1 - d u),  u = 2^-24        (fp64 rows: u = 2^-53)
    |dq|     <= sum_c (2 |y| |dy| + dy^2)
    |dlogp|  <= |dq| / 2 + 2^-50 (|logc| + q / 2 + 1)          the fp64 evaluation of the exponent and of exp
    |dr|     <= frac expm1(2 max_j |dlogp_j|),  frac = max_j g_j / (EPS + g_j) <= 1,  g_j = exp(logp_j)
    |dS_ab|  <= 1e-5 |S_ab| + 1e-3 sqrt(n) max w + sum_rows w |dr| |z_a z_b|,  z = [t | 1]
               (the first two terms are test_gram_f32's bound for the exact-fp32 MFMA Gram with fp32 block sums)
    |d sum w log s| <= sum_rows w max_j |dlogp_j| + 1e-12 sum_rows w |log s|
"""
import functools

import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble


class Ref:
    """The op's outputs on one input, in the reference arithmetic, with the ingredients of the bounds."""

    def __init__(self, X, w, mu, A, logc, sgemm=False):
        """``sgemm``: for fp32 rows, run the two products as numpy fp32 matmuls (fp32 accumulation) instead of
        exactly -- an fp32 RUN of the reference, used only to measure how far fp32 arithmetic moves a whole fit."""
        n, d = X.shape
        k = mu.shape[0]
        f32 = X.dtype == np.float32
        self.n, self.d, self.k, self.f32, self.sgemm = n, d, k, f32, sgemm and f32
        ww = np.ones(n) if w is None else np.asarray(w, np.float64)
        c = mu.astype(np.float32).astype(np.float64) if f32 else mu
        Ar = A.astype(np.float32).astype(np.float64) if f32 else A
        u = 2.0 ** -24 if f32 else 2.0 ** -53
        gam = d * u / (1 - d * u)
        q = np.empty((n, k))
        dq = np.empty((n, k))
        self.t = []
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(k):
                t = (X - c[j].astype(np.float32)).astype(np.float64) if f32 else X - c[j]
                ty = t @ Ar[j].T if not self.sgemm else \
                    (t.astype(np.float32) @ Ar[j].T.astype(np.float32)).astype(np.float64)
                y = ty - Ar[j] @ (mu[j] - c[j])
                dy = gam * (np.abs(t) @ np.abs(Ar[j]).T)
                q[:, j] = (y * y).sum(1)
                dq[:, j] = (2 * np.abs(y) * dy + dy * dy).sum(1)
                self.t.append(t)
            self.bad = ~np.isfinite(q).all(1)
            good = ~self.bad
            e = logc.astype(LD) - q.astype(LD) / 2
            p = EPS + np.exp(e)
            s = p.sum(1)
            r = p / s[:, None]
            self.q, self.logp = q, np.asarray(e, np.float64)
            self.dlogp = dq / 2 + 2.0 ** -50 * (np.abs(logc) + q / 2 + 1)
            # per row, absolute (r <= 1).  p_j = EPS + g_j and only g_j = exp(.) carries the error: the relative
            # error of p_j is that of g_j times g_j / p_j <= frac, so (1 + frac a) / (1 - frac b) - 1 <=
            # frac (e^(2 delta) - 1) with a = e^delta - 1, b = 1 - e^-delta.  A row whose densities all underflow
            # has frac = 0: its uniform r is exact.  Left-out rows carry no bound (they are not compared).
            g = np.exp(e + self.dlogp)
            frac = np.asarray((g / (EPS + g)).max(1), np.float64)
            big = np.expm1(np.minimum(2 * self.dlogp.max(1), 700.0))
            self.dr = np.where(self.bad, 0.0, np.minimum(1.0, np.where(frac > 0, frac * big, 0.0)))
            self.R = np.where(self.bad[:, None], np.nan, np.asarray(r, np.float64))
            self.assign = np.where(self.bad, 0, np.argmax(np.where(self.bad[:, None], 0.0, self.R), 1)).astype(np.int32)
            logs = np.asarray(np.log(s), np.float64)
            self.stats = np.array([float((ww[good].astype(LD) * np.log(s[good])).sum()), float(ww[good].sum()),
                                   float(self.bad.sum())])
            self.dstats0 = float((ww[good] * self.dlogp[good].max(1)).sum()
                                 + 1e-12 * (ww[good] * np.abs(logs[good])).sum())
        self.w, self.good = ww, good
        self._S = None

    def top2_gap(self):
        srt = np.sort(np.where(self.bad[:, None], 0.0, self.R), 1)
        return srt[:, -1] - srt[:, -2]

    def moments(self):
        """(S [k, d+1, d+1], its bound) -- computed on demand, once."""
        if self._S is None:
            n, d, k = self.n, self.d, self.k
            S = np.zeros((k, d + 1, d + 1))
            dS = np.zeros_like(S)
            wmax = float(self.w.max()) if n else 0.0
            for j in range(k):
                sr = np.sqrt(np.where(self.good, self.w * np.nan_to_num(self.R[:, j]), 0.0))
                z = np.concatenate([np.nan_to_num(self.t[j], nan=0.0, posinf=0.0, neginf=0.0), np.ones((n, 1))], 1)
                z[~self.good] = 0.0
                if self.f32:
                    sr = sr.astype(np.float32)
                    zs = np.where(sr[:, None] != 0, z.astype(np.float32) * sr[:, None], np.float32(0))
                    zs = zs if self.sgemm else zs.astype(np.float64)
                else:
                    zs = z * sr[:, None]
                S[j] = zs.T @ zs                              # an fp32 matmul when sgemm
                za = np.abs(z)
                dS[j] = 1e-5 * np.abs(S[j]) + 1e-3 * np.sqrt(n) * wmax + (za * (self.w * self.dr)[:, None]).T @ za
            self._S = (S, dS)
        return self._S

    def overlap_ok(self):
        """The condition every test asserts on its data: at least a quarter of the rows have their largest
        responsibility below 0.9 (saturated responsibilities would test nothing of r)."""
        return (np.nanmax(self.R[self.good], 1) < 0.9).mean() >= 0.25


# ------------------------------------------------------------------------------------------ mixture parameters
def tables(weights, means, covs):
    """(A, logc) from the mixture's parameters with Spark's pseudo-inverse rule: eigenvalues <= EPS d max are
    dropped; ValueError if none is left."""
    k, d = means.shape
    A = np.zeros((k, d, d))
    logc = np.zeros(k)
    for j in range(k):
        vals, vecs = np.linalg.eigh(covs[j])
        keep = vals > EPS * d * vals.max()
        if not keep.any():
            raise ValueError("no non-zero singular values")
        A[j, :keep.sum()] = (vecs[:, keep] / np.sqrt(vals[keep])).T
        logc[j] = np.log(weights[j]) - 0.5 * (d * np.log(2 * np.pi) + np.log(vals[keep]).sum())
    return A, logc


def ref_em(X, w, weights, means, covs, tol, max_iter, sgemm=False):
    """Spark's EM loop from a given initial state on the reference op: (weights, means, covs, logLik trace)."""
    f32 = X.dtype == np.float32
    d = X.shape[1]
    trace = []
    ll, prev, it = -np.finfo(np.float64).max, 0.0, 0
    while it < max_iter and not abs(ll - prev) < tol:
        A, logc = tables(weights, means, covs)
        ref = Ref(X, w, means, A, logc, sgemm)
        S = ref.moments()[0]
        c = means.astype(np.float32).astype(np.float64) if f32 else means
        N = S[:, d, d]
        delta = S[:, :d, d] / N[:, None]
        means = c + delta
        covs = S[:, :d, :d] / N[:, None, None] - delta[:, :, None] * delta[:, None, :]
        weights = N / N.sum()
        prev, ll = ll, float(ref.stats[0])
        trace.append(ll)
        it += 1
    return weights, means, covs, trace


# ------------------------------------------------------------------------------------------------ input makers
@functools.lru_cache(maxsize=None)
def make_inputs(n, d, k, ldx=None, zero_w=False, f64=False):
    """(X [n, d] (a view of an [n, ldx] array when ldx is given), w or None, mu, A, logc): rows drawn from k
    overlapping Gaussians -- means about one Mahalanobis unit apart, covariances equal up to a few per cent --
    and the parameters of a nearby mixture (the generating one, perturbed), with A_j the inverse Cholesky factor."""
    rng = np.random.default_rng(7919 * d + 31 * k + n % 1009)
    # column sd 0.1 .. 0.25: the densities stay far above the EPS Spark adds to them, also at d = 127
    scale = rng.uniform(0.1, 0.25, d)
    L0 = (np.eye(d) + 0.3 / np.sqrt(d) * np.tril(rng.standard_normal((d, d)), -1)) * scale[:, None]
    base = 0.5 * rng.standard_normal(d)
    base[0] = 37.77                                   # a latitude-like column: mean far from 0
    L = np.stack([L0 * (1.0 + 0.04 * j / k) for j in range(k)])
    means = base + np.einsum("ab,jb->ja", L0, 0.7 / np.sqrt(d) * rng.standard_normal((k, d)))
    comp = rng.integers(k, size=n)
    Xf = means[comp] + np.einsum("nab,nb->na", L[comp], rng.standard_normal((n, d))) if n * d * d < 5e7 else \
        means[comp] + (rng.standard_normal((n, d)) @ L0.T) * (1.0 + 0.04 * comp / k)[:, None]
    buf = np.zeros((n, ldx or d), dtype=np.float64 if f64 else np.float32)
    buf[:, :d] = Xf
    X = buf[:, :d]
    w = None
    if zero_w:
        w = rng.uniform(0.5, 2.0, n)
        w[rng.uniform(size=n) < 0.1] = 0.0
    pi = rng.dirichlet(np.full(k, 20.0))
    mu = means + 0.05 / np.sqrt(d) * np.einsum("ab,jb->ja", L0, rng.standard_normal((k, d)))
    A = np.stack([np.linalg.inv(L[j]) for j in range(k)])
    logc = np.log(pi) - 0.5 * (d * np.log(2 * np.pi) + 2 * np.log(np.abs(np.diagonal(L, axis1=1, axis2=2))).sum(1))
    return X, w, mu, A, logc


@functools.lru_cache(maxsize=None)
def ref_for(n, d, k, ldx=None, zero_w=False, f64=False):
    return Ref(*make_inputs(n, d, k, ldx, zero_w, f64))


def separated_data(n, d, k, seed, sep=8.0):
    """Well-separated spherical-ish components for whole-fit tests: fp32-representable fp64 rows."""
    rng = np.random.default_rng(seed)
    centres = sep * rng.standard_normal((k, d))
    comp = rng.integers(k, size=n)
    X = centres[comp] + rng.standard_normal((n, d)) * rng.uniform(0.7, 1.3, (k, d))[comp]
    return X.astype(np.float32).astype(np.float64)


def overlapping_data(n, d, k, seed, sep=3.0):
    """Overlapping components (centres about ``sep`` sd apart) for whole-fit tests: EM takes tens of iterations."""
    rng = np.random.default_rng(seed)
    centres = sep / np.sqrt(2 * d) * rng.standard_normal((k, d))
    comp = rng.integers(k, size=n)
    X = centres[comp] + rng.standard_normal((n, d)) * rng.uniform(0.7, 1.3, (k, d))[comp]
    return X.astype(np.float32).astype(np.float64)
