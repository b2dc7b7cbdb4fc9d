"""K23 ``gmm_step`` on the device against the numpy reference of ``tests/_gmm_refs.py`` within the bounds that
module derives from the inputs, and a GaussianMixture fitted end to end on the GPU against the CPU fit.

Shapes are the smallest at which the kernels can go wrong: a single row, the 64-row tile edge with d % 4 != 0 (the
scalar-load variant), one feature, the benchmark's d = 100 and k = 8, many blocks with a ragged last tile, the d and
k caps, strided rows (one float4-addressable, one not), zero weights, a 65..96-wide moment matrix (two tile pairs per
wave) with either kind of load.  Every test prints its observed error / bound
ratios before it asserts (``-s`` shows them; profiles/r10/gmm.md records a run).

End to end (``test_fit_on_device_matches_cpu``): 20000 x 20, k = 3, both fits on fp32 rows from the same seed.  The
bounds are four times the difference between an fp32 run and the fp64 run of the numpy reference EM on the same
data -- a property of the reference arithmetic, computed in the test with ``_gmm_refs.ref_em``: logLikelihood
1.08e-3 (of -6.0e5), weights 1.10e-8, means 2.53e-7, covariances 1.76e-6 (largest entry 8.5).  The fp32 run rounds
centres, matrices and scaled rows as the op defines AND forms the two products as numpy fp32 matmuls
(``ref_em(..., sgemm=True)``): the rounding of the products is the one difference between the device and the CPU
fit, so a run that forms them exactly (logLikelihood 5.62e-4, weights 2.94e-10, means 4.49e-8, covariances
1.12e-7) measures only the rounding of the operands, which the two fits share bit for bit.  EM's first iterations,
where the components still overlap, amplify either perturbation some 50 times.  ``tol`` is 0.04 so that the stopping
decision is far from its threshold: on the reference trace every change of the log-likelihood before the last is
above 0.7 (18 x tol) and the last is 2.0e-3 (tol / 19); the test asserts both at 10 x.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from cdnaml.ops import _lib, kernels as K
from tests import _gmm_refs as G
from tests.conftest import session_device
from tests.test_gmm_cpu import check_against_ref, params, tt

pytestmark = pytest.mark.gpu

# (n, d, k, ldx or None, zero weights)
SHAPES = [(1, 4, 2, None, False), (63, 3, 2, None, False), (64, 3, 2, None, False), (65, 3, 2, None, False),
          (200, 1, 2, None, False), (5000, 100, 8, None, False), (70001, 126, 4, None, False),
          (3000, 127, 3, None, False), (4096, 20, 32, None, False), (9000, 100, 8, 101, False),
          (5000, 100, 8, 104, False), (4096, 30, 5, None, True),
          # 65 <= d + 1 <= 96: 6 tile pairs, the moment kernels with two tile pairs per wave (float4 and scalar loads)
          (4097, 64, 3, None, False), (1500, 66, 2, None, True)]


class Counting:
    """test_glm_gpu's counting wrapper around ``_lib.check``: the native entry points a block of code called."""

    def __enter__(self):
        self.calls = []
        self.orig = _lib.check

        def counting(code, name):
            self.calls.append(name)
            return self.orig(code, name)
        _lib.check = counting
        return self.calls

    def __exit__(self, *exc):
        _lib.check = self.orig


def on_device(dev, X, w, mu, A, logc):
    base = X.base if X.base is not None else X
    Xd = torch.empty(base.shape, dtype=tt(base).dtype, device=dev)[:, :X.shape[1]]   # keeps the row stride
    Xd.copy_(tt(X))
    return (Xd,) + tuple(None if a is None else tt(a).to(dev) for a in (w, mu, A, logc))


def run_all_modes(dev, inputs):
    """STEP, PREDICT and EVAL twice each: the outputs on the host, the native calls, and bit-identity of reruns."""
    args = on_device(dev, *inputs)
    with Counting() as calls:
        S, st = K.gmm_step(*args, K.GMM_STEP)
        S2, st2 = K.gmm_step(*args, K.GMM_STEP)
        R, a, st_p = K.gmm_step(*args, K.GMM_PREDICT)
        R2, a2, _ = K.gmm_step(*args, K.GMM_PREDICT)
        st_e = K.gmm_step(*args, K.GMM_EVAL)
    return dict(S=S, S2=S2, st=st, st2=st2, R=R, R2=R2, a=a, a2=a2, st_p=st_p, st_e=st_e), calls


def report(tag, ref, out):
    Sr, dS = ref.moments()
    g = ref.good
    r_ratio = (np.abs(out["R"].cpu().numpy()[g] - ref.R[g]).max(1) / np.maximum(ref.dr[g], 1e-300)).max() if g.any() \
        else 0.0
    print(f"gmm {tag}: observed / bound  R {r_ratio:.3e}  S {(np.abs(out['S'].cpu().numpy() - Sr) / dS).max():.3e}  "
          f"sum w log s {abs(out['st'][0].item() - ref.stats[0]) / ref.dstats0:.3e}")


@pytest.mark.parametrize("n,d,k,ldx,zero_w", SHAPES)
def test_device_matches_reference(gpu_device, n, d, k, ldx, zero_w):
    ref = G.ref_for(n, d, k, ldx, zero_w)
    out, calls = run_all_modes(gpu_device, G.make_inputs(n, d, k, ldx, zero_w))
    assert calls == ["cdna_gmm_step"] * 5, calls
    # no float atomics: the same bits twice, in every mode
    assert torch.equal(out["S"], out["S2"]) and torch.equal(out["st"], out["st2"])
    assert torch.equal(out["R"], out["R2"]) and torch.equal(out["a"], out["a2"])
    assert torch.equal(out["st"], out["st_p"]) and torch.equal(out["st"], out["st_e"])
    report(f"{n}x{d} k={k} ldx={ldx} zero_w={zero_w}", ref, out)
    S = out["S"].cpu().numpy()
    assert np.array_equal(S, S.transpose(0, 2, 1))
    check_against_ref(ref, S, out["R"].cpu().numpy(), out["a"].cpu().numpy(), out["st"].cpu().numpy())


def test_device_far_row_and_nan_row(gpu_device):
    n, d, k = 300, 5, 3
    X, w, mu, A, logc = G.make_inputs(n, d, k)
    X = X.copy()
    X[11] = 1e3
    X[257, 2] = np.nan
    X[130, 4] = np.inf
    ref = G.Ref(X, w, mu, A, logc)
    assert ref.bad.sum() == 2
    out, calls = run_all_modes(gpu_device, (X, w, mu, A, logc))
    assert calls == ["cdna_gmm_step"] * 5
    assert out["st"][2].item() == 2 and torch.isfinite(out["S"]).all()
    assert np.array_equal(out["R"][11].cpu().numpy(), np.full(k, 1.0 / k)) and out["a"][11].item() == 0
    check_against_ref(ref, out["S"].cpu().numpy(), out["R"].cpu().numpy(), out["a"].cpu().numpy(),
                      out["st"].cpu().numpy())


@pytest.mark.parametrize("n,d,k,f64", [(300, 128, 3, False), (300, 8, 33, False), (300, 7, 3, True)])
def test_outside_the_native_range_takes_the_host_formulation(gpu_device, n, d, k, f64):
    assert d > K.GMM_MAX_D or k > K.GMM_MAX_K or f64
    ref = G.ref_for(n, d, k, None, False, f64)
    out, calls = run_all_modes(gpu_device, G.make_inputs(n, d, k, None, False, f64))
    assert not [c for c in calls if c.startswith("cdna_gmm")], calls
    report(f"{n}x{d} k={k} f64={f64} (host formulation on the device)", ref, out)
    check_against_ref(ref, out["S"].cpu().numpy(), out["R"].cpu().numpy(), out["a"].cpu().numpy(),
                      out["st"].cpu().numpy())


# ------------------------------------------------------------------------------------------------ end to end
E2E_TOL = 0.04


def _fit(device, tmp_path, pdf, names, seed):
    import cdnaml
    from cdnaml.ml.clustering import GaussianMixture
    from cdnaml.ml.feature import VectorAssembler
    with session_device(device):
        spark = cdnaml.SparkSession.builder.config("cdnaml.warehouse.dir", str(tmp_path / f"wh_{device}")) \
            .getOrCreate()
        spark.conf.set("cdnaml.ml.vectorPrecision", "fp32")
        try:
            with Counting() as calls:
                df = VectorAssembler(inputCols=names, outputCol="features").transform(spark.createDataFrame(pdf))
                m0 = GaussianMixture(k=3, seed=seed, maxIter=0).fit(df)
                m = GaussianMixture(k=3, seed=seed, tol=E2E_TOL).fit(df)
                pred = m.transform(df).select("prediction").toPandas().prediction.to_numpy()
            out = (params(m0), params(m), m.summary.numIter, m.summary.logLikelihood, pred)
        finally:
            spark.conf.set("cdnaml.ml.vectorPrecision", "auto")
            spark.stop()
    return out, calls


def test_fit_on_device_matches_cpu(gpu_device, tmp_path):
    n, d, k = 20000, 20, 3
    X = G.overlapping_data(n, d, k, seed=33, sep=12.0)
    names = [f"x{i}" for i in range(d)]
    pdf = pd.DataFrame(X, columns=names)
    (i_g, p_g, it_g, ll_g, pred_g), calls = _fit("cuda", tmp_path, pdf, names, 12)
    (i_c, p_c, it_c, ll_c, pred_c), _ = _fit("cpu", tmp_path, pdf, names, 12)
    for a, b in zip(i_g, i_c):
        assert np.array_equal(a, b)                      # the same initial state on both devices
    # one STEP per iteration, EVAL for maxIter = 0, PREDICT for each summary and for transform
    assert calls.count("cdna_gmm_step") >= it_g + 4, calls
    r64 = G.ref_em(X, None, *i_c, E2E_TOL, 100)
    r32 = G.ref_em(X.astype(np.float32), None, *i_c, E2E_TOL, 100, sgemm=True)
    trace = r64[3]
    # fp32-run vs fp64-run difference of the numpy reference EM on this data (figures in the module docstring)
    ref_gap = {"logLikelihood": abs(r32[3][-1] - trace[-1])}
    ref_gap.update({name: np.abs(a - b).max() for name, a, b in zip(("weights", "means", "covs"), r32, r64)})
    dl = np.abs(np.diff(trace))
    assert dl[-1] <= E2E_TOL / 10 and (dl[:-1] >= 10 * E2E_TOL).all(), dl
    gaps = {"logLikelihood": abs(ll_g - ll_c)}
    gaps.update({name: np.abs(a - b).max() for name, a, b in zip(("weights", "means", "covs"), p_g, p_c)})
    print("gmm e2e: iterations", it_g, it_c, len(trace),
          " device vs cpu / 4 x reference gap:",
          {name: f"{v:.3e} / {4 * ref_gap[name]:.3e}" for name, v in gaps.items()})
    assert it_g == it_c == len(trace)
    # the device's predictions are the CPU's, apart from rows inside the dr bound of the final model
    ref = G.Ref(X.astype(np.float32), None, p_c[1], *G.tables(*p_c))
    sure = ref.top2_gap() > 2 * ref.dr
    assert sure.mean() > 0.9 and np.array_equal(pred_g[sure], pred_c[sure])
    for name, v in gaps.items():
        assert v <= 4 * ref_gap[name], (name, v, 4 * ref_gap[name])
