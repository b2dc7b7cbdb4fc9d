// K26 aft_step — loss and gradient (or the predictions and quantiles) of Spark's AFTSurvivalRegression (Weibull
// accelerated failure time) in one fp64 pass over the rows.
//
// Per row, with features x, log t, censor delta (1: the event occurred), coefficients beta, intercept b, sigma:
//   eps  = (log t - x.beta - b) / sigma
//   loss = delta log sigma - delta eps + e^eps,   m = (delta - e^eps) / sigma
//   dbeta = m x,   db = m,   dlogsigma = delta + (delta - e^eps) eps
//   predict = exp(x.beta + b),   quantile_p = predict * exp(sigma log(-log(1 - p)))
// The kernel works on the raw rows: the host passes beta already divided by the features' std.
//
// aft_step_kernel<MODE, VW>: 256 threads, 64-row tiles, the next tile of X prefetched in registers, the tile row-major
// fp32 in LDS with the odd row stride kLD (rowblock.h's scaffolding: the row split, the tile and its pipeline).  LDS:
// the tile (33024 B), fp64 coef [128], this tile's m [64], the tile rows' running loss, sum of m and sum of dlogsigma
// [3][64], the quantile factors [16], the rows' bad counts (int [64]): 36480 B, four blocks per CU of 160 KB (the
// registers of the STEP instantiations let three in, see aft_plan).
//   x.beta: the four threads of a row take 32 columns each, in fp64 from the LDS tile, and add their partials with
//     lane shuffles.  Thread q starts its quarter 8 q columns in (and wraps), so the 32 lanes of a half wave (8 rows x
//     4 quarters; row stride 129 = 1 mod 32) read 32 different banks.  The same loop sums x * 0 in fp32: anything but
//     0 there is a non-finite feature.
//   per row: eps, e^eps, the loss term, m and the dlogsigma term in fp64.  A bad row -- a non-finite feature or log t,
//     a censor that is neither 0 nor 1, or a non-finite loss, m or dlogsigma term (e^eps overflowed) -- is counted and
//     adds exactly nothing to any other sum: its three terms become 0 and its four threads zero its tile row, so the
//     gradient never multiplies a NaN by 0.  Rows past the end of the block's range are zeros in the tile and are
//     never read from memory.
//   gradient: thread (column tid & 127, row half tid >> 7) adds m_r x_rc over its 32 rows into one fp64 register for
//     all the block's tiles (a wave reads 64 consecutive floats of a tile row).  At the end the
//     two halves fold through LDS and the block writes [dbeta (d) .. | sum m | sum dlogsigma | loss | bad] to its own
//     workspace slot of kSlot doubles.
//   PREDICT: exp(x.beta + b) per row, and with Q > 0 the [n][Q] quantiles in the same pass (the tile's predictions
//     go through LDS so that the [64][Q] block is written in consecutive doubles).
// aft_reduce_kernel: the slots' sum over the blocks in a fixed order in fp64 (rowblock.h's sum_blocks).  No float
// atomics on global memory: reruns are bit-identical.
// Native range: fp32 rows, d <= 128, Q <= 16, any n, row stride and alignment.
#include <cmath>

#include "rowblock.h"

namespace {

using namespace rowblock;

constexpr int kMaxQ = 16;
// fp64 words of LDS behind the tile: coef [kMaxD], per tile row m, loss, sum of m, sum of dlogsigma; the quantile
// factors [kMaxQ]
constexpr int kRedD = kMaxD + 4 * kRows;
// per block of the workspace: dbeta [kMaxD], sum of m, sum of dlogsigma, loss, bad
constexpr int kSlot = kMaxD + 4;
constexpr size_t kLds = (size_t)kXF * 4 + (size_t)(kRedD + kMaxQ) * 8 + kRows * 4;

enum { kStep = 0, kPredict = 1 };

struct AftParams {
  double b0, sigma, log_sigma;
  int d, Q;
};

// VW = 4: float4 row loads, VW = 1: scalar loads, any layout.
template <int MODE, int VW>
__global__ __launch_bounds__(256) void aft_step_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const double* __restrict__ logt,
    const double* __restrict__ cens, const double* __restrict__ coef, const double* __restrict__ qfac,
    const AftParams pr, double* __restrict__ ws, double* __restrict__ pred, double* __restrict__ quant,
    int64_t rows_per_block) {
  __shared__ __attribute__((aligned(16))) float xb[kXF];
  __shared__ double red[kRedD + kMaxQ];
  __shared__ int cnt[kRows];
  double* cf = red;                 // [kMaxD]
  double* mrow = red + kMaxD;       // [kRows] this tile's m (PREDICT: its predictions)
  double* lsum = mrow + kRows;      // [kRows] running loss of the tile row
  double* msum = lsum + kRows;      // [kRows] running sum of m
  double* ssum = msum + kRows;      // [kRows] running sum of the dlogsigma term
  double* qf = red + kRedD;         // [kMaxQ]
  constexpr bool kTrain = MODE == kStep;
  const int tid = threadIdx.x;
  const int d = pr.d, dv = d / VW, Q = pr.Q;

  for (int i = tid; i < kRedD + kMaxQ; i += 256) {
    double v = 0.0;
    if (i < d) v = coef[i];
    if (i >= kRedD && i - kRedD < Q) v = qfac[i - kRedD];
    red[i] = v;
  }
  if (tid < kRows) cnt[tid] = 0;
  double gacc = 0.0;  // dbeta of column tid & 127 over the row half tid >> 7, summed over the block's tiles

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  const int rr = tid >> 2, qq = tid & 3, bc = tid & (kMaxD - 1), bh = tid >> 7;
  double ltn = 0.0, dln = 0.0;
  // the row's log t and censor travel with its tile
  const auto side = [&](int64_t t, int i) {
    if (kTrain && t + (i >> 2) < rb1) {
      ltn = logt[t + (i >> 2)];
      dln = cens[t + (i >> 2)];
    }
  };
  TileStream<VW> ts;
  ts.begin(xb, kXF, X, ldx, rb0, rb1, dv, tid, side);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    const bool valid = t0 + rr < rb1;
    const double lt = ltn, dl = dln;
    ts.put(xb, tid);
    ts.fetch(t0, tid, side);

    // x.beta, four threads per row, and the features' finiteness
    float* xq = xb + rr * kLD + 32 * qq;
    const double* cq = cf + 32 * qq;
    const bool mine = 32 * qq < d;
    double dot = 0.0;
    float z = 0.f;
    if (mine) {
#pragma unroll 8
      for (int j = 0; j < 32; ++j) {
        const int c = (j + 8 * qq) & 31;
        const float x = xq[c];
        z = fmaf(x, 0.f, z);
        dot = fma((double)x, cq[c], dot);
      }
    }
    dot += __shfl_xor(dot, 1);
    dot += __shfl_xor(dot, 2);
    z += __shfl_xor(z, 1);
    z += __shfl_xor(z, 2);

    if (!kTrain) {
      const double p = exp(dot + pr.b0);
      if (valid && qq == 0) pred[t0 + rr] = p;
      if (Q > 0) {
        if (qq == 0) mrow[rr] = p;
        __syncthreads();
        const int64_t left = rb1 - t0;
        double* qo = quant + t0 * Q;
        for (int e = tid; e < kRows * Q; e += 256) {
          const int r = e / Q;
          if (r < left) qo[e] = mrow[r] * qf[e - r * Q];
        }
      }
      continue;
    }

    // the row's terms in fp64
    {
      const double eps = (lt - dot - pr.b0) / pr.sigma;
      const double ee = exp(eps);
      double loss = dl * pr.log_sigma - dl * eps + ee;
      double mm = (dl - ee) / pr.sigma;
      double ss = dl + (dl - ee) * eps;
      const bool ok = z == 0.f && cdna::finite_d(lt) && (dl == 0.0 || dl == 1.0) && cdna::finite_d(loss) &&
                      cdna::finite_d(mm) && cdna::finite_d(ss);
      const bool bad = valid && !ok;
      if (!valid || !ok) loss = mm = ss = 0.0;
      if (qq == 0) {
        mrow[rr] = mm;
        lsum[rr] += loss;
        msum[rr] += mm;
        ssum[rr] += ss;
        cnt[rr] += bad ? 1 : 0;
      }
      if (bad && mine)
        for (int j = 0; j < 32; ++j) xq[j] = 0.f;
    }
    __syncthreads();  // m complete, bad rows zeroed

    // dbeta_c += sum_r m_r x_rc
    if (bc < d) {
      const float* xc = xb + (32 * bh) * kLD + bc;
      const double* mr = mrow + 32 * bh;
      double c = 0.0;
#pragma unroll 8
      for (int r = 0; r < 32; ++r) c = fma((double)xc[r * kLD], mr[r], c);
      gacc += c;
    }
  }

  if (!kTrain) return;
  __syncthreads();  // the last tile's reads of mrow are done: the upper row half's column sums go over it and lsum
  double a = 0.0, b = 0.0, c = 0.0, e = 0.0;
  if (tid >= 192) {  // wave 3: the 64 tile rows' sums in a fixed order
    const int l = tid - 192;
    a = cdna::wave_sum(msum[l]);
    b = cdna::wave_sum(ssum[l]);
    c = cdna::wave_sum(lsum[l]);
    e = cdna::wave_sum((double)cnt[l]);
  }
  __syncthreads();
  if (tid >= kMaxD) mrow[tid - kMaxD] = gacc;  // [kMaxD] doubles: mrow and lsum
  __syncthreads();
  double* slot = ws + (int64_t)blockIdx.x * kSlot;
  if (tid < d) slot[tid] = gacc + mrow[tid];
  if (tid == 192) {
    slot[kMaxD] = a;
    slot[kMaxD + 1] = b;
    slot[kMaxD + 2] = c;
    slot[kMaxD + 3] = e;
  }
}

// One block of 256 threads per 16 output values: out [d + 4] = [dbeta | sum m | sum dlogsigma | loss | bad].
__global__ __launch_bounds__(256) void aft_reduce_kernel(const double* __restrict__ ws, int nblk, int d,
                                                         double* __restrict__ out) {
  __shared__ double red[16][16];
  const int idx = blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = idx < d + 4;
  const int src = idx < d ? idx : kMaxD + (idx - d);
  const double t = sum_blocks(red, nblk, ok, [&](int b) { return ws[(int64_t)b * kSlot + src]; });
  if (threadIdx.x < 16 && ok) out[idx] = t;
}

struct AftPlan : RowSplit {
  bool native;
};

// One round of resident blocks on the 256 CUs: three per CU by registers (the float4 STEP instantiation holds 142 per
// lane; LDS would let four in); at least 1024 rows per block.
AftPlan aft_plan(int64_t n, int d) {
  AftPlan pl{};
  pl.native = n >= 1 && d >= 1 && d <= kMaxD;
  if (!pl.native) return pl;
  static_cast<RowSplit&>(pl) = split_rows(n, 3 * 256);
  return pl;
}

template <int MODE, int VW>
int step_launch(const AftPlan& pl, const float* X, int64_t n, int64_t ldx, const double* logt, const double* cens,
                const double* coef, const double* qfac, const AftParams& pr, double* ws, double* pred, double* quant,
                hipStream_t st) {
  hipLaunchKernelGGL((aft_step_kernel<MODE, VW>), dim3(pl.nblk), dim3(256), 0, st, X, n, ldx, logt, cens, coef, qfac,
                     pr, ws, pred, quant, pl.rows_per_block);
  return (int)hipGetLastError();
}

}  // namespace

static_assert((size_t)kXF * 4 % 8 == 0, "the fp64 words of LDS start 8-byte aligned");
static_assert(kLds <= 40960, "four blocks per CU");

// What cdna_aft_step runs for these operands (nothing is launched): out = [native, load width (4: float4 rows, 1:
// scalar), blocks, rows per block, LDS bytes, workspace doubles per block].
CDNA_API int cdna_aft_plan(const float* X, int64_t n, int64_t ldx, int d, int64_t* out) {
  const AftPlan pl = aft_plan(n, d);
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (!pl.native || ldx < d) return 0;
  out[0] = 1;
  out[1] = float4_rows(X, d, ldx) ? 4 : 1;
  out[2] = pl.nblk;
  out[3] = pl.rows_per_block;
  out[4] = (int64_t)kLds;
  out[5] = kSlot;
  return 0;
}

// Workspace of a STEP in doubles: one slot per block.
CDNA_API int64_t cdna_aft_step_workspace(int64_t n, int d) {
  const AftPlan pl = aft_plan(n, d);
  return pl.native ? (int64_t)pl.nblk * kSlot : 0;
}

// coef [d] f64 (for the raw rows), b0 the intercept, sigma = exp(log_sigma).
// STEP: logt, cens [n] f64, out [d + 4] f64 = [dbeta | sum m | sum dlogsigma | loss | bad] (un-normalised sums over
// the rows that are not bad, and the number of bad rows), ws: cdna_aft_step_workspace doubles.
// PREDICT: pred [n] f64; Q > 0: qfac [Q] f64 and quant [n][Q] f64 = pred * qfac.
CDNA_API int cdna_aft_step(const float* X, int64_t n, int64_t ldx, const double* logt, const double* cens,
                           const double* coef, double b0, double sigma, double log_sigma, int d, int mode, int Q,
                           const double* qfac, double* out, double* ws, double* pred, double* quant,
                           hipStream_t st) {
  const AftPlan pl = aft_plan(n, d);
  if (!pl.native || ldx < d || X == nullptr || coef == nullptr) return (int)hipErrorInvalidValue;
  if (mode != kStep && mode != kPredict) return (int)hipErrorInvalidValue;
  if (mode == kStep && (logt == nullptr || cens == nullptr || out == nullptr || ws == nullptr))
    return (int)hipErrorInvalidValue;
  if (mode == kPredict && (pred == nullptr || Q < 0 || Q > kMaxQ || (Q > 0 && (qfac == nullptr || quant == nullptr))))
    return (int)hipErrorInvalidValue;
  const AftParams pr{b0, sigma, log_sigma, d, mode == kPredict ? Q : 0};
  const bool vec = float4_rows(X, d, ldx);
  int rc;
  if (mode == kStep)
    rc = vec ? step_launch<kStep, 4>(pl, X, n, ldx, logt, cens, coef, qfac, pr, ws, pred, quant, st)
             : step_launch<kStep, 1>(pl, X, n, ldx, logt, cens, coef, qfac, pr, ws, pred, quant, st);
  else
    rc = vec ? step_launch<kPredict, 4>(pl, X, n, ldx, logt, cens, coef, qfac, pr, ws, pred, quant, st)
             : step_launch<kPredict, 1>(pl, X, n, ldx, logt, cens, coef, qfac, pr, ws, pred, quant, st);
  if (rc != 0 || mode == kPredict) return rc;
  hipLaunchKernelGGL(aft_reduce_kernel, dim3((unsigned)((d + 4 + 15) / 16)), dim3(256), 0, st, ws, pl.nblk, d, out);
  return (int)hipGetLastError();
}
