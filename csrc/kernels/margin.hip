// K32 margin_step — loss and gradient (or the margins) of the linear models with one margin per row, LinearSVC's
// squared hinge and LinearRegression's Huber loss, in one fp64 pass over the rows.
//
// Per row, with features x, label y, weight w, coefficients coef, intercept b:  m = x.coef + b, and a top chosen by
// LOSS gives the row's loss term, u = d loss / d m and (Huber) v = d loss / d sigma:
//   SQUARED_HINGE (labels 0 / 1):  s = 2 y - 1, t = 1 - s m;  t > 0: loss = w t^2, u = -2 w s t;  otherwise both are 0
//     (t == 0 exactly is inactive).
//   HUBER (Spark's HuberAggregator, scale sigma, shape epsilon):  r = y - m;
//     |r| <= epsilon sigma:  loss = w (sigma + r^2 / sigma) / 2,  u = -w r / sigma,  v = w (1 - (r / sigma)^2) / 2
//     otherwise:  loss = w (sigma + 2 epsilon |r| - sigma epsilon^2) / 2,  u = -w epsilon sign(r),
//                 v = w (1 - epsilon^2) / 2              (|r| == epsilon sigma takes the quadratic branch)
//   dcoef = sum u x,  db = sum u,  dsigma = sum v.
// The kernel works on the raw rows: the host passes coef already divided by the features' std where the model
// standardises.
//
// margin_step_kernel<LOSS, MODE, VW>: 256 threads, 64-row tiles, the next tile of X prefetched in registers, the tile
// row-major fp32 in LDS with the odd row stride kLD (rowblock.h's scaffolding: the row split, the tile and its
// pipeline).  LDS: the tile (33024 B), fp64 coef [128], this tile's u [64], the tile rows' running loss, sum of u, sum
// of v and sum of w [4][64], the rows' bad counts (int [64]): 36864 B.
//   x.coef: the four threads of a row take 32 columns each, in fp64 from the LDS tile, and add their partials with
//     lane shuffles.  Thread q starts its quarter 8 q columns in (and wraps), so the 32 lanes of a half wave (8 rows x
//     4 quarters; row stride 129 = 1 mod 32) read 32 different banks.  The same loop sums x * 0 in fp32: anything but
//     0 there is a non-finite feature.
//   per row: the top in fp64, all vector arithmetic, no transcendental: the kernel is a streaming pass with a few
//     dozen fp64 operations per row on top of the two products.  A bad row -- a non-finite feature or weight, a label
//     that is not 0 or 1 (hinge) or not finite (Huber), or a loss, u or v term that is not finite -- is counted and
//     adds exactly nothing to any other sum: its terms become 0 by selection and its four threads zero its tile row,
//     so the gradient never multiplies a NaN by 0.  Rows past the end of the block's range are zeros in the tile and
//     are never read from memory.  The row's label and weight are loaded with its tile (TileStream's side callback).
//   gradient: thread (column tid & 127, row half tid >> 7) adds u_r x_rc over its 32 rows into one fp64 register for
//     all the block's tiles (a wave reads 64 consecutive floats of a tile row).  At the end the two halves fold
//     through LDS and the block writes [dcoef (d) .. | sum u | sum v | loss | sum w | bad] to its own workspace slot
//     of kSlot doubles.
//   PREDICT: m per row, [n] fp64.
// margin_reduce_kernel: the slots' sum over the blocks in a fixed order in fp64 (rowblock.h's sum_blocks).  No float
// atomics on global memory: reruns are bit-identical.
// Native range: fp32 rows, d <= 128, any n, row stride and alignment.
#include <cmath>

#include "rowblock.h"

namespace {

using namespace rowblock;

// fp64 words of LDS behind the tile: coef [kMaxD], per tile row u, loss, sum of u, sum of v, sum of w
constexpr int kRedD = kMaxD + 5 * kRows;
// per block of the workspace: dcoef [kMaxD], sum of u, sum of v, loss, sum of w, bad
constexpr int kTail = 5;
constexpr int kSlot = kMaxD + kTail;
constexpr size_t kLds = (size_t)kXF * 4 + (size_t)kRedD * 8 + kRows * 4;
// resident blocks per CU the row split counts on: by LDS (160 KB) four fit; the registers of the float4
// instantiations (at most 124 per lane) let four in, those of the scalar-load ones (255) two (profiles/r24/margin.md)
constexpr int kPerCuLds = 4;
constexpr int per_cu(bool vec) { return vec ? kPerCuLds : 2; }

enum { kStep = 0, kPredict = 1 };
enum { kSquaredHinge = 0, kHuber = 1 };

struct MarginParams {
  double b0, sigma, eps;
  int d;
};

// the row's loss term, u = d loss / d m and v = d loss / d sigma; `lab`: the label is one the loss takes
template <int LOSS>
__device__ __forceinline__ void margin_top(double m, double y, double w, const MarginParams& pr, double& loss,
                                           double& u, double& v, bool& lab) {
  if (LOSS == kSquaredHinge) {
    const double s = 2.0 * y - 1.0, t = 1.0 - s * m;
    const bool act = !(t <= 0.0);  // a NaN margin is active: its terms are NaN and the row is bad
    loss = act ? w * t * t : 0.0;
    u = act ? -2.0 * w * s * t : 0.0;
    v = 0.0;
    lab = y == 0.0 || y == 1.0;
  } else {
    const double r = y - m, a = fabs(r), q = r / pr.sigma;
    const bool quad = a <= pr.eps * pr.sigma;
    loss = 0.5 * w * (quad ? pr.sigma + r * q : pr.sigma + 2.0 * pr.eps * a - pr.sigma * pr.eps * pr.eps);
    u = quad ? -w * q : (r < 0.0 ? w * pr.eps : -w * pr.eps);
    v = 0.5 * w * (quad ? 1.0 - q * q : 1.0 - pr.eps * pr.eps);
    lab = cdna::finite_d(y);
  }
}

// VW = 4: float4 row loads, VW = 1: scalar loads, any layout.
template <int LOSS, int MODE, int VW>
__global__ __launch_bounds__(256) void margin_step_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const double* __restrict__ y, const double* __restrict__ wt,
    const double* __restrict__ coef, const MarginParams pr, double* __restrict__ ws, double* __restrict__ marg,
    int64_t rows_per_block) {
  __shared__ __attribute__((aligned(16))) float xb[kXF];
  __shared__ double red[kRedD];
  __shared__ int cnt[kRows];
  double* cf = red;               // [kMaxD]
  double* urow = red + kMaxD;     // [kRows] this tile's u
  double* lsum = urow + kRows;    // [kRows] running loss of the tile row
  double* usum = lsum + kRows;    // [kRows] running sum of u
  double* vsum = usum + kRows;    // [kRows] running sum of v
  double* wsum = vsum + kRows;    // [kRows] running sum of w
  constexpr bool kTrain = MODE == kStep;
  const int tid = threadIdx.x;
  const int d = pr.d, dv = d / VW;

  for (int i = tid; i < kRedD; i += 256) red[i] = i < d ? coef[i] : 0.0;
  if (tid < kRows) cnt[tid] = 0;
  double gacc = 0.0;  // dcoef of column tid & 127 over the row half tid >> 7, summed over the block's tiles

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  const int rr = tid >> 2, qq = tid & 3, bc = tid & (kMaxD - 1), bh = tid >> 7;
  double yn = 0.0, wn = 1.0;
  // the row's label and weight travel with its tile
  const auto side = [&](int64_t t, int i) {
    if (kTrain && t + (i >> 2) < rb1) {
      yn = y[t + (i >> 2)];
      wn = wt != nullptr ? wt[t + (i >> 2)] : 1.0;
    }
  };
  TileStream<VW> ts;
  ts.begin(xb, kXF, X, ldx, rb0, rb1, dv, tid, side);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    const bool valid = t0 + rr < rb1;
    const double yy = yn, ww = wn;
    ts.put(xb, tid);
    ts.fetch(t0, tid, side);

    // x.coef, four threads per row, and the features' finiteness
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
    const double m = dot + pr.b0;

    if (!kTrain) {
      if (valid && qq == 0) marg[t0 + rr] = m;
      continue;
    }

    // the row's terms in fp64
    {
      double loss, u, v;
      bool lab;
      margin_top<LOSS>(m, yy, ww, pr, loss, u, v, lab);
      const bool ok = z == 0.f && lab && cdna::finite_d(ww) && cdna::finite_d(loss) && cdna::finite_d(u) &&
                      cdna::finite_d(v);
      const bool bad = valid && !ok;
      const bool use = valid && ok;
      if (qq == 0) {
        urow[rr] = use ? u : 0.0;
        lsum[rr] += use ? loss : 0.0;
        usum[rr] += use ? u : 0.0;
        if (LOSS == kHuber) vsum[rr] += use ? v : 0.0;
        wsum[rr] += use ? ww : 0.0;
        cnt[rr] += bad ? 1 : 0;
      }
      if (bad && mine)
        for (int j = 0; j < 32; ++j) xq[j] = 0.f;
    }
    __syncthreads();  // u complete, bad rows zeroed

    // dcoef_c += sum_r u_r x_rc
    if (bc < d) {
      const float* xc = xb + (32 * bh) * kLD + bc;
      const double* ur = urow + 32 * bh;
      double c = 0.0;
#pragma unroll 8
      for (int r = 0; r < 32; ++r) c = fma((double)xc[r * kLD], ur[r], c);
      gacc += c;
    }
  }

  if (!kTrain) return;
  __syncthreads();  // the last tile's reads of urow are done: the upper row half's column sums go over it and lsum
  double t[kTail] = {};
  if (tid >= 192) {  // wave 3: the 64 tile rows' sums in a fixed order
    const int l = tid - 192;
    t[0] = cdna::wave_sum(usum[l]);
    t[1] = cdna::wave_sum(vsum[l]);
    t[2] = cdna::wave_sum(lsum[l]);
    t[3] = cdna::wave_sum(wsum[l]);
    t[4] = cdna::wave_sum((double)cnt[l]);
  }
  __syncthreads();
  if (tid >= kMaxD) urow[tid - kMaxD] = gacc;  // [kMaxD] doubles: urow and lsum
  __syncthreads();
  double* slot = ws + (int64_t)blockIdx.x * kSlot;
  if (tid < d) slot[tid] = gacc + urow[tid];
  if (tid == 192)
    for (int i = 0; i < kTail; ++i) slot[kMaxD + i] = t[i];
}

// One block of 256 threads per 16 output values: out [d + 5] = [dcoef | sum u | sum v | loss | sum w | bad].
__global__ __launch_bounds__(256) void margin_reduce_kernel(const double* __restrict__ ws, int nblk, int d,
                                                            double* __restrict__ out) {
  __shared__ double red[16][16];
  const int idx = blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = idx < d + kTail;
  const int src = idx < d ? idx : kMaxD + (idx - d);
  const double t = sum_blocks(red, nblk, ok, [&](int b) { return ws[(int64_t)b * kSlot + src]; });
  if (threadIdx.x < 16 && ok) out[idx] = t;
}

struct MarginPlan : RowSplit {
  bool native, vec;
  int per_cu;
};

// One round of resident blocks on the 256 CUs, per_cu(vec) per CU; at least 1024 rows per block.
MarginPlan margin_plan(const float* X, int64_t n, int64_t ldx, int d) {
  MarginPlan pl{};
  pl.native = n >= 1 && d >= 1 && d <= kMaxD && ldx >= d && X != nullptr;
  if (!pl.native) return pl;
  pl.vec = float4_rows(X, d, ldx);
  pl.per_cu = per_cu(pl.vec);
  static_cast<RowSplit&>(pl) = split_rows(n, (int64_t)pl.per_cu * 256);
  return pl;
}

template <int LOSS, int MODE>
int step_launch(const MarginPlan& pl, const float* X, int64_t n, int64_t ldx, const double* y,
                const double* wt, const double* coef, const MarginParams& pr, double* ws, double* marg,
                hipStream_t st) {
  if (pl.vec)
    hipLaunchKernelGGL((margin_step_kernel<LOSS, MODE, 4>), dim3(pl.nblk), dim3(256), 0, st, X, n, ldx, y, wt, coef, pr,
                       ws, marg, pl.rows_per_block);
  else
    hipLaunchKernelGGL((margin_step_kernel<LOSS, MODE, 1>), dim3(pl.nblk), dim3(256), 0, st, X, n, ldx, y, wt, coef, pr,
                       ws, marg, pl.rows_per_block);
  return (int)hipGetLastError();
}

}  // namespace

static_assert((size_t)kXF * 4 % 8 == 0, "the fp64 words of LDS start 8-byte aligned");
static_assert(kLds * kPerCuLds <= 160 * 1024, "kPerCuLds blocks per CU");

// What cdna_margin_step runs for these operands (nothing is launched): out = [native, load width (4: float4 rows, 1:
// scalar), blocks, rows per block, LDS bytes, workspace doubles per block, blocks per CU].
CDNA_API int cdna_margin_plan(const float* X, int64_t n, int64_t ldx, int d, int64_t* out) {
  const MarginPlan pl = margin_plan(X, n, ldx, d);
  for (int i = 0; i < 7; ++i) out[i] = 0;
  if (!pl.native) return 0;
  out[0] = 1;
  out[1] = pl.vec ? 4 : 1;
  out[2] = pl.nblk;
  out[3] = pl.rows_per_block;
  out[4] = (int64_t)kLds;
  out[5] = kSlot;
  out[6] = pl.per_cu;
  return 0;
}

// coef [d] f64 (for the raw rows), b0 the intercept; loss 0: squared hinge, 1: Huber with sigma > 0 and epsilon.
// STEP (mode 0): y [n] f64, wt [n] f64 row weights or null, out [d + 5] f64 = [dcoef | sum u | sum v | loss | sum w |
// bad] (un-normalised sums over the rows that are not bad, and the number of bad rows), ws: blocks x workspace doubles
// per block of cdna_margin_plan.
// PREDICT (mode 1): marg [n] f64 = x.coef + b0.
CDNA_API int cdna_margin_step(const float* X, int64_t n, int64_t ldx, const double* y, const double* wt,
                              const double* coef, double b0, double sigma, double epsilon, int d, int loss, int mode,
                              double* out, double* ws, double* marg, hipStream_t st) {
  const MarginPlan pl = margin_plan(X, n, ldx, d);
  if (!pl.native || coef == nullptr) return (int)hipErrorInvalidValue;
  if ((mode != kStep && mode != kPredict) || (loss != kSquaredHinge && loss != kHuber))
    return (int)hipErrorInvalidValue;
  if (mode == kStep && (y == nullptr || out == nullptr || ws == nullptr)) return (int)hipErrorInvalidValue;
  if (mode == kStep && loss == kHuber && !(sigma > 0.0 && sigma <= 1.7976931348623157e308 && epsilon > 0.0 &&
                                           epsilon <= 1.7976931348623157e308))
    return (int)hipErrorInvalidValue;
  if (mode == kPredict && marg == nullptr) return (int)hipErrorInvalidValue;
  const MarginParams pr{b0, sigma, epsilon, d};
  if (mode == kPredict)
    return step_launch<kSquaredHinge, kPredict>(pl, X, n, ldx, y, wt, coef, pr, ws, marg, st);
  const int rc = loss == kHuber ? step_launch<kHuber, kStep>(pl, X, n, ldx, y, wt, coef, pr, ws, marg, st)
                                : step_launch<kSquaredHinge, kStep>(pl, X, n, ldx, y, wt, coef, pr, ws, marg, st);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(margin_reduce_kernel, dim3((unsigned)((d + kTail + 15) / 16)), dim3(256), 0, st, ws, pl.nblk, d,
                     out);
  return (int)hipGetLastError();
}
