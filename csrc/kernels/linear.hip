// K31 linear_step — one loss-and-gradient evaluation (or the predictions) of a binomial or multinomial logistic model
// in one pass over fp32 rows, every product and sum in fp64 on v_mfma_f64_16x16x4_f64.
//
// K margins per row: K = 1 with the binomial top (margin m = x.w + b, loss w (log(1 + e^m) - y m), R = w (sigma(m) -
// y)), K = C in 2 .. 32 with the softmax top (z_c = x.W_c + b_c, loss w (lse(z) - z_y), R_c = w (P_c - [c == y])).
// The gradient is G = R^T X ([K][d]) with the column sums of R for the intercepts.  The kernel works on the raw rows:
// the host passes W already divided by the features' std, as a zero-padded fp64 table Wt [d4 = d rounded up to 4]
// [NC = 16 KB] (KB = ceil(K / 16) column blocks of the MFMA).
//
// linear_step_kernel<MODE, KB, VW>: 256 threads, 64-row tiles, the next tile of X prefetched in registers, the tile
// row-major fp32 in LDS with the odd row stride kLD (rowblock.h's scaffolding).  LDS behind the tile: Wt as it
// comes (every wave reads all of it for every tile: 16 to 32 KB a tile from L2 per block would rival the rows
// themselves, from LDS it is one conflict-free 8-byte read per MFMA), Z [64][NC + 1] fp64, the intercepts, the tile
// rows' running loss and weight sums and bad counts, and the rows' bad-feature flags.
//   The instruction: D [16][16] += A [16][4] B [4][16], one fp64 of A and of B and four of D per lane; lane l holds
//     A[l % 16][l / 16], B[l / 16][l % 16] and D[4 v + l / 16][l % 16] in its v-th result register.  The products are
//     summed over the four k slots whatever columns they stand for, as long as A and B agree: the lane maps below use
//     that to keep the fp32 tile reads off shared banks (row stride 129 = 1 mod 32).
//   put: the tile goes to LDS through RowTile::store, which flags the rows that hold a non-finite feature.
//   margins: Z^T = Wt^T X^T, so that the tile is the B operand.  Wave w takes the 16 rows 32 (w / 2) + 2 j + w % 2
//     (j = l % 16: every other row, so a half wave's 16 rows x 2 k slots read 32 different banks) and all KB class
//     blocks; step s of ceil(d / 4) multiplies columns 4 s .. 4 s + 3 (k slot g = l / 16 is column 4 s + g), the
//     floats converted as they are read.  D goes to Z [row][class].
//   top: the four threads of a row take the classes q, q + 4, ..: intercepts, the max-subtracted logsumexp (or the
//     overflow-free log(1 + e^m) and sigmoid), the loss term and R written over the row of Z, zeros in the padding
//     classes.  A bad row -- a non-finite feature or weight, a label that is not an integer in [0, C), or a loss term
//     that is not finite (the margins overflowed) -- is counted and adds exactly nothing: its terms become 0 and its
//     four threads zero its tile row, so the gradient never multiplies a NaN by 0.  Rows past the end of the block's
//     range are zeros in the tile and are never read from memory.
//   gradient: G [NC][d] += R^T X on the same instruction, the 64 tile rows the reduction dimension: step s of 16
//     multiplies tile rows s, 16 + s, 32 + s, 48 + s (k slot g is row 16 g + s: two k slots of a half wave are 16
//     banks apart).  Wave w takes the 16-column blocks w and w + 4 of d, all KB class blocks: up to 4 accumulators of
//     4 fp64 per lane, kept over all the block's tiles.  The intercept gradient: thread (class tid % NC, part tid /
//     NC) adds its NC / 4 rows of R per tile into one register.
//   At the end each block writes one workspace slot [G [K][d] | intercepts [K] | loss | sum w | bad].
//   PREDICT: margins and top only: raw [n][C], prob [n][C] fp64 and pred [n] int32 (softmax: the lowest index among
//     equal probabilities; binomial: raw = [-m, m], prob = [1 - p, p], pred = p > threshold).
// linear_reduce_kernel: the slots' sum over the blocks in a fixed order in fp64 (rowblock.h's sum_blocks), straight
// into the caller's layout.  No float atomics: reruns at the same grid are bit-identical.
// Native range: fp32 rows, 1 <= d <= 128, 1 <= K <= 32, any n, row stride and alignment.
#include <cmath>

#include "rowblock.h"

namespace {

using namespace rowblock;

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxK = 32;
constexpr size_t kCuLds = 160 * 1024;

enum { kStep = 0, kPredict = 1 };

struct LinParams {
  double threshold;
  int d, K, binomial;
};

// doubles of LDS behind the tile: Wt [d4][NC], Z [64][NC + 1], intercepts [NC], loss and weight sums [2][64]
constexpr int lds_doubles(int d, int KB) { return ((d + 3) / 4 * 4 + kRows) * 16 * KB + kRows + 16 * KB + 2 * kRows; }
constexpr size_t lds_bytes(int d, int KB) { return (size_t)kXF * 4 + (size_t)lds_doubles(d, KB) * 8 + 2 * kRows * 4; }
constexpr int slot_doubles(int d, int K) { return K * (d + 1) + 3; }

template <int MODE, int KB, int VW>
__global__ __launch_bounds__(256, VW == 4 ? 2 : 1) void linear_step_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const double* __restrict__ y, const double* __restrict__ wt,
    const double* __restrict__ Wt, const double* __restrict__ bias, const LinParams pr, double* __restrict__ ws,
    double* __restrict__ raw, double* __restrict__ prob, int* __restrict__ pred, int64_t rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool kTrain = MODE == kStep;
  constexpr int NC = 16 * KB, P = NC + 1, NJ = NC / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = pr.d, K = pr.K, dv = d / VW, d4 = (d + 3) / 4 * 4;
  float* xb = reinterpret_cast<float*>(smem);                 // [kXF]
  double* Wl = reinterpret_cast<double*>(smem + kXF * 4);     // [d4][NC]
  double* Zb = Wl + d4 * NC;                                  // [kRows][P]
  double* bl = Zb + kRows * P;                                // [NC]
  double* lsum = bl + NC;                                     // [kRows] running loss of the tile row
  double* wsum = lsum + kRows;                                // [kRows] running sum of its weights
  int* cnt = reinterpret_cast<int*>(wsum + kRows);            // [kRows] its bad rows
  int* flag = cnt + kRows;                                    // [kRows] this tile's rows with a non-finite feature

  for (int i = tid; i < d4 * NC; i += 256) Wl[i] = Wt[i];
  for (int i = tid; i < kRows * P + NC + 2 * kRows; i += 256)
    Zb[i] = i >= kRows * P && i - kRows * P < K ? bias[i - kRows * P] : 0.0;
  if (tid < 2 * kRows) cnt[tid] = 0;

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  const int rr = tid >> 2, qq = tid & 3, ln = lane & 15, lg = lane >> 4;
  const int mrow = 32 * (wave >> 1) + 2 * ln + (wave & 1);  // margins: this lane's tile row
  const int bc = tid % NC, br0 = tid / NC * NJ;             // intercepts: this thread's class and first row
  f64x4 acc[2][KB] = {};
  double bacc = 0.0;
  double yn = 0.0, wn = 1.0;
  // the row's label and weight travel with its tile
  const auto side = [&](int64_t t, int i) {
    if (kTrain && t + (i >> 2) < rb1) {
      yn = y[t + (i >> 2)];
      if (wt != nullptr) wn = wt[t + (i >> 2)];
    }
  };
  TileStream<VW> ts;
  ts.begin(xb, kXF, X, ldx, rb0, rb1, dv, tid, side);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    const bool valid = t0 + rr < rb1;
    const double yy = yn, ww = wn;
    __syncthreads();  // every wave is past its reads of the previous tile (and the zeroing, at first)
    ts.xt.store(xb, kLD, tid, dv, [&](int r, int, float x) {
      if (kTrain && !(fabsf(x) <= 3.4028234663852886e38f)) flag[r] = 1;
      return x;
    });
    ts.fetch(t0, tid, side);

    // margins: Z^T [NC][16 rows of this wave] = Wt^T X^T
    {
      f64x4 z[KB] = {};
      const float* xr = xb + mrow * kLD + lg;
      const double* wr = Wl + lg * NC + ln;
      for (int s = 0; s < d4; s += 4) {
        const double b = (double)xr[s];
#pragma unroll
        for (int cb = 0; cb < KB; ++cb)
          z[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[s * NC + 16 * cb], b, z[cb], 0, 0, 0);
      }
#pragma unroll
      for (int cb = 0; cb < KB; ++cb)
#pragma unroll
        for (int v = 0; v < 4; ++v) Zb[mrow * P + 16 * cb + 4 * v + lg] = z[cb][v];
    }
    __syncthreads();

    // top: the four threads of a row, classes qq + 4 j
    {
      double* zr = Zb + rr * P + qq;
      double z[NJ], e[NJ];
      double loss, sum = 1.0, mx = 0.0;
      int yi = -1;
      bool ok = true;
      if (kTrain) {
        ok = yy >= 0.0 && yy < (pr.binomial ? 2.0 : (double)K);
        yi = ok ? (int)yy : -1;
        ok = ok && (double)yi == yy && cdna::finite_d(ww) && flag[rr] == 0;
      }
      if (pr.binomial) {
        // the row's four threads all form m; e[0] = sigma(m) without overflow
        const double m = Zb[rr * P] + bl[0], t = exp(-fabs(m));
        e[0] = (m >= 0.0 ? 1.0 : t) / (1.0 + t);
        z[0] = m;
        loss = ww * (log1p(t) + fmax(m, 0.0) - yy * m);
#pragma unroll
        for (int j = 1; j < NJ; ++j) e[j] = 0.0;
      } else {
        mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int c = qq + 4 * j;
          z[j] = c < K ? zr[4 * j] + bl[c] : -INFINITY;
          mx = fmax(mx, z[j]);
        }
        mx = fmax(mx, __shfl_xor(mx, 1));
        mx = fmax(mx, __shfl_xor(mx, 2));
        sum = 0.0;
        double zy = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          e[j] = qq + 4 * j < K ? exp(z[j] - mx) : 0.0;
          sum += e[j];
          if (qq + 4 * j == yi) zy = z[j];
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        zy += __shfl_xor(zy, 1);
        zy += __shfl_xor(zy, 2);
        loss = ww * (mx + log(sum) - zy);
#pragma unroll
        for (int j = 0; j < NJ; ++j) e[j] /= sum;
      }

      if (!kTrain) {
        if (valid) {
          if (pr.binomial) {
            if (qq == 0) {
              const int64_t o = (t0 + rr) * 2;
              raw[o] = -z[0], raw[o + 1] = z[0];
              prob[o] = 1.0 - e[0], prob[o + 1] = e[0];
              pred[t0 + rr] = e[0] > pr.threshold ? 1 : 0;
            }
          } else {
            const int64_t o = (t0 + rr) * K + qq;
            double best = -1.0;
            int arg = 0;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
              if (qq + 4 * j < K) {
                raw[o + 4 * j] = z[j];
                prob[o + 4 * j] = e[j];
                if (e[j] > best) best = e[j], arg = qq + 4 * j;
              }
#pragma unroll
            for (int o2 = 1; o2 <= 2; o2 <<= 1) {
              const double ob = __shfl_xor(best, o2);
              const int oa = __shfl_xor(arg, o2);
              if (ob > best || (ob == best && oa < arg)) best = ob, arg = oa;
            }
            if (qq == 0) pred[t0 + rr] = arg;
          }
        }
        continue;
      }

      ok = ok && cdna::finite_d(loss);
      const bool live = valid && ok;
      if (pr.binomial) e[0] -= yy;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = qq + 4 * j;
        double r = 0.0;
        if (live && c < K && (!pr.binomial || c == 0)) r = ww * (pr.binomial ? e[0] : e[j] - (c == yi ? 1.0 : 0.0));
        zr[4 * j] = r;
      }
      if (qq == 0) {
        lsum[rr] += live ? loss : 0.0;
        wsum[rr] += live ? ww : 0.0;
        cnt[rr] += valid && !ok ? 1 : 0;
      }
      if (valid && !ok && 32 * qq < d) {
        float* xq = xb + rr * kLD + 32 * qq;
        for (int j = 0; j < 32; ++j) xq[j] = 0.f;
      }
    }
    __syncthreads();  // R complete, bad rows zeroed

    if (tid < kRows) flag[tid] = 0;
    // G [NC][16 columns] += R^T X, tile rows 16 g + s in step s
#pragma unroll 2
    for (int s = 0; s < 16; ++s) {
      const int r = 16 * lg + s;
      double a[KB];
#pragma unroll
      for (int cb = 0; cb < KB; ++cb) a[cb] = Zb[r * P + 16 * cb + ln];
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) {
        const int c0 = 16 * (wave + 4 * jb);
        if (c0 < d) {
          const double b = (double)xb[r * kLD + c0 + ln];
#pragma unroll
          for (int cb = 0; cb < KB; ++cb)
            acc[jb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cb], b, acc[jb][cb], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) bacc += Zb[(br0 + j) * P + bc];
  }

  if (!kTrain) return;
  double* slot = ws + (int64_t)blockIdx.x * slot_doubles(d, K);
#pragma unroll
  for (int jb = 0; jb < 2; ++jb)
#pragma unroll
    for (int cb = 0; cb < KB; ++cb)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int c = 16 * cb + 4 * v + lg, col = 16 * (wave + 4 * jb) + ln;
        if (c < K && col < d) slot[c * d + col] = acc[jb][cb][v];
      }
  __syncthreads();  // the last tile's reads of Z are done: the intercept parts go over it
  Zb[tid] = bacc;   // [256 / NC parts][NC]
  double a = 0.0, b = 0.0, c = 0.0;
  if (wave == 3) {  // the 64 tile rows' sums in a fixed order
    a = cdna::wave_sum(lsum[lane]);
    b = cdna::wave_sum(wsum[lane]);
    c = cdna::wave_sum((double)cnt[lane]);
  }
  __syncthreads();
  if (tid < K) {
    double t = 0.0;
    for (int p = 0; p < 256 / NC; ++p) t += Zb[p * NC + tid];
    slot[K * d + tid] = t;
  }
  if (tid == 192) {
    slot[K * (d + 1)] = a;
    slot[K * (d + 1) + 1] = b;
    slot[K * (d + 1) + 2] = c;
  }
}

// One block of 256 threads per 16 output values: out [K (d + 1) + 3] = the slots' sum.
__global__ __launch_bounds__(256) void linear_reduce_kernel(const double* __restrict__ ws, int nblk, int slot,
                                                            double* __restrict__ out) {
  __shared__ double red[16][16];
  const int idx = blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = idx < slot;
  const double t = sum_blocks(red, nblk, ok, [&](int b) { return ws[(int64_t)b * slot + idx]; });
  if (threadIdx.x < 16 && ok) out[idx] = t;
}

struct LinPlan : RowSplit {
  bool native;
  int KB, per_cu;
  size_t lds;
};

// One round of resident blocks on the 256 CUs: as many per CU as the LDS lets in, and by registers two of the float4
// instantiations (held to 256 registers a lane) and one of the scalar ones (their 32 row addresses a lane take more:
// see the README's K31 row); at least 1024 rows per block.
LinPlan lin_plan(int64_t n, int d, int K, bool vec) {
  LinPlan pl{};
  pl.native = n >= 1 && d >= 1 && d <= kMaxD && K >= 1 && K <= kMaxK;
  if (!pl.native) return pl;
  pl.KB = (K + 15) / 16;
  pl.lds = lds_bytes(d, pl.KB);
  pl.per_cu = (int)(kCuLds / pl.lds);
  if (pl.per_cu > (vec ? 2 : 1)) pl.per_cu = vec ? 2 : 1;
  static_cast<RowSplit&>(pl) = split_rows(n, (int64_t)pl.per_cu * 256);
  return pl;
}

template <int MODE, int KB, int VW>
int lin_launch(const LinPlan& pl, const float* X, int64_t n, int64_t ldx, const double* y, const double* wt,
               const double* Wt, const double* bias, const LinParams& pr, double* ws, double* raw, double* prob,
               int* pred, hipStream_t st) {
  static bool raised[64] = {};
  const int rc = cdna::raise_lds(reinterpret_cast<const void*>(linear_step_kernel<MODE, KB, VW>), raised,
                                 lds_bytes(kMaxD, KB));
  if (rc != 0) return rc;
  hipLaunchKernelGGL((linear_step_kernel<MODE, KB, VW>), dim3(pl.nblk), dim3(256), pl.lds, st, X, n, ldx, y, wt, Wt,
                     bias, pr, ws, raw, prob, pred, pl.rows_per_block);
  return (int)hipGetLastError();
}

template <int MODE, int KB>
int lin_launch_vw(bool vec, const LinPlan& pl, const float* X, int64_t n, int64_t ldx, const double* y,
                  const double* wt, const double* Wt, const double* bias, const LinParams& pr, double* ws, double* raw,
                  double* prob, int* pred, hipStream_t st) {
  return vec ? lin_launch<MODE, KB, 4>(pl, X, n, ldx, y, wt, Wt, bias, pr, ws, raw, prob, pred, st)
             : lin_launch<MODE, KB, 1>(pl, X, n, ldx, y, wt, Wt, bias, pr, ws, raw, prob, pred, st);
}

}  // namespace

static_assert((size_t)kXF * 4 % 16 == 0, "the fp64 words of LDS start aligned");
static_assert(lds_bytes(kMaxD, 2) <= kCuLds, "the widest block fits a CU");
static_assert(256 <= kRows * 17, "the fold of the intercept parts fits Z");

// What cdna_linear_step runs for these operands (nothing is launched): out = [native, KB (16-class blocks), load
// width (4: float4 rows, 1: scalar), blocks, rows per block, LDS bytes per block, workspace doubles per block, blocks
// per CU].
CDNA_API int cdna_linear_plan(const float* X, int64_t n, int64_t ldx, int d, int K, int64_t* out) {
  const LinPlan pl = lin_plan(n, d, K, float4_rows(X, d, ldx));
  for (int i = 0; i < 8; ++i) out[i] = 0;
  if (!pl.native || ldx < d) return 0;
  out[0] = 1;
  out[1] = pl.KB;
  out[2] = float4_rows(X, d, ldx) ? 4 : 1;
  out[3] = pl.nblk;
  out[4] = pl.rows_per_block;
  out[5] = (int64_t)pl.lds;
  out[6] = slot_doubles(d, K);
  out[7] = pl.per_cu;
  return 0;
}

// Wt [d rounded up to 4][16 ceil(K / 16)] f64: the coefficients for the raw rows, class c in column c, zeros in the
// padding; bias [K] f64.  binomial: K = 1, the labels 0 / 1.
// STEP: y [n] f64 labels, wt [n] f64 row weights or null, out [K (d + 1) + 3] f64 = [G [K][d] | intercepts [K] | loss
// | sum w | bad] (un-normalised sums over the rows that are not bad, and the number of bad rows), ws: blocks x
// workspace doubles per block of cdna_linear_plan.
// PREDICT: raw, prob [n][binomial ? 2 : K] f64, pred [n] int32.
CDNA_API int cdna_linear_step(const float* X, int64_t n, int64_t ldx, const double* y, const double* wt,
                              const double* Wt, const double* bias, int d, int K, int binomial, double threshold,
                              int mode, double* out, double* ws, double* raw, double* prob, int* pred,
                              hipStream_t st) {
  const bool vec = float4_rows(X, d, ldx);
  const LinPlan pl = lin_plan(n, d, K, vec);
  if (!pl.native || ldx < d || X == nullptr || Wt == nullptr || bias == nullptr) return (int)hipErrorInvalidValue;
  if (mode != kStep && mode != kPredict) return (int)hipErrorInvalidValue;
  if (binomial ? K != 1 : K < 2) return (int)hipErrorInvalidValue;
  if (mode == kStep && (y == nullptr || out == nullptr || ws == nullptr)) return (int)hipErrorInvalidValue;
  if (mode == kPredict && (raw == nullptr || prob == nullptr || pred == nullptr)) return (int)hipErrorInvalidValue;
  const LinParams pr{threshold, d, K, binomial ? 1 : 0};
  int rc;
  if (mode == kStep)
    rc = pl.KB == 1 ? lin_launch_vw<kStep, 1>(vec, pl, X, n, ldx, y, wt, Wt, bias, pr, ws, raw, prob, pred, st)
                    : lin_launch_vw<kStep, 2>(vec, pl, X, n, ldx, y, wt, Wt, bias, pr, ws, raw, prob, pred, st);
  else
    rc = pl.KB == 1 ? lin_launch_vw<kPredict, 1>(vec, pl, X, n, ldx, y, wt, Wt, bias, pr, ws, raw, prob, pred, st)
                    : lin_launch_vw<kPredict, 2>(vec, pl, X, n, ldx, y, wt, Wt, bias, pr, ws, raw, prob, pred, st);
  if (rc != 0 || mode == kPredict) return rc;
  const int slot = slot_doubles(d, K);
  hipLaunchKernelGGL(linear_reduce_kernel, dim3((unsigned)((slot + 15) / 16)), dim3(256), 0, st, ws, pl.nblk, slot,
                     out);
  return (int)hipGetLastError();
}
