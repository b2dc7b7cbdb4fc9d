// K34 nb_step — the sufficient statistics of a naive Bayes fit, or its predictions, in one pass over fp32 rows, every
// product and sum in fp64 on v_mfma_f64_16x16x4_f64.
//
// STATS: per class c in [0, C), W_c = sum w, S_c[j] = sum w (x_j - s_j) and (QUAD) Q_c[j] = sum w (x_j - s_j)^2 over
//   the rows of label c, s an fp32 shift vector (zeros for the count models, a point near the mean for Gaussian: the
//   variance is then formed about it and does not cancel).
// PREDICT: raw [n][C], prob = softmax(raw) [n][C] fp64 and pred [n] int32 (the lowest index among equal
//   probabilities) with  raw_c = g_c + sum_j T1[j][c] u_j  (+ sum_j T2[j][c] u_j^2 with QUAD),  u = x (QUAD: x - s).
//   Multinomial, complement and Bernoulli are the linear form; Gaussian is the quadratic one with T2 = -1/(2 sigma),
//   T1 = (mu - s) / sigma and the constant folded into g: no [n][C][d] intermediate exists.
//
// nb_step_kernel<MODE, QUAD, KB, VW>: 256 threads, 64-row tiles, the next tile of X prefetched in registers, the tile
// row-major fp32 in LDS with the odd row stride kLD (rowblock.h's scaffolding).  KB = ceil(C / 16) class blocks of the
// MFMA, NC = 16 KB.  The instruction: D [16][16] += A [16][4] B [4][16]; lane l holds A[l % 16][l / 16],
// B[l / 16][l % 16] and D[4 v + l / 16][l % 16] in its v-th result register (linear.hip has the lane maps' reasons).
//   STATS
//     rows: the four threads of a row scan 32 columns each (thread q starts 8 q columns in: a half wave reads 32
//       banks) for a non-finite value and for one that breaks the value rule (FINITE: none; NONNEG: x < 0; BINARY:
//       x not 0 or 1), and check the label (an integer in [0, C)) and the weight (finite, >= 0).  A bad row is counted
//       in the first of the three counters that applies, gets class -1 and weight 0, and its tile row is zeroed: it
//       adds exactly nothing and a NaN is never multiplied by 0.  Rows past the end of the block's range are zeros in
//       the tile and are never read from memory.
//     sums: G [NC][16 columns] += R^T X~ with the 64 tile rows the reduction dimension (step s multiplies tile rows
//       s, 16 + s, 32 + s, 48 + s).  The A operand R[r][c] = w_r [y_r == c] is formed in registers from the rows'
//       class and weight in LDS (one broadcast read per k slot); the B operand is the tile's float, converted and the
//       shift subtracted as it is read; QUAD feeds the same A against the squared B into a second accumulator set.
//       Wave w takes the 16-column blocks w and w + 4 of d for every class block: up to 4 (QUAD: 8) accumulators of
//       4 fp64 per lane, kept over all the block's tiles.  W: thread (class tid % NC, part tid / NC) adds its NC / 4
//       rows per tile into one register, in row order.
//     At the end each block writes one workspace slot [S [C][d] | Q [C][d] (QUAD) | W [C] | 3 counters].
//   PREDICT
//     margins: Z^T = T^T U^T, the tile the B operand (linear.hip's margin phase), the fp64 tables T1 (and T2) [d4][NC]
//       in LDS; QUAD runs two chains over the same tile values, on u and on u^2, into one accumulator.
//     top: the four threads of a row take the classes q, q + 4, ..: g_c, the max-subtracted softmax and the argmax.
//       A row with a non-finite feature gets NaN raw and prob and pred 0, and is counted (one integer atomic per
//       block on a counter the caller zeroed).
// nb_reduce_kernel: the slots' sum over the blocks in a fixed order in fp64 (rowblock.h's sum_blocks).  No float
// atomics: reruns at the same grid are bit-identical, and integer-valued inputs give exact integer sums below 2^53.
// Native range: fp32 rows, 1 <= d <= 128, 2 <= C <= 32, any n, row stride and alignment.
#include <cmath>

#include "rowblock.h"

namespace {

using namespace rowblock;

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxC = 32;
constexpr size_t kCuLds = 160 * 1024;

enum { kStats = 0, kPredict = 1 };
enum { kFinite = 0, kNonNeg = 1, kBinary = 2 };

struct NbParams {
  int d, C, rule;
};

constexpr int d4_of(int d) { return (d + 3) / 4 * 4; }
// LDS behind the tile (bytes).  STATS: shift [128] f32, the rows' weight [64] f64 and class [64] int, the tile rows'
// three counters [3][64] int, the fold of W [256] f64.  PREDICT: shift [128] f32, T1 (and T2) [d4][NC], Z [64][NC + 1],
// g [NC] f64, the rows' flags and counts [2][64] int.
constexpr size_t stats_lds() { return (size_t)kXF * 4 + kMaxD * 4 + kRows * 8 + 256 * 8 + kRows * 4 + 3 * kRows * 4; }
constexpr size_t predict_lds(int d, int KB, int quad) {
  return (size_t)kXF * 4 + kMaxD * 4 + ((size_t)(1 + quad) * d4_of(d) * 16 * KB + kRows * (16 * KB + 1) + 16 * KB) * 8 +
         2 * kRows * 4;
}
constexpr int slot_doubles(int d, int C, int quad) { return (1 + quad) * C * d + C + 3; }

template <int MODE, int QUAD, int KB, int VW>
__global__ __launch_bounds__(256, VW == 4 ? 2 : 1) void nb_step_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const double* __restrict__ y, const double* __restrict__ wt,
    const float* __restrict__ shift, const double* __restrict__ T1, const double* __restrict__ T2,
    const double* __restrict__ g, const NbParams pr, double* __restrict__ ws, double* __restrict__ raw,
    double* __restrict__ prob, int* __restrict__ pred, int* __restrict__ nbad, int64_t rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NC = 16 * KB, P = NC + 1, NJ = NC / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = pr.d, C = pr.C, dv = d / VW, d4 = d4_of(d);
  const int rr = tid >> 2, qq = tid & 3, ln = lane & 15, lg = lane >> 4;
  float* xb = reinterpret_cast<float*>(smem);  // [kXF]
  float* shl = xb + kXF;                       // [kMaxD] the shift, zeros from d on
  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  if (tid < kMaxD) shl[tid] = (shift != nullptr && tid < d) ? shift[tid] : 0.f;

  if constexpr (MODE == kStats) {
    double* rw = reinterpret_cast<double*>(shl + kMaxD);  // [kRows] this tile's weights, 0 for a row that adds nothing
    double* fold = rw + kRows;                            // [256] the parts of W at the end
    int* rc = reinterpret_cast<int*>(fold + 256);         // [kRows] this tile's classes, -1 for such a row
    int* cnt = rc + kRows;                                // [3][kRows] the tile rows' bad rows by kind
    if (tid < 3 * kRows) cnt[tid] = 0;
    const int bc = tid % NC, br0 = tid / NC * NJ;  // W: this thread's class and first row
    f64x4 acc[1 + QUAD][2][KB] = {};
    double wacc = 0.0;
    double yn = 0.0, wn = 1.0;
    // the row's label and weight travel with its tile
    const auto side = [&](int64_t t, int i) {
      if (t + (i >> 2) < rb1) {
        yn = y[t + (i >> 2)];
        if (wt != nullptr) wn = wt[t + (i >> 2)];
      }
    };
    TileStream<VW> ts;
    ts.begin(xb, kXF, X, ldx, rb0, rb1, dv, tid, side);
    for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
      const bool valid = t0 + rr < rb1;
      const double yy = yn, ww = wn;
      ts.put(xb, tid);
      ts.fetch(t0, tid, side);

      // the row's values, label and weight
      {
        float* xq = xb + rr * kLD + 32 * qq;
        const bool mine = 32 * qq < d;
        int nf = 0, rb = 0;
        if (mine) {
#pragma unroll 8
          for (int j = 0; j < 32; ++j) {
            const float x = xq[(j + 8 * qq) & 31];
            nf |= !(fabsf(x) <= 3.4028234663852886e38f);
            rb |= pr.rule == kNonNeg ? x < 0.f : (pr.rule == kBinary ? (x != 0.f && x != 1.f) : false);
          }
        }
        nf |= __shfl_xor(nf, 1);
        nf |= __shfl_xor(nf, 2);
        rb |= __shfl_xor(rb, 1);
        rb |= __shfl_xor(rb, 2);
        bool lab = yy >= 0.0 && yy < (double)C;
        const int yi = lab ? (int)yy : -1;
        lab = lab && (double)yi == yy && ww >= 0.0 && cdna::finite_d(ww);
        const int kind = nf ? 0 : (rb ? 1 : (lab ? -1 : 2));
        const bool live = valid && kind < 0;
        if (qq == 0) {
          rw[rr] = live ? ww : 0.0;
          rc[rr] = live ? yi : -1;
          if (valid && kind >= 0) cnt[kind * kRows + rr] += 1;
        }
        if (valid && kind >= 0 && mine)
          for (int j = 0; j < 32; ++j) xq[j] = 0.f;
      }
      __syncthreads();  // the rows' weights and classes complete, bad rows zeroed

      // G [NC][16 columns] += R^T X~, tile rows 16 g + s in step s
#pragma unroll 2
      for (int s = 0; s < 16; ++s) {
        const int r = 16 * lg + s;
        const double w = rw[r];
        const int c = rc[r];
        double a[KB];
#pragma unroll
        for (int cb = 0; cb < KB; ++cb) a[cb] = c == 16 * cb + ln ? w : 0.0;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
          const int c0 = 16 * (wave + 4 * jb);
          if (c0 < d) {
            const double b = (double)xb[r * kLD + c0 + ln] - (double)shl[c0 + ln];
#pragma unroll
            for (int cb = 0; cb < KB; ++cb)
              acc[0][jb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cb], b, acc[0][jb][cb], 0, 0, 0);
            if (QUAD) {
              const double b2 = b * b;
#pragma unroll
              for (int cb = 0; cb < KB; ++cb)
                acc[QUAD][jb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cb], b2, acc[QUAD][jb][cb], 0, 0, 0);
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) wacc += rc[br0 + j] == bc ? rw[br0 + j] : 0.0;
    }

    double* slot = ws + (int64_t)blockIdx.x * slot_doubles(d, C, QUAD);
#pragma unroll
    for (int q = 0; q <= QUAD; ++q)
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int cb = 0; cb < KB; ++cb)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int c = 16 * cb + 4 * v + lg, col = 16 * (wave + 4 * jb) + ln;
            if (c < C && col < d) slot[(q * C + c) * d + col] = acc[q][jb][cb][v];
          }
    fold[tid] = wacc;  // [256 / NC parts][NC]
    __syncthreads();   // also: the last tile's counts are complete
    const int wbase = (1 + QUAD) * C * d;
    if (tid < C) {
      double t = 0.0;
      for (int p = 0; p < 256 / NC; ++p) t += fold[p * NC + tid];
      slot[wbase + tid] = t;
    }
    if (wave == 3) {  // the 64 tile rows' counts
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double t = cdna::wave_sum((double)cnt[k * kRows + lane]);
        if (lane == 0) slot[wbase + C + k] = t;
      }
    }
  } else {
    double* Tl = reinterpret_cast<double*>(shl + kMaxD);  // [1 + QUAD][d4][NC]
    double* Zb = Tl + (1 + QUAD) * d4 * NC;               // [kRows][P]
    double* gl = Zb + kRows * P;                          // [NC]
    int* flag = reinterpret_cast<int*>(gl + NC);          // [kRows] this tile's rows with a non-finite feature
    int* cnt = flag + kRows;                              // [kRows] the tile rows' such rows
    for (int i = tid; i < d4 * NC; i += 256) {
      Tl[i] = T1[i];
      if (QUAD) Tl[d4 * NC + i] = T2[i];
    }
    if (tid < NC) gl[tid] = tid < C ? g[tid] : 0.0;
    if (tid < 2 * kRows) flag[tid] = 0;
    const int mrow = 32 * (wave >> 1) + 2 * ln + (wave & 1);  // this lane's tile row (see linear.hip)
    const auto side = [](int64_t, int) {};
    TileStream<VW> ts;
    ts.begin(xb, kXF, X, ldx, rb0, rb1, dv, tid, side);
    for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
      const bool valid = t0 + rr < rb1;
      __syncthreads();  // every wave is past its reads of the previous tile (and the zeroing, at first)
      ts.xt.store(xb, kLD, tid, dv, [&](int r, int, float x) {
        if (!(fabsf(x) <= 3.4028234663852886e38f)) flag[r] = 1;
        return x;
      });
      ts.fetch(t0, tid, side);

      // margins: Z^T [NC][16 rows of this wave] = T^T U^T
      {
        f64x4 z[KB] = {};
        const float* xr = xb + mrow * kLD + lg;
        const double* tr = Tl + lg * NC + ln;
        for (int s = 0; s < d4; s += 4) {
          double u = (double)xr[s];
          if (QUAD) u -= (double)shl[s + lg];
#pragma unroll
          for (int cb = 0; cb < KB; ++cb)
            z[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[s * NC + 16 * cb], u, z[cb], 0, 0, 0);
          if (QUAD) {
            const double u2 = u * u;
#pragma unroll
            for (int cb = 0; cb < KB; ++cb)
              z[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[(d4 + s) * NC + 16 * cb], u2, z[cb], 0, 0, 0);
          }
        }
#pragma unroll
        for (int cb = 0; cb < KB; ++cb)
#pragma unroll
          for (int v = 0; v < 4; ++v) Zb[mrow * P + 16 * cb + 4 * v + lg] = z[cb][v];
      }
      __syncthreads();

      // top: the four threads of a row, classes qq + 4 j
      {
        const double* zr = Zb + rr * P + qq;
        const bool nonf = flag[rr] != 0;
        double z[NJ], e[NJ];
        double mx = -INFINITY, sum = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int c = qq + 4 * j;
          z[j] = c < C ? zr[4 * j] + gl[c] : -INFINITY;
          mx = fmax(mx, z[j]);
        }
        mx = fmax(mx, __shfl_xor(mx, 1));
        mx = fmax(mx, __shfl_xor(mx, 2));
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          e[j] = qq + 4 * j < C ? exp(z[j] - mx) : 0.0;
          sum += e[j];
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        double best = -1.0;
        int arg = 0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          e[j] /= sum;
          if (qq + 4 * j < C && e[j] > best) best = e[j], arg = qq + 4 * j;
        }
#pragma unroll
        for (int o2 = 1; o2 <= 2; o2 <<= 1) {
          const double ob = __shfl_xor(best, o2);
          const int oa = __shfl_xor(arg, o2);
          if (ob > best || (ob == best && oa < arg)) best = ob, arg = oa;
        }
        if (valid) {
          const int64_t o = (t0 + rr) * C + qq;
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            if (qq + 4 * j < C) {
              raw[o + 4 * j] = nonf ? (double)NAN : z[j];
              prob[o + 4 * j] = nonf ? (double)NAN : e[j];
            }
          if (qq == 0) {
            pred[t0 + rr] = nonf ? 0 : arg;
            cnt[rr] += nonf ? 1 : 0;
          }
        }
      }
      __syncthreads();  // the flags are read
      if (tid < kRows) flag[tid] = 0;
    }
    __syncthreads();
    if (wave == 0) {
      int t = cnt[lane];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
      if (lane == 0 && t > 0) atomicAdd(nbad, t);
    }
  }
}

// One block of 256 threads per 16 output values: out [slot] = the slots' sum.
__global__ __launch_bounds__(256) void nb_reduce_kernel(const double* __restrict__ ws, int nblk, int slot,
                                                        double* __restrict__ out) {
  __shared__ double red[16][16];
  const int idx = blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = idx < slot;
  const double t = sum_blocks(red, nblk, ok, [&](int b) { return ws[(int64_t)b * slot + idx]; });
  if (threadIdx.x < 16 && ok) out[idx] = t;
}

struct NbPlan : RowSplit {
  bool native, vec;
  int KB, per_cu;
  size_t lds;
};

// One round of resident blocks on the 256 CUs: as many per CU as the LDS lets in, and by registers two of the float4
// instantiations (held to 256 registers a lane) and one of the scalar ones; at least 1024 rows per block.
NbPlan nb_plan(const float* X, int64_t n, int64_t ldx, int d, int C, int mode, int quad) {
  NbPlan pl{};
  pl.native = X != nullptr && n >= 1 && d >= 1 && d <= kMaxD && ldx >= d && C >= 2 && C <= kMaxC &&
              (mode == kStats || mode == kPredict) && (quad == 0 || quad == 1);
  if (!pl.native) return pl;
  pl.vec = float4_rows(X, d, ldx);
  pl.KB = (C + 15) / 16;
  pl.lds = mode == kStats ? stats_lds() : predict_lds(d, pl.KB, quad);
  pl.per_cu = (int)(kCuLds / pl.lds);
  if (pl.per_cu > (pl.vec ? 2 : 1)) pl.per_cu = pl.vec ? 2 : 1;
  static_cast<RowSplit&>(pl) = split_rows(n, (int64_t)pl.per_cu * 256);
  return pl;
}

struct NbArgs {
  const float* X;
  int64_t n, ldx;
  const double *y, *wt;
  const float* shift;
  const double *T1, *T2, *g;
  NbParams pr;
  double *ws, *raw, *prob;
  int *pred, *nbad;
};

template <int MODE, int QUAD, int KB, int VW>
int nb_launch(const NbPlan& pl, const NbArgs& a, hipStream_t st) {
  static bool raised[64] = {};
  const int rc = cdna::raise_lds(reinterpret_cast<const void*>(nb_step_kernel<MODE, QUAD, KB, VW>), raised,
                                 MODE == kStats ? stats_lds() : predict_lds(kMaxD, KB, QUAD));
  if (rc != 0) return rc;
  hipLaunchKernelGGL((nb_step_kernel<MODE, QUAD, KB, VW>), dim3(pl.nblk), dim3(256), pl.lds, st, a.X, a.n, a.ldx, a.y,
                     a.wt, a.shift, a.T1, a.T2, a.g, a.pr, a.ws, a.raw, a.prob, a.pred, a.nbad, pl.rows_per_block);
  return (int)hipGetLastError();
}

template <int MODE, int QUAD>
int nb_launch_kv(const NbPlan& pl, const NbArgs& a, hipStream_t st) {
  if (pl.KB == 1) return pl.vec ? nb_launch<MODE, QUAD, 1, 4>(pl, a, st) : nb_launch<MODE, QUAD, 1, 1>(pl, a, st);
  return pl.vec ? nb_launch<MODE, QUAD, 2, 4>(pl, a, st) : nb_launch<MODE, QUAD, 2, 1>(pl, a, st);
}

}  // namespace

static_assert(((size_t)kXF * 4 + kMaxD * 4) % 8 == 0, "the fp64 words of LDS start aligned");
static_assert(predict_lds(kMaxD, 2, 1) <= kCuLds, "the widest block fits a CU");

// What cdna_nb_step runs for these operands (nothing is launched): out = [native, KB (16-class blocks), load width
// (4: float4 rows, 1: scalar), blocks, rows per block, LDS bytes per block, workspace doubles per block (STATS),
// blocks per CU].
CDNA_API int cdna_nb_plan(const float* X, int64_t n, int64_t ldx, int d, int C, int mode, int quad, int64_t* out) {
  const NbPlan pl = nb_plan(X, n, ldx, d, C, mode, quad);
  for (int i = 0; i < 8; ++i) out[i] = 0;
  if (!pl.native) return 0;
  out[0] = 1;
  out[1] = pl.KB;
  out[2] = pl.vec ? 4 : 1;
  out[3] = pl.nblk;
  out[4] = pl.rows_per_block;
  out[5] = (int64_t)pl.lds;
  out[6] = mode == kStats ? slot_doubles(d, C, quad) : 0;
  out[7] = pl.per_cu;
  return 0;
}

// shift [d] f32 or null (zeros).
// STATS (mode 0): y [n] f64 labels, wt [n] f64 row weights or null, rule 0 / 1 / 2 (finite / nonnegative / 0 or 1
// values), out [slot] f64 = [S [C][d] | Q [C][d] (quad) | W [C] | rows with a non-finite value | with a value that
// breaks the rule | with a bad label or weight], ws: blocks x workspace doubles per block of cdna_nb_plan.
// PREDICT (mode 1): T1 (and, quad, T2) [d rounded up to 4][16 ceil(C / 16)] f64, class c in column c, zeros in the
// padding; g [C] f64; raw, prob [n][C] f64, pred [n] int32, nbad [1] int32 zeroed by the caller += the rows with a
// non-finite feature.
CDNA_API int cdna_nb_step(const float* X, int64_t n, int64_t ldx, const double* y, const double* wt,
                          const float* shift, const double* T1, const double* T2, const double* g, int d, int C,
                          int rule, int quad, int mode, double* out, double* ws, double* raw, double* prob, int* pred,
                          int* nbad, hipStream_t st) {
  const NbPlan pl = nb_plan(X, n, ldx, d, C, mode, quad);
  if (!pl.native || rule < kFinite || rule > kBinary) return (int)hipErrorInvalidValue;
  if (mode == kStats && (y == nullptr || out == nullptr || ws == nullptr)) return (int)hipErrorInvalidValue;
  if (mode == kPredict && (T1 == nullptr || g == nullptr || (quad && T2 == nullptr) || raw == nullptr ||
                           prob == nullptr || pred == nullptr || nbad == nullptr))
    return (int)hipErrorInvalidValue;
  const NbArgs a{X, n, ldx, y, wt, shift, T1, T2, g, NbParams{d, C, rule}, ws, raw, prob, pred, nbad};
  if (mode == kPredict) return quad ? nb_launch_kv<kPredict, 1>(pl, a, st) : nb_launch_kv<kPredict, 0>(pl, a, st);
  const int rc = quad ? nb_launch_kv<kStats, 1>(pl, a, st) : nb_launch_kv<kStats, 0>(pl, a, st);
  if (rc != 0) return rc;
  const int slot = slot_doubles(d, C, quad);
  hipLaunchKernelGGL(nb_reduce_kernel, dim3((unsigned)((slot + 15) / 16)), dim3(256), 0, st, ws, pl.nblk, slot, out);
  return (int)hipGetLastError();
}
