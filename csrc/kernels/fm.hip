// K25 fm_step — loss and gradient (or the raw predictions) of a factorization machine in one pass over the rows, on
// the fp32 MFMA.
//
// The model (Spark's FMRegressor / FMClassifier), factors V [d][k], linear weights w [d], intercept b.  Per row:
//   s_f = sum_i v_if x_i,   raw = b + w.x + 1/2 sum_f (s_f^2 - sum_i v_if^2 x_i^2)
//   squared loss (raw - y)^2 with m = 2 (raw - y); logistic loss log1p(exp(-+raw)) with m = sigmoid(raw) - y
//   db = m,  dw_i = m x_i,  dv_if = m (s_f x_i - v_if x_i^2)
//
// fm_step_kernel: 256 threads, 64-row tiles, the next tile of X prefetched in registers (rowblock.h's scaffolding:
// the row split, the tile and its pipeline).  The X tile is row-major fp32 in LDS with the odd row stride kLD, the
// [64][KC] product buffer with the odd stride kSD.
//   X V: w is carried as column k of V (KC = k + 1 columns with linear weights), so S = X [V | w] gives s and w.x
//     from one product on v_mfma_f32_32x32x2_f32.  Wave w forms the 32-row block (w & 1) of column block (w >> 1);
//     its B operand is consecutive floats of the zero-padded fp32 table [d up to 2][KC up to 32] the host prepares.
//   X^2 V^2: only its row sums enter raw, and sum_f sum_i v_if^2 x_i^2 = sum_i x_i^2 u_i with u_i = sum_f v_if^2,
//     which the host prepares in fp64: one dot product per row in place of a second matrix product.  The four
//     threads of a row form it in fp64 from the LDS tile, with sum_f s_f^2, raw, the loss term and m (overflow-free
//     sigmoid and log1p(exp)); a row that is not selected (or past the end) gets m = 0 and adds exactly nothing.
//     They write m s_f (and m itself in column k) back over S, rounded to fp32.
//   gradient: G = X^T (m s | m) [d][KC] is tiled 32x32, the tiles dealt round-robin to the 4 waves (SLOTS per
//     wave); both operands are consecutive floats of one LDS row (symtile.h's mfma_rows pattern with two buffers).
//     fp32 accumulators in registers for kFoldTiles tiles, then folded into the block's fp64 slab (each element
//     owned by one lane).  c_i = sum_r m_r x_ri^2: fp64 column sums, one thread per (column, row half).
// fm_reduce_kernel: slabs, column sums, loss, sum of m and count of the blocks in a fixed order in fp64 (rowblock.h's
// sum_blocks), straight into the flat layout: dV_if = G_if - v_if c_i, dw_i = G_ik, db = sum m.  No float atomics on
// global memory: reruns are bit-identical.
// Row selection (miniBatchFraction): row r is in when philox_uniform(seed, row_offset + r, stream) < frac, drawn here.
// Native range: d <= 128, k <= 32.
#include "symtile.h"

namespace {

using namespace symtile;

constexpr int kMaxK = 32;
constexpr int kSD = 2 * 32 + 1;      // the product buffer: up to 2 column blocks, odd like kLD
constexpr int kSF = kRows * kSD;     // its floats
constexpr int kFoldTiles = 8;        // 512 rows of fp32 accumulation between folds into the fp64 slab
// fp64 words of LDS behind the two buffers: u [kMaxD], per tile row m, loss, sum of m; then the rows' counts (int).
// 52.5 KB in all: three blocks share a CU's 160 KB
constexpr int kRedD = kMaxD + 3 * kRows;
// per block of the workspace behind the slabs: c [kMaxD], loss, sum of m, count (+ 1 pad)
constexpr int kTail = kMaxD + 4;

enum { kStep = 0, kPredict = 1 };
enum { kSquared = 0, kLogistic = 1 };

struct FmShape {
  int d, k, kc;        // kc: k + 1 with linear weights
  int Td, Tc, ldw;     // 32-tiles of d and of kc; ldw = 32 Tc: the table's row length
  int fit_linear, fit_intercept, loss;
  int P;
};

__host__ __device__ __forceinline__ int up(int v, int m) { return (v + m - 1) / m * m; }

FmShape make_shape(int d, int k, int fit_linear, int fit_intercept, int loss) {
  FmShape s{};
  s.d = d;
  s.k = k;
  s.kc = k + (fit_linear ? 1 : 0);
  s.Td = up(d, 32) / 32;
  s.Tc = up(s.kc, 32) / 32;
  s.ldw = 32 * s.Tc;
  s.fit_linear = fit_linear;
  s.fit_intercept = fit_intercept;
  s.loss = loss;
  s.P = d * k + (fit_linear ? d : 0) + (fit_intercept ? 1 : 0);
  return s;
}

struct FmSample {
  int on;              // 0: every row
  uint32_t stream;
  uint64_t seed;
  int64_t row_offset;
  double frac;
};

// The value is what it was, but the compiler no longer knows where it came from (see mlp.hip).
__device__ __forceinline__ void opaque(int& v) { asm volatile("" : "+v"(v)); }

__host__ __device__ __forceinline__ int64_t block_doubles(int tiles) { return (int64_t)tiles * 1024 + kTail; }

// SLOTS: gradient tiles per wave (0: PREDICT); VW = 4: float4 row loads, VW = 1: scalar loads, any layout.
template <int SLOTS, int VW>
__global__ __launch_bounds__(256) void fm_step_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const double* __restrict__ y, const float* __restrict__ tab,
    const double* __restrict__ u, double b0, const FmShape sh, const FmSample smp, double* __restrict__ ws,
    double* __restrict__ raw, int64_t rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xb = reinterpret_cast<float*>(smem);
  float* sb = xb + kXF;
  double* red = reinterpret_cast<double*>(smem + (size_t)(kXF + kSF) * 4);
  double* uL = red;                    // [kMaxD]
  double* mrow = red + kMaxD;          // [kRows] this tile's m
  double* lsum = mrow + kRows;         // [kRows] running loss of the tile row
  double* msum = lsum + kRows;         // [kRows] running sum of m
  int* cnt = reinterpret_cast<int*>(msum + kRows);  // [kRows] running count of selected rows (< 2^31 per block)
  constexpr bool kTrain = SLOTS > 0;
  constexpr int NS = kTrain ? SLOTS : 1;
  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = sh.d, dv = d / VW, k = sh.k;
  const int NT = sh.Td * sh.Tc;

  for (int i = tid; i < kRedD; i += 256) red[i] = i < kMaxD ? u[i] : 0.0;
  if (tid < kRows) cnt[tid] = 0;
  double cacc = 0.0;  // c_i of column tid & 127 over the row half tid >> 7, summed over the block's tiles

  f32x16 acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[s][e] = 0.f;

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  double* myws = ws != nullptr ? ws + (int64_t)blockIdx.x * block_doubles(NT) : nullptr;
  double yv = 0.0;
  bool first = true;
  int pending = 0;
  // the row's y travels with its tile
  const auto side = [&](int64_t t, int i) {
    if (kTrain && t + (i >> 2) < rb1) yv = y[t + (i >> 2)];
  };
  TileStream<VW> ts;
  // both buffers are zeroed: column d of the X tile is read when d is odd
  ts.begin(xb, kXF + kSF, X, ldx, rb0, rb1, dv, tid, side);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    const bool more = t0 + kRows < rb1;
    int tl = tid;
    opaque(tl);
    const int lane = tl & 63, rr = tl >> 2, qq = tl & 3, bc = tl & (kMaxD - 1), bh = tl >> 7;
    const bool valid = t0 + rr < rb1;
    const double lab = yv;
    ts.put(xb, tl);
    ts.fetch(t0, tl, side);

    // S = X [V | w]
    {
      const int rb = wid & 1, cb = wid >> 1;
      if (cb < sh.Tc) {
        int ml = lane;
        opaque(ml);
        const int half = ml >> 5, col = ml & 31;
        f32x16 a0;
#pragma unroll
        for (int e = 0; e < 16; ++e) a0[e] = 0.f;
        const float* ap = xb + (32 * rb + col) * kLD + half;
        const float* bp = tab + half * sh.ldw + 32 * cb + col;
        const int kd = up(d, 2), ldw = sh.ldw;
        // 8 k-steps' operand loads (LDS, and the table through L2) are in flight
        int m = 0;
        for (; m + 16 <= kd; m += 16)
#pragma unroll
          for (int q = 0; q < 16; q += 2)
            a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[m + q], bp[(m + q) * ldw], a0, 0, 0, 0);
        for (; m < kd; m += 2) a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[m], bp[m * ldw], a0, 0, 0, 0);
        float* dst = sb + (32 * rb) * kSD + 32 * cb + col;
#pragma unroll
        for (int e = 0; e < 16; ++e) dst[acc_row(e, half) * kSD] = a0[e];
      }
    }
    __syncthreads();

    // top: raw, the loss term and m in fp64, four threads per row
    {
      const float* xr = xb + rr * kLD;
      float* sr = sb + rr * kSD;
      double ss = 0.0, tt = 0.0;
      for (int f = qq; f < k; f += 4) {
        const double s = (double)sr[f];
        ss += s * s;
      }
      for (int i = qq; i < d; i += 4) {
        const double x = (double)xr[i];
        tt += (x * x) * uL[i];
      }
      double part = 0.5 * (ss - tt);
      part += __shfl_xor(part, 1);
      part += __shfl_xor(part, 2);
      const double rw = b0 + (sh.fit_linear ? (double)sr[k] : 0.0) + part;
      if (kTrain) {
        bool sel = valid;
        if (sel && smp.on)
          sel = cdna::philox_uniform(smp.seed, (uint64_t)(smp.row_offset + t0 + rr), smp.stream) < smp.frac;
        double loss, m;
        if (sh.loss == kSquared) {
          const double r = rw - lab;
          loss = r * r;
          m = 2.0 * r;
        } else {
          const double e = exp(-fabs(rw));
          const double sg = rw >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
          const double z = lab > 0.0 ? -rw : rw;
          loss = (z > 0.0 ? z : 0.0) + log1p(e);
          m = sg - lab;
        }
        if (!sel) loss = m = 0.0;
        if (qq == 0) {
          mrow[rr] = m;
          lsum[rr] += loss;
          msum[rr] += m;
          cnt[rr] += sel ? 1 : 0;
        }
        for (int f = qq; f < k; f += 4) sr[f] = sel ? (float)(m * (double)sr[f]) : 0.f;
        if (sh.fit_linear && qq == 0) sr[k] = (float)m;
      } else if (valid && qq == 0) {
        raw[t0 + rr] = rw;
      }
    }
    if (!kTrain) continue;
    __syncthreads();  // m and m s complete

    // G += X^T (m s | m) over the tile's rows
    {
      int gl = lane;
      opaque(gl);
      const int goff = gl >> 5, gcol = gl & 31;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int t = wid + 4 * s;
        if (t >= NT) continue;
        const int tc = t >= sh.Td ? 1 : 0, ti = t - tc * sh.Td;  // Tc <= 2
        const float* a = xb + goff * kLD + 32 * ti + gcol;
        const float* b = sb + goff * kSD + 32 * tc + gcol;
#pragma unroll 4
        for (int r = 0; r < kRows; r += 2)
          acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r * kLD], b[r * kSD], acc[s], 0, 0, 0);
      }
      // c_i += sum_r m_r x_ri^2
      if (bc < d) {
        const float* xc = xb + (32 * bh) * kLD + bc;
        const double* mr = mrow + 32 * bh;
        double c = 0.0;
#pragma unroll 8
        for (int r = 0; r < 32; ++r) {
          const double x = (double)xc[r * kLD];
          c += mr[r] * (x * x);
        }
        cacc += c;
      }
    }

    if (++pending == kFoldTiles || !more) {
      int fl = lane;
      opaque(fl);
      const int fi = acc_row(0, fl >> 5) * 32 + (fl & 31);  // element e is 32 (acc_row(e, 0)) floats further
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (wid + 4 * s >= NT) continue;
        double* slab = myws + (int64_t)(wid + 4 * s) * 1024;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = fi + acc_row(e, 0) * 32;
          const double v = (double)acc[s][e];
          slab[i] = first ? v : slab[i] + v;
          acc[s][e] = 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);  // one slab's 16 loads in flight, not every slab's
      }
      first = false;
      pending = 0;
    }
  }

  if (!kTrain) return;
  __syncthreads();  // the last tile's reads of mrow are done: the upper row half's column sums go over it and lsum
  double* tail = myws + (int64_t)NT * 1024;
  double a = 0.0, b = 0.0, c = 0.0;
  if (tid >= 192) {  // wave 3: the 64 rows' loss, m and count sums in a fixed order
    const int l = tid - 192;
    a = cdna::wave_sum(lsum[l]);
    b = cdna::wave_sum(msum[l]);
    c = cdna::wave_sum((double)cnt[l]);
  }
  __syncthreads();
  if (tid >= kMaxD) mrow[tid - kMaxD] = cacc;  // [kMaxD] doubles: mrow and lsum
  __syncthreads();
  if (tid < kMaxD) tail[tid] = cacc + mrow[tid];
  if (tid == 192) {
    tail[kMaxD] = a;
    tail[kMaxD + 1] = b;
    tail[kMaxD + 2] = c;
  }
}

// One block of 256 threads per 16 output values, summed over the blocks (a slab element together with the column sum
// c_i it is corrected by); the value goes to its place in out [P + 2]: the flat gradient, the loss, the count.
__global__ __launch_bounds__(256) void fm_reduce_kernel(const double* __restrict__ ws, int nblk, const FmShape sh,
                                                        const float* __restrict__ tab, double* __restrict__ out) {
  __shared__ double red[2][16][16];
  const int NT = sh.Td * sh.Tc;
  const int64_t stride = block_doubles(NT);
  const int64_t slabs = (int64_t)NT * 1024, total = slabs + 3;
  const int64_t idx = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = idx < total;
  const bool slab = idx < slabs;
  int i = 0, f = 0;
  int64_t src = idx;
  if (slab) {
    const int tile = (int)(idx >> 10), e = (int)(idx & 1023);
    const int tc = tile >= sh.Td ? 1 : 0, ti = tile - tc * sh.Td;
    i = 32 * ti + (e >> 5);
    f = 32 * tc + (e & 31);
  } else {
    src = slabs + kMaxD + (idx - slabs);
  }
  double tt[2];  // the value, and for a slab element the column sum c_i
  sum_blocks(red, nblk, ok, tt, [&](int b, double* s) {
    s[0] += ws[(int64_t)b * stride + src];
    if (slab) s[1] += ws[(int64_t)b * stride + slabs + i];
  });
  if (threadIdx.x >= 16 || !ok) return;
  const double t = tt[0], ct = tt[1];
  if (slab) {
    if (i >= sh.d) return;
    if (f < sh.k)
      out[(int64_t)i * sh.k + f] = t - (double)tab[i * sh.ldw + f] * ct;
    else if (f == sh.k && sh.fit_linear)
      out[sh.d * sh.k + i] = t;
  } else {
    const int r = (int)(idx - slabs);  // 0 loss, 1 sum of m, 2 count
    if (r == 0) out[sh.P] = t;
    if (r == 1 && sh.fit_intercept) out[sh.P - 1] = t;
    if (r == 2) out[sh.P + 1] = t;
  }
}

struct FmPlan : RowSplit {
  bool native;
  int slots;  // gradient tiles per wave of the STEP instantiation
  size_t lds;
};

// One round of resident blocks on the 256 CUs: three per CU by LDS (52.5 KB each) and registers, two for the STEP
// instantiation with two gradient tiles per wave (202 registers per lane).
FmPlan fm_plan(int64_t n, int d, int k, int fit_linear, bool step = true) {
  FmPlan pl{};
  pl.native = n >= 1 && d >= 1 && d <= kMaxD && k >= 1 && k <= kMaxK;
  if (!pl.native) return pl;
  const FmShape sh = make_shape(d, k, fit_linear, 0, 0);
  pl.slots = sh.Td * sh.Tc <= 4 ? 1 : 2;
  static_cast<RowSplit&>(pl) = split_rows(n, step && pl.slots == 2 ? 2 * 256 : 3 * 256);
  pl.lds = (size_t)(kXF + kSF) * 4 + (size_t)kRedD * 8 + kRows * 4;
  return pl;
}

template <int SLOTS, int VW>
int step_launch(const FmPlan& pl, const FmShape& sh, const FmSample& smp, const float* X, int64_t n, int64_t ldx,
                const double* y, const float* tab, const double* u, double b0, double* ws, double* raw,
                hipStream_t st) {
  hipLaunchKernelGGL((fm_step_kernel<SLOTS, VW>), dim3(pl.nblk), dim3(256), pl.lds, st, X, n, ldx, y, tab, u, b0, sh,
                     smp, ws, raw, pl.rows_per_block);
  return (int)hipGetLastError();
}

template <int VW>
int step_launch_slots(int slots, const FmPlan& pl, const FmShape& sh, const FmSample& smp, const float* X, int64_t n,
                      int64_t ldx, const double* y, const float* tab, const double* u, double b0, double* ws,
                      double* raw, hipStream_t st) {
  switch (slots) {
    case 0: return step_launch<0, VW>(pl, sh, smp, X, n, ldx, y, tab, u, b0, ws, raw, st);
    case 1: return step_launch<1, VW>(pl, sh, smp, X, n, ldx, y, tab, u, b0, ws, raw, st);
    default: return step_launch<2, VW>(pl, sh, smp, X, n, ldx, y, tab, u, b0, ws, raw, st);
  }
}

}  // namespace

static_assert((size_t)(kXF + kSF) * 4 % 8 == 0, "the fp64 words of LDS start 8-byte aligned");
static_assert((size_t)(kXF + kSF) * 4 + (size_t)kRedD * 8 + kRows * 4 <= 53248, "three blocks per CU");

// What cdna_fm_step runs for these operands (nothing is launched): out = [native, gradient tiles per wave, load
// width (4: float4 rows, 1: scalar), blocks and rows per block of a STEP, gradient tiles, LDS bytes, table floats,
// table row length, rows between folds].
CDNA_API int cdna_fm_plan(const float* X, int64_t n, int64_t ldx, int d, int k, int fit_linear, int64_t* out) {
  const FmPlan pl = fm_plan(n, d, k, fit_linear);
  for (int i = 0; i < 10; ++i) out[i] = 0;
  if (!pl.native || ldx < d) return 0;
  const FmShape sh = make_shape(d, k, fit_linear, 0, 0);
  out[0] = 1;
  out[1] = pl.slots;
  out[2] = float4_rows(X, d, ldx) ? 4 : 1;
  out[3] = pl.nblk;
  out[4] = pl.rows_per_block;
  out[5] = sh.Td * sh.Tc;
  out[6] = (int64_t)pl.lds;
  out[7] = (int64_t)up(d, 2) * sh.ldw;
  out[8] = sh.ldw;
  out[9] = kFoldTiles * kRows;
  return 0;
}

// Workspace of a STEP in doubles: per block the gradient slabs, the column sums, the loss, the sum of m, the count.
CDNA_API int64_t cdna_fm_step_workspace(int64_t n, int d, int k, int fit_linear) {
  const FmPlan pl = fm_plan(n, d, k, fit_linear);
  if (!pl.native) return 0;
  const FmShape sh = make_shape(d, k, fit_linear, 0, 0);
  return (int64_t)pl.nblk * block_doubles(sh.Td * sh.Tc);
}

// tab: fp32 [d up to 2][out[8] of cdna_fm_plan], row i = v_i0 .. v_i(k-1), then w_i with linear weights, zeros
// elsewhere; u [128] f64: u_i = sum_f v_if^2 (zeros from d on); b0: the intercept.
// STEP: y [n] f64, out [P + 2] f64 (the flat gradient sum, the loss sum, the count of selected rows), ws:
// cdna_fm_step_workspace doubles; use_sample != 0: row r is selected when philox_uniform(seed, row_offset + r,
// stream) < frac.  PREDICT: raw [n] f64.
CDNA_API int cdna_fm_step(const float* X, int64_t n, int64_t ldx, const double* y, const float* tab, const double* u,
                          double b0, int d, int k, int fit_linear, int fit_intercept, int loss, int mode,
                          int use_sample, uint64_t seed, int64_t row_offset, double frac, uint32_t stream, double* out,
                          double* ws, double* raw, hipStream_t st) {
  const FmPlan pl = fm_plan(n, d, k, fit_linear, mode == kStep);
  if (!pl.native || ldx < d || X == nullptr || tab == nullptr || u == nullptr) return (int)hipErrorInvalidValue;
  if (mode != kStep && mode != kPredict) return (int)hipErrorInvalidValue;
  if (loss != kSquared && loss != kLogistic) return (int)hipErrorInvalidValue;
  if (mode == kStep && (y == nullptr || out == nullptr || ws == nullptr)) return (int)hipErrorInvalidValue;
  if (mode == kPredict && raw == nullptr) return (int)hipErrorInvalidValue;
  const FmShape sh = make_shape(d, k, fit_linear, fit_intercept, loss);
  const FmSample smp{use_sample != 0 && frac < 1.0 ? 1 : 0, stream, seed, row_offset, frac};
  const bool vec = float4_rows(X, d, ldx);
  const int slots = mode == kStep ? pl.slots : 0;
  const int rc = vec ? step_launch_slots<4>(slots, pl, sh, smp, X, n, ldx, y, tab, u, b0, ws, raw, st)
                     : step_launch_slots<1>(slots, pl, sh, smp, X, n, ldx, y, tab, u, b0, ws, raw, st);
  if (rc != 0 || mode == kPredict) return rc;
  const int64_t total = (int64_t)sh.Td * sh.Tc * 1024 + 3;
  hipLaunchKernelGGL(fm_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, ws, pl.nblk, sh, tab,
                     out);
  return (int)hipGetLastError();
}
