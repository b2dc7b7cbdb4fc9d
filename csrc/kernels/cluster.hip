// K30 cluster_step — one k-means step (nearest centre, weighted centre sums, weight sums, cost), or the assignment
// alone, in one pass over the rows, on the fp32 MFMA and without atomics.
//
// The distance of row r to centre j is the affine form D[r][j] = alpha |x~_r|^2 + x~_r . Y_j + gamma_j over the
// transformed row x~ and three tables the host prepares per call:
//   Euclidean: x~ = x - shift (a caller-supplied fp32 vector: distances do not depend on it, and near the data it
//              takes the cancellation out of the expanded form), alpha = 1, Y_j = -2 c~_j, gamma_j = |c~_j|^2 with
//              c~_j = fl32(c_j - shift), so D = |x~ - c~_j|^2.
//   cosine:    x~ = x / max(|x|, 1e-30), alpha = 0, Y_j = -c^_j, gamma_j = 1, so D = 1 - cos(x, c_j).
//
// cluster_step_kernel: 256 threads, 64-row tiles, the next tile of X prefetched in registers (rowblock.h's row split,
// tile and pipeline).  The tile is row-major fp32 in LDS at stride kLD, transformed on its way in (the shift) or by
// the row's four threads right after (the norm, |x|^2 in fp64).  Per tile:
//   score:  S = X~ Y^T on v_mfma_f32_32x32x2_f32, the 2 x Tk output tiles dealt to the 4 waves; the A operand comes
//           from the LDS tile, the B operand is consecutive floats of the zero-padded, L2-resident fp32 table
//           [d up to 2][k up to 32]; S goes to an LDS buffer [64][32 Tk + 1].
//   argmin: four threads per row form |x~|^2 in fp64 (32 columns each, staggered starts), then D in fp64 over a
//           quarter of the columns each, and combine by lane shuffles.  K10's and torch.min's rules: the lowest index
//           among equal distances, the first NaN wins and stays, centre 0 when every distance is +inf.  A row whose
//           |x~|^2 is NaN or >= 2^120 (a non-finite feature, or one that would overflow the fp32 products) is bad:
//           centre 0, distance NaN or +inf, counted, and it adds exactly nothing to the sums.
//   sums:   the four threads write A[r][j] = fl32(w_r) [j = a_r] over the row of S (zero rows past the end and for bad
//           rows, whose tile row is zeroed too); A^T X~ [k][d] is tiled 32 x 32, the tiles dealt round-robin to the
//           waves (SLOTS each), both operands consecutive floats of one LDS row (symtile.h's mfma_rows pattern with
//           two buffers).  fp32 accumulators for kFoldTiles tiles, then folded into the block's fp64 slab (each
//           element owned by one lane).  N_j = sum of w over the rows of centre j: thread j, fp64, tile-row order.
// cluster_reduce_kernel: slabs, N, cost and bad count of the blocks summed in a fixed order in fp64 (rowblock.h's
// sum_blocks).  No float atomics: reruns at the same grid are bit-identical.
// Native range: fp32 rows, d <= 128, k <= 128.
#include <climits>

#include "symtile.h"

namespace {

using namespace symtile;

constexpr int kMaxK = 128;
constexpr int kFoldTiles = 8;     // 512 rows of fp32 accumulation between folds into the fp64 slab
constexpr double kBadQ = 0x1p120; // |x~|^2 from here on (or NaN): a bad row
// LDS in front of the two buffers: gamma [kMaxK], the tile rows' weights [kRows] and the waves' final sums [8] in
// fp64, then shift [kMaxD] fp32 and the tile rows' centres [kRows] int
constexpr size_t kHeadBytes = (size_t)(kMaxK + kRows + 8) * 8 + kMaxD * 4 + kRows * 4;
// per block of the workspace behind the slabs: cost, bad count, 2 pads, then N [kMaxK] (STEP only)
constexpr int kTail = 4;

enum { kStep = 0, kPredict = 1 };

struct ClShape {
  int d, k;
  int Td, Tk, ldw;  // 32-tiles of d and of k; ldw = 32 Tk: the table's row length
  int sd;           // row stride of the S / A buffer: ldw + 1, odd like kLD
  int cosine;
};

__host__ __device__ __forceinline__ int up(int v, int m) { return (v + m - 1) / m * m; }

ClShape make_shape(int d, int k, int cosine) {
  ClShape s{};
  s.d = d;
  s.k = k;
  s.Td = up(d, 32) / 32;
  s.Tk = up(k, 32) / 32;
  s.ldw = 32 * s.Tk;
  s.sd = s.ldw + 1;
  s.cosine = cosine;
  return s;
}

// The value is what it was, but the compiler no longer knows where it came from (see mlp.hip).
__device__ __forceinline__ void opaque(int& v) { asm volatile("" : "+v"(v)); }

__host__ __device__ __forceinline__ int64_t block_doubles(int tiles, bool sums) {
  return sums ? (int64_t)tiles * 1024 + kTail + kMaxK : kTail;
}

// SLOTS: sum tiles per wave (0: PREDICT); VW = 4: float4 row loads, VW = 1: scalar loads, any layout.
template <int SLOTS, int VW>
__global__ __launch_bounds__(256) void cluster_step_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const double* __restrict__ w, const float* __restrict__ tab,
    const double* __restrict__ gamma, const float* __restrict__ shift, const ClShape sh, int* __restrict__ assign,
    double* __restrict__ ws, int64_t rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* gam = reinterpret_cast<double*>(smem);  // [kMaxK]
  double* wrow = gam + kMaxK;                     // [kRows] this tile's weights
  double* fin = wrow + kRows;                     // [8] the waves' cost and bad count
  float* shf = reinterpret_cast<float*>(fin + 8); // [kMaxD]
  int* arow = reinterpret_cast<int*>(shf + kMaxD);  // [kRows] this tile's centres, -1: the row adds nothing
  float* xb = reinterpret_cast<float*>(arow + kRows);
  float* sb = xb + kXF;
  constexpr bool kSums = SLOTS > 0;
  constexpr int NS = kSums ? SLOTS : 1;
  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = sh.d, dv = d / VW, k = sh.k, sd = sh.sd;
  const int NT = sh.Td * sh.Tk;

  if (tid < kMaxK) {  // kMaxK == kMaxD: both tables arrive zero-padded
    gam[tid] = gamma[tid];
    shf[tid] = shift[tid];
  }
  double nacc = 0.0;  // N_j of centre tid
  double cacc = 0.0;  // cost and bad count of tile row tid >> 2, in its first thread
  double bacc = 0.0;

  f32x16 acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[s][e] = 0.f;

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  double* myws = ws + (int64_t)blockIdx.x * block_doubles(NT, kSums);
  double wv = 1.0;
  bool first = true;
  int pending = 0;
  // the row's weight travels with its tile
  const auto side = [&](int64_t t, int i) {
    if (w != nullptr && t + (i >> 2) < rb1) wv = w[t + (i >> 2)];
  };
  TileStream<VW> ts;
  // both buffers are zeroed: column d of the X tile is read when d is odd
  ts.begin(xb, kXF + kRows * sd, X, ldx, rb0, rb1, dv, tid, side);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    const bool more = t0 + kRows < rb1;
    int tl = tid;
    opaque(tl);
    const int lane = tl & 63, rr = tl >> 2, qq = tl & 3;
    const int lim = rb1 - t0 < kRows ? (int)(rb1 - t0) : kRows;
    const bool valid = rr < lim;
    const double wr = wv;
    // TileStream's put with the shift: x~ = x - shift (zeros for the cosine), rows past the end stay zero
    __syncthreads();
    ts.xt.store(xb, kLD, tl, dv, [&](int r, int c, float x) { return r < lim ? x - shf[c] : 0.f; });
    ts.fetch(t0, tl, side);

    // |x~|^2 in fp64, four threads per row
    float* xq = xb + rr * kLD + 32 * qq;
    const bool mine = 32 * qq < d;
    double q = 0.0;
    if (mine) {
#pragma unroll 8
      for (int j = 0; j < 32; ++j) {
        const double x = (double)xq[(j + 8 * qq) & 31];
        q = fma(x, x, q);
      }
    }
    q += __shfl_xor(q, 1);
    q += __shfl_xor(q, 2);
    const bool bad = !(q < kBadQ);
    if (sh.cosine) {
      const double inv = 1.0 / fmax(sqrt(q), 1e-30);
      if (mine && !bad) {
#pragma unroll 8
        for (int j = 0; j < 32; ++j) xq[j] = (float)((double)xq[j] * inv);
      }
      __syncthreads();
    }

    // S = X~ Y^T
    for (int t = wid; t < 2 * sh.Tk; t += 4) {
      const int rb = t & 1, cb = t >> 1;
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
        for (int u = 0; u < 16; u += 2)
          a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[m + u], bp[(m + u) * ldw], a0, 0, 0, 0);
      for (; m < kd; m += 2) a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[m], bp[m * ldw], a0, 0, 0, 0);
      float* dst = sb + (32 * rb) * sd + 32 * cb + col;
#pragma unroll
      for (int e = 0; e < 16; ++e) dst[acc_row(e, half) * sd] = a0[e];
    }
    __syncthreads();

    // argmin over the row's D, a quarter of the columns per thread
    float* sr = sb + rr * sd;
    double best = INFINITY;
    int bi = INT_MAX;
    {
      const int kq = (k + 3) >> 2, j0 = qq * kq, j1 = j0 + kq < k ? j0 + kq : k;
      const double aq = sh.cosine ? 0.0 : q;
      for (int j = j0; j < j1; ++j) {
        const double dj = aq + (double)sr[j] + gam[j];
        if (dj < best || (dj != dj && best == best)) {
          best = dj;
          bi = j;
        }
      }
#pragma unroll
      for (int o = 1; o <= 2; o <<= 1) {
        const double od = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        // of the two candidates the one with the lower index stays, unless the other is smaller, or NaN while it
        // is not
        const bool later = bi > oi;
        const double ed = later ? od : best, ld = later ? best : od;
        const int ei = later ? oi : bi, li = later ? bi : oi;
        const bool take = ld < ed || (ld != ld && ed == ed);
        best = take ? ld : ed;
        bi = take ? li : ei;
      }
      if (bi == INT_MAX) bi = 0;  // every distance +inf
      if (bad) {
        bi = 0;
        best = q != q ? q : (double)INFINITY;
      }
      if (!sh.cosine && best < 0.0) best = 0.0;  // a NaN stays
    }
    if (valid && qq == 0) {
      cacc += wr * best;
      bacc += bad ? 1.0 : 0.0;
      if (assign != nullptr) assign[t0 + rr] = bi;
    }
    if (!kSums) continue;

    // A over S: the row's weight in the column of its centre
    {
      const bool live = valid && !bad;
      const float wa = live ? (float)wr : 0.f;
      const int nc = 8 * sh.Tk, c0 = nc * qq;
      for (int j = 0; j < nc; ++j) sr[c0 + j] = c0 + j == bi ? wa : 0.f;
      if (qq == 0) {
        arow[rr] = live ? bi : -1;
        wrow[rr] = wr;
      }
      if (valid && bad && mine) {
#pragma unroll 8
        for (int j = 0; j < 32; ++j) xq[j] = 0.f;
      }
    }
    __syncthreads();

    // sums += A^T X~ over the tile's rows
    {
      int gl = lane;
      opaque(gl);
      const int goff = gl >> 5, gcol = gl & 31;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int t = wid + 4 * s;
        if (t >= NT) continue;
        const int tj = t / sh.Td, ti = t - tj * sh.Td;
        const float* a = sb + goff * sd + 32 * tj + gcol;
        const float* b = xb + goff * kLD + 32 * ti + gcol;
#pragma unroll 4
        for (int r = 0; r < kRows; r += 2)
          acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r * sd], b[r * kLD], acc[s], 0, 0, 0);
      }
      // N_j += the weights of centre j's rows
      if (tl < k) {
#pragma unroll 8
        for (int r = 0; r < kRows; ++r) nacc += arow[r] == tl ? wrow[r] : 0.0;
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

  // the 64 rows' cost and bad count in a fixed order: the waves' sums, then the four of them
  double* tail = myws + (kSums ? (int64_t)NT * 1024 : 0);
  const double cw = cdna::wave_sum(cacc), bw = cdna::wave_sum(bacc);
  if ((tid & 63) == 0) {
    fin[wid] = cw;
    fin[4 + wid] = bw;
  }
  __syncthreads();
  if (tid == 0) {
    tail[0] = ((fin[0] + fin[1]) + fin[2]) + fin[3];
    tail[1] = ((fin[4] + fin[5]) + fin[6]) + fin[7];
    tail[2] = tail[3] = 0.0;
  }
  if (kSums && tid < kMaxK) tail[kTail + tid] = nacc;
}

// One block of 256 threads per 16 output values, summed over the blocks; the value goes to its place in out: STEP
// [k d sums, k N, cost, bad count], PREDICT [cost, bad count].
__global__ __launch_bounds__(256) void cluster_reduce_kernel(const double* __restrict__ ws, int nblk, const ClShape sh,
                                                             int sums, double* __restrict__ out) {
  __shared__ double red[16][16];
  const int NT = sh.Td * sh.Tk;
  const int64_t stride = block_doubles(NT, sums != 0);
  const int64_t idx = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = idx < stride;
  const double t = sum_blocks(red, nblk, ok, [&](int b) { return ws[(int64_t)b * stride + idx]; });
  if (threadIdx.x >= 16 || !ok) return;
  const int64_t slabs = sums ? (int64_t)NT * 1024 : 0;
  const int64_t base = sums ? (int64_t)sh.k * sh.d + sh.k : 0;
  if (idx < slabs) {
    const int tile = (int)(idx >> 10), e = (int)(idx & 1023);
    const int tj = tile / sh.Td, ti = tile - tj * sh.Td;
    const int j = 32 * tj + (e >> 5), i = 32 * ti + (e & 31);
    if (j < sh.k && i < sh.d) out[(int64_t)j * sh.d + i] = t;
  } else {
    const int r = (int)(idx - slabs);  // 0 cost, 1 bad count, 2 and 3 pads, then N
    if (r < 2) out[base + r] = t;
    if (r >= kTail && r - kTail < sh.k) out[(int64_t)sh.k * sh.d + (r - kTail)] = t;
  }
}

struct ClPlan : RowSplit {
  bool native;
  int slots;  // sum tiles per wave of the STEP instantiation
  int bpc;    // blocks per CU of the one round
  size_t lds;
};

size_t lds_bytes(int sd) { return kHeadBytes + (size_t)(kXF + kRows * sd) * 4; }

// One round of resident blocks on the 256 CUs.  Per CU the 160 KB of LDS hold 3 blocks up to k = 64 and 2 beyond;
// registers admit 3 for PREDICT and for STEP with one sum tile per wave on float4 rows (at most 139 per lane), and 2
// for every other instantiation (at most 248).
ClPlan cl_plan(int64_t n, int d, int k, int mode, bool vec) {
  ClPlan pl{};
  pl.native = n >= 1 && d >= 1 && d <= kMaxD && k >= 1 && k <= kMaxK;
  if (!pl.native) return pl;
  const ClShape sh = make_shape(d, k, 0);
  const int NT = sh.Td * sh.Tk;
  pl.slots = NT <= 4 ? 1 : (NT <= 8 ? 2 : 4);
  pl.lds = lds_bytes(sh.sd);
  pl.bpc = (int)((size_t)160 * 1024 / pl.lds);
  const int by_regs = vec && (mode == kPredict || pl.slots == 1) ? 3 : 2;
  if (pl.bpc > by_regs) pl.bpc = by_regs;
  static_cast<RowSplit&>(pl) = split_rows(n, (int64_t)pl.bpc * 256);
  return pl;
}

template <int SLOTS, int VW>
int step_launch(const ClPlan& pl, const ClShape& sh, const float* X, int64_t n, int64_t ldx, const double* w,
                const float* tab, const double* gamma, const float* shift, int* assign, double* ws, hipStream_t st) {
  if (pl.lds > 64 * 1024) {
    static bool raised[64] = {};
    const int rc = cdna::raise_lds(reinterpret_cast<const void*>(cluster_step_kernel<SLOTS, VW>), raised,
                                   lds_bytes(kMaxK + 1));
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL((cluster_step_kernel<SLOTS, VW>), dim3(pl.nblk), dim3(256), pl.lds, st, X, n, ldx, w, tab, gamma,
                     shift, sh, assign, ws, pl.rows_per_block);
  return (int)hipGetLastError();
}

template <int VW>
int step_launch_slots(int slots, const ClPlan& pl, const ClShape& sh, const float* X, int64_t n, int64_t ldx,
                      const double* w, const float* tab, const double* gamma, const float* shift, int* assign,
                      double* ws, hipStream_t st) {
  switch (slots) {
    case 0: return step_launch<0, VW>(pl, sh, X, n, ldx, w, tab, gamma, shift, assign, ws, st);
    case 1: return step_launch<1, VW>(pl, sh, X, n, ldx, w, tab, gamma, shift, assign, ws, st);
    case 2: return step_launch<2, VW>(pl, sh, X, n, ldx, w, tab, gamma, shift, assign, ws, st);
    default: return step_launch<4, VW>(pl, sh, X, n, ldx, w, tab, gamma, shift, assign, ws, st);
  }
}

}  // namespace

static_assert(kMaxK == kMaxD, "one guard loads gamma and shift");
static_assert(kHeadBytes % 16 == 0, "the tile starts 16-byte aligned");
static_assert(kHeadBytes + (size_t)(kXF + kRows * (kMaxK + 1)) * 4 <= 80 * 1024, "two blocks per CU at k = 128");

// What cdna_cluster_step runs for these operands (nothing is launched): out = [native, sum tiles per wave of a STEP,
// load width (4: float4 rows, 1: scalar), blocks, rows per block, sum tiles, LDS bytes, table floats, table row
// length, rows between folds, blocks per CU, workspace doubles of this mode].
CDNA_API int cdna_cluster_plan(const float* X, int64_t n, int64_t ldx, int d, int k, int mode, int64_t* out) {
  const ClPlan pl = cl_plan(n, d, k, mode, float4_rows(X, d, ldx));
  for (int i = 0; i < 12; ++i) out[i] = 0;
  if (!pl.native || ldx < d || (mode != kStep && mode != kPredict)) return 0;
  const ClShape sh = make_shape(d, k, 0);
  out[0] = 1;
  out[1] = pl.slots;
  out[2] = float4_rows(X, d, ldx) ? 4 : 1;
  out[3] = pl.nblk;
  out[4] = pl.rows_per_block;
  out[5] = sh.Td * sh.Tk;
  out[6] = (int64_t)pl.lds;
  out[7] = (int64_t)up(d, 2) * sh.ldw;
  out[8] = sh.ldw;
  out[9] = kFoldTiles * kRows;
  out[10] = pl.bpc;
  out[11] = (int64_t)pl.nblk * block_doubles(sh.Td * sh.Tk, mode == kStep);
  return 0;
}

// tab: fp32 [d up to 2][out[8] of cdna_cluster_plan], entry (i, j) = Y_j[i], zeros elsewhere; gamma [128] f64 and
// shift [128] fp32, zeros from k and d on (shift all zeros for the cosine); w [n] f64 or null (every weight 1);
// assign [n] int32 or null; ws: out[11] of the plan doubles.
// STEP: out [k d + k + 2] f64: sum of w x~ per centre, sum of w per centre, sum of w D_min, count of bad rows.
// PREDICT: out [2] f64: the last two.
CDNA_API int cdna_cluster_step(const float* X, int64_t n, int64_t ldx, const double* w, const float* tab,
                               const double* gamma, const float* shift, int d, int k, int cosine, int mode,
                               int* assign, double* out, double* ws, hipStream_t st) {
  const ClPlan pl = cl_plan(n, d, k, mode, float4_rows(X, d, ldx));
  if (!pl.native || ldx < d || X == nullptr || tab == nullptr || gamma == nullptr || shift == nullptr ||
      out == nullptr || ws == nullptr)
    return (int)hipErrorInvalidValue;
  if (mode != kStep && mode != kPredict) return (int)hipErrorInvalidValue;
  const ClShape sh = make_shape(d, k, cosine != 0);
  const int slots = mode == kStep ? pl.slots : 0;
  const int rc = float4_rows(X, d, ldx)
                     ? step_launch_slots<4>(slots, pl, sh, X, n, ldx, w, tab, gamma, shift, assign, ws, st)
                     : step_launch_slots<1>(slots, pl, sh, X, n, ldx, w, tab, gamma, shift, assign, ws, st);
  if (rc != 0) return rc;
  const int64_t total = block_doubles(sh.Td * sh.Tk, mode == kStep);
  hipLaunchKernelGGL(cluster_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, ws, pl.nblk, sh,
                     mode == kStep ? 1 : 0, out);
  return (int)hipGetLastError();
}
