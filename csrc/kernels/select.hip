// K27 label_stats — the per-feature statistics of a feature matrix against a label that the univariate tests of
// pyspark.ml.stat need (ChiSquareTest, ANOVATest, FValueTest and the selectors on top), in one pass over the rows.
//
//   COUNT   (chi-square): the exact contingency table [d][K][C] of cells (feature, int(x), label code), 64-bit.
//           A cell is bad when x is non-finite, not integer-valued, < 0 or >= K.
//   CLASS   (ANOVA): per (class, feature) sum (x - s), per feature sum (x - s)^2, per class n_c; fp64 from
//           (double)x - shift[c].  A cell is bad when x is non-finite.
//   REGRESS (F-value): per feature sum (x - s), sum (x - s)^2, sum (x - s)(y - ys); sum (y - ys), sum (y - ys)^2 and the
//           row count; fp64.  A cell is bad when x is non-finite.
// Every mode also counts bad[d], the bad cells per feature: a bad cell adds nothing to its feature's statistics.  A row
// whose label is bad (a code outside 0 .. C-1, a non-finite y) is never accumulated and is counted in bad_label.
//
// label_stats_kernel<MODE, VW>: rowblock.h's scaffolding -- 256 threads, 64-row tiles, the next tile of X prefetched
// in registers, a row-major fp32 LDS tile with the odd row stride kLD whose columns d .. are zeroed once; rows past
// the end of the block's range are never read from memory (they are zeros in the tile and their label slot says
// "skip").  Thread (column tid & 127, row half tid >> 7) owns that column's statistics: a wave reads 64 consecutive
// floats of one tile row, and all its lanes share the row's label.
//   COUNT: a per-block LDS table of u32 cells cell[(k * C + y) * pitch + c] with the column innermost and an odd
//     pitch (d | 1): the lanes of a wave share y and differ in c and k, so they spread over the banks (a [c][k][y]
//     layout puts every lane in one bank whenever K C is a multiple of 64).  LDS integer atomics (two threads own a
//     column), flushed once per block to the 64-bit totals with global integer atomics: deterministic.  The plan keeps a
//     block's row range below 2^32, so a cell cannot wrap.  The table has a fixed budget of kCountBudget bytes; a
//     wider one is outside the native range.
//   CLASS: an LDS fp64 table [row half][class][column] whose cells are private to the owning thread: no atomics, lanes
//     are consecutive columns (conflict-free), and the row order is fixed.  sum (x - s)^2 and bad stay in registers.
//   REGRESS: everything in registers; the tile rows' y - ys go through LDS.
//   The label statistics (n_c; sum (y - ys), its square and the count; bad_label) belong to the 64 threads that load the
//   tile's labels.
// CLASS and REGRESS write one workspace slot per block (all 128 columns: the ones past d hold zeros) and
// label_reduce_kernel sums the slots in a fixed order in fp64 (rowblock.h's sum_blocks).  No float atomics on global
// memory: reruns are bit-identical.
// Native range: fp32 rows, 1 <= d <= 128, any n >= 1, row stride and alignment; CLASS: 2 <= C <= 32; COUNT: K, C >= 1
// with K C (d | 1) 4 <= kCountBudget.
#include <cmath>

#include "rowblock.h"

namespace {

using namespace rowblock;

constexpr int kMaxC = 32;  // CLASS
// the COUNT table's LDS budget: with the 33 KB tile a block stays under the 160 KB of a CU (one block per CU at the
// budget; smaller tables let up to four in)
constexpr size_t kCountBudget = 96 * 1024;
constexpr size_t kCuLds = 160 * 1024;

enum { kCount = 0, kClass = 1, kRegress = 2 };

struct SelParams {
  double yshift;
  int d, C, K, pitch;
};

// workspace doubles per block.  CLASS: [C][128] class sums | sq [128] | bad [128] | n_c [C] | bad_label.
// REGRESS: sx | sxx | sxy | bad, [128] each | sum y | sum y^2 | rows | bad_label.
__host__ __device__ constexpr int slot_doubles(int mode, int C) {
  return mode == kClass ? C * kMaxD + 2 * kMaxD + C + 1 : mode == kRegress ? 4 * kMaxD + 4 : 0;
}

// static LDS of an instantiation: the tile and the rows' label codes; REGRESS: the rows' y; CLASS: the rows per class
constexpr size_t static_lds(int mode) {
  return (size_t)kXF * 4 + kRows * 4 + (mode == kRegress ? kRows * 8 : 0) + (mode == kClass ? kMaxC * 4 : 0);
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }

// VW = 4: float4 row loads, VW = 1: scalar loads, any layout.
template <int MODE, int VW>
__global__ __launch_bounds__(256) void label_stats_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const int* __restrict__ codes,
    const double* __restrict__ yin, const double* __restrict__ shift, const SelParams pr, double* __restrict__ ws,
    unsigned long long* __restrict__ cnt, int64_t rows_per_block) {
  __shared__ __attribute__((aligned(16))) float xb[kXF];
  __shared__ double yv[kRows];         // REGRESS: the tile rows' y - ys
  __shared__ int lab[kRows];           // the tile rows' label code; -1: skip the row
  __shared__ unsigned int ncls[kMaxC];  // CLASS: rows per class
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  unsigned int* cell = reinterpret_cast<unsigned int*>(dyn);  // COUNT [K C][pitch]
  double* tab = reinterpret_cast<double*>(dyn);               // CLASS [2][C][kMaxD]
  const int tid = threadIdx.x;
  const int d = pr.d, dv = d / VW, C = pr.C;

  if (tid < kMaxC) ncls[tid] = 0u;
  if (MODE == kCount)
    for (int i = tid; i < pr.K * C * pr.pitch; i += 256) cell[i] = 0u;
  if (MODE == kClass)
    for (int i = tid; i < 2 * C * kMaxD; i += 256) tab[i] = 0.0;

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  const int bc = tid & (kMaxD - 1), bh = tid >> 7;
  const double sh = MODE != kCount && bc < d ? shift[bc] : 0.0;
  int labn = -1;
  double yn = 0.0;
  // the column's statistics over the row half, summed over the block's tiles
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;  // CLASS: a1 = sq; REGRESS: sx, sxx, sxy
  unsigned int bad = 0u;
  // the label statistics of tile row tid (tid < 64)
  double sy = 0.0, syy = 0.0;
  unsigned int rows_ok = 0u, badl = 0u;

  // the tile rows' labels travel with the tile, in its first 64 threads
  const auto side = [&](int64_t t, int i) {
    if (i < kRows && t + i < rb1) {
      if (MODE == kRegress) yn = yin[t + i];
      else labn = codes[t + i];
    }
  };
  TileStream<VW> ts;
  ts.begin(xb, kXF, X, ldx, rb0, rb1, dv, tid, side);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    ts.put(xb, tid);
    if (tid < kRows) {
      const bool valid = t0 + tid < rb1;
      bool ok;
      if (MODE == kRegress) {
        ok = valid && cdna::finite_d(yn);
        const double yy = ok ? yn - pr.yshift : 0.0;
        yv[tid] = yy;
        lab[tid] = ok ? 0 : -1;
        sy += yy;
        syy = fma(yy, yy, syy);
      } else {
        ok = valid && (unsigned)labn < (unsigned)C;
        lab[tid] = ok ? labn : -1;
        if (MODE == kClass && ok) atomicAdd(&ncls[labn], 1u);
      }
      rows_ok += ok ? 1u : 0u;
      badl += valid && !ok ? 1u : 0u;
    }
    ts.fetch(t0, tid, side);  // tile and labels complete

    if (bc < d) {
      const float* xc = xb + (32 * bh) * kLD + bc;
      const int* lr = lab + 32 * bh;
      if (MODE == kCount) {
        const float fk = (float)pr.K;
        unsigned int* cc = cell + bc;
#pragma unroll 8
        for (int r = 0; r < 32; ++r) {
          const int yl = lr[r];
          const float x = xc[r * kLD];
          if (yl < 0) continue;
          if (x >= 0.f && x < fk && x == truncf(x))  // NaN fails x >= 0, inf fails x < K
            atomicAdd(cc + ((int)x * C + yl) * pr.pitch, 1u);
          else
            ++bad;
        }
      } else if (MODE == kClass) {
        double* tc = tab + bh * C * kMaxD + bc;
#pragma unroll 8
        for (int r = 0; r < 32; ++r) {
          const int yl = lr[r];
          const float x = xc[r * kLD];
          if (yl < 0) continue;
          if (finite_f(x)) {
            const double v = (double)x - sh;
            tc[yl * kMaxD] += v;
            a1 = fma(v, v, a1);
          } else {
            ++bad;
          }
        }
      } else {
        const double* yr = yv + 32 * bh;
#pragma unroll 8
        for (int r = 0; r < 32; ++r) {
          const int yl = lr[r];
          const float x = xc[r * kLD];
          if (yl < 0) continue;
          if (finite_f(x)) {
            const double v = (double)x - sh;
            a0 += v;
            a1 = fma(v, v, a1);
            a2 = fma(v, yr[r], a2);
          } else {
            ++bad;
          }
        }
      }
    }
  }

  __syncthreads();  // the last tile's reads are done: the tile's memory folds the two row halves
  if (MODE == kCount) {
    const int kc = pr.K * C;
    for (int i = tid; i < kc * pr.pitch; i += 256) {
      const unsigned int v = cell[i];
      const int q = i / pr.pitch, c = i - q * pr.pitch;
      if (v != 0u && c < d) atomicAdd(cnt + (int64_t)c * kc + q, (unsigned long long)v);
    }
    if (bc < d && bad != 0u) atomicAdd(cnt + (int64_t)d * kc + bc, (unsigned long long)bad);
    if (tid < kRows) {
      const double b = cdna::wave_sum((double)badl);
      if (tid == 0 && b != 0.0) atomicAdd(cnt + (int64_t)d * kc + d, (unsigned long long)b);
    }
    return;
  }
  double* fold = reinterpret_cast<double*>(xb);  // [4][kMaxD]
  if (bh == 1) {
    fold[bc] = a0;
    fold[kMaxD + bc] = a1;
    fold[2 * kMaxD + bc] = a2;
    fold[3 * kMaxD + bc] = (double)bad;
  }
  double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0;
  if (tid < kRows) {  // wave 0: the 64 tile rows' label sums in a fixed order
    l0 = cdna::wave_sum(sy);
    l1 = cdna::wave_sum(syy);
    l2 = cdna::wave_sum((double)rows_ok);
    l3 = cdna::wave_sum((double)badl);
  }
  __syncthreads();
  double* slot = ws + (int64_t)blockIdx.x * slot_doubles(MODE, C);
  if (MODE == kClass) {
    const int cd = C * kMaxD;
    for (int i = tid; i < cd; i += 256) slot[i] = tab[i] + tab[cd + i];
    if (bh == 0) {
      slot[cd + bc] = a1 + fold[kMaxD + bc];
      slot[cd + kMaxD + bc] = (double)bad + fold[3 * kMaxD + bc];
    }
    if (tid < C) slot[cd + 2 * kMaxD + tid] = (double)ncls[tid];
    if (tid == 0) slot[cd + 2 * kMaxD + C] = l3;
  } else {
    if (bh == 0) {
      slot[bc] = a0 + fold[bc];
      slot[kMaxD + bc] = a1 + fold[kMaxD + bc];
      slot[2 * kMaxD + bc] = a2 + fold[2 * kMaxD + bc];
      slot[3 * kMaxD + bc] = (double)bad + fold[3 * kMaxD + bc];
    }
    if (tid == 0) {
      slot[4 * kMaxD] = l0;
      slot[4 * kMaxD + 1] = l1;
      slot[4 * kMaxD + 2] = l2;
      slot[4 * kMaxD + 3] = l3;
    }
  }
}

// One block of 256 threads per 16 output values: out [slot] = the sum of the blocks' slots.
__global__ __launch_bounds__(256) void label_reduce_kernel(const double* __restrict__ ws, int nblk, int slot,
                                                           double* __restrict__ out) {
  __shared__ double red[16][16];
  const int idx = blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = idx < slot;
  const double t = sum_blocks(red, nblk, ok, [&](int b) { return ws[(int64_t)b * slot + idx]; });
  if (threadIdx.x < 16 && ok) out[idx] = t;
}

struct SelPlan : RowSplit {
  bool native;
  int per_cu, pitch, slot;
  size_t dyn;  // dynamic LDS bytes
};

// One round of resident blocks on the 256 CUs, as many per CU as the LDS lets in (at most four); at least 1024 rows
// per block, and fewer than 2^31 (a u32 cell of the COUNT table cannot wrap).
SelPlan sel_plan(int64_t n, int d, int mode, int C, int K) {
  SelPlan pl{};
  if (n < 1 || d < 1 || d > kMaxD) return pl;
  if (mode == kCount) {
    if (C < 1 || K < 1 || C > (1 << 20) || K > (1 << 20)) return pl;
    pl.pitch = d | 1;
    const int64_t bytes = (int64_t)K * C * pl.pitch * 4;
    if (bytes > (int64_t)kCountBudget) return pl;
    pl.dyn = (size_t)bytes;
  } else if (mode == kClass) {
    if (C < 2 || C > kMaxC) return pl;
    pl.dyn = (size_t)2 * C * kMaxD * 8;
  } else if (mode != kRegress) {
    return pl;
  }
  pl.native = true;
  pl.slot = slot_doubles(mode, C);
  pl.per_cu = (int)(kCuLds / (static_lds(mode) + pl.dyn));
  if (pl.per_cu > 4) pl.per_cu = 4;
  static_cast<RowSplit&>(pl) = split_rows(n, (int64_t)pl.per_cu * 256, (n + (((int64_t)1 << 31) - 1)) >> 31);
  return pl;
}

template <int MODE, int VW>
int stats_launch(const SelPlan& pl, const float* X, int64_t n, int64_t ldx, const int* codes, const double* y,
                 const double* shift, const SelParams& pr, double* ws, unsigned long long* cnt, hipStream_t st) {
  if (pl.dyn > 0) {
    static bool raised[64] = {};
    const size_t widest = MODE == kCount ? kCountBudget : (size_t)2 * kMaxC * kMaxD * 8;
    const int rc = cdna::raise_lds(reinterpret_cast<const void*>(label_stats_kernel<MODE, VW>), raised, widest);
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL((label_stats_kernel<MODE, VW>), dim3(pl.nblk), dim3(256), pl.dyn, st, X, n, ldx, codes, y, shift,
                     pr, ws, cnt, pl.rows_per_block);
  return (int)hipGetLastError();
}

}  // namespace

static_assert((size_t)kXF * 4 % 16 == 0, "the fp64 words of LDS start aligned");
static_assert(static_lds(kCount) + kCountBudget <= kCuLds, "a block at the COUNT budget fits a CU");
static_assert(static_lds(kClass) + (size_t)2 * kMaxC * kMaxD * 8 <= kCuLds, "a block at the widest CLASS table fits a CU");
static_assert(4 * kMaxD * 8 <= kXF * 4, "the fold of the row halves fits the tile");

// What cdna_label_stats runs for these operands (nothing is launched): out = [native, load width (4: float4 rows, 1:
// scalar), blocks, rows per block, LDS bytes per block, workspace doubles per block, the COUNT table's LDS budget in
// bytes, blocks per CU by LDS].
CDNA_API int cdna_label_stats_plan(const float* X, int64_t n, int64_t ldx, int d, int mode, int C, int K,
                                   int64_t* out) {
  const SelPlan pl = sel_plan(n, d, mode, C, K);
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[6] = (int64_t)kCountBudget;
  if (!pl.native || ldx < d) return 0;
  out[0] = 1;
  out[1] = float4_rows(X, d, ldx) ? 4 : 1;
  out[2] = pl.nblk;
  out[3] = pl.rows_per_block;
  out[4] = (int64_t)(static_lds(mode) + pl.dyn);
  out[5] = pl.slot;
  out[7] = pl.per_cu;
  return 0;
}

// Workspace in doubles: one slot per block (COUNT needs none).
CDNA_API int64_t cdna_label_stats_workspace(int64_t n, int d, int mode, int C, int K) {
  const SelPlan pl = sel_plan(n, d, mode, C, K);
  return pl.native ? (int64_t)pl.nblk * pl.slot : 0;
}

// codes [n] int32 (COUNT, CLASS) or y [n] f64 (REGRESS); shift [d] f64 (CLASS, REGRESS).
// COUNT: out = u64 [d K C + d + 1] = [table [d][K][C] | bad [d] | bad_label] (cleared here).
// CLASS / REGRESS: out = f64 [slot] in the layout of slot_doubles, ws: cdna_label_stats_workspace doubles.
CDNA_API int cdna_label_stats(const float* X, int64_t n, int64_t ldx, const int* codes, const double* y,
                              const double* shift, double yshift, int d, int mode, int C, int K, void* out, double* ws,
                              hipStream_t st) {
  const SelPlan pl = sel_plan(n, d, mode, C, K);
  if (!pl.native || ldx < d || X == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
  if (mode == kRegress ? y == nullptr : codes == nullptr) return (int)hipErrorInvalidValue;
  if (mode != kCount && (shift == nullptr || ws == nullptr)) return (int)hipErrorInvalidValue;
  const SelParams pr{yshift, d, mode == kRegress ? 1 : C, mode == kCount ? K : 0, pl.pitch};
  const bool vec = float4_rows(X, d, ldx);
  unsigned long long* cnt = static_cast<unsigned long long*>(out);
  int rc;
  if (mode == kCount) {
    const hipError_t e = hipMemsetAsync(out, 0, ((size_t)d * K * C + d + 1) * 8, st);
    if (e != hipSuccess) return (int)e;
    return vec ? stats_launch<kCount, 4>(pl, X, n, ldx, codes, y, shift, pr, ws, cnt, st)
               : stats_launch<kCount, 1>(pl, X, n, ldx, codes, y, shift, pr, ws, cnt, st);
  }
  if (mode == kClass)
    rc = vec ? stats_launch<kClass, 4>(pl, X, n, ldx, codes, y, shift, pr, ws, cnt, st)
             : stats_launch<kClass, 1>(pl, X, n, ldx, codes, y, shift, pr, ws, cnt, st);
  else
    rc = vec ? stats_launch<kRegress, 4>(pl, X, n, ldx, codes, y, shift, pr, ws, cnt, st)
             : stats_launch<kRegress, 1>(pl, X, n, ldx, codes, y, shift, pr, ws, cnt, st);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(label_reduce_kernel, dim3((unsigned)((pl.slot + 15) / 16)), dim3(256), 0, st, ws, pl.nblk,
                     pl.slot, static_cast<double*>(out));
  return (int)hipGetLastError();
}
