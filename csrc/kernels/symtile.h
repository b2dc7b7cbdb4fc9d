// Shared machinery of the kernels that sum a symmetric D x D matrix over rows on the MFMA (K1 gram.hip, K22
// glm.hip, K23 gmm.hip): the matrix is tiled into upper-triangular 32x32 tile pairs, every block writes one
// [32][32] slab per pair, and a second kernel sums the slabs over blocks in a fixed order in fp64 and mirrors them.
#pragma once
#include "common.h"

namespace symtile {

// upper-triangular tile pair p of a T x T tile grid, row-major: (0,0), (0,1), ..
__device__ __host__ __forceinline__ void pair_ij(int p, int T, int& I, int& J) {
  int i = 0;
  while (p >= T - i) {
    p -= T - i;
    ++i;
  }
  I = i;
  J = i + p;
}

// v_mfma_f32_32x32x*: accumulator element e of the lanes' half `half` (lane >> 5) is tile row acc_row, column lane & 31
__device__ __forceinline__ int acc_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }

// a wave's accumulators (f32x16 or an array of 16) -> the [32][32] slab of its tile pair
template <typename S, typename A>
__device__ __forceinline__ void store_slab(S* __restrict__ dst, const A& acc, int half, int col) {
#pragma unroll
  for (int e = 0; e < 16; ++e) dst[acc_row(e, half) * 32 + col] = acc[e];
}

// Wave `wid` of 4 owns tile pairs wid, wid + 4, ..: at most PW of them.
template <int PW>
struct WavePairs {
  int TI[PW], TJ[PW];
  bool own[PW];
  __device__ __forceinline__ WavePairs(int wid, int T, int npairs) {
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      const int p = wid + 4 * j;
      own[j] = p < npairs;
      pair_ij(own[j] ? p : 0, T, TI[j], TJ[j]);
    }
  }
};

// The MFMA phase over ROWS rows of a row-major fp32 LDS tile with row stride LD.  tc = tile + (lane >> 5) * LD +
// (lane & 31): lane l's operand for tile column block I at k-step k is tile[k + (l >> 5)][32 I + (l & 31)] --
// consecutive floats of one row, no transposition.  For each pair of rows the owned pairs go in j order.
template <int ROWS, int PW>
__device__ __forceinline__ void mfma_rows(const WavePairs<PW>& wp, const float* tc, int LD, f32x16 (&acc)[PW]) {
#pragma unroll 4
  for (int k = 0; k < ROWS; k += 2) {
    const float* rp = tc + k * LD;
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      if (!wp.own[j]) continue;
      const float a = rp[32 * wp.TI[j]], b = rp[32 * wp.TJ[j]];
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[j], 0, 0, 0);
    }
  }
}

// A thread's share of a 64-row tile of X, held in registers while the previous tile is worked on: 64 rows x dv =
// d / VW load items over 256 threads, item e = (row e / dv, load item e % dv).  VW = 4: float4 row loads (rows
// float4-addressable, see float4_rows); VW = 1: scalar loads, any layout.  K23's two kernels use it; K22 keeps
// the same loops as macros (this form costs it registers, see glm.hip).
template <int VW>
struct RowTile {
  typedef float vec_t __attribute__((ext_vector_type(VW)));
  static constexpr int kNI = 32 / VW;  // 64 * 128 / VW items over 256 threads
  vec_t v[kNI];

  // rows t0 .. of X -> registers; rows from `lim` (= end of the block's rows - t0) on become zeros
  __device__ __forceinline__ void load(const float* __restrict__ X, int64_t t0, int64_t ldx, int64_t lim, int tid,
                                       int dv) {
#pragma unroll
    for (int i = 0; i < kNI; ++i) {
      const int e = tid + 256 * i;
      const int r = e / dv, c = e - r * dv;
      vec_t t = {};
      if (e < 64 * dv && r < lim) t = *reinterpret_cast<const vec_t*>(X + (t0 + r) * ldx + (int64_t)c * VW);
      v[i] = t;
    }
  }

  // registers -> tile[r][c] = f(r, c, x), columns c < d only (the tile's zeroed padding columns stay zero); scalar
  // stores, so any row stride LD
  template <class F>
  __device__ __forceinline__ void store(float* tile, int LD, int tid, int dv, F f) const {
#pragma unroll
    for (int i = 0; i < kNI; ++i) {
      const int e = tid + 256 * i;
      const int r = e / dv, c = e - r * dv;
      if (e < 64 * dv) {
        vec_t t;
#pragma unroll
        for (int u = 0; u < VW; ++u) t[u] = f(r, c * VW + u, v[i][u]);
#pragma unroll
        for (int u = 0; u < VW; ++u) tile[r * LD + c * VW + u] = t[u];
      }
    }
  }
};

// Slab reduction, one block of 256 threads per 16 slab elements: slabs [nblk][bstride >= npairs][1024] of S, this
// matrix's at `partial` -> out [D][D] (symmetric fill).  16 threads per element each sum a fixed stride of blocks,
// then a fixed-order sum of the 16: deterministic, and 16x the parallelism of one thread per element (the serial
// 1024-block loop took 0.35 ms of a 3.6 ms fit).  pij(pair, I, J) resolves a pair; skip(i, j): an entry not written.
template <typename S, class PairFn, class SkipFn>
__device__ __forceinline__ void reduce_slabs(double (&red)[16][16], const S* __restrict__ partial, int64_t bstride,
                                             int nblk, int npairs, PairFn pij, int D, double* __restrict__ out,
                                             SkipFn skip) {
  const int el = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int64_t idx = (int64_t)blockIdx.x * 16 + el;
  const bool ok = idx < (int64_t)npairs * 1024;
  const int gp = ok ? (int)(idx >> 10) : 0, e = ok ? (int)(idx & 1023) : 0;
  double s = 0.0;
  if (ok)
    for (int b = part; b < nblk; b += 16) s += (double)partial[((int64_t)b * bstride + gp) * 1024 + e];
  red[part][el] = s;
  __syncthreads();
  if (part == 0 && ok) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += red[q][el];
    int I, J;
    pij(gp, I, J);
    const int i = I * 32 + (e >> 5), j = J * 32 + (e & 31);
    if (i < D && j < D && !skip(i, j)) {
      out[(int64_t)i * D + j] = t;
      out[(int64_t)j * D + i] = t;
    }
  }
}

// rows of X addressable as float4: what the VW = 4 kernels need
inline bool float4_rows(const float* X, int d, int64_t ldx) {
  return d % 4 == 0 && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
}

}  // namespace symtile
