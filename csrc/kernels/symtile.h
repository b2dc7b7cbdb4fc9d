// Shared machinery of the kernels that sum a symmetric D x D matrix over rows on the MFMA (K1 gram.hip, K22
// glm.hip, K23 gmm.hip): the matrix is tiled into upper-triangular 32x32 tile pairs, every block writes one
// [32][32] slab per pair, and a second kernel sums the slabs over blocks in a fixed order in fp64 and mirrors them.
#pragma once
#include "rowblock.h"

namespace symtile {

using namespace rowblock;

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

// Slab reduction, one block of 256 threads per 16 slab elements: slabs [nblk][bstride >= npairs][1024] of S, this
// matrix's at `partial` -> out [D][D] (symmetric fill), summed over the blocks by rowblock.h's sum_blocks.
// pij(pair, I, J) resolves a pair; skip(i, j): an entry not written.
template <typename S, class PairFn, class SkipFn>
__device__ __forceinline__ void reduce_slabs(double (&red)[16][16], const S* __restrict__ partial, int64_t bstride,
                                             int nblk, int npairs, PairFn pij, int D, double* __restrict__ out,
                                             SkipFn skip) {
  const int64_t idx = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = idx < (int64_t)npairs * 1024;
  const int gp = ok ? (int)(idx >> 10) : 0, e = ok ? (int)(idx & 1023) : 0;
  const double t =
      sum_blocks(red, nblk, ok, [&](int b) { return (double)partial[((int64_t)b * bstride + gp) * 1024 + e]; });
  if (threadIdx.x < 16 && ok) {
    int I, J;
    pij(gp, I, J);
    const int i = I * 32 + (e >> 5), j = J * 32 + (e & 31);
    if (i < D && j < D && !skip(i, j)) {
      out[(int64_t)i * D + j] = t;
      out[(int64_t)j * D + i] = t;
    }
  }
}

}  // namespace symtile
