// K23 gmm_step — one EM pass of a full-covariance Gaussian mixture on the fp32 MFMA.
//
// Per row and component j (Spark's formulas, pyspark.ml.clustering.GaussianMixture):
//   t = x − c_j (fp32),  y = A_j t − A_j (mu_j − c_j),  q_j = |y|²  (fp64 from the fp32 products on),
//   p_j = ε + exp(logc_j − ½ q_j),  s = Σ_j p_j,  r_j = p_j / s.
// STEP returns S_j = Σ_rows w r_j [t | 1][t | 1]ᵀ and [Σ w log s, Σ w, rows with a non-finite q]; PREDICT the
// responsibilities and their argmax; EVAL the scalars only.  Both products are matmul-shaped and run on
// v_mfma_f32_32x32x2_f32 (exact fp32: responsibilities span hundreds of orders of magnitude and covariances are
// differences of moments, so no bf16 here).
//
// gmm_resp_kernel (E-step): 256 threads, 64-row tiles, row-major fp32 LDS tile with an odd row stride, the next
// tile prefetched in registers.  Per component, wave w forms the 32-row block (w & 1) of Y = T A_jᵀ for the column
// blocks (w >> 1) and (w >> 1) + 2: lane l's A operand at k-step m is tile[32 rb + (l & 31)][m + (l >> 5)] − c_j[..]
// (odd stride: 32 rows hit 32 banks), its B operand consecutive floats of the transposed, zero-padded fp32 copy of
// A_j the host prepares (L2-resident).  The correction constant is subtracted from the accumulators in fp64, the
// squares are summed over the 32 columns by a halving butterfly (16 values x 32 lanes -> one row sum per lane pair)
// and land in an fp64 q[column half][row][j] table in LDS: no block barrier between components.  After the last
// component 4 threads per row form p, s and r in fp64.
//
// gmm_moment_kernel (M-step sums): grid over (row chunk, component), the components of one chunk adjacent in the
// XCD-remapped launch order so their re-reads of the chunk's rows meet in one L2 (the plan keeps the number of
// chunks a multiple of 8 from 8 chunks on, so no chunk straddles two XCDs; below 8 chunks some do).  The tile is
// centred at c_j and scaled by fp32 √(w r_j) on its way into LDS (the tile's 64 scales are prefetched with its rows
// and staged in LDS), with the scale itself as column d; symtile.h's MFMA phase (K22's) over the upper triangular
// 32x32 tile pairs of the (d+1)x(d+1) moment matrix; two levels of accumulators held for the whole chunk (fp32 within
// a tile, fp64 across tiles), one fp64 slab per block.  N_j = S_j[d][d] is not taken from the slabs: the E-step sums
// w r_j in fp64.
//
// gmm_reduce_kernel: slabs and per-block scalars in a fixed order in fp64.  No float atomics on global memory: two
// calls on the same input return the same bits.
// Native range: d + 1 <= 128, 2 <= k <= 32.
#include "symtile.h"

namespace {

using namespace symtile;

// kRows, kMaxD: rowblock.h's 64-row tile and its 128 columns; d + 1 <= kMaxD
constexpr int kMaxK = 32;
constexpr double kGmmEps = 2.220446049250313e-16;  // 2^-52, Spark's EPSILON

enum { kStep = 0, kPredict = 1, kEval = 2 };

// VW = 4: float4 row loads (d % 4 == 0, ldx % 4 == 0, 16-byte aligned X); VW = 1: scalar loads, any layout.
// The kernel fills the register file: one block per CU.
template <int VW>
__global__ __launch_bounds__(256) void gmm_resp_kernel(
    const float* __restrict__ X, int64_t n, int d, int64_t ldx, const double* __restrict__ w,
    const float* __restrict__ cf, const float* __restrict__ AT, const double* __restrict__ corr,
    const double* __restrict__ logc, int k, int mode, int dk, int dc, int LD, float* __restrict__ sr,
    double* __restrict__ R, int* __restrict__ assign, double* __restrict__ spart, int64_t rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile = reinterpret_cast<float*>(smem);                            // [kRows][LD]
  double* qtab = reinterpret_cast<double*>(smem + (size_t)kRows * LD * 4);  // [2][kRows][k]
  double* red = qtab + 2 * kRows * k;                                       // [4][3 + kMaxK]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, half = lane >> 5, col = lane & 31;
  const int dv = d / VW;
  const int Tc = dc >> 5;
  const int rb = wid & 1, cb0 = wid >> 1, cb1 = cb0 + 2;
  const bool own0 = cb0 < Tc, own1 = cb1 < Tc;

  // zero the tile once: columns d .. LD - 1 are never written again (column d is read when d is odd)
  for (int i = tid; i < kRows * LD; i += 256) tile[i] = 0.f;

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  const int rr = tid >> 2, qq = tid & 3;  // row phase: 4 threads per row
  RowTile<VW> xt;
  double wv = 0.0;
  double s_ll = 0.0, s_w = 0.0, s_bad = 0.0;
  double nj[kMaxK / 4];  // STEP: this thread's share of N_j = sum w r_j, j = qq + 4 i
#pragma unroll
  for (int i = 0; i < kMaxK / 4; ++i) nj[i] = 0.0;

  if (rb0 < rb1) {
    xt.load(X, rb0, ldx, rb1 - rb0, tid, dv);
    wv = (rr < rb1 - rb0) ? (w != nullptr ? w[rb0 + rr] : 1.0) : 0.0;
  }
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    const bool more = t0 + kRows < rb1;
    const double rw = wv;
    const bool valid = t0 + rr < rb1;
    __syncthreads();  // every wave is past the MFMAs on the previous tile (and the zeroing, the first time)
    xt.store(tile, LD, tid, dv, [](int, int, float x) { return x; });  // odd LD: scalar stores
    if (more) {
      xt.load(X, t0 + kRows, ldx, rb1 - (t0 + kRows), tid, dv);
      wv = (rr < rb1 - (t0 + kRows)) ? (w != nullptr ? w[t0 + kRows + rr] : 1.0) : 0.0;
    }
    __syncthreads();  // tile complete

    const float* ap = tile + (32 * rb + col) * LD + half;
    for (int j = 0; j < k; ++j) {
      f32x16 acc0, acc1;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc0[e] = acc1[e] = 0.f;
      const float* cj = cf + (int64_t)j * dk + half;
      const float* bp = AT + ((int64_t)j * dk + half) * dc + col;
      // unrolled: 8 k-steps' operand loads (LDS, and A_jᵀ / c_j through L2) in flight, one wave per SIMD hides none
      if (own1) {
#pragma unroll 8
        for (int m = 0; m < dk; m += 2) {
          const float a = ap[m] - cj[m];
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[m * dc + 32 * cb0], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[m * dc + 32 * cb1], acc1, 0, 0, 0);
        }
      } else if (own0) {
#pragma unroll 8
        for (int m = 0; m < dk; m += 2)
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[m] - cj[m], bp[m * dc + 32 * cb0], acc0, 0, 0, 0);
      }
      // y² in fp64, this wave's two column blocks together
      double sq[16];
      const double k0 = own0 ? corr[(int64_t)j * dc + 32 * cb0 + col] : 0.0;
      const double k1 = own1 ? corr[(int64_t)j * dc + 32 * cb1 + col] : 0.0;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const double y0 = (double)acc0[e] - k0, y1 = (double)acc1[e] - k1;
        sq[e] = y0 * y0 + y1 * y1;
      }
      // halving butterfly over the 32 columns: lane bit 4 picks accumulator bit 3, .. lane bit 1 picks bit 0
#pragma unroll
      for (int h = 8; h >= 1; h >>= 1) {
        const bool up = (col & (2 * h)) != 0;
#pragma unroll
        for (int i = 0; i < h; ++i) {
          const double send = up ? sq[i] : sq[i + h];
          const double keep = up ? sq[i + h] : sq[i];
          sq[i] = keep + __shfl_xor(send, 2 * h);
        }
      }
      sq[0] += __shfl_xor(sq[0], 1);
      if ((col & 1) == 0) {
        const int row = 32 * rb + acc_row(col >> 1, half);  // col >> 1: the accumulator element this lane holds
        qtab[((int64_t)cb0 * kRows + row) * k + j] = sq[0];
      }
    }
    __syncthreads();  // q table complete

    double p[kMaxK / 4];
    double s = 0.0;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < kMaxK / 4; ++i) {
      const int j = qq + 4 * i;
      p[i] = 0.0;
      if (j < k) {
        const double qv = qtab[rr * k + j] + qtab[(kRows + rr) * k + j];
        if (!cdna::finite_d(qv)) bad = true;
        p[i] = kGmmEps + exp(logc[j] - 0.5 * qv);
        s += p[i];
      }
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    bad = __shfl_xor((int)bad, 1) != 0 || bad;
    bad = __shfl_xor((int)bad, 2) != 0 || bad;
    if (valid) {
      if (qq == 0) {
        if (bad) {
          s_bad += 1.0;
        } else {
          s_ll += rw * log(s);
          s_w += rw;
        }
      }
      const int64_t row = t0 + rr;
      if (mode == kStep) {
#pragma unroll
        for (int i = 0; i < kMaxK / 4; ++i) {
          const int j = qq + 4 * i;
          if (j < k) {
            const double wr = bad ? 0.0 : rw * (p[i] / s);
            sr[row * k + j] = (float)sqrt(wr);
            nj[i] += wr;
          }
        }
      } else if (mode == kPredict) {
        double best = -1.0;
        int bj = 0;
#pragma unroll
        for (int i = 0; i < kMaxK / 4; ++i) {
          const int j = qq + 4 * i;
          if (j < k) {
            const double r = p[i] / s;
            R[row * k + j] = bad ? __builtin_nan("") : r;
            if (r > best) {
              best = r;
              bj = j;
            }
          }
        }
#pragma unroll
        for (int o = 1; o <= 2; o <<= 1) {
          const double ob = __shfl_xor(best, o);
          const int oj = __shfl_xor(bj, o);
          if (ob > best || (ob == best && oj < bj)) {
            best = ob;
            bj = oj;
          }
        }
        if (qq == 0) assign[row] = bad ? 0 : bj;
      }
    }
  }

  s_ll = cdna::wave_sum(s_ll);
  s_w = cdna::wave_sum(s_w);
  s_bad = cdna::wave_sum(s_bad);
  // N_j: the 16 rows of a wave (lanes with the same qq), then the 4 waves in order
#pragma unroll
  for (int i = 0; i < kMaxK / 4; ++i)
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) nj[i] += __shfl_xor(nj[i], o);
  constexpr int kNS = 3 + kMaxK;
  __syncthreads();
  if (lane == 0) {
    red[wid * kNS + 0] = s_ll;
    red[wid * kNS + 1] = s_w;
    red[wid * kNS + 2] = s_bad;
  }
  if (lane < 4) {
#pragma unroll
    for (int i = 0; i < kMaxK / 4; ++i) red[wid * kNS + 3 + lane + 4 * i] = nj[i];
  }
  __syncthreads();
  if (tid < 3 + k)
    spart[(int64_t)blockIdx.x * (3 + k) + tid] =
        ((red[tid] + red[kNS + tid]) + red[2 * kNS + tid]) + red[3 * kNS + tid];
}

// PW: tile pairs per wave; VW as above.  One block per CU here too (PW = 1 with float4 loads fits two).  No
// instantiation uses scratch: the scalar-load variants' 32 loads in flight per thread and the two levels of
// accumulators go to 108-238 AGPRs instead (resource table: profiles/r11/symtile.md).
template <int PW, int VW>
__global__ __launch_bounds__(256) void gmm_moment_kernel(
    const float* __restrict__ X, int64_t n, int d, int64_t ldx, const float* __restrict__ sr, int k,
    const float* __restrict__ cf, int dk, int T, int npairs, int LD, double* __restrict__ partial,
    int64_t rows_per_chunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile = reinterpret_cast<float*>(smem);  // [kRows][LD]
  float* cs = tile + kRows * LD;                 // [kMaxD]
  float* ss = cs + kMaxD;                        // [kRows]: the tile rows' scales
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, half = lane >> 5, col = lane & 31;
  const int dv = d / VW;
  // an XCD's work items are consecutive: the k components of a chunk run on one XCD whenever that XCD's share of the
  // grid is a multiple of k (gmm_plan: always from 8 chunks on)
  const uint32_t work = cdna::xcd_remap(blockIdx.x, gridDim.x);
  const int64_t chunk = work / (uint32_t)k;
  const int j = (int)(work % (uint32_t)k);

  for (int i = tid; i < kRows * LD; i += 256) tile[i] = 0.f;
  for (int i = tid; i < kMaxD; i += 256) cs[i] = i < d ? cf[(int64_t)j * dk + i] : 0.f;
  const WavePairs<PW> wp(wid, T, npairs);
  // two levels of accumulators: the MFMAs add into the fp32 `acc` for kFoldRows rows, then `acc` is folded into the
  // fp64 `tot`.  A chunk-long fp32 chain carries about 3.5e-8 sqrt(roundings / 3) of a sum of positive terms, 1e-6
  // at 4096 rows, and EM's early iterations amplify a perturbation of the moments some 50 times: on the 20000 x 20
  // end-to-end fit the covariances moved by 1.9e-6 against the CPU fit with fp32 totals folded every 8 tiles, by
  // 3e-7 with fp64 totals folded every tile; folding every 16 rows changed nothing more (the E-step's product
  // rounding is what is left) and cost 8 % of the kernel.
  constexpr int kFoldRows = kRows;
  f32x16 acc[PW];
  double tot[PW][16];
#pragma unroll
  for (int q = 0; q < PW; ++q)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      acc[q][e] = 0.f;
      tot[q][e] = 0.0;
    }

  const int64_t rb0 = chunk * rows_per_chunk;
  int64_t rb1 = rb0 + rows_per_chunk;
  if (rb1 > n) rb1 = n;
  RowTile<VW> xt;
  float s1 = 0.f;  // threads 0 .. 63: the scale of tile row tid, prefetched with the rows
  auto load = [&](int64_t T0) __attribute__((always_inline)) {
    xt.load(X, T0, ldx, rb1 - T0, tid, dv);
    s1 = (tid < kRows && tid < rb1 - T0) ? sr[(T0 + tid) * k + j] : 0.f;
  };

  if (rb0 < rb1) load(rb0);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    const bool more = t0 + kRows < rb1;
    if (tid < kRows) ss[tid] = s1;  // its readers of the previous tile are past that tile's second barrier
    __syncthreads();  // every wave is past the MFMAs on the previous tile (and the zeroing, the first time)
    // a row with scale 0 (left out, zero weight, past the end) is zeroed, not scaled: NaN / inf stay out of S
    xt.store(tile, LD, tid, dv, [&](int r, int c, float x) {
      const float sc = ss[r];
      return sc != 0.f ? (x - cs[c]) * sc : 0.f;
    });
    if (tid < kRows) tile[tid * LD + d] = s1;
    if (more) load(t0 + kRows);
    __syncthreads();  // scaled tile complete
    for (int r0 = 0; r0 < kRows; r0 += kFoldRows) {
      mfma_rows<kFoldRows>(wp, tile + (r0 + half) * LD + col, LD, acc);
#pragma unroll
      for (int q = 0; q < PW; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          tot[q][e] += (double)acc[q][e];
          acc[q][e] = 0.f;
        }
    }
  }

#pragma unroll
  for (int q = 0; q < PW; ++q)
    if (wp.own[q]) store_slab(partial + ((chunk * k + j) * npairs + wid + 4 * q) * 1024, tot[q], half, col);
}

// blockIdx.y = component j < k: partial [nchunk][k][npairs][1024] -> S_j (symmetric fill), 16 threads per element
// each summing a fixed stride of chunks, then a fixed-order sum.  blockIdx.y == k (one block): the scalars,
// spart [nblk][3 + k] -> stats[3] and N_j -> S_j[d][d], the same way (4 strides of 64 values).  N_j is the E-step's
// fp64 sum of w r_j: the slabs' fp32 sum of the squared fp32 scales is not written.
__global__ __launch_bounds__(256) void gmm_reduce_kernel(const double* __restrict__ partial, int nchunk, int k,
                                                         int with_S, int npairs, int T, int D,
                                                         double* __restrict__ S,
                                                         const double* __restrict__ spart, int nblk,
                                                         double* __restrict__ stats) {
  __shared__ double red[16][16];
  if ((int)blockIdx.y == (with_S ? k : 0)) {  // without S (PREDICT / EVAL) the grid is this one block
    if (blockIdx.x != 0) return;
    double* red4 = &red[0][0];  // [4][64]
    const int v = threadIdx.x & 63, pt = threadIdx.x >> 6;
    double s = 0.0;
    if (v < 3 + k)
      for (int b = pt; b < nblk; b += 4) s += spart[(int64_t)b * (3 + k) + v];
    red4[pt * 64 + v] = s;
    __syncthreads();
    if (pt == 0 && v < 3 + k) {
      const double t = ((red4[v] + red4[64 + v]) + red4[128 + v]) + red4[192 + v];
      if (v < 3)
        stats[v] = t;
      else if (with_S)
        S[((int64_t)(v - 3) * D + (D - 1)) * D + (D - 1)] = t;
    }
    return;
  }
  const int64_t j = blockIdx.y;
  reduce_slabs(red, partial + j * npairs * 1024, (int64_t)k * npairs, nchunk, npairs,
               [T](int p, int& I, int& J) { pair_ij(p, T, I, J); }, D, S + j * D * D,
               [D](int a, int b) { return a == D - 1 && b == D - 1; });
}

struct GmmPlan {
  int dk, dc, LDr;       // E-step: k-steps (d rounded up to 2), padded columns of A_jᵀ, tile row stride
  int nblk;              // E-step blocks
  int64_t rows_per_block;
  size_t lds_r;
  int T, npairs, LDm;    // moment matrix: 32-wide tiles of d + 1, tile pairs, tile row stride
  int nchunk;
  int64_t rows_per_chunk;
  size_t lds_m;
};

GmmPlan gmm_plan(int64_t n, int d, int k) {
  GmmPlan pl{};
  pl.dk = (d + 1) / 2 * 2;
  pl.dc = (d + 31) / 32 * 32;
  pl.LDr = pl.dc + 1;  // odd: the A operand's 32 rows hit 32 banks
  int64_t nb = (n + 1023) / 1024;
  if (nb > 1024) nb = 1024;
  if (nb < 1) nb = 1;
  pl.nblk = (int)nb;
  const int64_t rpb = (n + nb - 1) / nb;
  pl.rows_per_block = (rpb + kRows - 1) / kRows * kRows;
  pl.lds_r = (size_t)kRows * pl.LDr * 4 + (size_t)2 * kRows * k * 8 + (size_t)4 * (3 + kMaxK) * 8;
  pl.T = (d + 1 + 31) / 32;
  pl.npairs = pl.T * (pl.T + 1) / 2;
  pl.LDm = pl.T * 32 + 1;
  int64_t nc = (n + 4095) / 4096, cap = 2048 / k;
  if (nc > cap) nc = cap;
  if (nc >= 8) nc = nc / 8 * 8;  // each of the 8 XCDs gets whole chunks: nchunk k / 8 work items, a multiple of k
  if (nc < 1) nc = 1;
  pl.nchunk = (int)nc;
  const int64_t rpc = (n + nc - 1) / nc;
  pl.rows_per_chunk = (rpc + kRows - 1) / kRows * kRows;
  pl.lds_m = (size_t)kRows * pl.LDm * 4 + (size_t)kMaxD * 4 + (size_t)kRows * 4;
  return pl;
}

// the E-step's dynamic LDS passes the 64 KB default at k = 32 and d > 96; the moment kernel's widest plan is 33 KB
template <int VW>
int resp_launch(const GmmPlan& pl, const float* X, int64_t n, int d, int64_t ldx, const double* w, const float* cf,
                const float* AT, const double* corr, const double* logc, int k, int mode, float* sr, double* R,
                int* assign, double* spart, hipStream_t st) {
  static bool raised[64] = {};
  const int rc = cdna::raise_lds(reinterpret_cast<const void*>(gmm_resp_kernel<VW>), raised,
                                 gmm_plan(1, kMaxD - 1, kMaxK).lds_r);
  if (rc != 0) return rc;
  hipLaunchKernelGGL((gmm_resp_kernel<VW>), dim3(pl.nblk), dim3(256), pl.lds_r, st, X, n, d, ldx, w, cf, AT, corr,
                     logc, k, mode, pl.dk, pl.dc, pl.LDr, sr, R, assign, spart, pl.rows_per_block);
  return (int)hipGetLastError();
}

template <int PW, int VW>
int moment_launch(const GmmPlan& pl, const float* X, int64_t n, int d, int64_t ldx, const float* sr, int k,
                  const float* cf, double* partial, hipStream_t st) {
  hipLaunchKernelGGL((gmm_moment_kernel<PW, VW>), dim3((unsigned)pl.nchunk * k), dim3(256), pl.lds_m, st, X, n, d,
                     ldx, sr, k, cf, pl.dk, pl.T, pl.npairs, pl.LDm, partial, pl.rows_per_chunk);
  return (int)hipGetLastError();
}

template <int VW>
int moment_launch_pw(const GmmPlan& pl, const float* X, int64_t n, int d, int64_t ldx, const float* sr, int k,
                     const float* cf, double* partial, hipStream_t st) {
  switch ((pl.npairs + 3) / 4) {
    case 1: return moment_launch<1, VW>(pl, X, n, d, ldx, sr, k, cf, partial, st);
    case 2: return moment_launch<2, VW>(pl, X, n, d, ldx, sr, k, cf, partial, st);
    default: return moment_launch<3, VW>(pl, X, n, d, ldx, sr, k, cf, partial, st);
  }
}

}  // namespace

// Padded sizes of the per-component tables the caller prepares: cf [k][dk] fp32 (centres), AT [k][dk][dc] fp32
// (AT[j][m][c] = A_j[c][m]), corr [k][dc] fp64 (A_j (mu_j − c_j)); all zero-padded.
CDNA_API int cdna_gmm_dk(int d) { return gmm_plan(1, d, 2).dk; }
CDNA_API int cdna_gmm_dc(int d) { return gmm_plan(1, d, 2).dc; }

// Blocks of the E-step launch: the scalar workspace holds 3 + k doubles per block.
CDNA_API int cdna_gmm_step_blocks(int64_t n) { return gmm_plan(n, 1, 2).nblk; }

// Workspace (in floats) of a STEP: the [n][k] fp32 scales (padded to 8 bytes), then the per-block fp64 moment slabs.
CDNA_API int64_t cdna_gmm_step_workspace(int64_t n, int d, int k) {
  const GmmPlan pl = gmm_plan(n, d, k);
  return (n * k + 1) / 2 * 2 + 2 * (int64_t)pl.nchunk * k * pl.npairs * 1024;
}

// S: [k][d+1][d+1] f64 (STEP only); R: [n][k] f64 and assign: [n] i32 (PREDICT only); stats: [Σ w log s, Σ w,
// rows with a non-finite q] f64.  w may be null (unit weights).  ws: cdna_gmm_step_workspace floats, 8-byte aligned
// (STEP only); sws: (3 + k) * cdna_gmm_step_blocks doubles.
CDNA_API int cdna_gmm_step(const float* X, int64_t n, int d, int64_t ldx, const double* w, const float* cf,
                           const float* AT, const double* corr, const double* logc, int k, int mode, double* S,
                           double* R, int* assign, double* stats, float* ws, double* sws, hipStream_t st) {
  if (n < 1 || d < 1 || d + 1 > kMaxD || k < 2 || k > kMaxK || ldx < d) return (int)hipErrorInvalidValue;
  if (mode < kStep || mode > kEval) return (int)hipErrorInvalidValue;
  if (mode == kStep && (S == nullptr || ws == nullptr)) return (int)hipErrorInvalidValue;
  if (mode == kPredict && (R == nullptr || assign == nullptr)) return (int)hipErrorInvalidValue;
  const GmmPlan pl = gmm_plan(n, d, k);
  const bool vec = float4_rows(X, d, ldx);
  float* sr = ws;
  double* partial = ws != nullptr ? reinterpret_cast<double*>(ws + (n * k + 1) / 2 * 2) : nullptr;
  int rc = vec ? resp_launch<4>(pl, X, n, d, ldx, w, cf, AT, corr, logc, k, mode, sr, R, assign, sws, st)
               : resp_launch<1>(pl, X, n, d, ldx, w, cf, AT, corr, logc, k, mode, sr, R, assign, sws, st);
  if (rc != 0) return rc;
  if (mode == kStep) {
    rc = vec ? moment_launch_pw<4>(pl, X, n, d, ldx, sr, k, cf, partial, st)
             : moment_launch_pw<1>(pl, X, n, d, ldx, sr, k, cf, partial, st);
    if (rc != 0) return rc;
  }
  const int64_t tot = mode == kStep ? (int64_t)pl.npairs * 1024 : 0;
  const unsigned gx = tot > 0 ? (unsigned)((tot + 15) / 16) : 1u;
  hipLaunchKernelGGL(gmm_reduce_kernel, dim3(gx, mode == kStep ? k + 1 : 1), dim3(256), 0, st, partial, pl.nchunk,
                     k, mode == kStep ? 1 : 0, pl.npairs, pl.T, d + 1, S, sws, pl.nblk, stats);
  return (int)hipGetLastError();
}
