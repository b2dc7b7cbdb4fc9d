// K35 als_topk — for every source row s_i of S [ns, r] the k destination rows d_j of D [nd, r] with the largest
// s_i . d_j, in the order (score descending, position ascending), without ever forming the ns x nd score matrix.
//
// topk_kernel: grid (source blocks, destination slabs), 256 threads.  A block owns 128 source rows, 32 per wave, and
// walks one contiguous slab of destination rows in 32-row tiles through LDS; the next tile is on its way in registers
// while the current one is multiplied (the pipeline of rowblock.h, with a tile of this kernel's own: DstTile).
//   scores: v_mfma_f32_32x32x2_f32 with the destinations as the A operand and the sources as the B operand, so that
//           accumulator element e of lane l is the score of source row l & 31 against destination row acc_row(e,
//           l >> 5) of the tile: a source row lives in lanes l and l + 32, 16 scores each.  The order of the
//           inner dimension is free as long as both operands agree, so half h of the lanes takes columns 4 q + 2 h and
//           4 q + 2 h + 1 for the k-steps 2 q and 2 q + 1: one 8-byte LDS read feeds two MFMAs.  The wave's source
//           operand is loaded once into registers in that order (NQ pairs: r rounded up to 4, zero padded; the
//           instantiations hold 8, 16, 32, 64 or 128 columns and skip the k-steps from r on).  The LDS tile's row
//           stride is 4 NQ + 2 floats: 2 (mod 4), so the 32 rows of a half wave's 8-byte reads fall on distinct bank
//           pairs.
//   select: every source row has a sorted list of k (value, position) pairs in LDS (entry j belongs to lane j of the
//           row's wave), empty entries (-inf, INT_MAX), and its k-th value as a threshold in the registers of its two
//           lanes.  After a tile a lane compares its 16 scores with the threshold the row had when the tile
//           began; the steady state is that compare.  A passer is inserted by the whole wave: every lane compares its
//           entry with the candidate under the full (value, position) rule, the ballot's population count is the
//           place, the entries behind it move up one lane.  Because the candidates of a tile all passed the same
//           threshold and the insert applies the full rule, their order of insertion does not matter; candidates of
//           later tiles have higher positions, so "strictly greater than the threshold" is the tie rule.  While a row
//           of the wave has fewer than k entries (threshold -inf) the compare is >=, so that scores of -inf are kept
//           and NaN scores (which fail every compare) never are.
// topk_merge_kernel (slabs > 1 only): one wave per source row holds the final list in registers, entry j in lane j,
// and inserts the slabs' partial lists in slab order under the same rule; a partial list is left at its first
// rejected entry.  With one slab the first kernel writes the final result.
// No atomics and a fixed order everywhere: the result is a function of the operands alone.
// Native range: fp32 rows, 1 <= r <= 128, 1 <= k <= 64, ns >= 1, 1 <= nd < 2^31.
#include <climits>

#include "symtile.h"

namespace {

using rowblock::float4_rows;
using symtile::acc_row;

constexpr int kMaxR = 128;
constexpr int kMaxTopK = 64;
constexpr int kSrcRows = 128;     // source rows of a block, 32 per wave
constexpr int kTile = 32;         // destination rows of a tile: one MFMA's
constexpr int kMinSlab = 512;     // destination rows a slab has at least
constexpr int kCUs = 256;
constexpr int kEmpty = INT_MAX;   // position of an empty list entry: behind every real one

__host__ __device__ __forceinline__ int tile_ld(int NQ) { return 4 * NQ + 2; }
__host__ __device__ __forceinline__ size_t lds_bytes(int NQ, int k) {
  return (size_t)kTile * tile_ld(NQ) * 4 + (size_t)kSrcRows * k * 8;
}

// A thread's share of a 32-row tile of D, held in registers while the previous tile is multiplied.  The instantiation's
// 4 NQ columns make W = 4 NQ / VW load items a row (a power of two: no division), thread tid takes item tid % W of the
// rows tid / W, tid / W + 256 / W, ..: at most 16 floats a thread.  Rows from `lim` on and columns from r on are zeros.
template <int NQ, int VW>
struct DstTile {
  typedef float vec_t __attribute__((ext_vector_type(VW)));
  static constexpr int W = 4 * NQ / VW;
  static constexpr int RP = 256 / W;                     // rows per pass of the block
  static constexpr int NI = (kTile + RP - 1) / RP;
  static constexpr int LD = 4 * NQ + 2;
  vec_t v[NI];

  __device__ __forceinline__ void load(const float* __restrict__ D, int64_t p0, int64_t ldd, int64_t lim, int tid,
                                       int r) {
    const int c = (tid % W) * VW, r0 = tid / W;
    const float* src = D + (p0 + r0) * ldd + c;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = r0 + i * RP;
      vec_t t = {};
      if (row < kTile && row < lim && c < r) t = *reinterpret_cast<const vec_t*>(src + (int64_t)(i * RP) * ldd);
      v[i] = t;
    }
  }

  // registers -> tile[row][c ..]; scalar stores (the row stride is no multiple of 4)
  __device__ __forceinline__ void store(float* tile, int tid, int r) const {
    const int c = (tid % W) * VW, r0 = tid / W;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = r0 + i * RP;
      if (row < kTile && c < r) {
#pragma unroll
        for (int u = 0; u < VW; ++u) tile[row * LD + c + u] = v[i][u];
      }
    }
  }
};

// The wave inserts the candidate (v, i) into a sorted list whose entry j is (a, b) in lane j < k.  Returns whether it
// went in; kth is then the list's new k-th value.
__device__ __forceinline__ bool list_insert(float& a, int& b, int lane, int k, float v, int i, float& kth) {
  const bool in = lane < k;
  const bool before = in && (a > v || (a == v && b < i));
  const int pos = __popcll(__ballot(before));
  if (pos >= k) return false;
  const float pa = __shfl_up(a, 1);
  const int pb = __shfl_up(b, 1);
  kth = pos == k - 1 ? v : __shfl(a, k >= 2 ? k - 2 : 0);
  if (lane == pos) {
    a = v;
    b = i;
  } else if (lane > pos) {
    a = pa;
    b = pb;
  }
  return true;
}

// NQ: column pairs per half of the lanes the instantiation holds (r <= 4 NQ); VW = 4: float4 row loads of D, VW = 1:
// scalar loads, any layout.  oval / oidx: [gridDim.y][ns][k], a slab's lists (the result itself for one slab).
template <int NQ, int VW>
__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ S, int64_t ns, int64_t lds,
                                                   const float* __restrict__ D, int64_t nd, int64_t ldd, int r, int k,
                                                   int64_t rows_per_slab, float* __restrict__ oval,
                                                   int* __restrict__ oidx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LD = 4 * NQ + 2;
  float* tile = reinterpret_cast<float*>(smem);  // [kTile][LD]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, half = lane >> 5;
  float* lv = tile + kTile * LD + wid * 32 * k;  // [32][k] the wave's lists
  int* li = reinterpret_cast<int*>(tile + kTile * LD + 4 * 32 * k) + wid * 32 * k;
  const int nq = (r + 3) >> 2;

  // the wave's source rows: the B operand of every MFMA of the block
  const int64_t srow0 = (int64_t)blockIdx.x * kSrcRows + wid * 32;
  const bool live = srow0 + col < ns;
  float sreg[NQ][2];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = 4 * q + 2 * half + u;
      sreg[q][u] = live && c < r ? S[(srow0 + col) * lds + c] : 0.f;
    }
  for (int i = lane; i < 32 * k; i += 64) {
    lv[i] = -INFINITY;
    li[i] = kEmpty;
  }
  for (int i = tid; i < kTile * LD; i += 256) tile[i] = 0.f;  // the columns from r on stay zero
  // the row's k-th value; a row past ns never passes
  float thr = live ? -INFINITY : INFINITY;

  const int64_t d0 = (int64_t)blockIdx.y * rows_per_slab;
  const int64_t d1 = d0 + rows_per_slab < nd ? d0 + rows_per_slab : nd;
  DstTile<NQ, VW> xt;
  xt.load(D, d0, ldd, d1 - d0, tid, r);
  for (int64_t p0 = d0; p0 < d1; p0 += kTile) {
    __syncthreads();  // every wave is past its reads of the previous tile (and the zeroing, at first)
    xt.store(tile, tid, r);
    if (p0 + kTile < d1) xt.load(D, p0 + kTile, ldd, d1 - (p0 + kTile), tid, r);
    __syncthreads();
    {
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
      const float* ap = tile + col * LD + 2 * half;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (q < nq) {
          const float2 dq = *reinterpret_cast<const float2*>(ap + 4 * q);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dq.x, sreg[q][0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dq.y, sreg[q][1], acc, 0, 0, 0);
        }
      }
      if (d1 - p0 < kTile) {  // the slab's last rows: the zero rows behind them are no destinations
        const int lim = (int)(d1 - p0);
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (acc_row(e, half) >= lim) acc[e] = __builtin_nanf("");
      }

      const bool filling = __ballot(thr == -INFINITY) != 0;  // a row of the wave has fewer than k entries
      const float t_in = thr;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float score = acc[e];  // a scalar copy: the lane read below takes its bits, not the vector element's
        unsigned long long pass = __ballot(filling ? score >= t_in : score > t_in);
        while (pass) {
          const int src = __builtin_ctzll(pass);
          pass &= pass - 1;
          const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(score), src));
          const int row = src & 31;
          const int pos = (int)p0 + acc_row(e, src >> 5);
          float a = 0.f, kth = 0.f;
          int b = 0;
          if (lane < k) {
            a = lv[row * k + lane];
            b = li[row * k + lane];
          }
          if (list_insert(a, b, lane, k, v, pos, kth)) {
            if (lane < k) {  // a lane reads and writes its own entry only
              lv[row * k + lane] = a;
              li[row * k + lane] = b;
            }
            if (col == row) thr = kth;
          }
        }
      }
    }
  }

  for (int row = 0; row < 32; ++row) {
    if (srow0 + row >= ns) break;
    if (lane < k) {
      const int64_t o = ((int64_t)blockIdx.y * ns + srow0 + row) * k + lane;
      const int b = li[row * k + lane];
      oval[o] = lv[row * k + lane];
      oidx[o] = b == kEmpty ? -1 : b;
    }
  }
}

// pval / pidx: [slabs][ns][k] the slabs' lists (position -1: the list ends); one wave per source row.
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ pval, const int* __restrict__ pidx,
                                                         int64_t ns, int k, int slabs, float* __restrict__ oval,
                                                         int* __restrict__ oidx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= ns) return;
  float a = -INFINITY;
  int b = kEmpty;
  if (lane < k) {
    const int i = pidx[row * k + lane];
    if (i >= 0) {
      a = pval[row * k + lane];
      b = i;
    }
  }
  for (int s = 1; s < slabs; ++s) {
    const int64_t base = ((int64_t)s * ns + row) * k;
    for (int t = 0; t < k; ++t) {
      const int i = pidx[base + t];
      float kth;
      if (i < 0 || !list_insert(a, b, lane, k, pval[base + t], i, kth)) break;  // the rest of the list is no better
    }
  }
  if (lane < k) {
    oval[row * k + lane] = a;
    oidx[row * k + lane] = b == kEmpty ? -1 : b;
  }
}

struct TopkPlan {
  bool native;
  int vw, NQ, slabs, per_cu;
  int64_t nsb, rows_per_slab;
  size_t lds, ws_bytes;
};

// The dispatch.  Source blocks x slabs: with enough source blocks to fill the machine one slab (no merge); otherwise
// the destinations are split into as many slabs as bring the grid to one round of resident blocks, each of at least
// kMinSlab rows and a multiple of the tile.  Resident blocks per CU: what the 160 KB of LDS admit and what the
// registers admit: 4 up to 32 columns (at most 99 registers a lane), 3 at 64 (139), 2 at 128 (196).
TopkPlan topk_plan(const float* S, int64_t ns, int64_t lds, const float* D, int64_t nd, int64_t ldd, int r, int k) {
  TopkPlan pl{};
  pl.native = ns >= 1 && nd >= 1 && nd <= INT_MAX && r >= 1 && r <= kMaxR && k >= 1 && k <= kMaxTopK && lds >= r &&
              ldd >= r && S != nullptr && D != nullptr;
  if (!pl.native) return pl;
  pl.vw = float4_rows(D, r, ldd) ? 4 : 1;
  pl.NQ = r <= 8 ? 2 : (r <= 16 ? 4 : (r <= 32 ? 8 : (r <= 64 ? 16 : 32)));
  pl.lds = lds_bytes(pl.NQ, k);
  pl.per_cu = (int)((size_t)160 * 1024 / pl.lds);
  const int by_regs = pl.NQ <= 8 ? 4 : (pl.NQ == 16 ? 3 : 2);
  if (pl.per_cu > by_regs) pl.per_cu = by_regs;
  pl.nsb = (ns + kSrcRows - 1) / kSrcRows;
  const int64_t round = (int64_t)kCUs * pl.per_cu;
  int64_t slabs = round / pl.nsb, most = (nd + kMinSlab - 1) / kMinSlab;
  if (slabs > most) slabs = most;
  if (slabs < 1) slabs = 1;
  pl.rows_per_slab = ((nd + slabs - 1) / slabs + kTile - 1) / kTile * kTile;
  pl.slabs = (int)((nd + pl.rows_per_slab - 1) / pl.rows_per_slab);  // every slab has rows
  pl.ws_bytes = pl.slabs > 1 ? (size_t)pl.slabs * ns * k * 8 : 0;
  return pl;
}

template <int NQ, int VW>
int topk_launch(const TopkPlan& pl, const float* S, int64_t ns, int64_t lds, const float* D, int64_t nd, int64_t ldd,
                int r, int k, float* oval, int* oidx, hipStream_t st) {
  if (pl.lds > 64 * 1024) {
    static bool raised[64] = {};
    const int rc =
        cdna::raise_lds(reinterpret_cast<const void*>(topk_kernel<NQ, VW>), raised, lds_bytes(NQ, kMaxTopK));
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL((topk_kernel<NQ, VW>), dim3((unsigned)pl.nsb, (unsigned)pl.slabs), dim3(256), pl.lds, st, S, ns,
                     lds, D, nd, ldd, r, k, pl.rows_per_slab, oval, oidx);
  return (int)hipGetLastError();
}

template <int VW>
int topk_launch_nq(const TopkPlan& pl, const float* S, int64_t ns, int64_t lds, const float* D, int64_t nd,
                   int64_t ldd, int r, int k, float* oval, int* oidx, hipStream_t st) {
  switch (pl.NQ) {
    case 2: return topk_launch<2, VW>(pl, S, ns, lds, D, nd, ldd, r, k, oval, oidx, st);
    case 4: return topk_launch<4, VW>(pl, S, ns, lds, D, nd, ldd, r, k, oval, oidx, st);
    case 8: return topk_launch<8, VW>(pl, S, ns, lds, D, nd, ldd, r, k, oval, oidx, st);
    case 16: return topk_launch<16, VW>(pl, S, ns, lds, D, nd, ldd, r, k, oval, oidx, st);
    default: return topk_launch<32, VW>(pl, S, ns, lds, D, nd, ldd, r, k, oval, oidx, st);
  }
}

}  // namespace

static_assert((size_t)kTile * (kMaxR + 2) * 4 + (size_t)kSrcRows * kMaxTopK * 8 <= 160 * 1024,
              "the widest plan fits the CU's LDS");

// What cdna_als_topk runs for these operands (nothing is launched): out = [native, load width of D (4: float4 rows,
// 1: scalar), source blocks, slabs, destination rows per slab, LDS bytes, workspace bytes, resident blocks per CU,
// columns the instantiation holds].
CDNA_API int cdna_als_topk_plan(const float* S, int64_t ns, int64_t lds, const float* D, int64_t nd, int64_t ldd,
                                int r, int k, int64_t* out) {
  const TopkPlan pl = topk_plan(S, ns, lds, D, nd, ldd, r, k);
  for (int i = 0; i < 9; ++i) out[i] = 0;
  if (!pl.native) return 0;
  out[0] = 1;
  out[1] = pl.vw;
  out[2] = pl.nsb;
  out[3] = pl.slabs;
  out[4] = pl.rows_per_slab;
  out[5] = (int64_t)pl.lds;
  out[6] = (int64_t)pl.ws_bytes;
  out[7] = pl.per_cu;
  out[8] = 4 * pl.NQ;
  return 0;
}

// S [ns, r] and D [nd, r] fp32 rows of stride lds and ldd; val [ns, k] fp32 and idx [ns, k] int32: per source row the
// k positions of the largest s . d, (score descending, position ascending), the tail (-inf, -1) when fewer qualify;
// ws: out[6] of the plan bytes, 8-byte aligned (unused with one slab).
CDNA_API int cdna_als_topk(const float* S, int64_t ns, int64_t lds, const float* D, int64_t nd, int64_t ldd, int r,
                           int k, float* val, int* idx, void* ws, hipStream_t st) {
  const TopkPlan pl = topk_plan(S, ns, lds, D, nd, ldd, r, k);
  if (!pl.native || val == nullptr || idx == nullptr || (pl.slabs > 1 && ws == nullptr))
    return (int)hipErrorInvalidValue;
  float* pval = val;
  int* pidx = idx;
  if (pl.slabs > 1) {
    pval = reinterpret_cast<float*>(ws);
    pidx = reinterpret_cast<int*>(pval + (size_t)pl.slabs * ns * k);
  }
  const int rc = pl.vw == 4 ? topk_launch_nq<4>(pl, S, ns, lds, D, nd, ldd, r, k, pval, pidx, st)
                            : topk_launch_nq<1>(pl, S, ns, lds, D, nd, ldd, r, k, pval, pidx, st);
  if (rc != 0 || pl.slabs == 1) return rc;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, st, pval, pidx, ns, k, pl.slabs,
                     val, idx);
  return (int)hipGetLastError();
}
