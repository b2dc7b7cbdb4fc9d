// Shared scaffolding of the kernels that stream the rows of X once in one round of resident blocks of 256 threads, each
// block walking its own contiguous row range in 64-row tiles (K24 mlp.hip, K25 fm.hip, K26 aft.hip, K27 select.hip;
// K1, K22 and K23 take the row range, the register prefetch and the block sum): the row split, the tile and its
// pipeline, and the fixed-order sum of the blocks' workspace slots.  symtile.h builds on it.
#pragma once
#include "common.h"

namespace rowblock {

// The tile: 64 rows of up to 128 columns, row-major fp32 in LDS with the odd row stride 129 (column reads of 32 or 64
// rows hit different banks), zeroed once so that the columns from d on stay zero.  Per-column sums over a tile belong
// to thread (column tid & 127, row half tid >> 7): a wave reads 64 consecutive floats of one tile row.
constexpr int kRows = 64;
constexpr int kMaxD = 128;
constexpr int kLD = kMaxD + 1;
constexpr int kXF = kRows * kLD;  // floats

// n rows over at most `cap` blocks (one round of resident blocks: the caller's cap says how many fit) and at least
// `least`: at least 1024 rows per block, a multiple of the tile.
struct RowSplit {
  int nblk;
  int64_t rows_per_block;
};
inline RowSplit split_rows(int64_t n, int64_t cap, int64_t least = 1) {
  int64_t nb = (n + 1023) / 1024;
  if (nb > cap) nb = cap;
  if (nb < least) nb = least;
  const int64_t rpb = ((n + nb - 1) / nb + kRows - 1) / kRows * kRows;
  return {(int)((n + rpb - 1) / rpb), rpb};  // every block has rows
}

// rows rb0 .. rb1 - 1 are this block's
__device__ __forceinline__ void block_rows(int64_t rows_per_block, int64_t n, int64_t& rb0, int64_t& rb1) {
  rb0 = (int64_t)blockIdx.x * rows_per_block;
  rb1 = rb0 + rows_per_block;
  if (rb1 > n) rb1 = n;
}

// rows of X addressable as float4: what the VW = 4 kernels need
inline bool float4_rows(const float* X, int d, int64_t ldx) {
  return d % 4 == 0 && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
}

// A thread's share of a 64-row tile of X, held in registers while the previous tile is worked on: 64 rows x dv =
// d / VW load items over 256 threads, item e = (row e / dv, load item e % dv).  VW = 4: float4 row loads (rows
// float4-addressable, see float4_rows); VW = 1: scalar loads, any layout.  K22 keeps the same loops as macros (this
// form costs it registers, see glm.hip).
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

// The tile pipeline of a block over its rows rb0 .. rb1 - 1: while tile t0 is worked on in LDS, tile t0 + 64 is on its
// way to registers.  side(t, tid) issues the kernel's own loads for the tile that starts at row t (labels, y, log t),
// so that they are in flight with the rows; the kernel copies what it loaded for tile t0 before fetch() replaces it.
//   begin(..);  for (t0 = rb0; t0 < rb1; t0 += kRows) { put(tile, tid);  fetch(t0, tid, side);  .. work on the tile }
// tid is passed in: K24 and K25 hand the loop an opaque copy of it (see mlp.hip).
template <int VW>
struct TileStream {
  RowTile<VW> xt;
  const float* X;
  int64_t ldx, rb1;
  int dv;

  // zero `floats` floats from `tile` on (the tile and the buffers behind it) once, and fetch the block's first tile
  template <class Side>
  __device__ __forceinline__ void begin(float* tile, int floats, const float* __restrict__ X_, int64_t ldx_,
                                        int64_t rb0, int64_t rb1_, int dv_, int tid, Side side) {
    X = X_, ldx = ldx_, rb1 = rb1_, dv = dv_;
    for (int i = tid; i < floats; i += 256) tile[i] = 0.f;
    if (rb0 < rb1) {
      xt.load(X, rb0, ldx, rb1 - rb0, tid, dv);
      side(rb0, tid);
    }
  }

  // the fetched tile -> LDS
  __device__ __forceinline__ void put(float* tile, int tid) const {
    __syncthreads();  // every wave is past its reads of the previous tile (and the zeroing, at first)
    xt.store(tile, kLD, tid, dv, [](int, int, float x) { return x; });
  }

  // the tile after t0 -> registers, if the block has one; then the tile in LDS is complete
  template <class Side>
  __device__ __forceinline__ void fetch(int64_t t0, int tid, Side side) {
    if (t0 + kRows < rb1) {
      xt.load(X, t0 + kRows, ldx, rb1 - (t0 + kRows), tid, dv);
      side(t0 + kRows, tid);
    }
    __syncthreads();
  }
};

// The fixed-order sum over blocks, by a block of 256 threads for 16 output values at a time: thread (el = tid & 15,
// part = tid >> 4) sums what add(b, s) adds for the blocks b = part, part + 16, .. of value el, then thread (el, 0)
// sums the 16 parts in the order q = 0 .. 15.  Deterministic, and 16x the parallelism of one thread per value (the
// serial 1024-block loop took 0.35 ms of a 3.6 ms fit).  NV values per thread share the loop over the blocks.  ok: the
// thread has a value; t is the total in the threads with part == 0 and ok.
template <int NV, class Add>
__device__ __forceinline__ void sum_blocks(double (&red)[NV][16][16], int nblk, bool ok, double (&t)[NV], Add add) {
  const int el = threadIdx.x & 15, part = threadIdx.x >> 4;
  double s[NV] = {};
  if (ok)
    for (int b = part; b < nblk; b += 16) add(b, s);
#pragma unroll
  for (int v = 0; v < NV; ++v) red[v][part][el] = s[v];
  __syncthreads();
#pragma unroll
  for (int v = 0; v < NV; ++v) t[v] = 0.0;
  if (part != 0 || !ok) return;
#pragma unroll
  for (int q = 0; q < 16; ++q)
#pragma unroll
    for (int v = 0; v < NV; ++v) t[v] += red[v][q][el];
}

// one value per thread: src(b) is block b's
template <class Src>
__device__ __forceinline__ double sum_blocks(double (&red)[16][16], int nblk, bool ok, Src src) {
  double t[1];
  sum_blocks<1>(reinterpret_cast<double (&)[1][16][16]>(red), nblk, ok, t, [&](int b, double* s) { s[0] += src(b); });
  return t[0];
}

}  // namespace rowblock
