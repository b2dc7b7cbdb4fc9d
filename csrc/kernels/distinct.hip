// K29 col_distinct / col_recode — the set of distinct values of every column of a feature matrix, capped at cap + 1, in
// one pass over the rows (VectorIndexer's fit), and the recode of the categorical columns to their category indices
// (its transform).
//
// Key of an fp32 value: K28's order-preserving map u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000) of its bits u, after -0.0
// became +0.0 (the two are one category).  Unsigned key order is numeric order, +-inf are ordinary values.  A NaN has
// no key: the fit counts it per column and otherwise ignores it, the transform treats it as an unseen value.
//
// col_distinct_kernel<VW>: rowblock.h's scaffolding laid out like K27 COUNT / K28 FIRST: one round of resident blocks
// of 256 threads, 64-row tiles with the next tile of X prefetched in registers, rows past n never read; thread (column
// tid & 127, row half tid >> 7) owns its column for the block.  The thread keeps the distinct keys of its rows as a
// sorted list in LDS, set[(half (cap + 1) + slot) pitch + c], column innermost with the odd pitch d | 1: the lanes of
// a wave differ in c, so they hit different banks whatever slot each is at, and the list is the thread's own, so there
// are no atomics.  A value is first compared with the last key the thread hit (kept in a register: category columns
// repeat), then binary-searched, then inserted by shifting.  A list that would grow past cap entries marks the column
// overflowed (count = cap + 1, sticky) and the thread stops searching: a continuous column costs a handful of rows
// per block and then only the NaN test.  At the end of the block the half-1 list is merged into the half-0 list
// through LDS and the block writes keys [d][cap + 1], the count and the NaN count to its own workspace slot.
// col_distinct_merge_kernel: one wave per column walks the blocks' lists in block order (the next block's count and
// first 64 keys are prefetched); every lane searches the merged list for its key, and only a block that brings new
// keys (a ballot) makes lane 0 insert them.  The union of sets does not depend on the order or the grid: reruns are
// bit-identical.  An overflowed column ends its wave at once.
//
// col_recode_kernel<VW>: the same scaffolding.  The sorted key table of every categorical column and its index table
// (the category index of each sorted position: 0.0 first, the rest ascending) sit in LDS in the same odd-pitch layout;
// thread (column, half) binary-searches its 32 tile values and overwrites them with the index as fp32; continuous
// columns are not touched, so they pass through bit for bit.  The tile then goes out as whole rows (float4 where the
// rows of X and Y allow).  A value that is not in the table, NaN included, is counted per column into the block's own
// slot; under skip the row's byte in the drop mask is set, under keep the value becomes the number of categories,
// under error it passes through (the host raises after the pass).
//
// LDS: both kernels take 2 (cap + 1) (d | 1) 4 bytes beside the tile, within K27's 96 KiB budget: cdna_col_distinct_plan
// is the single source of whether that fits and of the blocks per CU.  No float atomics, no float arithmetic.
// Native range: fp32 rows, 1 <= d <= 128, cap within the plan, any n, row stride and alignment.
#include "rowblock.h"

namespace {

using namespace rowblock;

constexpr size_t kSetBudget = 96 * 1024;  // K27's COUNT budget
constexpr size_t kCuLds = 160 * 1024;
constexpr size_t kStaticLds = (size_t)kXF * 4 + 1024;  // the tile and the per-column / per-row words

enum { kError = 0, kSkip = 1, kKeep = 2 };

__device__ __forceinline__ bool key_of(float x, unsigned int& key) {
  unsigned int u = __float_as_uint(x);
  if ((u & 0x7FFFFFFFu) == 0u) u = 0u;  // -0.0 is +0.0
  key = u ^ ((u >> 31) != 0u ? 0xFFFFFFFFu : 0x80000000u);
  return (u & 0x7FFFFFFFu) <= 0x7F800000u;  // not a NaN
}

// the first position of the sorted list S[0 .. cnt) (stride pitch) whose key is not below `key`
__device__ __forceinline__ int lower_bound(const unsigned int* S, int pitch, int cnt, unsigned int key) {
  int lo = 0, hi = cnt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (S[mid * pitch] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// key into the sorted list of cnt <= cap keys; a list that would pass cap becomes cnt = cap + 1 (overflowed)
__device__ __forceinline__ void set_add(unsigned int* S, int pitch, int cap, int& cnt, unsigned int key) {
  const int lo = lower_bound(S, pitch, cnt, key);
  if (lo < cnt && S[lo * pitch] == key) return;
  if (cnt >= cap) {
    cnt = cap + 1;
    return;
  }
  for (int i = cnt; i > lo; --i) S[i * pitch] = S[(i - 1) * pitch];
  S[lo * pitch] = key;
  ++cnt;
}

// wk u32 [nblk][d][cap + 1], wcnt / wnan u32 [nblk][d]: the blocks' workspace slots
template <int VW>
__global__ __launch_bounds__(256) void col_distinct_kernel(const float* __restrict__ X, int64_t n, int64_t ldx, int d,
                                                           int cap, unsigned int* __restrict__ wk,
                                                           unsigned int* __restrict__ wcnt,
                                                           unsigned int* __restrict__ wnan, int64_t rows_per_block) {
  __shared__ __attribute__((aligned(16))) float xb[kXF];
  __shared__ unsigned int cntS[kMaxD], nanS[kMaxD];
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  unsigned int* set = reinterpret_cast<unsigned int*>(dyn);  // [2][cap + 1][pitch]
  const int tid = threadIdx.x;
  const int dv = d / VW, pitch = d | 1, w = cap + 1;

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  const int bc = tid & (kMaxD - 1), bh = tid >> 7;
  unsigned int* S = set + (bh * w) * pitch + bc;  // the thread's list (bc < d)
  int cnt = 0;
  unsigned int lastk = 0u, nanc = 0u;

  const auto side = [](int64_t, int) {};
  TileStream<VW> ts;
  ts.begin(xb, kXF, X, ldx, rb0, rb1, dv, tid, side);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    ts.put(xb, tid);
    ts.fetch(t0, tid, side);

    if (bc < d) {
      const float* xc = xb + (32 * bh) * kLD + bc;
      const int64_t left = rb1 - t0 - 32 * bh;  // the tile rows of this half that the block has
      const int nr = left >= 32 ? 32 : left > 0 ? (int)left : 0;
      if (cnt > cap) {  // overflowed: only the NaN count goes on
#pragma unroll 8
        for (int r = 0; r < nr; ++r) nanc += (__float_as_uint(xc[r * kLD]) & 0x7FFFFFFFu) > 0x7F800000u ? 1u : 0u;
      } else {
        for (int r = 0; r < nr; ++r) {
          unsigned int key;
          if (!key_of(xc[r * kLD], key)) {
            ++nanc;
            continue;
          }
          if (cnt > cap || (cnt > 0 && key == lastk)) continue;
          set_add(S, pitch, cap, cnt, key);
          lastk = key;
        }
      }
    }
  }

  // half 1 -> half 0
  __syncthreads();
  if (bh == 1 && bc < d) {
    cntS[bc] = (unsigned int)cnt;
    nanS[bc] = nanc;
  }
  __syncthreads();
  const int64_t slot = (int64_t)blockIdx.x * d;
  if (bh == 0 && bc < d) {
    const int c1 = (int)cntS[bc];
    const unsigned int* S1 = S + w * pitch;
    if (c1 > cap) cnt = w;
    for (int j = 0; j < c1 && cnt <= cap; ++j) set_add(S, pitch, cap, cnt, S1[j * pitch]);
    cntS[bc] = (unsigned int)cnt;
    wcnt[slot + bc] = (unsigned int)cnt;
    wnan[slot + bc] = nanc + nanS[bc];
  }
  __syncthreads();
  for (int i = tid; i < d * w; i += 256) {
    const int c = i / w, s = i - c * w;
    wk[slot * w + i] = s < (int)cntS[c] && s < cap ? set[s * pitch + c] : 0xFFFFFFFFu;
  }
}

// One wave per column c = blockIdx.x.  keys u32 [d][cap + 1] (slots from the count on, and every slot of an overflowed
// column, are 0xFFFFFFFF), count [d] (cap + 1: more than cap), nan [d].
__global__ __launch_bounds__(64) void col_distinct_merge_kernel(const unsigned int* __restrict__ wk,
                                                                const unsigned int* __restrict__ wcnt,
                                                                const unsigned int* __restrict__ wnan, int nblk, int d,
                                                                int cap, unsigned int* __restrict__ keys,
                                                                long long* __restrict__ count,
                                                                long long* __restrict__ nan) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  unsigned int* list = reinterpret_cast<unsigned int*>(dyn);  // [cap + 1]
  __shared__ unsigned int stage[64];
  const int c = blockIdx.x, lane = threadIdx.x, w = cap + 1;

  unsigned long long nn = 0ull;
  for (int b = lane; b < nblk; b += 64) nn += wnan[(int64_t)b * d + c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nn += __shfl_xor(nn, o);

  int cnt = 0;  // the same in every lane
  int cbn = (int)wcnt[c];
  unsigned int k0n = lane < w ? wk[(int64_t)c * w + lane] : 0u;
  for (int b = 0; b < nblk && cnt <= cap; ++b) {
    const int cb = cbn;
    const unsigned int k0 = k0n;
    const unsigned int* kb = wk + ((int64_t)b * d + c) * w;
    if (b + 1 < nblk) {  // the next block's count and first keys are on their way
      cbn = (int)wcnt[(int64_t)(b + 1) * d + c];
      k0n = lane < w ? kb[(int64_t)d * w + lane] : 0u;
    }
    if (cb > cap) {
      cnt = w;
      break;
    }
    for (int j0 = 0; j0 < cb; j0 += 64) {
      const int j = j0 + lane;
      const bool have = j < cb;
      const unsigned int key = j0 == 0 ? k0 : have ? kb[j] : 0u;
      bool isnew = false;
      if (have) {
        const int lo = lower_bound(list, 1, cnt, key);
        isnew = !(lo < cnt && list[lo] == key);
      }
      const unsigned long long m = __ballot(isnew);
      if (m == 0ull) continue;
      const int nnew = __popcll(m);
      if (cnt + nnew > cap) {  // the block's keys are distinct: the union has cnt + nnew
        cnt = w;
        break;
      }
      if (isnew) stage[__popcll(m & ((1ull << lane) - 1ull))] = key;
      __syncthreads();
      if (lane == 0) {
        int c0 = cnt;
        for (int t = 0; t < nnew; ++t) set_add(list, 1, cap, c0, stage[t]);
      }
      __syncthreads();
      cnt += nnew;
    }
  }
  for (int j = lane; j < w; j += 64) keys[(int64_t)c * w + j] = j < cnt && cnt <= cap ? list[j] : 0xFFFFFFFFu;
  if (lane == 0) {
    count[c] = cnt;
    nan[c] = (long long)nn;
  }
}

// tk / ti u32 [d][cap + 1]: the sorted keys of column c's ncat[c] categories and the category index of each sorted
// position (ncat[c] = 0: a continuous column).  Y fp32 [n][d] of row stride ldy, wbad u32 [nblk][d], drop u8 [n]
// (kSkip only; every byte is written).
template <int VW>
__global__ __launch_bounds__(256) void col_recode_kernel(const float* __restrict__ X, int64_t n, int64_t ldx, int d,
                                                         int cap, const unsigned int* __restrict__ tk,
                                                         const unsigned int* __restrict__ ti,
                                                         const int* __restrict__ ncat, int mode, float* __restrict__ Y,
                                                         int64_t ldy, unsigned int* __restrict__ wbad,
                                                         unsigned char* __restrict__ drop, int64_t rows_per_block) {
  typedef float vec_t __attribute__((ext_vector_type(VW)));
  __shared__ __attribute__((aligned(16))) float xb[kXF];
  __shared__ unsigned int dropS[kRows];
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  const int tid = threadIdx.x;
  const int dv = d / VW, pitch = d | 1, w = cap + 1;
  unsigned int* keyT = reinterpret_cast<unsigned int*>(dyn);  // [cap + 1][pitch]
  unsigned int* idxT = keyT + w * pitch;

  for (int i = tid; i < d * w; i += 256) {
    const int c = i / w, s = i - c * w;
    keyT[s * pitch + c] = tk[i];
    idxT[s * pitch + c] = ti[i];
  }
  if (tid < kRows) dropS[tid] = 0u;

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  const int bc = tid & (kMaxD - 1), bh = tid >> 7;
  const int nc = bc < d ? ncat[bc] : 0;
  const unsigned int* K = keyT + bc;
  unsigned int bad = 0u;

  const auto side = [](int64_t, int) {};
  TileStream<VW> ts;
  ts.begin(xb, kXF, X, ldx, rb0, rb1, dv, tid, side);  // its first barrier also covers the tables
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    ts.put(xb, tid);
    ts.fetch(t0, tid, side);

    if (nc > 0) {
      float* xc = xb + (32 * bh) * kLD + bc;
      const int64_t left = rb1 - t0 - 32 * bh;
      const int nr = left >= 32 ? 32 : left > 0 ? (int)left : 0;
      for (int r = 0; r < nr; ++r) {
        unsigned int key;
        const bool ok = key_of(xc[r * kLD], key);
        const int lo = ok ? lower_bound(K, pitch, nc, key) : nc;
        if (lo < nc && K[lo * pitch] == key) {
          xc[r * kLD] = (float)idxT[lo * pitch + bc];
          continue;
        }
        ++bad;
        if (mode == kSkip) dropS[32 * bh + r] = 1u;
        if (mode == kKeep) xc[r * kLD] = (float)nc;
      }
    }
    __syncthreads();

    // the tile goes out as whole rows, in the items of the load
#pragma unroll
    for (int i = 0; i < RowTile<VW>::kNI; ++i) {
      const int e = tid + 256 * i;
      const int r = e / dv, c = e - r * dv;
      if (e < 64 * dv && t0 + r < rb1) {
        vec_t v;
#pragma unroll
        for (int u = 0; u < VW; ++u) v[u] = xb[r * kLD + c * VW + u];
        *reinterpret_cast<vec_t*>(Y + (t0 + r) * ldy + (int64_t)c * VW) = v;
      }
    }
    if (mode == kSkip && tid < kRows && t0 + tid < rb1) {
      drop[t0 + tid] = (unsigned char)dropS[tid];
      dropS[tid] = 0u;
    }
  }

  // the halves' counts meet in the tile (put's barrier is behind the last tile's reads)
  __syncthreads();
  unsigned int* badS = reinterpret_cast<unsigned int*>(xb);
  if (bh == 1) badS[bc] = bad;
  __syncthreads();
  if (bh == 0 && bc < d) wbad[(int64_t)blockIdx.x * d + bc] = bad + badS[bc];
}

// cap + 1 lists of d | 1 words, twice (the two row halves; the key and the index table)
size_t set_bytes(int d, int cap) { return 2 * ((size_t)cap + 1) * (d | 1) * 4; }

struct DistinctPlan : RowSplit {
  bool native;
  int per_cu, max_cap;
  size_t dyn;
};

// One round of resident blocks on the 256 CUs, as many per CU as the LDS lets in (at most four); at least 1024 rows
// per block, and fewer than 2^31 (a block's u32 NaN count cannot wrap).  n = 0: no block.
DistinctPlan distinct_plan(int64_t n, int d, int cap) {
  DistinctPlan pl{};
  if (n < 0 || d < 1 || d > kMaxD || cap < 1) return pl;
  pl.max_cap = (int)(kSetBudget / (8 * (size_t)(d | 1))) - 1;
  if (cap > pl.max_cap) return pl;
  pl.native = true;
  pl.dyn = set_bytes(d, cap);
  pl.per_cu = (int)(kCuLds / (kStaticLds + pl.dyn));
  if (pl.per_cu > 4) pl.per_cu = 4;
  if (n == 0) return pl;
  static_cast<RowSplit&>(pl) = split_rows(n, (int64_t)pl.per_cu * 256, (n + (((int64_t)1 << 31) - 1)) >> 31);
  return pl;
}

template <class Kern>
int raise_once(Kern kern, bool* raised) {
  return cdna::raise_lds(reinterpret_cast<const void*>(kern), raised, kSetBudget);
}

}  // namespace

static_assert(kStaticLds % 16 == 0, "the lists start aligned");
static_assert(kStaticLds + kSetBudget <= kCuLds, "a block at the budget fits a CU");
static_assert(kSetBudget / (8 * (size_t)(kMaxD | 1)) - 1 == 94, "cap <= 94 at d = 128");

// What cdna_col_distinct and cdna_col_recode run for these operands (nothing is launched): out [8] = [native, load
// width (4: float4 rows, 1: scalar), blocks, rows per block, LDS bytes per block, blocks per CU, the largest native cap
// for d, 0].
CDNA_API int cdna_col_distinct_plan(const float* X, int64_t n, int64_t ldx, int d, int cap, int64_t* out) {
  const DistinctPlan pl = distinct_plan(n, d, cap);
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[6] = pl.max_cap;
  if (!pl.native || ldx < d) return 0;
  out[0] = 1;
  out[1] = float4_rows(X, d, ldx) ? 4 : 1;
  out[2] = pl.nblk;
  out[3] = pl.rows_per_block;
  out[4] = (int64_t)(kStaticLds + pl.dyn);
  out[5] = pl.per_cu;
  return 0;
}

// u32 words of cdna_col_distinct's workspace: [wk [nblk][d][cap + 1] | wcnt [nblk][d] | wnan [nblk][d]]
CDNA_API int64_t cdna_col_distinct_workspace(int64_t n, int d, int cap) {
  const DistinctPlan pl = distinct_plan(n, d, cap);
  return pl.native ? (int64_t)pl.nblk * d * (cap + 3) : 0;
}

// The distinct values of the columns of X [n][d], n > 0.  out = i64 [2 d] = [count [d] | nan [d]] and then u32
// keys [d][cap + 1]; ws: cdna_col_distinct_workspace words.  Every word of out is written.
CDNA_API int cdna_col_distinct(const float* X, int64_t n, int64_t ldx, int d, int cap, unsigned int* ws, void* out,
                               hipStream_t st) {
  const DistinctPlan pl = distinct_plan(n, d, cap);
  if (!pl.native || n < 1 || ldx < d || X == nullptr || ws == nullptr || out == nullptr)
    return (int)hipErrorInvalidValue;
  static bool raised[2][64] = {};
  const bool vec = float4_rows(X, d, ldx);
  const int rc = vec ? raise_once(col_distinct_kernel<4>, raised[0]) : raise_once(col_distinct_kernel<1>, raised[1]);
  if (rc != 0) return rc;
  unsigned int* wk = ws;
  unsigned int* wcnt = wk + (int64_t)pl.nblk * d * (cap + 1);
  unsigned int* wnan = wcnt + (int64_t)pl.nblk * d;
  if (vec)
    hipLaunchKernelGGL(col_distinct_kernel<4>, dim3(pl.nblk), dim3(256), pl.dyn, st, X, n, ldx, d, cap, wk, wcnt, wnan,
                       pl.rows_per_block);
  else
    hipLaunchKernelGGL(col_distinct_kernel<1>, dim3(pl.nblk), dim3(256), pl.dyn, st, X, n, ldx, d, cap, wk, wcnt, wnan,
                       pl.rows_per_block);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  long long* count = static_cast<long long*>(out);
  hipLaunchKernelGGL(col_distinct_merge_kernel, dim3(d), dim3(64), ((size_t)cap + 1) * 4, st, wk, wcnt, wnan, pl.nblk,
                     d, cap, reinterpret_cast<unsigned int*>(count + 2 * d), count, count + d);
  return (int)hipGetLastError();
}

// The recode of X [n][d], n > 0, into Y [n][d] of row stride ldy by the tables tk / ti u32 [d][cap + 1] and ncat i32
// [d] (see col_recode_kernel); mode 0 error, 1 skip, 2 keep.  wbad u32 [blocks of the plan][d]; drop u8 [n] (skip).
CDNA_API int cdna_col_recode(const float* X, int64_t n, int64_t ldx, int d, int cap, const unsigned int* tk,
                             const unsigned int* ti, const int* ncat, int mode, float* Y, int64_t ldy,
                             unsigned int* wbad, unsigned char* drop, hipStream_t st) {
  const DistinctPlan pl = distinct_plan(n, d, cap);
  if (!pl.native || n < 1 || ldx < d || ldy < d || X == nullptr || Y == nullptr || tk == nullptr || ti == nullptr ||
      ncat == nullptr || wbad == nullptr || mode < kError || mode > kKeep || (mode == kSkip && drop == nullptr))
    return (int)hipErrorInvalidValue;
  static bool raised[2][64] = {};
  const bool vec = float4_rows(X, d, ldx) && float4_rows(Y, d, ldy);
  const int rc = vec ? raise_once(col_recode_kernel<4>, raised[0]) : raise_once(col_recode_kernel<1>, raised[1]);
  if (rc != 0) return rc;
  if (vec)
    hipLaunchKernelGGL(col_recode_kernel<4>, dim3(pl.nblk), dim3(256), pl.dyn, st, X, n, ldx, d, cap, tk, ti, ncat,
                       mode, Y, ldy, wbad, drop, pl.rows_per_block);
  else
    hipLaunchKernelGGL(col_recode_kernel<1>, dim3(pl.nblk), dim3(256), pl.dyn, st, X, n, ldx, d, cap, tk, ti, ncat,
                       mode, Y, ldy, wbad, drop, pl.rows_per_block);
  return (int)hipGetLastError();
}
