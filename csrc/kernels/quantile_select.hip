// K28 col_digit_hist / col_select — exact order statistics of every column of a feature matrix by an MSB-first radix
// select (RobustScaler's median and quantiles, MaxAbsScaler's extrema).
//
// Key of an fp32 value: u = bits(x); u ^= (u >> 31) ? 0xFFFFFFFF : 0x80000000.  Unsigned order of the keys is numeric
// order: -0.0 sorts just below +0.0, +-inf are ordinary values at the ends.  A NaN of either sign has no key: it is
// counted per column and otherwise ignored.  With m non-NaN values in a column, the quantile for probability q is the
// value whose key has the 1-based rank r = min(max(ceil(q m), 1), m), the product taken in fp64; m = 0 gives NaN.
//
// One pass is one launch of col_digit_hist_kernel<MODE, VW> on rowblock.h's scaffolding, laid out like K27 COUNT
// (select.hip): 256 threads, 64-row tiles, the next tile of X prefetched in registers; thread (column tid & 127, row
// half tid >> 7) owns its column and a wave reads 64 consecutive floats of a tile row.  Rows past the end of the
// block's range are never read from memory, and the tile's rows past it are not counted.
//   FIRST (pass 0): every non-NaN value adds 1 to cell[digit * pitch + c], digit = key >> shift (shift = 32 - bits);
//     the thread keeps the column's smallest and largest key and its NaN count in registers, which go out at the end
//     of the block as atomicMin / atomicMax on u32 words and atomicAdd on 64-bit counts.
//   NEXT: with hi = key >> (shift + bits) (shift + bits < 32: no shift by 32 is ever executed), every target t < Q
//     with hi == prefix[c][t] adds 1 to cell[(digit * Q + t) * pitch + c], digit = (key >> shift) & (2^bits - 1).
//     Targets that share a prefix (a constant column) each get their own identical counts.
// The cells are u32 in LDS with the column innermost and the odd pitch d | 1 (the lanes of a wave differ in c and in
// the digit, so they spread over the banks), updated with LDS integer atomics and flushed once per block into the
// int64 table [d][Q'][2^bits] with global 64-bit integer atomics (zero cells are skipped).  The plan keeps a block's
// row range below 2^31, so a cell cannot wrap.  No float atomics anywhere: reruns are bit-identical, and per-rank
// tables all-reduce exactly.
// The table has K27's LDS budget of 96 KiB beside the 33 KB tile.  B(Q') is the largest b <= 8 with
// Q' 2^b (d | 1) 4 <= budget; pass 0 takes B(1) bits and every later pass min(B(Q), bits left): col_plan is the single
// source of the widths.
//
// col_select_kernel: one block, one thread per (column, target), on the (all-reduced) table.  After pass 0 it forms
// m = sum hist and the rank; in every pass it finds the smallest digit g with cum(hist[0 .. g]) >= r, sets
// prefix = (prefix << bits) | g and r -= cum(hist[0 .. g - 1]).  After the last pass the prefix is the key and the
// thread writes the fp32 value (NaN when m = 0).  Prefixes and ranks stay on the device between the passes.
// Native range: fp32 rows, 1 <= d <= 128, 1 <= Q <= 8 (B(Q) >= 4 at d = 128), any n, row stride and alignment.
#include "rowblock.h"

namespace {

using namespace rowblock;

constexpr int kMaxQ = 8;
constexpr int kMaxBits = 8;
constexpr int kKeyBits = 32;
constexpr size_t kTableBudget = 96 * 1024;  // K27's COUNT budget
constexpr size_t kCuLds = 160 * 1024;
constexpr size_t kStaticLds = (size_t)kXF * 4;  // the tile

enum { kFirst = 0, kNext = 1 };

struct ColParams {
  int d, Q, pitch, shift, bits;
};

__device__ __forceinline__ bool key_of(float x, unsigned int& key) {
  const unsigned int u = __float_as_uint(x);
  key = u ^ ((u >> 31) != 0u ? 0xFFFFFFFFu : 0x80000000u);
  return (u & 0x7FFFFFFFu) <= 0x7F800000u;  // not a NaN
}

// VW = 4: float4 row loads, VW = 1: scalar loads, any layout.  out: hist [d][Q'][2^bits] (Q' = 1 in FIRST).
template <int MODE, int VW>
__global__ __launch_bounds__(256) void col_digit_hist_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const unsigned int* __restrict__ prefix, const ColParams pr,
    unsigned long long* __restrict__ hist, unsigned long long* __restrict__ nan, unsigned int* __restrict__ kmin,
    unsigned int* __restrict__ kmax, int64_t rows_per_block) {
  __shared__ __attribute__((aligned(16))) float xb[kXF];
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  unsigned int* cell = reinterpret_cast<unsigned int*>(dyn);  // [2^bits Q'][pitch]
  const int tid = threadIdx.x;
  const int d = pr.d, dv = d / VW;
  const int Q = MODE == kFirst ? 1 : pr.Q;
  const int ncell = (Q << pr.bits) * pr.pitch;

  for (int i = tid; i < ncell; i += 256) cell[i] = 0u;

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  const int bc = tid & (kMaxD - 1), bh = tid >> 7;
  unsigned int pf[kMaxQ] = {};  // NEXT: the column's target prefixes
  if (MODE == kNext && bc < d) {
#pragma unroll
    for (int t = 0; t < kMaxQ; ++t)
      if (t < Q) pf[t] = prefix[bc * Q + t];
  }
  const unsigned int mask = (1u << pr.bits) - 1u;
  const int hshift = pr.shift + pr.bits;  // NEXT: < 32
  unsigned int kmn = 0xFFFFFFFFu, kmx = 0u, nanc = 0u;

  const auto side = [](int64_t, int) {};
  TileStream<VW> ts;
  ts.begin(xb, kXF, X, ldx, rb0, rb1, dv, tid, side);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    ts.put(xb, tid);
    ts.fetch(t0, tid, side);

    if (bc < d) {
      const float* xc = xb + (32 * bh) * kLD + bc;
      unsigned int* cc = cell + bc;
      // the tile rows of this half that the block has
      const int64_t left = rb1 - t0 - 32 * bh;
      const int nr = left >= 32 ? 32 : left > 0 ? (int)left : 0;
#pragma unroll 8
      for (int r = 0; r < nr; ++r) {
        unsigned int key;
        if (!key_of(xc[r * kLD], key)) {
          ++nanc;
          continue;
        }
        if (MODE == kFirst) {
          kmn = key < kmn ? key : kmn;
          kmx = key > kmx ? key : kmx;
          atomicAdd(cc + (key >> pr.shift) * pr.pitch, 1u);
        } else {
          const unsigned int hi = key >> hshift;
          const int dq = (int)((key >> pr.shift) & mask) * Q;
#pragma unroll
          for (int t = 0; t < kMaxQ; ++t)
            if (t < Q && hi == pf[t]) atomicAdd(cc + (dq + t) * pr.pitch, 1u);
        }
      }
    }
  }

  __syncthreads();
  const int nd = 1 << pr.bits;
  for (int i = tid; i < ncell; i += 256) {
    const unsigned int v = cell[i];
    const int q = i / pr.pitch, c = i - q * pr.pitch;  // q = digit Q' + t
    const int g = q / Q, t = q - g * Q;
    if (v != 0u && c < d) atomicAdd(hist + ((int64_t)c * Q + t) * nd + g, (unsigned long long)v);
  }
  if (MODE == kFirst && bc < d) {
    if (nanc != 0u) atomicAdd(nan + bc, (unsigned long long)nanc);
    if (kmn <= kmx) {  // the thread saw a value
      atomicMin(kmin + bc, kmn);
      atomicMax(kmax + bc, kmx);
    }
  }
}

// One block, thread i = (column i / Q, target i % Q).  hist [d][Q'][2^bits] int64 (Q' = 1 when first).  first: count [d]
// = m and rank [d][Q] from probs [Q] are formed here; otherwise they and prefix [d][Q] are read and updated.  last:
// out [Q][d] = the value of key prefix, NaN when m = 0.
// No FMA contraction: the rank's product q m is rounded to fp64 as the host formulation rounds it.
#pragma clang fp contract(off)
__global__ __launch_bounds__(1024) void col_select_kernel(const long long* __restrict__ hist, int d, int Q, int bits,
                                                          int first, int last, const double* __restrict__ probs,
                                                          unsigned int* __restrict__ prefix,
                                                          long long* __restrict__ rank, long long* __restrict__ count,
                                                          float* __restrict__ out) {
  const int i = threadIdx.x;
  if (i >= d * Q) return;
  const int c = i / Q, t = i - c * Q;
  const int nd = 1 << bits;
  const long long* h = hist + (int64_t)(first ? c : i) * nd;
  long long r, m;
  unsigned int pre = 0u;
  if (first) {
    m = 0;
#pragma unroll 8
    for (int g = 0; g < nd; ++g) m += h[g];
    const double p = ceil(probs[t] * (double)m);
    r = p >= (double)m ? m : (long long)p;  // m < 2^63: the comparison guards the conversion
    r = r < 1 ? 1 : r;
    r = r > m ? m : r;
    if (t == 0) count[c] = m;
  } else {
    m = count[c];
    r = rank[i];
    pre = prefix[i];
  }
  // the digits whose inclusive cumulative count stays below r come before the rank's digit
  long long cum = 0, below = 0;
  unsigned int g_sel = 0u;
#pragma unroll 8
  for (int g = 0; g < nd; ++g) {
    const long long v = h[g];
    cum += v;
    const bool lt = cum < r;
    g_sel += lt ? 1u : 0u;
    below += lt ? v : 0;
  }
  pre = first ? g_sel : (pre << bits) | g_sel;
  prefix[i] = pre;
  rank[i] = r - below;
  if (last) {
    const unsigned int u = pre ^ ((pre >> 31) != 0u ? 0x80000000u : 0xFFFFFFFFu);
    out[(int64_t)t * d + c] = m > 0 ? __uint_as_float(u) : __uint_as_float(0x7FC00000u);
  }
}

// B(Q'): the widest digit whose table fits the budget (0: none does)
int max_bits(int d, int Q) {
  int b = kMaxBits;
  while (b > 0 && ((size_t)Q << b) * (d | 1) * 4 > kTableBudget) --b;
  return b;
}

struct ColPlan : RowSplit {
  bool native;
  int b1, bq;  // B(1), B(Q)
  int npass, widths[kKeyBits];
  size_t dyn;  // the widest pass's table in bytes
};

size_t table_bytes(int d, int Q, int bits) { return ((size_t)Q << bits) * (d | 1) * 4; }

// One round of resident blocks on the 256 CUs, as many per CU as the LDS of a pass at full width lets in (at most
// four); at least 1024 rows per block, and fewer than 2^31 (a u32 cell cannot wrap).  n = 0: no block.
ColPlan col_plan(int64_t n, int d, int Q) {
  ColPlan pl{};
  if (n < 0 || d < 1 || d > kMaxD || Q < 1 || Q > kMaxQ) return pl;
  pl.b1 = max_bits(d, 1);
  pl.bq = max_bits(d, Q);
  if (pl.b1 < 1 || pl.bq < 1) return pl;
  pl.native = true;
  pl.widths[pl.npass++] = pl.b1;
  pl.dyn = table_bytes(d, 1, pl.b1);
  for (int left = kKeyBits - pl.b1; left > 0;) {
    const int b = pl.bq < left ? pl.bq : left;
    pl.widths[pl.npass++] = b;
    left -= b;
    if (table_bytes(d, Q, b) > pl.dyn) pl.dyn = table_bytes(d, Q, b);
  }
  if (n == 0) return pl;
  int per_cu = (int)(kCuLds / (kStaticLds + pl.dyn));
  if (per_cu > 4) per_cu = 4;
  static_cast<RowSplit&>(pl) = split_rows(n, (int64_t)per_cu * 256, (n + (((int64_t)1 << 31) - 1)) >> 31);
  return pl;
}

template <int MODE, int VW>
int hist_launch(const ColPlan& pl, size_t dyn, const float* X, int64_t n, int64_t ldx, const unsigned int* prefix,
                const ColParams& pr, unsigned long long* hist, unsigned long long* nan, unsigned int* kmin,
                unsigned int* kmax, hipStream_t st) {
  static bool raised[64] = {};
  const int rc = cdna::raise_lds(reinterpret_cast<const void*>(col_digit_hist_kernel<MODE, VW>), raised, kTableBudget);
  if (rc != 0) return rc;
  hipLaunchKernelGGL((col_digit_hist_kernel<MODE, VW>), dim3(pl.nblk), dim3(256), dyn, st, X, n, ldx, prefix, pr, hist,
                     nan, kmin, kmax, pl.rows_per_block);
  return (int)hipGetLastError();
}

}  // namespace

static_assert(kStaticLds % 16 == 0, "the table starts aligned");
static_assert(kStaticLds + kTableBudget <= kCuLds, "a block at the table budget fits a CU");
static_assert(((size_t)kMaxQ << 4) * (kMaxD | 1) * 4 <= kTableBudget, "B(Q) >= 4 over the native range");
static_assert(kMaxD * kMaxQ <= 1024, "one select thread per (column, target)");

// What cdna_col_digit_hist and the passes of a quantile call run for these operands (nothing is launched): out [8 + 32]
// = [native, load width (4: float4 rows, 1: scalar), blocks, rows per block, LDS bytes per block at the widest pass,
// B(1), B(Q), passes | the passes' digit widths].
CDNA_API int cdna_col_quantiles_plan(const float* X, int64_t n, int64_t ldx, int d, int Q, int64_t* out) {
  const ColPlan pl = col_plan(n, d, Q);
  for (int i = 0; i < 8 + kKeyBits; ++i) out[i] = 0;
  if (!pl.native || ldx < d) return 0;
  out[0] = 1;
  out[1] = float4_rows(X, d, ldx) ? 4 : 1;
  out[2] = pl.nblk;
  out[3] = pl.rows_per_block;
  out[4] = (int64_t)(kStaticLds + pl.dyn);
  out[5] = pl.b1;
  out[6] = pl.bq;
  out[7] = pl.npass;
  for (int i = 0; i < pl.npass; ++i) out[8 + i] = pl.widths[i];
  return 0;
}

// One pass of a call for Q targets.  prefix == nullptr: FIRST (shift + bits == 32, bits <= B(1)); out = u64 [d 2^bits + d] = [hist [d][2^bits] |
// nan [d]] and then u32 [2 d] = [kmin [d] | kmax [d]] (0xFFFFFFFF / 0 for a column without a value).  Otherwise NEXT
// with prefix u32 [d][Q] (shift + bits < 32, bits <= B(Q)); out = u64 hist [d][Q][2^bits].  out is cleared here;
// n = 0 launches nothing.
CDNA_API int cdna_col_digit_hist(const float* X, int64_t n, int64_t ldx, int d, int Q, int bits, int shift,
                                 const unsigned int* prefix, void* out, hipStream_t st) {
  const bool first = prefix == nullptr;
  const ColPlan pl = col_plan(n, d, Q);  // FIRST too: every pass of a call for Q targets splits the rows alike
  if (!pl.native || ldx < d || out == nullptr || (n > 0 && X == nullptr)) return (int)hipErrorInvalidValue;
  if (bits < 1 || shift < 0 || bits > (first ? pl.b1 : pl.bq)) return (int)hipErrorInvalidValue;
  if (first ? shift + bits != kKeyBits : shift + bits >= kKeyBits) return (int)hipErrorInvalidValue;
  const int Qe = first ? 1 : Q;
  const size_t cells = ((size_t)d * Qe) << bits;
  unsigned long long* hist = static_cast<unsigned long long*>(out);
  unsigned int* kmin = reinterpret_cast<unsigned int*>(hist + cells + d);
  hipError_t e = hipMemsetAsync(out, 0, (cells + (first ? 2 * (size_t)d : 0)) * 8, st);
  if (e == hipSuccess && first) e = hipMemsetAsync(kmin, 0xFF, (size_t)d * 4, st);
  if (e != hipSuccess) return (int)e;
  if (n == 0) return 0;
  const ColParams pr{d, Qe, d | 1, shift, bits};
  const size_t dyn = table_bytes(d, Qe, bits);
  const bool vec = float4_rows(X, d, ldx);
  if (first)
    return vec ? hist_launch<kFirst, 4>(pl, dyn, X, n, ldx, prefix, pr, hist, hist + cells, kmin, kmin + d, st)
               : hist_launch<kFirst, 1>(pl, dyn, X, n, ldx, prefix, pr, hist, hist + cells, kmin, kmin + d, st);
  return vec ? hist_launch<kNext, 4>(pl, dyn, X, n, ldx, prefix, pr, hist, nullptr, nullptr, nullptr, st)
             : hist_launch<kNext, 1>(pl, dyn, X, n, ldx, prefix, pr, hist, nullptr, nullptr, nullptr, st);
}

// The select step of one pass on the (all-reduced) table hist int64 [d][Q'][2^bits]: see col_select_kernel.
// probs f64 [Q], prefix u32 [d][Q], rank i64 [d][Q], count i64 [d], out f32 [Q][d], all on the device.
CDNA_API int cdna_col_select(const void* hist, int d, int Q, int bits, int first, int last, const double* probs,
                             unsigned int* prefix, void* rank, void* count, float* out, hipStream_t st) {
  if (d < 1 || d > kMaxD || Q < 1 || Q > kMaxQ || bits < 1 || bits > kMaxBits) return (int)hipErrorInvalidValue;
  if (hist == nullptr || probs == nullptr || prefix == nullptr || rank == nullptr || count == nullptr ||
      out == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(col_select_kernel, dim3(1), dim3((unsigned)((d * Q + 63) / 64 * 64)), 0, st,
                     static_cast<const long long*>(hist), d, Q, bits, first, last, probs, prefix,
                     static_cast<long long*>(rank), static_cast<long long*>(count), out);
  return (int)hipGetLastError();
}
