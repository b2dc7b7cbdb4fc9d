// K33 bisect_step — one level step of bisecting k-means (which side of its leaf's bisector every row takes, and the
// children's weight sums, row counts, weighted row sums and weighted square sums), the commit of a level, or the
// descent of a fitted tree with its cost, in one pass over the rows and without atomics.
//
// One table of M split entries drives every mode.  Entry e: a hyperplane h_e [d] (fp32), a threshold t_e (fp64) and two
// targets; a target >= 0 is another entry, a target < 0 the leaf -1 - target.  A row takes the right side iff
// x~ . h_e > t_e: equality goes left.  A missing child is h = 0 with t = +inf (everything left) or -inf (everything
// right): the test needs no special case.  x~ = fl32(x - shift) (Euclidean; shift a caller-supplied fp32 vector) or x
// (cosine: the side does not depend on |x|, and the sums take x^ = x / max(|x|, 1e-30)).
//
// bisect_kernel: 256 threads, 64-row tiles, the next tile of X prefetched in registers (rowblock.h's row split, tile
// and pipeline).  The tile is row-major fp32 in LDS at stride kLD, shifted on its way in; the M hyperplanes sit behind
// it in LDS, row-major at the odd stride 32 Td + 1 (rows of a wave stand at different entries: a gathered read).
//   side:    four threads per row, 32 columns each (staggered starts), form |x~|^2 and x~ . h_e of the row's own entry in
//            fp64 on the VALU and combine by lane shuffles: d fp64 FMAs per row against 4 d bytes of traffic, and no
//            fp32 rounding in the test.  A row whose |x~|^2 is NaN or >= 2^120 is bad: left (PREDICT: leaf 0), counted,
//            and it adds exactly nothing to the sums (its tile row is zeroed); the PREDICT cost becomes NaN or +inf.
//   STEP:    node[r] (read only) is the row's entry, -1: the row adds nothing.  Child slot 2 e + side.  S = A^T X~
//            [2 M][d] on v_mfma_f32_32x32x2_f32, A[r][slot] = fl32(w_r): A is one-hot per row, so the A operand is
//            formed in registers from the tile rows' slots and weights in LDS (two broadcast reads and a select per
//            MFMA) and no [64][2 M] buffer exists.  32 x 32 tiles dealt round-robin to the waves (SLOTS each), fp32
//            accumulators for kFoldTiles tiles, then folded into the block's fp64 slab (each element owned by one
//            lane).  W, cnt (threads 0 .. 127, one slot each) and Q (threads 128 .. 255) in fp64, tile-row order.
//   ASSIGN:  the same test; node[r] <- the target of the row's side.
//   PREDICT: every row starts at entry 0 and walks until a target is a leaf (targets point forward, so at most M
//            steps; the loop is wave-uniform).  The leaf centres [L][32 Td] fp32 stay in global memory (64 KiB at
//            d = L = 128, L2-resident): LDS holds the rows and up to 128 hyperplanes (101 KiB), and a row reads one
//            centre once, at the end of its walk.  D = sum (x~ - c~)^2 in the direct form, or 1 - x . c^ / |x|, fp64.
// bisect_reduce_kernel: slabs, W, cnt, Q, cost and bad count of the blocks summed in a fixed order in fp64 (rowblock.h's
// sum_blocks).  No float atomics: reruns at the same grid are bit-identical.
// Native range: fp32 rows, d <= 128; STEP and ASSIGN M <= 64 entries; PREDICT M <= 128 entries and <= 128 leaves.
#include "symtile.h"

namespace {

using namespace symtile;

constexpr int kMaxE = 128;        // entries of a PREDICT table; child slots of a STEP table
constexpr int kMaxStepE = 64;
constexpr int kFoldTiles = 8;     // 512 rows of fp32 accumulation between folds into the fp64 slab
constexpr double kBadQ = 0x1p120; // |x~|^2 from here on (or NaN): a bad row
// LDS in front of the tile: thresholds [kMaxE], the tile rows' weights and |x~|^2 [kRows] each and the waves' final
// sums [8] in fp64, then shift [kMaxD] fp32, the targets [2][kMaxE] int, the tile rows' slots [kRows] int and fp32
// weights [kRows]
constexpr size_t kHeadBytes = (size_t)(kMaxE + 2 * kRows + 8) * 8 + kMaxD * 4 + 2 * kMaxE * 4 + 2 * kRows * 4;
// per block of the workspace behind the slabs: cost, bad count, 2 pads, then W, cnt and Q [kMaxE] each (STEP only)
constexpr int kTail = 4;

enum { kStep = 0, kAssign = 1, kPredict = 2 };

struct BsShape {
  int d, M, L;
  int Td, Tk;  // 32-tiles of d and of the 2 M child slots
  int hld;     // row stride of the hyperplanes in LDS and in the table: 32 Td + 1
  int cosine;
};

__host__ __device__ __forceinline__ int up(int v, int m) { return (v + m - 1) / m * m; }

BsShape make_shape(int d, int M, int L, int cosine) {
  BsShape s{};
  s.d = d;
  s.M = M;
  s.L = L;
  s.Td = up(d, 32) / 32;
  s.Tk = up(2 * M, 32) / 32;
  s.hld = 32 * s.Td + 1;
  s.cosine = cosine;
  return s;
}

// The value is what it was, but the compiler no longer knows where it came from (see mlp.hip).
__device__ __forceinline__ void opaque(int& v) { asm volatile("" : "+v"(v)); }

__host__ __device__ __forceinline__ int64_t block_doubles(int tiles, bool sums) {
  return sums ? (int64_t)tiles * 1024 + kTail + 3 * kMaxE : kTail;
}

// x . y over the thread's 32 columns of a row, in fp64; the row's four threads then hold the whole sum
__device__ __forceinline__ double dot4(const float* xq, const float* yq, int qq, bool mine) {
  double s = 0.0;
  if (mine) {
#pragma unroll 8
    for (int j = 0; j < 32; ++j) {
      const int c = (j + 8 * qq) & 31;
      s = fma((double)xq[c], (double)yq[c], s);
    }
  }
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  return s;
}

// SLOTS: sum tiles per wave (STEP only, else 0); VW = 4: float4 row loads, VW = 1: scalar loads, any layout.
template <int MODE, int SLOTS, int VW>
__global__ __launch_bounds__(256) void bisect_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const double* __restrict__ w, const float* __restrict__ hyp,
    const double* __restrict__ thr, const int* __restrict__ tgt, const float* __restrict__ shift,
    const float* __restrict__ cen, const BsShape sh, int* __restrict__ node, double* __restrict__ ws,
    int64_t rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* thl = reinterpret_cast<double*>(smem);    // [kMaxE]
  double* wrow = thl + kMaxE;                       // [kRows] this tile's weights
  double* qrow = wrow + kRows;                      // [kRows] and |x~|^2
  double* fin = qrow + kRows;                       // [8] the waves' cost and bad count
  float* shf = reinterpret_cast<float*>(fin + 8);   // [kMaxD]
  int* lft = reinterpret_cast<int*>(shf + kMaxD);   // [kMaxE]
  int* rgt = lft + kMaxE;                           // [kMaxE]
  int* srow = rgt + kMaxE;                          // [kRows] this tile's child slots, -1: the row adds nothing
  float* wf = reinterpret_cast<float*>(srow + kRows);  // [kRows] fl32(w) of the rows that add something, else 0
  float* xb = wf + kRows;
  float* hb = xb + kXF;                             // [M][hld]
  constexpr bool kSums = MODE == kStep;
  constexpr int NS = kSums ? SLOTS : 1;
  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = sh.d, dv = d / VW, M = sh.M, hld = sh.hld;
  const int NT = sh.Td * sh.Tk;

  if (tid < kMaxE) {  // kMaxE == kMaxD; shift arrives zero-padded, the entries' tables do not
    const bool in = tid < M;
    thl[tid] = in ? thr[tid] : (double)INFINITY;
    lft[tid] = in ? tgt[tid] : -1;
    rgt[tid] = in ? tgt[M + tid] : -1;
    shf[tid] = shift[tid];
  }
  for (int i = tid; i < M * hld; i += 256) hb[i] = hyp[i];
  double wacc = 0.0, nacc = 0.0;  // STEP: W and cnt of slot tid (threads 0 .. 127), Q of slot tid - 128 (in wacc)
  double cacc = 0.0;              // cost and bad count of tile row tid >> 2, in its first thread
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
  int ev = 0;
  bool first = true;
  int pending = 0;
  // the row's weight and entry travel with its tile
  const auto side = [&](int64_t t, int i) {
    if (t + (i >> 2) < rb1) {
      if (w != nullptr) wv = w[t + (i >> 2)];
      if (MODE != kPredict) ev = node[t + (i >> 2)];
    }
  };
  TileStream<VW> ts;
  ts.begin(xb, kXF, X, ldx, rb0, rb1, dv, tid, side);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    const bool more = t0 + kRows < rb1;
    int tl = tid;
    opaque(tl);
    const int lane = tl & 63, rr = tl >> 2, qq = tl & 3;
    const int lim = rb1 - t0 < kRows ? (int)(rb1 - t0) : kRows;
    const bool valid = rr < lim;
    const double wr = wv;
    int e = MODE == kPredict ? 0 : ev;
    if ((unsigned)e >= (unsigned)M) e = -1;
    // TileStream's put with the shift: x~ = x - shift (zeros for the cosine), rows past the end stay zero
    __syncthreads();
    ts.xt.store(xb, kLD, tl, dv, [&](int r, int c, float x) { return r < lim ? x - shf[c] : 0.f; });
    ts.fetch(t0, tl, side);

    float* xq = xb + rr * kLD + 32 * qq;
    const bool mine = 32 * qq < d;
    const double q = dot4(xq, xq, qq, mine);
    const bool bad = !(q < kBadQ);
    const double inv = 1.0 / fmax(sqrt(q), 1e-30);

    if (MODE == kPredict) {
      // the walk: wave-uniform, every step the gathered dot product of the rows still on their way
      for (int it = 0; it < M; ++it) {
        const bool act = e >= 0;
        if (!__any(act)) break;
        const int ee = act ? e : 0;
        const double s = dot4(xq, hb + ee * hld + 32 * qq, qq, mine);
        const int nx = s > thl[ee] ? rgt[ee] : lft[ee];
        e = act ? nx : e;
      }
      int leaf = e < 0 ? -1 - e : 0;
      if (bad || leaf >= sh.L) leaf = 0;
      const float* cq = cen + (int64_t)leaf * (32 * sh.Td) + 32 * qq;
      double c = 0.0;
      if (mine) {
#pragma unroll 8
        for (int j = 0; j < 32; ++j) {
          const int col = (j + 8 * qq) & 31;
          const double x = (double)xq[col], y = (double)cq[col];
          c = sh.cosine ? fma(x, y, c) : fma(x - y, x - y, c);
        }
      }
      c += __shfl_xor(c, 1);
      c += __shfl_xor(c, 2);
      if (sh.cosine) c = 1.0 - c * inv;
      if (bad) c = q != q ? q : (double)INFINITY;
      if (valid && qq == 0) {
        cacc += wr * c;
        bacc += bad ? 1.0 : 0.0;
        node[t0 + rr] = leaf;
      }
      continue;
    }

    const int ee = e < 0 ? 0 : e;
    const bool right = e >= 0 && !bad && dot4(xq, hb + ee * hld + 32 * qq, qq, mine) > thl[ee];
    if (valid && qq == 0) bacc += bad ? 1.0 : 0.0;
    if (MODE == kAssign) {
      if (valid && qq == 0 && e >= 0) node[t0 + rr] = right ? rgt[e] : lft[e];
      continue;
    }

    // STEP: the tile row becomes x^ (cosine) or zeros (a bad row: 0 * NaN in the MFMA otherwise)
    {
      const bool live = valid && !bad && e >= 0;
      if (mine && (bad || sh.cosine)) {
#pragma unroll 8
        for (int j = 0; j < 32; ++j) xq[j] = bad ? 0.f : (float)((double)xq[j] * inv);
      }
      if (qq == 0) {
        srow[rr] = live ? 2 * e + (right ? 1 : 0) : -1;
        wf[rr] = live ? (float)wr : 0.f;
        wrow[rr] = wr;
        qrow[rr] = sh.cosine ? q * inv * inv : q;
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
        const int slot = 32 * tj + gcol;
        const float* b = xb + goff * kLD + 32 * ti + gcol;
        const int* sr = srow + goff;
        const float* wp = wf + goff;
#pragma unroll 4
        for (int r = 0; r < kRows; r += 2) {
          const float a = sr[r] == slot ? wp[r] : 0.f;
          acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[r * kLD], acc[s], 0, 0, 0);
        }
      }
      // W and cnt of slot j in threads 0 .. 127, Q in threads 128 .. 255
      const int j = tl & (kMaxE - 1);
      if (j < 2 * M) {
        if (tl < kMaxE) {
#pragma unroll 8
          for (int r = 0; r < kRows; ++r) {
            const bool hit = srow[r] == j;
            wacc += hit ? wrow[r] : 0.0;
            nacc += hit ? 1.0 : 0.0;
          }
        } else {
#pragma unroll 8
          for (int r = 0; r < kRows; ++r) wacc += srow[r] == j ? wrow[r] * qrow[r] : 0.0;
        }
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
        for (int e2 = 0; e2 < 16; ++e2) {
          const int i = fi + acc_row(e2, 0) * 32;
          const double v = (double)acc[s][e2];
          slab[i] = first ? v : slab[i] + v;
          acc[s][e2] = 0.f;
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
  if (kSums) {
    if (tid < kMaxE) {
      tail[kTail + tid] = wacc;
      tail[kTail + kMaxE + tid] = nacc;
    } else {
      tail[kTail + kMaxE + tid] = wacc;  // Q: the third table
    }
  }
}

// One block of 256 threads per 16 output values, summed over the blocks; the value goes to its place in out: STEP
// [2 M d sums, 2 M W, 2 M cnt, 2 M Q, cost, bad count], ASSIGN and PREDICT [cost, bad count].
__global__ __launch_bounds__(256) void bisect_reduce_kernel(const double* __restrict__ ws, int nblk, const BsShape sh,
                                                            int sums, double* __restrict__ out) {
  __shared__ double red[16][16];
  const int NT = sh.Td * sh.Tk, S2 = 2 * sh.M;
  const int64_t stride = block_doubles(NT, sums != 0);
  const int64_t idx = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = idx < stride;
  const double t = sum_blocks(red, nblk, ok, [&](int b) { return ws[(int64_t)b * stride + idx]; });
  if (threadIdx.x >= 16 || !ok) return;
  const int64_t slabs = sums ? (int64_t)NT * 1024 : 0;
  const int64_t base = sums ? (int64_t)S2 * (sh.d + 3) : 0;
  if (idx < slabs) {
    const int tile = (int)(idx >> 10), e = (int)(idx & 1023);
    const int tj = tile / sh.Td, ti = tile - tj * sh.Td;
    const int j = 32 * tj + (e >> 5), i = 32 * ti + (e & 31);
    if (j < S2 && i < sh.d) out[(int64_t)j * sh.d + i] = t;
  } else {
    const int r = (int)(idx - slabs);  // 0 cost, 1 bad count, 2 and 3 pads, then W, cnt, Q
    if (r < 2) out[base + r] = t;
    if (r >= kTail) {
      const int v = (r - kTail) / kMaxE, j = (r - kTail) % kMaxE;
      if (j < S2) out[(int64_t)S2 * sh.d + (int64_t)v * S2 + j] = t;
    }
  }
}

struct BsPlan : RowSplit {
  bool native;
  int slots;  // sum tiles per wave of the STEP instantiation
  int bpc;    // blocks per CU of the one round
  size_t lds;
};

size_t lds_bytes(int M, int hld) { return kHeadBytes + (size_t)(kXF + M * hld) * 4; }

bool mode_ok(int mode) { return mode == kStep || mode == kAssign || mode == kPredict; }

// One round of resident blocks on the 256 CUs.  Per CU the 160 KB of LDS hold 4 blocks up to 13 entries at d = 128,
// 2 at 64 entries and 1 for a PREDICT table of more than 91.  Registers (VGPRs + AGPRs per lane, no scratch): on float4
// rows ASSIGN 80, PREDICT 96 and STEP 118 / 152 / 214 at 1 / 2 / 4 sum tiles per wave, which admit 4, 4, 4, 3 and 2
// blocks; on scalar rows 140, 151 and 167 / 184 / 216, which admit 3, 3, 3, 2 and 2.
BsPlan bs_plan(int64_t n, int d, int M, int L, int mode, bool vec) {
  BsPlan pl{};
  pl.native = mode_ok(mode) && n >= 1 && d >= 1 && d <= kMaxD && M >= 1 &&
              (mode == kPredict ? M <= kMaxE && L >= 1 && L <= kMaxE : M <= kMaxStepE);
  if (!pl.native) return pl;
  const BsShape sh = make_shape(d, M, L, 0);
  const int NT = sh.Td * sh.Tk;
  pl.slots = mode != kStep ? 0 : (NT <= 4 ? 1 : (NT <= 8 ? 2 : 4));
  pl.lds = lds_bytes(M, sh.hld);
  pl.bpc = (int)((size_t)160 * 1024 / pl.lds);
  const int by_regs = pl.slots <= 1 ? (vec ? 4 : 3) : (pl.slots == 2 && vec ? 3 : 2);
  if (pl.bpc > by_regs) pl.bpc = by_regs;
  static_cast<RowSplit&>(pl) = split_rows(n, (int64_t)pl.bpc * 256);
  return pl;
}

struct BsArgs {
  const float* X;
  int64_t n, ldx;
  const double* w;
  const float* hyp;
  const double* thr;
  const int* tgt;
  const float* shift;
  const float* cen;
  int* node;
  double* ws;
};

template <int MODE, int SLOTS, int VW>
int launch(const BsPlan& pl, const BsShape& sh, const BsArgs& a, hipStream_t st) {
  if (pl.lds > 64 * 1024) {
    static bool raised[64] = {};
    const int rc = cdna::raise_lds(reinterpret_cast<const void*>(bisect_kernel<MODE, SLOTS, VW>), raised,
                                   lds_bytes(kMaxE, kLD));
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL((bisect_kernel<MODE, SLOTS, VW>), dim3(pl.nblk), dim3(256), pl.lds, st, a.X, a.n, a.ldx, a.w,
                     a.hyp, a.thr, a.tgt, a.shift, a.cen, sh, a.node, a.ws, pl.rows_per_block);
  return (int)hipGetLastError();
}

template <int VW>
int launch_mode(int mode, const BsPlan& pl, const BsShape& sh, const BsArgs& a, hipStream_t st) {
  if (mode == kAssign) return launch<kAssign, 0, VW>(pl, sh, a, st);
  if (mode == kPredict) return launch<kPredict, 0, VW>(pl, sh, a, st);
  switch (pl.slots) {
    case 1: return launch<kStep, 1, VW>(pl, sh, a, st);
    case 2: return launch<kStep, 2, VW>(pl, sh, a, st);
    default: return launch<kStep, 4, VW>(pl, sh, a, st);
  }
}

}  // namespace

static_assert(kMaxE == kMaxD && kMaxE == 2 * kMaxStepE, "one guard loads the tables; the child slots fill a table");
static_assert(kHeadBytes % 16 == 0, "the tile starts 16-byte aligned");
static_assert(kHeadBytes + (size_t)(kXF + kMaxStepE * kLD) * 4 <= 80 * 1024, "two blocks per CU at 64 entries");
static_assert(kHeadBytes + (size_t)(kXF + kMaxE * kLD) * 4 <= 160 * 1024, "a PREDICT table of 128 entries fits");

// What cdna_bisect_step runs for these operands (nothing is launched): out = [native, sum tiles per wave of a STEP,
// load width (4: float4 rows, 1: scalar), blocks, rows per block, sum tiles, LDS bytes, hyperplane table row length,
// leaf-centre table row length, rows between folds, blocks per CU, workspace doubles of this mode].
CDNA_API int cdna_bisect_plan(const float* X, int64_t n, int64_t ldx, int d, int M, int L, int mode, int64_t* out) {
  const BsPlan pl = bs_plan(n, d, M, L, mode, float4_rows(X, d, ldx));
  for (int i = 0; i < 12; ++i) out[i] = 0;
  if (!pl.native || ldx < d) return 0;
  const BsShape sh = make_shape(d, M, L, 0);
  out[0] = 1;
  out[1] = pl.slots;
  out[2] = float4_rows(X, d, ldx) ? 4 : 1;
  out[3] = pl.nblk;
  out[4] = pl.rows_per_block;
  out[5] = mode == kStep ? sh.Td * sh.Tk : 0;
  out[6] = (int64_t)pl.lds;
  out[7] = sh.hld;
  out[8] = 32 * sh.Td;
  out[9] = kFoldTiles * kRows;
  out[10] = pl.bpc;
  out[11] = (int64_t)pl.nblk * block_doubles(sh.Td * sh.Tk, mode == kStep);
  return 0;
}

// hyp: fp32 [M][out[7] of cdna_bisect_plan], zeros from d on; thr [M] f64; tgt [2][M] int32, the left targets and then
// the right ones (PREDICT: a target >= 0 is greater than its entry's index, a leaf is < L; the caller checks); shift
// [128] fp32, zeros from d on (all zeros for the cosine); cen (PREDICT): fp32 [L][out[8]] leaf centres c~ (cosine:
// c^), zeros from d on; w [n] f64 or null (every weight 1); ws: out[11] of the plan doubles.
// STEP: node [n] int32 is read; out [2 M (d + 3) + 2] f64: per child slot 2 e + side the sum of w x~ [d], then the sums
// of w, the row counts and the sums of w |x~|^2 [2 M] each, then 0 and the count of bad rows.
// ASSIGN: node is rewritten; out [2]: 0, bad rows.  PREDICT: node receives the leaves; out [2]: cost, bad rows.
CDNA_API int cdna_bisect_step(const float* X, int64_t n, int64_t ldx, const double* w, const float* hyp,
                              const double* thr, const int* tgt, const float* shift, const float* cen, int d, int M,
                              int L, int cosine, int mode, int* node, double* out, double* ws, hipStream_t st) {
  const bool vec = float4_rows(X, d, ldx);
  const BsPlan pl = bs_plan(n, d, M, L, mode, vec);
  if (!pl.native || ldx < d || X == nullptr || hyp == nullptr || thr == nullptr || tgt == nullptr ||
      shift == nullptr || node == nullptr || out == nullptr || ws == nullptr || (mode == kPredict && cen == nullptr))
    return (int)hipErrorInvalidValue;
  const BsShape sh = make_shape(d, M, L, cosine != 0);
  const BsArgs a{X, n, ldx, w, hyp, thr, tgt, shift, cen, node, ws};
  const int rc = vec ? launch_mode<4>(mode, pl, sh, a, st) : launch_mode<1>(mode, pl, sh, a, st);
  if (rc != 0) return rc;
  const int64_t total = block_doubles(sh.Td * sh.Tk, mode == kStep);
  hipLaunchKernelGGL(bisect_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, ws, pl.nblk, sh,
                     mode == kStep ? 1 : 0, out);
  return (int)hipGetLastError();
}
