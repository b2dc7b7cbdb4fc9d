// K24 mlp_step — loss and gradient (or the predictions) of a multilayer perceptron in one pass over the rows, on the
// fp32 MFMA.
//
// The net (Spark's MultilayerPerceptronClassifier): affine layers l = 0 .. L-1 of widths w[l] -> w[l+1], sigmoid
// after every layer but the last, softmax with cross-entropy on top.  Per row: a_0 = x, z_l = W_l a_l + b_l,
// a_{l+1} = sigmoid(z_l) (l < L-1), loss = logsumexp(z_{L-1}) - z_{L-1}[label], delta_{L-1} = softmax - onehot,
// delta_{l-1} = (W_lᵀ delta_l) a_l (1 - a_l), dW_l = sum_rows delta_l a_lᵀ, db_l = sum_rows delta_l.
//
// mlp_step_kernel: 256 threads, 64-row tiles, the next tile of X prefetched in registers (rowblock.h's scaffolding:
// the row split, the tile and its pipeline).  Buffer l of LDS holds the tile's a_l, row-major fp32 with the odd row
// stride kLD; the logits take buffer L.  Every matmul is
// v_mfma_f32_32x32x2_f32:
//   forward / backward (layer_mm): wave w forms the 32-row block (w & 1) of Y = S M for the column blocks (w >> 1) and
//     (w >> 1) + 2; lane l's A operand at k-step m is S[32 rb + (l & 31)][m + (l >> 5)] (odd stride: 32 rows hit 32
//     banks), its B operand consecutive floats of a zero-padded fp32 copy of the weights (L2-resident) the host
//     prepares in both orientations: W_lᵀ [in][out] for the forward, W_l [out][in] for the backward delta, which is
//     written over a_l in place once the weight gradient that reads a_l is done;
//   top: 4 threads per row form logsumexp, the loss term and softmax - onehot in fp64 (max-subtracted), the delta
//     rounded to fp32 over the logits; rows past the end get delta 0, so they add exactly nothing below;
//   weight gradient: dW_l is tiled 32x32, the tiles of all layers dealt round-robin to the 4 waves (SLOTS per wave);
//     a tile sums delta_l[r][32 to + i] a_l[r][32 ti + j] over the 64 rows, both operands consecutive floats of one
//     LDS row (symtile.h's mfma_rows pattern with two different buffers).  fp32 accumulators in registers for
//     kFoldTiles tiles, then folded into the block's fp64 slab (each element owned by one lane: plain load, add,
//     store).  db_l: column sums of the delta buffer, fp32 over 32 rows, fp64 across tiles.
// mlp_reduce_kernel: slabs, bias sums and loss partials of the blocks in a fixed order in fp64 (sum_blocks), scattered
// into Spark's flat layout (W_l column-major [out][in], then b_l).  No float atomics on global memory: reruns are
// bit-identical.
// SLOTS = 0 is PREDICT: the forward half and the top, writing raw, prob and pred.
// Native range: every width <= 128, 1 <= L <= 3 affine layers, 2 <= classes.
#include "symtile.h"

namespace {

using namespace symtile;

constexpr int kMaxW = kMaxD;
constexpr int kMaxL = 3;
// every buffer is a tile of rowblock.h: its row stride kLD is odd (the A operand's 32 rows hit 32 banks) and a
// constant, so that the epilogues' and the gradient's LDS addresses are one register plus an immediate
constexpr int kBuf = kXF;  // floats per buffer
constexpr int kFoldTiles = 8;  // 512 rows of fp32 accumulation between folds into the fp64 slab

enum { kStep = 0, kPredict = 1 };

struct MlpNet {
  int L;
  int w[kMaxL + 1];      // widths
  // offsets in the table (floats): W_lᵀ [in up to 2][out up to 32], W_l [out up to 2][in up to 32], b_l [out up to 32]
  int wt[kMaxL], wb[kMaxL], bs[kMaxL];
  int tile0[kMaxL + 1];  // first gradient tile of layer l; tile0[L] = all tiles
  int goff[kMaxL];       // layer l's offset in the flat parameter vector
  int lds_floats, table_floats, P;
};

__host__ __device__ __forceinline__ int up(int v, int m) { return (v + m - 1) / m * m; }

MlpNet make_net(const int* layers, int nl) {
  MlpNet net{};
  net.L = nl - 1;
  int lds = 0, tab = 0, tiles = 0, p = 0;
  for (int l = 0; l < nl; ++l) {
    net.w[l] = layers[l];
    lds += kBuf;
  }
  for (int l = 0; l + 1 < nl; ++l) {
    const int in = layers[l], out = layers[l + 1];
    net.wt[l] = tab;
    tab += up(in, 2) * up(out, 32);
    net.wb[l] = tab;
    tab += up(out, 2) * up(in, 32);
    net.bs[l] = tab;
    tab += up(out, 32);
    net.tile0[l] = tiles;
    tiles += (up(out, 32) / 32) * (up(in, 32) / 32);
    net.goff[l] = p;
    p += out * in + out;
  }
  net.tile0[net.L] = tiles;
  for (int l = net.L + 1; l <= kMaxL; ++l) net.tile0[l] = tiles;
  net.lds_floats = lds;
  net.table_floats = tab;
  net.P = p;
  return net;
}

// a field of the net by a runtime layer index, without indexing the kernel argument dynamically
template <int N>
__device__ __forceinline__ int pick(const int (&a)[N], int l) {
  int v = a[0];
#pragma unroll
  for (int q = 1; q < N; ++q)
    if (l == q) v = a[q];
  return v;
}

// The value is what it was, but the compiler no longer knows where it came from: the addresses computed from it are
// formed where they are used, not hoisted out of the tile loop and held in registers across it.
__device__ __forceinline__ void opaque(int& v) { asm volatile("" : "+v"(v)); }

// sigmoid in fp32 from exp(-|z|): no overflow for large |z|
__device__ __forceinline__ float sigmoidf(float z) {
  const float e = expf(-fabsf(z));
  const float r = 1.f / (1.f + e);
  return z >= 0.f ? r : e * r;
}

// Y [64][32 Tc] = S [64][kd] M [kd][ldw]: S in LDS (row stride kLD), M consecutive floats in memory.  epi(r, c, v,
// cv): element (r, c) of Y with colv[c] (0 without colv).  8 k-steps' operand loads (LDS, and M through L2) are in
// flight: one wave per SIMD hides none.  (Loading a group ahead of the MFMAs that use it measured no faster.)
template <class Epi>
__device__ __forceinline__ void layer_mm(const float* src, int kd, const float* __restrict__ M, int ldw,
                                         int Tc, const float* __restrict__ colv, int wid, int lane, Epi epi) {
  opaque(lane);
  const int half = lane >> 5, col = lane & 31;
  const int rb = wid & 1, cb0 = wid >> 1, cb1 = cb0 + 2;
  const bool own0 = cb0 < Tc, own1 = cb1 < Tc;
  if (!own0) return;
  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc0[e] = acc1[e] = 0.f;
  const float* ap = src + (32 * rb + col) * kLD + half;
  const float* bp = M + half * ldw + col;
  if (own1) {
#pragma unroll 8
    for (int m = 0; m < kd; m += 2) {
      const float a = ap[m];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[m * ldw + 32 * cb0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[m * ldw + 32 * cb1], acc1, 0, 0, 0);
    }
  } else {
#pragma unroll 8
    for (int m = 0; m < kd; m += 2)
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[m], bp[m * ldw + 32 * cb0], acc0, 0, 0, 0);
  }
  const float c0 = colv != nullptr ? colv[32 * cb0 + col] : 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) epi(32 * rb + acc_row(e, half), 32 * cb0 + col, acc0[e], c0);
  if (own1) {
    const float c1 = colv != nullptr ? colv[32 * cb1 + col] : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) epi(32 * rb + acc_row(e, half), 32 * cb1 + col, acc1[e], c1);
  }
}

// Per block of the workspace: [tiles][1024] gradient slabs, [kMaxL][kMaxW] bias sums, the loss sum (+ 1 pad).
__host__ __device__ __forceinline__ int64_t block_doubles(int tiles) {
  return (int64_t)tiles * 1024 + kMaxL * kMaxW + 2;
}

// SLOTS: gradient tiles per wave (0: PREDICT); VW = 4: float4 row loads, VW = 1: scalar loads, any layout.
template <int SLOTS, int VW>
__global__ __launch_bounds__(256) void mlp_step_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const int* __restrict__ y, const float* __restrict__ tab,
    const MlpNet net, double* __restrict__ ws, double* __restrict__ raw, double* __restrict__ prob,
    int* __restrict__ pred, int64_t rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* buf = reinterpret_cast<float*>(smem);
  // [2][kMaxL][kMaxW] bias sums, [kRows] loss sums
  double* red = reinterpret_cast<double*>(smem + (size_t)net.lds_floats * 4);
  constexpr bool kTrain = SLOTS > 0;
  constexpr int NS = kTrain ? SLOTS : 1;
  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: what follows from it stays in SGPRs
  const int d = net.w[0], dv = d / VW;
  const int L = net.L;
  const int C = pick(net.w, L);
  const int NT = net.tile0[kMaxL];

  // this wave's gradient tiles are wid, wid + 4, ..: tile wid + 4 s accumulates in acc[s]
  f32x16 acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[s][e] = 0.f;

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  // top: 4 threads per row, row tid >> 2; bias sums: column tid & 127 of the row half tid >> 7
  double* myws = ws != nullptr ? ws + (int64_t)blockIdx.x * block_doubles(NT) : nullptr;
  int yv = 0;
  // the block's running fp64 sums live in LDS, each entry touched by one thread until the end: db_l[column] per row
  // half, the loss per tile row
  double* lsum = red + 2 * kMaxL * kMaxW;  // [kRows]
  if (kTrain) {
#pragma unroll
    for (int l = 0; l < kMaxL; ++l) red[((tid >> 7) * kMaxL + l) * kMaxW + (tid & (kMaxW - 1))] = 0.0;
    if ((tid & 3) == 0) lsum[tid >> 2] = 0.0;
  }
  bool first = true;
  int pending = 0;

  // the row's label travels with its tile
  const auto side = [&](int64_t t, int i) {
    if (kTrain && t + (i >> 2) < rb1) yv = y[t + (i >> 2)];
  };
  TileStream<VW> ts;
  // every buffer is zeroed: column d of buffer 0 is read when d is odd
  ts.begin(buf, net.lds_floats, X, ldx, rb0, rb1, dv, tid, side);
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    const bool more = t0 + kRows < rb1;
    int tl = tid;  // this tile's copy of the thread index (see opaque), and what the phases derive from it
    opaque(tl);
    const int lane = tl & 63, rr = tl >> 2, qq = tl & 3, bc = tl & (kMaxW - 1), bh = tl >> 7;
    const bool valid = t0 + rr < rb1;
    const int lab = yv;
    ts.put(buf, tl);
    ts.fetch(t0, tl, side);

    // forward
#pragma unroll
    for (int l = 0; l < kMaxL; ++l) {
      if (l >= L) break;
      const bool last = l == L - 1;
      float* dst = buf + (l + 1) * kBuf;
      const int outp = up(net.w[l + 1], 32);
      layer_mm(buf + l * kBuf, up(net.w[l], 2), tab + net.wt[l], outp, outp >> 5, tab + net.bs[l], wid,
               lane, [&](int r, int c, float v, float b) {
                 v += b;
                 dst[r * kLD + c] = last ? v : sigmoidf(v);
               });
      __syncthreads();
    }

    // top: logsumexp, loss and softmax - onehot in fp64
    {
      float* zl = buf + L * kBuf + rr * kLD;
      float zm = -__builtin_inff();
      int bj = C;  // no class yet
      for (int c = qq; c < C; c += 4) {
        const float z = zl[c];
        if (z > zm || c == qq) {  // the lowest index among equals
          zm = z;
          bj = c;
        }
      }
#pragma unroll
      for (int o = 1; o <= 2; o <<= 1) {
        const float oz = __shfl_xor(zm, o);
        const int oj = __shfl_xor(bj, o);
        if (oj < C && (bj >= C || oz > zm || (oz == zm && oj < bj))) {
          zm = oz;
          bj = oj;
        }
      }
      const double mx = (double)zm;
      double se = 0.0;
      for (int c = qq; c < C; c += 4) se += exp((double)zl[c] - mx);
      se += __shfl_xor(se, 1);
      se += __shfl_xor(se, 2);
      const double lse = mx + log(se);
      if (kTrain) {
        const bool inr = lab >= 0 && lab < C;
        const double zlab = inr ? (double)zl[lab] : 0.0;
        if (valid && qq == 0) lsum[rr] += lse - zlab;
        for (int c = qq; c < C; c += 4) {
          const double p = exp((double)zl[c] - lse);
          zl[c] = valid ? (float)(p - (c == lab ? 1.0 : 0.0)) : 0.f;
        }
      } else if (valid) {
        const int64_t row = t0 + rr;
        for (int c = qq; c < C; c += 4) {
          const double z = (double)zl[c];
          raw[row * C + c] = z;
          prob[row * C + c] = exp(z - lse);
        }
        if (qq == 0) pred[row] = bj;
      }
    }
    if (!kTrain) continue;
    __syncthreads();  // delta of the last layer complete

    // backward
#pragma unroll
    for (int l = kMaxL - 1; l >= 0; --l) {
      if (l >= L) continue;
      // dW_l += delta_lᵀ a_l over the tile's rows
      int gl = lane;
      opaque(gl);
      const float* gp = buf + (gl >> 5) * kLD + (gl & 31);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        // tile t of layer l's [out tiles][in tiles] grid, if it is one: scalar arithmetic, nothing held across tiles
        const int t = wid + 4 * s - net.tile0[l];
        if (t < 0 || t >= net.tile0[l + 1] - net.tile0[l]) continue;
        const int Tin = (net.w[l] + 31) >> 5;                             // 1 .. 4
        const int to = Tin == 3 ? (t * 11) >> 5 : t >> (Tin >> 1);        // t / Tin for t < 16
        const float* a = gp + (l + 1) * kBuf + 32 * to;
        const float* b = gp + l * kBuf + 32 * (t - to * Tin);
#pragma unroll 4
        for (int k = 0; k < kRows; k += 2)
          acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k * kLD], b[k * kLD], acc[s], 0, 0, 0);
      }
      // db_l += column sums of delta_l
      {
        const float* dl = buf + (l + 1) * kBuf + (32 * bh) * kLD + bc;
        if (bc < net.w[l + 1]) {
          float s = 0.f;
#pragma unroll 8
          for (int r = 0; r < 32; ++r) s += dl[r * kLD];
          red[(bh * kMaxL + l) * kMaxW + bc] += (double)s;
        }
      }
      if (l > 0) {
        __syncthreads();  // the gradient's reads of a_l are done: delta_{l-1} goes over it
        float* dst = buf + l * kBuf;
        const int inp = up(net.w[l], 32);
        layer_mm(buf + (l + 1) * kBuf, up(net.w[l + 1], 2), tab + net.wb[l], inp, inp >> 5, nullptr,
                 wid, lane, [&](int r, int c, float v, float) {
                   const float a = dst[r * kLD + c];
                   dst[r * kLD + c] = v * (a * (1.f - a));
                 });
        __syncthreads();
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

  if (!kTrain) return;
  __syncthreads();
  double* tail = myws + (int64_t)NT * 1024;
  for (int i = tid; i < kMaxL * kMaxW; i += 256) tail[i] = red[i] + red[kMaxL * kMaxW + i];
  if (tid < 32) {  // the 64 rows' loss sums in a fixed order
    double t = lsum[tid] + lsum[tid + 32];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (tid == 0) tail[kMaxL * kMaxW] = t;
  }
}

// One block of 256 threads per 16 values of a block's workspace, summed over the blocks; the value goes to its place
// in out [P + 1]: the flat gradient, then the loss.
__global__ __launch_bounds__(256) void mlp_reduce_kernel(const double* __restrict__ ws, int nblk, const MlpNet net,
                                                         double* __restrict__ out) {
  __shared__ double red[16][16];
  const int NT = net.tile0[kMaxL];
  const int64_t stride = block_doubles(NT);
  const int64_t total = (int64_t)NT * 1024 + kMaxL * kMaxW + 1;
  const int64_t idx = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const bool ok = idx < total;
  const double t = sum_blocks(red, nblk, ok, [&](int b) { return ws[(int64_t)b * stride + idx]; });
  if (threadIdx.x >= 16 || !ok) return;
  if (idx < (int64_t)NT * 1024) {
    const int tile = (int)(idx >> 10), e = (int)(idx & 1023);
    int l = 0;
#pragma unroll
    for (int q = 1; q < kMaxL; ++q)
      if (tile >= net.tile0[q]) l = q;
    const int in = pick(net.w, l), outw = pick(net.w, l + 1);
    const int Tin = (in + 31) / 32;
    const int loc = tile - pick(net.tile0, l);
    const int to = loc / Tin, ti = loc - to * Tin;
    const int o = 32 * to + (e >> 5), i = 32 * ti + (e & 31);
    if (o < outw && i < in) out[pick(net.goff, l) + o + (int64_t)i * outw] = t;
  } else if (idx < (int64_t)NT * 1024 + kMaxL * kMaxW) {
    const int r = (int)(idx - (int64_t)NT * 1024);
    const int l = r / kMaxW, c = r - l * kMaxW;
    if (l < net.L) {
      const int in = pick(net.w, l), outw = pick(net.w, l + 1);
      if (c < outw) out[pick(net.goff, l) + in * outw + c] = t;
    }
  } else {
    out[net.P] = t;
  }
}

struct MlpPlan : RowSplit {
  bool native;
  int slots;  // gradient tiles per wave of the STEP instantiation
  size_t lds;
};

constexpr int kSlotSteps[] = {1, 3, 6, 12};

MlpPlan mlp_plan(int64_t n, const int* layers, int nl) {
  MlpPlan pl{};
  pl.native = nl >= 2 && nl - 1 <= kMaxL && n >= 1 && layers[nl - 1] >= 2;
  for (int l = 0; l < nl && pl.native; ++l) pl.native = layers[l] >= 1 && layers[l] <= kMaxW;
  if (!pl.native) return pl;
  const MlpNet net = make_net(layers, nl);
  const int per_wave = (net.tile0[net.L] + 3) / 4;
  for (int s : kSlotSteps)
    if (pl.slots == 0 && per_wave <= s) pl.slots = s;
  static_cast<RowSplit&>(pl) = split_rows(n, 1024);
  pl.lds = (size_t)net.lds_floats * 4 + (size_t)(2 * kMaxL * kMaxW + kRows) * 8;
  return pl;
}

size_t max_lds() {
  const int widest[kMaxL + 1] = {kMaxW, kMaxW, kMaxW, kMaxW};
  return mlp_plan(1, widest, kMaxL + 1).lds;
}

template <int SLOTS, int VW>
int step_launch(const MlpPlan& pl, const MlpNet& net, const float* X, int64_t n, int64_t ldx, const int* y,
                const float* tab, double* ws, double* raw, double* prob, int* pred, hipStream_t st) {
  static bool raised[64] = {};
  const int rc = cdna::raise_lds(reinterpret_cast<const void*>(mlp_step_kernel<SLOTS, VW>), raised, max_lds());
  if (rc != 0) return rc;
  hipLaunchKernelGGL((mlp_step_kernel<SLOTS, VW>), dim3(pl.nblk), dim3(256), pl.lds, st, X, n, ldx, y, tab, net, ws,
                     raw, prob, pred, pl.rows_per_block);
  return (int)hipGetLastError();
}

template <int VW>
int step_launch_slots(int slots, const MlpPlan& pl, const MlpNet& net, const float* X, int64_t n, int64_t ldx,
                      const int* y, const float* tab, double* ws, double* raw, double* prob, int* pred,
                      hipStream_t st) {
  switch (slots) {
    case 0: return step_launch<0, VW>(pl, net, X, n, ldx, y, tab, ws, raw, prob, pred, st);
    case 1: return step_launch<1, VW>(pl, net, X, n, ldx, y, tab, ws, raw, prob, pred, st);
    case 3: return step_launch<3, VW>(pl, net, X, n, ldx, y, tab, ws, raw, prob, pred, st);
    case 6: return step_launch<6, VW>(pl, net, X, n, ldx, y, tab, ws, raw, prob, pred, st);
    default: return step_launch<12, VW>(pl, net, X, n, ldx, y, tab, ws, raw, prob, pred, st);
  }
}

}  // namespace

// What cdna_mlp_step runs for these operands (nothing is launched): out = [native, gradient tiles per wave, load
// width (4: float4 rows, 1: scalar), blocks, rows per block, gradient tiles, LDS bytes, table floats].
CDNA_API int cdna_mlp_plan(const float* X, int64_t n, int64_t ldx, const int* layers, int nl, int64_t* out) {
  const MlpPlan pl = mlp_plan(n, layers, nl);
  for (int i = 0; i < 8; ++i) out[i] = 0;
  if (!pl.native || ldx < layers[0]) return 0;
  const MlpNet net = make_net(layers, nl);
  out[0] = 1;
  out[1] = pl.slots;
  out[2] = float4_rows(X, layers[0], ldx) ? 4 : 1;
  out[3] = pl.nblk;
  out[4] = pl.rows_per_block;
  out[5] = net.tile0[net.L];
  out[6] = (int64_t)pl.lds;
  out[7] = net.table_floats;
  return 0;
}

// Offsets (in floats) of the zero-padded fp32 tables of layer l in the table the caller prepares: off[3 l] W_lᵀ
// [in rounded up to 2][out rounded up to 32], off[3 l + 1] W_l [out rounded up to 2][in rounded up to 32],
// off[3 l + 2] b_l [out rounded up to 32].  The table's size is cdna_mlp_plan's out[7].
CDNA_API int cdna_mlp_table_offsets(const int* layers, int nl, int64_t* off) {
  if (!mlp_plan(1, layers, nl).native) return (int)hipErrorInvalidValue;
  const MlpNet net = make_net(layers, nl);
  for (int l = 0; l < net.L; ++l) {
    off[3 * l] = net.wt[l];
    off[3 * l + 1] = net.wb[l];
    off[3 * l + 2] = net.bs[l];
  }
  return 0;
}

// Workspace of a STEP in doubles: per block the gradient slabs, the bias sums and the loss sum.
CDNA_API int64_t cdna_mlp_step_workspace(int64_t n, const int* layers, int nl) {
  const MlpPlan pl = mlp_plan(n, layers, nl);
  if (!pl.native) return 0;
  return (int64_t)pl.nblk * block_doubles(make_net(layers, nl).tile0[nl - 1]);
}

// STEP: y [n] i32 labels, out [P + 1] f64 (the flat gradient sum, then the loss sum), ws: cdna_mlp_step_workspace
// doubles.  PREDICT: raw, prob [n][C] f64, pred [n] i32.  tab: the fp32 table of cdna_mlp_table_offsets.
CDNA_API int cdna_mlp_step(const float* X, int64_t n, int64_t ldx, const int* y, const float* tab, const int* layers,
                           int nl, int mode, double* out, double* ws, double* raw, double* prob, int* pred,
                           hipStream_t st) {
  const MlpPlan pl = mlp_plan(n, layers, nl);
  if (!pl.native || ldx < layers[0] || X == nullptr || tab == nullptr) return (int)hipErrorInvalidValue;
  if (mode != kStep && mode != kPredict) return (int)hipErrorInvalidValue;
  if (mode == kStep && (y == nullptr || out == nullptr || ws == nullptr)) return (int)hipErrorInvalidValue;
  if (mode == kPredict && (raw == nullptr || prob == nullptr || pred == nullptr)) return (int)hipErrorInvalidValue;
  const MlpNet net = make_net(layers, nl);
  const bool vec = float4_rows(X, layers[0], ldx);
  const int slots = mode == kStep ? pl.slots : 0;
  const int rc = vec ? step_launch_slots<4>(slots, pl, net, X, n, ldx, y, tab, ws, raw, prob, pred, st)
                     : step_launch_slots<1>(slots, pl, net, X, n, ldx, y, tab, ws, raw, prob, pred, st);
  if (rc != 0 || mode == kPredict) return rc;
  const int64_t total = (int64_t)net.tile0[net.L] * 1024 + kMaxL * kMaxW + 1;
  hipLaunchKernelGGL(mlp_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, ws, pl.nblk, net, out);
  return (int)hipGetLastError();
}
