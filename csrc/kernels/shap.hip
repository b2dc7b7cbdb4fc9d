// K21 per-row outputs of a forest's root-to-leaf paths: exact path-dependent TreeSHAP feature contributions
// (Lundberg et al. 2018, Algorithm 2, evaluated per leaf path instead of by recursion) and the leaf a row reaches
// in every tree.  Split decisions are the predictors' (trees.hip): raw numeric left iff x <= thr as fp32 (NaN goes
// right), raw categorical left iff the mask bit of (int)x is set (out of [0, 256) and NaN go right); binned numeric
// left iff bin <= node bin, binned set splits the mask bit of the bin.
#include "common.h"

namespace {

// The X tile [rows][d] of row-major fp32 rows r0.. staged as sx[r * (d + 1) + f] (predict_kernel's staging).
template <int THREADS>
__device__ __forceinline__ void stage_x_tile(float* __restrict__ sx, const float* __restrict__ X, int64_t r0,
                                             int rows, int d, int64_t ldx) {
  const int dp = d + 1;
  if (ldx == d && (d % 4) == 0) {
    const float4* src = reinterpret_cast<const float4*>(X + r0 * ldx);
    const int nv = rows * d / 4;
    for (int i = threadIdx.x; i < nv; i += THREADS) {
      const float4 v = src[i];
      const int e = i * 4, r = e / d, f = e - r * d;  // d % 4 == 0: a float4 never crosses a row
      float* dst = sx + r * dp + f;
      dst[0] = v.x;
      dst[1] = v.y;
      dst[2] = v.z;
      dst[3] = v.w;
    }
  } else {
    for (int e = threadIdx.x; e < rows * d; e += THREADS) {
      const int r = e / d, f = e - r * d;
      sx[r * dp + f] = X[(r0 + r) * ldx + f];
    }
  }
}

__device__ __forceinline__ bool raw_left(const float* __restrict__ xr, int fcode, int payload,
                                         const uint32_t* __restrict__ masks) {
  if (fcode >= 0) return xr[fcode] <= __int_as_float(payload);
  const float xc = xr[-fcode - 2];
  const int c = (int)xc;  // xc > -1 && xc < 256  <=>  c in [0, 256), and false for NaN ((int)NaN is 0)
  return (xc > -1.f && xc < 256.f) ? ((masks[payload * 8 + (c >> 5)] >> (c & 31)) & 1u) : false;
}

// How a row's feature value is fetched and tested.  A step is {feature code, payload, path goes left, slot}:
// code >= 0 numeric (payload: fp32 threshold bits / bin), code <= -2 categorical feature -(code + 2) (payload:
// offset of its uint32[8] mask).
struct RawPolicy {
  const float* X;
  int64_t ldx;
  bool staged;  // the X tile fits in LDS next to the phi tile; else the rows are read in place
  __host__ __device__ size_t tile_bytes(int d) const { return staged ? (size_t)64 * (d + 1) * 4 : 0; }
  __device__ __forceinline__ void stage(float* sx, int64_t r0, int rows, int d) const {
    if (staged) stage_x_tile<64>(sx, X, r0, rows, d, ldx);
  }
  __device__ __forceinline__ bool left(const float* sx, int d, int64_t, int64_t r0, int row, int4 st,
                                       const uint32_t* __restrict__ masks) const {
    return raw_left(staged ? sx + row * (d + 1) : X + (r0 + row) * ldx, st.x, st.y, masks);
  }
};

struct BinnedPolicy {
  const uint8_t* b8;  // [G][n] u64 words: feature f of row r is byte ((f >> 3) * n + r) * 8 + (f & 7)
  __host__ __device__ size_t tile_bytes(int) const { return 0; }
  __device__ __forceinline__ void stage(float*, int64_t, int, int) const {}
  __device__ __forceinline__ bool left(const float*, int, int64_t n, int64_t r0, int row, int4 st,
                                       const uint32_t* __restrict__ masks) const {
    const int f = st.x >= 0 ? st.x : -st.x - 2;
    const int bin = b8[((int64_t)(f >> 3) * n + r0 + row) * 8 + (f & 7)];
    if (st.x >= 0) return bin <= st.y;
    return (masks[st.y * 8 + (bin >> 5)] >> (bin & 31)) & 1u;
  }
};

// Column d of phi, and the optional fp64 raw prediction of every row: base + the tree_w * leaf value of the leaf it
// reaches in every tree, added in path order (the same decisions as the contributions, summed independently of them).
struct ShapTail {
  double bias;
  double base;
  double* margin;  // [n] or null
};

constexpr int kPhiStride = 65;  // doubles per feature column of a phi tile: the transposed read-out is conflict-free
constexpr int kInv = 40;        // inv[i] = 1 / i for i < kInv (MAXU + 2 <= 34 used)

// One path's contributions of one row (lane): phi[slot feature] += unwound sum * (o - z) * v, slot by slot.
// ``ob`` bit k = o_k; z / rz / feat: the path's m slots (wave-uniform); ph = the lane's column of the phi tile.
// Every product is rounded before it is added, in one fixed order, and the coefficients are the same doubles in
// both forms below ((j + 1) * (1 / (l + 1)) etc.), so the two agree bit for bit with each other and with the host
// path (K.tree_shap).
//
// Fixed form, m = M known at compile time: both loops fully unrolled, pw[] in registers, every coefficient a
// constant and no guards.
template <int M>
__device__ __forceinline__ void shap_path_fixed(uint32_t ob, const double* __restrict__ z,
                                                const double* __restrict__ rz, const int* __restrict__ feat,
                                                double v, double* ph) {
#pragma clang fp contract(off)
  double pw[M + 1];
#pragma unroll
  for (int j = 1; j <= M; ++j) pw[j] = 0.0;
  pw[0] = 1.0;
#pragma unroll
  for (int k = 0; k < M; ++k) {  // extend by slot k
    const int l = k + 1;
    const double zk = z[k];
    const double o = ((ob >> k) & 1u) ? 1.0 : 0.0;
    const double rl = 1.0 / (double)(l + 1);
#pragma unroll
    for (int j = l - 1; j >= 0; --j) {
      const double a = (o * pw[j]) * ((double)(j + 1) * rl);
      pw[j + 1] = pw[j + 1] + a;
      pw[j] = (zk * pw[j]) * ((double)(l - j) * rl);
    }
  }
  const double mp1 = (double)(M + 1);
  const double rm1 = 1.0 / (double)(M + 1);
#pragma unroll
  for (int k = 0; k < M; ++k) {  // unwound sum of slot k
    const double zk = z[k];
    double nxt = pw[M], tot1 = 0.0, tot0 = 0.0;
#pragma unroll
    for (int j = M - 1; j >= 0; --j) {
      const double tmp = nxt * (mp1 * (1.0 / (double)(j + 1)));
      tot1 = tot1 + tmp;
      nxt = pw[j] - (tmp * zk) * ((double)(M - j) * rm1);
      tot0 = tot0 + pw[j] * (mp1 * (1.0 / (double)(M - j)));
    }
    tot0 = tot0 * rz[k];
    const bool on = (ob >> k) & 1u;
    const double c = ((on ? tot1 : tot0) * ((on ? 1.0 : 0.0) - zk)) * v;
    double* q = ph + feat[k] * kPhiStride;
    *q = *q + c;
  }
}

// General form, m <= MAXU known at run time (wave-uniform): the j loops are unrolled over MAXU under uniform
// guards so that pw[] still has compile-time indices; inv[i] = 1 / i from LDS.
template <int MAXU>
__device__ __forceinline__ void shap_path_any(int m, uint32_t ob, const double* __restrict__ z,
                                              const double* __restrict__ rz, const int* __restrict__ feat,
                                              double v, const double* inv, double* ph) {
#pragma clang fp contract(off)
  double pw[MAXU + 1];
#pragma unroll
  for (int j = 0; j <= MAXU; ++j) pw[j] = 0.0;
  pw[0] = 1.0;
  for (int k = 0; k < m; ++k) {  // extend by slot k
    const int l = k + 1;
    const double zk = z[k];
    const double o = ((ob >> k) & 1u) ? 1.0 : 0.0;
    const double rl = inv[l + 1];
#pragma unroll
    for (int j = MAXU - 1; j >= 0; --j) {
      if (j < l) {
        const double a = (o * pw[j]) * ((double)(j + 1) * rl);
        pw[j + 1] = pw[j + 1] + a;
        pw[j] = (zk * pw[j]) * ((double)(l - j) * rl);
      }
    }
  }
  double pwm = 0.0;
#pragma unroll
  for (int j = 1; j <= MAXU; ++j)
    if (j == m) pwm = pw[j];
  const double mp1 = (double)(m + 1);
  const double rm1 = inv[m + 1];
  for (int k = 0; k < m; ++k) {  // unwound sum of slot k
    const double zk = z[k];
    double nxt = pwm, tot1 = 0.0, tot0 = 0.0;
#pragma unroll
    for (int j = MAXU - 1; j >= 0; --j) {
      if (j < m) {
        const double tmp = nxt * (mp1 * inv[j + 1]);
        tot1 = tot1 + tmp;
        nxt = pw[j] - (tmp * zk) * ((double)(m - j) * rm1);
        tot0 = tot0 + pw[j] * (mp1 * inv[m - j]);
      }
    }
    tot0 = tot0 * rz[k];
    const bool on = (ob >> k) & 1u;
    const double c = ((on ? tot1 : tot0) * ((on ? 1.0 : 0.0) - zk)) * v;
    double* q = ph + feat[k] * kPhiStride;
    *q = *q + c;
  }
}

// Paths of up to kFixedSlots slots (every forest of depth <= 8) take the fixed form.
constexpr int kFixedSlots = 8;
template <int MAXU>
__device__ __forceinline__ void shap_path(int m, uint32_t ob, const double* __restrict__ z,
                                          const double* __restrict__ rz, const int* __restrict__ feat, double v,
                                          const double* inv, double* ph) {
  switch (m) {  // wave-uniform
    case 1: shap_path_fixed<1>(ob, z, rz, feat, v, ph); break;
    case 2: shap_path_fixed<2>(ob, z, rz, feat, v, ph); break;
    case 3: shap_path_fixed<3>(ob, z, rz, feat, v, ph); break;
    case 4: shap_path_fixed<4>(ob, z, rz, feat, v, ph); break;
    case 5: shap_path_fixed<5>(ob, z, rz, feat, v, ph); break;
    case 6: shap_path_fixed<6>(ob, z, rz, feat, v, ph); break;
    case 7: shap_path_fixed<7>(ob, z, rz, feat, v, ph); break;
    case 8: shap_path_fixed<8>(ob, z, rz, feat, v, ph); break;
    default:
      if (MAXU > kFixedSlots) shap_path_any<MAXU>(m, ob, z, rz, feat, v, inv, ph);
  }
}

// One wave = one block = a 64-row tile (lane = row), looping over every path of the forest.  Per path p:
//   hdr[p]   = {first step, steps, first slot, m slots}
//   steps[s] = {feature code, payload, direction, slot}   o_slot = AND over its steps of (left == direction)
//   slot_feat / slot_z / slot_rz (= 1 / z): the merged features of the path; pv[p] = tree_w * leaf value
// All of these are read with wave-uniform indices; only the o bits differ by lane (shap_path).  The sums of a row
// are made by its lane in (path, slot) order, products rounded before they are added (no contraction): the result
// does not depend on n, the grid or the tile.  PHI_LDS: the tile's phi[d][65] accumulates in LDS, else in the block's own
// global tile phi_g[blockIdx.x]; either way the tile is written out once as whole rows, column d = tail.bias.
template <class Policy, int MAXU, bool PHI_LDS>
__global__ __launch_bounds__(64) void tree_shap_kernel(Policy pol, int64_t n, int d, const int4* __restrict__ hdr,
                                                       int P, const int4* __restrict__ steps,
                                                       const int* __restrict__ slot_feat,
                                                       const double* __restrict__ slot_z,
                                                       const double* __restrict__ slot_rz,
                                                       const double* __restrict__ pv,
                                                       const uint32_t* __restrict__ masks, ShapTail tail,
                                                       double* __restrict__ phi_g, double* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double shap_smem[];
  double* inv = shap_smem;
  double* sphi = shap_smem + kInv;
  float* sx = reinterpret_cast<float*>(sphi + (PHI_LDS ? (size_t)d * kPhiStride : 0));
  const int lane = threadIdx.x;
  if (lane < kInv) inv[lane] = lane ? 1.0 / (double)lane : 0.0;
  double* phi = PHI_LDS ? sphi : phi_g + (size_t)blockIdx.x * d * kPhiStride;
  const int dp1 = d + 1;
  for (int64_t r0 = (int64_t)blockIdx.x * 64; r0 < n; r0 += (int64_t)gridDim.x * 64) {
    const int rows = (int)((n - r0) < 64 ? (n - r0) : 64);
    __syncthreads();
    pol.stage(sx, r0, rows, d);
    for (int j = 0; j < d; ++j) phi[j * kPhiStride + lane] = 0.0;
    __syncthreads();
    const int row = lane < rows ? lane : rows - 1;  // tail lanes repeat the last row (never written out)
    double macc = tail.base;
    for (int p = 0; p < P; ++p) {
      const int4 h = hdr[p];
      const int m = h.w;
      uint32_t ob = 0xFFFFFFFFu;
      for (int s = h.x; s < h.x + h.y; ++s) {
        const int4 st = steps[s];
        const bool left = pol.left(sx, d, n, r0, row, st, masks);
        if (left != (st.z != 0)) ob &= ~(1u << st.w);
      }
      const double v = pv[p];
      // the row reaches this path's leaf iff it agrees with every slot (m = 0: a single-leaf tree, always)
      const uint32_t all = m >= 32 ? 0xFFFFFFFFu : (1u << m) - 1u;
      if ((ob & all) == all) macc = macc + v;
      if (m == 0) continue;  // bias and margin only
      shap_path<MAXU>(m, ob, slot_z + h.z, slot_rz + h.z, slot_feat + h.z, v, inv, phi + lane);
    }
    __syncthreads();
    double* o_t = out + r0 * dp1;
    for (int e = lane; e < rows * dp1; e += 64) {
      const int r = e / dp1, j = e - r * dp1;
      o_t[e] = j < d ? phi[j * kPhiStride + r] : tail.bias;
    }
    if (tail.margin != nullptr && lane < rows) tail.margin[r0 + lane] = macc;
  }
}

// Leaf reached by every row in every tree: predict_kernel's int4 node table, X tile staging and decisions; block =
// 64 rows x 4 tree lanes (lane q walks trees q, q + 4, ...); out[r][t] = global id of the reached node.
__global__ __launch_bounds__(256) void tree_leaf_index_kernel(const float* __restrict__ X, int64_t n, int d,
                                                              int64_t ldx, bool staged,
                                                              const int4* __restrict__ nodes,
                                                              const int* __restrict__ roots, int T,
                                                              const uint32_t* __restrict__ masks,
                                                              int* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float leaf_sx[];
  const int tl = threadIdx.x >> 6, row = threadIdx.x & 63;
  for (int64_t r0 = (int64_t)blockIdx.x * 64; r0 < n; r0 += (int64_t)gridDim.x * 64) {
    const int rows = (int)((n - r0) < 64 ? (n - r0) : 64);
    __syncthreads();
    if (staged) stage_x_tile<256>(leaf_sx, X, r0, rows, d, ldx);
    __syncthreads();
    if (row < rows) {
      const float* xr = staged ? leaf_sx + row * (d + 1) : X + (r0 + row) * ldx;
      for (int t = tl; t < T; t += 4) {
        int id = roots[t];
        int4 nv = nodes[id];
        while (nv.x != -1) {
          id = raw_left(xr, nv.x, nv.y, masks) ? nv.z : nv.w;
          nv = nodes[id];
        }
        out[(r0 + row) * T + t] = id;
      }
    }
  }
}

template <class Policy, int MAXU, bool PHI_LDS>
int launch_shap(Policy pol, int64_t n, int d, const int4* hdr, int P, const int4* steps, const int* slot_feat,
                const double* slot_z, const double* slot_rz, const double* pv, const uint32_t* masks, ShapTail tail,
                double* phi_g, int grid, double* out, hipStream_t st) {
  const size_t lds = (size_t)kInv * 8 + (PHI_LDS ? (size_t)d * kPhiStride * 8 : 0) + pol.tile_bytes(d);
  if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
  auto kern = tree_shap_kernel<Policy, MAXU, PHI_LDS>;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64), lds, st, pol, n, d, hdr, P, steps, slot_feat, slot_z, slot_rz, pv,
                     masks, tail, phi_g, out);
  return (int)hipGetLastError();
}

template <class Policy>
int dispatch_shap(Policy pol, int maxu, bool phi_lds, int64_t n, int d, const int4* hdr, int P, const int4* steps,
                  const int* slot_feat, const double* slot_z, const double* slot_rz, const double* pv,
                  const uint32_t* masks, ShapTail tail, double* phi_g, int grid, double* out, hipStream_t st) {
#define CDNA_SHAP_GO(U)                                                                                         \
  return phi_lds ? launch_shap<Policy, U, true>(pol, n, d, hdr, P, steps, slot_feat, slot_z, slot_rz, pv, masks, \
                                                tail, phi_g, grid, out, st)                                     \
                 : launch_shap<Policy, U, false>(pol, n, d, hdr, P, steps, slot_feat, slot_z, slot_rz, pv,      \
                                                 masks, tail, phi_g, grid, out, st)
  if (maxu <= 8) CDNA_SHAP_GO(8);
  if (maxu <= 16) CDNA_SHAP_GO(16);
  CDNA_SHAP_GO(32);
#undef CDNA_SHAP_GO
}

}  // namespace

// LDS bytes of one tree_shap block with the phi tile, and the X tile of the raw policy, in LDS: the host keeps the
// phi tile in LDS while this fits kShapLdsBudget.
constexpr int64_t kShapLdsBudget = 160 * 1024;
CDNA_API int64_t cdna_tree_shap_lds_bytes(int d, int binned) {
  return (int64_t)kInv * 8 + (int64_t)d * kPhiStride * 8 + (binned ? 0 : (int64_t)64 * (d + 1) * 4);
}
CDNA_API int64_t cdna_tree_shap_lds_budget() { return kShapLdsBudget; }

// phi out[n][d + 1] fp64 (column d = bias); margin (optional) [n] fp64: base + the pv of the reached leaves.
// src: fp32 X[n][ldx] (binned = 0) or the uint8 bins as [G][n] u64 words (binned = 1).  max_slots: the forest's largest slot count (<= 32).  phi_lds = 0: the tiles accumulate in
// phi_g, [grid][d][65] doubles owned block by block.  grid: blocks (each loops over 64-row tiles).
CDNA_API int cdna_tree_shap(const void* src, int binned, int64_t n, int d, int64_t ldx, const int4* hdr, int P,
                            const int4* steps, const int* slot_feat, const double* slot_z, const double* slot_rz,
                            const double* pv, const uint32_t* masks, double bias, int max_slots, int phi_lds,
                            double* phi_g, int grid, double* out, double base, double* margin, hipStream_t st) {
  const ShapTail tail{bias, base, margin};
  if (n <= 0) return 0;
  if (max_slots > 32 || d < 1 || grid < 1 || (!phi_lds && phi_g == nullptr)) return (int)hipErrorInvalidValue;
  if (binned) {
    BinnedPolicy pol{reinterpret_cast<const uint8_t*>(src)};
    return dispatch_shap(pol, max_slots, phi_lds != 0, n, d, hdr, P, steps, slot_feat, slot_z, slot_rz, pv, masks,
                         tail, phi_g, grid, out, st);
  }
  // the X tile is staged while it fits next to the phi tile (any d: beyond that the rows are read in place)
  const int64_t phi_bytes = (int64_t)kInv * 8 + (phi_lds ? (int64_t)d * kPhiStride * 8 : 0);
  RawPolicy pol{reinterpret_cast<const float*>(src), ldx, phi_bytes + (int64_t)64 * (d + 1) * 4 <= kShapLdsBudget};
  return dispatch_shap(pol, max_slots, phi_lds != 0, n, d, hdr, P, steps, slot_feat, slot_z, slot_rz, pv, masks,
                       tail, phi_g, grid, out, st);
}

// out[n][T] int32: the global node id of the leaf row r reaches in tree t (nodes / roots / masks as
// cdna_tree_predict).
CDNA_API int cdna_tree_leaf_index(const float* X, int64_t n, int d, int64_t ldx, const int4* nodes, const int* roots,
                                  int T, const uint32_t* masks, int* out, hipStream_t st) {
  if (n <= 0 || T <= 0) return 0;
  if (d < 1) return (int)hipErrorInvalidValue;
  const bool staged = (size_t)64 * (d + 1) * 4 <= 64 * 1024;  // wider rows are read in place
  const size_t lds = staged ? (size_t)64 * (d + 1) * 4 : 0;
  int64_t g = (n + 63) / 64;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(tree_leaf_index_kernel, dim3((unsigned)g), dim3(256), lds, st, X, n, d, ldx, staged, nodes,
                     roots, T, masks, out);
  return (int)hipGetLastError();
}
