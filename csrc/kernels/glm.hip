// K22 glm_step — one fused IRLS pass of a generalized linear model on MFMA.
//
// Per row (all fp64):  eta = offset + b + x·beta,  mu = g⁻¹(eta) (clamped as Spark's families project it),
// gp = g'(mu),  W = w / (V(mu) gp²),  z = eta − offset + (y − mu) gp.  The row then contributes
// √W · [x − shift | 1 | z − zshift], rounded to fp32, to the augmented (d+2)×(d+2) Gram — the layout K1
// (gram.hip) returns: ΣW x̃x̃ᵀ, ΣW x̃, ΣW, ΣW x̃ z̃, ΣW z̃, ΣW z̃² — through v_mfma_f32_32x32x2_f32 (exact
// fp32; IRLS weights span orders of magnitude, so no bf16 here).  X is read ONCE per IRLS iteration: the
// unfused form (GEMV for eta, elementwise passes, a √W-scaled copy of X, K1 on the copy) reads it three times
// and writes it once.  Reference behaviour: pyspark.ml.regression.GeneralizedLinearRegression (IRLS solver).
//
// Structure: 256 threads, 64-row tiles, row-major fp32 LDS tile with a padded row stride (LD ≡ 4 mod 32).
//  * the next tile's rows are loaded into registers before the work on the current tile and land in the other
//    LDS buffer after its MFMAs;
//  * row phase: 4 threads per row form the fp64 dot product over the raw fp32 row in LDS (lane-pair butterfly,
//    so the 4 lanes hold the same bits), evaluate link and variance, and scale the row in place;
//  * MFMA phase: lane l's operand for tile column block I at k-step k0 is tile[k0 + (l>>5)][32I + (l&31)] —
//    consecutive floats of one row, no transposition.  Wave w owns tile pairs w, w+4, w+8 and writes its
//    accumulators straight to the block's fp32 partial slab.
// The slabs and the per-block fp64 scalars are reduced in a fixed order in fp64 (glm_reduce_kernel): no float
// atomics on global memory, two runs on the same input return the same bits.
//
// mode INIT: eta = g(mu0) from the label (the family's R / Spark starting value) instead of beta.
// mode EVAL: only the scalars (deviance Σ w d(y, mu), Σw, Σwy, count of non-finite rows); no Gram.
// Rows whose mu, W or z is not finite are counted and left out of the Gram and of the sums: their tile row is
// zeroed, so an inf / NaN feature that made eta non-finite does not reach G.  (INIT does not form eta from the
// features; a non-finite feature goes into G as it is there, and the next step counts the row.)
// Native range: d + 2 <= 128.
#include "symtile.h"

namespace {

using namespace symtile;

constexpr double kEps = 1e-16;
// kRows, kMaxD: rowblock.h's 64-row tile and its 128 columns; d + 2 <= kMaxD

enum { kGaussian = 0, kBinomial = 1, kPoisson = 2, kGamma = 3, kTweedie = 4 };
enum { kIdentity = 0, kLog = 1, kInverse = 2, kLogit = 3, kProbit = 4, kCloglog = 5, kSqrt = 6, kPower = 7 };
enum { kStep = 0, kInit = 1, kEval = 2 };

struct GlmSpec {
  int family, link;
  double vp, lp;
};

__device__ __forceinline__ double glm_link(const GlmSpec& s, double mu) {
  switch (s.link) {
    case kIdentity: return mu;
    case kLog: return log(mu);
    case kInverse: return 1.0 / mu;
    case kLogit: return log(mu / (1.0 - mu));
    case kProbit: return normcdfinv(mu);
    case kCloglog: return log(-log(1.0 - mu));
    case kSqrt: return sqrt(mu);
    default: return pow(mu, s.lp);
  }
}

__device__ __forceinline__ double glm_unlink(const GlmSpec& s, double eta) {
  switch (s.link) {
    case kIdentity: return eta;
    case kLog: return exp(eta);
    case kInverse: return 1.0 / eta;
    case kLogit: return 1.0 / (1.0 + exp(-eta));
    case kProbit: return normcdf(eta);
    case kCloglog: return 1.0 - exp(-exp(eta));
    case kSqrt: return eta * eta;
    default: return pow(eta, 1.0 / s.lp);
  }
}

// g'(mu)
__device__ __forceinline__ double glm_dlink(const GlmSpec& s, double mu) {
  switch (s.link) {
    case kIdentity: return 1.0;
    case kLog: return 1.0 / mu;
    case kInverse: return -1.0 / (mu * mu);
    case kLogit: return 1.0 / (mu * (1.0 - mu));
    case kProbit: {
      const double q = normcdfinv(mu);
      return 2.5066282746310002 * exp(0.5 * q * q);  // sqrt(2 pi) / exp(-q²/2)
    }
    case kCloglog: return 1.0 / ((mu - 1.0) * log(1.0 - mu));
    case kSqrt: return 0.5 / sqrt(mu);
    default: return s.lp * pow(mu, s.lp - 1.0);
  }
}

__device__ __forceinline__ double glm_clamp(const GlmSpec& s, double mu) {
  if (s.family == kBinomial) return mu < kEps ? kEps : (mu > 1.0 - kEps ? 1.0 - kEps : mu);
  if (s.family == kGaussian) return mu;
  return mu < kEps ? kEps : mu;
}

__device__ __forceinline__ double glm_variance(const GlmSpec& s, double mu) {
  switch (s.family) {
    case kGaussian: return 1.0;
    case kBinomial: return mu * (1.0 - mu);
    case kPoisson: return mu;
    case kGamma: return mu * mu;
    default: return pow(mu, s.vp);
  }
}

__device__ __forceinline__ double ylogy(double y, double mu) { return y == 0.0 ? 0.0 : y * log(y / mu); }

__device__ __forceinline__ double tw_yp(double y, double mu, double p) {
  return p == 0.0 ? log(y / mu) : (pow(y, p) - pow(mu, p)) / p;
}

// unit deviance d(y, mu) (the row's weight multiplies it)
__device__ __forceinline__ double glm_unit_dev(const GlmSpec& s, double y, double mu) {
  switch (s.family) {
    case kGaussian: return (y - mu) * (y - mu);
    case kBinomial: return 2.0 * (ylogy(y, mu) + ylogy(1.0 - y, 1.0 - mu));
    case kPoisson: return 2.0 * (ylogy(y, mu) - (y - mu));
    case kGamma: return -2.0 * (log(y / mu) - (y - mu) / mu);
    default: {
      const double y1 = (s.vp >= 1.0 && s.vp < 2.0) ? (y > 0.1 ? y : 0.1) : y;
      return 2.0 * (y * tw_yp(y1, mu, 1.0 - s.vp) - tw_yp(y, mu, 2.0 - s.vp));
    }
  }
}

// the family's starting mean from the label
__device__ __forceinline__ double glm_init_mu(const GlmSpec& s, double y, double w) {
  if (s.family == kBinomial) return (w * y + 0.5) / (w + 1.0);
  if (s.family == kPoisson || s.family == kTweedie) return y > 0.1 ? y : 0.1;
  return y;
}

// One row's IRLS terms.  Kept out of line: inlined, the fp64 link / variance / deviance bodies of every family
// (pow, normcdfinv, ...) pushed the streaming kernel past its register budget and into scratch.
struct RowTerms {
  double W, z, dev, fin;  // fin: 1.0 when mu, W and z are all finite
};

__device__ __noinline__ RowTerms glm_row(GlmSpec sp, int mode, double y, double w, double off, double lin) {
  double eta, mu;
  if (mode == kInit) {
    mu = glm_clamp(sp, glm_init_mu(sp, y, w));
    eta = glm_link(sp, mu);
  } else {
    eta = off + lin;
    mu = glm_clamp(sp, glm_unlink(sp, eta));
  }
  const double gp = glm_dlink(sp, mu);
  RowTerms r;
  r.W = w / (glm_variance(sp, mu) * gp * gp);
  r.z = eta - off + (y - mu) * gp;
  r.fin = (cdna::finite_d(mu) && cdna::finite_d(r.W) && cdna::finite_d(r.z)) ? 1.0 : 0.0;
  r.dev = r.fin != 0.0 ? glm_unit_dev(sp, y, mu) : 0.0;
  return r;
}

// VW = 4: float4 row loads (d % 4 == 0, ldx % 4 == 0, 16-byte aligned X); VW = 1: scalar loads, any layout.
// Two blocks per CU (LDS: 69 KB each at d + 2 > 96) for the float4 variant; the scalar variant's 32 loads in flight
// per thread need more than 256 registers, so it is left at one wave per SIMD.
template <int PW, int VW>
__global__ __launch_bounds__(256, VW == 4 ? 2 : 1) void glm_step_kernel(
    const float* __restrict__ X, int64_t n, int d, int64_t ldx, const double* __restrict__ y,
    const double* __restrict__ w, const double* __restrict__ off, const double* __restrict__ beta, double b0,
    const float* __restrict__ shift, float zshift, GlmSpec sp, int mode, int T, int npairs, int LD,
    float* __restrict__ partial, double* __restrict__ spart, int64_t rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int kNI = 32 / VW;  // items per thread: 64 rows x (d / VW) <= 64 * 126 / VW over 256 threads
  typedef float vec_t __attribute__((ext_vector_type(VW)));
  float* buf = reinterpret_cast<float*>(smem);                                  // [2][kRows][LD]
  const int tsz = kRows * LD;
  double* beta_s = reinterpret_cast<double*>(smem + (size_t)2 * tsz * 4);       // [kMaxD]
  float* shift_s = reinterpret_cast<float*>(beta_s + kMaxD);                    // [kMaxD]
  double* red = reinterpret_cast<double*>(shift_s + kMaxD);                     // [4][4]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, half = lane >> 5, col = lane & 31;
  const int dv = d / VW;               // row length in load items
  const int items = kRows * dv;

  // zero both tiles once: columns d + 2 .. LD - 1 are never written again
  for (int i = tid; i < 2 * tsz; i += 256) buf[i] = 0.f;
  for (int i = tid; i < kMaxD; i += 256) {
    beta_s[i] = (i < d && beta != nullptr) ? beta[i] : 0.0;
    shift_s[i] = (i < d && shift != nullptr) ? shift[i] : 0.f;
  }
  const WavePairs<PW> wp(wid, T, npairs);
  f32x16 acc[PW];
#pragma unroll
  for (int j = 0; j < PW; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  int64_t rb0, rb1;
  block_rows(rows_per_block, n, rb0, rb1);
  const int rr = tid >> 2, q = tid & 3;  // row phase: 4 threads per row
  vec_t v[kNI];
  double yv = 0.0, wv = 0.0, ov = 0.0;
  double s_dev = 0.0, s_w = 0.0, s_wy = 0.0, s_bad = 0.0;

// Next tile's rows -> registers (rows past rb1 become zeros with weight 0), then registers -> LDS.  Kept here as
// macros: written through symtile::RowTile (as K23 does) the float4 kernels take 200 / 217 / 249 VGPRs for 196 /
// 216 / 234 and EVAL measured 0.3 % slower (profiles/r11/symtile.md).
#define GLM_LOAD(T0)                                                                   \
  {                                                                                    \
    const int64_t lim_ = rb1 - (T0);                                                   \
    _Pragma("unroll") for (int i = 0; i < kNI; ++i) {                                  \
      const int e_ = tid + 256 * i;                                                    \
      const int r_ = e_ / dv, c_ = e_ - r_ * dv;                                       \
      vec_t t_ = {};                                                                   \
      if (e_ < items && r_ < lim_)                                                     \
        t_ = *reinterpret_cast<const vec_t*>(X + ((T0) + r_) * ldx + (int64_t)c_ * VW); \
      v[i] = t_;                                                                       \
    }                                                                                  \
    const bool ok_ = rr < lim_;                                                        \
    yv = ok_ ? y[(T0) + rr] : 0.0;                                                     \
    wv = ok_ ? (w != nullptr ? w[(T0) + rr] : 1.0) : 0.0;                              \
    ov = (ok_ && off != nullptr) ? off[(T0) + rr] : 0.0;                               \
  }
#define GLM_STORE(TB)                                                                  \
  {                                                                                    \
    _Pragma("unroll") for (int i = 0; i < kNI; ++i) {                                  \
      const int e_ = tid + 256 * i;                                                    \
      const int r_ = e_ / dv, c_ = e_ - r_ * dv;                                       \
      if (e_ < items) *reinterpret_cast<vec_t*>((TB) + r_ * LD + c_ * VW) = v[i];      \
    }                                                                                  \
  }

  __syncthreads();  // zeroed tiles, beta and shift are in LDS
  int cur = 0;
  if (rb0 < rb1) {
    GLM_LOAD(rb0);
    GLM_STORE(buf);
  }
  for (int64_t t0 = rb0; t0 < rb1; t0 += kRows) {
    const bool more = t0 + kRows < rb1;
    // this tile's row scalars (loaded with the tile); the prefetch below overwrites them
    const double ry = yv, rw = wv, ro = ov;
    const bool valid = t0 + rr < rb1;
    if (more) GLM_LOAD(t0 + kRows);
    __syncthreads();  // raw tile `cur` complete; every wave is past the MFMAs on the other buffer
    float* row = buf + cur * tsz + rr * LD;
    double lin = 0.0;
    if (mode != kInit) {
#pragma unroll 8  // independent LDS reads in flight: one read per trip left the phase latency-bound
      for (int c = q; c < d; c += 4) lin = fma((double)row[c], beta_s[c], lin);
      lin += __shfl_xor(lin, 1);
      lin += __shfl_xor(lin, 2);
    }
    const RowTerms rt = glm_row(sp, mode, ry, rw, ro, b0 + lin);
    const bool fin = rt.fin != 0.0;
    const double W = (valid && fin) ? rt.W : 0.0, z = (valid && fin) ? rt.z : 0.0;
    if (q == 0 && valid) {
      if (fin) {
        s_dev += rw * rt.dev;
        s_w += rw;
        s_wy += rw * ry;
      } else {
        s_bad += 1.0;
      }
    }
    if (mode != kEval) {
      const double sw = sqrt(W);
      const float swf = (float)sw;
      const bool keep = valid && fin;  // a left-out row is zeroed, not scaled by 0: an inf / NaN feature stays out of G
#pragma unroll 8
      for (int c = q; c < d; c += 4) row[c] = keep ? (row[c] - shift_s[c]) * swf : 0.f;
      if (q == 0) {
        row[d] = swf;
        row[d + 1] = (float)(sw * (z - (double)zshift));
      }
      __syncthreads();  // scaled tile complete
      mfma_rows<kRows>(wp, buf + cur * tsz + half * LD + col, LD, acc);
    }
    if (more) GLM_STORE(buf + (cur ^ 1) * tsz);
    cur ^= 1;
  }
#undef GLM_LOAD
#undef GLM_STORE

  if (mode != kEval) {
#pragma unroll
    for (int j = 0; j < PW; ++j)
      if (wp.own[j]) store_slab(partial + ((int64_t)blockIdx.x * npairs + wid + 4 * j) * 1024, acc[j], half, col);
  }
  // the block's scalars: wave butterflies, then the 4 waves in order
  s_dev = cdna::wave_sum(s_dev);
  s_w = cdna::wave_sum(s_w);
  s_wy = cdna::wave_sum(s_wy);
  s_bad = cdna::wave_sum(s_bad);
  if (lane == 0) {
    red[wid * 4 + 0] = s_dev;
    red[wid * 4 + 1] = s_w;
    red[wid * 4 + 2] = s_wy;
    red[wid * 4 + 3] = s_bad;
  }
  __syncthreads();
  if (tid < 4) spart[(int64_t)blockIdx.x * 4 + tid] = ((red[tid] + red[4 + tid]) + red[8 + tid]) + red[12 + tid];
}

// Blocks 0 .. gridDim.x - 2: partial [nblk][npairs][1024] -> G (symmetric fill), symtile::reduce_slabs.  Last block:
// the scalars, spart [nblk][4] -> stats[4]; both in the fixed order of rowblock.h's sum_blocks.
__global__ __launch_bounds__(256) void glm_reduce_kernel(const float* __restrict__ partial, int nblk, int npairs,
                                                         int T, int D, double* __restrict__ G,
                                                         const double* __restrict__ spart,
                                                         double* __restrict__ stats) {
  __shared__ double red[16][16];
  if (blockIdx.x == gridDim.x - 1) {
    const int el = threadIdx.x & 15;  // < 4: a scalar
    const double t = sum_blocks(red, nblk, el < 4, [&](int b) { return spart[(int64_t)b * 4 + el]; });
    if (threadIdx.x < 4) stats[el] = t;
    return;
  }
  reduce_slabs(red, partial, npairs, nblk, npairs, [T](int p, int& I, int& J) { pair_ij(p, T, I, J); }, D, G,
               [](int, int) { return false; });
}

struct GlmPlan {
  int T, npairs, nblk, LD;
  int64_t rows_per_block;
  size_t lds;
};

GlmPlan glm_plan(int64_t n, int d) {
  GlmPlan pl{};
  pl.T = (d + 2 + 31) / 32;
  pl.npairs = pl.T * (pl.T + 1) / 2;
  int64_t nb = (n + 2047) / 2048;
  if (nb > 512) nb = 512;  // 2 resident blocks x 256 CUs
  if (nb < 1) nb = 1;
  pl.nblk = (int)nb;
  const int64_t rpb = (n + nb - 1) / nb;
  pl.rows_per_block = (rpb + kRows - 1) / kRows * kRows;
  pl.LD = pl.T * 32 + 4;  // ≡ 4 mod 32: the row phase's 8 rows x 4 lanes hit 32 different banks
  pl.lds = (size_t)2 * kRows * pl.LD * 4 + (size_t)kMaxD * 8 + (size_t)kMaxD * 4 + 16 * 8;
  return pl;
}

template <int PW, int VW>
int glm_launch(const GlmPlan& pl, const float* X, int64_t n, int d, int64_t ldx, const double* y, const double* w,
               const double* off, const double* beta, double b0, const float* shift, float zshift, GlmSpec sp,
               int mode, float* ws, double* sws, hipStream_t st) {
  // the dynamic LDS passes the 64 KB default at d + 2 > 96: raised to the widest plan's size, once per
  // instantiation and device
  static bool raised[64] = {};
  const int rc = cdna::raise_lds(reinterpret_cast<const void*>(glm_step_kernel<PW, VW>), raised,
                                 glm_plan(1, kMaxD - 2).lds);
  if (rc != 0) return rc;
  hipLaunchKernelGGL((glm_step_kernel<PW, VW>), dim3(pl.nblk), dim3(256), pl.lds, st, X, n, d, ldx, y, w, off, beta,
                     b0, shift, zshift, sp, mode, pl.T, pl.npairs, pl.LD, ws, sws, pl.rows_per_block);
  return (int)hipGetLastError();
}

template <int VW>
int glm_launch_pw(const GlmPlan& pl, const float* X, int64_t n, int d, int64_t ldx, const double* y,
                  const double* w, const double* off, const double* beta, double b0, const float* shift,
                  float zshift, GlmSpec sp, int mode, float* ws, double* sws, hipStream_t st) {
  switch ((pl.npairs + 3) / 4) {
    case 1: return glm_launch<1, VW>(pl, X, n, d, ldx, y, w, off, beta, b0, shift, zshift, sp, mode, ws, sws, st);
    case 2: return glm_launch<2, VW>(pl, X, n, d, ldx, y, w, off, beta, b0, shift, zshift, sp, mode, ws, sws, st);
    default: return glm_launch<3, VW>(pl, X, n, d, ldx, y, w, off, beta, b0, shift, zshift, sp, mode, ws, sws, st);
  }
}

}  // namespace

// Blocks of the launch: the scalar workspace holds 4 doubles per block.
CDNA_API int cdna_glm_step_blocks(int64_t n) { return glm_plan(n, 1).nblk; }

// Workspace (in floats) of the per-block Gram slabs.
CDNA_API int64_t cdna_glm_step_workspace(int64_t n, int d) {
  const GlmPlan pl = glm_plan(n, d);
  return (int64_t)pl.nblk * pl.npairs * 1024;
}

// G: (d+2)×(d+2) f64 row-major (untouched in EVAL mode); stats: [deviance, Σw, Σwy, non-finite rows] f64.
// w, off, beta and shift may be null (unit weights, no offset, zeros).
CDNA_API int cdna_glm_step(const float* X, int64_t n, int d, int64_t ldx, const double* y, const double* w,
                           const double* off, const double* beta, double b0, const float* shift, float zshift,
                           int family, int link, double var_power, double link_power, int mode, double* G,
                           double* stats, float* ws, double* sws, hipStream_t st) {
  if (n < 1 || d < 1 || d + 2 > kMaxD || ldx < d) return (int)hipErrorInvalidValue;
  if (family < kGaussian || family > kTweedie || link < kIdentity || link > kPower || mode < kStep || mode > kEval)
    return (int)hipErrorInvalidValue;
  const GlmPlan pl = glm_plan(n, d);
  const GlmSpec sp{family, link, var_power, link_power};
  const bool vec = float4_rows(X, d, ldx);
  const int rc = vec ? glm_launch_pw<4>(pl, X, n, d, ldx, y, w, off, beta, b0, shift, zshift, sp, mode, ws, sws, st)
                     : glm_launch_pw<1>(pl, X, n, d, ldx, y, w, off, beta, b0, shift, zshift, sp, mode, ws, sws, st);
  if (rc != 0) return rc;
  // EVAL has no Gram: only the scalars' block
  const int64_t tot = mode != kEval ? (int64_t)pl.npairs * 1024 : 0;
  hipLaunchKernelGGL(glm_reduce_kernel, dim3((unsigned)((tot + 15) / 16) + 1), dim3(256), 0, st, ws, pl.nblk,
                     pl.npairs, pl.T, d + 2, G, sws, stats);
  return (int)hipGetLastError();
}
