// Block scaffolding of the LDS integer level histograms: the node-id kernels of hist4.hip (hist4, hist4f) and the
// row-code kernels of hist5.hip (hist5, hist5p, hist5q).  One block = (8-feature group g, slot group, row chunk);
// it clears its LDS planes, stages its tables, runs the kernel's own row loop and flushes to out[S][d][B][K].
// Written here once: the launch arguments and their host fill, the block decode, the LDS carve-up and clear, the
// feature-mask staging, the rotated-feature constants, the local-node -> slot tables of the row-code kernels, the
// two flushes, the trees-per-group bucket and the launch.  The row loops stay in the kernels: they are what differs.
#pragma once
#include <type_traits>

#include "common.h"

namespace cdna {

constexpr size_t kHistLdsMax = 160 * 1024;  // gfx950: LDS of one CU, the widest plan the host checks admit

struct HistArgs {
  const uint64_t* bins;  // [G][n] 8 bins per word
  int64_t n;
  int d, T;
  const float* v0;
  const float* v1;
  const int* label;
  int C;
  const int* build_slot;  // [A] slot or -1
  const uint32_t* feat_mask;
  int mask_words, S, B, SB, K;
  const int* grp;  // [ngroups][5] = s0, t0, t1, id0, id1
  int ngroups, nchunk;
  int64_t rows_per_chunk;
  float qs0, qs1;           // fixed-point scales (powers of two) for v0, v1
  int n64, n32;             // planes held as 64-bit / 32-bit integers in LDS
  unsigned long long* out;  // [S][d][B][K] int64
};

// mode bit0: classes; bit2: v0 present (moments).  hipErrorInvalidValue when a chunk could overflow a u32 LDS count.
inline int hist_fill(HistArgs& a, int mode, const uint64_t* bins, int64_t n, int d, int T, const float* v0,
                     const float* v1, const int* label, int C, const int* build_slot, const uint32_t* feat_mask,
                     int mask_words, int S, int B, int SB, const int* grp, int ngroups, int nchunk, float qs0,
                     float qs1, unsigned long long* out) {
  const bool classes = (mode & 1) != 0, has_v0 = (mode & 4) != 0;
  a.bins = bins;
  a.n = n;
  a.d = d;
  a.T = T;
  a.v0 = v0;
  a.v1 = v1;
  a.label = label;
  a.C = C;
  a.build_slot = build_slot;
  a.feat_mask = feat_mask;
  a.mask_words = mask_words;
  a.S = S;
  a.B = B;
  a.SB = SB;
  a.K = classes ? C : 2;
  a.grp = grp;
  a.ngroups = ngroups;
  a.nchunk = nchunk;
  a.rows_per_chunk = (n + nchunk - 1) / nchunk;
  a.qs0 = qs0;
  a.qs1 = qs1;
  a.n64 = classes ? 0 : (has_v0 ? 2 : 1);
  a.n32 = classes ? C : (has_v0 ? 0 : 1);
  a.out = out;
  // u32 LDS counts: at most rows_per_chunk * 255 per word
  return a.rows_per_chunk * 255 >= (int64_t)1 << 32 ? (int)hipErrorInvalidValue : 0;
}

// bytes of the LDS planes of a launch (64-bit planes, then the 32-bit planes padded to 4 words)
inline size_t hist_plane_bytes(const HistArgs& a) {
  const size_t plane = (size_t)a.SB * 8 * a.B;
  return plane * 8 * a.n64 + ((plane * a.n32 + 3) & ~(size_t)3) * 4;
}
inline unsigned hist_blocks(const HistArgs& a) { return (unsigned)((a.d + 7) / 8) * a.ngroups * a.nchunk; }

// The trees-per-group bucket NT of the row-code kernels: f(integral_constant<int, NT>) for the smallest bucket that
// holds nt trees.
template <typename F>
auto nt_dispatch(int nt, F&& f) {
  if (nt <= 1) return f(std::integral_constant<int, 1>{});
  if (nt <= 2) return f(std::integral_constant<int, 2>{});
  if (nt <= 4) return f(std::integral_constant<int, 4>{});
  if (nt <= 8) return f(std::integral_constant<int, 8>{});
  return f(std::integral_constant<int, 16>{});
}
inline int nt_bucket(int nt) {
  return nt_dispatch(nt, [](auto b) { return (int)decltype(b)::value; });
}

// Launch of a histogram kernel instantiation.  Blocks above 64 KB of dynamic LDS must opt in: raised once per
// instantiation and device to the widest plan the host admits.
template <auto KERN, typename Args>
int hist_launch(unsigned nblk, int threads, size_t lds, hipStream_t st, const Args& a) {
  if (lds > kHistLdsMax) return (int)hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    static bool raised[64] = {};
    const int rc = raise_lds(reinterpret_cast<const void*>(KERN), raised, kHistLdsMax);
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(KERN, dim3(nblk), dim3(threads), lds, st, a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------------------------

// remapped block id -> (8-feature group, slot-group row of a.grp, row chunk [rb, re))
struct HistBlock {
  int g, fbase;
  int s0, t0, t1, id0, id1;
  int64_t rb, re;
};

__device__ __forceinline__ HistBlock hist_block(const HistArgs& a) {
  HistBlock b;
  const int G = (a.d + 7) / 8;
  const uint32_t w = xcd_remap(blockIdx.x, gridDim.x);
  b.g = (int)(w % G);
  const int grp = (int)((w / G) % a.ngroups);
  const int chunk = (int)(w / ((uint32_t)G * a.ngroups));
  b.s0 = a.grp[grp * 5 + 0];
  b.t0 = a.grp[grp * 5 + 1];
  b.t1 = a.grp[grp * 5 + 2];
  b.id0 = a.grp[grp * 5 + 3];
  b.id1 = a.grp[grp * 5 + 4];
  b.fbase = b.g * 8;
  b.rb = (int64_t)chunk * a.rows_per_chunk;
  b.re = b.rb + a.rows_per_chunk;
  if (b.re > a.n) b.re = a.n;
  return b;
}

// The dynamic LDS of a block: n64 planes of 64-bit words, n32 planes of 32-bit words padded to 4 words, then `rest`
// (the kernel's own buffers and tables).
struct HistLds {
  unsigned long long* h64;
  uint32_t* h32;
  char* rest;
};

__device__ __forceinline__ HistLds hist_lds(char* smem, int n64, int n32, int plane) {
  HistLds l;
  l.h64 = reinterpret_cast<unsigned long long*>(smem);
  l.h32 = reinterpret_cast<uint32_t*>(l.h64 + (size_t)n64 * plane);
  l.rest = reinterpret_cast<char*>(l.h32 + ((n32 * plane + 3) & ~3));
  return l;
}

template <int TH>
__device__ __forceinline__ void hist_clear(const HistLds& l, int n64, int n32, int plane) {
  for (int i = threadIdx.x; i < n64 * plane; i += TH) l.h64[i] = 0ull;
  for (int i = threadIdx.x; i < n32 * plane; i += TH) l.h32[i] = 0u;
}

// features of group fbase that exist (bit j: feature fbase + j < d)
__device__ __forceinline__ uint32_t hist_fvalid(int d, int fbase) {
  const int valid = d - fbase;
  return valid >= 8 ? 0xFFu : ((1u << (valid > 0 ? valid : 0)) - 1u);
}

// lmask[i] = the 8 feature-mask bits of slot s0 + i for this feature group.  NULLABLE: a null feat_mask stages all
// existing features (the node-id kernels); otherwise the caller stages only when it has a mask.  A slot past S stages
// 0 under a mask (the node-id kernels used to stage 0xFF there): no table yields such a slot, so the byte is never read.
template <int TH, bool NULLABLE>
__device__ __forceinline__ void hist_stage_mask(uint8_t* lmask, const HistArgs& a, const HistBlock& b) {
  for (int i = threadIdx.x; i < a.SB; i += TH) {
    const int slot = b.s0 + i;
    uint32_t m = 0u;
    if (NULLABLE && a.feat_mask == nullptr) m = 0xFFu;
    else if (slot < a.S) m = (a.feat_mask[(int64_t)slot * a.mask_words + (b.fbase >> 5)] >> (b.fbase & 31)) & 0xFFu;
    lmask[i] = (uint8_t)(m & hist_fvalid(a.d, b.fbase));
  }
}

__device__ __forceinline__ uint32_t rot8(uint32_t m, int rot) { return ((m >> rot) | (m << (8 - rot))) & 0xFFu; }

// Per-thread constants of the rotated feature order: lane `rot` visits feature (j + rot) & 7 at step j.
struct HistRot {
  int fsel[8];  // which 32-bit half of the bins word
  int fsh[8];   // byte position inside it
  int foff[8];  // feature row inside the slot's [8][B] block
};

__device__ __forceinline__ HistRot hist_rot(int rot, int B) {
  HistRot r;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int jj = (j + rot) & 7;
    r.fsel[j] = jj >> 2;
    r.fsh[j] = (jj & 3) * 8;
    r.foff[j] = jj * B;
  }
  return r;
}
// the group's existing features in the rotated order, and (block-uniform) whether all 8 exist
__device__ __forceinline__ uint32_t hist_frot(const HistArgs& a, int fbase, int rot) {
  return rot8(hist_fvalid(a.d, fbase), rot);
}
__device__ __forceinline__ bool hist_all8(const HistArgs& a, int fbase) { return a.d - fbase >= 8; }

// Per-tree local-node -> slot tables of a row-code block: lt[k][loc] = slot - s0 or -1 (loc 255 = done; trees past
// the group's are all -1).  tfirst[t] = first active id of tree t.
template <int NT, int TH>
__device__ __forceinline__ void hist_local_tables(int16_t* lt, const HistArgs& a, const int* tfirst,
                                                  const HistBlock& b) {
  const int nt = b.t1 - b.t0 + 1;
  for (int i = threadIdx.x; i < NT * 256; i += TH) {
    const int k = i >> 8, loc = i & 255;
    int v = -1;
    const int id = k < nt ? tfirst[b.t0 + k] + loc : 0;
    const int idend = k + 1 < nt ? tfirst[b.t0 + k + 1] : b.id1;
    if (k < nt && loc != 255 && id < idend) {
      const int sl = a.build_slot[id];
      if (sl >= b.s0 && sl < b.s0 + a.SB) v = sl - b.s0;
    }
    lt[i] = (int16_t)v;
  }
}

// cell `rem` of the block's [SB][8][B] plane -> e = the index of its out[slot][f][bin][0]; false outside [S] x [d]
__device__ __forceinline__ bool hist_out_cell(const HistArgs& a, const HistBlock& b, int rem, int64_t& e) {
  const int ls = rem / (8 * a.B);
  const int jj = (rem / a.B) & 7;
  const int bn = rem % a.B;
  const int f = b.fbase + jj;
  const int slot = b.s0 + ls;
  e = (((int64_t)slot * a.d + f) * a.B + bn) * a.K;
  return f < a.d && slot < a.S;
}

// Flush of the LDS planes: 64-bit plane p -> out plane 1 when SUM_K1 (count + sum moments: the one 64-bit plane is
// the sum), else p; 32-bit plane p -> out plane p.
template <bool SUM_K1, int TH>
__device__ __forceinline__ void hist_flush_planes(const HistArgs& a, const HistBlock& b, const HistLds& l, int plane) {
  const int total = (a.n64 + a.n32) * plane;
  for (int i = threadIdx.x; i < total; i += TH) {
    const bool is64 = i < a.n64 * plane;
    const int p = is64 ? i / plane : (i - a.n64 * plane) / plane;
    const int rem = i - (is64 ? p : a.n64 + p) * plane;
    long long v;
    int k;
    if (is64) {
      v = (long long)l.h64[i];
      k = SUM_K1 ? 1 : p;
    } else {
      v = (long long)l.h32[i - a.n64 * plane];
      k = p;
    }
    if (v == 0) continue;
    int64_t e;
    if (hist_out_cell(a, b, rem, e)) atomicAdd(&a.out[e + k], (unsigned long long)v);
  }
}

// Flush of the packed kernels' register accumulators (thread t: cells t, t + TH, ...) to out[..][0] / out[..][1]
template <int TH, int N>
__device__ __forceinline__ void hist_flush_cells(const HistArgs& a, const HistBlock& b, int plane,
                                                 const uint32_t (&acc_c)[N], const long long (&acc_s)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int idx = (int)threadIdx.x + i * TH;
    if (idx >= plane || acc_c[i] == 0u) continue;
    int64_t e;
    if (hist_out_cell(a, b, idx, e)) {
      unsigned long long* o = &a.out[e];
      atomicAdd(o, (unsigned long long)acc_c[i]);
      atomicAdd(o + 1, (unsigned long long)acc_s[i]);
    }
  }
}

}  // namespace cdna
