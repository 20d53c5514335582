// rfa_qknorm.hip — per-head RMSNorm of q and k fused with the rotary embedding at GLOBAL positions (gfx950; include/rfa.h:
// rfa_qk_norm_rotary_fwd / _bwd; ring_flash_attn.apply_qk_norm_rotary).  Qwen3, Gemma-3 and OLMo-style models compute
//     q = rope(rmsnorm_D(q) * w_q),   k = rope(rmsnorm_D(k) * w_k)
// per head; as a torch composite in front of rfa_rotary that is two more passes forward, four or five backward, a rounding to
// the io dtype between norm and rotation and an atomics-based weight gradient.  Here q and k go through ONE launch per
// direction, every value is rounded once, and nothing depends on the order in which workgroups finish.
//
// Streaming kernels in the style of rfa_rotary.hip.  A (row, head) lives in a lane group of G = qknorm_group(D) lanes of one wave
// (rfa_qknorm_index.h), lane w owning the 16-byte chunk of columns 8 w .. 8 w + 7 — whatever is rotated, so the row sums have one
// order per D.  No LDS in the forward, no atomics anywhere, plain vector loads and stores.
//
// SUMMATION ORDERS (the tests' tolerances are derived from these):
//   row sums (sum x^2; backward also sum (g a) xh): in a lane e = 0 .. 7 as a chain of fmas starting from 0, then the xor
//     butterfly over the group with masks G/2, G/4, .. 1 (v += shfl_xor(v, m); idle lanes hold 0): 8 + log2 G <= 13 roundings.
//     Every lane of the group ends with the same bits, and they do not depend on where the group sits in the wave.
//   rstd = rsqrt(ss / D + eps) (one division, one addition, the hardware's rsqrt), computed by ONE device function (row_rstd)
//     in both directions: the backward recomputes the forward's bits.
//   forward: y = (x rstd) a, a = weight_offset + w, then rot() of rfa_rotary_math.hpp on the rotated columns; one rounding.
//   backward: g = rot() with s -> -s of dO (fp32, not rounded), xh = x rstd, m = (sum (g a) xh) / D,
//     dx = rstd (g a - xh m) with the subtraction as ONE fma; one rounding.
//   dw (per tensor): a lane adds g xh of its 8 columns (fma) over the `walk` items it visits, item (it * nparts + p) * (256/G) + group for
//     it = 0, 1, ..; workgroup p adds its 256/G groups in group order through LDS and stores an fp32 (D,) partial; the fold
//     kernel adds a column's nparts partials in 16 runs of ceil(nparts/16) consecutive ones, then the 16 sums in order.
//     Longest chain: walk + 256/G + ceil(nparts/16) + 16 additions.
// The halves pairing needs the partner chunk's 8 values from the lane R/16 away: 8 shuffles (ds_bpermute) in the wave.
// grid: forward x = ceil(max items / (256/G)), y = tensor; backward x = max over tensors of nparts, y = tensor, where a tensor's
// nparts = min(ceil(ITS items / (256/G)), 1024): its weight gradient's bits do not depend on the tensor that rides along.
#include "rfa_common.hpp"
#include "rfa_kernels.hpp"
#include "rfa_rotary_math.hpp"

namespace rfa {

__device__ __forceinline__ float group_sum(float v, uint32_t G) {
  for (uint32_t m = G >> 1; m; m >>= 1) v += __shfl_xor(v, (int)m, 64);
  return v;
}

// 1 / sqrt(mean of the row's squares + eps) from the lane's 8 values (idle lanes: zeros); all lanes of a wave call it
__device__ __forceinline__ float row_rstd(const float (&x)[8], uint32_t G, uint32_t D, float eps) {
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) ss = __builtin_fmaf(x[e], x[e], ss);
  ss = group_sum(ss, G);
  return rsqrtf(ss / (float)D + eps);
}

// a_c = weight_offset + w_c of the lane's 8 columns
template <typename TW>
__device__ __forceinline__ void load_scale(const TW* wp, float off, float (&a)[8]) {
  float lo[4], hi[4];
  load_tab<TW, 4>(wp, lo);
  load_tab<TW, 4>(wp + 4, hi);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = off + lo[e];
    a[4 + e] = off + hi[e];
  }
}

// what a launch rotates — a template parameter: every instance holds one pairing's code alone
enum { kModeNone = 0, kModeHalves = 1, kModeInterleaved = 2 };

// first element of the lane's run in the cos / sin tables at the item's position (clamped to the tables)
__device__ __forceinline__ int64_t table_at(const QkNormParams& p, const QkNormLane& l, uint32_t b, uint32_t i) {
  int64_t pos = p.positions ? p.pos_off + (int64_t)p.positions[(int64_t)b * p.pos_batch + i]
                            : rotary_map_pos(p.pos_off, p.pos_stride, p.pos_split, p.pos_off2, i);
  pos = rotary_clamp_pos(pos, p.P);
  return pos * (int64_t)(p.g.R / 2) + l.tcol;
}

// the lane's 8 columns after the rotation (CONJ: the inverse one) at table run `trow` (rotating lanes only read it).  Every
// lane of the wave takes part in the shuffles of the halves pairing; `src` is the wave lane of the partner chunk (its own
// where it has none).  Pass-through lanes return their values' own bits.
template <int MODE, bool CONJ, typename TT>
__device__ __forceinline__ void rotate8(const QkNormParams& p, const float (&v)[8], float (&o)[8], int kind, bool rotating,
                                        int64_t trow, int src) {
  if constexpr (MODE == kModeHalves) {
    float c[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f}, s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (rotating) {
      load_tab<TT, 8>((const TT*)p.cos + trow, c);
      load_tab<TT, 8>((const TT*)p.sin + trow, s);
    }
    const bool lo = kind == kQkNormLo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float pv = __shfl(v[e], src, 64);
      float o1, o2;
      rot(lo ? v[e] : pv, lo ? pv : v[e], c[e], CONJ ? -s[e] : s[e], o1, o2);
      o[e] = rotating ? (lo ? o1 : o2) : v[e];
    }
  } else if constexpr (MODE == kModeInterleaved) {
    float c[4] = {1.f, 1.f, 1.f, 1.f}, s[4] = {0.f, 0.f, 0.f, 0.f};
    if (rotating) {
      load_tab<TT, 4>((const TT*)p.cos + trow, c);
      load_tab<TT, 4>((const TT*)p.sin + trow, s);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float o1, o2;
      rot(v[2 * e], v[2 * e + 1], c[e], CONJ ? -s[e] : s[e], o1, o2);
      o[2 * e] = rotating ? o1 : v[2 * e];
      o[2 * e + 1] = rotating ? o2 : v[2 * e + 1];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = v[e];
  }
}

typedef float f32x8 __attribute__((ext_vector_type(8)));

template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&f)[8]) {
  const vec8<T> v = *(const vec8<T>*)p;
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
}

template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&f)[8]) {
  f32x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = f[e];
  *(vec8<T>*)p = __builtin_convertvector(v, vec8<T>);
}

template <typename T, typename TT, typename TW, int MODE>
__global__ __launch_bounds__(256) void qknorm_fwd_kernel(const QkNormParams p) {
  const int k = blockIdx.y;
  const QkNormTensor t = p.t[k];
  const uint32_t G = p.g.group, per = kQkNormThreads / G;
  if ((uint64_t)blockIdx.x * per >= t.nitems) return;            // (the whole workgroup: the other tensor is longer)
  const uint32_t w = threadIdx.x & (G - 1);
  const uint32_t item = blockIdx.x * per + threadIdx.x / G;
  const bool live = item < t.nitems && w < p.g.chunks;
  QkNormLane l;
  qknorm_lane(p.g, w, &l);
  const int src = (int)((threadIdx.x & 63u & ~(G - 1)) + l.partner);
  const bool rotating = live && l.kind != kQkNormPass;
  float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  QkNormChunk ch{};
  int64_t trow = 0;
  if (live) {
    qknorm_chunk(p.g, t, item, w, &ch);
    load8<T>((const T*)p.x[k] + ch.x, x);
    load_scale<TW>((const TW*)p.weight[k] + l.col, p.weight_offset, a);
  }
  if (MODE != kModeNone && rotating) trow = table_at(p, l, ch.b, ch.i);
  const float rstd = row_rstd(x, G, p.g.D, p.eps);
  float y[8], o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = (x[e] * rstd) * a[e];
  rotate8<MODE, false, TT>(p, y, o, l.kind, rotating, trow, src);
  if (live) store8<T>((T*)p.out[k] + ch.o, o);
}

template <typename T, typename TT, typename TW, int MODE>
__global__ __launch_bounds__(256) void qknorm_bwd_kernel(const QkNormParams p) {
  __shared__ float part[kQkNormThreads * 8];                     // (256/G groups) x D columns, D <= 8 G
  const int k = blockIdx.y;
  const QkNormTensor t = p.t[k];
  const uint32_t G = p.g.group, per = kQkNormThreads / G, D = p.g.D;
  const uint32_t w = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const bool owns = w < p.g.chunks;
  const bool want_dw = p.dweight[k] != nullptr;
  const uint32_t nparts = p.nparts[k], walk = p.walk[k];
  if (blockIdx.x >= nparts) return;                              // (the whole workgroup: the other tensor has more partials)
  QkNormLane l;
  qknorm_lane(p.g, w, &l);
  const int src = (int)((threadIdx.x & 63u & ~(G - 1)) + l.partner);
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (owns) load_scale<TW>((const TW*)p.weight[k] + l.col, p.weight_offset, a);
  for (uint32_t it = 0; it < walk; ++it) {
    const uint64_t first = ((uint64_t)it * nparts + blockIdx.x) * per;
    if (first >= t.nitems) break;                                // (the whole workgroup, and every later step of its walk)
    const uint64_t item = first + grp;
    const bool live = owns && item < t.nitems;
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool rotating = live && l.kind != kQkNormPass;
    QkNormChunk ch{};
    int64_t trow = 0;
    if (live) {
      qknorm_chunk(p.g, t, (uint32_t)item, w, &ch);
      load8<T>((const T*)p.x[k] + ch.x, x);
      load8<T>((const T*)p.dout[k] + ch.g, d);
    }
    if (MODE != kModeNone && rotating) trow = table_at(p, l, ch.b, ch.i);
    // (a lane group past the tensor's end holds zeros: with eps == 0 its rsqrt(0) is inf and 0 * inf would poison the weight
    //  gradient its lanes accumulate — such a group counts with rstd 0; every lane of the wave still takes part in the shuffles)
    const float rs = row_rstd(x, G, D, p.eps);
    const float rstd = item < t.nitems ? rs : 0.f;
    float g[8], ga[8], xh[8], dx[8];
    rotate8<MODE, true, TT>(p, d, g, l.kind, rotating, trow, src);
    float ms = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xh[e] = x[e] * rstd;
      ga[e] = g[e] * a[e];
      ms = __builtin_fmaf(ga[e], xh[e], ms);
    }
    const float m = group_sum(ms, G) / (float)D;
#pragma unroll
    for (int e = 0; e < 8; ++e) dx[e] = rstd * __builtin_fmaf(-xh[e], m, ga[e]);
    if (live) store8<T>((T*)p.out[k] + ch.o, dx);
    if (want_dw) {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(g[e], xh[e], acc[e]);
    }
  }
  if (!want_dw) return;                                          // (uniform over the workgroup)
  if (owns) {
#pragma unroll
    for (int e = 0; e < 8; ++e) part[grp * D + l.col + e] = acc[e];
  }
  __syncthreads();
  if (threadIdx.x < D) {
    float sum = 0.f;
    for (uint32_t gi = 0; gi < per; ++gi) sum += part[gi * D + threadIdx.x];
    p.workspace[((size_t)(k ? p.nparts[0] : 0u) + blockIdx.x) * D + threadIdx.x] = sum;
  }
}

// dweight[k][c] = the nparts partials of column c: 16 runs of consecutive partials, then the runs in order
__global__ __launch_bounds__(256) void qknorm_fold_kernel(const QkNormParams p) {
  __shared__ float runs[kQkNormFoldSlices][16];
  const int k = blockIdx.y;
  if (!p.dweight[k]) return;
  const uint32_t c = blockIdx.x * 16 + (threadIdx.x & 15), j = threadIdx.x >> 4, D = p.g.D;
  const uint32_t nparts = p.nparts[k], len = qknorm_fold_len(nparts);
  const uint32_t lo = j * len < nparts ? j * len : nparts, hi = lo + len < nparts ? lo + len : nparts;
  float sum = 0.f;
  if (c < D)
    for (uint32_t q = lo; q < hi; ++q) sum += p.workspace[((size_t)(k ? p.nparts[0] : 0u) + q) * D + c];
  runs[j][threadIdx.x & 15] = sum;
  __syncthreads();
  if (j == 0 && c < D) {
    float total = 0.f;
    for (int r = 0; r < kQkNormFoldSlices; ++r) total += runs[r][threadIdx.x];
    p.dweight[k][c] = total;
  }
}

template <typename T, typename TT, typename TW, int MODE>
static void launch_m(const QkNormParams& p, bool bwd, dim3 grid, hipStream_t stream) {
  const dim3 block(kQkNormThreads);
  if (bwd) hipLaunchKernelGGL((qknorm_bwd_kernel<T, TT, TW, MODE>), grid, block, 0, stream, p);
  else hipLaunchKernelGGL((qknorm_fwd_kernel<T, TT, TW, MODE>), grid, block, 0, stream, p);
}

template <typename T, typename TW>
static void launch_tw(const QkNormParams& p, bool bwd, bool table_f32, dim3 grid, hipStream_t stream) {
  if (p.g.R == 0) {                                              // the norm alone reads no table: ONE table type serves it
    launch_m<T, T, TW, kModeNone>(p, bwd, grid, stream);
  } else if (p.g.interleaved) {
    if (table_f32) launch_m<T, float, TW, kModeInterleaved>(p, bwd, grid, stream);
    else launch_m<T, T, TW, kModeInterleaved>(p, bwd, grid, stream);
  } else {
    if (table_f32) launch_m<T, float, TW, kModeHalves>(p, bwd, grid, stream);
    else launch_m<T, T, TW, kModeHalves>(p, bwd, grid, stream);
  }
}

template <typename T>
static void launch_t(const QkNormParams& p, bool bwd, bool table_f32, bool weight_f32, dim3 grid, hipStream_t stream) {
  if (weight_f32) launch_tw<T, float>(p, bwd, table_f32, grid, stream);
  else launch_tw<T, T>(p, bwd, table_f32, grid, stream);
}

static uint32_t most_items(const QkNormParams& p) {
  uint32_t most = 0;
  for (int i = 0; i < p.ntensors; ++i) most = p.t[i].nitems > most ? p.t[i].nitems : most;
  return most;
}

int launch_qknorm_fwd(const QkNormParams& p, int dtype, bool table_f32, bool weight_f32, hipStream_t stream) {
  const uint32_t most = most_items(p);
  if (most == 0) return 0;
  dim3 grid(qknorm_blocks(most, p.g.group), (unsigned)p.ntensors);
  if (dtype == 0) launch_t<bf16_t>(p, false, table_f32, weight_f32, grid, stream);
  else launch_t<f16_t>(p, false, table_f32, weight_f32, grid, stream);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_qknorm_bwd(const QkNormParams& p, int dtype, bool table_f32, bool weight_f32, hipStream_t stream) {
  const uint32_t blocks = p.ntensors > 1 && p.nparts[1] > p.nparts[0] ? p.nparts[1] : p.nparts[0];
  if (most_items(p) == 0 || blocks == 0) return 0;
  dim3 grid(blocks, (unsigned)p.ntensors);
  if (dtype == 0) launch_t<bf16_t>(p, true, table_f32, weight_f32, grid, stream);
  else launch_t<f16_t>(p, true, table_f32, weight_f32, grid, stream);
  if (hipGetLastError() != hipSuccess) return -1;
  bool any = false;
  for (int i = 0; i < p.ntensors; ++i) any = any || p.dweight[i] != nullptr;
  if (any) {
    hipLaunchKernelGGL(qknorm_fold_kernel, dim3((p.g.D + 15) / 16, (unsigned)p.ntensors), dim3(kQkNormThreads), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  return 0;
}

}  // namespace rfa
