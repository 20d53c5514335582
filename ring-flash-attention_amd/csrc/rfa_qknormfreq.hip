// rfa_qknormfreq.hip — per-head RMSNorm of q and k fused with a rotary embedding whose angles are formed IN the kernel, one to
// four position axes per row (gfx950; include/rfa.h: rfa_qk_norm_rotary_freqs_fwd / _bwd;
// ring_flash_attn.apply_qk_norm_rotary_freqs).  Qwen3-VL runs a per-head QK RMSNorm in front of a three-axis M-RoPE, for
// which no table exists; Qwen3 / Gemma-3 at long context would need tables of the whole unsharded sequence on every rank.
// Neither existing kernel serves them by a flag: rfa_qknorm.hip owns one (row, head) per lane group and would call sincosf
// per HEAD; rfa_rotfreq.hip streams 16-byte units and knows no row statistic.  This one joins their two ideas.
//
// A workgroup of 256 threads owns a TILE of kQkNfRows rows of one batch entry, for all H + Hk heads of q and k
// (rfa_qknormfreq_index.h):
//   1. angle phase   the nrows * R/2 entries (row, c) of the tile, strided over the threads, by rotfreq_kernel's
//                    expressions: pos (the map, or one int32 of the axis c reads; the axis map travels 2 bits per frequency in the
//                    kernel arguments), ang = mul_rn(float(pos), inv_freq[c]), the precise sincosf, c' = scaling cos,
//                    s' = scaling sin (backward: -s'), as fp32 into two LDS arrays [rows][R/2] (halves: quads permuted,
//                    rotfreq_lds_col) — once for all heads.
//   __syncthreads()  the one barrier of a tile (the backward, which walks several tiles, has a second one in front of the next
//                    tile's angle phase)
//   2. norm + rotate the tile's (row, head) items of q, then of k (backward: of the tensor blockIdx.y names — the two
//                    tensors' strides, pointers and accumulators together do not fit the scalar registers without spilling,
//                    so a tile's angles are formed once per tensor there), in passes over the 256/G lane groups, G = qknorm_group(D).
//                    Lane w of a group holds the 16-byte chunk of columns 8 w .. 8 w + 7; the row statistic, the scale and the
//                    partner chunk by shuffles are rfa_qknorm.hip's (rfa_qknorm_math.hpp: the same functions); the lane's 8
//                    (interleaved: 4) c' / s' values are 16-byte LDS reads without bank conflicts — all groups on one row
//                    read the same addresses (a broadcast).  Idle lanes and groups past the tile's end hold zeros and take
//                    part in every shuffle.
// Plain vector loads and stores, 64-bit global offsets, no atomics, nothing depends on the order in which workgroups finish.
//
// SUMMATION ORDERS (the tests' tolerances are derived from these):
//   row sums (sum x^2; backward also sum (g a) xh): in a lane e = 0 .. 7 as a chain of fmas starting from 0, then the xor
//     butterfly over the group with masks G/2, G/4, .. 1: 8 + log2 G <= 13 roundings — row_rstd() / group_sum() themselves.
//   rstd = rsqrt(ss / D + eps): row_rstd(); forward and backward compute the same bits, and they are rfa_qknorm.hip's.
//   angle: ONE rounded multiply, sincosf, ONE rounded multiply by the scaling — per (row, c) the same expression whichever
//     thread, tile or direction gets it.
//   forward: y = (x rstd) a, a = weight_offset + w, then rot() of rfa_rotary_math.hpp on the rotated columns; one rounding.
//   backward: g = rot() with s' -> -s' of dO (fp32, not rounded), xh = x rstd (a group past the tile's end: rstd = 0, the
//     eps = 0 rule), m = (sum (g a) xh) / D, dx = rstd (g a - xh m) with the subtraction as ONE fma; one rounding.
//   dw (per tensor): workgroup p of nparts = min(tiles, 1024) walks the tiles p, p + nparts, ..; a lane adds g xh of its 8
//     columns (fma) over the items it visits — tile after tile, pass after pass; the workgroup adds its 256/G groups in group
//     order through LDS and stores an fp32 (D,) partial; the fold kernel adds a column's nparts partials in 16 runs of
//     ceil(nparts/16) consecutive ones, then the 16 sums in order.  With tiles = B ceil(S / rows) and
//     passes = ceil(rows H / (256/G)), the longest chain is  ceil(tiles/nparts) passes + 256/G + ceil(nparts/16) + 16
//     additions.  nparts and the walk depend on B and S alone: a tensor's dw bits do not depend on the one that rides along.
// grid: forward x = tiles; backward x = nparts, y = tensor, then the fold (ceil(D/16), tensors).  LDS: 4 KiB forward, 12 KiB backward.
#include "rfa_common.hpp"
#include "rfa_kernels.hpp"
#include "rfa_rotary_math.hpp"     // rot(), mul_rn()
#include "rfa_qknorm_math.hpp"     // row_rstd(), group_sum(), load_scale(), load8(), store8()

namespace rfa {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// 1. the (cos', sin') entries of the tile's rows into LDS.  Entry e = r * R/2 + c of a tile goes to thread e % 256 whatever the
// tile, so what depends on (r, c) alone — the frequency, where the axis of c starts in `positions`, the LDS slot — is found
// ONCE per thread (qknf_entries), in front of the backward's walk over its tiles; what a tile adds is the position itself.
template <int ROWS>
struct QknfEntries {
  enum { kN = (ROWS * kRotFreqMaxHalf + kQkNfThreads - 1) / kQkNfThreads };
  float inv[kN];            // inv_freq[c]
  int64_t axis[kN];         // axis(c) * pos_axis
  uint32_t r[kN], at[kN];   // row of the tile (>= ROWS: the thread has no such entry), float index in the LDS arrays
};

template <int INTER, int ROWS>
__device__ __forceinline__ void qknf_entries(const QkNormFreqParams& p, uint32_t half, QknfEntries<ROWS>& en) {
#pragma unroll
  for (int m = 0; m < QknfEntries<ROWS>::kN; ++m) {
    const uint32_t e = threadIdx.x + m * kQkNfThreads;
    const uint32_t r = e / half, c = e - r * half;
    en.r[m] = r < (uint32_t)ROWS ? r : (uint32_t)ROWS;
    en.inv[m] = 0.f;
    en.axis[m] = 0;
    en.at[m] = 0;
    if (r < (uint32_t)ROWS) {
      en.inv[m] = p.inv_freq[c];
      en.axis[m] = (int64_t)rotfreq_axis(p.freq_axis[0], p.freq_axis[1], p.freq_axis[2], p.freq_axis[3], c) * p.pos_axis;
      en.at[m] = r * half + rotfreq_lds_col(half, INTER, c);
    }
  }
}

// CONJ (the backward): sin' -> -sin'
template <bool CONJ, int ROWS>
__device__ __forceinline__ void qknf_angles(const QkNormFreqParams& p, const RotFreqTile& tile, const QknfEntries<ROWS>& en,
                                            float* lds_c, float* lds_s) {
#pragma unroll
  for (int m = 0; m < QknfEntries<ROWS>::kN; ++m) {
    if (en.r[m] >= tile.nrows) continue;
    const uint32_t i = tile.row0 + en.r[m];
    const int64_t pos = p.positions ? p.pos_off + (int64_t)p.positions[en.axis[m] + (int64_t)tile.b * p.pos_batch + i]
                                    : rotary_map_pos(p.pos_off, p.pos_stride, p.pos_split, p.pos_off2, i);
    const float ang = mul_rn((float)pos, en.inv[m]);
    float sn, cs;
    sincosf(ang, &sn, &cs);
    cs = mul_rn(cs, p.scaling);
    sn = mul_rn(sn, p.scaling);
    lds_c[en.at[m]] = cs;
    lds_s[en.at[m]] = CONJ ? -sn : sn;
  }
}

// the lane's 8 columns after the rotation by the LDS entries of tile row r (rotating lanes only read them).  Every lane of the
// wave takes part in the shuffles of the halves pairing; `src` is the wave lane of the partner chunk (its own where it has
// none).  Pass-through lanes return their values' own bits.
template <int INTER>
__device__ __forceinline__ void qknf_rotate8(const f32x4* lds_c4, const f32x4* lds_s4, uint32_t half, const float (&v)[8],
                                             float (&o)[8], const QkNormLane& l, bool rotating, uint32_t r, int src) {
  if constexpr (INTER == 0) {
    f32x4 c0 = {1.f, 1.f, 1.f, 1.f}, c1 = c0, s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    if (rotating) {
      const uint32_t lo = qknf_lds_at(half, 0, r, l.tcol, 0) / 4, hi = qknf_lds_at(half, 0, r, l.tcol, 1) / 4;
      c0 = lds_c4[lo]; c1 = lds_c4[hi];
      s0 = lds_s4[lo]; s1 = lds_s4[hi];
    }
    const bool lo = l.kind == kQkNormLo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float pv = __shfl(v[e], src, 64);
      float o1, o2;
      rot(lo ? v[e] : pv, lo ? pv : v[e], e < 4 ? c0[e & 3] : c1[e & 3], e < 4 ? s0[e & 3] : s1[e & 3], o1, o2);
      o[e] = rotating ? (lo ? o1 : o2) : v[e];
    }
  } else {
    f32x4 c = {1.f, 1.f, 1.f, 1.f}, s = {0.f, 0.f, 0.f, 0.f};
    if (rotating) {
      const uint32_t at = qknf_lds_at(half, 1, r, l.tcol, 0) / 4;
      c = lds_c4[at];
      s = lds_s4[at];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float o1, o2;
      rot(v[2 * e], v[2 * e + 1], c[e], s[e], o1, o2);
      o[2 * e] = rotating ? o1 : v[2 * e];
      o[2 * e + 1] = rotating ? o2 : v[2 * e + 1];
    }
  }
}

template <typename T, typename TW, int INTER, int ROWS = kQkNfRows>
__global__ __launch_bounds__(kQkNfThreads) void qknormfreq_fwd_kernel(const QkNormFreqParams p) {
  __shared__ f32x4 lds_c4[ROWS * kRotFreqMaxHalf / 4];      // written as floats, read as quads
  __shared__ f32x4 lds_s4[ROWS * kRotFreqMaxHalf / 4];
  const RotFreqTile tile = rotfreq_tile(p.g.S, blockIdx.x, ROWS);
  const uint32_t half = p.g.R / 2;
  QknfEntries<ROWS> en;
  qknf_entries<INTER>(p, half, en);
  qknf_angles<false>(p, tile, en, (float*)lds_c4, (float*)lds_s4);
  __syncthreads();

  const uint32_t G = p.g.group, per = kQkNfThreads / G;
  const uint32_t w = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const bool owns = w < p.g.chunks;
  QkNormLane l;
  qknorm_lane(p.g, w, &l);
  const int src = (int)((threadIdx.x & 63u & ~(G - 1)) + l.partner);
  for (int k = 0; k < p.ntensors; ++k) {
    const QkNormTensor t = p.t[k];
    const uint32_t n = qknf_tile_items(tile.nrows, t.H);
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (owns) load_scale<TW>((const TW*)p.weight[k] + l.col, p.weight_offset, a);
    for (uint32_t j0 = 0; j0 < n; j0 += per) {                 // (uniform over the workgroup)
      const uint32_t j = j0 + grp;
      const bool live = owns && j < n;
      float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      QkNormChunk ch{};
      if (live) {
        qknf_chunk(t, tile, j, w, &ch);
        load8<T>((const T*)p.x[k] + ch.x, x);
      }
      const float rstd = row_rstd(x, G, p.g.D, p.eps);
      float y[8], o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = (x[e] * rstd) * a[e];
      qknf_rotate8<INTER>(lds_c4, lds_s4, half, y, o, l, live && l.kind != kQkNormPass, ch.i - tile.row0, src);
      if (live) store8<T>((T*)p.out[k] + ch.o, o);
    }
  }
}

template <typename T, typename TW, int INTER, int ROWS = kQkNfRows>
__global__ __launch_bounds__(kQkNfThreads) void qknormfreq_bwd_kernel(const QkNormFreqParams p) {
  __shared__ f32x4 lds_c4[ROWS * kRotFreqMaxHalf / 4];
  __shared__ f32x4 lds_s4[ROWS * kRotFreqMaxHalf / 4];
  __shared__ float part[kQkNfThreads * 8];                     // (256/G groups) x D columns, D <= 8 G
  const uint32_t half = p.g.R / 2, D = p.g.D;
  const uint32_t G = p.g.group, per = kQkNfThreads / G;
  const uint32_t w = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  const bool owns = w < p.g.chunks;
  const uint32_t tiles = qknf_tiles(p.g.B, p.g.S, ROWS);
  QkNormLane l;
  qknorm_lane(p.g, w, &l);
  const int src = (int)((threadIdx.x & 63u & ~(G - 1)) + l.partner);
  const int k = blockIdx.y;
  const QkNormTensor t = p.t[k];
  const bool want_dw = p.dweight[k] != nullptr;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (owns) load_scale<TW>((const TW*)p.weight[k] + l.col, p.weight_offset, a);
  QknfEntries<ROWS> en;
  qknf_entries<INTER>(p, half, en);

  for (uint32_t ti = blockIdx.x; ti < tiles; ti += p.nparts) {   // (uniform over the workgroup)
    const RotFreqTile tile = rotfreq_tile(p.g.S, ti, ROWS);
    if (ti != blockIdx.x) __syncthreads();                     // (the last tile's LDS reads are done)
    qknf_angles<true>(p, tile, en, (float*)lds_c4, (float*)lds_s4);
    __syncthreads();
    const uint32_t n = qknf_tile_items(tile.nrows, t.H);
    for (uint32_t j0 = 0; j0 < n; j0 += per) {
      const uint32_t j = j0 + grp;
      const bool live = owns && j < n;
      float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      QkNormChunk ch{};
      if (live) {
        qknf_chunk(t, tile, j, w, &ch);
        load8<T>((const T*)p.x[k] + ch.x, x);
        load8<T>((const T*)p.dout[k] + ch.g, d);
      }
      // (a lane group past the tile's end holds zeros: with eps == 0 its rsqrt(0) is inf and 0 * inf would poison the weight
      //  gradient its lanes accumulate — such a group counts with rstd 0; every lane of the wave still takes part in the shuffles)
      const float rs = row_rstd(x, G, D, p.eps);
      const float rstd = j < n ? rs : 0.f;
      float g[8], ga[8], xh[8], dx[8];
      qknf_rotate8<INTER>(lds_c4, lds_s4, half, d, g, l, live && l.kind != kQkNormPass, ch.i - tile.row0, src);
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
  }
  if (!want_dw) return;                                          // (uniform over the workgroup)
  // the workgroup's partial of the weight gradient: its lane groups in group order
  if (owns) {
#pragma unroll
    for (int e = 0; e < 8; ++e) part[grp * D + l.col + e] = acc[e];
  }
  __syncthreads();
  if (threadIdx.x < D) {
    float sum = 0.f;
    for (uint32_t gi = 0; gi < per; ++gi) sum += part[gi * D + threadIdx.x];
    p.workspace[((size_t)k * p.nparts + blockIdx.x) * D + threadIdx.x] = sum;
  }
}

// dweight[k][c] = the nparts partials of column c: 16 runs of consecutive partials, then the runs in order
__global__ __launch_bounds__(kQkNfThreads) void qknormfreq_fold_kernel(const QkNormFreqParams p) {
  __shared__ float runs[kQkNormFoldSlices][16];
  const int k = blockIdx.y;
  if (!p.dweight[k]) return;
  const uint32_t c = blockIdx.x * 16 + (threadIdx.x & 15), j = threadIdx.x >> 4, D = p.g.D;
  const uint32_t nparts = p.nparts, len = qknorm_fold_len(nparts);
  const uint32_t lo = j * len < nparts ? j * len : nparts, hi = lo + len < nparts ? lo + len : nparts;
  float sum = 0.f;
  if (c < D)
    for (uint32_t q = lo; q < hi; ++q) sum += p.workspace[((size_t)k * nparts + q) * D + c];
  runs[j][threadIdx.x & 15] = sum;
  __syncthreads();
  if (j == 0 && c < D) {
    float total = 0.f;
    for (int r = 0; r < kQkNormFoldSlices; ++r) total += runs[r][threadIdx.x];
    p.dweight[k][c] = total;
  }
}

template <typename T, typename TW>
static void launch_tw(const QkNormFreqParams& p, bool bwd, dim3 grid, hipStream_t stream) {
  const dim3 block(kQkNfThreads);
  if (bwd) {
    if (p.g.interleaved) hipLaunchKernelGGL((qknormfreq_bwd_kernel<T, TW, 1>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((qknormfreq_bwd_kernel<T, TW, 0>), grid, block, 0, stream, p);
  } else {
    if (p.g.interleaved) hipLaunchKernelGGL((qknormfreq_fwd_kernel<T, TW, 1>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((qknormfreq_fwd_kernel<T, TW, 0>), grid, block, 0, stream, p);
  }
}

static void launch_t(const QkNormFreqParams& p, bool bwd, int dtype, bool weight_f32, dim3 grid, hipStream_t stream) {
  if (dtype == 0) {
    if (weight_f32) launch_tw<bf16_t, float>(p, bwd, grid, stream);
    else launch_tw<bf16_t, bf16_t>(p, bwd, grid, stream);
  } else {
    if (weight_f32) launch_tw<f16_t, float>(p, bwd, grid, stream);
    else launch_tw<f16_t, f16_t>(p, bwd, grid, stream);
  }
}

int launch_qknormfreq_fwd(const QkNormFreqParams& p, int dtype, bool weight_f32, hipStream_t stream) {
  const uint32_t tiles = qknf_tiles(p.g.B, p.g.S);
  if (tiles == 0) return 0;
  launch_t(p, false, dtype, weight_f32, dim3(tiles), stream);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_qknormfreq_bwd(const QkNormFreqParams& p, int dtype, bool weight_f32, hipStream_t stream) {
  if (p.nparts == 0) return 0;
  launch_t(p, true, dtype, weight_f32, dim3(p.nparts, (unsigned)p.ntensors), stream);
  if (hipGetLastError() != hipSuccess) return -1;
  bool any = false;
  for (int i = 0; i < p.ntensors; ++i) any = any || p.dweight[i] != nullptr;
  if (any) {
    hipLaunchKernelGGL(qknormfreq_fold_kernel, dim3((p.g.D + 15) / 16, (unsigned)p.ntensors), dim3(kQkNfThreads), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  return 0;
}

}  // namespace rfa
