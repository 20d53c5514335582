// rfa_mlarope.hip — the K / V assembly of multi-head latent attention fused with the rotary embedding at GLOBAL positions
// (gfx950; include/rfa.h: rfa_mla_rotary_fwd / _bwd; ring_flash_attn.apply_mla_rotary).  Between its projections and the
// attention call a DeepSeek-V2 / V3 / Kimi K2 layer holds, per token, q (Hq, Dn + Dr), kv (H, Dn + Dv) = [k_nope | v] and ONE rope
// key k_pe (Dr) shared by all heads, and needs q with its last Dr columns rotated, k (H, Dn + Dr) = [k_nope | rope(k_pe)] and
// v (H, Dv).  As torch ops that is split, two rotations, expand, cat and two contiguous copies — and, backward, a sum over heads
// whose order nobody controls.  Here each direction is ONE launch that reads every input once and writes every output once.
//
// A workgroup of 256 threads owns a tile of kMlaRopeRows rows of one batch entry (rfa_mlarope_index.h).
// Forward:
//   1. table phase  lane (row r, rotation unit w): the row's position — the map's arithmetic or one int32 — clamped into the
//                   tables, 8 (interleaved: 4) cos and sin values as fp32 into two LDS arrays [rows][Dr/2] (rfa_rotfreq_index.h's
//                   quad order: the stream phase reads them without bank conflicts), and with them the unit's chunk(s) of k_pe
//                   through rot(): the rotated row goes to LDS as Dr io-dtype values.  The row's cos / sin are fetched ONCE,
//                   not once per head, and k_pe is rotated once.
//   __syncthreads()
//   2. q stream     the tile's run of rotary units (rotary_unit(): rfa_rotary.hip's offsets and partners): pass-through chunks
//                   16-byte copies, rotated chunks through rot() with 16-byte LDS reads of cos / sin
//   3. k / v stream the tile's (row, head, chunk) units in the order of the written side: a kv row is read once front to back,
//                   its Dn columns go to k and its Dv columns to v; between them the head's Dr rope columns are 16-byte LDS
//                   reads of the rotated row — the same bits for every head
// Backward (conjugate rotation: s -> -s):
//   1. table phase  as above, without k_pe; the lane keeps its cos / sin in registers
//   1b. head sum    lane (row r, slice, chunk) of rfa_mlarope_index.h adds its heads' dk rope chunks in ascending order in fp32
//                   (8 accumulators), the partial sums go to LDS
//   __syncthreads()
//   1c. fold        lane (r, w) adds the partials of its chunk(s) over the slices in ascending order, applies rot() with the
//                   registers of phase 1 — AFTER the sum: the rotation is linear — rounds once and stores dk_pe
//   2. dq stream    the forward's q stream on the incoming gradient
//   3. dkv stream   dk's Dn columns and dv's Dv columns of every (row, head) into one dkv row
// Sixteen-byte loads and stores, 64-bit global offsets, no atomics, no scratch; the order of every sum depends on H and Dr alone.
// Arithmetic of a rotated pair: rot() of rfa_rotary_math.hpp on the fp32 values rotary_kernel feeds it — the bits apply_rotary
// gives.
// grid: x = B * ceil(S / kMlaRopeRows).  LDS: 2 KiB cos / sin + 1 KiB rotated k_pe (forward) or 8 KiB partial sums (backward).
#include "rfa_mlarope_stream.hpp"  // the streams and the head sum, shared with rfa_mlaropefreq.hip
#include "rfa_rotary_math.hpp"     // rot(), load_tab()

namespace rfa {

// table phase of lane (row r of the tile, rotation unit w): the unit's cos / sin as fp32 in c / s (8 values; interleaved: the
// first 4), sin negated where CONJ, and in LDS where the streams read them
template <typename TT, int INTER, int CONJ>
__device__ __forceinline__ void mlarope_angles(const MlaRopeParams& p, const RotFreqTile& tile, uint32_t r, uint32_t w, f32x4* lds_c4,
                                               f32x4* lds_s4, float (&c)[8], float (&s)[8]) {
  constexpr int N = INTER ? 4 : 8;
  const uint32_t half = p.g.Dr / 2, i = tile.row0 + r, tcol = (uint32_t)N * w;
  int64_t pos = p.positions ? p.pos_off + (int64_t)p.positions[(int64_t)tile.b * p.pos_batch + i]
                            : rotary_map_pos(p.pos_off, p.pos_stride, p.pos_split, p.pos_off2, i);
  pos = rotary_clamp_pos(pos, p.P);                          // (never outside the tables, whatever `positions` holds)
  const int64_t trow = pos * (int64_t)half + tcol;
  float cc[N], ss[N];
  load_tab<TT, N>((const TT*)p.cos + trow, cc);
  load_tab<TT, N>((const TT*)p.sin + trow, ss);
#pragma unroll
  for (int e = 0; e < N; ++e) {
    c[e] = cc[e];
    s[e] = CONJ ? -ss[e] : ss[e];
  }
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const uint32_t at = r * half + rotfreq_lds_quad(half, INTER, tcol, (uint32_t)q);
    lds_c4[at / 4] = f32x4{c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]};
    lds_s4[at / 4] = f32x4{s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]};
  }
}

template <typename T, typename TT, int INTER>
__global__ __launch_bounds__(kMlaRopeThreads) void mlarope_fwd_kernel(const MlaRopeParams p) {
  __shared__ f32x4 lds_c4[kMlaRopeLdsTab];
  __shared__ f32x4 lds_s4[kMlaRopeLdsTab];
  __shared__ vec8<T> lds_k[kMlaRopeRows * kMlaRopeMaxRot / 8];          // the tile's rotated k_pe rows
  const RotFreqTile tile = rotfreq_tile(p.g.S, blockIdx.x, kMlaRopeRows);
  const uint32_t nch = p.g.Dr / 8;

  // ---- 1. cos / sin of the tile's rows and the rotated k_pe, once for all heads
  {
    const uint32_t r = threadIdx.x / kMlaRopeRowThreads, w = threadIdx.x % kMlaRopeRowThreads;
    if (r < tile.nrows && w < p.g.rot_units) {
      float c[8], s[8];
      mlarope_angles<TT, INTER, 0>(p, tile, r, w, lds_c4, lds_s4, c, s);
      const T* src = (const T*)p.k_pe + mlarope_off(p.k_pe_st, tile.b, tile.row0 + r, 0, 0);
      if (INTER == 0) {
        const vec8<T> a = *(const vec8<T>*)(src + 8 * w);
        const vec8<T> b = *(const vec8<T>*)(src + 8 * w + p.g.Dr / 2);
        f32x8 o1, o2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float y1, y2;
          rot((float)a[e], (float)b[e], c[e], s[e], y1, y2);
          o1[e] = y1;
          o2[e] = y2;
        }
        lds_k[r * nch + w] = __builtin_convertvector(o1, vec8<T>);
        lds_k[r * nch + w + nch / 2] = __builtin_convertvector(o2, vec8<T>);
      } else {
        const vec8<T> a = *(const vec8<T>*)(src + 8 * w);
        f32x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float y1, y2;
          rot((float)a[2 * e], (float)a[2 * e + 1], c[e], s[e], y1, y2);
          o[2 * e] = y1;
          o[2 * e + 1] = y2;
        }
        lds_k[r * nch + w] = __builtin_convertvector(o, vec8<T>);
      }
    }
  }
  __syncthreads();

  // ---- 2. q
  if (p.tq.H) mlarope_q_stream<T, INTER>(p, tile, lds_c4, lds_s4);

  // ---- 3. k and v
  mlarope_kv_stream<T>(p, tile, lds_k);
}

template <typename T, typename TT, int INTER>
__global__ __launch_bounds__(kMlaRopeThreads) void mlarope_bwd_kernel(const MlaRopeParams p) {
  __shared__ f32x4 lds_c4[kMlaRopeLdsTab];
  __shared__ f32x4 lds_s4[kMlaRopeLdsTab];
  __shared__ f32x4 lds_part[kMlaRopeRows * kMlaRopeRowThreads * 8 / 4];  // the head sum's partials, fp32
  const RotFreqTile tile = rotfreq_tile(p.g.S, blockIdx.x, kMlaRopeRows);
  const uint32_t r = threadIdx.x / kMlaRopeRowThreads, l = threadIdx.x % kMlaRopeRowThreads;
  const bool sum = p.k_pe != nullptr;                        // (the host: then dk is there)

  // ---- 1. cos / sin of the tile's rows; the lane of a rotation unit keeps its own for the fold
  const bool unit = r < tile.nrows && l < p.g.rot_units;
  float c[8], s[8];
  if (unit) mlarope_angles<TT, INTER, 1>(p, tile, r, l, lds_c4, lds_s4, c, s);

  // ---- 1b. every lane's heads, ascending, in fp32
  if (sum) mlarope_head_sum<T>(p, tile, r, l, lds_part);
  __syncthreads();

  // ---- 1c. the slices' partials, ascending; the conjugate rotation of the SUM; one rounding
  if (sum && unit) mlarope_fold<T, INTER>(p, tile, r, l, lds_part, c, s);

  // ---- 2. dq
  if (p.tq.H) mlarope_q_stream<T, INTER>(p, tile, lds_c4, lds_s4);

  // ---- 3. dkv = [dk's Dn columns | dv]
  if (p.kv) mlarope_dkv_stream<T>(p, tile);
}

template <typename T, typename TT>
static void launch_tt(const MlaRopeParams& p, bool bwd, dim3 grid, hipStream_t stream) {
  const dim3 block(kMlaRopeThreads);
  if (bwd) {
    if (p.g.interleaved) hipLaunchKernelGGL((mlarope_bwd_kernel<T, TT, 1>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((mlarope_bwd_kernel<T, TT, 0>), grid, block, 0, stream, p);
  } else {
    if (p.g.interleaved) hipLaunchKernelGGL((mlarope_fwd_kernel<T, TT, 1>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((mlarope_fwd_kernel<T, TT, 0>), grid, block, 0, stream, p);
  }
}

static int launch(const MlaRopeParams& p, int dtype, bool table_f32, bool bwd, hipStream_t stream) {
  if (p.g.B == 0 || p.g.S == 0) return 0;
  const dim3 grid(p.g.B * rotfreq_tiles_per_batch(p.g.S, kMlaRopeRows));
  if (dtype == 0) {
    if (table_f32) launch_tt<bf16_t, float>(p, bwd, grid, stream);
    else launch_tt<bf16_t, bf16_t>(p, bwd, grid, stream);
  } else {
    if (table_f32) launch_tt<f16_t, float>(p, bwd, grid, stream);
    else launch_tt<f16_t, f16_t>(p, bwd, grid, stream);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_mla_rotary_fwd(const MlaRopeParams& p, int dtype, bool table_f32, hipStream_t stream) {
  return launch(p, dtype, table_f32, false, stream);
}

int launch_mla_rotary_bwd(const MlaRopeParams& p, int dtype, bool table_f32, hipStream_t stream) {
  return launch(p, dtype, table_f32, true, stream);
}

}  // namespace rfa
