// rfa_mlaropefreq.hip — the K / V assembly of multi-head latent attention fused with a rotary embedding whose angles are formed
// IN the kernel (gfx950; include/rfa.h: rfa_mla_rotary_freqs_fwd / _bwd; ring_flash_attn.apply_mla_rotary_freqs).  What
// rfa_mlarope.hip does with (P, Dr/2) tables this does with inv_freq (Dr/2 fp32 numbers), the positions and a scaling — YaRN's
// attention_scaling, which DeepSeek-V2 / V3 / R1 and Kimi K2 all run with: no table of the unsharded sequence on every rank.
// Per row and frequency c < Dr/2, in fp32, rfa_rotfreq.hip's expression to the letter:
//     ang = float(pos) * inv_freq[c]      ONE rounded multiply (mul_rn: contraction off)
//     (s, c) = sincosf(ang)               the precise function with its full range reduction
//     c' = scaling * c,  s' = scaling * s (backward: s' -> -s')
// and then rot() of rfa_rotary_math.hpp, each result rounded once: the bits apply_rotary_freqs gives.
//
// Ownership, streams and head sum are rfa_mlarope.hip's (rfa_mlarope_stream.hpp — the same device functions): a workgroup of 256
// threads owns a tile of kMlaRopeRows = 2 rows of one batch entry.  The preparation phase is new.  The table kernel gives a
// row to its Dr/16 (interleaved: Dr/8) rotation-unit lanes, 8 (4) table values each; with sincosf in place of a load those few
// lanes would each run 8 range reductions while 240 idle.  Here ONE LANE OWNS ONE (row, frequency): lane e < nrows * Dr/2 is row
// e / (Dr/2), frequency e % (Dr/2) — 64 lanes at Dr = 64, all 256 at Dr = 256 — and
// Forward:
//   1. angle phase  the lane issues the 2-byte loads of ITS pair of k_pe (c, c + Dr/2; interleaved: 2c, 2c + 1), resolves the
//                   row's position (the map's arithmetic or one int32), forms the angle, calls sincosf ONCE, writes c' / s' as
//                   fp32 into the two LDS arrays in rfa_rotfreq_index.h's quad order, and rotates its own pair with the values
//                   it still holds: two io-dtype values into the LDS row of the rotated k_pe.  The pair of a frequency needs no
//                   other lane's angle, so k_pe is rotated in FRONT of the barrier: one barrier, as in the table kernel (a
//                   rotation by the rotation-unit lanes out of LDS would wait for a second one)
//   __syncthreads()
//   2. q stream, 3. k / v stream: rfa_mlarope.hip's, untouched — 16-byte LDS reads of c' / s' and of the rotated k_pe row
// Backward:
//   1. angle phase  as above without k_pe, s' negated
//   1b. head sum    rfa_mlarope.hip's: 128 lanes a row, slices of Dr/8 lanes, heads ascending, partials to LDS
//   __syncthreads() the barrier the fold waits on anyway now also publishes the angles: the backward gains none
//   1c. fold        the lane of rotation unit w takes ITS c' / -s' out of LDS (the 16-byte quads the q stream reads), adds the
//                   slices' partials in ascending order, rotates the SUM, rounds once, stores dk_pe
//   2. dq stream, 3. dkv stream: untouched
// Sixteen-byte global loads and stores in the streams, 64-bit global offsets, no atomics, no scratch; an element's bits depend on
// its values, its position, inv_freq and the scaling alone; the order of every sum depends on H and Dr alone.
// grid: x = B * ceil(S / kMlaRopeRows).  LDS: 2 KiB c' / s' + 1 KiB rotated k_pe (forward) or 8 KiB partial sums (backward).
#include "rfa_mlarope_stream.hpp"  // the streams and the head sum, shared with rfa_mlarope.hip
#include "rfa_rotary_math.hpp"     // rot(), mul_rn()

namespace rfa {

static_assert(kMlaRopeRows * (kMlaRopeMaxRot / 2) <= kMlaRopeThreads, "one lane per (row, frequency) of a tile");

// angle phase of lane e = (row r of the tile, frequency c): c' and s' (negated where CONJ) in cs / sn and in LDS
template <int INTER, int CONJ>
__device__ __forceinline__ void mlaropefreq_angle(const MlaRopeFreqParams& p, const RotFreqTile& tile, uint32_t r, uint32_t c, float* lds_c,
                                                  float* lds_s, float& cs, float& sn) {
  const uint32_t half = p.g.Dr / 2, i = tile.row0 + r;
  const int64_t pos = p.positions ? p.pos_off + (int64_t)p.positions[(int64_t)tile.b * p.pos_batch + i]
                                  : rotary_map_pos(p.pos_off, p.pos_stride, p.pos_split, p.pos_off2, i);
  const float ang = mul_rn((float)pos, p.inv_freq[c]);
  sincosf(ang, &sn, &cs);
  cs = mul_rn(cs, p.scaling);
  sn = mul_rn(sn, p.scaling);
  if (CONJ) sn = -sn;
  const uint32_t at = r * half + rotfreq_lds_col(half, INTER, c);
  lds_c[at] = cs;
  lds_s[at] = sn;
}

template <typename T, int INTER>
__global__ __launch_bounds__(kMlaRopeThreads) void mlaropefreq_fwd_kernel(const MlaRopeFreqParams p) {
  __shared__ f32x4 lds_c4[kMlaRopeLdsTab];                              // written as floats, read as quads
  __shared__ f32x4 lds_s4[kMlaRopeLdsTab];
  __shared__ vec8<T> lds_k[kMlaRopeRows * kMlaRopeMaxRot / 8];          // the tile's rotated k_pe rows: written as elements
  const RotFreqTile tile = rotfreq_tile(p.g.S, blockIdx.x, kMlaRopeRows);
  const uint32_t Dr = p.g.Dr, half = Dr / 2;

  // ---- 1. one lane per (row, frequency): its angle, once for all heads, and with it its own pair of k_pe
  if (threadIdx.x < tile.nrows * half) {
    const uint32_t r = threadIdx.x / half, c = threadIdx.x - r * half;
    const uint32_t c1 = INTER ? 2 * c : c, c2 = INTER ? 2 * c + 1 : c + half;
    const T* src = (const T*)p.k_pe + mlarope_off(p.k_pe_st, tile.b, tile.row0 + r, 0, 0);
    const float x1 = (float)src[c1], x2 = (float)src[c2];  // (in front of sincosf: their latency hides behind it)
    float cs, sn, y1, y2;
    mlaropefreq_angle<INTER, 0>(p, tile, r, c, (float*)lds_c4, (float*)lds_s4, cs, sn);
    rot(x1, x2, cs, sn, y1, y2);
    // (the fp32 results are pinned in registers: for a lone fp16 value the compiler would otherwise fold rot()'s last fma and
    // the conversion into v_fma_mixlo_f16, which rounds ONCE — the streams' packed conversion rounds the fp32 value, and one
    // element in a few thousand would miss apply_rotary_freqs' bits by an ulp)
    asm volatile("" : "+v"(y1), "+v"(y2));
    T* row = (T*)lds_k + r * Dr;
    row[c1] = (T)y1;
    row[c2] = (T)y2;
  }
  __syncthreads();

  // ---- 2. q
  if (p.tq.H) mlarope_q_stream<T, INTER>(p, tile, lds_c4, lds_s4);

  // ---- 3. k and v
  mlarope_kv_stream<T>(p, tile, lds_k);
}

template <typename T, int INTER>
__global__ __launch_bounds__(kMlaRopeThreads) void mlaropefreq_bwd_kernel(const MlaRopeFreqParams p) {
  __shared__ f32x4 lds_c4[kMlaRopeLdsTab];
  __shared__ f32x4 lds_s4[kMlaRopeLdsTab];
  __shared__ f32x4 lds_part[kMlaRopeRows * kMlaRopeRowThreads * 8 / 4];  // the head sum's partials, fp32
  const RotFreqTile tile = rotfreq_tile(p.g.S, blockIdx.x, kMlaRopeRows);
  const uint32_t half = p.g.Dr / 2;
  const uint32_t r = threadIdx.x / kMlaRopeRowThreads, l = threadIdx.x % kMlaRopeRowThreads;
  const bool sum = p.k_pe != nullptr;                        // (the host: then dk is there)

  // ---- 1. one lane per (row, frequency): c' and -s' to LDS
  if (threadIdx.x < tile.nrows * half) {
    const uint32_t ar = threadIdx.x / half;
    float cs, sn;
    mlaropefreq_angle<INTER, 1>(p, tile, ar, threadIdx.x - ar * half, (float*)lds_c4, (float*)lds_s4, cs, sn);
  }

  // ---- 1b. every lane's heads, ascending, in fp32
  if (sum) mlarope_head_sum<T>(p, tile, r, l, lds_part);
  __syncthreads();

  // ---- 1c. the rotation unit's c' / -s' out of LDS; the slices' partials, ascending; the rotation of the SUM; one rounding
  if (sum && r < tile.nrows && l < p.g.rot_units) {
    constexpr int N = INTER ? 4 : 8;
    float c[8], s[8];
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      const uint32_t at = r * half + rotfreq_lds_quad(half, INTER, (uint32_t)N * l, (uint32_t)q);
      const f32x4 cq = lds_c4[at / 4], sq = lds_s4[at / 4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        c[4 * q + e] = cq[e];
        s[4 * q + e] = sq[e];
      }
    }
    mlarope_fold<T, INTER>(p, tile, r, l, lds_part, c, s);
  }

  // ---- 2. dq
  if (p.tq.H) mlarope_q_stream<T, INTER>(p, tile, lds_c4, lds_s4);

  // ---- 3. dkv = [dk's Dn columns | dv]
  if (p.kv) mlarope_dkv_stream<T>(p, tile);
}

template <typename T>
static void launch_t(const MlaRopeFreqParams& p, bool bwd, dim3 grid, hipStream_t stream) {
  const dim3 block(kMlaRopeThreads);
  if (bwd) {
    if (p.g.interleaved) hipLaunchKernelGGL((mlaropefreq_bwd_kernel<T, 1>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((mlaropefreq_bwd_kernel<T, 0>), grid, block, 0, stream, p);
  } else {
    if (p.g.interleaved) hipLaunchKernelGGL((mlaropefreq_fwd_kernel<T, 1>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((mlaropefreq_fwd_kernel<T, 0>), grid, block, 0, stream, p);
  }
}

static int launch(const MlaRopeFreqParams& p, int dtype, bool bwd, hipStream_t stream) {
  if (p.g.B == 0 || p.g.S == 0) return 0;
  const dim3 grid(p.g.B * rotfreq_tiles_per_batch(p.g.S, kMlaRopeRows));
  if (dtype == 0) launch_t<bf16_t>(p, bwd, grid, stream);
  else launch_t<f16_t>(p, bwd, grid, stream);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_mla_rotary_freqs_fwd(const MlaRopeFreqParams& p, int dtype, hipStream_t stream) { return launch(p, dtype, false, stream); }

int launch_mla_rotary_freqs_bwd(const MlaRopeFreqParams& p, int dtype, hipStream_t stream) { return launch(p, dtype, true, stream); }

}  // namespace rfa
