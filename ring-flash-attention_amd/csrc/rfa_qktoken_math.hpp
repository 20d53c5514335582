// rfa_qktoken_math.hpp — what the two token-wide QK RMSNorm + rotary kernel families share (rfa_qktoken.hip: cos / sin from
// tables; rfa_qktokenfreq.hip: angles formed in the kernel): the row sums' three stages, rstd, the scale, the rotation of a
// chunk and the hand-over of a workgroup's weight gradient partial.  ONE set of device functions, so that a row's rstd, a
// rotated pair and a dw partial have the same bits whichever kernel computes them.  Ownership (which lane holds which chunk)
// is rfa_qktoken_index.h's; the SUMMATION ORDERS these functions fix are stated in the two sources' headers.
#ifndef RFA_QKTOKEN_MATH_HPP_
#define RFA_QKTOKEN_MATH_HPP_

#include "rfa_common.hpp"
#include "rfa_kernels.hpp"
#include "rfa_rotary_math.hpp"

namespace rfa {
namespace qktoken_math {

enum { kTokNone = 0, kTokHalves = 1, kTokInterleaved = 2 };
constexpr uint32_t kStageBytes = 32768;       // 16 B x (4 rows x 128 | 2 rows x 512 | 1 row x 2048) chunks
constexpr uint32_t kTabFloats = 128;          // R / 2 <= 128
constexpr uint32_t kMaxSlots = 4;

typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ void widen(const vec8<T>& v, float (&f)[8]) {
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

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the team's sum of the per-wave sums in `red` (written in front of the last barrier), in wave order
__device__ __forceinline__ float team_total(const float* red, uint32_t team, uint32_t wave) {
  const uint32_t nw = team >> 6, fw = wave & ~(nw - 1);
  float total = red[fw];
  for (uint32_t j = 1; j < nw; ++j) total += red[fw + j];
  return total;
}

__device__ __forceinline__ float row_rstd(float ss, uint32_t N, float eps) { return rsqrtf(ss / (float)N + eps); }

// a_c = weight_offset + w_c of the 8 columns of chunk c
template <typename T>
__device__ __forceinline__ void load_scale(const QkTokenParams& p, const void* weight, uint32_t c, float (&a)[8]) {
  if (p.weight_f32) {
    float lo[4], hi[4];
    load_tab<float, 4>((const float*)weight + 8 * (size_t)c, lo);
    load_tab<float, 4>((const float*)weight + 8 * (size_t)c + 4, hi);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = p.weight_offset + lo[e];
      a[4 + e] = p.weight_offset + hi[e];
    }
  } else {
    float w[8];
    load_tab<T, 8>((const T*)weight + 8 * (size_t)c, w);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = p.weight_offset + w[e];
  }
}

// a wave-uniform 64-bit value held in vector registers.  The backward keeps more uniform values live across its walk than there
// are scalar registers; strides and position offsets only ever enter per-lane (vector) arithmetic, so they live there
__device__ __forceinline__ int64_t in_vgpr(int64_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ uint32_t in_vgpr(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

// the chunk's 8 columns after the rotation (CONJ: the inverse one); v the chunk's values, pv its partner's (halves only)
template <int MODE, bool CONJ>
__device__ __forceinline__ void rotate8(const float (&v)[8], const float (&pv)[8], float (&o)[8], int kind, const float* c,
                                        const float* s) {
  if constexpr (MODE == kTokHalves) {
    const bool lo = kind == kQkTokenLo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float o1, o2;
      rot(lo ? v[e] : pv[e], lo ? pv[e] : v[e], c[e], CONJ ? -s[e] : s[e], o1, o2);
      o[e] = lo ? o1 : o2;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) rot(v[2 * e], v[2 * e + 1], c[e], CONJ ? -s[e] : s[e], o[2 * e], o[2 * e + 1]);
  }
}

// lane tl's j-th chunk, tl + j * team, exists: a uniform test for all j but one (every lane has its first chunks / team ones)
__device__ __forceinline__ bool has_chunk(uint32_t j, uint32_t tl, uint32_t jfull, uint32_t tail) {
  return j < jfull || (j == jfull && tl < tail);
}

// (head << 16 | first column) and (kind << 16 | table column) of the lane's chunks: functions of the chunk alone
template <int K>
__device__ __forceinline__ void lane_roles(const QkTokenGeom& g, const QkTokenTensor& t, uint32_t tl, uint32_t (&hc)[K],
                                           uint32_t (&kt)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t c = tl + j * t.team;
    QkTokenRole r{};
    r.kind = kQkTokenPass;
    if (c < t.chunks) qktoken_role(g, c, &r);
    hc[j] = r.head << 16 | r.col;
    kt[j] = (uint32_t)r.kind << 16 | r.tcol;
  }
}

// the end of a backward workgroup: its teams' weight gradient sums `acc`, added in slot order — slots 1 .. hand theirs over
// through LDS (`hand`: (slots - 1) N floats <= 16 KiB, the staging area, whose last reads are done behind the first barrier) —
// and stored as ONE fp32 (N,) partial where qktoken_fold_kernel looks for it
template <int K>
__device__ __forceinline__ void store_dw_partial(const QkTokenParams& p, int k, uint32_t N, float* hand, float (&acc)[K][8],
                                                 uint32_t slots, uint32_t slot, uint32_t tl, uint32_t teamv, uint32_t jfull,
                                                 uint32_t tail) {
  if (slots > 1) {
    __syncthreads();                                             // (the last step's reads of `stage` are done)
    if (slot > 0) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const uint32_t c = tl + j * teamv;
        if (!has_chunk(j, tl, jfull, tail)) continue;
#pragma unroll
        for (int e = 0; e < 8; ++e) hand[(size_t)(slot - 1) * N + 8 * c + e] = acc[j][e];
      }
    }
    __syncthreads();
  }
  if (slot > 0) return;
  float* part = p.workspace + (k ? (size_t)p.nparts[0] * p.t[0].N : (size_t)0) + (size_t)blockIdx.x * N;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t c = tl + j * teamv;
    if (!has_chunk(j, tl, jfull, tail)) continue;
    for (uint32_t s = 1; s < slots; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[j][e] += hand[(size_t)(s - 1) * N + 8 * c + e];
    f32x4 lo, hi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lo[e] = acc[j][e];
      hi[e] = acc[j][4 + e];
    }
    *(f32x4*)(part + 8 * c) = lo;
    *(f32x4*)(part + 8 * c + 4) = hi;
  }
}

}  // namespace qktoken_math
}  // namespace rfa
#endif  // RFA_QKTOKEN_MATH_HPP_
