// rfa_mlarope_stream.hpp — the device code that the two MLA K / V assembly kernels share: rfa_mlarope.hip (cos / sin out of
// tables) and rfa_mlaropefreq.hip (angles formed in the kernel).  They differ in their preparation phase alone — how a tile's
// cos / sin reach LDS and how k_pe is rotated; everything behind it is here, once: the q stream, the k / v stream, the dkv stream
// and the two halves of the backward's head sum.  All of it reads the geometry, strides and pointers of MlaRopeParams and the
// LDS arrays its caller declares; rfa_mlarope_index.h has the arithmetic.
#ifndef RFA_MLAROPE_STREAM_HPP_
#define RFA_MLAROPE_STREAM_HPP_

#include "rfa_common.hpp"
#include "rfa_kernels.hpp"
#include "rfa_rotary_math.hpp"     // rot()

namespace rfa {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

enum { kMlaRopeLdsTab = kMlaRopeRows * (kMlaRopeMaxRot / 2) / 4 };      // quads of one cos (sin) array

// the q stream of a tile: q -> q_out (backward: dq_out -> dq), cos / sin out of LDS
template <typename T, int INTER>
__device__ __forceinline__ void mlarope_q_stream(const MlaRopeParams& p, const RotFreqTile& tile, const f32x4* lds_c4,
                                                 const f32x4* lds_s4) {
  const RotaryTensor t = p.tq;
  const T* src = (const T*)p.q;
  T* dst = (T*)p.q_out;
  const uint32_t half = p.g.Dr / 2;
  const uint32_t first = rotfreq_first_unit(p.gq, t, tile), n = rotfreq_tile_units(t, tile);
  for (uint32_t u = threadIdx.x; u < n; u += kMlaRopeThreads) {
    RotaryUnit x;
    rotary_unit(p.gq, t, first + u, &x);
    const vec8<T> a = *(const vec8<T>*)(src + x.s1);
    if (x.kind == kRotaryPass) {
      *(vec8<T>*)(dst + x.d1) = a;
      continue;
    }
    const uint32_t row = (x.i - tile.row0) * half;
    if (INTER == 0) {
      const vec8<T> b = *(const vec8<T>*)(src + x.s2);
      const uint32_t lo = row + rotfreq_lds_quad(half, 0, x.tcol, 0), hi = row + rotfreq_lds_quad(half, 0, x.tcol, 1);
      const f32x4 c0 = lds_c4[lo / 4], c1 = lds_c4[hi / 4], s0 = lds_s4[lo / 4], s1 = lds_s4[hi / 4];
      f32x8 o1, o2;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float y1, y2;
        rot((float)a[e], (float)b[e], e < 4 ? c0[e & 3] : c1[e & 3], e < 4 ? s0[e & 3] : s1[e & 3], y1, y2);
        o1[e] = y1;
        o2[e] = y2;
      }
      *(vec8<T>*)(dst + x.d1) = __builtin_convertvector(o1, vec8<T>);
      *(vec8<T>*)(dst + x.d2) = __builtin_convertvector(o2, vec8<T>);
    } else {
      const uint32_t at = row + rotfreq_lds_quad(half, 1, x.tcol, 0);
      const f32x4 c = lds_c4[at / 4], s = lds_s4[at / 4];
      f32x8 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float y1, y2;
        rot((float)a[2 * e], (float)a[2 * e + 1], c[e], s[e], y1, y2);
        o[2 * e] = y1;
        o[2 * e + 1] = y2;
      }
      *(vec8<T>*)(dst + x.d1) = __builtin_convertvector(o, vec8<T>);
    }
  }
}

// the k / v stream of a tile (forward): kv's Dn columns and lds_k's rotated k_pe row into k, kv's Dv columns into v
template <typename T>
__device__ __forceinline__ void mlarope_kv_stream(const MlaRopeParams& p, const RotFreqTile& tile, const vec8<T>* lds_k) {
  const T* kv = (const T*)p.kv;
  T* k = (T*)p.k;
  T* v = (T*)p.v;
  const uint32_t nch = p.g.Dr / 8;
  const uint32_t n = tile.nrows * p.g.H * mlarope_units_per_head(p.g, true);
  for (uint32_t u = threadIdx.x; u < n; u += kMlaRopeThreads) {
    const MlaRopeUnit x = mlarope_unit(p.g, true, u);
    const uint32_t i = tile.row0 + x.r;
    if (x.kind == kMlaRope) {
      *(vec8<T>*)(k + mlarope_off(p.k_st, tile.b, i, x.h, x.out_col)) = lds_k[x.r * nch + x.kv_col / 8];
    } else {
      const vec8<T> a = *(const vec8<T>*)(kv + mlarope_off(p.kv_st, tile.b, i, x.h, x.kv_col));
      T* dst = x.kind == kMlaNope ? k + mlarope_off(p.k_st, tile.b, i, x.h, x.out_col) : v + mlarope_off(p.v_st, tile.b, i, x.h, x.out_col);
      *(vec8<T>*)dst = a;
    }
  }
}

// the head sum of lane l of row r of the tile (backward): its heads' dk rope chunks, ascending, in fp32; the partial sums to LDS
template <typename T>
__device__ __forceinline__ void mlarope_head_sum(const MlaRopeParams& p, const RotFreqTile& tile, uint32_t r, uint32_t l, f32x4* lds_part) {
  const T* dk = (const T*)p.k;
  const uint32_t Dr = p.g.Dr;
  const MlaRopeLane lane = mlarope_red_lane(Dr, l);
  if (r < tile.nrows && lane.active) {
    f32x8 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const uint32_t ns = mlarope_red_slices(Dr);
    for (uint32_t h = lane.slice; h < p.g.H; h += ns) {
      const vec8<T> a = *(const vec8<T>*)(dk + mlarope_off(p.k_st, tile.b, tile.row0 + r, h, p.g.Dn + 8 * lane.chunk));
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += (float)a[e];
    }
    const uint32_t at = mlarope_red_slot(Dr, r, lane.slice, lane.chunk);
    lds_part[at / 4] = f32x4{acc[0], acc[1], acc[2], acc[3]};
    lds_part[at / 4 + 1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
  }
}

// the fold of rotation unit l of row r (backward, behind the barrier): the slices' partials, ascending; the rotation of the SUM by
// the unit's c / s (8 values; interleaved: the first 4; sin already negated); one rounding; dk_pe
template <typename T, int INTER>
__device__ __forceinline__ void mlarope_fold(const MlaRopeParams& p, const RotFreqTile& tile, uint32_t r, uint32_t l, const f32x4* lds_part,
                                             const float (&c)[8], const float (&s)[8]) {
  const uint32_t Dr = p.g.Dr, nch = Dr / 8;
  const uint32_t nfold = mlarope_red_fold(Dr, p.g.H);
  const uint32_t ca = l, cb = INTER ? l : l + nch / 2;   // the unit's chunk and (halves) its partner
  f32x8 a = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b = a;
  for (uint32_t sl = 0; sl < nfold; ++sl) {
    const uint32_t at = mlarope_red_slot(Dr, r, sl, ca);
    const f32x4 a0 = lds_part[at / 4], a1 = lds_part[at / 4 + 1];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] += a0[e];
      a[4 + e] += a1[e];
    }
    if (INTER == 0) {
      const uint32_t bt = mlarope_red_slot(Dr, r, sl, cb);
      const f32x4 b0 = lds_part[bt / 4], b1 = lds_part[bt / 4 + 1];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        b[e] += b0[e];
        b[4 + e] += b1[e];
      }
    }
  }
  T* dst = (T*)p.k_pe + mlarope_off(p.k_pe_st, tile.b, tile.row0 + r, 0, 0);
  if (INTER == 0) {
    f32x8 o1, o2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float y1, y2;
      rot(a[e], b[e], c[e], s[e], y1, y2);
      o1[e] = y1;
      o2[e] = y2;
    }
    *(vec8<T>*)(dst + 8 * ca) = __builtin_convertvector(o1, vec8<T>);
    *(vec8<T>*)(dst + 8 * cb) = __builtin_convertvector(o2, vec8<T>);
  } else {
    f32x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float y1, y2;
      rot(a[2 * e], a[2 * e + 1], c[e], s[e], y1, y2);
      o[2 * e] = y1;
      o[2 * e + 1] = y2;
    }
    *(vec8<T>*)(dst + 8 * ca) = __builtin_convertvector(o, vec8<T>);
  }
}

// the dkv stream of a tile (backward): dkv = [dk's Dn columns | dv]; a NULL dk or dv leaves its part alone
template <typename T>
__device__ __forceinline__ void mlarope_dkv_stream(const MlaRopeParams& p, const RotFreqTile& tile) {
  const T* dk = (const T*)p.k;
  const T* dv = (const T*)p.v;
  T* dkv = (T*)p.kv;
  const uint32_t n = tile.nrows * p.g.H * mlarope_units_per_head(p.g, false);
  for (uint32_t u = threadIdx.x; u < n; u += kMlaRopeThreads) {
    const MlaRopeUnit x = mlarope_unit(p.g, false, u);
    const uint32_t i = tile.row0 + x.r;
    const T* src = x.kind == kMlaNope ? dk : dv;
    if (!src) continue;
    const MlaRopeTensor& st = x.kind == kMlaNope ? p.k_st : p.v_st;
    *(vec8<T>*)(dkv + mlarope_off(p.kv_st, tile.b, i, x.h, x.kv_col)) = *(const vec8<T>*)(src + mlarope_off(st, tile.b, i, x.h, x.out_col));
  }
}

}  // namespace rfa
#endif  // RFA_MLAROPE_STREAM_HPP_
