// rfa_qknorm_math.hpp — the arithmetic that rfa_qknorm.hip and rfa_qknormfreq.hip share: ONE function for the row statistic of a
// lane group and one for the scale, the load and the store of a lane's 8 columns, so that a (row, head) normalised in front of
// angles formed in the kernel has the bits the table kernel gives it.
#ifndef RFA_QKNORM_MATH_HPP_
#define RFA_QKNORM_MATH_HPP_

#include "rfa_common.hpp"
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

}  // namespace rfa
#endif  // RFA_QKNORM_MATH_HPP_
