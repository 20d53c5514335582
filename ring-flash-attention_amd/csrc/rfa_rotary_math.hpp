// rfa_rotary_math.hpp — the arithmetic that rfa_rotary.hip and rfa_qknorm.hip share: ONE expression for a rotated pair and the
// load of a run of cos / sin values, so that a pair rotated behind the QK norm has the bits the plain rotation gives it.
#ifndef RFA_ROTARY_MATH_HPP_
#define RFA_ROTARY_MATH_HPP_

namespace rfa {

// (o1, o2) of one pair; the product that is subtracted / added is rounded to fp32 first, the other one is fused
__device__ __forceinline__ void rot(float x1, float x2, float c, float s, float& o1, float& o2) {
  o1 = __builtin_fmaf(x1, c, -(x2 * s));
  o2 = __builtin_fmaf(x2, c, x1 * s);
}

// N consecutive values of a cos / sin row as fp32 (N * sizeof(TT) bytes, aligned to that)
template <typename TT, int N>
__device__ __forceinline__ void load_tab(const TT* p, float (&f)[N]) {
  typedef TT vecn __attribute__((ext_vector_type(N)));
  const vecn v = *(const vecn*)p;
#pragma unroll
  for (int e = 0; e < N; ++e) f[e] = (float)v[e];
}

}  // namespace rfa
#endif  // RFA_ROTARY_MATH_HPP_
