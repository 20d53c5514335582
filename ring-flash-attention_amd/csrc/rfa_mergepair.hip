// rfa_mergepair.hip — the pairwise merge of two FINISHED attention results and its backward (gfx950).
//
// Attention over the union of two key sets A and B composes exactly from the two parts' (out, lse):
//     lse = logaddexp(lse_a, lse_b),   w_x = exp(lse_x - lse),   out = w_a out_a + w_b out_b              (merge_pair_kernel)
// — what the ring schedules do between their steps (merge_kernel, rfa_aux.hip), here as a public, differentiable operator on
// io-dtype tensors: fp32 arithmetic, out rounded ONCE.  With x = sum_d dout_d (out_a - out_b)_d its backward is
//     dout_a = w_a dout,  dout_b = w_b dout,  dlse_a = w_a dlse + w_a w_b x,  dlse_b = w_b dlse - w_a w_b x  (merge_pair_bwd_kernel)
// from the four forward inputs alone (the weights are recomputed; nothing else is saved).
// Empty rows: the package spells "no visible key" +inf (a direct forward) and -inf (an accumulate-mode forward); an infinite
// lse_x of either sign means side x is empty — weight 0, its values are never multiplied (so garbage or NaN in an empty side's
// out stays out of the result), all its gradients are 0.  Both empty: out = 0, lse = -inf.
// Both are streaming kernels in the style of merge_kernel: 16 lanes per (row, head), 16 bytes per lane and pass (two passes
// above 128 columns), vector loads and stores only, no LDS, no atomics; x is summed in a fixed order (per lane over its
// columns, then a fixed butterfly over the 16 lanes), so two runs give the same bits.
#include "rfa_common.hpp"
#include "rfa_kernels.hpp"

namespace rfa {

// (w_a, w_b, lse) of one row; ea / eb: side a / b is empty.  The larger side's weight is 1 / (1 + t), the smaller one's
// t / (1 + t), t = exp(-|lse_a - lse_b|): they sum to 1 and neither can overflow.
__device__ __forceinline__ void pair_weights(float la, float lb, bool& ea, bool& eb, float& wa, float& wb, float& l) {
  ea = la == INFINITY || la == -INFINITY;
  eb = lb == INFINITY || lb == -INFINITY;
  if (ea || eb) {
    wa = ea ? 0.f : 1.f;
    wb = eb ? 0.f : 1.f;
    l = ea ? (eb ? -INFINITY : lb) : la;
    return;
  }
  const float d = la - lb;
  const float t = expf(-fabsf(d));
  const float big = 1.f / (1.f + t), small = t * big;
  wa = d >= 0.f ? big : small;
  wb = d >= 0.f ? small : big;
  l = fmaxf(la, lb) + log1pf(t);
}

// ------------------------------------------------------------------------------------
// grid: x = ceil(S*H / 16) blocks of 256 threads (16 row-heads per block), y = B
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void merge_pair_kernel(const MergePairParams p) {
  const int b = blockIdx.y;
  const int64_t item = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  const int64_t row = item / p.H;
  const int h = (int)(item % p.H);
  if (row >= p.S) return;
  const float la = p.lse_a[(int64_t)b * p.lse_a_st.batch + (int64_t)h * p.lse_a_st.head + row];
  const float lb = p.lse_b[(int64_t)b * p.lse_b_st.batch + (int64_t)h * p.lse_b_st.head + row];
  bool ea, eb;
  float wa, wb, l;
  pair_weights(la, lb, ea, eb, wa, wb, l);
  typedef float f32x8 __attribute__((ext_vector_type(8)));
  for (int d = sub * 8; d < p.D; d += 128) {                 // (one pass for head dims <= 128)
    f32x8 x;
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = 0.f;
    if (!ea) {
      const vec8<T> v = *(const vec8<T>*)((const T*)p.out_a + (int64_t)b * p.out_a_st.batch + row * p.out_a_st.row +
                                          (int64_t)h * p.out_a_st.head + d);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = wa * (float)v[e];
    }
    if (!eb) {
      const vec8<T> v = *(const vec8<T>*)((const T*)p.out_b + (int64_t)b * p.out_b_st.batch + row * p.out_b_st.row +
                                          (int64_t)h * p.out_b_st.head + d);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] += wb * (float)v[e];
    }
    *(vec8<T>*)((T*)p.out + (int64_t)b * p.out_st.batch + row * p.out_st.row + (int64_t)h * p.out_st.head + d) =
        __builtin_convertvector(x, vec8<T>);
  }
  if (sub == 0) p.lse[(int64_t)b * p.lse_st.batch + (int64_t)h * p.lse_st.head + row] = l;
}

// ------------------------------------------------------------------------------------
// same grid.  Pass 1 reads the three rows (dout stays in registers: at most two 16-byte pieces per lane, head dims <= 256) and
// forms x; the second loop writes dout_a / dout_b.
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void merge_pair_bwd_kernel(const MergePairBwdParams p) {
  static_assert(kMaxHeadDim <= 256, "two 128-column passes per lane");
  const int b = blockIdx.y;
  const int64_t item = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  const int64_t row = item / p.H;
  const int h = (int)(item % p.H);
  if (row >= p.S) return;
  const float la = p.lse_a[(int64_t)b * p.lse_a_st.batch + (int64_t)h * p.lse_a_st.head + row];
  const float lb = p.lse_b[(int64_t)b * p.lse_b_st.batch + (int64_t)h * p.lse_b_st.head + row];
  bool ea, eb;
  float wa, wb, l;
  pair_weights(la, lb, ea, eb, wa, wb, l);
  const bool live = !ea && !eb;                              // (an empty side: w_a w_b = 0, x is not formed)
  const T* dop = (const T*)p.dout + (int64_t)b * p.dout_st.batch + row * p.dout_st.row + (int64_t)h * p.dout_st.head;
  const T* ap = (const T*)p.out_a + (int64_t)b * p.out_a_st.batch + row * p.out_a_st.row + (int64_t)h * p.out_a_st.head;
  const T* bp = (const T*)p.out_b + (int64_t)b * p.out_b_st.batch + row * p.out_b_st.row + (int64_t)h * p.out_b_st.head;
  vec8<T> dreg[2];
  float acc = 0.f;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int d = sub * 8 + it * 128;
    if (d < p.D) {
      dreg[it] = *(const vec8<T>*)(dop + d);
      if (live) {
        const vec8<T> va = *(const vec8<T>*)(ap + d);
        const vec8<T> vb = *(const vec8<T>*)(bp + d);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += (float)dreg[it][e] * ((float)va[e] - (float)vb[e]);
      }
    }
  }
#pragma unroll
  for (int s = 8; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 64);
  typedef float f32x8 __attribute__((ext_vector_type(8)));
  T* dap = (T*)p.dout_a + (int64_t)b * p.dout_a_st.batch + row * p.dout_a_st.row + (int64_t)h * p.dout_a_st.head;
  T* dbp = (T*)p.dout_b + (int64_t)b * p.dout_b_st.batch + row * p.dout_b_st.row + (int64_t)h * p.dout_b_st.head;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int d = sub * 8 + it * 128;
    if (d < p.D) {
      f32x8 xa, xb;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = (float)dreg[it][e];
        xa[e] = ea ? 0.f : wa * g;
        xb[e] = eb ? 0.f : wb * g;
      }
      *(vec8<T>*)(dap + d) = __builtin_convertvector(xa, vec8<T>);
      *(vec8<T>*)(dbp + d) = __builtin_convertvector(xb, vec8<T>);
    }
  }
  if (sub == 0) {
    const float g = p.dlse ? p.dlse[(int64_t)b * p.dlse_st.batch + (int64_t)h * p.dlse_st.head + row] : 0.f;
    const float cross = live ? wa * wb * acc : 0.f;
    p.dlse_a[(int64_t)b * p.dlse_a_st.batch + (int64_t)h * p.dlse_a_st.head + row] = ea ? 0.f : wa * g + cross;
    p.dlse_b[(int64_t)b * p.dlse_b_st.batch + (int64_t)h * p.dlse_b_st.head + row] = eb ? 0.f : wb * g - cross;
  }
}

// ------------------------------------------------------------------------------------
static inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

int launch_merge_pair(const MergePairParams& p, int dtype, hipStream_t stream) {
  const int64_t items = (int64_t)p.S * p.H;
  if (items <= 0 || p.B <= 0) return 0;
  dim3 grid((unsigned)((items + 15) / 16), (unsigned)p.B);
  if (dtype == 0) hipLaunchKernelGGL(merge_pair_kernel<bf16_t>, grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(merge_pair_kernel<f16_t>, grid, dim3(256), 0, stream, p);
  return ok();
}

int launch_merge_pair_bwd(const MergePairBwdParams& p, int dtype, hipStream_t stream) {
  const int64_t items = (int64_t)p.S * p.H;
  if (items <= 0 || p.B <= 0) return 0;
  dim3 grid((unsigned)((items + 15) / 16), (unsigned)p.B);
  if (dtype == 0) hipLaunchKernelGGL(merge_pair_bwd_kernel<bf16_t>, grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(merge_pair_bwd_kernel<f16_t>, grid, dim3(256), 0, stream, p);
  return ok();
}

}  // namespace rfa
