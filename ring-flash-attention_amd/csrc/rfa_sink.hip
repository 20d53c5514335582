// rfa_sink.hip — attention sinks (gfx950): one learnable logit per query head that joins the softmax as an extra column whose
// value vector is zero (GPT-OSS, the streaming-LLM family; flash_attn's / Hugging Face's `s_aux`).
//
// Nothing inside an attention kernel changes for it.  With (out, lse) of the attention WITHOUT the sink, merged over all blocks
// and ranks,
//     lse' = logaddexp(lse, sink_h),   out' = out * exp(lse - lse')                                       (sink_apply_kernel)
// and, because the sink column's value is zero (its dP is 0), the existing backward handed (out', lse') yields the exact
// dq / dk / dv.  The sink's own gradient is
//     dsink_h = - sum_rows exp(sink_h - lse'_row) * rowsum(dO * out')_row                                  (sink_grad_kernel)
// summed in a FIXED order: per 16-lane group over its rows, over the 16 groups of a workgroup, then over the workgroups by
// sink_grad_finish_kernel — no float atomics, two runs give the same bits.
// Both are one-pass streaming kernels in the style of merge_kernel (rfa_aux.hip): 16 lanes per (row, head), 16 bytes per lane
// and pass (two passes above 128 columns), vector loads and stores only.
#include "rfa_common.hpp"
#include "rfa_kernels.hpp"

namespace rfa {

// ------------------------------------------------------------------------------------
// grid: x = ceil(S*H / 16) blocks of 256 threads (16 row-heads per block), y = B
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void sink_apply_kernel(const SinkApplyParams p) {
  const int b = blockIdx.y;
  const int64_t item = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  const int64_t row = item / p.H;
  const int h = (int)(item % p.H);
  if (row >= p.S) return;
  const float l = p.lse_src[(int64_t)b * p.lse_src_batch + (int64_t)h * p.lse_src_head + row];
  const float s = p.sinks[h];
  float w, lnew;
  if (l == INFINITY || l == -INFINITY) {
    // a row without a visible key (public lse = +inf, out = 0): the sink is the only column
    w = 0.f; lnew = s;
  } else {
    // a sink so low that exp(d) underflows returns the input bits: w == 1.0f, log1p(0) == 0
    const float d = s - l;
    w = 1.f / (1.f + expf(d));
    lnew = fmaxf(l, s) + log1pf(expf(-fabsf(d)));
  }
  typedef float f32x8 __attribute__((ext_vector_type(8)));
  for (int d = sub * 8; d < p.D; d += 128) {                 // (one pass for head dims <= 128)
    const vec8<T> v = *(const vec8<T>*)((const T*)p.out_src + (int64_t)b * p.out_src_st.batch + row * p.out_src_st.row +
                                        (int64_t)h * p.out_src_st.head + d);
    f32x8 x;
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (float)v[e] * w;
    // (out_dst may be out_src: this lane has read the 16 bytes it overwrites)
    *(vec8<T>*)((T*)p.out_dst + (int64_t)b * p.out_dst_st.batch + row * p.out_dst_st.row + (int64_t)h * p.out_dst_st.head + d) =
        __builtin_convertvector(x, vec8<T>);
  }
  if (sub == 0) p.lse_dst[(int64_t)b * p.lse_dst_batch + (int64_t)h * p.lse_dst_head + row] = lnew;
}

// ------------------------------------------------------------------------------------
// grid: x = ceil(S / kSinkGradRows) row chunks, y = H, z = B; 256 threads = 16 groups of 16 lanes, group g takes rows
// r0 + g, r0 + g + 16, ... of its chunk.  partial[(b * gridDim.x + chunk) * H + h] = the chunk's sum for head h.
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void sink_grad_kernel(const SinkGradParams p) {
  __shared__ float part[16];
  const int b = blockIdx.z, h = blockIdx.y;
  const int g = threadIdx.x >> 4, sub = threadIdx.x & 15;
  const int64_t r0 = (int64_t)blockIdx.x * kSinkGradRows;
  const float s = p.sinks[h];
  const T* dop = (const T*)p.dout + (int64_t)b * p.dout_st.batch + (int64_t)h * p.dout_st.head;
  const T* op = (const T*)p.out + (int64_t)b * p.out_st.batch + (int64_t)h * p.out_st.head;
  const float* lp = p.lse + (int64_t)b * p.lse_batch + (int64_t)h * p.lse_head;
  float sum = 0.f;
  for (int i = g; i < kSinkGradRows; i += 16) {
    const int64_t row = r0 + i;
    if (row >= p.S) break;
    float acc = 0.f;
    for (int d = sub * 8; d < p.D; d += 128) {               // (one pass for head dims <= 128)
      const vec8<T> a = *(const vec8<T>*)(dop + row * p.dout_st.row + d);
      const vec8<T> o = *(const vec8<T>*)(op + row * p.out_st.row + d);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc += (float)a[e] * (float)o[e];
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    const float l = lp[row];
    // (a saved lse' is finite — it is at least the sink; an infinite one marks a row that carries nothing)
    sum += (l == INFINITY || l == -INFINITY) ? 0.f : -expf(s - l) * acc;
  }
  if (sub == 0) part[g] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += part[i];
    p.partial[((int64_t)b * gridDim.x + blockIdx.x) * p.H + h] = t;
  }
}

// dsink[h] = sum of the nparts partials of head h: one wave per head, lane l adds partials l, l + 64, ... in index order,
// then the 64 lane sums are added by a fixed butterfly.  nparts == 0 writes zeros.  grid: x = ceil(H / 4), 256 threads
__global__ __launch_bounds__(256) void sink_grad_finish_kernel(float* dsink, const float* partial, int64_t nparts, int H) {
  const int h = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (h >= H) return;
  float t = 0.f;
  for (int64_t i = lane; i < nparts; i += 64) t += partial[i * H + h];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
  if (lane == 0) dsink[h] = t;
}

// ------------------------------------------------------------------------------------
static inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

int launch_sink_apply(const SinkApplyParams& p, int dtype, hipStream_t stream) {
  const int64_t items = (int64_t)p.S * p.H;
  if (items <= 0 || p.B <= 0) return 0;
  dim3 grid((unsigned)((items + 15) / 16), (unsigned)p.B);
  if (dtype == 0) hipLaunchKernelGGL(sink_apply_kernel<bf16_t>, grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(sink_apply_kernel<f16_t>, grid, dim3(256), 0, stream, p);
  return ok();
}

int64_t sink_grad_parts(int B, int S) {
  return B <= 0 || S <= 0 ? 0 : (int64_t)B * ((S + kSinkGradRows - 1) / kSinkGradRows);
}

int launch_sink_grad(const SinkGradParams& p, int dtype, hipStream_t stream) {
  if (p.H <= 0) return 0;
  const int64_t nparts = sink_grad_parts(p.B, p.S);
  if (nparts > 0) {
    dim3 grid((unsigned)((p.S + kSinkGradRows - 1) / kSinkGradRows), (unsigned)p.H, (unsigned)p.B);
    if (dtype == 0) hipLaunchKernelGGL(sink_grad_kernel<bf16_t>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(sink_grad_kernel<f16_t>, grid, dim3(256), 0, stream, p);
    if (ok()) return -1;
  }
  hipLaunchKernelGGL(sink_grad_finish_kernel, dim3((unsigned)((p.H + 3) / 4)), dim3(256), 0, stream, p.dsink, p.partial,
                     nparts, p.H);
  return ok();
}

}  // namespace rfa
