// rfa_rotary.hip — rotary position embedding of q and k at GLOBAL positions (gfx950; include/rfa.h: rfa_rotary;
// ring_flash_attn.apply_rotary).  Under context parallelism the angle of local row i is its position in the unsharded
// sequence — two distant chunks on a zigzag rank, every W-th token on a stripe rank — which the call hands over either as the
// four numbers of a position map (the one the dropout hash uses: rfa.h q_pos_stride ...) or as an int32 tensor.  The eager
// composite is a gather of cos / sin, a rotate_half copy, two multiplies and an add over q and k; here q and k go through ONE
// launch, read once and written once.
//
// Pure streaming, in the style of seq_head_copy_kernel (rfa_seqhead.hip): one thread per unit (rfa_rotary_index.h) — two
// 16-byte loads, 8 cos and 8 sin values, two 16-byte stores (halves), or one chunk of 4 interleaved pairs; out of place the
// pass-through columns are 16-byte copies of the same launch, in place they are never touched.  No LDS, plain vector loads and
// stores, no atomics.  The 8 threads of a 128-wide head read two runs of 128 bytes — the two halves of the head's 256 bytes —
// so a wave's two loads together cover whole cache lines; the cos / sin row of a position (256 .. 512 bytes) is shared by all
// heads of the row and stays in L2.  The kernel holds a few dozen registers: occupancy is set by the 256-thread workgroups
// alone (8 waves per SIMD), which is what a memory-bound pass wants.
// Arithmetic: fp32, o1 = x1 c - x2 s, o2 = x2 c + x1 s (conj: s -> -s), written as ONE expression (rot) for every mode, each
// result rounded once to the io dtype: an element's bits depend on its values and its position alone.
// grid: x = ceil(max over tensors of nunits / 256), y = tensor of the call.
#include "rfa_common.hpp"
#include "rfa_kernels.hpp"
#include "rfa_rotary_math.hpp"     // rot(), load_tab(): shared with rfa_qknorm.hip

namespace rfa {

template <typename T, typename TT>
__global__ __launch_bounds__(256) void rotary_kernel(const RotaryParams p) {
  const RotaryTensor t = p.t[blockIdx.y];
  const uint32_t u = blockIdx.x * 256u + threadIdx.x;
  if (u >= t.nunits) return;
  RotaryUnit x;
  rotary_unit(p.g, t, u, &x);
  const T* src = (const T*)p.src[blockIdx.y];
  T* dst = (T*)p.dst[blockIdx.y];
  if (x.kind == kRotaryPass) {
    *(vec8<T>*)(dst + x.d1) = *(const vec8<T>*)(src + x.s1);
    return;
  }
  int64_t pos = p.positions ? p.pos_off + (int64_t)p.positions[(int64_t)x.b * p.pos_batch + x.i]
                            : rotary_map_pos(p.pos_off, p.pos_stride, p.pos_split, p.pos_off2, x.i);
  pos = rotary_clamp_pos(pos, p.P);                        // (never outside the tables, whatever `positions` holds)
  const int64_t trow = pos * (int64_t)(p.g.R / 2) + x.tcol;
  const TT* cp = (const TT*)p.cos + trow;
  const TT* sp = (const TT*)p.sin + trow;
  typedef float f32x8 __attribute__((ext_vector_type(8)));
  if (x.kind == kRotaryHalves) {
    float c[8], s[8];
    load_tab<TT, 8>(cp, c);
    load_tab<TT, 8>(sp, s);
    const vec8<T> a = *(const vec8<T>*)(src + x.s1);
    const vec8<T> b = *(const vec8<T>*)(src + x.s2);
    f32x8 o1, o2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float y1, y2;
      rot((float)a[e], (float)b[e], c[e], p.conj ? -s[e] : s[e], y1, y2);
      o1[e] = y1;
      o2[e] = y2;
    }
    *(vec8<T>*)(dst + x.d1) = __builtin_convertvector(o1, vec8<T>);
    *(vec8<T>*)(dst + x.d2) = __builtin_convertvector(o2, vec8<T>);
  } else {
    float c[4], s[4];
    load_tab<TT, 4>(cp, c);
    load_tab<TT, 4>(sp, s);
    const vec8<T> a = *(const vec8<T>*)(src + x.s1);
    f32x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float y1, y2;
      rot((float)a[2 * e], (float)a[2 * e + 1], c[e], p.conj ? -s[e] : s[e], y1, y2);
      o[2 * e] = y1;
      o[2 * e + 1] = y2;
    }
    *(vec8<T>*)(dst + x.d1) = __builtin_convertvector(o, vec8<T>);
  }
}

template <typename T>
static void launch_t(const RotaryParams& p, bool table_f32, dim3 grid, hipStream_t stream) {
  if (table_f32) hipLaunchKernelGGL((rotary_kernel<T, float>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((rotary_kernel<T, T>), grid, dim3(256), 0, stream, p);
}

int launch_rotary(const RotaryParams& p, int dtype, bool table_f32, hipStream_t stream) {
  uint32_t most = 0;
  for (int i = 0; i < p.ntensors; ++i) most = p.t[i].nunits > most ? p.t[i].nunits : most;
  if (most == 0) return 0;
  dim3 grid((most + 255u) / 256u, (unsigned)p.ntensors);
  if (dtype == 0) launch_t<bf16_t>(p, table_f32, grid, stream);
  else launch_t<f16_t>(p, table_f32, grid, stream);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rfa
