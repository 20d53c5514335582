// rfa_rotfreq.hip — rotary position embedding of q and k with the angles formed IN the kernel (gfx950; include/rfa.h:
// rfa_rotary_freqs; ring_flash_attn.apply_rotary_freqs).  The table kernel (rfa_rotary.hip) looks cos / sin up in (P, R/2)
// tables indexed by ONE global position per row: at a million tokens that is half a gigabyte per rank that no rank needs, and
// a row with several positions — multi-axis M-RoPE, where every frequency reads one of up to four axes (t, h, w) — has no
// table at all.  Here the call brings inv_freq (R/2 fp32 numbers) and the positions, and per rotated pair, in fp32,
//     ang = float(pos[axis(c)]) * inv_freq[c]      ONE rounded multiply, nothing fused into it (mul_rn: contraction off)
//     (s, c) = sincosf(ang)                        the precise function with its full range reduction: positions pass 10^6
//     c' = scaling * c,  s' = scaling * s          (conj: s' -> -s')
// and then rot() of rfa_rotary_math.hpp, each result rounded once to the io dtype.
//
// The split of the work is what makes this a kernel of its own.  One thread per unit, as the table kernel runs, would call
// sincosf 8 times for 16 elements and stop being memory-bound; but the angles of a row are shared by all H + Hk heads of q and
// k.  So a workgroup of 256 threads owns a TILE of kRotFreqRows rows of one batch entry (rfa_rotfreq_index.h):
//   1. angle phase   the nrows * R/2 entries (row, c) of the tile, strided over the threads: the position — the map's
//                    arithmetic, or one int32 of the axis that c reads — the angle, sincosf, scaling, conj; c' and s' go as
//                    fp32 into two LDS arrays [rows][R/2] (halves: quads permuted so that the stream phase reads without
//                    bank conflicts).  At the benchmark shape: 128 sincosf per 640 units instead of 8 per unit.
//   __syncthreads()
//   2. stream phase  the tile's units of q, then of k — one run of consecutive unit indices each, walked by the 256 threads
//                    and decoded by rotary_unit() itself: two 16-byte loads and two 16-byte stores per halves unit, one chunk
//                    of four pairs interleaved, pass-through chunks 16-byte copies out of place and untouched in place; the
//                    8 (4) c' / s' values are 16-byte LDS reads.
// No atomics, plain vector loads and stores, 64-bit global offsets.  An element's bits depend on its values, its position(s),
// inv_freq and the scaling alone: every (row, c) entry is computed by the same expression whichever thread gets it.
// grid: x = B * ceil(S / kRotFreqRows).  LDS: 2 * kRotFreqRows * 128 * 4 = 2 KiB, static.
#include "rfa_common.hpp"
#include "rfa_kernels.hpp"
#include "rfa_rotary_math.hpp"     // rot(), mul_rn()

namespace rfa {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

// VAR: measurement switches of tools/rotfreq_variants.hip — what the kernel costs WITHOUT one of its phases.  Every shipped
// instance has VAR == 0 and ROWS == kRotFreqRows; the switched-off code is dead there.  A variant's results are wrong on
// purpose (its addresses are the kernel's own).
enum {
  kRotFreqNoSincos = 1,      // angle phase without sincosf: position and inv_freq still loaded, two cheap ops in its place
  kRotFreqNoBarrier = 2,     // no __syncthreads() between the phases
  kRotFreqNoLdsRead = 4,     // stream phase takes c' / s' from a register instead of LDS
};

template <typename T, int INTER, int ROWS = kRotFreqRows, int VAR = 0>
__global__ __launch_bounds__(kRotFreqThreads) void rotfreq_kernel(const RotFreqParams p) {
  __shared__ f32x4 lds_c4[ROWS * kRotFreqMaxHalf / 4];      // written as floats, read as quads
  __shared__ f32x4 lds_s4[ROWS * kRotFreqMaxHalf / 4];
  float* lds_c = (float*)lds_c4;
  float* lds_s = (float*)lds_s4;
  const RotFreqTile tile = rotfreq_tile(p.g.S, blockIdx.x, ROWS);
  const uint32_t half = p.g.R / 2;

  // ---- 1. the angles of the tile's rows, once for all heads of q and k
  for (uint32_t e = threadIdx.x; e < tile.nrows * half; e += kRotFreqThreads) {
    const uint32_t r = e / half, c = e - r * half;
    const uint32_t i = tile.row0 + r;
    int64_t pos;
    if (p.positions) {
      const uint32_t axis = rotfreq_axis(p.freq_axis[0], p.freq_axis[1], p.freq_axis[2], p.freq_axis[3], c);
      pos = p.pos_off + (int64_t)p.positions[(int64_t)axis * p.pos_axis + (int64_t)tile.b * p.pos_batch + i];
    } else {
      pos = rotary_map_pos(p.pos_off, p.pos_stride, p.pos_split, p.pos_off2, i);
    }
    const float ang = mul_rn((float)pos, p.inv_freq[c]);
    float sn, cs;
    if (VAR & kRotFreqNoSincos) {
      cs = __builtin_fminf(__builtin_fabsf(ang), 0.8f);
      sn = __builtin_fminf(__builtin_fabsf(ang), 0.6f);
    } else {
      sincosf(ang, &sn, &cs);
    }
    cs = mul_rn(cs, p.scaling);
    sn = mul_rn(sn, p.scaling);
    const uint32_t at = r * half + rotfreq_lds_col(half, INTER, c);
    lds_c[at] = cs;
    lds_s[at] = p.conj ? -sn : sn;
  }
  if (!(VAR & kRotFreqNoBarrier)) __syncthreads();

  // ---- 2. the tile's units of every tensor
  for (int k = 0; k < p.ntensors; ++k) {
    const RotaryTensor t = p.t[k];
    const T* src = (const T*)p.src[k];
    T* dst = (T*)p.dst[k];
    const uint32_t first = rotfreq_first_unit(p.g, t, tile), n = rotfreq_tile_units(t, tile);
    for (uint32_t u = threadIdx.x; u < n; u += kRotFreqThreads) {
      RotaryUnit x;
      rotary_unit(p.g, t, first + u, &x);
      const vec8<T> a = *(const vec8<T>*)(src + x.s1);
      vec8<T> b = a;
      if (INTER == 0 && x.kind != kRotaryPass) b = *(const vec8<T>*)(src + x.s2);
      if (x.kind == kRotaryPass) {
        *(vec8<T>*)(dst + x.d1) = a;
        continue;
      }
      const uint32_t row = (x.i - tile.row0) * half;
      const f32x4 reg = {p.scaling, p.scaling, p.scaling, p.scaling};     // (kRotFreqNoLdsRead)
      if (INTER == 0) {
        const uint32_t lo = row + rotfreq_lds_quad(half, 0, x.tcol, 0), hi = row + rotfreq_lds_quad(half, 0, x.tcol, 1);
        const bool lds = !(VAR & kRotFreqNoLdsRead);
        const f32x4 c0 = lds ? lds_c4[lo / 4] : reg, c1 = lds ? lds_c4[hi / 4] : reg;
        const f32x4 s0 = lds ? lds_s4[lo / 4] : reg, s1 = lds ? lds_s4[hi / 4] : reg;
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
        const bool lds = !(VAR & kRotFreqNoLdsRead);
        const f32x4 c = lds ? lds_c4[at / 4] : reg, s = lds ? lds_s4[at / 4] : reg;
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
}

template <typename T>
static void launch_t(const RotFreqParams& p, dim3 grid, hipStream_t stream) {
  if (p.g.interleaved) hipLaunchKernelGGL((rotfreq_kernel<T, 1>), grid, dim3(kRotFreqThreads), 0, stream, p);
  else hipLaunchKernelGGL((rotfreq_kernel<T, 0>), grid, dim3(kRotFreqThreads), 0, stream, p);
}

int launch_rotary_freqs(const RotFreqParams& p, int dtype, hipStream_t stream) {
  if (p.g.B == 0 || p.g.S == 0) return 0;
  dim3 grid(p.g.B * rotfreq_tiles_per_batch(p.g.S));
  if (dtype == 0) launch_t<bf16_t>(p, grid, stream);
  else launch_t<f16_t>(p, grid, stream);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rfa
