// rfa_maxlogit.hip — per-head max attention logit for gfx950 (MI355X): the largest softmax_scale * q.k over the (query, key)
// pairs the attention looks at (QK-Clip / MuonClip; Transformer Engine's and Megatron's `max_logit`).  include/rfa.h:
// rfa_max_logit.
//
// It is the forward kernel's S phase with nothing behind it (rfa_fwd.hip): one workgroup = 8 waves = 256 query rows of one
// head, a wave owns 32 rows whose Q fragments stay in registers; K tiles of 64 keys go global -> LDS (LDS-DMA for a full
// 128- / 64-wide row, through registers with zeroed chunks otherwise), double buffered, one barrier per tile, swizzled as
// everywhere (rfa_common.hpp); S^T = K Q^T on v_mfma_f32_32x32x16, one ds_read_b128 per MFMA.  No V, no softmax, no O: a lane
// keeps ONE running max over the scores it sees.  Head dims 136 .. 256 run two 128-column parts of the K tile into the same
// S accumulators.
//   * band: the forward's (rfa_maxlogit_band.h).  A wave skips tiles none of its rows sees; a tile wholly inside the band
//     takes the bare max, only edge tiles (the diagonal, the window's left edge, the last tile's keys behind lk) pay
//     per-element predicates.  Keys behind lk read as ZERO and are masked, or an all-negative head would report 0; lanes of
//     rows behind lq compute on a clamped copy of row lq - 1 and are dropped before the reduction.
//   * reduction: lane -> wave (butterfly) -> workgroup (LDS) -> one float per workgroup in the workspace; EVERY workgroup
//     writes its slot, the early exits (beyond lq, an empty tile range, a dark sequence of a packed batch) write -inf.
//     maxlogit_finish_kernel folds a head's slots in index order, multiplies by softmax_scale once (fp32; the scale is
//     positive, so it commutes with the max) and writes or max-accumulates dst[h].  No atomics: two runs give the same bits,
//     and a block cut into block calls gives the bits of the uncut call (every pair's dot product is the same chain of MFMAs
//     wherever its tile lies).
//   * NaN: the hardware max returns its other operand, so NaN scores are ignored.
#include <type_traits>

#include "rfa_common.hpp"
#include "rfa_kernels.hpp"
#include "rfa_maxlogit_band.h"

namespace rfa {

static_assert(kMlKV <= kDescMaxRows, "a buffer descriptor spans at most kDescMaxRows rows (rfa_kernels.hpp)");

// kD: compiled head dim — 64, 128, or 256 = two 128-column parts
template <int kD>
struct MlGeo {
  static_assert(kD == 64 || kD == 128 || kD == 256, "compiled head dims");
  static constexpr int kParts = kD == 256 ? 2 : 1;
  static constexpr int kDl = kD == 256 ? 128 : kD;            // width of one part = of the LDS layout
  typedef HeadGeo<kDl> Geo;
  static constexpr int kTileBytes = kMlKV * Geo::kRowBytes;   // one part of a K tile: 16 KiB (8 KiB at 64)
  static constexpr int kStageBytes = kParts * kTileBytes;
  static constexpr int kSmem = 2 * kStageBytes;               // two stages
};

// kFullD: D == kD (LDS-DMA staging); otherwise D < kD, zero padded through the register staging path
template <typename T, int kD, bool kFullD>
__global__ __launch_bounds__(kMlWaves * 64, 2) void maxlogit_kernel(const MaxLogitParams p) {
  typedef MlGeo<kD> M;
  typedef typename M::Geo Geo;
  constexpr int kDl = M::kDl, kParts = M::kParts;
  constexpr int kRowBytes = Geo::kRowBytes;
  constexpr int kNKp = Geo::kKSteps;                          // 16-wide k-steps per part
  constexpr int kNK = kParts * kNKp;
  constexpr int kTileBytes = M::kTileBytes, kStageBytes = M::kStageBytes;
  constexpr int kThreads = kMlWaves * 64;
  constexpr int kShare = kTileBytes / 1024 / kMlWaves;        // 1 KiB pieces (4 physical rows) per wave and part
  constexpr int kChunks = Geo::kLay / 8;                      // 16-byte chunks per logical row
  constexpr int kSub = kMlKV / 32;                            // 32-key sub-tiles per tile
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  lds_t* smem = (lds_t*)smem_raw;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 5;
  const int l31 = lane & 31;

  // ---- work decode: kv-head fastest (workgroups sharing K sit together), batch slowest; heavy causal blocks first
  int idx = blockIdx.x;
  const int G = p.H / p.Hk;
  const int hk = idx % p.Hk;
  idx /= p.Hk;
  const int gq = idx % G;
  idx /= G;
  const int qblk_i = idx % p.nqblk, b = idx / p.nqblk;
  const int qblk = p.nqblk - 1 - qblk_i;
  const int h = hk * G + gq;
  float* slot = p.partial + (int64_t)h * ((int64_t)p.B * p.nqblk) + idx;

  const SeqSpan qs = resolve_span(p.cu_q, b, p.Sq, p.q_half);
  const SeqSpan ks = resolve_span(p.cu_k, b, p.Sk, p.k_half);
  const int lq = qs.len, lk = ks.len;
  const int qwg0 = qblk * kMlQRows;
  // the early exits are workgroup-uniform and lie in front of the first barrier; each leaves -inf in the slot
  if (qwg0 >= lq || lk <= 0) {
    if (tid == 0) *slot = -INFINITY;
    return;
  }
  const MlBand band{ml_off(lq, lk, p.shift, p.shift_lens), p.wl, p.wr};
  const int qend = qwg0 + kMlQRows < lq ? qwg0 + kMlQRows : lq;
  int jt0, ntiles;
  ml_tile_range(qwg0, qend, lk, band, jt0, ntiles);
  if (jt0 >= ntiles) {
    if (tid == 0) *slot = -INFINITY;
    return;
  }
  const int qw0 = qwg0 + wave * kMlWaveRows;
  const int qrow = qw0 + l31;
  const int qrow_c = qrow < lq ? qrow : lq - 1;
  int klo, khi;                                               // this lane's visible keys (edge tiles)
  ml_row_keys(qrow_c, lk, band, klo, khi);

  const int64_t qbatch = p.cu_q ? 0 : (int64_t)b;
  const int64_t kbatch = p.cu_k ? 0 : (int64_t)b;
  const T* qbase = (const T*)p.q + qbatch * p.q_st.batch + (qs.row0 + qrow_c) * p.q_st.row + (int64_t)h * p.q_st.head;
  const T* kbase = (const T*)p.k + kbatch * p.k_st.batch + ks.row0 * p.k_st.row + (int64_t)hk * p.k_st.head;

  // ---- Q fragment (B operand of S^T = K Q^T): lane (q = l31, g) holds d = 16 kk + 8 g .. + 7
  vec8<T> qf[kNK];
#pragma unroll
  for (int kk = 0; kk < kNK; ++kk) {
    const int d0 = 16 * kk + 8 * g;
    qf[kk] = (kFullD || d0 < p.D) ? *(const vec8<T>*)(qbase + d0) : zero8<T>();
  }

  // ---- K tile staging (as rfa_fwd.hip): fixed per-thread byte offsets, the tile advance in the descriptor's base, rows
  // behind the sequence's end read as zero
  constexpr bool kDma = kFullD;
  constexpr int kRowsPerPass = kThreads / kChunks;
  const int sc = tid % kChunks;
  const int sr = tid / kChunks;
  vec8<T> kreg[kParts][kShare];
  int voff_k[kShare];
#pragma unroll
  for (int i = 0; i < kShare; ++i) {
    int row = sr + kRowsPerPass * i, chunk = sc;
    if (kDma) dma_lane_src<kDl>(wave + kMlWaves * i, lane, row, chunk);
    voff_k[i] = (row * (int)p.k_st.row + chunk * 8) * 2;
  }
  const int64_t k_tile_e = (int64_t)kMlKV * p.k_st.row;
  const T* ld_k = kbase + jt0 * k_tile_e;
  auto load_tile = [&](int j, auto stage) {
    constexpr int kStage = decltype(stage)::value;
    int rows = lk - j * kMlKV;
    rows = rows < kMlKV ? rows : kMlKV;
    const T* kt = ld_k;
    ld_k += k_tile_e;
#pragma unroll
    for (int part = 0; part < kParts; ++part) {
      int cols = p.D - kDl * part;                            // columns of this part that exist (>= 8)
      cols = cols < kDl ? cols : kDl;
      const int nk = rows > 0 ? ((rows - 1) * (int)p.k_st.row + cols) * 2 : 0;
      const T* base = kt + kDl * part;
      if (kDma) {
        const dma_rsrc_t rk = make_dma_rsrc(base, nk);
#pragma unroll
        for (int i = 0; i < kShare; ++i)
          dma_load128(rk, lds_addr(smem) + kStage * kStageBytes + part * kTileBytes + (wave + kMlWaves * i) * 1024, voff_k[i]);
      } else {
        const buf_rsrc_t rk = make_rsrc(base, nk);
        const bool sd_ok = sc * 8 < cols;
#pragma unroll
        for (int i = 0; i < kShare; ++i) {
          kreg[part][i] = buffer_load128<T>(rk, voff_k[i]);
          if (!sd_ok) kreg[part][i] = zero8<T>();
        }
      }
    }
  };
  auto write_tile = [&](auto stage) {
    constexpr int kStage = decltype(stage)::value;
    if (!kDma) {
#pragma unroll
      for (int part = 0; part < kParts; ++part)
#pragma unroll
        for (int i = 0; i < kShare; ++i)
          lds_write128<T>(smem + kStage * kStageBytes + part * kTileBytes + tile_off_d<kDl>(sr + kRowsPerPass * i, sc),
                          kreg[part][i]);
    }
  };

  // K fragment (A operand): row = 32 t + l31, chunk = 2 kk + g of its part
  int koff[kNKp];
#pragma unroll
  for (int kk = 0; kk < kNKp; ++kk) {
    koff[kk] = lds_addr(smem) + tile_off_d<kDl>(l31, 2 * kk + g);
    pin_vgpr(koff[kk]);
  }

  float m = -INFINITY;

  // the prologue is unconditional and every earlier global load has landed when the loop starts (rfa_fwd.hip)
  load_tile(jt0, std::integral_constant<int, 0>{});
  write_tile(std::integral_constant<int, 0>{});
  wait_all_vmem();
  __syncthreads();

  auto tile_step = [&](int j, auto stage) {
    constexpr int kStage = decltype(stage)::value;
    typedef std::integral_constant<int, 1 - kStage> next_t;
    const bool more = j + 1 < ntiles;
    if (more) load_tile(j + 1, next_t{});

    const int cls = __builtin_amdgcn_readfirstlane(ml_tile_class(qw0, lq, lk, band, j));
    if (cls != kMlSkip) {
      f32x16 s[kSub];
#pragma unroll
      for (int t = 0; t < kSub; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
      {
        constexpr int kAhead = 6;                             // K fragments read ahead of their MFMA (the forward's value)
        constexpr int kN = kSub * kNK;
        vec8<T> a[kN];
        auto fa = [&](int i) {
          const int kk = i % kNK;
          return lds_read128<T>(lds_ptr(koff[kk % kNKp]) + kStage * kStageBytes + (kk / kNKp) * kTileBytes +
                                (i / kNK) * 32 * kRowBytes);
        };
#pragma unroll
        for (int i = 0; i < kAhead; ++i) a[i] = fa(i);
#pragma unroll
        for (int i = 0; i < kN; ++i) {
          if (i + kAhead < kN) a[i + kAhead] = fa(i + kAhead);
          s[i / kNK] = mfma(a[i], qf[i % kNK], s[i / kNK]);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, kAhead, 0);
#pragma unroll
        for (int i = 0; i < kN - kAhead; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, kAhead, 0);
      }
      if (cls == kMlEdge) {
        const int kt0 = j * kMlKV;
#pragma unroll
        for (int t = 0; t < kSub; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kt0 + 32 * t + crow(r, g);
            if (key > khi || key < klo) s[t][r] = -INFINITY;
          }
      }
      // (pairs of scores against the running max: v_max3_f32)
#pragma unroll
      for (int t = 0; t < kSub; ++t)
#pragma unroll
        for (int r = 0; r < 16; r += 2) m = fmaxf(fmaxf(m, s[t][r]), s[t][r + 1]);
    }
    if (!kDma && more) write_tile(next_t{});
    if (kDma) wait_all_vmem();                                // tile j + 1 has landed before the barrier publishes it
    __syncthreads();
  };
  for (int j = jt0; j < ntiles; j += 2) {
    tile_step(j, std::integral_constant<int, 0>{});
    if (j + 1 < ntiles) tile_step(j + 1, std::integral_constant<int, 1>{});
  }

  // ---- lane -> wave -> workgroup.  Behind the loop's last barrier no wave reads a tile any more: the LDS is free.
  if (qrow >= lq) m = -INFINITY;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float* red = (float*)smem_raw;
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (tid == 0) {
    float t = red[0];
#pragma unroll
    for (int w = 1; w < kMlWaves; ++w) t = fmaxf(t, red[w]);
    *slot = t;
  }
}

// dst[h] = (accumulate ? max(dst[h], x) : x),  x = scale * max over the nparts slots of head h, in index order: one wave per
// head, lane l folds slots l, l + 64, ..., then a fixed butterfly.  nparts == 0: x = -inf.  grid: x = ceil(H / 4), 256 threads
__global__ __launch_bounds__(256) void maxlogit_finish_kernel(float* dst, const float* partial, int64_t nparts, int H,
                                                              float scale, int accumulate) {
  const int h = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (h >= H) return;
  float t = -INFINITY;
  for (int64_t i = lane; i < nparts; i += 64) t = fmaxf(t, partial[(int64_t)h * nparts + i]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) t = fmaxf(t, __shfl_xor(t, o, 64));
  if (lane == 0) {
    t *= scale;
    dst[h] = accumulate ? fmaxf(dst[h], t) : t;
  }
}

// ------------------------------------------------------------------------------------
template <typename T, int kD, bool kFullD>
static int launch_ml_i(const MaxLogitParams& p, int64_t nblocks, hipStream_t stream) {
  static std::atomic<unsigned long long> attr_done{0};
  if (int rc = opt_in_dynamic_lds((const void*)maxlogit_kernel<T, kD, kFullD>, MlGeo<kD>::kSmem, attr_done)) return rc;
  hipLaunchKernelGGL((maxlogit_kernel<T, kD, kFullD>), dim3((unsigned)nblocks), dim3(kMlWaves * 64), MlGeo<kD>::kSmem, stream, p);
  return hipGetLastError() == hipSuccess ? kLaunchOk : kLaunchFailed;
}

template <typename T>
static int launch_ml_t(const MaxLogitParams& p, int64_t nblocks, hipStream_t stream) {
  if (p.D == 64) return launch_ml_i<T, 64, true>(p, nblocks, stream);
  if (p.D < 64) return launch_ml_i<T, 64, false>(p, nblocks, stream);
  if (p.D == 128) return launch_ml_i<T, 128, true>(p, nblocks, stream);
  if (p.D < 128) return launch_ml_i<T, 128, false>(p, nblocks, stream);
  if (p.D == 256) return launch_ml_i<T, 256, true>(p, nblocks, stream);
  return launch_ml_i<T, 256, false>(p, nblocks, stream);
}

// attention = false: the call's band is empty — only the finish kernel runs, on no slots
int launch_max_logit(const MaxLogitParams& p, int dtype, bool attention, hipStream_t stream) {
  const int64_t nparts = attention ? (int64_t)p.B * p.nqblk : 0;
  if (nparts > 0) {
    const int rc = dtype == 0 ? launch_ml_t<bf16_t>(p, nparts * p.H, stream) : launch_ml_t<f16_t>(p, nparts * p.H, stream);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(maxlogit_finish_kernel, dim3((unsigned)((p.H + 3) / 4)), dim3(256), 0, stream, p.dst, p.partial, nparts,
                     p.H, p.scale, p.accumulate);
  return hipGetLastError() == hipSuccess ? kLaunchOk : kLaunchFailed;
}

}  // namespace rfa
