// rfa_qktokenfreq.hip — RMSNorm of q and k over ALL heads of a token, fused with a rotary embedding whose angles are formed IN the
// kernel, one to four position axes per row (gfx950; include/rfa.h: rfa_qk_token_norm_rotary_freqs_fwd / _bwd;
// ring_flash_attn.apply_qk_token_norm_rotary_freqs).  OLMo-2 / OLMo-3 under context parallelism would otherwise hold cos / sin
// tables of the whole unsharded sequence on every rank, or run the token norm and rfa_rotfreq.hip one after the other — a second
// pass and a rounding to the io dtype in between; a token-wide norm in front of a multi-axis rotation had no kernel at all.
// Neither neighbour serves it by a flag: rfa_qktoken.hip fetches a token's cos / sin row from memory, rfa_qknormfreq.hip owns
// TILES of rows with one (row, head) per lane group and knows no statistic that crosses heads and waves.
//
// OWNERSHIP is rfa_qktoken.hip's (rfa_qktoken_index.h, unchanged): a token row belongs to a TEAM of 64, 128 or 256 lanes — 1, 2
//   or 4 waves of one 256-thread workgroup, chosen from N = H D alone; team lane l owns the 16-byte chunks l + j * team, j < K
//   (K <= 8, a template parameter: the larger tensor's need); x (backward: x and dO) stays in registers in the io dtype and is
//   read from HBM once per direction, every output written once, all offsets 64 bits wide.  q and k share one launch
//   (blockIdx.y), each with ITS team.
// ANGLE PHASE (in the place of the table fetch).  A row's R/2 (cos', sin') entries are formed ONCE for all its heads, by the
//   row's own team: team lane l takes the frequencies c = l and l + team (the second one exists only for one wave and R > 128),
//   so the sincosf of a row runs in the team's FIRST wave(s) and the others go straight to the barrier.  Per entry, in fp32, by
//   rotfreq_kernel's expressions:
//       pos = the map's arithmetic of the row, or pos_off + the int32 of the axis that c reads (axis map: 2 bits per frequency in
//             the kernel arguments)
//       ang = mul_rn(float(pos), inv_freq[c]);  (s, c) = sincosf(ang);  c' = mul_rn(c, scaling),  s' = mul_rn(s, scaling)
//   and c', s' (backward: -s') go as fp32 to tab[0 / 1][slot][c] in LDS.  What depends on (lane, c) alone — inv_freq[c] and
//   where the axis of c starts in `positions` — is per-LANE data: it is loaded once in front of the backward's walk and lives in
//   VECTOR registers (2 x 3), so the walk carries no per-entry scalar; the LDS slot is c itself.
// LDS, one barrier per row sum:
//   stage  halves pairing only: the row's chunks in the io dtype as they were loaded (forward x, backward dO), 16 B x chunks x
//          rows in flight <= 32 KiB.  The partner chunk R/16 further on / back is read from here and taken through the owner's
//          own expression, so both lanes of a pair hold the same bits.  Interleaved pairs are in-lane.
//   tab    the token's c' / s' row (R/2 fp32 each, 4 KiB for 4 rows in flight); a lane reads the 8 (interleaved: 4) values of
//          each of its rotated chunks from it
//   red    one partial row sum per wave
//   The staging, the angles and the first row sum's partials are all written in front of the SAME barrier.  The backward's walk
//   needs no further one: a step's writes of stage / tab / red[0] come behind the previous step's second barrier, in front of
//   which every read of them was done.
// SUMMATION ORDERS (the tests' tolerances are derived from these; they are rfa_qktoken.hip's, by rfa_qktoken_math.hpp's functions):
//   row sums (sum x^2; backward also sum (g a) xh): in a lane j = 0 .. K-1, e = 0 .. 7 as ONE chain of fmas starting from 0 (a
//     chunk that does not exist adds nothing), then the xor butterfly over the wave with masks 32, 16, .. 1, then the team's
//     waves' sums from LDS added in wave order starting from the first: 8 K + 6 + (team/64 - 1) <= 73 roundings.  Every lane of
//     the team ends with the same bits; they depend on (N, the row's values) alone.
//   rstd = rsqrt(ss / N + eps): row_rstd(), the bits of rfa_qktoken.hip, in both directions.
//   angle: ONE rounded multiply, sincosf, ONE rounded multiply by the scaling — per (row, c) the same expression whichever
//     lane, team, tensor or direction forms it.
//   forward: y = (x rstd) a, a = weight_offset + w, then rot() of rfa_rotary_math.hpp on the rotated columns; one rounding.
//   backward: g = rot() with s' -> -s' of dO (fp32, not rounded), xh = x rstd, m = (sum (g a) xh) / N,
//     dx = rstd (g a - xh m) with the subtraction as ONE fma; one rounding.
//   dw (per tensor): a lane adds g xh of its own columns (fma) over the `walk` rows its team visits, row (it * nparts + p) * slots
//     + slot for it = 0, 1, ..; the workgroup adds its `slots` teams in slot order through LDS and stores ONE fp32 (N,) partial;
//     rfa_qktoken.hip's fold kernel adds a column's nparts partials in 8 runs of ceil(nparts/8) consecutive ones, then the 8 sums
//     in order.  Longest chain: walk + slots + ceil(nparts/8) + 8 additions.  No atomics; nparts = min(ceil(rows/slots), 512) is
//     a function of the tensor's shape alone, so its weight gradient's bits do not depend on the tensor that rides along.
// grid: forward x = max over tensors of ceil(rows/slots), y = tensor; backward x = max over tensors of nparts, y = tensor; then
// launch_qktoken_fold.
#include "rfa_common.hpp"
#include "rfa_kernels.hpp"
#include "rfa_rotary_math.hpp"     // rot(), mul_rn()
#include "rfa_qktoken_math.hpp"

namespace rfa {
namespace {

using namespace qktoken_math;

// what team lane tl needs of its (at most two) frequencies c = tl + m * team, whatever the row
struct TokFreqEntries {
  float inv[2];             // inv_freq[c]
  int64_t axis[2];          // axis(c) * pos_axis: where the axis that c reads starts in `positions`
};

__device__ __forceinline__ void tokfreq_entries(const QkTokenFreqParams& p, uint32_t tl, uint32_t team, uint32_t half,
                                                TokFreqEntries& en) {
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const uint32_t c = tl + m * team;
    en.inv[m] = 0.f;
    en.axis[m] = 0;
    if (c < half) {
      en.inv[m] = p.inv_freq[c];
      en.axis[m] = (int64_t)rotfreq_axis(p.freq_axis[0], p.freq_axis[1], p.freq_axis[2], p.freq_axis[3], c) * p.pos_axis;
    }
  }
}

// the row's (cos', sin') entries into tab[0 / 1][slot][0 .. R/2), by the row's own team; CONJ (the backward): sin' -> -sin'
template <bool CONJ>
__device__ __forceinline__ void tokfreq_angles(const QkTokenFreqParams& p, const TokFreqEntries& en,
                                               float (*tab)[kMaxSlots][kTabFloats], uint32_t slot, uint32_t tl, uint32_t team,
                                               uint32_t half, uint32_t row, int64_t pos_off, int64_t pos_off2, int64_t pos_batch) {
  const uint32_t b = row / p.g.S, i = row % p.g.S;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const uint32_t c = tl + m * team;
    if (c >= half) continue;
    const int64_t pos = p.positions ? pos_off + (int64_t)p.positions[en.axis[m] + (int64_t)b * pos_batch + i]
                                    : rotary_map_pos(pos_off, p.pos_stride, p.pos_split, pos_off2, i);
    const float ang = mul_rn((float)pos, en.inv[m]);
    float sn, cs;
    sincosf(ang, &sn, &cs);
    cs = mul_rn(cs, p.scaling);
    sn = mul_rn(sn, p.scaling);
    tab[0][slot][c] = cs;
    tab[1][slot][c] = CONJ ? -sn : sn;
  }
}

template <typename T, int MODE, int K>
__global__ __launch_bounds__(256) void qktokenfreq_fwd_kernel(const QkTokenFreqParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char stage_raw[MODE == kTokHalves ? kStageBytes : 16];
  __shared__ float tab[2][kMaxSlots][kTabFloats];
  __shared__ float red[4];
  const int k = blockIdx.y;
  const QkTokenTensor t = p.t[k];
  const uint32_t team = t.team, slots = qktoken_slots(team);
  if ((uint64_t)blockIdx.x * slots >= t.rows) return;            // (the whole workgroup: the other tensor needs more of them)
  const uint32_t slot = threadIdx.x / team, tl = threadIdx.x % team, wave = threadIdx.x >> 6;
  const uint32_t jfull = t.chunks / team, tail = t.chunks % team;
  const uint32_t half = p.g.R / 2;
  const T* xp = (const T*)p.x[k];
  T* outp = (T*)p.out[k];
  const void* wp = p.weight[k];
  const uint64_t row64 = qktoken_row(0, 0, blockIdx.x, slot, team);
  const bool rlive = row64 < t.rows;
  const uint32_t row = rlive ? (uint32_t)row64 : 0u;
  vec8<T>* stage = (vec8<T>*)stage_raw;
  uint32_t hc[K], kt[K];
  lane_roles<K>(p.g, t, tl, hc, kt);
  vec8<T> xv[K];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t c = tl + j * team;
    const bool own = rlive && has_chunk(j, tl, jfull, tail);
    xv[j] = zero8<T>();
    if (own) {
      xv[j] = *(const vec8<T>*)(xp + qktoken_offset(p.g, row, hc[j] >> 16, hc[j] & 0xffffu, t.xb, t.xr, t.xh));
      if constexpr (MODE == kTokHalves) stage[slot * t.chunks + c] = xv[j];
    }
    float x[8];
    widen<T>(xv[j], x);
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = __builtin_fmaf(x[e], x[e], ss);
  }
  // (behind the loads, so that the sincosf of the team's first wave runs while they are in flight)
  if (rlive && tl < half) {
    TokFreqEntries en;
    tokfreq_entries(p, tl, team, half, en);
    tokfreq_angles<false>(p, en, tab, slot, tl, team, half, row, p.pos_off, p.pos_off2, p.pos_batch);
  }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63u) == 0) red[wave] = ss;
  __syncthreads();
  const float rstd = row_rstd(team_total(red, team, wave), t.N, p.eps);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t c = tl + j * team;
    if (!(rlive && has_chunk(j, tl, jfull, tail))) continue;
    const int kind = (int)(kt[j] >> 16);
    const uint32_t tcol = kt[j] & 0xffffu;
    float x[8], a[8], y[8], o[8];
    widen<T>(xv[j], x);
    load_scale<T>(p, wp, c, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (x[e] * rstd) * a[e];
    if (kind != kQkTokenPass) {
      float py[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if constexpr (MODE == kTokHalves) {
        const uint32_t pc = kind == kQkTokenLo ? c + p.g.R / 16 : c - p.g.R / 16;
        float px[8], pa[8];
        widen<T>(stage[slot * t.chunks + pc], px);
        load_scale<T>(p, wp, pc, pa);
#pragma unroll
        for (int e = 0; e < 8; ++e) py[e] = (px[e] * rstd) * pa[e];
      }
      rotate8<MODE, false>(y, py, o, kind, &tab[0][slot][tcol], &tab[1][slot][tcol]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = y[e];
    }
    store8<T>(outp + qktoken_offset(p.g, row, hc[j] >> 16, hc[j] & 0xffffu, t.ob, t.orow, t.oh), o);
  }
}

template <typename T, int MODE, int K>
__global__ __launch_bounds__(256) void qktokenfreq_bwd_kernel(const QkTokenFreqParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char stage_raw[kStageBytes];   // dO rows (halves); at the end the teams' dw
  __shared__ float tab[2][kMaxSlots][kTabFloats];
  __shared__ float red[2][4];
  const int k = blockIdx.y;
  QkTokenTensor t = p.t[k];
  t.xb = in_vgpr(t.xb), t.xr = in_vgpr(t.xr), t.xh = in_vgpr(t.xh);
  t.ob = in_vgpr(t.ob), t.orow = in_vgpr(t.orow), t.oh = in_vgpr(t.oh);
  t.gb = in_vgpr(t.gb), t.gr = in_vgpr(t.gr), t.gh = in_vgpr(t.gh);
  const int64_t pos_off = in_vgpr(p.pos_off), pos_off2 = in_vgpr(p.pos_off2), pos_batch = in_vgpr(p.pos_batch);
  const uint32_t team = t.team, slots = qktoken_slots(team);
  const uint32_t nparts = p.nparts[k], walk = p.walk[k];
  if (blockIdx.x >= nparts) return;                              // (the whole workgroup: the other tensor has more partials)
  const uint32_t slot = threadIdx.x / team, tl = threadIdx.x % team, wave = threadIdx.x >> 6;
  const uint32_t teamv = in_vgpr(team);                          // (j * team: K more scalars otherwise)
  const uint32_t jfull = t.chunks / team, tail = in_vgpr(t.chunks % team);
  const uint32_t half = p.g.R / 2;
  const T* xp = (const T*)in_vgpr((int64_t)p.x[k]);               // (bases of per-lane addresses: see in_vgpr)
  T* outp = (T*)in_vgpr((int64_t)p.out[k]);
  const void* wp = (const void*)in_vgpr((int64_t)p.weight[k]);
  const uint32_t wantv = p.dweight[k] != nullptr ? 1u : 0u;      // (tested through in_vgpr: its lane mask is formed at each use)
  const T* dp = (const T*)in_vgpr((int64_t)p.dout[k]);
  vec8<T>* stage = (vec8<T>*)stage_raw;
  uint32_t hc[K], kt[K];
  lane_roles<K>(p.g, t, tl, hc, kt);
  TokFreqEntries en;                                             // (per-lane values: vector registers across the walk)
  tokfreq_entries(p, tl, team, half, en);
  float acc[K][8];
#pragma unroll
  for (int j = 0; j < K; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
  for (uint32_t it = 0; it < walk; ++it) {
    if (qktoken_row(it, nparts, blockIdx.x, 0, team) >= t.rows) break;   // (the whole workgroup, and every later step)
    const uint64_t row64 = qktoken_row(it, nparts, blockIdx.x, slot, team);
    const bool rlive = row64 < t.rows;
    const uint32_t row = rlive ? (uint32_t)row64 : 0u;
    const bool want_dw = in_vgpr(wantv) != 0;
    vec8<T> xv[K], dv[K];
    float ss = 0.f;
    // (the roles do not change from step to step; made opaque here so that the lane masks of the K chunks' kinds are formed
    //  where they are used, not all kept in scalar registers across the walk)
#pragma unroll
    for (int j = 0; j < K; ++j) asm volatile("" : "+v"(kt[j]));
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const uint32_t c = tl + j * teamv;
      const bool own = rlive && has_chunk(j, tl, jfull, tail);
      xv[j] = zero8<T>();
      dv[j] = zero8<T>();
      if (own) {
        const uint32_t head = hc[j] >> 16, col = hc[j] & 0xffffu;
        xv[j] = *(const vec8<T>*)(xp + qktoken_offset(p.g, row, head, col, t.xb, t.xr, t.xh));
        dv[j] = *(const vec8<T>*)(dp + qktoken_offset(p.g, row, head, col, t.gb, t.gr, t.gh));
        if constexpr (MODE == kTokHalves) stage[slot * t.chunks + c] = dv[j];
      }
      float x[8];
      widen<T>(xv[j], x);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss = __builtin_fmaf(x[e], x[e], ss);
    }
    if (rlive && tl < half) tokfreq_angles<true>(p, en, tab, slot, tl, teamv, half, row, pos_off, pos_off2, pos_batch);
    ss = wave_sum(ss);
    if ((threadIdx.x & 63u) == 0) red[0][wave] = ss;
    __syncthreads();
    // (a slot past the tensor's end holds zeros: with eps == 0 its rsqrt(0) is inf — such a row counts with rstd 0 and its
    //  lanes skip the arithmetic, whose angles were not formed)
    const float rs = row_rstd(team_total(red[0], team, wave), t.N, p.eps);
    const float rstd = rlive ? rs : 0.f;
    float ga[K][8];
    float ms = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const uint32_t c = tl + j * teamv;
#pragma unroll
      for (int e = 0; e < 8; ++e) ga[j][e] = 0.f;
      if (!(rlive && has_chunk(j, tl, jfull, tail))) continue;
      const int kind = (int)(kt[j] >> 16);
      const uint32_t tcol = kt[j] & 0xffffu;
      float x[8], d[8], a[8], g[8];
      widen<T>(xv[j], x);
      widen<T>(dv[j], d);
      load_scale<T>(p, wp, c, a);
      if (kind != kQkTokenPass) {
        float pd[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if constexpr (MODE == kTokHalves) {
          const uint32_t pc = kind == kQkTokenLo ? c + p.g.R / 16 : c - p.g.R / 16;
          widen<T>(stage[slot * t.chunks + pc], pd);
        }
        rotate8<MODE, false>(d, pd, g, kind, &tab[0][slot][tcol], &tab[1][slot][tcol]);   // (tab[1] holds -s')
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = d[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xh = x[e] * rstd;
        ga[j][e] = g[e] * a[e];
        ms = __builtin_fmaf(ga[j][e], xh, ms);
        if (want_dw) acc[j][e] = __builtin_fmaf(g[e], xh, acc[j][e]);
      }
    }
    ms = wave_sum(ms);
    if ((threadIdx.x & 63u) == 0) red[1][wave] = ms;
    __syncthreads();
    const float m = team_total(red[1], team, wave) / (float)t.N;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (!(rlive && has_chunk(j, tl, jfull, tail))) continue;
      float x[8], dx[8];
      widen<T>(xv[j], x);
#pragma unroll
      for (int e = 0; e < 8; ++e) dx[e] = rstd * __builtin_fmaf(-(x[e] * rstd), m, ga[j][e]);
      store8<T>(outp + qktoken_offset(p.g, row, hc[j] >> 16, hc[j] & 0xffffu, t.ob, t.orow, t.oh), dx);
    }
  }
  if (in_vgpr(wantv) == 0) return;                                          // (uniform over the workgroup)
  store_dw_partial<K>(p, k, t.N, (float*)stage_raw, acc, slots, slot, tl, teamv, jfull, tail);
}

template <typename T, int MODE, int K>
void launch_k(const QkTokenFreqParams& p, bool bwd, dim3 grid, hipStream_t stream) {
  const dim3 block(kQkTokenThreads);
  if (bwd) hipLaunchKernelGGL((qktokenfreq_bwd_kernel<T, MODE, K>), grid, block, 0, stream, p);
  else hipLaunchKernelGGL((qktokenfreq_fwd_kernel<T, MODE, K>), grid, block, 0, stream, p);
}

template <typename T, int MODE>
void launch_m(const QkTokenFreqParams& p, bool bwd, dim3 grid, hipStream_t stream) {
  uint32_t need = 0;
  for (int i = 0; i < p.ntensors; ++i) {
    const uint32_t per = qktoken_per_lane(p.t[i].N);
    need = per > need ? per : need;
  }
  if (need <= 2) launch_k<T, MODE, 2>(p, bwd, grid, stream);
  else if (need <= 4) launch_k<T, MODE, 4>(p, bwd, grid, stream);
  else launch_k<T, MODE, 8>(p, bwd, grid, stream);
}

template <typename T>
void launch_t(const QkTokenFreqParams& p, bool bwd, dim3 grid, hipStream_t stream) {
  if (p.g.interleaved) launch_m<T, kTokInterleaved>(p, bwd, grid, stream);
  else launch_m<T, kTokHalves>(p, bwd, grid, stream);
}

}  // namespace

int launch_qktokenfreq_fwd(const QkTokenFreqParams& p, int dtype, hipStream_t stream) {
  uint32_t blocks = 0;
  for (int i = 0; i < p.ntensors; ++i) {
    const uint32_t n = qktoken_blocks(p.t[i].rows, p.t[i].team);
    blocks = n > blocks ? n : blocks;
  }
  if (blocks == 0) return 0;
  const dim3 grid(blocks, (unsigned)p.ntensors);
  if (dtype == 0) launch_t<bf16_t>(p, false, grid, stream);
  else launch_t<f16_t>(p, false, grid, stream);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_qktokenfreq_bwd(const QkTokenFreqParams& p, int dtype, hipStream_t stream) {
  const uint32_t blocks = p.ntensors > 1 && p.nparts[1] > p.nparts[0] ? p.nparts[1] : p.nparts[0];
  if (blocks == 0) return 0;
  const dim3 grid(blocks, (unsigned)p.ntensors);
  if (dtype == 0) launch_t<bf16_t>(p, true, grid, stream);
  else launch_t<f16_t>(p, true, grid, stream);
  if (hipGetLastError() != hipSuccess) return -1;
  return launch_qktoken_fold(p, stream);
}

}  // namespace rfa
