// rfa_maxlogit_band.h — which key tiles a workgroup of maxlogit_kernel (rfa_maxlogit.hip) visits and how a wave treats each
// of them.  Plain integer arithmetic, __host__ __device__: the kernel and the CPU check tests/native/maxlogit_check.cpp
// (every geometry of a grid against the brute-force mask) compile the same lines.
//
// The band is the forward's (include/rfa.h: mask_shift, mask_shift_lens): query row i of a sequence with lq rows and lk keys
// sees key j iff
//     i + off - wl <= j <= i + off + wr,   0 <= j < lk,      off = lk - lq + shift + shift_lens * lk
// each side only when set (wl / wr >= 0; causal arrives as wr = 0).  Everything is formed in 64 bits, so no combination of
// 32-bit lengths, shifts and windows wraps.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RFA_ML_HD __host__ __device__ inline
#else
#define RFA_ML_HD inline
#endif

namespace rfa {

constexpr int kMlWaves = 8;                     // waves per workgroup
constexpr int kMlWaveRows = 32;                 // query rows per wave
constexpr int kMlQRows = kMlWaves * kMlWaveRows;   // query rows per workgroup
constexpr int kMlKV = 64;                       // keys per tile

struct MlBand {
  int64_t off;
  int wl, wr;                                   // < 0: that side is unbounded
};

RFA_ML_HD int64_t ml_off(int lq, int lk, int64_t shift, int shift_lens) {
  return (int64_t)lk - lq + shift + (int64_t)shift_lens * lk;
}

// visible keys of query row `row`: [klo, khi] (empty when klo > khi); both fit an int: -1 <= khi < lk, 0 <= klo <= lk
RFA_ML_HD void ml_row_keys(int row, int lk, const MlBand& b, int& klo, int& khi) {
  int64_t hi = (int64_t)lk - 1, lo = 0;
  if (b.wr >= 0 && row + b.off + b.wr < hi) hi = row + b.off + b.wr;
  if (b.wl >= 0 && row + b.off - b.wl > lo) lo = row + b.off - b.wl;
  khi = (int)(hi < -1 ? -1 : hi);
  klo = (int)(lo > lk ? lk : lo);
}

// tiles [jt0, ntiles) hold every key that a row of [r0, r1) sees (0 <= r0 < r1 <= lq); jt0 >= ntiles: the rows see nothing
RFA_ML_HD void ml_tile_range(int r0, int r1, int lk, const MlBand& b, int& jt0, int& ntiles) {
  int64_t kmax = lk;
  if (b.wr >= 0 && r1 + b.off + b.wr < kmax) kmax = r1 + b.off + b.wr;          // (last row r1 - 1 sees keys <= r1 - 1 + off + wr)
  ntiles = kmax > 0 ? (int)((kmax + kMlKV - 1) / kMlKV) : 0;
  int64_t kmin = b.wl >= 0 ? r0 + b.off - b.wl : 0;
  kmin = kmin > 0 ? (kmin < lk ? kmin : lk) : 0;
  jt0 = (int)(kmin / kMlKV);
}

enum { kMlSkip = 0, kMlInside = 1, kMlEdge = 2 };
// how the wave whose first row is w0 treats key tile j.  Its REAL rows are [w0, min(w0 + 32, lq)); rows behind lq are
// computed on a clamped copy of row lq - 1 and dropped at the end, so they do not count here.
//   kMlSkip    no real row sees a key of the tile
//   kMlInside  every real row sees every key of the tile and all 64 keys exist: the bare max
//   kMlEdge    anything else: per-element predicates against ml_row_keys
RFA_ML_HD int ml_tile_class(int w0, int lq, int lk, const MlBand& b, int j) {
  if (w0 >= lq) return kMlSkip;
  const int64_t rl = w0, rh = (w0 + kMlWaveRows < lq ? w0 + kMlWaveRows : lq) - 1;
  const int64_t kt0 = (int64_t)j * kMlKV, kt1 = kt0 + kMlKV - 1;
  if (kt0 >= lk) return kMlSkip;
  const int64_t klast = kt1 < lk - 1 ? kt1 : (int64_t)lk - 1;                   // last key of the tile that exists
  if (b.wr >= 0 && kt0 > rh + b.off + b.wr) return kMlSkip;
  if (b.wl >= 0 && klast < rl + b.off - b.wl) return kMlSkip;
  if (kt1 > lk - 1) return kMlEdge;
  if (b.wr >= 0 && kt1 > rl + b.off + b.wr) return kMlEdge;
  if (b.wl >= 0 && kt0 < rh + b.off - b.wl) return kMlEdge;
  return kMlInside;
}

}  // namespace rfa
