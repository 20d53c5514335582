// rfa_rowrange.h — the clamp and skip arithmetic of per-row key ranges (rfa.h: rfa_rowrange_args), shared by the forward, dQ
// and dK/dV kernels, the tile-bounds pre-kernel and the host-side check (tests/native/rowrange_check.cpp).
//
// Query row i of a block sees key j of the block iff start[i] <= k_pos0 + j < end[i] (and the call's own band allows the
// pair).  Everything below works on BLOCK-RELATIVE bounds: [lo, hi) in key rows of the block, clamped to [0, lk].
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RFA_RR_HD __host__ __device__ inline
#else
#define RFA_RR_HD inline
#endif

namespace rfa {

constexpr int kRrNoLo = 0x3fffffff;   // lo of an empty row: neutral under min (its hi is 0: neutral under max)

// one bound: the global key position v against the block's key row 0 at k_pos0, clamped to [0, lk]
RFA_RR_HD int rr_rel(int32_t v, int64_t k_pos0, int lk) {
  const int64_t x = (int64_t)v - k_pos0;
  return x < 0 ? 0 : (x > (int64_t)lk ? lk : (int)x);
}

// a row's visible keys [lo, hi) inside a block of lk keys; a row that sees none of them: (kRrNoLo, 0)
struct RrRow {
  int lo, hi;
};
RFA_RR_HD RrRow rr_row(int32_t start, int32_t end, int64_t k_pos0, int lk) {
  RrRow r{rr_rel(start, k_pos0, lk), rr_rel(end, k_pos0, lk)};
  if (r.lo >= r.hi) r = RrRow{kRrNoLo, 0};
  return r;
}

// the key tiles a workgroup walks: the band's key range [kmin, kmax) (kmax may be <= 0: nothing) cut to the rows' range
// [wlo, whi) = (min lo, max hi) over the workgroup's rows.  Tiles of `tile` keys; the first tile is aligned down to a multiple
// of `align` (the LDS ring: stage = tile index % align).  Nothing visible: {0, 0}.
struct RrTiles {
  int jt0, ntiles;   // tiles jt0 .. ntiles - 1
};
RFA_RR_HD RrTiles rr_tiles(int kmin, int kmax, int wlo, int whi, int tile, int align) {
  const int lo = kmin > wlo ? kmin : wlo;
  const int hi = kmax < whi ? kmax : whi;
  if (hi <= lo || hi <= 0) return RrTiles{0, 0};
  return RrTiles{(lo / tile) / align * align, (hi + tile - 1) / tile};
}

// does a query tile whose rows' (min lo, max hi) is (lo, hi) hold a row that sees a key of the block [k0, k0 + n)?
// (necessary, not sufficient: a visited tile still applies the per-row bounds)
RFA_RR_HD bool rr_touches(int lo, int hi, int k0, int n) { return lo < k0 + n && hi > k0; }

#if defined(__HIPCC__)
// over the 64 rows a wave's lanes hold: (min lo, max hi) — what the wave's tiles are skipped by — and (max lo, min hi) — a
// tile inside [max lo, min hi) needs no per-row predicate; wave-uniform (scalar registers)
struct RrWave {
  int lo, hi, mlo, mhi;
};
__device__ __forceinline__ RrWave rr_wave(int lo, int hi) {
  RrWave w{lo, hi, lo, hi};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(w.lo, o, 64), b = __shfl_xor(w.hi, o, 64), c = __shfl_xor(w.mlo, o, 64), d = __shfl_xor(w.mhi, o, 64);
    w.lo = a < w.lo ? a : w.lo;
    w.hi = b > w.hi ? b : w.hi;
    w.mlo = c > w.mlo ? c : w.mlo;
    w.mhi = d < w.mhi ? d : w.mhi;
  }
  return RrWave{__builtin_amdgcn_readfirstlane(w.lo), __builtin_amdgcn_readfirstlane(w.hi),
                __builtin_amdgcn_readfirstlane(w.mlo), __builtin_amdgcn_readfirstlane(w.mhi)};
}
// (min lo, max hi) over a workgroup's `nwaves` waves through `xch` (2 * nwaves ints of LDS that nobody writes before the
// next barrier); one barrier, every thread of the workgroup must call it
__device__ __forceinline__ void rr_workgroup(const RrWave& w, int wave, int lane, int nwaves, volatile int* xch, int& lo, int& hi) {
  if (lane == 0) {
    xch[2 * wave] = w.lo;
    xch[2 * wave + 1] = w.hi;
  }
  __syncthreads();
  lo = xch[0];
  hi = xch[1];
  for (int i = 1; i < nwaves; ++i) {
    const int a = xch[2 * i], b = xch[2 * i + 1];
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
}
#endif

}  // namespace rfa
