// rowrange_check.cpp — stand-alone host check of the clamp and skip arithmetic of per-row key ranges
// (ring-flash-attention_amd/csrc/rfa_rowrange.h: the functions the gfx950 kernels and the tile-bounds pre-kernel use as well).
// No GPU, no HIP:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ring-flash-attention_amd/csrc tests/native/rowrange_check.cpp
// For small geometries — lq, lk off and on the tile boundaries, k_pos0 in front of, inside and behind the ranges, bands
// (none, causal, windows, shifted), row patterns (documents, prefix, random, empty rows, ranges wholly before / after the
// block, negative and oversized values) — it builds the brute-force mask
//     vis(i, j) = band(i, j) and start[i] <= k_pos0 + j < end[i]
// and checks, exactly as the kernels walk:
//   * rr_row: key j of the block is inside [lo, hi) iff start <= k_pos0 + j < end; an empty row is (kRrNoLo, 0);
//   * forward / dQ (workgroups of 256 rows, 64-key tiles, ring depths 2 and 3): every visible (i, j) lies in a tile of
//     [jt0, ntiles) of its workgroup; a workgroup without a visible pair gets NO tile; the first tile is aligned to the ring
//     and no tile in front of the first aligned one that holds a visible key, none behind the last, is walked;
//   * dK/dV (key blocks of 128, query tiles of 64): rr_touches(min lo, max hi) is true for every (tile, key block) that
//     holds a visible pair (ranges alone: it is exact for tiles whose rows' ranges form one interval — documents —, and
//     never false where a pair is visible), and the per-row bounds rr_rel give the mask inside a visited tile.
// Exit status 0 and "rowrange_check: N configurations ok" on success; the first failure is printed and the status is 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rfa_rowrange.h"

using namespace rfa;

struct Band {
  int causal, wl, wr, shift;
};

static bool band_ok(const Band& b, int lq, int lk, int i, int j) {
  const int off = lk - lq + b.shift;
  const int wr = b.causal ? 0 : b.wr;
  if (wr >= 0 && j > i + off + wr) return false;
  if (b.wl >= 0 && j < i + off - b.wl) return false;
  return true;
}

static uint32_t rng_state = 12345u;
static int rnd(int n) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (int)((rng_state >> 8) % (uint32_t)n);
}

static void make_rows(int pattern, int lq, int total, std::vector<int32_t>& s, std::vector<int32_t>& e) {
  s.assign(lq, 0);
  e.assign(lq, 0);
  for (int i = 0; i < lq; ++i) {
    switch (pattern) {
      case 0: { const int d = 37; s[i] = (i / d) * d; e[i] = s[i] + d; break; }                 // documents
      case 1: s[i] = 0; e[i] = i + 1 > total / 3 ? i + 1 : total / 3; break;                      // prefix-LM
      case 2: s[i] = rnd(total + 40) - 20; e[i] = s[i] + rnd(total) - 10; if (i % 5 == 0) e[i] = s[i]; break;   // random, empty rows
      case 3: s[i] = -2147483647 - 1; e[i] = 2147483647; break;                                   // everything, by the extremes
      case 4: s[i] = total + 5; e[i] = total + 50; break;                                        // wholly behind
      case 5: s[i] = -90; e[i] = -3; break;                                                      // wholly in front
      case 6: s[i] = i; e[i] = i + 1; break;                                                     // one key per row
      default: s[i] = 63 + (i % 3); e[i] = 127 + (i % 3); break;                                 // edges at 63 / 64 / 65, 127 / 128 / 129
    }
  }
}

static int fail(const char* what, int lq, int lk, long long k0, int pattern, const Band& b) {
  std::printf("rowrange_check: FAILED: %s (lq %d lk %d k_pos0 %lld pattern %d causal %d wl %d wr %d shift %d)\n", what, lq, lk,
              k0, pattern, b.causal, b.wl, b.wr, b.shift);
  return 1;
}

static int check(int lq, int lk, int64_t k0, int pattern, const Band& b) {
  std::vector<int32_t> s, e;
  make_rows(pattern, lq, lk + (int)(k0 > 0 ? k0 : 0), s, e);
  std::vector<char> vis((size_t)lq * lk, 0), rvis((size_t)lq * lk, 0);
  std::vector<RrRow> rows(lq);
  for (int i = 0; i < lq; ++i) {
    rows[i] = rr_row(s[i], e[i], k0, lk);
    if (rows[i].lo >= rows[i].hi && !(rows[i].lo == kRrNoLo && rows[i].hi == 0)) return fail("empty row not canonical", lq, lk, k0, pattern, b);
    if (rows[i].lo < rows[i].hi && (rows[i].lo < 0 || rows[i].hi > lk)) return fail("bounds outside the block", lq, lk, k0, pattern, b);
    const int lo1 = rr_rel(s[i], k0, lk), hi1 = rr_rel(e[i], k0, lk);
    for (int j = 0; j < lk; ++j) {
      const bool in_range = (int64_t)s[i] <= k0 + j && k0 + j < (int64_t)e[i];
      if (in_range != (j >= rows[i].lo && j < rows[i].hi)) return fail("rr_row disagrees with the range", lq, lk, k0, pattern, b);
      if (in_range != (j >= lo1 && j < hi1)) return fail("rr_rel disagrees with the range", lq, lk, k0, pattern, b);
      rvis[(size_t)i * lk + j] = in_range;
      vis[(size_t)i * lk + j] = in_range && band_ok(b, lq, lk, i, j);
    }
  }
  const int off = lk - lq + b.shift;
  const int wr = b.causal ? 0 : b.wr;
  // ---- forward / dQ: workgroups of 256 rows, tiles of 64 keys
  for (int align = 2; align <= 3; ++align)
    for (int q0 = 0; q0 < lq; q0 += 256) {
      const int qend = q0 + 256 < lq ? q0 + 256 : lq;
      int wlo = kRrNoLo, whi = 0;
      for (int i = q0; i < qend; ++i) {
        wlo = rows[i].lo < wlo ? rows[i].lo : wlo;
        whi = rows[i].hi > whi ? rows[i].hi : whi;
      }
      int kmax = lk;
      if (wr >= 0 && qend + off + wr < kmax) kmax = qend + off + wr;
      const int kmin = b.wl >= 0 ? q0 + off - b.wl : 0;
      const RrTiles t = rr_tiles(kmin, kmax, wlo, whi, 64, align);
      if (t.jt0 < 0 || t.ntiles < 0 || t.jt0 % align) return fail("tile range malformed", lq, lk, k0, pattern, b);
      int first = -1, last = -1;
      for (int i = q0; i < qend; ++i)
        for (int j = 0; j < lk; ++j)
          if (vis[(size_t)i * lk + j]) {
            if (first < 0 || j < first) first = j;
            if (j > last) last = j;
            if (j / 64 < t.jt0 || j / 64 >= t.ntiles) return fail("a visible key outside the workgroup's tiles", lq, lk, k0, pattern, b);
          }
      if (first < 0) {
        // (the range and the band may each be non-empty and still share no key: then tiles may be walked, all masked; where
        //  either is empty nothing may be walked)
        if ((whi == 0 || kmax <= 0) && t.ntiles != 0) return fail("tiles for a workgroup without a key", lq, lk, k0, pattern, b);
      } else if (t.ntiles * 64 >= lk + 64) {
        return fail("tiles past the end of the block", lq, lk, k0, pattern, b);
      }
      // the range part alone is tight: the walked tiles start at the (aligned) tile of min lo and end at the tile of max hi
      if (whi > 0 && b.wl < 0 && wr < 0) {
        if (t.jt0 != (wlo / 64) / align * align || t.ntiles != (whi + 63) / 64) return fail("tile range not tight", lq, lk, k0, pattern, b);
      }
    }
  // ---- dK/dV: key blocks of 128, query tiles of 64 and their (min lo, max hi)
  for (int t0 = 0; t0 < lq; t0 += 64) {
    const int tend = t0 + 64 < lq ? t0 + 64 : lq;
    int lo = kRrNoLo, hi = 0;
    bool one_interval = true;
    for (int i = t0; i < tend; ++i) {
      lo = rows[i].lo < lo ? rows[i].lo : lo;
      hi = rows[i].hi > hi ? rows[i].hi : hi;
    }
    for (int j = 0; j < lk && one_interval; ++j) {
      bool any = false;
      for (int i = t0; i < tend; ++i) any = any || rvis[(size_t)i * lk + j];
      if (j >= lo && j < hi && !any) one_interval = false;
    }
    for (int kb = 0; kb < lk; kb += 128) {
      bool any = false;
      for (int i = t0; i < tend; ++i)
        for (int j = kb; j < kb + 128 && j < lk; ++j) any = any || rvis[(size_t)i * lk + j];
      const bool touch = rr_touches(lo, hi, kb, 128);
      if (any && !touch) return fail("a tile with a visible pair is skipped", lq, lk, k0, pattern, b);
      if (!any && touch && one_interval) return fail("a tile without a visible pair is visited", lq, lk, k0, pattern, b);
    }
  }
  return 0;
}

int main() {
  const int lqs[] = {1, 65, 130, 256, 320};
  const int lks[] = {1, 63, 64, 129, 200, 320};
  const long long k0s[] = {0, 64, 100, 320, -50, 5000000000LL, -5000000000LL};
  const Band bands[] = {{0, -1, -1, 0}, {1, -1, -1, 0}, {1, 40, -1, 0}, {0, 17, 9, 0}, {1, -1, -1, 64}, {1, 100, -1, -70}, {0, -1, 5, 200}};
  long n = 0;
  for (int lq : lqs)
    for (int lk : lks)
      for (long long k0 : k0s)
        for (int pattern = 0; pattern < 8; ++pattern)
          for (const Band& b : bands) {
            if (check(lq, lk, (int64_t)k0, pattern, b)) return 1;
            ++n;
          }
  std::printf("rowrange_check: %ld configurations ok\n", n);
  return 0;
}
