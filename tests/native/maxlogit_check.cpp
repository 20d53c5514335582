// maxlogit_check.cpp — host check of csrc/rfa_maxlogit_band.h, the tile arithmetic of the max-logit kernel: compiled with
// -fsanitize=address,undefined and run by tests/test_max_logit_cpu.py.  For every geometry of the grid
//     lq, lk   in {1, 31, 64, 65, 255, 256, 257, 777, 1000} and the front / back halves of those lengths (what q_half / k_half
//              make of them: S / 2 and S - S / 2)
//     off      (= lk - lq + shift) m - 2 .. m + 2 around every multiple m of 32 (so of 64) from below -lq to above lk, and
//              the same around the offsets at which the band's edges off - wl / off + wr are such multiples
//     band     causal; causal with a left window; left window only; right window only; two-sided
// it checks, against the brute-force mask (the predicate of include/rfa.h evaluated for every key of a row):
//     * [jt0, ntiles) of every workgroup covers all keys its rows see, and a workgroup classified empty sees nothing
//     * a (wave, tile) classified kMlSkip holds no visible element of a real row
//     * a (wave, tile) classified kMlInside holds no masked element among its real rows, and all its 64 keys exist
//     * ml_row_keys of every row is exactly the row's visible set
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "rfa_maxlogit_band.h"

using namespace rfa;

struct Form { const char* name; int wl, wr; };
static const Form kForms[] = {{"causal", -1, 0}, {"causal+left", 130, 0}, {"left", 300, -1}, {"right", -1, 40}, {"two-sided", 90, 40}};

static long g_fail = 0, g_geoms = 0, g_inside = 0, g_edge = 0, g_skip = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 20) { std::printf("FAIL %s:%d ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// brute force: the visible keys of a row with x = i + off, by evaluating the predicate for every key; [lo, hi], lo > hi: none
struct RowVis { int lo, hi; };
static RowVis brute_row(int64_t x, int lk, int wl, int wr) {
  RowVis r{lk, -1};
  bool seen = false, ended = false;
  for (int j = 0; j < lk; ++j) {
    const bool v = (wr < 0 || j <= x + wr) && (wl < 0 || j >= x - wl);
    if (v) {
      if (ended) { ++g_fail; std::printf("FAIL: visible set of x=%lld not contiguous\n", (long long)x); }
      if (!seen) r.lo = j;
      r.hi = j;
      seen = true;
    } else if (seen) {
      ended = true;
    }
  }
  return r;
}

static void check_geometry(int lq, int lk, int64_t off, const Form& f, const std::vector<RowVis>& cache, int64_t x0) {
  ++g_geoms;
  const MlBand b{off, f.wl, f.wr};
  auto row = [&](int i) { return cache[(size_t)(i + off - x0)]; };
  for (int i = 0; i < lq; ++i) {
    int klo, khi;
    ml_row_keys(i, lk, b, klo, khi);
    const RowVis r = row(i);
    if (r.lo > r.hi) CHECK(klo > khi, "row_keys: %s lq %d lk %d off %lld row %d: [%d, %d] but the row sees nothing", f.name, lq, lk, (long long)off, i, klo, khi);
    else CHECK(klo == r.lo && khi == r.hi, "row_keys: %s lq %d lk %d off %lld row %d: [%d, %d], brute force [%d, %d]", f.name, lq, lk, (long long)off, i, klo, khi, r.lo, r.hi);
  }
  const int all_tiles = (lk + kMlKV - 1) / kMlKV;
  for (int qwg0 = 0; qwg0 < lq; qwg0 += kMlQRows) {
    const int qend = qwg0 + kMlQRows < lq ? qwg0 + kMlQRows : lq;
    int jt0, ntiles;
    ml_tile_range(qwg0, qend, lk, b, jt0, ntiles);
    CHECK(jt0 >= 0 && ntiles <= all_tiles, "range: %s lq %d lk %d off %lld wg %d: [%d, %d) outside [0, %d)", f.name, lq, lk, (long long)off, qwg0, jt0, ntiles, all_tiles);
    for (int w0 = qwg0; w0 < qwg0 + kMlQRows; w0 += kMlWaveRows) {
      const int r1 = w0 + kMlWaveRows < lq ? w0 + kMlWaveRows : lq;            // real rows [w0, r1)
      for (int j = 0; j < all_tiles + 1; ++j) {
        const int kt0 = j * kMlKV, kt1 = kt0 + kMlKV - 1;
        bool any = false, all = kt1 <= lk - 1 && w0 < lq;
        for (int i = w0; i < r1; ++i) {
          const RowVis r = row(i);
          if (r.lo <= r.hi && r.lo <= kt1 && r.hi >= kt0) any = true;
          if (!(r.lo <= kt0 && r.hi >= kt1)) all = false;
        }
        const bool in_range = j >= jt0 && j < ntiles;
        if (!in_range) CHECK(!any, "cover: %s lq %d lk %d off %lld wave %d tile %d outside [%d, %d) holds a visible element", f.name, lq, lk, (long long)off, w0, j, jt0, ntiles);
        const int cls = ml_tile_class(w0, lq, lk, b, j);
        if (cls == kMlSkip) { ++g_skip; CHECK(!any, "skip: %s lq %d lk %d off %lld wave %d tile %d holds a visible element", f.name, lq, lk, (long long)off, w0, j); }
        else if (cls == kMlInside) { ++g_inside; CHECK(all, "inside: %s lq %d lk %d off %lld wave %d tile %d holds a masked element or a key behind lk", f.name, lq, lk, (long long)off, w0, j); }
        else { ++g_edge; CHECK(cls == kMlEdge, "class %d", cls); }
      }
    }
  }
}

int main() {
  const int base[] = {1, 31, 64, 65, 255, 256, 257, 777, 1000};
  std::set<int> lens;
  for (int s : base) {
    lens.insert(s);
    if (s / 2 > 0) lens.insert(s / 2);
    lens.insert(s - s / 2);
  }
  for (const Form& f : kForms)
    for (int lk : lens) {
      // x = i + off ranges over [-(max lq) - 65, lk + 65 + max lq]
      const int64_t x0 = -1200, x1 = lk + 1200;
      std::vector<RowVis> cache;
      cache.reserve((size_t)(x1 - x0 + 1));
      for (int64_t x = x0; x <= x1; ++x) cache.push_back(brute_row(x, lk, f.wl, f.wr));
      for (int lq : lens) {
        std::set<int64_t> offs;
        // m - 2 .. m + 2: an off-by-one in a bound shows at the offset NEXT to the one where the bound meets a tile edge;
        // and the same around the offsets at which the band's own edges (off - wl, off + wr) meet a multiple of 32
        for (int64_t m = -((lq + 63) / 32) * 32; m <= ((lk + 63) / 32) * 32; m += 32)
          for (int d = -2; d <= 2; ++d) {
            offs.insert(m + d);
            if (f.wl > 0) offs.insert(m + d + f.wl % 32);
            if (f.wr > 0) offs.insert(m + d - f.wr % 32);
          }
        for (int64_t off : offs) check_geometry(lq, lk, off, f, cache, x0);
      }
    }
  // numbers no 32-bit expression could hold: every step is formed in 64 bits (UBSan watches)
  {
    const MlBand b{(int64_t)1 << 40, 2147483647, 2147483647};
    int jt0, ntiles, klo, khi;
    ml_tile_range(0, 256, 1000, b, jt0, ntiles);
    ml_row_keys(255, 1000, b, klo, khi);
    CHECK(jt0 >= ntiles || ml_tile_class(0, 300, 1000, b, jt0) != kMlInside || true, "unreachable");
    const MlBand c{-((int64_t)1 << 40), 2147483647, 2147483647};
    ml_tile_range(0, 256, 1000, c, jt0, ntiles);
    ml_row_keys(255, 1000, c, klo, khi);
    (void)ml_tile_class(0, 300, 1000, c, 0);
  }
  std::printf("%ld geometries, %ld wave-tiles inside, %ld edge, %ld skipped\n", g_geoms, g_inside, g_edge, g_skip);
  if (g_fail) { std::printf("%ld failures\n", g_fail); return 1; }
  std::printf("max-logit tile arithmetic ok\n");
  return 0;
}
