// blockmask_check.cpp — the bit addressing and walk arithmetic of csrc/rfa_blockmask.h (the header the forward, dQ and dK/dV
// kernels share) against the brute-force boolean mask, as a host program of its own: built with -fsanitize=address,undefined
// by tests/test_block_mask_cpu.py.  The mask rows / columns are heap buffers of exactly the stated size, so a read outside
// [0, nk_blocks) or past the last query block is an ASan error, not a silent zero.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>

#include "rfa_blockmask.h"

using namespace rfa;

static long long n_ok = 0;
#define CHECK(c)                                                                   \
  do {                                                                             \
    if (!(c)) {                                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);                   \
      std::exit(1);                                                                \
    }                                                                              \
  } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

// ---- forward / dQ: rows, windows, the visited list --------------------------------------------------------------------------------
// pattern: 0 random, 1 all lit, 2 all dark, 3 only the last block, 4 first + last, 5 every other block
static std::vector<uint8_t> make_row(int nk, int pattern, int density) {
  std::vector<uint8_t> r((size_t)nk);
  for (int c = 0; c < nk; ++c) {
    bool on = false;
    switch (pattern) {
      case 0: on = (int)(rnd() % 100) < density; break;
      case 1: on = true; break;
      case 2: on = false; break;
      case 3: on = c == nk - 1; break;
      case 4: on = c == 0 || c == nk - 1; break;
      default: on = (c & 1) == 0; break;
    }
    r[(size_t)c] = on ? (uint8_t)(1 + rnd() % 255) : 0;       // (non-zero = lit, not just 1)
  }
  return r;
}

static void check_rows(int nk, int64_t k_blk0, int ntile_local, int pattern, int density) {
  const std::vector<uint8_t> r0 = make_row(nk, pattern, density), r1 = make_row(nk, pattern == 0 ? 0 : 2, density);
  // brute force: key tile j (64 keys) of the block call is block kb = j / 2, column k_blk0 + kb
  auto lit = [&](const std::vector<uint8_t>& r, int j) {
    const int64_t c = k_blk0 + j / 2;
    return c >= 0 && c < nk && r[(size_t)c] != 0;
  };
  const int nwin = (ntile_local + kBmWinTiles - 1) / kBmWinTiles + 1;
  for (int w = 0; w < nwin; ++w) {
    const uint64_t a = bm_word(r0.data(), nk, k_blk0, w), b = bm_word(r1.data(), nk, k_blk0, w);
    const uint64_t u = bm_union(a, b);
    for (int i = 0; i < 128; ++i) {
      const int j = 128 * w + i;
      CHECK(bm_tile_lit(a, w, j) == lit(r0, j));
      CHECK(bm_tile_lit(u, w, j) == (lit(r0, j) || lit(r1, j)));
      CHECK(!bm_tile_lit(a, w + 1, j));
    }
  }
  // band ranges [jbeg, jend) of every kind: empty, one tile, odd ends, across windows
  const int ends[] = {0, 1, 2, 3, 5, 126, 127, 128, 129, 131, 255, 256, 257, ntile_local};
  for (int jbeg : ends)
    for (int jend : ends) {
      if (jbeg > ntile_local || jend > ntile_local) continue;
      std::vector<int> want;
      for (int j = jbeg; j < jend; ++j)
        if (lit(r0, j) || lit(r1, j)) want.push_back(j);
      // the walk, as the kernels run it: one window of bits, refilled when the walk leaves it
      int cur_w = -1, fills = 0;
      uint64_t word = 0, own = 0;
      auto fill = [&](int w) {
        ++fills;
        own = bm_word(r0.data(), nk, k_blk0, w);
        return bm_union(own, bm_word(r1.data(), nk, k_blk0, w));
      };
      std::vector<int> got;
      std::vector<int> stage;
      for (int j = bm_next_visited(fill, cur_w, word, jbeg, jend); j < jend; j = bm_next_visited(fill, cur_w, word, j + 1, jend)) {
        CHECK(bm_tile_lit(own, cur_w, j) == lit(r0, j));        // this wave's own activity comes from the current window
        stage.push_back(bm_stage((int)got.size(), 2));
        got.push_back(j);
        CHECK(got.size() <= want.size());
      }
      CHECK(got == want);
      for (size_t i = 1; i < stage.size(); ++i) CHECK(stage[i] != stage[i - 1]);   // consecutive visited tiles never share a stage
      CHECK(fills <= nwin + 1);
      // count, next and previous inside each window
      int cnt = 0;
      for (int w = 0; w < nwin; ++w) {
        const uint64_t u = bm_union(bm_word(r0.data(), nk, k_blk0, w), bm_word(r1.data(), nk, k_blk0, w));
        cnt += bm_count_tiles(u, w, jbeg, jend);
        for (int j = 128 * w - 2; j < 128 * w + 130; ++j) {
          int nx = -1, pv = -1;
          for (int t = (j > 128 * w ? j : 128 * w); t < 128 * w + 128 && t < jend; ++t)
            if (t >= 0 && (lit(r0, t) || lit(r1, t))) { nx = t; break; }
          for (int t = (j < 128 * w + 127 ? j : 128 * w + 127); t >= 128 * w && t >= jbeg; --t)
            if (lit(r0, t) || lit(r1, t)) { pv = t; break; }
          if (j >= 0) CHECK(bm_next_tile(u, w, j, jend) == nx);
          if (j >= 0) CHECK(bm_prev_tile(u, w, j, jbeg) == pv);
        }
      }
      CHECK(cnt == (int)want.size());
      ++n_ok;
    }
}

// ---- dK/dV: a column, (tile, head) items ------------------------------------------------------------------------------------------
static void check_items(int nqb, int G, int hstride_on, int jt0, int jt1, int density, int64_t k_blk0, int nk, int kb) {
  // mask (G or 1 heads, nqb query blocks, nk columns), bytes exactly that many
  const int Hm = hstride_on ? G : 1;
  std::vector<uint8_t> m((size_t)Hm * nqb * nk);
  for (auto& x : m) x = ((int)(rnd() % 100) < density) ? (uint8_t)(1 + rnd() % 255) : 0;
  const int64_t hs = hstride_on ? (int64_t)nqb * nk : 0, rs = nk;
  const int Gp = bm_gp(G);
  CHECK(Gp >= G && Gp < 2 * G + (G == 0) && (Gp & (Gp - 1)) == 0 && Gp <= 64);
  const BmCol col = bm_col(m.data(), hs, rs, nqb, nk, k_blk0, kb);
  const int64_t c = k_blk0 + kb;
  auto lit = [&](int j, int g) { return c >= 0 && c < nk && j >= jt0 && j < jt1 && m[(size_t)(g * hs + (j / 2) * rs + c)] != 0; };
  std::vector<BmItem> want;                       // tiles downward, the heads of a tile upward
  for (int j = jt1 - 1; j >= jt0; --j)
    for (int g = 0; g < G; ++g)
      if (lit(j, g)) want.push_back(BmItem{j, g});
  const int per = 64 / Gp;
  int cnt = 0;
  for (int wq = (jt0 >> 1) / per; 2 * wq * per < jt1; ++wq)
    cnt += bm_item_count(bm_item_word(col, G, Gp, wq, 0, jt0, jt1), bm_item_word(col, G, Gp, wq, 1, jt0, jt1));
  CHECK(cnt == (int)want.size());
  for (int nsplit = 1; nsplit <= 4; ++nsplit) {
    std::vector<int> owner(want.size(), -1);
    for (int s = 0; s < nsplit; ++s) {
      int cur_w = -1;
      uint64_t we = 0, wo = 0;
      auto fill = [&](int wq, uint64_t& e, uint64_t& o) {
        e = bm_item_word(col, G, Gp, wq, 0, jt0, jt1);
        o = bm_item_word(col, G, Gp, wq, 1, jt0, jt1);
      };
      // share s: skip s + 1 items from the start, then every nsplit-th
      BmItem it = bm_item_prev_n(fill, cur_w, we, wo, Gp, bm_walk_start(jt1), 64, jt0, s + 1);
      size_t i = (size_t)s;
      while (it.j >= 0) {
        CHECK(i < want.size());
        CHECK(it.j == want[i].j && it.g == want[i].g);
        CHECK(owner[i] == -1);
        owner[i] = s;
        it = bm_item_prev_n(fill, cur_w, we, wo, Gp, it.j, it.g, jt0, nsplit);
        i += (size_t)nsplit;
      }
      CHECK(i >= want.size());
    }
    for (size_t i = 0; i < want.size(); ++i) CHECK(owner[i] == (int)(i % (size_t)nsplit));
  }
  ++n_ok;
}

int main() {
  // k_blk0 negative, unaligned to the word size, partly and wholly outside [0, nk)
  const int64_t k0s[] = {0, 1, 63, 65, -1, -64, -70, -200, 500};
  for (int nk : {1, 7, 65, 130})
    for (int64_t k0 : k0s)
      for (int ntile : {1, 3, 16, 259})
        for (int pattern = 0; pattern < 6; ++pattern)
          for (int density : {8, 50})
            if (pattern == 0 || density == 8) check_rows(nk, k0, ntile, pattern, density);
  // visited lists of length 0, 1, 2, 3 and ring depth + 1 (= 3) are among the above (patterns 2, 3, 4 with small tile counts);
  // pin them explicitly on one geometry
  for (int len = 0; len <= 3; ++len) {
    std::vector<uint8_t> r(8, 0);
    // tiles 2c, 2c + 1 per lit column c; a band range that cuts the list to `len` tiles
    r[1] = 1;
    r[6] = 1;
    int cur_w = -1;
    uint64_t word = 0;
    auto fill = [&](int w) { return bm_word(r.data(), 8, 0, w); };
    const int jend = len == 0 ? 2 : (len == 1 ? 3 : (len == 2 ? 4 : 13));
    int n = 0;
    for (int j = bm_next_visited(fill, cur_w, word, 0, jend); j < jend; j = bm_next_visited(fill, cur_w, word, j + 1, jend)) ++n;
    CHECK(n == len);
    ++n_ok;
  }
  for (int G : {1, 2, 4, 3, 8, 64})
    for (int per_head = 0; per_head < 2; ++per_head)
      for (int nqb : {1, 5, 33, 70})
        for (int density : {0, 10, 100})
          for (int64_t k0 : {(int64_t)0, (int64_t)-2, (int64_t)3})
            for (int kb : {0, 5}) {
              const int nt = 2 * nqb;
              const int ranges[][2] = {{0, nt}, {0, nt - 1}, {1, nt}, {nt / 2, nt}, {nt / 2 + 1, nt / 2 + 1}, {3 < nt ? 3 : 0, nt}};
              for (auto& rg : ranges) check_items(nqb, G, per_head, rg[0], rg[1], density, k0, 5, kb);
            }
  std::printf("%lld configurations ok\n", n_ok);
  return 0;
}
