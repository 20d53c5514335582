// rfa_blockmask.h — the bit addressing and walk arithmetic of block-sparse masks (rfa.h: rfa_blockmask_args), shared by the
// forward, dQ and dK/dV kernels and the host-side check (tests/native/blockmask_check.cpp).
//
// The mask is one byte per (query block, key block) pair of 128 x 128 positions, non-zero = lit.  Its columns are the key
// blocks of the whole (unsharded) sequence; a block call's key row 0 sits in column k_blk0, so block-relative key block kb
// is column k_blk0 + kb, and a column outside [0, nk_blocks) is dark.  The kernels never hold a whole row or column: they
// keep a WINDOW of 64 bits in scalar registers (a ballot of bm_lit / bm_item_lit over the wave's lanes) and refill it when
// the walk leaves it; everything below works on such windows, so that the host can check it bit for bit.
//
// What the kernels call: bm_lit, bm_union, bm_tile_lit, bm_next_tile (through bm_next_visited) in the forward and dQ kernels;
// bm_gp, bm_col, bm_item_lit, bm_item_count, bm_item_prev_in (through bm_item_prev), bm_walk_start in the dK/dV kernel.  The
// kernels make their windows with a ballot where the host makes them with bm_word / bm_item_word (the same predicate per bit).
// bm_prev_tile, bm_count_tiles, bm_stage and bm_item_prev_n (shares of a column: no kernel has them yet) are used by NO kernel:
// the host check covers their arithmetic, not a device path.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RFA_BM_HD __host__ __device__ inline
#else
#define RFA_BM_HD inline
#endif

namespace rfa {

constexpr int kBmBlock = 128;        // positions per mask block, both ways
constexpr int kBmTile = 64;          // the kernels' tile: key tiles of the forward / dQ walk, Q/dO tiles of the dK/dV walk
constexpr int kBmWinTiles = 128;     // key tiles a forward / dQ window covers (64 key blocks)

RFA_BM_HD int bm_ctz(uint64_t x) { return __builtin_ctzll(x); }
RFA_BM_HD int bm_top(uint64_t x) { return 63 - __builtin_clzll(x); }
RFA_BM_HD int bm_popc(uint64_t x) { return __builtin_popcountll(x); }

// ---- forward / dQ: one mask row (a query block), key tiles walked upward ------------------------------------------------------
// is block-relative key block kb lit in the mask row `row` (nk_blocks bytes)?
RFA_BM_HD bool bm_lit(const uint8_t* row, int nk_blocks, int64_t k_blk0, int kb) {
  const int64_t c = k_blk0 + kb;
  return c >= 0 && c < (int64_t)nk_blocks && row[c] != 0;
}
// window w of a row: bit i = key block 64 w + i (the kernels: a ballot of bm_lit with i = lane)
RFA_BM_HD uint64_t bm_word(const uint8_t* row, int nk_blocks, int64_t k_blk0, int w) {
  uint64_t m = 0;
  for (int i = 0; i < 64; ++i)
    if (bm_lit(row, nk_blocks, k_blk0, 64 * w + i)) m |= 1ull << i;
  return m;
}
// a 256-row workgroup holds two query blocks: it visits what either of them sees
RFA_BM_HD uint64_t bm_union(uint64_t a, uint64_t b) { return a | b; }
// is key tile j (inside window w) lit?
RFA_BM_HD bool bm_tile_lit(uint64_t word, int w, int j) { return (j >> 7) == w && ((word >> ((j >> 1) & 63)) & 1ull) != 0; }
// the first visited tile >= j and < jend inside window w (tiles 128 w .. 128 w + 127); none: -1
RFA_BM_HD int bm_next_tile(uint64_t word, int w, int j, int jend) {
  const int base = w * kBmWinTiles;
  if (j < base) j = base;
  if (j >= base + kBmWinTiles || j >= jend) return -1;
  const uint64_t rest = word >> ((j - base) >> 1);
  if (!rest) return -1;
  const int t = 2 * (((j - base) >> 1) + bm_ctz(rest)) + base;      // the lit block's first tile
  const int r = t > j ? t : j;                                       // (j may be the second tile of its block)
  return r < jend ? r : -1;
}
// the last visited tile <= j and >= jbeg inside window w; none: -1
RFA_BM_HD int bm_prev_tile(uint64_t word, int w, int j, int jbeg) {
  const int base = w * kBmWinTiles;
  if (j >= base + kBmWinTiles) j = base + kBmWinTiles - 1;
  if (j < base || j < jbeg) return -1;
  const int kb = (j - base) >> 1;
  const uint64_t rest = kb == 63 ? word : word & ((1ull << (kb + 1)) - 1);
  if (!rest) return -1;
  const int t = 2 * bm_top(rest) + 1 + base;                         // the lit block's second tile
  const int r = t < j ? t : j;
  return r >= jbeg ? r : -1;
}
// visited tiles in [j0, j1) inside window w
RFA_BM_HD int bm_count_tiles(uint64_t word, int w, int j0, int j1) {
  const int base = w * kBmWinTiles;
  if (j0 < base) j0 = base;
  if (j1 > base + kBmWinTiles) j1 = base + kBmWinTiles;
  if (j1 <= j0) return 0;
  const int a = j0 - base, b = j1 - base;                            // tiles [a, b) of the window
  const int ka = (a + 1) >> 1, kb = b >> 1;                          // key blocks wholly inside: [ka, kb)
  int n = 0;
  if (kb > ka) {
    uint64_t m = word >> ka;
    if (kb - ka < 64) m &= (1ull << (kb - ka)) - 1;
    n = 2 * bm_popc(m);
  }
  if (a & 1) n += (int)((word >> (a >> 1)) & 1ull);                  // the second tile of a's block
  if (b & 1) n += (int)((word >> (b >> 1)) & 1ull);                  // the first tile of b's block
  return n;
}
// the walk across windows: the first visited tile >= j and < jend, or jend.  fill(w) makes window w current and returns its
// word (the union of the workgroup's rows); cur_w / word are the walk's state (cur_w = -1: nothing loaded yet).
template <class Fill>
RFA_BM_HD int bm_next_visited(Fill&& fill, int& cur_w, uint64_t& word, int j, int jend) {
  while (j < jend) {
    const int w = j >> 7;
    if (w != cur_w) {
      word = fill(w);
      cur_w = w;
    }
    const int r = bm_next_tile(word, w, j, jend);
    if (r >= 0) return r;
    j = (w + 1) * kBmWinTiles;
  }
  return jend;
}
// the LDS ring stage of a visited tile: its POSITION in the visited list, not its index
RFA_BM_HD int bm_stage(int pos, int depth) { return pos % depth; }

// ---- dK/dV: one mask column (a key block), (Q/dO tile, query head) items walked downward --------------------------------------
// The workgroup of a key block serves the G query heads of its K/V head.  A window holds 64 / Gp query blocks (Gp: G rounded
// up to a power of two, at most 64) as bit qo * Gp + g, in two words: `we` the even Q/dO tile of each query block, `wo` the
// odd one — the band's tile range [jt0, jt1) is folded into the bits, so the walk needs no range of its own.
RFA_BM_HD int bm_gp(int G) {
  int gp = 1;
  while (gp < G) gp <<= 1;
  return gp;
}
struct BmCol {
  const uint8_t* base;          // mask[b, h0 (or 0), 0, column]
  int64_t hstride, rstride;     // bytes between two heads (0: shared) and two query blocks
  int nqb;                      // query blocks of the call
  bool ok;                      // the column lies inside [0, nk_blocks)
};
RFA_BM_HD BmCol bm_col(const uint8_t* mask_bh, int64_t hstride, int64_t rstride, int nqb, int nk_blocks, int64_t k_blk0, int kb) {
  const int64_t c = k_blk0 + kb;
  const bool ok = c >= 0 && c < (int64_t)nk_blocks;
  return BmCol{mask_bh + (ok ? c : 0), hstride, rstride, nqb, ok};
}
// bit `lane` of window wq, tile parity 0 / 1
RFA_BM_HD bool bm_item_lit(const BmCol& c, int G, int Gp, int wq, int lane, int parity, int jt0, int jt1) {
  const int qb = wq * (64 / Gp) + lane / Gp, g = lane % Gp;
  const int j = 2 * qb + parity;
  return c.ok && g < G && qb < c.nqb && j >= jt0 && j < jt1 && c.base[(int64_t)g * c.hstride + (int64_t)qb * c.rstride] != 0;
}
RFA_BM_HD uint64_t bm_item_word(const BmCol& c, int G, int Gp, int wq, int parity, int jt0, int jt1) {
  uint64_t m = 0;
  for (int i = 0; i < 64; ++i)
    if (bm_item_lit(c, G, Gp, wq, i, parity, jt0, jt1)) m |= 1ull << i;
  return m;
}
RFA_BM_HD int bm_item_count(uint64_t we, uint64_t wo) { return bm_popc(we) + bm_popc(wo); }
struct BmItem {
  int j, g;                     // Q/dO tile and head in the group; j < 0: none
};
RFA_BM_HD uint64_t bm_field(uint64_t w, int Gp, int qo) { return Gp >= 64 ? w : (w >> (qo * Gp)) & ((1ull << Gp) - 1); }
// the item behind (j, g) in walk order — tiles downward, the heads of a tile upward — inside window wq.  (j, g) need not be
// lit; j = 2 * (wq + 1) * (64 / Gp) (one above the window) starts at the window's top.  None left in the window: j = -1.
RFA_BM_HD BmItem bm_item_prev_in(uint64_t we, uint64_t wo, int Gp, int wq, int j, int g) {
  const int per = 64 / Gp;
  const int qo = (j >> 1) - wq * per;                                // 0 .. per (per: above the window)
  if (qo < per) {
    uint64_t f = bm_field((j & 1) ? wo : we, Gp, qo);
    const uint64_t rest = g + 1 < 64 ? f >> (g + 1) : 0;             // the tile's higher heads
    if (rest) return BmItem{j, g + 1 + bm_ctz(rest)};
    if (j & 1) {                                                     // the query block's even tile
      f = bm_field(we, Gp, qo);
      if (f) return BmItem{j - 1, bm_ctz(f)};
    }
  }
  const int sh = qo * Gp;                                            // the query blocks below
  const uint64_t below = sh >= 64 ? ~0ull : (1ull << sh) - 1;
  const uint64_t any = (we | wo) & below;
  if (!any) return BmItem{-1, 0};
  const int q2 = bm_top(any) / Gp;
  uint64_t f = bm_field(wo, Gp, q2);
  int jj = 2 * (wq * per + q2) + 1;
  if (!f) {
    f = bm_field(we, Gp, q2);
    --jj;
  }
  return BmItem{jj, bm_ctz(f)};
}
// the walk across windows: the item behind (j, g), or j = -1.  fill(wq, we, wo) loads window wq; cur_w / we / wo are the walk's
// state.  Start: j = the first even number >= jt1, g = 64.
template <class Fill>
RFA_BM_HD BmItem bm_item_prev(Fill&& fill, int& cur_w, uint64_t& we, uint64_t& wo, int Gp, int j, int g, int jt0) {
  const int per = 64 / Gp;
  int wq = (j >> 1) / per;
  for (;;) {
    if (wq != cur_w) {
      fill(wq, we, wo);
      cur_w = wq;
    }
    const BmItem it = bm_item_prev_in(we, wo, Gp, wq, j, g);
    if (it.j >= 0) return it;
    if (2 * wq * per <= jt0) return BmItem{-1, 0};                   // nothing of the band lies below this window
    j = 2 * wq * per;                                                // one above the window below
    g = 64;
    --wq;
  }
}
// a launch that shares a key block between nsplit workgroups deals every nsplit-th VISITED item: share s takes the items
// s, s + nsplit, ... of the walk
template <class Fill>
RFA_BM_HD BmItem bm_item_prev_n(Fill&& fill, int& cur_w, uint64_t& we, uint64_t& wo, int Gp, int j, int g, int jt0, int n) {
  BmItem it{j, g};
  for (int i = 0; i < n && it.j >= 0; ++i) it = bm_item_prev(fill, cur_w, we, wo, Gp, it.j, it.g, jt0);
  return it;
}
RFA_BM_HD int bm_walk_start(int jt1) { return (jt1 + 1) & ~1; }

}  // namespace rfa
