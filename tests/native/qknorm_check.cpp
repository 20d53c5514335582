// qknorm_check.cpp — stand-alone host check of the index arithmetic of the fused QK RMSNorm + rotary kernels
// (csrc/rfa_qknorm_index.h), on the very header the kernels include.  Built by tests/test_qk_norm_cpu.py with
// -fsanitize=address,undefined and run; no GPU, no HIP.  Against brute force, for every configuration of the grid below:
//   the lane-group size (smallest power of two >= D/8, dividing 256, at most 32)
//   every chunk's element offsets on the three sides (input, written tensor, incoming gradient), inside their buffers
//   every column of every (row, head) is owned by exactly one live lane — in the forward's grid and in the backward's walk
//   every lane's role, partner lane and table columns, column by column
//   the LDS index of the weight gradient fold, the partial count, the walk length, the fold runs and the workspace size
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "rfa_qknorm_index.h"

using namespace rfa;

static long g_configs = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      fprintf(stderr, "FAILED %s: ", #cond);              \
      fprintf(stderr, __VA_ARGS__);                       \
      fprintf(stderr, "\n");                              \
      exit(1);                                            \
    }                                                     \
  } while (0)

static void check_group(uint32_t D) {
  const uint32_t G = qknorm_group(D);
  uint32_t want = 1;
  while (want < D / 8) want *= 2;
  CHECK(G == want && G >= D / 8 && G <= 32 && kQkNormThreads % G == 0 && (G == 1 || G / 2 < D / 8), "D %u G %u", D, G);
  // the LDS image of the weight gradient fold: (256/G) groups x D columns inside 256 * 8 floats
  CHECK((kQkNormThreads / G) * D <= (uint32_t)kQkNormThreads * 8, "D %u", D);
}

static void check_lanes(const QkNormGeom& g) {
  std::vector<int> owner(g.D, 0);
  for (uint32_t w = 0; w < g.group; ++w) {
    QkNormLane l;
    qknorm_lane(g, w, &l);
    if (w >= g.chunks) {
      CHECK(l.kind == kQkNormPass && l.partner == w, "idle lane %u", w);
      continue;
    }
    CHECK(l.col == 8 * w && l.partner < g.chunks, "lane %u", w);
    QkNormLane pl;
    qknorm_lane(g, l.partner, &pl);
    CHECK(pl.partner == w, "partner of partner, lane %u", w);
    for (uint32_t e = 0; e < 8; ++e) {
      const uint32_t c = l.col + e;
      CHECK(c < g.D, "column");
      owner[c]++;
      const bool rotated = g.R && c >= g.rot_off && c < g.rot_off + g.R;
      if (!rotated) {
        CHECK(l.kind == kQkNormPass && l.partner == w, "pass column %u", c);
      } else if (g.interleaved) {
        CHECK(l.kind == kQkNormInterleaved && l.partner == w, "gptj column %u", c);
        CHECK(l.tcol + e / 2 == (c - g.rot_off) / 2 && l.tcol % 4 == 0 && l.tcol + 4 <= g.R / 2, "gptj table column %u", c);
        CHECK(((c - g.rot_off) ^ 1u) / 8 == (c - g.rot_off) / 8, "gptj pair inside the chunk");
      } else if (c - g.rot_off < g.R / 2) {
        CHECK(l.kind == kQkNormLo && 8 * l.partner + e == c + g.R / 2, "lo column %u", c);
        CHECK(l.tcol + e == c - g.rot_off && l.tcol + 8 <= g.R / 2, "lo table column %u", c);
      } else {
        CHECK(l.kind == kQkNormHi && 8 * l.partner + e == c - g.R / 2, "hi column %u", c);
        CHECK(l.tcol + e == c - g.rot_off - g.R / 2 && l.tcol + 8 <= g.R / 2, "hi table column %u", c);
      }
    }
  }
  for (uint32_t c = 0; c < g.D; ++c) CHECK(owner[c] == 1, "column %u owned %d times", c, owner[c]);
}

static void check_walk(uint32_t items, uint32_t G, bool enumerate) {
  const uint32_t per = kQkNormThreads / G;
  const uint64_t want_blocks = ((uint64_t)items + per - 1) / per;
  CHECK(qknorm_blocks(items, G) == want_blocks, "blocks");
  const uint32_t nparts = qknorm_parts(items, G);
  CHECK(nparts == (want_blocks < (uint64_t)kQkNormMaxParts ? want_blocks : (uint64_t)kQkNormMaxParts), "parts");
  const uint32_t walk = qknorm_walk(items, nparts, G);
  if (items == 0) {
    CHECK(nparts == 0 && walk == 0, "empty");
    return;
  }
  CHECK((uint64_t)walk * nparts * per >= items && (uint64_t)(walk - 1) * nparts * per < items, "walk %u", walk);
  const uint32_t len = qknorm_fold_len(nparts);
  CHECK((uint64_t)len * kQkNormFoldSlices >= nparts && (uint64_t)(len - 1) * kQkNormFoldSlices < nparts, "fold runs");
  CHECK(qknorm_workspace_bytes(2, nparts, 256) == (int64_t)2 * nparts * 256 * 4, "workspace");
  if (!enumerate) return;
  std::vector<uint8_t> seen(items, 0);
  for (uint32_t it = 0; it < walk; ++it)
    for (uint32_t p = 0; p < nparts; ++p)
      for (uint32_t grp = 0; grp < per; ++grp) {
        const uint64_t item = ((uint64_t)it * nparts + p) * per + grp;
        if (item < items) seen[item]++;
      }
  for (uint32_t i = 0; i < items; ++i) CHECK(seen[i] == 1, "item %u walked %d times", i, seen[i]);
  // the fold's runs cover every partial once
  std::vector<uint8_t> part(nparts, 0);
  for (uint32_t j = 0; j < (uint32_t)kQkNormFoldSlices; ++j)
    for (uint32_t q = j * len; q < nparts && q < (j + 1) * len; ++q) part[q]++;
  for (uint32_t q = 0; q < nparts; ++q) CHECK(part[q] == 1, "partial %u folded %d times", q, part[q]);
}

// one tensor with padded strides on every side: offsets against the plain formula, inside the buffers, every element once
static void check_offsets(const QkNormGeom& g, uint32_t H, int64_t pad) {
  QkNormTensor t{};
  t.H = H;
  t.nitems = g.B * g.S * H;
  t.xh = g.D + pad; t.xr = t.xh * H + pad; t.xb = t.xr * g.S + pad;
  t.oh = g.D; t.orow = t.oh * H; t.ob = t.orow * g.S;
  t.gh = g.D + 2 * pad; t.gr = t.gh * (H + 1); t.gb = t.gr * (g.S + 2);
  const int64_t xn = t.xb * g.B, on = t.ob * g.B, gn = t.gb * g.B;
  std::vector<uint8_t> xs(xn, 0), os(on, 0), gs(gn, 0);
  const uint32_t per = kQkNormThreads / g.group, blocks = qknorm_blocks(t.nitems, g.group);
  for (uint32_t blk = 0; blk < blocks; ++blk)
    for (uint32_t tid = 0; tid < (uint32_t)kQkNormThreads; ++tid) {
      const uint32_t w = tid & (g.group - 1), item = blk * per + tid / g.group;
      if (item >= t.nitems || w >= g.chunks) continue;
      QkNormChunk c;
      qknorm_chunk(g, t, item, w, &c);
      CHECK(c.b < g.B && c.i < g.S && c.h < H && (c.b * g.S + c.i) * H + c.h == item, "item %u", item);
      CHECK(c.x == (int64_t)c.b * t.xb + (int64_t)c.i * t.xr + (int64_t)c.h * t.xh + 8 * w, "x offset");
      CHECK(c.o == (int64_t)c.b * t.ob + (int64_t)c.i * t.orow + (int64_t)c.h * t.oh + 8 * w, "o offset");
      CHECK(c.g == (int64_t)c.b * t.gb + (int64_t)c.i * t.gr + (int64_t)c.h * t.gh + 8 * w, "g offset");
      CHECK(c.x >= 0 && c.x + 8 <= xn && c.o >= 0 && c.o + 8 <= on && c.g >= 0 && c.g + 8 <= gn, "bounds");
      CHECK(c.x % 8 == 0 || pad % 8, "alignment");
      for (int e = 0; e < 8; ++e) {
        xs[c.x + e]++;
        os[c.o + e]++;
        gs[c.g + e]++;
      }
    }
  for (int64_t i = 0; i < on; ++i) CHECK(os[i] == 1, "output element %lld written %d times", (long long)i, os[i]);
  int64_t nx = 0, ng = 0;
  for (int64_t i = 0; i < xn; ++i) {
    CHECK(xs[i] <= 1, "input element read twice");
    nx += xs[i];
  }
  for (int64_t i = 0; i < gn; ++i) {
    CHECK(gs[i] <= 1, "gradient element read twice");
    ng += gs[i];
  }
  CHECK(nx == on && ng == on, "elements read");
}

int main() {
  for (uint32_t D = 8; D <= 256; D += 8) {
    check_group(D);
    for (int inter = 0; inter < 2; ++inter) {
      const uint32_t step = inter ? 8 : 16;
      for (uint32_t R = 0; R <= D; R += step)
        for (uint32_t ro = 0; ro + R <= D; ro += 8) {
          if (R == 0 && (ro || inter)) continue;
          if (D > 64 && (ro % 32 || R % 32) && ro + R != D) continue;      // (thinned above 64 columns)
          QkNormGeom g{};
          g.B = 2; g.S = 3; g.D = D; g.R = R; g.rot_off = ro; g.interleaved = inter;
          g.chunks = D / 8; g.group = qknorm_group(D);
          check_lanes(g);
          check_offsets(g, 3, 8);
          if (ro == 0) check_offsets(g, 1, 0);
          ++g_configs;
        }
    }
  }
  // the partial count and the walk over a sweep of item counts, for every group size
  const uint32_t counts[] = {0, 1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 4200, 8191, 8192, 8193, 32767, 32768, 32769, 262144, 300001};
  for (uint32_t G = 1; G <= 32; G *= 2) {
    for (uint32_t n : counts) {
      check_walk(n, G, true);
      ++g_configs;
    }
    const uint32_t big[] = {1u << 24, (1u << 31) - 1};
    for (uint32_t n : big) {
      check_walk(n, G, false);
      ++g_configs;
    }
  }
  // a far stride: offsets are 64-bit
  {
    QkNormGeom g{};
    g.B = 1; g.S = 3; g.D = 64; g.chunks = 8; g.group = 8;
    QkNormTensor t{};
    t.H = 1; t.nitems = 3; t.xr = (1ll << 31) + 4096; t.orow = 64; t.gr = (1ll << 33);
    QkNormChunk c;
    qknorm_chunk(g, t, 2, 7, &c);
    CHECK(c.x == 2 * ((1ll << 31) + 4096) + 56 && c.o == 128 + 56 && c.g == (1ll << 34) + 56, "far offsets");
    ++g_configs;
  }
  printf("%ld configurations ok\n", g_configs);
  return 0;
}
