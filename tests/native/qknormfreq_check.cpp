// qknormfreq_check.cpp — stand-alone host check of the index arithmetic of the per-head QK RMSNorm + rotary kernels that form
// their own angles (csrc/rfa_qknormfreq_index.h, with the tile, lane and LDS functions it takes from rfa_rotfreq_index.h and
// rfa_qknorm_index.h), on the very header the kernels include.  Built by tests/test_qk_norm_freqs_cpu.py with
// -fsanitize=address,undefined and run; no GPU, no HIP.  Against brute force, for every configuration of the grid below:
//   every (row, head, chunk) of q and k is visited exactly once by the forward's grid of tiles and by the backward's walk of
//     nparts workgroups, at the element offsets of the plain formula, inside the buffers
//   every LDS read of a rotating lane lands on the entry (tile row, frequency) the angle phase wrote there, inside the arrays
//   the pass count, the partial count, the walk and the workspace size
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "rfa_qknormfreq_index.h"

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

// what the angle phase leaves in an LDS array of `rows` rows: slot -> r * half + c (the entry), -1 = never written
static std::vector<int> angle_phase(uint32_t half, int inter, uint32_t nrows, uint32_t rows) {
  std::vector<int> lds(rows * kRotFreqMaxHalf, -1);
  for (uint32_t e = 0; e < nrows * half; ++e) {                // (entry e goes to thread e % 256: the order does not matter)
    const uint32_t r = e / half, c = e - r * half;
    const uint32_t at = r * half + rotfreq_lds_col(half, inter, c);
    CHECK(at < rows * half && lds[at] == -1, "LDS slot %u written twice or outside", at);
    lds[at] = (int)e;
  }
  return lds;
}

// one tile of one tensor as the workgroup walks it: every live lane's chunk counted in `seen`, its LDS reads checked
static void walk_tile(const QkNormGeom& g, const QkNormTensor& t, const RotFreqTile& tile, const std::vector<int>& lds,
                      std::vector<uint8_t>& seen, int64_t xn) {
  const uint32_t per = kQkNfThreads / g.group, half = g.R / 2;
  const uint32_t n = qknf_tile_items(tile.nrows, t.H), passes = qknf_passes(tile.nrows, t.H, g.group);
  CHECK((uint64_t)passes * per >= n && (passes == 0 || (uint64_t)(passes - 1) * per < n), "passes %u for %u items", passes, n);
  uint32_t steps = 0;
  for (uint32_t j0 = 0; j0 < n; j0 += per) {                   // (the kernels' loop)
    ++steps;
    for (uint32_t tid = 0; tid < (uint32_t)kQkNfThreads; ++tid) {
      const uint32_t w = tid & (g.group - 1), j = j0 + tid / g.group;
      if (w >= g.chunks || j >= n) continue;
      QkNormChunk c;
      qknf_chunk(t, tile, j, w, &c);
      CHECK(c.b == tile.b && c.i >= tile.row0 && c.i < tile.row0 + tile.nrows && c.i < g.S && c.h < t.H, "item %u", j);
      CHECK((c.i - tile.row0) * t.H + c.h == j, "item %u decoded", j);
      CHECK(c.x == (int64_t)c.b * t.xb + (int64_t)c.i * t.xr + (int64_t)c.h * t.xh + 8 * w, "x offset");
      CHECK(c.o == (int64_t)c.b * t.ob + (int64_t)c.i * t.orow + (int64_t)c.h * t.oh + 8 * w, "o offset");
      CHECK(c.g == (int64_t)c.b * t.gb + (int64_t)c.i * t.gr + (int64_t)c.h * t.gh + 8 * w, "g offset");
      CHECK(c.x >= 0 && c.x + 8 <= xn, "x bounds");
      seen[(((size_t)c.b * g.S + c.i) * t.H + c.h) * g.chunks + w]++;
      QkNormLane l;
      qknorm_lane(g, w, &l);
      if (l.kind == kQkNormPass) continue;
      const uint32_t r = c.i - tile.row0;
      for (uint32_t q = 0; q < (g.interleaved ? 1u : 2u); ++q) {
        const uint32_t at = qknf_lds_at(half, g.interleaved, r, l.tcol, q);
        CHECK(at % 4 == 0 && at + 4 <= (uint32_t)lds.size(), "LDS read at %u", at);
        for (uint32_t e = 0; e < 4; ++e)
          CHECK(lds[at + e] == (int)(r * half + l.tcol + 4 * q + e), "row %u table column %u: slot %u holds entry %d", r,
                l.tcol + 4 * q + e, at + e, lds[at + e]);
      }
    }
  }
  CHECK(steps == passes, "the loop runs %u passes, qknf_passes says %u", steps, passes);
}

static void check_config(uint32_t B, uint32_t S, uint32_t D, uint32_t R, uint32_t ro, int inter, uint32_t H, uint32_t Hk,
                         uint32_t rows) {
  QkNormGeom g{};
  g.B = B; g.S = S; g.D = D; g.R = R; g.rot_off = ro; g.interleaved = inter;
  g.chunks = D / 8; g.group = qknorm_group(D);
  const uint32_t heads[2] = {H, Hk};
  const uint32_t tiles = qknf_tiles(B, S, rows), per_batch = rotfreq_tiles_per_batch(S, rows);
  CHECK(tiles == B * ((S + rows - 1) / rows), "tiles");
  for (int bwd = 0; bwd < 2; ++bwd)
    for (int k = 0; k < 2; ++k) {
      if (!heads[k]) continue;
      QkNormTensor t{};
      t.H = heads[k];
      t.nitems = B * S * t.H;
      const int64_t pad = 8;                                   // padded strides on the input side
      t.xh = D + pad; t.xr = t.xh * t.H + pad; t.xb = t.xr * S + pad;
      t.oh = D; t.orow = t.oh * t.H; t.ob = t.orow * S;
      t.gh = D; t.gr = t.gh * t.H; t.gb = t.gr * S;
      std::vector<uint8_t> seen((size_t)t.nitems * g.chunks, 0);
      // forward: workgroup = tile; backward: workgroup p of nparts walks the tiles p, p + nparts, ..
      const uint32_t nparts = bwd ? qknf_parts(tiles) : tiles, walk = bwd ? qknf_walk(tiles, nparts) : 1;
      if (bwd && tiles) CHECK((uint64_t)walk * nparts >= tiles && (uint64_t)(walk - 1) * nparts < tiles, "walk %u", walk);
      for (uint32_t p = 0; p < nparts; ++p) {
        uint32_t visited = 0;
        for (uint32_t ti = p; ti < tiles; ti += nparts) {      // (the backward kernel's loop)
          ++visited;
          const RotFreqTile tile = rotfreq_tile(S, ti, rows);
          CHECK(tile.b == ti / per_batch && tile.row0 == (ti % per_batch) * rows && tile.nrows >= 1 && tile.nrows <= rows &&
                    tile.row0 + tile.nrows <= S && (tile.nrows == rows || tile.row0 + tile.nrows == S), "tile %u", ti);
          walk_tile(g, t, tile, angle_phase(R / 2, inter, tile.nrows, rows), seen, t.xb * B);
        }
        CHECK(visited <= walk && visited + 1 >= walk, "workgroup %u walks %u tiles of %u", p, visited, walk);
      }
      for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "chunk %zu visited %d times (bwd %d)", i, seen[i], bwd);
    }
  ++g_configs;
}

int main() {
  // D, R, rot_off, interleaved: full and partial rotation, idle lanes (72, 40), every group size
  const uint32_t geom[][4] = {{128, 128, 0, 0}, {64, 64, 0, 0}, {72, 32, 8, 0}, {256, 256, 0, 0}, {192, 64, 128, 0}, {40, 16, 8, 0},
                              {128, 128, 0, 1}, {72, 72, 0, 1}, {40, 8, 8, 1}, {256, 256, 0, 1}, {8, 8, 0, 1}, {16, 16, 0, 0}};
  // B, S: a ragged last tile, one row, whole tiles
  const uint32_t shape[][2] = {{2, 5}, {1, 1}, {3, 8}, {2, 4}, {1, 7}};
  // H, Hk (0: q alone): tile items that do not fill the lane groups, more than a pass
  const uint32_t heads[][2] = {{5, 1}, {1, 0}, {32, 8}, {3, 3}, {70, 1}};
  for (const auto& gm : geom)
    for (const auto& sh : shape)
      for (const auto& hd : heads) check_config(sh[0], sh[1], gm[0], gm[1], gm[2], (int)gm[3], hd[0], hd[1], kQkNfRows);
  // other tile heights use the same functions
  for (uint32_t rows : {1u, 2u, 8u}) check_config(2, 11, 128, 64, 32, 0, 5, 1, rows);
  // more tiles than partials: the walk
  check_config(1, 4 * kQkNfMaxParts + 9, 16, 16, 0, 0, 1, 1, kQkNfRows);
  CHECK(qknf_parts(0) == 0 && qknf_walk(0, 0) == 0 && qknf_parts(5) == 5 && qknf_parts(5000) == (uint32_t)kQkNfMaxParts, "parts");
  CHECK(qknf_walk(5000, kQkNfMaxParts) == 5 && qknf_walk(1024, 1024) == 1 && qknf_walk(1025, 1024) == 2, "walk");
  CHECK(qknorm_workspace_bytes(2, qknf_parts(qknf_tiles(2, 4100)), 128) == (int64_t)2 * 1024 * 128 * 4, "workspace");
  // a far stride: offsets are 64-bit
  {
    QkNormTensor t{};
    t.H = 2; t.xr = (1ll << 31) + 4096; t.xh = 64; t.orow = 128; t.oh = 64; t.gr = (1ll << 33); t.gh = 64;
    RotFreqTile tile = rotfreq_tile(7, 1, kQkNfRows);
    QkNormChunk c;
    qknf_chunk(t, tile, 5, 7, &c);                             // row 4 + 2, head 1
    CHECK(c.i == 6 && c.h == 1 && c.x == 6 * ((1ll << 31) + 4096) + 64 + 56 && c.o == 6 * 128 + 64 + 56 && c.g == 6 * (1ll << 33) + 64 + 56,
          "far offsets");
    ++g_configs;
  }
  printf("%ld configurations ok\n", g_configs);
  return 0;
}
