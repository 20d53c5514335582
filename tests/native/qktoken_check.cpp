// qktoken_check.cpp — stand-alone host check of the index arithmetic of the token-wide QK RMSNorm + rotary kernels
// (ring-flash-attention_amd/csrc/rfa_qktoken_index.h: the very functions the gfx950 kernels use).  No GPU, no HIP:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ring-flash-attention_amd/csrc tests/native/qktoken_check.cpp
// Against brute force, over H x D up to 16384 columns, both pairings, padded permuted strides: the team (a function of N alone,
// <= 8 chunks a lane, <= 32 KiB of row copies in flight) and its lanes' chunks covering the row once; a chunk's head, column,
// element offset (every element once, padding never), kind, partner (mutual, same head, R/2 columns away) and table columns;
// every row visited once forward and backward; the partial count, the workspace size and the fold's runs.
// Exit status 0 and "qktoken_check: N configurations ok" on success; the first failure is printed and the status is 1.
#include <cstdio>
#include <vector>

#include "rfa_qktoken_index.h"

using namespace rfa;

static int check(int H, int D, int R, int ro, int inter, int B, int S) {
#define REQUIRE(cond, what) do { if (!(cond)) { std::printf("qktoken_check: FAILED: %s (H %d D %d R %d rot_offset %d interleaved %d B %d S %d)\n", what, H, D, R, ro, inter, B, S); return 1; } } while (0)
  const uint32_t N = (uint32_t)H * D, C = N / 8;
  QkTokenGeom g{};
  g.B = B; g.S = S; g.D = D; g.R = R; g.rot_off = ro; g.interleaved = inter; g.hchunks = D / 8;
  const uint32_t team = qktoken_team(N), per = qktoken_per_lane(N), slots = qktoken_slots(team);
  REQUIRE(team == 64 || team == 128 || team == 256, "team size");
  REQUIRE(team == (C <= 128 ? 64u : C <= 512 ? 128u : 256u), "team is a function of N");
  REQUIRE(per >= 1 && per <= kQkTokenMaxPerLane && per * team >= C && (per - 1) * team < C, "chunks per lane");
  REQUIRE(slots * team == kQkTokenThreads && (uint64_t)slots * C * 16 <= 32768, "rows in flight fit 32 KiB");
  REQUIRE(slots == 1 || (uint64_t)(slots - 1) * N * 4 <= 32768, "the teams' dw hand-over fits the staging buffer");
  // the lanes' chunks cover the row once
  std::vector<int> owner(C, 0);
  for (uint32_t l = 0; l < team; ++l)
    for (uint32_t j = 0; j < per; ++j)
      if (l + j * team < C) ++owner[l + j * team];
  for (uint32_t c = 0; c < C; ++c) REQUIRE(owner[c] == 1, "a chunk has one owner");
  // strides: head-major padded storage (b, h, i, D + 8), as a permuted view gives it
  const int64_t sh = (int64_t)S * (D + 8), sr = D + 8, sb = (int64_t)H * sh;
  std::vector<int> seen((size_t)B * sb, 0);
  for (uint32_t row = 0; row < (uint32_t)(B * S); ++row) {
    for (uint32_t c = 0; c < C; ++c) {
      QkTokenRole r{};
      qktoken_role(g, c, &r);
      REQUIRE(r.head == c / (D / 8) && r.col == 8 * (c % (D / 8)) && r.head < (uint32_t)H && r.col + 8 <= (uint32_t)D, "head and column");
      const int64_t off = qktoken_offset(g, row, r.head, r.col, sb, sr, sh);
      const int64_t want = (int64_t)(row / S) * sb + (int64_t)r.head * sh + (int64_t)(row % S) * sr + r.col;
      REQUIRE(off == want && off >= 0 && off + 8 <= (int64_t)seen.size(), "element offset");
      for (int e = 0; e < 8; ++e) ++seen[off + e];
      if (row) continue;
      // the role, by the definition of the pairings
      const int col = (int)r.col;
      const bool rotated = R > 0 && col >= ro && col < ro + R;
      if (!rotated) {
        REQUIRE(r.kind == kQkTokenPass && r.partner == c, "pass-through chunk");
      } else if (inter) {
        REQUIRE(r.kind == kQkTokenInterleaved && r.partner == c && (int)r.tcol == (col - ro) / 2 && (int)r.tcol + 4 <= R / 2,
                "interleaved chunk");
      } else {
        const bool lo = col < ro + R / 2;
        REQUIRE(r.kind == (lo ? kQkTokenLo : kQkTokenHi), "halves kind");
        REQUIRE((int64_t)r.partner * 8 == (int64_t)c * 8 + (lo ? R / 2 : -(R / 2)) && r.partner < C, "halves partner");
        QkTokenRole pr{};
        qktoken_role(g, r.partner, &pr);
        REQUIRE(pr.head == r.head && pr.partner == c && pr.tcol == r.tcol && pr.kind == (lo ? kQkTokenHi : kQkTokenLo), "partners are mutual");
        REQUIRE((int)r.tcol == (lo ? col - ro : col - ro - R / 2) && (int)r.tcol + 8 <= R / 2, "halves table columns");
      }
    }
  }
  for (uint32_t b = 0; b < (uint32_t)B; ++b)
    for (int h = 0; h < H; ++h)
      for (int i = 0; i < S; ++i)
        for (int d = 0; d < D + 8; ++d)
          REQUIRE(seen[b * sb + h * sh + i * sr + d] == (d < D ? 1 : 0), "every element once, padding never");
  return 0;
#undef REQUIRE
}

// the backward's walk, the partial count and the fold for row counts around the cap
static int check_walk(uint32_t rows, uint32_t N) {
  const uint32_t team = qktoken_team(N), slots = qktoken_slots(team);
  const uint32_t nparts = qktoken_parts(rows, team), walk = qktoken_walk(rows, nparts, team);
  const uint32_t want = (rows + slots - 1) / slots;
  bool ok = nparts == (want > (uint32_t)kQkTokenMaxParts ? (uint32_t)kQkTokenMaxParts : want) && nparts >= 1;
  ok = ok && (uint64_t)walk * nparts * slots >= rows && (uint64_t)(walk - 1) * nparts * slots < rows;
  ok = ok && qktoken_blocks(rows, team) == want;                // (the forward: workgroup p holds the rows p * slots + slot)
  for (uint32_t r = 0; r < rows && ok; ++r) ok = qktoken_row(0, 0, r / slots, r % slots, team) == r;
  std::vector<int> hit(rows, 0);
  for (uint32_t p = 0; p < nparts && ok; ++p)
    for (uint32_t it = 0; it < walk; ++it) {
      if (qktoken_row(it, nparts, p, 0, team) >= rows) break;    // (as the kernel leaves its walk)
      for (uint32_t s = 0; s < slots; ++s) {
        const uint64_t row = qktoken_row(it, nparts, p, s, team);
        if (row < rows) ++hit[row];
      }
    }
  for (uint32_t r = 0; r < rows && ok; ++r) ok = hit[r] == 1;
  ok = ok && qktoken_workspace_bytes(nparts, N) == (int64_t)nparts * N * 4;
  const uint32_t len = qktoken_fold_len(nparts);
  std::vector<int> folded(nparts, 0);
  for (uint32_t j = 0; j < (uint32_t)kQkTokenFoldSlices; ++j) {
    const uint32_t lo = j * len < nparts ? j * len : nparts, hi = lo + len < nparts ? lo + len : nparts;
    for (uint32_t q = lo; q < hi; ++q) ++folded[q];
  }
  for (uint32_t q = 0; q < nparts && ok; ++q) ok = folded[q] == 1;
  if (!ok) std::printf("qktoken_check: FAILED: walk / partials / fold (rows %u N %u nparts %u walk %u)\n", rows, N, nparts, walk);
  return ok ? 0 : 1;
}

int main() {
  static const int Hs[] = {1, 3, 4, 5, 8, 40, 64}, Ds[] = {8, 40, 64, 128, 256}, Bs[] = {1, 2}, Ss[] = {1, 5, 37};
  int n = 0;
  for (int H : Hs)
    for (int D : Ds) {
      if (H * D > kQkTokenMaxWidth) continue;
      // (R, rot_offset, interleaved): the norm alone, all of D, a part behind an offset — in both pairings where D allows
      const int rots[][3] = {{0, 0, 0}, {D % 16 ? 0 : D, 0, 0}, {D, 0, 1}, {D >= 40 ? 16 : 0, 8, 0}, {8, D - 8, 1}};
      for (const auto& r : rots)
        for (int B : Bs)
          for (int S : Ss) {
            if (H * D > 4096 && S > 5) continue;                 // (the wide rows: fewer of them)
            if (check(H, D, r[0], r[1], r[2], B, S)) return 1;
            ++n;
          }
    }
  static const uint32_t Ns[] = {8, 120, 1024, 1032, 4096, 4104, 16384};
  static const uint32_t rows[] = {1, 2, 3, 4, 5, 74, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2100, 4097, 8192, 100000};
  for (uint32_t N : Ns)
    for (uint32_t r : rows) {
      if (check_walk(r, N)) return 1;
      ++n;
    }
  std::printf("qktoken_check: %d configurations ok\n", n);
  return 0;
}
