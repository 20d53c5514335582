// rotfreq_check.cpp — stand-alone host check of the tile / unit arithmetic of the rotary kernel that forms its own angles
// (csrc/rfa_rotfreq_index.h), meant to be built with -fsanitize=address,undefined (tests/test_rotary_freqs_cpu.py).  No device,
// no HIP.  Over a grid of B, S (ragged last tiles), H, D, R, rot_offset, both pairings, in and out of place it plays the kernel —
// every workgroup, every thread's strided walk of both phases — against brute-force enumeration:
//   * the tiles cover every row of every batch entry once, none has more than kRotFreqRows rows;
//   * the angle phase fills every LDS slot of the tile's rows exactly once, inside [0, nrows * R/2);
//   * every (row, head, chunk) is served exactly once, by the workgroup that owns the row, its 8-element chunks inside the
//     tensor (the sanitizer sees every access), pass-through chunks only out of place;
//   * the quads a unit reads from LDS hold the frequencies of its columns: tcol .. tcol + 7 (interleaved: + 3);
//   * the 2-bit axis map survives pack / unpack for every frequency and every axis.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "rfa_rotfreq_index.h"

using namespace rfa;

static int fails = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
      ++fails;                                                \
    }                                                         \
  } while (0)

static void run(uint32_t B, uint32_t S, uint32_t H, uint32_t D, uint32_t R, uint32_t off, int inter, int inplace) {
  RotaryGeom g{};
  g.B = B; g.S = S; g.R = R; g.rot_off = off; g.rot_units = inter ? R / 8 : R / 16; g.interleaved = inter;
  RotaryTensor t{};
  t.sh = D + 8; t.sr = (int64_t)H * t.sh + 16; t.sb = (int64_t)S * t.sr;                  // padded on the read side
  if (inplace) { t.dh = t.sh; t.dr = t.sr; t.db = t.sb; } else { t.dh = D; t.dr = (int64_t)H * D; t.db = (int64_t)S * t.dr; }
  t.H = H;
  t.uph = rotary_units_per_head(D, R, inter, inplace != 0);
  const uint32_t half = R / 2;
  std::vector<uint8_t> src((size_t)B * t.sb, 0), written((size_t)B * t.db, 0), rows(B * S, 0);
  for (uint32_t wg = 0; wg < B * rotfreq_tiles_per_batch(S); ++wg) {
    const RotFreqTile tile = rotfreq_tile(S, wg);
    CHECK(tile.b < B && tile.nrows >= 1 && tile.nrows <= (uint32_t)kRotFreqRows && tile.row0 + tile.nrows <= S, "tile %u", wg);
    for (uint32_t r = 0; r < tile.nrows; ++r) ++rows[tile.b * S + tile.row0 + r];
    // angle phase: which frequency every LDS slot holds
    std::vector<int32_t> lds(tile.nrows * half, -1);
    for (uint32_t tid = 0; tid < (uint32_t)kRotFreqThreads; ++tid)
      for (uint32_t e = tid; e < tile.nrows * half; e += kRotFreqThreads) {
        const uint32_t r = e / half, c = e - r * half;
        int32_t& slot = lds.at(r * half + rotfreq_lds_col(half, inter, c));
        CHECK(slot == -1, "LDS slot written twice");
        slot = (int32_t)c;
      }
    // stream phase
    const uint32_t first = rotfreq_first_unit(g, t, tile), n = rotfreq_tile_units(t, tile);
    for (uint32_t tid = 0; tid < (uint32_t)kRotFreqThreads; ++tid)
      for (uint32_t u = tid; u < n; u += kRotFreqThreads) {
        RotaryUnit x;
        rotary_unit(g, t, first + u, &x);
        CHECK(x.b == tile.b && x.i >= tile.row0 && x.i < tile.row0 + tile.nrows && x.h < H, "unit %u leaves its tile", u);
        CHECK(!(inplace && x.kind == kRotaryPass), "a pass-through unit in place");
        const int chunks = x.kind == kRotaryHalves ? 2 : 1;
        for (int q = 0; q < chunks; ++q)
          for (int e = 0; e < 8; ++e) {
            (void)src.at((size_t)((q ? x.s2 : x.s1) + e));
            ++written.at((size_t)((q ? x.d2 : x.d1) + e));
          }
        if (x.kind == kRotaryPass) continue;
        const uint32_t row = (x.i - tile.row0) * half;
        for (uint32_t q = 0; q < (inter ? 1u : 2u); ++q) {
          const uint32_t at = row + rotfreq_lds_quad(half, inter, x.tcol, q);
          CHECK(at % 4 == 0, "an LDS quad off 16 bytes");
          for (uint32_t e = 0; e < 4; ++e) CHECK(lds.at(at + e) == (int32_t)(x.tcol + 4 * q + e), "LDS quad holds the wrong frequency");
        }
      }
  }
  for (uint32_t r = 0; r < B * S; ++r) CHECK(rows[r] == 1, "row %u in %u tiles", r, rows[r]);
  // brute force: which elements of the written side must have been written, once
  for (uint32_t b = 0; b < B; ++b)
    for (uint32_t i = 0; i < S; ++i)
      for (uint32_t h = 0; h < H; ++h)
        for (uint32_t c = 0; c < D; ++c) {
          const bool rotated = c >= off && c < off + R;
          const int want = rotated || !inplace ? 1 : 0;
          const size_t at = (size_t)(b * t.db + i * t.dr + h * t.dh + c);
          CHECK(written[at] == want, "element (%u,%u,%u,%u) written %d times", b, i, h, c, written[at]);
          written[at] = 0;
        }
  for (size_t at = 0; at < written.size(); ++at) CHECK(written[at] == 0, "padding written at %zu", at);
}

int main() {
  int configs = 0;
  const uint32_t shapes[][3] = {{128, 128, 0}, {192, 64, 128}, {40, 16, 8}, {256, 256, 0}, {64, 32, 16}, {8, 8, 0}};   // D, R, off
  for (uint32_t B : {1u, 2u})
    for (uint32_t S : {1u, 7u, 8u, 9u, 19u})
      for (uint32_t H : {1u, 5u, 40u})
        for (const auto& s : shapes)
          for (int inter = 0; inter < 2; ++inter)
            for (int inplace = 0; inplace < 2; ++inplace) {
              if (s[1] % (inter ? 8 : 16)) continue;
              run(B, S, H, s[0], s[1], s[2], inter, inplace);
              ++configs;
            }
  // the axis map: every frequency, every axis, alone among other values
  for (uint32_t c = 0; c < 128; ++c)
    for (uint32_t axis = 0; axis < 4; ++axis) {
      uint64_t w[4] = {0, 0, 0, 0};
      for (uint32_t o = 0; o < 128; ++o) rotfreq_pack_axis(w, o, o == c ? axis : (o * 7 + axis + 1) & 3);
      CHECK(rotfreq_axis(w[0], w[1], w[2], w[3], c) == axis, "axis of frequency %u", c);
      for (uint32_t o = 0; o < 128; ++o)
        if (o != c) CHECK(rotfreq_axis(w[0], w[1], w[2], w[3], o) == ((o * 7 + axis + 1) & 3), "axis of frequency %u", o);
    }
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("%d configurations ok\n", configs);
  return 0;
}
