// rotary_check.cpp — stand-alone host check of the rotary kernel's index arithmetic (csrc/rfa_rotary_index.h), meant to be
// built with -fsanitize=address,undefined (tests/test_rotary_cpu.py).  No device, no HIP: the header is plain C++.
// Over a grid of B, S, H, D, R, rot_offset, both pairings, in place and out of place, dense and padded strides it plays the
// kernel — every unit index, as a thread would — against a brute-force enumeration of the elements:
//   * every unit's 8-element chunks lie inside the tensor's extent (the sanitizer sees every access);
//   * every rotated element is written exactly once, out of place every pass-through element too, nothing else is written
//     (padding between heads, rows and batch entries; in place the pass-through columns);
//   * a rotated element is paired with the right partner, in the right role, and reads the right table column;
//   * the position of every unit's row under a map equals the map's definition (ring_flash_attn._common.map_positions),
//     also where the split falls inside a workgroup's 256 units;
//   * offsets stay exact when a stride puts a row past 2^32 elements (arithmetic only: nothing is allocated).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rfa_rotary_index.h"

using namespace rfa;

static int fails = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
      ++fails;                                                \
    }                                                         \
  } while (0)

struct Cfg { uint32_t B, S, H, D, R, off; int inter, inplace, padded; };

static RotaryGeom geom(const Cfg& c) {
  RotaryGeom g{};
  g.B = c.B; g.S = c.S; g.R = c.R; g.rot_off = c.off;
  g.rot_units = c.inter ? c.R / 8 : c.R / 16;
  g.interleaved = c.inter;
  return g;
}

// strides of one side: dense, or with padding after every head, row and batch entry (multiples of 8: the 16-byte contract)
static void strides(const Cfg& c, int padded, int64_t* b, int64_t* r, int64_t* h, int64_t* extent) {
  *h = c.D + (padded ? 8 : 0);
  *r = (int64_t)c.H * *h + (padded ? 16 : 0);
  *b = (int64_t)c.S * *r + (padded ? 24 : 0);
  *extent = (int64_t)c.B * *b;
}

static void run(const Cfg& c) {
  const RotaryGeom g = geom(c);
  RotaryTensor t{};
  int64_t sext, dext;
  strides(c, c.padded, &t.sb, &t.sr, &t.sh, &sext);
  if (c.inplace) { t.db = t.sb; t.dr = t.sr; t.dh = t.sh; dext = sext; }
  else strides(c, !c.padded, &t.db, &t.dr, &t.dh, &dext);           // (the other side has the other kind of strides)
  t.H = c.H;
  t.uph = rotary_units_per_head(c.D, c.R, c.inter, c.inplace != 0);
  t.nunits = c.B * c.S * c.H * t.uph;
  std::vector<uint8_t> src(sext, 0), written(dext, 0);
  std::vector<int32_t> partner(dext, -1), tcol(dext, -1), role(dext, -1);
  // a map whose split falls inside a workgroup's 256 units whenever the tensor has that many
  const int32_t split = c.S > 1 ? (int32_t)(c.S / 2 + (c.S > 4)) : 0;
  const int64_t off = 1000, off2 = 70000;
  const uint32_t stride = c.padded ? 3 : 1;
  for (uint32_t u = 0; u < t.nunits; ++u) {
    RotaryUnit x;
    rotary_unit(g, t, u, &x);
    CHECK(x.b < c.B && x.i < c.S && x.h < c.H, "unit %u names (%u, %u, %u)", u, x.b, x.i, x.h);
    CHECK(x.s1 >= 0 && x.s1 + 8 <= sext && x.s2 >= 0 && x.s2 + 8 <= sext, "unit %u reads outside: %lld %lld of %lld", u,
          (long long)x.s1, (long long)x.s2, (long long)sext);
    CHECK(x.d1 >= 0 && x.d1 + 8 <= dext && x.d2 >= 0 && x.d2 + 8 <= dext, "unit %u writes outside: %lld %lld of %lld", u,
          (long long)x.d1, (long long)x.d2, (long long)dext);
    if (fails) return;
    const int64_t sbase = (int64_t)x.b * t.sb + (int64_t)x.i * t.sr + (int64_t)x.h * t.sh;
    const int64_t dbase = (int64_t)x.b * t.db + (int64_t)x.i * t.dr + (int64_t)x.h * t.dh;
    CHECK(x.s1 - sbase == x.d1 - dbase && x.s2 - sbase == x.d2 - dbase, "unit %u: columns differ between the sides", u);
    for (int e = 0; e < 8; ++e) {
      (void)src[x.s1 + e];
      (void)src[x.s2 + e];
      ++written[x.d1 + e];
      if (x.kind == kRotaryHalves) {
        ++written[x.d2 + e];
        partner[x.d1 + e] = (int32_t)(x.col2 + e); role[x.d1 + e] = 0; tcol[x.d1 + e] = (int32_t)(x.tcol + e);
        partner[x.d2 + e] = (int32_t)(x.col + e);  role[x.d2 + e] = 1; tcol[x.d2 + e] = (int32_t)(x.tcol + e);
      } else if (x.kind == kRotaryInterleaved) {
        partner[x.d1 + e] = (int32_t)(x.col + (e ^ 1)); role[x.d1 + e] = e & 1; tcol[x.d1 + e] = (int32_t)(x.tcol + e / 2);
      }
    }
    // the row's position under a map: the definition, restated
    const int64_t want = (split == 0 || (int32_t)x.i < split) ? off + (int64_t)x.i * stride : off2 + (int64_t)((int32_t)x.i - split) * stride;
    CHECK(rotary_map_pos(off, stride, split, off2, x.i) == want, "unit %u: row %u at %lld, not %lld", u, x.i,
          (long long)rotary_map_pos(off, stride, split, off2, x.i), (long long)want);
  }
  // brute force over the destination's elements
  std::vector<uint8_t> expect(dext, 0);
  for (uint32_t b = 0; b < c.B; ++b)
    for (uint32_t i = 0; i < c.S; ++i)
      for (uint32_t h = 0; h < c.H; ++h)
        for (uint32_t col = 0; col < c.D; ++col) {
          const int64_t d = (int64_t)b * t.db + (int64_t)i * t.dr + (int64_t)h * t.dh + col;
          const bool rotated = col >= c.off && col < c.off + c.R;
          expect[d] = (rotated || !c.inplace) ? 1 : 0;
          if (!rotated) {
            CHECK(partner[d] == -1, "a pass-through element was rotated");
            continue;
          }
          const uint32_t r = col - c.off;
          const int32_t wp = c.inter ? (int32_t)(c.off + (r ^ 1u)) : (int32_t)(c.off + (r < c.R / 2 ? r + c.R / 2 : r - c.R / 2));
          const int32_t wr = c.inter ? (int32_t)(r & 1u) : (int32_t)(r >= c.R / 2);
          const int32_t wt = c.inter ? (int32_t)(r / 2) : (int32_t)(r % (c.R / 2));
          CHECK(partner[d] == wp && role[d] == wr && tcol[d] == wt, "column %u: partner %d role %d table %d, want %d %d %d", col,
                partner[d], role[d], tcol[d], wp, wr, wt);
        }
  for (int64_t d = 0; d < dext; ++d)
    CHECK(written[d] == expect[d], "element %lld written %d times, want %d", (long long)d, written[d], expect[d]);
}

// strides that put rows and batch entries past 2^32 elements: the offsets against 128-bit arithmetic, nothing allocated
static void far() {
  Cfg c{2, 5, 3, 128, 64, 32, 0, 0, 0};
  const RotaryGeom g = geom(c);
  RotaryTensor t{};
  t.sh = 128; t.sr = (1ll << 33) + 8; t.sb = (1ll << 40);
  t.dh = 136; t.dr = (1ll << 34) + 16; t.db = (1ll << 41);
  t.H = c.H; t.uph = rotary_units_per_head(c.D, c.R, 0, false); t.nunits = c.B * c.S * c.H * t.uph;
  for (uint32_t u = 0; u < t.nunits; ++u) {
    RotaryUnit x;
    rotary_unit(g, t, u, &x);
    const __int128 s = (__int128)x.b * t.sb + (__int128)x.i * t.sr + (__int128)x.h * t.sh;
    const __int128 d = (__int128)x.b * t.db + (__int128)x.i * t.dr + (__int128)x.h * t.dh;
    CHECK((__int128)x.s1 == s + x.col && (__int128)x.s2 == s + x.col2 && (__int128)x.d1 == d + x.col && (__int128)x.d2 == d + x.col2,
          "far unit %u", u);
    if (x.i >= 1) CHECK(x.s1 > (1ll << 32) && x.d1 > (1ll << 32), "far unit %u is not far", u);
  }
  // positions: 64-bit offsets, a stride, and the clamp
  CHECK(rotary_map_pos((1ll << 35), 7, 3, (1ll << 36), 2) == (1ll << 35) + 14, "far position");
  CHECK(rotary_map_pos((1ll << 35), 7, 3, (1ll << 36), 5) == (1ll << 36) + 14, "far position behind the split");
  CHECK(rotary_clamp_pos(-1, 10) == 0 && rotary_clamp_pos(10, 10) == 9 && rotary_clamp_pos(4, 10) == 4 &&
        rotary_clamp_pos(INT64_MIN, 1) == 0 && rotary_clamp_pos(INT64_MAX, 1) == 0, "clamp");
}

int main() {
  const uint32_t Bs[] = {1, 2}, Ss[] = {1, 5, 38}, Hs[] = {1, 3}, Ds[] = {8, 40, 64, 128, 192, 256};
  int n = 0;
  for (uint32_t B : Bs) for (uint32_t S : Ss) for (uint32_t H : Hs) for (uint32_t D : Ds)
    for (int inter = 0; inter < 2; ++inter) {
      const uint32_t step = inter ? 8 : 16;
      // rotary widths: the smallest, the whole head, and one in between; offsets: 0, 8, and flush with the end
      const uint32_t Rs[] = {step, D / step * step, (D / 2) / step * step};
      for (uint32_t R : Rs) {
        if (R == 0 || R > D) continue;
        const uint32_t offs[] = {0, 8, D - R};
        for (int k = 0; k < 3; ++k) {
          const uint32_t off = offs[k];
          if (off + R > D || (k > 0 && off == offs[k - 1]) || (k == 2 && off == offs[0])) continue;
          for (int inplace = 0; inplace < 2; ++inplace)
            for (int padded = 0; padded < 2; ++padded) {
              run(Cfg{B, S, H, D, R, off, inter, inplace, padded});
              ++n;
              if (fails) { printf("first failure in B %u S %u H %u D %u R %u off %u inter %d inplace %d padded %d\n", B, S, H, D, R, off, inter, inplace, padded); return 1; }
            }
        }
      }
    }
  far();
  if (fails) return 1;
  printf("%d configurations ok\n", n);
  return 0;
}
