// mlarope_check.cpp — stand-alone host check of the tile / unit / head-sum arithmetic of the MLA rotary kernels
// (csrc/rfa_mlarope_index.h), built with -fsanitize=address,undefined (tests/test_mla_rotary_cpu.py).  No device, no HIP.  It
// plays every workgroup's strided walk against brute force: each element of k, v (forward) and dkv (backward) is written once,
// from the column it must hold, inside the tensors (the sanitizer sees every access; kv is padded and the padding is never
// touched); the lanes of a row's head sum cover every (head, chunk) once, the fold adds exactly the slices that own a head, no
// partial slot is shared; a row stride past 4 GiB stays in 64-bit arithmetic.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "rfa_mlarope_index.h"

using namespace rfa;

static int fails = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
      ++fails;                                                \
    }                                                         \
  } while (0)

static void run(uint32_t B, uint32_t S, uint32_t H, uint32_t Dn, uint32_t Dr, uint32_t Dv, int inter) {
  MlaRopeGeom g{};
  g.B = B; g.S = S; g.H = H; g.Dn = Dn; g.Dr = Dr; g.Dv = Dv; g.rot_units = inter ? Dr / 8 : Dr / 16; g.interleaved = inter;
  MlaRopeTensor kv{}, k{}, v{};
  kv.sh = Dn + Dv + 8; kv.sr = (int64_t)H * kv.sh + 16; kv.sb = (int64_t)S * kv.sr;        // padded
  k.sh = Dn + Dr; k.sr = (int64_t)H * k.sh; k.sb = (int64_t)S * k.sr;
  v.sh = Dv; v.sr = (int64_t)H * v.sh; v.sb = (int64_t)S * v.sr;
  // what a written element holds: 1 + the kv column it came from, or -(1 + the k_pe column); dkv: 1 + its own column
  std::vector<int32_t> kbuf((size_t)B * k.sb, 0), vbuf((size_t)B * v.sb, 0), dkv((size_t)B * kv.sb, 0), rows(B * S, 0);
  for (uint32_t wg = 0; wg < B * rotfreq_tiles_per_batch(S, kMlaRopeRows); ++wg) {
    const RotFreqTile tile = rotfreq_tile(S, wg, kMlaRopeRows);
    CHECK(tile.b < B && tile.nrows >= 1 && tile.nrows <= (uint32_t)kMlaRopeRows && tile.row0 + tile.nrows <= S, "tile %u", wg);
    for (uint32_t r = 0; r < tile.nrows; ++r) ++rows[tile.b * S + tile.row0 + r];
    for (int bwd = 0; bwd < 2; ++bwd)
      for (uint32_t tid = 0; tid < (uint32_t)kMlaRopeThreads; ++tid)
        for (uint32_t u = tid; u < tile.nrows * H * mlarope_units_per_head(g, !bwd); u += kMlaRopeThreads) {
          const MlaRopeUnit x = mlarope_unit(g, !bwd, u);
          CHECK(x.r < tile.nrows && x.h < H && !(bwd && x.kind == kMlaRope), "unit %u", u);
          for (uint32_t e = 0; e < 8; ++e) {
            int32_t& out = (x.kind == kMlaValue ? vbuf : kbuf).at((size_t)mlarope_off(x.kind == kMlaValue ? v : k, tile.b, tile.row0 + x.r, x.h, x.out_col + e));
            if (x.kind == kMlaRope) {
              CHECK(x.kv_col + e < Dr, "a rope column outside the rotated row");
              out -= (int32_t)(1 + x.kv_col + e);
              continue;
            }
            int32_t& in = dkv.at((size_t)mlarope_off(kv, tile.b, tile.row0 + x.r, x.h, x.kv_col + e));
            if (bwd) in += (int32_t)(1 + (x.kind == kMlaValue ? Dn : 0u) + x.out_col + e);
            else out += (int32_t)(1 + x.kv_col + e);
          }
        }
  }
  for (uint32_t r = 0; r < B * S; ++r) CHECK(rows[r] == 1, "row %u in %d tiles", r, rows[r]);
  for (uint32_t b = 0; b < B; ++b)
    for (uint32_t i = 0; i < S; ++i)
      for (uint32_t h = 0; h < H; ++h) {
        for (uint32_t c = 0; c < Dn + Dr; ++c)
          CHECK(kbuf[(size_t)mlarope_off(k, b, i, h, c)] == (c < Dn ? (int32_t)(1 + c) : -(int32_t)(1 + c - Dn)), "k (%u,%u,%u,%u)", b, i, h, c);
        for (uint32_t c = 0; c < Dv; ++c) CHECK(vbuf[(size_t)mlarope_off(v, b, i, h, c)] == (int32_t)(1 + Dn + c), "v (%u,%u,%u,%u)", b, i, h, c);
        for (uint32_t c = 0; c < Dn + Dv; ++c) {
          int32_t& at = dkv[(size_t)mlarope_off(kv, b, i, h, c)];
          CHECK(at == (int32_t)(1 + c), "dkv (%u,%u,%u,%u) holds %d", b, i, h, c, at);
          at = 0;
        }
      }
  for (size_t at = 0; at < dkv.size(); ++at) CHECK(dkv[at] == 0, "dkv padding written at %zu", at);
  // the head sum of a row: lanes, slots and the fold
  const uint32_t nch = Dr / 8, ns = mlarope_red_slices(Dr), nfold = mlarope_red_fold(Dr, H);
  CHECK(ns >= 1 && ns * nch <= (uint32_t)kMlaRopeRowThreads && g.rot_units <= (uint32_t)kMlaRopeRowThreads, "lanes of a row");
  std::vector<uint8_t> pair(H * nch, 0), slot((size_t)kMlaRopeRows * kMlaRopeRowThreads * 8, 0);
  for (uint32_t r = 0; r < (uint32_t)kMlaRopeRows; ++r)
    for (uint32_t l = 0; l < (uint32_t)kMlaRopeRowThreads; ++l) {
      const MlaRopeLane x = mlarope_red_lane(Dr, l);
      if (!x.active) continue;
      uint32_t heads = 0;
      for (uint32_t h = x.slice; h < H; h += ns, ++heads)
        if (r == 0) ++pair.at(h * nch + x.chunk);
      CHECK(x.slice < ns && x.chunk < nch && (heads > 0) == (x.slice < nfold), "lane %u: slice %u owns %u heads", l, x.slice, heads);
      for (uint32_t e = 0; e < 8; ++e) ++slot.at(mlarope_red_slot(Dr, r, x.slice, x.chunk) + e);
    }
  for (uint32_t at = 0; at < H * nch; ++at) CHECK(pair[at] == 1, "(head, chunk) %u summed %d times", at, pair[at]);
  for (size_t at = 0; at < slot.size(); ++at) CHECK(slot[at] <= 1, "partial slot %zu written %d times", at, slot[at]);
}

int main() {
  int configs = 0;
  const uint32_t dims[][4] = {{128, 64, 128, 0}, {192, 64, 128, 0}, {8, 16, 8, 0}, {24, 8, 40, 1}, {0, 32, 16, 1}, {0, 256, 256, 0},
                              {0, 256, 8, 1}};                          // Dn, Dr, Dv, interleaved
  for (uint32_t B : {1u, 2u})
    for (uint32_t S : {1u, 2u, 7u, 19u})
      for (uint32_t H : {1u, 3u, 16u, 131u})
        for (const auto& d : dims) {
          run(B, S, H, d[0], d[1], d[2], (int)d[3]);
          ++configs;
        }
  MlaRopeTensor far{};                                                  // rows past 4 GiB of elements
  far.sr = ((int64_t)1 << 32) + 4096; far.sh = 192; far.sb = far.sr * 5;
  CHECK(mlarope_off(far, 1, 3, 2, 136) == 8 * far.sr + 2 * 192 + 136 && mlarope_off(far, 3, 4, 127, 184) > ((int64_t)1 << 36), "a far row");
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("%d configurations ok\n", configs);
  return 0;
}
