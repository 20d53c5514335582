// rfa_rotfreq_index.h — the index arithmetic of the rotary kernel that forms its own angles (rfa_rotfreq.hip; include/rfa.h:
// rfa_rotary_freqs), in functions that the kernel, the host launcher and the stand-alone host check
// (tests/native/rotfreq_check.cpp) share.  Plain C++ without HIP types.
//
// The tensors, the columns and the UNITS are rfa_rotary_index.h's, and so is their order: unit ((b*S + i)*H + h)*uph + w.  What
// is new is the split of the work.  A workgroup owns a TILE: kRotFreqRows consecutive rows of one batch entry (the last tile of
// a batch entry is ragged).  In that order the units of a tile are ONE run of consecutive unit indices,
//     [ (b*S + row0) * H * uph,  + nrows * H * uph ),
// of every tensor of the call, so the workgroup walks the run with its 256 threads and decodes each index with rotary_unit()
// itself — the same offsets, partners and pass-through chunks as the table kernel, for any H.
// The angles of the tile's rows are computed once, before that walk: nrows * R/2 entries (row, c), entry e = row * R/2 + c,
// into two LDS arrays [kRotFreqRows][R/2] of fp32 (cos', sin').  A halves unit w needs columns 8w .. 8w+7 of both; stored in
// column order, the 8 lanes of a head would read 16 bytes at a pitch of 32 — every other quad of banks — twice.  So a row is
// stored with its even quads first and its odd quads behind them (rotfreq_lds_col): lane w then reads quad w of the first half
// of the row and quad w of the second, 16 bytes at a pitch of 16 both times, the whole row of a 128-wide head in one pass
// without a conflict whatever the bank count, and with no padding (the pitch stays R/2: all heads of a row read the SAME
// addresses — a broadcast — and a wave straddles two rows only at a row's end).  Interleaved units read ONE quad, 4w .. 4w+3,
// which is conflict-free in column order: no permutation there.
// The axis of every frequency (M-RoPE) travels in the kernel arguments: 2 bits each, 32 frequencies per 64-bit word.
#ifndef RFA_ROTFREQ_INDEX_H_
#define RFA_ROTFREQ_INDEX_H_

#include "rfa_rotary_index.h"

namespace rfa {

// rows of a tile.  LDS: 2 arrays * 2 rows * R/2 fp32 = 2 KiB at R = 256 (the bound asked for is 16 KiB); q (1, 8192, 32, 128) +
// k (1, 8192, 8, 128) is 4096 workgroups = 16 per CU on 256 CUs, each with 128 sincosf for its 640 units (2.5 per thread).
// Measured (profiles/rotary_freqs.md): the time falls with the tile height, 16 rows 40.7 us .. 8 rows 36.7 .. 2 rows 33.7 ..
// 1 row 32.9, and no phase in front of the stream phase costs anything; 2 keeps a workgroup's threads busy where H + Hk is small.
enum { kRotFreqRows = 2, kRotFreqThreads = 256, kRotFreqMaxHalf = 128 };

struct RotFreqTile {
  uint32_t b, row0, nrows;          // batch entry, first row, rows (1 .. kRotFreqRows)
};

// (`rows`: the rows of a tile — kRotFreqRows in every shipped instance; tools/rotfreq_variants.hip times others)
RFA_ROTARY_HD uint32_t rotfreq_tiles_per_batch(uint32_t S, uint32_t rows = kRotFreqRows) { return (S + rows - 1) / rows; }

// tile `tile` of the grid's B * tiles_per_batch
RFA_ROTARY_HD RotFreqTile rotfreq_tile(uint32_t S, uint32_t tile, uint32_t rows = kRotFreqRows) {
  const uint32_t per = rotfreq_tiles_per_batch(S, rows);
  RotFreqTile t;
  t.b = tile / per;
  t.row0 = (tile % per) * rows;
  t.nrows = S - t.row0 < rows ? S - t.row0 : rows;
  return t;
}

// the run of unit indices of tensor `t` that the tile owns: first index and count (the host has checked that B S H uph fits 31
// bits, so neither overflows)
RFA_ROTARY_HD uint32_t rotfreq_first_unit(const RotaryGeom& g, const RotaryTensor& t, const RotFreqTile& tile) {
  return (tile.b * g.S + tile.row0) * t.H * t.uph;
}
RFA_ROTARY_HD uint32_t rotfreq_tile_units(const RotaryTensor& t, const RotFreqTile& tile) { return tile.nrows * t.H * t.uph; }

// where frequency c of a row sits in the row's LDS run of R/2 floats
RFA_ROTARY_HD uint32_t rotfreq_lds_col(uint32_t half, int interleaved, uint32_t c) {
  if (interleaved) return c;
  return ((c >> 2) & 1u) * (half / 2) + ((c >> 3) << 2) + (c & 3u);
}

// first float of the 4 that a unit reads: q = 0 for columns tcol .. tcol+3, q = 1 (halves only) for tcol+4 .. tcol+7
RFA_ROTARY_HD uint32_t rotfreq_lds_quad(uint32_t half, int interleaved, uint32_t tcol, uint32_t q) {
  return interleaved ? tcol : q * (half / 2) + (tcol >> 1);
}

// the axis of frequency c in the packed map, and the packing (words must start as zero)
RFA_ROTARY_HD uint32_t rotfreq_axis(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t c) {
  const uint32_t k = c >> 5;
  const uint64_t w = k == 0 ? w0 : (k == 1 ? w1 : (k == 2 ? w2 : w3));
  return (uint32_t)(w >> (2 * (c & 31u))) & 3u;
}
RFA_ROTARY_HD void rotfreq_pack_axis(uint64_t* words, uint32_t c, uint32_t axis) {
  words[c >> 5] |= (uint64_t)(axis & 3u) << (2 * (c & 31u));
}

}  // namespace rfa
#endif  // RFA_ROTFREQ_INDEX_H_
