// rfa_mlarope_index.h — the tile, unit and reduction arithmetic of the MLA K / V assembly fused with the rotary embedding
// (rfa_mlarope.hip; include/rfa.h: rfa_mla_rotary_fwd / _bwd), in functions that the kernels, the host launcher and the
// stand-alone host check (tests/native/mlarope_check.cpp) share.  Plain C++ without HIP types.
//
// Per token the projections of a multi-head latent attention layer leave  q (Hq, Dn + Dr),  kv (H, Dn + Dv) = [k_nope | v]  and
// ONE rope key k_pe (Dr) for all heads; attention wants  k (H, Dn + Dr) = [k_nope | rope(k_pe)]  and  v (H, Dv).  A workgroup owns
// a TILE of kMlaRopeRows consecutive rows of one batch entry (rfa_rotfreq_index.h: rotfreq_tile) and serves three streams of
// 16-byte UNITS (8 elements) for it:
//   q       rfa_rotary_index.h's units with R = Dr, rot_off = Dn, out of place: the tile's run of unit indices, decoded by
//           rotary_unit() itself — the offsets, partners and pass-through chunks of the table kernel
//   k, v    forward: (Dn + Dr + Dv) / 8 units per (row, head), in the order of the written side — the head's k row first
//           (kMlaNope: a chunk of kv;  kMlaRope: a chunk of the row's rotated k_pe, out of LDS), then its v row (kMlaValue: a
//           chunk of kv behind the Dn columns); a run of consecutive units reads one kv row front to back and writes one k row and
//           one v row front to back
//   dkv     backward: (Dn + Dv) / 8 units per (row, head), the same without the rope chunks: dk's and dv's chunks into one dkv row
// and unit u of a tile is (r * H + h) * units_per_head + w.  All element offsets are 64-bit (mlarope_off).
// The backward's sum over heads,  dk_pe[row] = rope^-1( sum_h dk[row, h, Dn:] ),  stays inside the workgroup: each row of the tile
// has kMlaRopeRowThreads lanes, whatever the tile holds (a ragged last tile idles the others), cut into
//     slices = kMlaRopeRowThreads / (Dr / 8)  lane groups of Dr / 8 lanes, lane l = slice * (Dr / 8) + chunk;
// the lane of (slice s, chunk c) adds the chunk c of heads s, s + slices, s + 2 slices, ... < H in that order in fp32, the partial
// sums go to LDS, and the lane of rotation unit w adds the partials of slices 0, 1, ... min(slices, H) - 1 in that order before
// it rotates.  The order of every sum is a function of H and Dr alone.
#ifndef RFA_MLAROPE_INDEX_H_
#define RFA_MLAROPE_INDEX_H_

#include "rfa_rotfreq_index.h"     // the rotary units, the position map, the tiles and the LDS order of a row's cos / sin

namespace rfa {

// rows of a tile.  An MLA layer has no grouped heads: at H = Hq = 128 (DeepSeek-V3) one row is 3072 q units, 5120 k / v units,
// 28 .. 32 per thread, so a taller tile only lengthens every thread's walk — which rotfreq_kernel's measurements
// (profiles/rotary_freqs.md: 16 rows 40.7 us .. 2 rows 33.7 .. 1 row 32.9) say costs time; 2 rather than 1 keeps the 256 threads
// busy at the 16 heads a tensor-parallel rank holds, and gives the backward's head sum 128 lanes per row.
enum { kMlaRopeRows = 2, kMlaRopeThreads = 256, kMlaRopeRowThreads = kMlaRopeThreads / kMlaRopeRows, kMlaRopeMaxRot = 256 };

enum { kMlaNope = 0, kMlaRope = 1, kMlaValue = 2 };

// element strides of one tensor: batch, row, head (k_pe has no heads: sh is not used)
struct MlaRopeTensor {
  int64_t sb, sr, sh;
};

struct MlaRopeGeom {
  uint32_t B, S, H;                 // H: heads of kv, k and v
  uint32_t Dn, Dr, Dv;
  uint32_t rot_units;               // halves: Dr / 16; interleaved: Dr / 8
  int32_t interleaved;
};

struct MlaRopeUnit {
  uint32_t r, h;                    // row inside the tile, head
  int32_t kind;                     // kMlaNope / kMlaRope / kMlaValue
  uint32_t kv_col;                  // first column in the kv (dkv) row; kMlaRope: in the row's rotated k_pe
  uint32_t out_col;                 // first column in the k (dk) row; kMlaValue: in the v (dv) row
};

RFA_ROTARY_HD uint32_t mlarope_units_per_head(const MlaRopeGeom& g, bool with_rope) {
  return (g.Dn + g.Dv + (with_rope ? g.Dr : 0u)) / 8;
}

// unit u in [0, nrows * H * units_per_head) of a tile's k / v stream (with_rope) or dkv stream (without)
RFA_ROTARY_HD MlaRopeUnit mlarope_unit(const MlaRopeGeom& g, bool with_rope, uint32_t u) {
  const uint32_t uph = mlarope_units_per_head(g, with_rope);
  const uint32_t c = 8 * (u % uph);                 // column of the written side's [k row | v row] (dkv: of [dk nope | dv])
  const uint32_t rh = u / uph;
  const uint32_t kw = g.Dn + (with_rope ? g.Dr : 0u);
  const bool nope = c < g.Dn, rope = !nope && c < kw;
  MlaRopeUnit x;
  x.h = rh % g.H;
  x.r = rh / g.H;
  x.kind = nope ? kMlaNope : (rope ? kMlaRope : kMlaValue);
  x.kv_col = nope ? c : (rope ? c - g.Dn : c - kw + g.Dn);
  x.out_col = nope || rope ? c : c - kw;
  return x;
}

// element offset of column `col` of (batch entry b, row i, head h)
RFA_ROTARY_HD int64_t mlarope_off(const MlaRopeTensor& t, uint32_t b, uint32_t i, uint32_t h, uint32_t col) {
  return (int64_t)b * t.sb + (int64_t)i * t.sr + (int64_t)h * t.sh + (int64_t)col;
}

// the backward's head sum: lane groups per row, and what lane l in [0, kMlaRopeRowThreads) of a row adds up
RFA_ROTARY_HD uint32_t mlarope_red_slices(uint32_t Dr) { return (uint32_t)kMlaRopeRowThreads / (Dr / 8); }

struct MlaRopeLane {
  bool active;                      // false: the lanes behind slices * (Dr / 8)
  uint32_t slice, chunk;            // heads slice, slice + slices, ... < H; columns Dn + 8 chunk .. + 7 of dk
};

RFA_ROTARY_HD MlaRopeLane mlarope_red_lane(uint32_t Dr, uint32_t l) {
  const uint32_t nch = Dr / 8;
  MlaRopeLane x;
  x.active = l < mlarope_red_slices(Dr) * nch;
  x.slice = l / nch;
  x.chunk = l % nch;
  return x;
}

// first float of the 8 partial sums of (row r of the tile, slice, chunk) in the LDS array of kMlaRopeRows * kMlaRopeRowThreads * 8
RFA_ROTARY_HD uint32_t mlarope_red_slot(uint32_t Dr, uint32_t r, uint32_t slice, uint32_t chunk) {
  return (r * (uint32_t)kMlaRopeRowThreads + slice * (Dr / 8) + chunk) * 8;
}

// slices whose partial sums the fold adds: the others own no head
RFA_ROTARY_HD uint32_t mlarope_red_fold(uint32_t Dr, uint32_t H) {
  const uint32_t ns = mlarope_red_slices(Dr);
  return H < ns ? H : ns;
}

}  // namespace rfa
#endif  // RFA_MLAROPE_INDEX_H_
