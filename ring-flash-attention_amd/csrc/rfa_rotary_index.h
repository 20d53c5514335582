// rfa_rotary_index.h — the index arithmetic of the rotary embedding kernel (rfa_rotary.hip; include/rfa.h: rfa_rotary), in
// functions that the kernel and the stand-alone host check (tests/native/rotary_check.cpp) share.  Plain C++ without HIP
// types: the host check compiles it with any compiler.
//
// One tensor of a call is (B, S, H, D) with any (batch, row, head) element strides and last stride 1, read at `src` strides and
// written at `dst` strides.  The columns [rot_off, rot_off + R) of every (row, head) are rotated, the others pass through.  The
// work is cut into UNITS, one per thread; the units of one (row, head), index w in [0, uph):
//   halves (GPT-NeoX)   w < R/16:  the 8 columns at c = rot_off + 8 w and the 8 at c + R/2; table columns 8 w .. 8 w + 7
//   interleaved (GPT-J) w < R/8:   the 8 columns at c = rot_off + 8 w = 4 pairs (2e, 2e+1);  table columns 4 w .. 4 w + 3
//   pass-through        the (D - R)/8 chunks outside the rotated columns, in column order — OUT OF PLACE only: in place (dst ==
//                       src) these units do not exist and the columns are never touched
// and a unit index u in [0, B*S*H*uph) is ((b*S + i)*H + h)*uph + w: consecutive threads walk one head's columns, then the next
// head of the row — memory order for a contiguous tensor.  All element offsets are 64-bit.
#ifndef RFA_ROTARY_INDEX_H_
#define RFA_ROTARY_INDEX_H_

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RFA_ROTARY_HD __host__ __device__ __forceinline__
#else
#define RFA_ROTARY_HD inline
#endif

namespace rfa {

enum { kRotaryHalves = 0, kRotaryInterleaved = 1, kRotaryPass = 2 };

// one tensor of a call
struct RotaryTensor {
  int64_t sb, sr, sh;               // element strides of the side that is read: batch, row, head
  int64_t db, dr, dh;               // ... of the side that is written (in place: the same)
  uint32_t H;
  uint32_t uph;                     // units per (row, head): the rotating ones, plus the pass-through chunks out of place
  uint32_t nunits;                  // B * S * H * uph
};

struct RotaryGeom {
  uint32_t B, S;
  uint32_t R, rot_off;              // rotary width and first rotated column (elements)
  uint32_t rot_units;               // halves: R / 16; interleaved: R / 8
  int32_t interleaved;
};

struct RotaryUnit {
  uint32_t b, i, h;                 // batch entry, row, head
  int32_t kind;                     // kRotaryHalves / kRotaryInterleaved / kRotaryPass
  uint32_t col, col2;               // first column of the unit's chunk; halves: of its partner chunk (else == col)
  uint32_t tcol;                    // first column of the cos / sin row the unit reads (8 values; interleaved: 4)
  int64_t s1, s2, d1, d2;           // ELEMENT offsets of the chunk(s) on the read and on the written side
};

// units per (row, head) of a tensor: `inplace` tensors have no pass-through units
RFA_ROTARY_HD uint32_t rotary_units_per_head(uint32_t D, uint32_t R, int interleaved, bool inplace) {
  return (interleaved ? R / 8 : R / 16) + (inplace ? 0u : (D - R) / 8);
}

RFA_ROTARY_HD void rotary_unit(const RotaryGeom& g, const RotaryTensor& t, uint32_t u, RotaryUnit* x) {
  const uint32_t w = u % t.uph;
  uint32_t r = u / t.uph;                        // (b*S + i)*H + h
  x->h = r % t.H;
  r /= t.H;
  x->i = r % g.S;
  x->b = r / g.S;
  if (w < g.rot_units) {
    x->kind = g.interleaved ? kRotaryInterleaved : kRotaryHalves;
    x->col = g.rot_off + 8 * w;
    x->col2 = g.interleaved ? x->col : x->col + g.R / 2;
    x->tcol = g.interleaved ? 4 * w : 8 * w;
  } else {
    const uint32_t c = 8 * (w - g.rot_units);    // column among the pass-through ones
    x->kind = kRotaryPass;
    x->col = x->col2 = c < g.rot_off ? c : c + g.R;
    x->tcol = 0;
  }
  const int64_t s = (int64_t)x->b * t.sb + (int64_t)x->i * t.sr + (int64_t)x->h * t.sh;
  const int64_t d = (int64_t)x->b * t.db + (int64_t)x->i * t.dr + (int64_t)x->h * t.dh;
  x->s1 = s + x->col;
  x->s2 = s + x->col2;
  x->d1 = d + x->col;
  x->d2 = d + x->col2;
}

// the position map (include/rfa.h: q_pos_stride ...; ring_flash_attn._common.pos_map): local row i sits at
//     (split == 0 || i < split) ? off + i * stride : off2 + (i - split) * stride
RFA_ROTARY_HD int64_t rotary_map_pos(int64_t off, uint32_t stride, int32_t split, int64_t off2, uint32_t i) {
  return (split == 0 || i < (uint32_t)split) ? off + (int64_t)i * stride : off2 + (int64_t)(i - (uint32_t)split) * stride;
}

// a position as the tables are read: inside [0, P - 1] whatever came in
RFA_ROTARY_HD int64_t rotary_clamp_pos(int64_t pos, int64_t P) { return pos < 0 ? 0 : (pos > P - 1 ? P - 1 : pos); }

}  // namespace rfa
#endif  // RFA_ROTARY_INDEX_H_
