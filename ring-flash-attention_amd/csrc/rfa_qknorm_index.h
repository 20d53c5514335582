// rfa_qknorm_index.h — the index arithmetic of the fused per-head QK RMSNorm + rotary kernels (rfa_qknorm.hip; include/rfa.h:
// rfa_qk_norm_rotary_fwd / _bwd), in functions that the kernels, the C entry points and the stand-alone host check
// (tests/native/qknorm_check.cpp) share.  Plain C++ without HIP types: the host check compiles it with any compiler.
//
// One tensor of a call is (B, S, H, D); an ITEM is one (row, head), index ((b*S + i)*H + h).  An item lives in a LANE GROUP of
// G = qknorm_group(D) consecutive lanes of one wave — the smallest power of two >= D/8, 1 .. 32 — and lane w < D/8 of the group
// owns CHUNK w: the 8 columns (16 bytes) at 8 w.  Lanes w >= D/8 are idle.  A workgroup of 256 threads holds 256/G items.
// The chunk-to-lane map depends on D alone — not on R, rot_off or the pairing — so the row sums (8 values in a lane in column
// order, then the xor butterfly G/2, G/4, .. 1 over the group) have ONE order per D, and an element's bits do not depend on
// what is rotated.  What the rotation needs from another lane comes by a shuffle:
//   halves (GPT-NeoX)  chunk w with rot_off/8 <= w < rot_off/8 + R/16 is the x1 side ("lo"), its partner the chunk at w + R/16;
//                      the next R/16 chunks are the x2 side ("hi"), partner w - R/16; both read table columns 8 (w - first lo)
//   interleaved (GPT-J) chunk w inside the rotated columns holds 4 pairs of its own; table columns 4 (w - rot_off/8)
//   pass-through       every other chunk (R == 0, the norm-only call: all of them)
// Backward, per tensor (nparts and walk are functions of ITS item count): workgroup p of nparts walks the items
// (it * nparts + p) * (256/G) + group, it = 0 .. walk-1; the fp32 (D,) weight gradient partial of workgroup p sits at
// workspace[(partials of the tensors in front + p) * D]; the fold kernel sums a column's partials in
// kQkNormFoldSlices runs of qknorm_fold_len(nparts) consecutive ones, then the runs' sums in index order.
#ifndef RFA_QKNORM_INDEX_H_
#define RFA_QKNORM_INDEX_H_

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RFA_QKNORM_HD __host__ __device__ __forceinline__
#else
#define RFA_QKNORM_HD inline
#endif

namespace rfa {

enum { kQkNormLo = 0, kQkNormHi = 1, kQkNormInterleaved = 2, kQkNormPass = 3 };
enum { kQkNormThreads = 256, kQkNormMaxParts = 1024, kQkNormFoldSlices = 16 };

struct QkNormGeom {
  uint32_t B, S, D;
  uint32_t R, rot_off;              // rotary width (0: norm only) and first rotated column
  int32_t interleaved;
  uint32_t chunks;                  // D / 8
  uint32_t group;                   // qknorm_group(D)
};

// one tensor of a call: element strides (batch, row, head) of the input x, of what is written (forward: the output; backward:
// dx) and — backward only — of the incoming gradient
struct QkNormTensor {
  int64_t xb, xr, xh;
  int64_t ob, orow, oh;
  int64_t gb, gr, gh;
  uint32_t H;
  uint32_t nitems;                  // B * S * H
};

struct QkNormChunk {
  uint32_t b, i, h;                 // batch entry, row, head of the item
  int64_t x, o, g;                  // ELEMENT offsets of the chunk in the input, the written tensor, the incoming gradient
};

// what lane w of a group does; depends on the geometry alone
struct QkNormLane {
  int32_t kind;                     // kQkNormLo / Hi / Interleaved / Pass
  uint32_t col;                     // 8 w
  uint32_t partner;                 // lane of the group that holds the other half of the pairs (else == w)
  uint32_t tcol;                    // first column of the cos / sin row the lane reads (8 values; interleaved: 4)
};

RFA_QKNORM_HD uint32_t qknorm_group(uint32_t D) {
  uint32_t g = 1;
  while (g * 8 < D) g *= 2;
  return g;
}

RFA_QKNORM_HD void qknorm_lane(const QkNormGeom& g, uint32_t w, QkNormLane* l) {
  const uint32_t first = g.rot_off / 8;
  l->col = 8 * w;
  l->partner = w;
  l->tcol = 0;
  l->kind = kQkNormPass;
  if (g.R == 0 || w < first || w >= first + g.R / 8) return;
  if (g.interleaved) {
    l->kind = kQkNormInterleaved;
    l->tcol = 4 * (w - first);
  } else if (w < first + g.R / 16) {
    l->kind = kQkNormLo;
    l->partner = w + g.R / 16;
    l->tcol = 8 * (w - first);
  } else {
    l->kind = kQkNormHi;
    l->partner = w - g.R / 16;
    l->tcol = 8 * (w - first - g.R / 16);
  }
}

RFA_QKNORM_HD void qknorm_chunk(const QkNormGeom& g, const QkNormTensor& t, uint32_t item, uint32_t w, QkNormChunk* c) {
  uint32_t r = item;
  c->h = r % t.H;
  r /= t.H;
  c->i = r % g.S;
  c->b = r / g.S;
  c->x = (int64_t)c->b * t.xb + (int64_t)c->i * t.xr + (int64_t)c->h * t.xh + 8 * w;
  c->o = (int64_t)c->b * t.ob + (int64_t)c->i * t.orow + (int64_t)c->h * t.oh + 8 * w;
  c->g = (int64_t)c->b * t.gb + (int64_t)c->i * t.gr + (int64_t)c->h * t.gh + 8 * w;
}

// workgroups of a launch that covers `items` (the largest tensor's) without a walk
RFA_QKNORM_HD uint32_t qknorm_blocks(uint32_t items, uint32_t group) {
  const uint32_t per = kQkNormThreads / group;
  return items / per + (items % per ? 1u : 0u);
}

// backward: the number of workgroups = of weight gradient partials per tensor — a function of the shape alone
RFA_QKNORM_HD uint32_t qknorm_parts(uint32_t items, uint32_t group) {
  const uint32_t n = qknorm_blocks(items, group);
  return n > (uint32_t)kQkNormMaxParts ? (uint32_t)kQkNormMaxParts : n;
}

// backward: items a lane group walks (the last ones may lie past the tensor's end)
RFA_QKNORM_HD uint32_t qknorm_walk(uint32_t items, uint32_t nparts, uint32_t group) {
  const uint64_t per = (uint64_t)nparts * (kQkNormThreads / group);
  return per ? (uint32_t)((items + per - 1) / per) : 0u;
}

RFA_QKNORM_HD uint32_t qknorm_fold_len(uint32_t nparts) { return (nparts + kQkNormFoldSlices - 1) / kQkNormFoldSlices; }

RFA_QKNORM_HD int64_t qknorm_workspace_bytes(int ntensors, uint32_t nparts, uint32_t D) {
  return (int64_t)ntensors * nparts * D * (int64_t)sizeof(float);
}

}  // namespace rfa
#endif  // RFA_QKNORM_INDEX_H_
