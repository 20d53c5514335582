// rfa_qktoken_index.h — the index arithmetic of the token-wide QK RMSNorm + rotary kernels (rfa_qktoken.hip; include/rfa.h:
// rfa_qk_token_norm_rotary_fwd / _bwd), in functions that the kernels, the C entry points and the stand-alone host check
// (tests/native/qktoken_check.cpp) share.  Plain C++ without HIP types: the host check compiles it with any compiler.
//
// One tensor of a call is (B, S, H, D); a ROW is one token, index b*S + i, of N = H*D columns = C = N/8 CHUNKS of 16 bytes.
// Chunk c holds the columns 8 (c % (D/8)) .. + 7 of head c / (D/8).  A row is owned by a TEAM of
//     qktoken_team(N) = 64 (C <= 128), 128 (C <= 512) or 256 lanes
// = 1, 2 or 4 whole waves of one 256-thread workgroup, which therefore holds 256/team rows (SLOTS) at a time.  Team lane l owns
// the chunks l + j * team, j = 0 .. qktoken_per_lane(N) - 1 (at most 8; those >= C do not exist): consecutive lanes read
// consecutive 16 bytes.  The map depends on N alone — not on R, rot_off or the pairing, nor on the other tensor of the launch —
// so the row sums have ONE order per N.  What the rotation pairs (inside every head, as rfa_qknorm_index.h has it):
//   halves       chunk w of a head with rot_off/8 <= w < rot_off/8 + R/16 is the x1 side ("lo"), its partner the chunk R/16
//                further on in the row; the next R/16 chunks are the x2 side ("hi"), partner R/16 back; both read the table
//                columns 8 (w - first lo).  The partner is in general another lane's, or another wave's: it comes from LDS.
//   interleaved  a chunk inside the rotated columns holds 4 pairs of its own; table columns 4 (w - rot_off/8)
//   pass-through every other chunk (R == 0, the norm-only call: all of them)
// Forward: workgroup p holds the rows p * slots + slot.  Backward, per tensor (nparts and walk are functions of ITS row count
// and N): workgroup p of nparts walks the rows (it * nparts + p) * slots + slot, it = 0 .. walk - 1; its fp32 (N,) weight
// gradient partial sits p * N floats behind the tensor's first one (tensor 0's at the workspace's start, tensor 1's behind all
// nparts_0 * N_0 floats of tensor 0); the fold kernel sums a column's partials in
// kQkTokenFoldSlices runs of qktoken_fold_len(nparts) consecutive ones, then the runs' sums in index order.
#ifndef RFA_QKTOKEN_INDEX_H_
#define RFA_QKTOKEN_INDEX_H_

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RFA_QKTOKEN_HD __host__ __device__ __forceinline__
#else
#define RFA_QKTOKEN_HD inline
#endif

namespace rfa {

enum { kQkTokenLo = 0, kQkTokenHi = 1, kQkTokenInterleaved = 2, kQkTokenPass = 3 };
enum { kQkTokenThreads = 256, kQkTokenMaxWidth = 16384, kQkTokenMaxPerLane = 8, kQkTokenMaxParts = 512, kQkTokenFoldSlices = 8,
       kQkTokenFoldCols = 32 };

struct QkTokenGeom {
  uint32_t B, S, D;
  uint32_t R, rot_off;              // rotary width (0: norm only) and first rotated column of every head
  int32_t interleaved;
  uint32_t hchunks;                 // D / 8: chunks of one head
};

// one tensor of a call: element strides (batch, row, head) of the input x, of what is written (forward: the output; backward:
// dx) and — backward only — of the incoming gradient
struct QkTokenTensor {
  int64_t xb, xr, xh;
  int64_t ob, orow, oh;
  int64_t gb, gr, gh;
  uint32_t H;
  uint32_t N;                       // H * D
  uint32_t chunks;                  // N / 8
  uint32_t team;                    // qktoken_team(N)
  uint32_t rows;                    // B * S
};

// what a chunk of a row is; depends on the geometry and the chunk alone
struct QkTokenRole {
  int32_t kind;                     // kQkTokenLo / Hi / Interleaved / Pass
  uint32_t head, col;               // the chunk's head and its first column there
  uint32_t partner;                 // chunk of the row that holds the other half of the pairs (else the chunk itself)
  uint32_t tcol;                    // first column of the cos / sin row the chunk reads (8 values; interleaved: 4)
};

RFA_QKTOKEN_HD uint32_t qktoken_team(uint32_t N) {
  const uint32_t C = N / 8;
  return C <= 128 ? 64u : (C <= 512 ? 128u : 256u);
}

RFA_QKTOKEN_HD uint32_t qktoken_per_lane(uint32_t N) {
  const uint32_t team = qktoken_team(N);
  return (N / 8 + team - 1) / team;
}

RFA_QKTOKEN_HD uint32_t qktoken_slots(uint32_t team) { return (uint32_t)kQkTokenThreads / team; }

RFA_QKTOKEN_HD void qktoken_role(const QkTokenGeom& g, uint32_t c, QkTokenRole* r) {
  const uint32_t w = c % g.hchunks, first = g.rot_off / 8;
  r->head = c / g.hchunks;
  r->col = 8 * w;
  r->partner = c;
  r->tcol = 0;
  r->kind = kQkTokenPass;
  if (g.R == 0 || w < first || w >= first + g.R / 8) return;
  if (g.interleaved) {
    r->kind = kQkTokenInterleaved;
    r->tcol = 4 * (w - first);
  } else if (w < first + g.R / 16) {
    r->kind = kQkTokenLo;
    r->partner = c + g.R / 16;
    r->tcol = 8 * (w - first);
  } else {
    r->kind = kQkTokenHi;
    r->partner = c - g.R / 16;
    r->tcol = 8 * (w - first - g.R / 16);
  }
}

// ELEMENT offset of chunk (head, col) of row `row` under the strides (sb, sr, sh)
RFA_QKTOKEN_HD int64_t qktoken_offset(const QkTokenGeom& g, uint32_t row, uint32_t head, uint32_t col, int64_t sb, int64_t sr,
                                      int64_t sh) {
  return (int64_t)(row / g.S) * sb + (int64_t)(row % g.S) * sr + (int64_t)head * sh + col;
}

// forward: workgroups that cover `rows` rows, one step each
RFA_QKTOKEN_HD uint32_t qktoken_blocks(uint32_t rows, uint32_t team) {
  const uint32_t per = qktoken_slots(team);
  return rows / per + (rows % per ? 1u : 0u);
}

// backward: the number of workgroups = of weight gradient partials of a tensor — a function of its shape alone
RFA_QKTOKEN_HD uint32_t qktoken_parts(uint32_t rows, uint32_t team) {
  const uint32_t n = qktoken_blocks(rows, team);
  return n > (uint32_t)kQkTokenMaxParts ? (uint32_t)kQkTokenMaxParts : n;
}

// backward: steps a workgroup walks (the last ones may lie past the tensor's end)
RFA_QKTOKEN_HD uint32_t qktoken_walk(uint32_t rows, uint32_t nparts, uint32_t team) {
  const uint64_t per = (uint64_t)nparts * qktoken_slots(team);
  return per ? (uint32_t)((rows + per - 1) / per) : 0u;
}

// the row that slot `slot` of workgroup p holds in step `it` (forward: it = 0, nparts = the launch's blocks); may be >= rows
RFA_QKTOKEN_HD uint64_t qktoken_row(uint32_t it, uint32_t nparts, uint32_t p, uint32_t slot, uint32_t team) {
  return ((uint64_t)it * nparts + p) * qktoken_slots(team) + slot;
}

RFA_QKTOKEN_HD uint32_t qktoken_fold_len(uint32_t nparts) { return (nparts + kQkTokenFoldSlices - 1) / kQkTokenFoldSlices; }

RFA_QKTOKEN_HD int64_t qktoken_workspace_bytes(uint32_t nparts, uint32_t N) { return (int64_t)nparts * N * (int64_t)sizeof(float); }

}  // namespace rfa
#endif  // RFA_QKTOKEN_INDEX_H_
