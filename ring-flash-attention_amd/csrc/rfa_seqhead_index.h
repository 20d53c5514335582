// rfa_seqhead_index.h — the index arithmetic of the sequence/head exchange copies (rfa_seqhead.hip; include/rfa.h:
// rfa_seq_head_copy), in ONE function that the kernel and the stand-alone host check (tests/native/seqhead_check.cpp) share.
// Plain C++ without HIP types: the host check compiles it with any compiler.
//
// Three views of one tensor of a Ulysses group of U ranks (this rank at index p), per part (P = 1: q, k, v, out; 2: a packed
// kv; 3: qkv) and in units of one 16-byte chunk (8 elements of 2 bytes):
//   local    (B, S, P, H, D)        this rank's rows, all H = U * Hs heads          — any strides, last stride 1
//   merged   (B, U*S, P, Hs, D)     the U ranks' rows, this rank's head slice       — any strides, last stride 1
//   slots    U x [B][S][P][Hs][D]   the all-to-all buffer: slot j is what rank j gets (or what came from rank j), contiguous
// A chunk index c in [0, U*B*S*P*Hs*D/8) names one chunk of the slot side in memory order: c = ((((j*B + b)*S + i)*P + part)*Hs
// + hs)*D8 + d8.  Its place on the other side:
//   local:   (b, i, part, j*Hs + hs, 8*d8)             slot j <-> head slice j of every row
//   merged:  (b, m(j, i), part, hs, 8*d8)              slot j's row i <-> merged row m(j, i):
//       contiguous (ring)   m = j*S + i
//       zigzag (C = S/2)    m = i < C ? j*C + i : U*C + (U-1-j)*C + (i - C)
//       stripe              m = i*U + j
// The four ops are this one map read in both directions (rfa.h): PACK local -> slots, UNPACK slots -> merged,
// MERGED_TO_SLOTS merged -> slots, SLOTS_TO_HEADS slots -> local.
#ifndef RFA_SEQHEAD_INDEX_H_
#define RFA_SEQHEAD_INDEX_H_

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RFA_SEQHEAD_HD __host__ __device__ __forceinline__
#else
#define RFA_SEQHEAD_HD inline
#endif

namespace rfa {

enum { kSeqHeadPack = 0, kSeqHeadUnpack = 1, kSeqHeadMergedToSlots = 2, kSeqHeadSlotsToHeads = 3 };
enum { kSeqHeadContiguous = 0, kSeqHeadZigzag = 1, kSeqHeadStripe = 2 };

// one tensor of a call: element strides of its strided (local or merged) side, and where its part of every slot starts
struct SeqHeadTensor {
  int64_t batch, row, part, head;   // element strides of the strided side
  int64_t slot_base;                // element offset of this tensor's part inside a slot
  uint32_t P, Hs, rowchunks;        // parts, heads per slot, P * Hs * D8
  uint32_t nchunks;                 // U * B * S * rowchunks
};

struct SeqHeadGeom {
  int32_t op, layout;
  uint32_t U, B, S, D8;             // D8 = D / 8
  int64_t slot_stride;              // elements from slot j to slot j + 1 (the sum of the tensors' parts)
};

RFA_SEQHEAD_HD uint32_t seqhead_merged_row(int layout, uint32_t U, uint32_t S, uint32_t j, uint32_t i) {
  if (layout == kSeqHeadStripe) return i * U + j;
  if (layout == kSeqHeadZigzag) {
    const uint32_t C = S >> 1;
    return i < C ? j * C + i : U * C + (U - 1 - j) * C + (i - C);
  }
  return j * S + i;
}

// chunk c of tensor t: ELEMENT offsets of its 8 elements on the slot side and on the strided side
RFA_SEQHEAD_HD void seqhead_chunk(const SeqHeadGeom& g, const SeqHeadTensor& t, uint32_t c, int64_t* slot_off,
                                  int64_t* strided_off) {
  const uint32_t r = c % t.rowchunks;            // chunk inside the (part, head, d) run of one row: contiguous on the slot side
  uint32_t x = c / t.rowchunks;                  // (j*B + b)*S + i
  const uint32_t i = x % g.S;
  x /= g.S;
  const uint32_t b = x % g.B, j = x / g.B;
  const uint32_t hd = t.Hs * g.D8;
  const uint32_t part = r / hd, rem = r % hd;
  const uint32_t hs = rem / g.D8, d8 = rem % g.D8;
  *slot_off = (int64_t)j * g.slot_stride + t.slot_base + ((int64_t)(b * (int64_t)g.S + i) * t.rowchunks + r) * 8;
  const bool local = g.op == kSeqHeadPack || g.op == kSeqHeadSlotsToHeads;
  const int64_t row = local ? (int64_t)i : (int64_t)seqhead_merged_row(g.layout, g.U, g.S, j, i);
  const int64_t head = local ? (int64_t)j * t.Hs + hs : (int64_t)hs;
  *strided_off = (int64_t)b * t.batch + row * t.row + (int64_t)part * t.part + head * t.head + (int64_t)d8 * 8;
}

// true when the op reads the slot side (and writes the strided one)
RFA_SEQHEAD_HD bool seqhead_from_slots(int op) { return op == kSeqHeadUnpack || op == kSeqHeadSlotsToHeads; }

}  // namespace rfa
#endif  // RFA_SEQHEAD_INDEX_H_
