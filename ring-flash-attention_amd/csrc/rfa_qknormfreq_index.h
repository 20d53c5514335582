// rfa_qknormfreq_index.h — the index arithmetic of the per-head QK RMSNorm fused with a rotary embedding whose angles are formed
// in the kernel (rfa_qknormfreq.hip; include/rfa.h: rfa_qk_norm_rotary_freqs_fwd / _bwd), in functions that the kernels, the C
// entry points and the stand-alone host check (tests/native/qknormfreq_check.cpp) share.  Plain C++ without HIP types.
//
// It joins two splits of the work that exist already.  From rfa_rotfreq_index.h: a workgroup owns a TILE of kQkNfRows
// consecutive rows of one batch entry (rotfreq_tile(), the last tile of a batch entry ragged) and computes the tile's
// nrows x R/2 (cos', sin') entries ONCE for all heads of q and k into two LDS arrays [rows][R/2], a row's quads permuted by
// rotfreq_lds_col() so that a lane's 8 values are two conflict-free 16-byte reads (interleaved: one, in column order).  From
// rfa_qknorm_index.h: an ITEM is one (row, head); it lives in a LANE GROUP of G = qknorm_group(D) lanes, lane w < D/8 owning
// the 8 columns at 8 w, with the role, the partner lane and the table columns of qknorm_lane() — so the row sums have the order
// of the table kernel, whatever is rotated.
// What is new: the items of a tile.  Tensor k has nrows * H_k of them, item j = r * H_k + h (row r of the tile, head h); the
// workgroup's 256/G lane groups walk them in PASSES, pass s holding items s * (256/G) + group; qknf_passes() of them, the
// same for every lane (groups past the tile's end hold zeros and take part in every shuffle).  First all passes of q, then k's.
// Backward: workgroup p of nparts = min(tiles, kQkNfMaxParts) walks the tiles p, p + nparts, .. (qknf_walk() of them, the
// angle phase repeated for each); nparts depends on B and S alone, which the tensors of a call share.  The fp32 (D,) weight
// gradient partial of workgroup p for tensor k sits at workspace[(k * nparts + p) * D]; the fold kernel sums a column's
// partials in kQkNormFoldSlices runs of qknorm_fold_len(nparts) consecutive ones, then the runs' sums in index order.
#ifndef RFA_QKNORMFREQ_INDEX_H_
#define RFA_QKNORMFREQ_INDEX_H_

#include "rfa_qknorm_index.h"
#include "rfa_rotfreq_index.h"

namespace rfa {

// rows of a tile.  The angle phase costs nrows * R/2 sincosf per workgroup whatever the heads — it wants a HIGH tile, one
// sincosf or more per thread — while the norm phase, like rfa_rotfreq's stream phase, is fastest with many small workgroups in
// flight.  Measured at q (1, 8192, 32, 128) + k (1, 8192, 8, 128) (profiles/qk_norm_freqs.md): see there for the heights timed.
// LDS: 2 arrays * 4 rows * 128 fp32 = 4 KiB, the backward 8 KiB more for the fold of its lane groups.
enum { kQkNfRows = 4, kQkNfThreads = 256, kQkNfMaxParts = 1024 };

// items of tensor `H` heads in a tile of nrows rows, and the passes the workgroup's lane groups need for them
RFA_QKNORM_HD uint32_t qknf_tile_items(uint32_t nrows, uint32_t H) { return nrows * H; }
RFA_QKNORM_HD uint32_t qknf_passes(uint32_t nrows, uint32_t H, uint32_t group) {
  const uint32_t per = kQkNfThreads / group;
  return (qknf_tile_items(nrows, H) + per - 1) / per;
}

// chunk w of item j of a tile: row, head and the ELEMENT offsets on the three sides (c->b = the tile's batch entry, c->i the
// row inside the batch entry)
RFA_QKNORM_HD void qknf_chunk(const QkNormTensor& t, const RotFreqTile& tile, uint32_t j, uint32_t w, QkNormChunk* c) {
  const uint32_t r = j / t.H;
  c->h = j - r * t.H;
  c->i = tile.row0 + r;
  c->b = tile.b;
  c->x = (int64_t)c->b * t.xb + (int64_t)c->i * t.xr + (int64_t)c->h * t.xh + 8 * w;
  c->o = (int64_t)c->b * t.ob + (int64_t)c->i * t.orow + (int64_t)c->h * t.oh + 8 * w;
  c->g = (int64_t)c->b * t.gb + (int64_t)c->i * t.gr + (int64_t)c->h * t.gh + 8 * w;
}

// first float of the 4 that a lane reads from row r of the tile's LDS arrays: q = 0 for table columns tcol .. tcol+3, q = 1
// (halves only) for tcol+4 .. tcol+7; a multiple of 4
RFA_QKNORM_HD uint32_t qknf_lds_at(uint32_t half, int interleaved, uint32_t r, uint32_t tcol, uint32_t q) {
  return r * half + rotfreq_lds_quad(half, interleaved, tcol, q);
}

RFA_QKNORM_HD uint32_t qknf_tiles(uint32_t B, uint32_t S, uint32_t rows = kQkNfRows) { return B * rotfreq_tiles_per_batch(S, rows); }

// backward: workgroups = weight gradient partials per tensor, and the tiles a workgroup walks
RFA_QKNORM_HD uint32_t qknf_parts(uint32_t tiles) { return tiles > (uint32_t)kQkNfMaxParts ? (uint32_t)kQkNfMaxParts : tiles; }
RFA_QKNORM_HD uint32_t qknf_walk(uint32_t tiles, uint32_t nparts) { return nparts ? (tiles + nparts - 1) / nparts : 0u; }

}  // namespace rfa
#endif  // RFA_QKNORMFREQ_INDEX_H_
