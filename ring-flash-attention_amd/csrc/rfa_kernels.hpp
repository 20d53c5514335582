// rfa_kernels.hpp — host-visible parameter blocks and launchers of the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rfa_common.hpp"
#include "rfa_seqhead_index.h"
#include "rfa_rotary_index.h"
#include "rfa_qknorm_index.h"
#include "rfa_maxlogit_band.h"
#include "rfa_rowrange.h"
#include "rfa_blockmask.h"

#include <atomic>
#include <type_traits>

namespace rfa {

// windowed instances are needed for a left bound, or for a right bound that is not the plain causal one
inline bool windowed(int causal, int wl, int wr) { return wl >= 0 || (wr >= 0 && !causal); }

// ---- what 32 bits inside a buffer descriptor allow (rfa.h: "row strides") ---------------------------------------------------
// The tile loaders form a tile's BASE with 64-bit products, but inside the descriptor everything is `int`: a lane's byte
// offset (row * row_stride + chunk * 8) * 2 and num_records = ((rows - 1) * row_stride + D) * 2, `rows` the rows of ONE
// descriptor.  kDescMaxRows is the largest such row count the contract allows for: the widest descriptor today spans 128
// rows (the V tile of the one-launch dK + dV kernels: kBgRows in rfa_bigd.hip, kVdRows in rfa_vdim.hip; K/V, Q/dO tiles
// span 64, the per-wave Q / out tiles 32), and 256 is the widest tile any workgroup owns (the rows of the 8-wave forward
// and dQ, the keys of the 256-key dK/dV form), so a loader may span its workgroup's whole tile without changing the
// contract.  The kernel files static_assert the tile constants their descriptors are sized by today (kFwdKV, kDqKV, kKvQ,
// kDsKV, kMlKV, kBgRows, kVdRows) against it — a reminder next to the constants, not a proof: a loader that builds a
// descriptor over another row count has to be checked against kDescMaxRows by whoever writes it.  rfa_api.cpp refuses
// (RFA_ERR_ARGS, before any launch) a row stride for which kDescMaxRows * row_stride * elt + D * elt would pass 2^31 - 1.
constexpr int kDescMaxRows = 256;
constexpr bool desc_row_stride_ok(int64_t row_stride, int D, int elt_bytes) {
  const int64_t r = row_stride < 0 ? -row_stride : row_stride;
  return r <= (int64_t)INT32_MAX && (int64_t)kDescMaxRows * r * elt_bytes + (int64_t)D * elt_bytes <= (int64_t)INT32_MAX;
}
// ---- what a launch can express: grid.y / grid.z up to 65535, a 1-D grid up to 2^31 - 1 blocks (rfa_api.cpp refuses more) ----
constexpr int64_t kGridYZMax = 65535;
constexpr int64_t kGridXMax = INT32_MAX;

// launcher status codes (rfa_api.cpp maps them to rfa_status)
enum { kLaunchOk = 0, kLaunchFailed = -1, kLaunchAttrFailed = -2 };

// Dynamic-LDS opt-in (hipFuncAttributeMaxDynamicSharedMemorySize) is a PER-DEVICE attribute of a kernel:
// `done` is a bit mask indexed by device ordinal, so a process driving several GPUs opts every device in,
// the call is made once per (kernel, device), concurrent first launches are benign (the attribute is
// idempotent), and a failure is reported instead of surfacing later as a generic launch error.
inline int opt_in_dynamic_lds(const void* kernel, int bytes, std::atomic<unsigned long long>& done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return kLaunchAttrFailed;
  const unsigned long long bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return kLaunchOk;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return kLaunchAttrFailed;
  }
  done.fetch_or(bit, std::memory_order_release);
  return kLaunchOk;
}

struct FwdParams {
  const void *q, *k, *v;
  void* out;
  float* lse;
  float* out_acc;
  float* lse_acc;
  const int32_t *cu_q, *cu_k;
  Strides q_st, k_st, v_st, out_st, out_acc_st;
  int64_t lse_batch, lse_head, lse_acc_batch, lse_acc_head;
  int B, H, Hk, D, Sq, Sk;
  int q_half, k_half;
  int causal, acc_init;
  int wl, wr;          // visible keys of query i: i + (Sk - Sq) + shift - wl <= j <= i + (Sk - Sq) + shift + wr; -1 = unbounded
                       // (causal is folded in by the API layer: wr = 0)
  int shift;           // rfa.h: mask_shift after the API layer's band normalisation (dense input only; the plain causal bound too)
  int shift_lens;      // rfa.h: mask_shift_lens — packed input only (dense calls fold it into shift): sequence b's band is moved by
                       // shift_lens * len_k(b), so every derived tile range / dark-workgroup exit follows the sequence's own length
  int nqblk;
  int qrows;           // query rows per workgroup the launch was sized for: 256 (8 waves) or 128 (4 waves, small grids)
  int persist_grid;    // > 0: the persistent 256-row form (fwd_persist_kernel) with this many workgroups
  // split-KV launches (short query ranges against long key ranges on under-filled grids): the key tiles of a workgroup's
  // range are divided between kv_nsplit workgroups; split s writes a NORMALISED partial (out fp32, lse; -inf = no key)
  // to part_out + s * part_out_split / part_lse + s * part_lse_split (laid out like out_acc / lse_acc), and
  // combine_kernel (rfa_aux.hip) merges the splits into the call's real outputs
  int kv_nsplit;
  float* part_out;
  float* part_lse;
  int64_t part_out_split, part_lse_split;
  float scale;
  // dropout (rfa_common.hpp: drop_word): keep threshold 0..256 (256 = off), scale of kept probabilities, seed and
  // the offsets that turn local (head, query position, key position) into global ones
  unsigned drop_keep;
  float drop_scale;
  unsigned long long drop_seed;
  unsigned q_pos0, k_pos0, head0;
  // position map of the mask (rfa.h: q_pos_stride ...; rfa_common.hpp: drop_pos): strides >= 1, split 0 = one piece;
  // drop_mapped = some field is not the identity's — the kernels then leave the word-per-four-keys path
  unsigned q_pstride, k_pstride;
  int q_psplit, k_psplit;
  unsigned q_pos2, k_pos2;
  int drop_mapped;
  // ALiBi (rfa.h: rfa_ext_args; the kBias instances only): alibi = nullptr is off.  The slope of (batch b, head h) is
  // alibi[b * alibi_bstride + h]; the kernels take it in SCORE units (slope * alibi_rscale, alibi_rscale = 1 / softmax_scale,
  // prepared by the API layer) because their row max runs on unscaled scores; alibi_shift as rfa.h (fits 32 bits: API layer)
  const float* alibi;
  int64_t alibi_bstride;
  int alibi_shift;
  float alibi_rscale;
  // logit soft-capping (rfa.h: rfa_ext_args.softcap; the kCap instances only): cap = softcap, 0 is off.  The two constants
  // of the kernels, made once by the API layer: t = cap_tanh(s * cap_in) with cap_in = 2 log2(e) softmax_scale / softcap
  // (rfa_common.hpp), and the exponent constant cap_c = softcap log2(e) that takes the place of softmax_scale log2(e)
  float cap, cap_in, cap_c;
};

struct PreParams {
  const void *dout, *out;
  float* delta;
  const int32_t* cu_q;
  Strides dout_st, out_st;
  int64_t delta_batch, delta_head;
  int B, H, D, Sq, q_half;
  // the gradient of lse (fp32, laid out like delta with strides of its own): the kDlse instance stores delta - dlse, the plain
  // instance never reads these fields
  const float* dlse;
  int64_t dlse_batch, dlse_head;
};

struct BwdParams {
  const void *dout, *q, *k, *v;
  const float *lse, *delta;
  void *dq;            // io dtype (or nullptr when dq_acc)
  float* dq_acc;
  void *dk, *dv;       // per-q-head outputs, io dtype: head index = q head
  const int32_t *cu_q, *cu_k;
  Strides dout_st, q_st, k_st, v_st, dq_st, dq_acc_st, dk_st, dv_st;
  int64_t lse_batch, lse_head, delta_batch, delta_head;
  int B, H, Hk, D, Sq, Sk;
  int q_half, k_half;
  int causal, acc_init;
  int wl, wr;          // attention window as in FwdParams (causal: wr = 0)
  int shift;           // as in FwdParams
  int shift_lens;      // as in FwdParams
  int kv_f32;          // dk / dv point to fp32 buffers (overwritten), strides in fp32 elements
  void* ds;            // dS spill scratch (rfa_dqs.hip) or nullptr: dkdv_kernel stores its packed dS blocks there
  int ds_tri, ds_c;    // scratch rows are triangular (dense causal calls): row qt holds key blocks 0 .. min(nKb, qt + ds_c) - 1
  int ds_packed;       // packed (cu_seqlens) layout of the scratch: [head][global query-block row][key block], see ds_rowpart()
  int64_t ds_head_blocks;   // blocks per head (dense: per (batch, head))
  int nqblk, nkblk;
  float scale;
  // 256-key dK/dV form (dkdv_kernel kWide): the tile range of a key block is shared by nsplit workgroups; split s
  // stores its partial kv_split_stride elements behind split 0's (rfa_api.cpp lays them out for reduce_kernel)
  int wide, nsplit;
  int64_t kv_split_stride;
  int kv_part_f32;     // dk / dv point to fp32 PARTIALS in the workspace (split launches): fp32 stores, strides in fp32 elements
  int kv_accum;        // fp32 stores ADD to what the partial holds (later query-head fractions of a chunked dS hand-off)
  // balanced causal schedule of the 256-key form (dkdv_kernel kBal; rfa_api.cpp: bwd_dkdv_plan): B * Hk * nkblk / 2 pair
  // slots of 8 waves x 2 tensors x D / 32 x 4 KiB (fp32 accumulators in lane order) and one flag word per pair
  // (0 = nobody yet, 1 = the first arriver is publishing, 2 = published), zeroed by a kernel of the launcher's before every launch
  int bal;
  void* pair_ws;
  unsigned* pair_flags;
  // dropout (rfa_common.hpp: drop_word): keep threshold 0..256 (256 = off), scale of kept probabilities, seed and
  // the offsets that turn local (head, query position, key position) into global ones
  unsigned drop_keep;
  float drop_scale;
  unsigned long long drop_seed;
  unsigned q_pos0, k_pos0, head0;
  // position map of the mask (rfa.h: q_pos_stride ...; rfa_common.hpp: drop_pos): strides >= 1, split 0 = one piece;
  // drop_mapped = some field is not the identity's — the kernels then leave the word-per-four-keys path
  unsigned q_pstride, k_pstride;
  int q_psplit, k_psplit;
  unsigned q_pos2, k_pos2;
  int drop_mapped;
  // ALiBi (rfa.h: rfa_ext_args; the kBias instances only): alibi = nullptr is off.  The slope of (batch b, head h) is
  // alibi[b * alibi_bstride + h]; the kernels take it in SCORE units (slope * alibi_rscale, alibi_rscale = 1 / softmax_scale,
  // prepared by the API layer) because their row max runs on unscaled scores; alibi_shift as rfa.h (fits 32 bits: API layer)
  const float* alibi;
  int64_t alibi_bstride;
  int alibi_shift;
  float alibi_rscale;
  // logit soft-capping (rfa.h: rfa_ext_args.softcap; the kCap instances only): cap = softcap, 0 is off.  The two constants
  // of the kernels, made once by the API layer: t = cap_tanh(s * cap_in) with cap_in = 2 log2(e) softmax_scale / softcap
  // (rfa_common.hpp), and the exponent constant cap_c = softcap log2(e) that takes the place of softmax_scale log2(e)
  float cap, cap_in, cap_c;
};

// dst[b, row, hk, :] (=|+=) sum_g src[b, row, hk*G+g, :]
struct ReduceParams {
  const void* src;     // partials (io dtype, or fp32 when src_f32), head index = q head
  void* dst;           // io dtype (or nullptr)
  float* dst_acc;      // fp32 accumulate target (or nullptr)
  // optional second tensor reduced by the same launch (blockIdx.z = 1): dV next to dK
  const void* src2;
  void* dst2;
  float* dst_acc2;
  const int32_t* cu_k;
  Strides src_st, dst_st, dst_acc_st, dst2_st, dst_acc2_st;
  int B, Hk, G, D, Sk, k_half, acc_init;
  int src_f32;
  int64_t g_stride;    // 0: member g of head hk is source head hk*G+g; else: head hk, g_stride elements further per g
};

// combine the kv_nsplit partial (out, lse) pairs of a split-KV forward launch into the call's outputs
struct CombineParams {
  const float* part_out;    // (nsplit, ...) laid out like out_acc: strides part_st, split stride part_out_split
  const float* part_lse;
  Strides part_st;
  int64_t part_lse_batch, part_lse_head, part_out_split, part_lse_split;
  int nsplit;
  void* out;                // io dtype (plain mode) or nullptr
  float* lse;
  float* out_acc;           // fp32 accumulate mode or nullptr
  float* lse_acc;
  Strides out_st, out_acc_st;
  int64_t lse_batch, lse_head, lse_acc_batch, lse_acc_head;
  const int32_t* cu_q;
  int B, H, D, Sq, q_half, acc_init;
};

struct MergeParams {
  float* out_acc;
  float* lse_acc;
  const void* block_out;
  const float* block_lse;
  Strides out_acc_st, block_out_st;
  int64_t lse_acc_batch, lse_acc_head, block_lse_batch, block_lse_head;
  int64_t lse_acc_row, block_lse_row;
  int B, H, D, S, acc_init;
};

// attention sinks (rfa_sink.hip): lse' = logaddexp(lse, sinks[h]), out' = out * exp(lse - lse'); B x S rows of H heads
// (packed input: B = 1, S = total rows, batch strides unused); lse row stride 1
struct SinkApplyParams {
  const void* out_src;
  void* out_dst;            // may be out_src
  const float* lse_src;
  float* lse_dst;           // may be lse_src
  const float* sinks;       // (H,)
  Strides out_src_st, out_dst_st;
  int64_t lse_src_batch, lse_src_head, lse_dst_batch, lse_dst_head;
  int B, H, D, S;
};

// dsink[h] = - sum_rows exp(sinks[h] - lse') rowsum(dout * out'): partials per (batch, chunk of kSinkGradRows rows, head),
// then their sum in index order
struct SinkGradParams {
  const void* dout;
  const void* out;
  const float* lse;
  const float* sinks;
  float* dsink;             // (H,)
  float* partial;           // sink_grad_parts(B, S) * H floats
  Strides dout_st, out_st;
  int64_t lse_batch, lse_head;
  int B, H, D, S;
};
constexpr int kSinkGradRows = 256;
int64_t sink_grad_parts(int B, int S);
int launch_sink_apply(const SinkApplyParams& p, int dtype, hipStream_t stream);
int launch_sink_grad(const SinkGradParams& p, int dtype, hipStream_t stream);

// sequence/head exchange copies (rfa_seqhead.hip; index arithmetic: rfa_seqhead_index.h): up to three tensors per launch
// between their strided side and the all-to-all slot buffer, 16 bytes per thread
struct SeqHeadParams {
  SeqHeadGeom g;
  SeqHeadTensor t[3];
  void* strided[3];         // read by PACK / MERGED_TO_SLOTS, written by UNPACK / SLOTS_TO_HEADS
  void* slots;              // the other side
  int ntensors;
};
int launch_seq_head_copy(const SeqHeadParams& p, hipStream_t stream);

// rotary position embedding (rfa_rotary.hip; index arithmetic: rfa_rotary_index.h): up to two tensors (q, k) per launch, one
// thread per unit.  positions != NULL: row i of batch entry b sits at pos_off + positions[b * pos_batch + i]; NULL: at the
// position map (pos_off, pos_stride, pos_split, pos_off2).  Either way clamped to [0, P - 1] where the tables are read.
struct RotaryParams {
  RotaryGeom g;
  RotaryTensor t[2];
  const void* src[2];
  void* dst[2];             // == src[k]: in place
  const void *cos, *sin;    // (P, R/2), contiguous, fp32 or the io dtype
  int64_t P;
  const int32_t* positions;
  int64_t pos_batch;
  int64_t pos_off, pos_off2;
  uint32_t pos_stride;
  int32_t pos_split;
  int32_t conj;             // s -> -s: the inverse rotation = the backward
  int ntensors;
};
int launch_rotary(const RotaryParams& p, int dtype, bool table_f32, hipStream_t stream);

// per-head QK RMSNorm fused with the rotary embedding (rfa_qknorm.hip; index arithmetic: rfa_qknorm_index.h): up to two tensors
// (q, k) per launch, one lane per 16-byte chunk, one (row, head) per lane group.  Positions as in RotaryParams; R == 0 (cos ==
// sin == NULL) is the norm alone.  Backward: dout / dx per tensor, dweight[k] != NULL asks for that tensor's fp32 (D,) weight
// gradient (workspace: tensor 0's nparts[0] partials, then tensor 1's nparts[1]; then the fold launch).
struct QkNormParams {
  QkNormGeom g;
  QkNormTensor t[2];
  const void* x[2];
  void* out[2];             // forward: y; backward: dx
  const void* dout[2];      // backward only
  const void* weight[2];    // (D,), fp32 or the io dtype
  float* dweight[2];        // backward: fp32 (D,) or NULL
  float* workspace;
  uint32_t nparts[2], walk[2]; // backward, per tensor (a function of ITS items alone): workgroups = partials, items a lane group walks
  float eps, weight_offset;
  const void *cos, *sin;
  int64_t P;
  const int32_t* positions;
  int64_t pos_batch;
  int64_t pos_off, pos_off2;
  uint32_t pos_stride;
  int32_t pos_split;
  int ntensors;
};
int launch_qknorm_fwd(const QkNormParams& p, int dtype, bool table_f32, bool weight_f32, hipStream_t stream);
int launch_qknorm_bwd(const QkNormParams& p, int dtype, bool table_f32, bool weight_f32, hipStream_t stream);

// per-head max attention logit (rfa_maxlogit.hip; tile arithmetic: rfa_maxlogit_band.h): the forward's S phase alone.
// Workgroup (batch b, query block qb, head h) stores the max of its UNSCALED visible scores to
// partial[h * nparts + b * nqblk + qb] (-inf: it saw nothing), nparts = B * nqblk; maxlogit_finish_kernel folds a head's
// partials in index order, multiplies by `scale` once and writes or max-accumulates dst[h].  nparts == 0 (an empty band): only
// the finish kernel runs, with -inf.
struct MaxLogitParams {
  const void *q, *k;
  const int32_t *cu_q, *cu_k;
  Strides q_st, k_st;
  int B, H, Hk, D, Sq, Sk;
  int q_half, k_half;
  int wl, wr;          // as in FwdParams (causal: wr = 0)
  int64_t shift;       // dense: after the band normalisation; packed: 0
  int shift_lens;      // packed input only
  int nqblk;
  float* partial;
  float* dst;          // (H,)
  float scale;
  int accumulate;
};
int launch_max_logit(const MaxLogitParams& p, int dtype, bool attention, hipStream_t stream);

int launch_fwd(const FwdParams& p, int dtype, hipStream_t stream);
int fwd_qrows_per_block();
// head dims 129 .. 256 (rfa_bigd.hip): same parameter blocks; the launchers set their own nqblk / nkblk
constexpr int kMaxHeadDim = 256;
int launch_fwd_big(const FwdParams& p, int dtype, hipStream_t stream);
int launch_bwd_dq_big(const BwdParams& p, int dtype, hipStream_t stream);
int launch_bwd_dkdv_big(const BwdParams& p, int dtype, hipStream_t stream);
// a value head dim of its own (rfa_vdim.hip): QK head dims 136 .. 192 (D of the block), V head dims 8 .. 128 (Dv).  The blocks
// above stay as they are — and with them the kernarg of every other kernel; v_st / out_st / out_acc_st / dout_st / dv_st
// describe Dv-wide rows
constexpr int kVdMinHeadDim = 136, kVdMaxHeadDim = 192, kVdMaxHeadDimV = 128;
struct FwdParamsVd {
  FwdParams base;
  int Dv;
};
struct BwdParamsVd {
  BwdParams base;
  int Dv;
};
int launch_fwd_vd(const FwdParams& p, int Dv, int dtype, hipStream_t stream);
int launch_bwd_dq_vd(const BwdParams& p, int Dv, int dtype, hipStream_t stream);
int launch_bwd_dkdv_vd(const BwdParams& p, int Dv, int dtype, hipStream_t stream);

// per-row key ranges (rfa.h: rfa_rowrange_args; arithmetic: rfa_rowrange.h): the kRng instances of the 8 x 32 forward, the
// 7-GEMM dQ kernel and the 128-key dK/dV kernel take the block above with this one behind it — the blocks above stay as they
// are, and with them the kernarg of every other kernel.  Dense input, head dims <= 128, built on the windowed instances.
struct RowRangeParams {
  const int32_t *start, *end;   // (B, Sq) global key positions, row stride 1
  int64_t bstride;              // batch stride of both, in elements
  int64_t k_pos0;               // global position of the block's key row 0
  int2* tile_bounds;            // dK/dV only: (min lo, max hi), block-relative, per (batch, 64-row query tile)
  int ntile_q;                  // query tiles per batch entry in tile_bounds
};
struct FwdParamsRr : FwdParams {
  RowRangeParams rr;
};
struct BwdParamsRr : BwdParams {
  RowRangeParams rr;
};
constexpr int kRrTileRows = 64;                // query rows per entry of tile_bounds: the dK/dV kernel's Q/dO tile
constexpr bool kRngPadded128 = true;           // the zero-padded 128-wide dK/dV instance (head dims 65 .. 127) is built
int launch_fwd_rr(const FwdParams& p, const RowRangeParams& r, int dtype, hipStream_t stream);
int launch_bwd_dq_rr(const BwdParams& p, const RowRangeParams& r, int dtype, hipStream_t stream);
int launch_bwd_dkdv_rr(const BwdParams& p, const RowRangeParams& r, int dtype, hipStream_t stream);   // (fills tile_bounds first)

// block-sparse masks (rfa.h: rfa_blockmask_args; arithmetic: rfa_blockmask.h): the kBlk instances of the same three kernels —
// one byte per (query block, key block) pair of 128 x 128 positions; the tile walks become list-driven.  As above, the block
// travels behind the parameter block of before, whose layout (and every other kernel's kernarg) stays as it is.
struct BlockMaskParams {
  const uint8_t* mask;          // (Bm, Hm, nq blocks, nk_blocks) bytes, non-zero = lit
  int64_t bstride, hstride;     // bytes between two batch entries / query heads (0: shared)
  int64_t rstride;              // bytes between two query blocks
  int nk_blocks;                // columns of the mask: key blocks of the whole sequence
  int k_blk0;                   // column of the block's key row 0 (any sign)
};
struct FwdParamsBm : FwdParams {
  BlockMaskParams bm;
};
struct BwdParamsBm : BwdParams {
  BlockMaskParams bm;
};
template <bool kRng, bool kBlk> using fwd_params_t = std::conditional_t<kBlk, FwdParamsBm, std::conditional_t<kRng, FwdParamsRr, FwdParams>>;
template <bool kRng, bool kBlk> using bwd_params_t = std::conditional_t<kBlk, BwdParamsBm, std::conditional_t<kRng, BwdParamsRr, BwdParams>>;
constexpr int kBmMaxGroup = 64;                // query heads per K/V head the dK/dV item walk holds in one window (rfa_blockmask.h)
int launch_fwd_bm(const FwdParams& p, const BlockMaskParams& m, int dtype, hipStream_t stream);
int launch_bwd_dq_bm(const BwdParams& p, const BlockMaskParams& m, int dtype, hipStream_t stream);
int launch_bwd_dkdv_bm(const BwdParams& p, const BlockMaskParams& m, int dtype, hipStream_t stream);

int launch_preprocess(const PreParams& p, int dtype, hipStream_t stream);
// soft cap + bounded window at head dims 65 .. 127: the zero-padded 128-wide dK/dV instance with both flags needs 40 bytes of
// scratch / 9 spilled registers, beyond what the padded instances are allowed (32 / 4) — with the read-ahead reduced by one or
// by two pairs alike — so it is not built and rfa_api.cpp refuses such calls (profiles/softcap.md)
constexpr bool kCapPaddedWin = false;
int launch_bwd_dq(const BwdParams& p, int dtype, hipStream_t stream);
int launch_bwd_dkdv(const BwdParams& p, int dtype, hipStream_t stream);
// dQ = scale * dS K from the dS blocks a preceding launch_bwd_dkdv (with p.ds set) stored; dense, D == 128
int launch_bwd_dq_from_ds(const BwdParams& p, int dtype, hipStream_t stream);
constexpr int kDsBlockBytes = 2048;
// rows / columns of 32 x 32 dS blocks the spill scratch reserves per (sequence, head): the longest (half) sequence
__host__ __device__ inline int ds_blocks(int S, int half) { return ((half ? (S + 1) / 2 : S) + 31) >> 5; }   // one (32 query x 32 key) block of dS in the io dtype
// Layout of the dS scratch of one (sequence, head): rows qt = query row / 32 of 2 KiB blocks kb = key / 32.
//   rectangular (packed input, non-causal): every row holds nKb blocks;
//   triangular (dense causal: block (qt, kb) is visited iff kb < qt + c, c = ((31 + lk - lq) >> 5) + 1): row qt holds
//   its first ds_row_len(qt) = clamp(qt + c, 0, nKb) blocks, rows packed back to back — half the scratch of a
//   square causal launch.  ds_row_off(nQt, ...) is the number of blocks per (sequence, head).
__host__ __device__ inline int ds_row_len(int qt, int nKb, int c, int tri) {
  if (!tri) return nKb;
  const int n = qt + c;
  return n < 0 ? 0 : (n > nKb ? nKb : n);
}
__host__ __device__ inline int64_t ds_row_off(int qt, int nKb, int c, int tri) {
  if (!tri) return (int64_t)qt * nKb;
  const int iA = c < 0 ? -c : 0;                        // first row with a non-negative length
  int iB = nKb - c;                                     // first row at full length
  iB = iB < iA ? iA : iB;
  const int e1 = qt < iB ? qt : iB;
  const int64_t n1 = e1 > iA ? e1 - iA : 0;
  const int64_t n2 = qt > iB ? qt - iB : 0;
  return n1 * (iA + c) + n1 * (n1 - 1) / 2 + n2 * nKb;
}
// Where the dS blocks of query-block row qt (counted inside its (half) sequence) live, in blocks from the scratch base:
//     ds_base_blocks(p, b) + hc * p.ds_head_blocks + ds_rowpart(p, qt, g0, nKb)          (hc: head index inside the launch)
//   dense:  [batch][head][rows], rows rectangular or packed triangular (ds_row_off above);
//   packed: [head][g][nKb] with the GLOBAL row index g = g0 + qt, g0 = (first packed row of the (half) sequence >> 5)
//           + sequence index — unique per (sequence, row) because ceil(len / 32) <= floor(end / 32) - floor(start / 32) + 1.
//           The scratch then holds total_q / 32 + B rows per head instead of B x max_seqlen / 32: bounded by the PACKED
//           row count whatever the mix of sequence lengths (one long and two short sequences used to cost three
//           times the longest: 10.5 GB instead of 3.9 GB for the varlen benchmark's second pattern).
__host__ __device__ inline int64_t ds_base_blocks(const BwdParams& p, int b) {
  return p.ds_packed ? 0 : (int64_t)b * p.H * p.ds_head_blocks;
}
__host__ __device__ inline int64_t ds_rowpart(const BwdParams& p, int qt, int64_t g0, int nKb) {
  return p.ds_packed ? (g0 + qt) * (int64_t)nKb : ds_row_off(qt, nKb, p.ds_c, 1);
}
__host__ __device__ inline int ds_rowlen(const BwdParams& p, int qt, int nKb) {
  return p.ds_packed ? nKb : ds_row_len(qt, nKb, p.ds_c, 1);
}
int bwd_dq_rows_per_block();
int bwd_dkdv_keys_per_block(bool wide);
int launch_reduce(const ReduceParams& p, int dtype, hipStream_t stream);
int launch_merge(const MergeParams& p, int dtype, hipStream_t stream);

// pairwise merge of two finished (out, lse) pairs and its backward (rfa_mergepair.hip): B x S rows of H heads (packed input:
// B = 1, S = total rows, batch strides unused); every lse-like tensor has row stride 1 and (batch, head) strides of its own
struct LseSt { int64_t batch, head; };
struct MergePairParams {
  const void *out_a, *out_b;
  void* out;
  const float *lse_a, *lse_b;
  float* lse;
  Strides out_a_st, out_b_st, out_st;
  LseSt lse_a_st, lse_b_st, lse_st;
  int B, H, D, S;
};
struct MergePairBwdParams {
  const void *dout, *out_a, *out_b;
  const float *dlse;        // may be nullptr: zero
  const float *lse_a, *lse_b;
  void *dout_a, *dout_b;
  float *dlse_a, *dlse_b;
  Strides dout_st, out_a_st, out_b_st, dout_a_st, dout_b_st;
  LseSt dlse_st, lse_a_st, lse_b_st, dlse_a_st, dlse_b_st;
  int B, H, D, S;
};
int launch_merge_pair(const MergePairParams& p, int dtype, hipStream_t stream);
int launch_merge_pair_bwd(const MergePairBwdParams& p, int dtype, hipStream_t stream);
int launch_combine(const CombineParams& p, int dtype, hipStream_t stream);
int launch_cast(void* dst, const float* src, int64_t n, int dtype, hipStream_t stream);
int launch_lse_relayout(float* dst, const float* src, const int32_t* cu, int B, int H,
                        int max_seqlen, int64_t packed_head_stride, int64_t packed_row_stride,
                        bool flatten, hipStream_t stream);

}  // namespace rfa
