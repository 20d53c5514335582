/*
 * rfa.h — C ABI of librfa_hip.so, the MI355X (gfx950) attention operator library.
 *
 * This is the drop-in boundary of the hot path.  Each entry point replaces one private
 * function of the (un-vendored, CUDA-only) `flash_attn.flash_attn_interface` module that the
 * reference calls, or one eager/Triton helper of the reference itself:
 *
 *   rfa_fwd            <- flash_attn._flash_attn_forward          (call sites
 *                         /root/reference/ring_flash_attn/ring_flash_attn.py:53,
 *                         zigzag_ring_flash_attn.py:52) and
 *                         flash_attn._flash_attn_varlen_forward   (ring_flash_attn_varlen.py:77,
 *                         zigzag_ring_flash_attn_varlen.py:137, llama3_flash_attn_varlen.py:147)
 *                         plus, when `out_acc/lse_acc` are given, the fused form of
 *                         update_out_and_lse (ring_flash_attn/utils.py:32-73).
 *   rfa_bwd_preprocess <- the rowsum(dO*O) prologue inside flash_attn._flash_attn_backward.
 *   rfa_bwd            <- flash_attn._flash_attn_backward          (ring_flash_attn.py:131,
 *                         zigzag_ring_flash_attn.py:156) and _flash_attn_varlen_backward
 *                         (ring_flash_attn_varlen.py:169, zigzag_ring_flash_attn_varlen.py:275,
 *                         llama3_flash_attn_varlen.py:282), plus, when `*_acc` are given, the
 *                         fp32 `dq += ...`, `dk += ...` accumulation of
 *                         zigzag_ring_flash_attn.py:164-187 / ring_flash_attn.py:134-141.
 *   rfa_merge          <- _update_out_and_lse (ring_flash_attn/utils.py:32-50) as a stand-alone
 *                         kernel (also covers the slice_ variant, utils.py:65-70).
 *   rfa_lse_flatten / rfa_lse_unflatten
 *                      <- triton_utils.flatten_varlen_lse / unflatten_varlen_lse
 *                         (ring_flash_attn/triton_utils.py:39-67,103-137).
 *   rfa_cast           <- `out.to(q.dtype)` / `dq.to(q.dtype)` tails (zigzag_ring_flash_attn.py:86,199).
 *
 * Conventions
 *   - Plain C, no torch types.  All pointers are DEVICE pointers owned by the caller.  The
 *     library never allocates, frees or synchronises; every launch goes to the `stream`
 *     argument (a hipStream_t passed as void*).
 *   - All strides are in ELEMENTS of the tensor's own dtype.  The innermost (head_dim) stride
 *     must be 1 and every row start must be 16-byte aligned.
 *   - Row strides: the batch and head strides (and rfa_sum_slots' slot stride) are free — tensors may lie any 64-bit
 *     distance apart — but the kernels address the rows of one tile with 32-bit byte offsets, so for every rfa_strides of
 *     every entry point, with `elt` the size of the tensor's elements (2, or 4 for an fp32 accumulator),
 *         256 * |row| * elt + D * elt <= 2^31 - 1        (io dtype, D = 128: |row| <= 4194303, so 4194296 elements)
 *     or the call returns RFA_ERR_ARGS before anything is launched (256: the most rows one tile spans).
 *   - Extents: B above 65535 where a launch needs it as a grid dimension (rfa_bwd_preprocess*, rfa_merge, rfa_sum_slots; with H
 *     alike: rfa_lse_flatten / rfa_lse_unflatten, rfa_sink_*, rfa_merge_pair*; rfa_fwd* with a split-KV share count asked for by
 *     name; rfa_bwd* when the call needs a workspace or carries row ranges) and more than 2^31 - 1 workgroups in a 1-D launch
 *     (rfa_fwd*: ceil(Sq / 128) * H * B * shares; rfa_bwd*: that without shares, ceil(Sk / 128) * Hk * B * dkdv_nsplit and,
 *     when the call needs a workspace, ceil(Sk * Hk / 16); the side kernels: ceil(S * H / 16)) return RFA_ERR_SHAPE before
 *     anything is launched.
 *   - Dense mode (cu_seqlens_* == NULL):  q is (B, Sq, H, D), k/v are (B, Sk, Hk, D), lse is
 *     (B, H, Sq).  Varlen mode: q is (Tq, H, D), k/v (Tk, Hk, D), lse is (H, Tq); `B` is the
 *     number of packed sequences, `Sq`/`Sk` the max sequence lengths, *_batch strides unused.
 *   - Causal masks are bottom-right aligned: key j is visible to query i iff
 *     j <= i + (len_k - len_q)  (flash_attn >= 2.1 semantics); `mask_shift` (ABI 7) moves the diagonal for a block
 *     of a longer sequence.
 *   - Rows with no visible key produce out = 0 and lse = +inf (flash_attn semantics); in
 *     accumulate mode such rows leave the accumulators untouched.
 *   - `q_half` / `k_half` select, per packed (or dense) sequence, the whole sequence (0), its
 *     front half (1) or its back half (2) WITHOUT gathering — the offset arithmetic that
 *     replaces get_half_index/get_half_lse (zigzag_ring_flash_attn_varlen.py:24-71).  Outputs
 *     (out, lse, dq, delta) are addressed like q; dk/dv like k.
 *   - ALiBi (flash_attn's alibi_slopes) is an EXTENSION argument (rfa_ext_args, below): per batch b, query head h, query row i
 *     and key j of a block call
 *         score = softmax_scale * q.k  -  slope[b,h] * | i + (len_k - len_q) + alibi_shift - j |
 *     added before masking and softmax (len_*: the effective lengths after q_half / k_half, per sequence for packed
 *     input).  lse is the log-sum-exp of the biased scores, the whole bias included, so blocks of a ring merge; the
 *     backward recomputes P with the same bias, the slopes get no gradient.
 *   - Return value: 0 on success, negative rfa_status otherwise; rfa_strerror() explains.
 */
#ifndef RFA_H_
#define RFA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RFA_ABI_VERSION 8

typedef enum {
  RFA_OK = 0,
  RFA_ERR_NULL = -1,        /* required pointer is NULL                       */
  RFA_ERR_DTYPE = -2,       /* dtype not RFA_BF16 / RFA_F16                    */
  RFA_ERR_HEAD_DIM = -3,    /* head_dim not a multiple of 8 or > 256           */
  RFA_ERR_HEADS = -4,       /* H not a multiple of Hk                          */
  RFA_ERR_SHAPE = -5,       /* negative / zero extents                         */
  RFA_ERR_ALIGN = -6,       /* pointer or stride breaks the 16-byte contract   */
  RFA_ERR_LAUNCH = -7,      /* hipLaunchKernel reported an error               */
  RFA_ERR_ARGS = -8,        /* inconsistent flag / pointer combination         */
  RFA_ERR_ATTR = -9         /* per-device dynamic-LDS opt-in of a kernel failed */
} rfa_status;

typedef enum { RFA_BF16 = 0, RFA_F16 = 1 } rfa_dtype;

enum { RFA_HALF_FULL = 0, RFA_HALF_FRONT = 1, RFA_HALF_BACK = 2 };

/* (batch, row, head) element strides of a (B, S, H, D) / (T, H, D) tensor */
typedef struct {
  int64_t batch;
  int64_t row;
  int64_t head;
} rfa_strides;

typedef struct {
  /* inputs */
  const void *q, *k, *v;
  rfa_strides q_st, k_st, v_st;
  /* plain outputs (io dtype out, fp32 lse).  Used when out_acc == NULL. */
  void *out;
  rfa_strides out_st;
  float *lse;              /* (B,H,Sq) or (H,Tq) */
  int64_t lse_batch, lse_head; /* element strides; row stride is 1 */
  /* fused online-merge accumulators (fp32).  When non-NULL the kernel merges its block
   * result into them instead of writing out/lse:  out_acc has out's logical shape,
   * lse_acc has lse's.  acc_init != 0: first block of a ring — overwrite, do not read. */
  float *out_acc;
  rfa_strides out_acc_st;
  float *lse_acc;
  int64_t lse_acc_batch, lse_acc_head;
  int32_t acc_init;
  /* varlen */
  const int32_t *cu_seqlens_q, *cu_seqlens_k; /* (B+1,) int32 device, or NULL */
  int32_t q_half, k_half;
  /* shape */
  int32_t B, H, Hk, D, Sq, Sk;
  float softmax_scale;
  int32_t causal;
  int32_t dtype; /* rfa_dtype */
  /* Local (sliding window) attention, flash_attn semantics (window_size_left / window_size_right of
   * _flash_attn_forward, forwarded by /root/reference/ring_flash_attn/llama3_flash_attn_varlen.py:147 and
   * adapters/hf_adapter.py:121-128): query i sees keys j with
   *     i + (len_k - len_q) - window_left <= j <= i + (len_k - len_q) + window_right ;
   * a negative value leaves that side unbounded; `causal` forces window_right = 0.  Only honoured when
   * `window` is non-zero, so that a zero-initialised struct means "no window". */
  int32_t window, window_left, window_right;
  /* Dropout (flash_attn's dropout_p; the reference forwards it on the llama3 path,
   * /root/reference/ring_flash_attn/llama3_flash_attn_varlen.py:131,135,266).  dropout_p = 0: off.  An attention
   * probability is kept with probability keep/256, keep = round((1 - dropout_p) * 256), and kept ones are scaled by
   * 256 / keep, keep = round((1 - dropout_p) * 256) — the reciprocal of the probability the mask really keeps with, so that
   * E[dropout(P)] = P for every p —; lse is that of the undropped softmax (flash_attn semantics).  DEVIATION from
   * flash_attn, deliberate: flash_attn also quantises its threshold to 8 bits but keeps scaling by 1 / (1 - dropout_p),
   * which is biased by up to 0.4 % (p = 0.17: 256 / 212 = 1.2075 here, 1 / 0.83 = 1.2048 there); its Philox mask cannot
   * be reproduced without the package anyway, so no bit-level parity is lost (tests/test_oracle.py pins the factor
   * and the unbiasedness against values written out by hand, not against the oracle).  The keep mask is a pure
   * function of (dropout_seed, batch, head_offset + head, q_pos_offset + query position, k_pos_offset + key
   * position) — csrc/rfa_common.hpp: drop_word — where a position is the row inside the dense sequence, or the
   * absolute row of the packed tensor for cu_seqlens input; a rank that holds rows [a, b) of a longer stream passes
   * a / the first gathered key row as offsets and gets the same bits as an unsharded call.  The backward must be
   * given the forward's values.  Not available together with a window (RFA_ERR_ARGS). */
  float dropout_p;
  uint64_t dropout_seed;
  int64_t q_pos_offset, k_pos_offset;
  /* ABI 8, revision 1 — position map of the dropout mask, for local tensors whose rows are not ONE contiguous run of the
   * global sequence (a zigzag rank holds two distant chunks, a stripe rank every W-th token).  Local row i of q (of k)
   * sits at global position
   *     pos(i) = (split == 0 || i < split) ? offset + i * stride : offset2 + (i - split) * stride      (mod 2^32)
   * stride 0 reads as 1, split 0 as "one piece": a zero-initialised map is the plain offset of before, through the same
   * code path, bit for bit.  Read only when dropout_p > 0; positions feed the mask hash ONLY — causal and window masks keep
   * working on local rows.  RFA_ERR_ARGS: a non-default map (stride > 1 or split != 0) with cu_seqlens input or with
   * q_half / k_half != RFA_HALF_FULL, a negative stride, a split outside [1, S - 1]. */
  int32_t q_pos_stride, k_pos_stride;
  int32_t q_pos_split, k_pos_split;
  int64_t q_pos_offset2, k_pos_offset2;
  int32_t head_offset;
  /* Kernel form (tuning / tests; 0 = chosen by the library): RFA_FWD_8x32 = 8 waves x 32 query rows, two waves per SIMD
   * (csrc/rfa_fwd.hip: every head dim, windows, dropout; 256 query rows per workgroup — RFA_FWD_AUTO also launches the
   * same kernel with 4 waves / 128 rows on grids that would under-fill the chip, RFA_FWD_4x32 asks for that form wherever
   * it exists: head dim 128 / 64, no window, no dropout).  Value 2 named a 4-wave x 64-row, one-wave-per-SIMD experiment
   * that lost to the 8 x 32 form by 7 - 13 % in two rounds and was removed in round 6: RFA_ERR_ARGS.
   * RFA_FWD_P8x32 (ABI 6): the PERSISTENT 256-row form — one workgroup per CU walks its share of the (batch, head, query
   * block) items, the next item's first K/V tile and Q fragments fetched under the current item's last tile and epilogue.
   * Head dim 128, dense input (no cu_seqlens) with Sk >= Sq, plain outputs (no out_acc), no window, no dropout, no split-KV
   * shares; where a call is not eligible the field reads as RFA_FWD_AUTO.  RFA_FWD_AUTO takes it for launches of at least
   * two items per CU.  Bit-identical to the 8 x 32 form. */
  int32_t fwd_form;
  /* ABI 5 — split-KV launches.  A call with few query rows and many keys (a llama3 head group at 2048 tokens per rank
   * against the gathered keys of 8 ranks: 256 key tiles per workgroup, half the CUs without one) is launched with the
   * key tiles of every workgroup divided between kv_nsplit workgroups; each writes a normalised partial (out, lse) to
   * `workspace` and a second, streaming kernel combines the partials into the call's outputs (plain or accumulate mode
   * alike).  workspace: rfa_fwd_workspace_bytes() bytes, or NULL (= never split).  kv_nsplit: 0 = chosen from the
   * shapes, 1 = off, 2..8 forced (tests).  total_q: varlen only, number of packed q rows addressed (sizes the
   * workspace).  Eligible: head dim 128 or 64 exactly, no window, no dropout. */
  void *workspace;
  int32_t kv_nsplit;
  int64_t total_q;
  /* ABI 7 — where this block sits in a longer sequence.  The band of the call (the plain causal bound included) becomes
   *     i + (len_k - len_q) + mask_shift - window_left <= j <= i + (len_k - len_q) + mask_shift + window_right ,
   * mask_shift = (global position of q row 0 + len_q) - (global position of k row 0 + len_k); for blocks of equal length
   * simply q_start - k_start.  A rank of a ring that holds rows [rS, (r+1)S) and has the K/V of rank r - d on hand passes
   * d * S and gets its share of ONE sliding-window attention over the whole sequence.  0 (a zero-initialised struct): the
   * block's own diagonal, as before.  Ignored without `causal` and without `window`.  Dense input without dropout only
   * (cu_seqlens != NULL or dropout_p > 0 with a non-zero shift: RFA_ERR_ARGS; packed input takes mask_shift_lens, below).  Any 64-bit value is accepted: the library
   * normalises the band before it plans or launches — a bound no element of the block can reach is
   * dropped, so a block wholly inside the window IS the unwindowed non-causal call (same instance, plan and dS-spill
   * form, bit for bit); a block with no visible element launches nothing in accumulate mode and writes out = 0,
   * lse = +inf / zero gradients in plain mode; what is left is re-expressed in numbers that fit the kernels' 32 bits.
   * The persistent forward, the balanced dK/dV schedule and split-KV plans keyed on the block's own diagonal decline a
   * shifted causal band; the triangular ds_scratch layout follows it. */
  int64_t mask_shift;
  /* ABI 8 — the same, in units of each sequence's own key length, so that it also serves packed (cu_seqlens) input, whose
   * lengths live on the device.  For sequence b of the call the band becomes
   *     i + off_b - window_left <= j <= i + off_b + window_right ,
   *     off_b = (len_k(b) - len_q(b)) + mask_shift + mask_shift_lens * len_k(b)
   * (len_*: the effective lengths after q_half / k_half).  A rank that holds the l_b local rows of every packed sequence and
   * has the K/V of the rank t places in front on hand passes t: every sequence is banded as its part of one window over
   * its full length.  In one packed launch some sequences may then be wholly dark, some wholly lit and some cut; a dark
   * sequence leaves accumulators untouched, writes out = 0 / lse = +inf in plain mode (out 0 / lse -inf with acc_init) and
   * exact-zero gradients in the plain and overwrite modes — the contracts of a dense shifted block.  0 (a zero-initialised
   * struct): as before.  Ignored without `causal` and without `window`.
   *   packed input: accepted with causal and / or window; the absolute mask_shift stays RFA_ERR_ARGS there (it has no
   *     meaning per sequence).  The band is not normalised on the host.  A bounded window runs the windowed instances; a
   *     causal call without a window keeps the default ones, the packed-row dS hand-off and the 256-key dK/dV form.
   *   dense input: mask_shift_lens * len_k is folded into mask_shift before the band is normalised — the call IS the call
   *     with mask_shift = n * len_k, bit for bit (same normalisation, plan and instance).
   *   dropout_p > 0 with a non-zero value, or |mask_shift_lens| * Sk >= 2^30 (the kernels keep off, off - window_left and
   *     off + window_right in 32 bits): RFA_ERR_ARGS.
   * The plans that decline a non-zero mask_shift decline this field too; estimates and memo keys take
   * mask_shift_lens * Sk as the stand-in shift of packed input. */
  int32_t mask_shift_lens;
} rfa_fwd_args;

enum { RFA_FWD_AUTO = 0, RFA_FWD_8x32 = 1, RFA_FWD_RETIRED_2 = 2, RFA_FWD_4x32 = 3, RFA_FWD_P8x32 = 4 };

typedef struct {
  const void *dout, *out; /* (B,Sq,H,D) io dtype */
  rfa_strides dout_st, out_st;
  float *delta;           /* same layout contract as lse */
  int64_t delta_batch, delta_head;
  const int32_t *cu_seqlens_q;
  int32_t q_half;
  int32_t B, H, D, Sq;
  int32_t dtype;
} rfa_bwd_preprocess_args;

typedef struct {
  const void *dout, *q, *k, *v;
  rfa_strides dout_st, q_st, k_st, v_st;
  const float *lse;   /* GLOBAL log-sum-exp of the rows (natural log)            */
  int64_t lse_batch, lse_head;
  const float *delta; /* rowsum(dout*out), from rfa_bwd_preprocess              */
  int64_t delta_batch, delta_head;
  /* plain outputs in io dtype (used when the matching *_acc pointer is NULL) */
  void *dq, *dk, *dv;
  rfa_strides dq_st, dk_st, dv_st;
  /* fp32 accumulators: dq_acc += dq ; dk_acc += dk ; dv_acc += dv  (acc_init: overwrite) */
  float *dq_acc, *dk_acc, *dv_acc;
  rfa_strides dq_acc_st, dk_acc_st, dv_acc_st;
  int32_t acc_init;
  /* workspace for dK/dV partials (already summed over the query heads of a K/V group),
   * rfa_bwd_workspace_bytes() bytes.  Unsplit launches: 2 * total_k*Hk*D elements of the io dtype (one
   * rounding per block, the rounding point of flash_attn's block gradients).  Launches whose key blocks
   * share their query range between `nsplit` workgroups (256-key kernel form, see dkdv_form): nsplit fp32
   * partials per element, summed and rounded ONCE by the reduction pass.
   * ALWAYS size it with rfa_bwd_workspace_bytes(); may be NULL whenever that returns 0 (single-phase
   * calls that write dk/dv or overwrite dk_acc/dv_acc on launches that need no such split). */
  void *workspace;
  const int32_t *cu_seqlens_q, *cu_seqlens_k;
  int32_t q_half, k_half;
  int32_t B, H, Hk, D, Sq, Sk;
  int64_t total_k;    /* varlen: number of packed k rows addressed (Tk); dense: B*Sk */
  float softmax_scale;
  int32_t causal;
  int32_t deterministic; /* accepted; this implementation is always deterministic */
  int32_t dtype;
  /* 0 = everything.  RFA_BWD_COMPUTE: dQ + dK/dV partials into `workspace` only;
   * RFA_BWD_REDUCE: add / copy the partials of a previous COMPUTE call into dk_acc/dv_acc or
   * dk/dv.  Splitting lets a ring step overlap the compute with the arrival of the
   * dk/dv accumulators it will add into (zigzag_ring_flash_attn.py:172-187).  With phases != 0
   * the workspace is always required. */
  int32_t phases;
  /* Optional dS spill scratch (io dtype, rfa_bwd_ds_scratch_bytes() bytes; NULL = not used).  When given and
   * rfa_bwd_ds_scratch_bytes() is non-zero for the call, the backward runs 5 GEMMs instead of 7: the dK/dV
   * kernel stores dS = P*(dP - delta) of every (32 query x 32 key) block it visits and dQ is computed by a
   * streaming GEMM over those blocks instead of recomputing S and dP (csrc/rfa_dqs.hip).  The contents are
   * only meaningful between the two kernels of one call (or between a RFA_BWD_SKIP_DQ call and the matching
   * RFA_BWD_SKIP_DKDV call).  Eligible: D == 128 (or 256), no bounded left window — dense or packed
   * (cu_seqlens: the scratch is then laid out with the extents of the longest sequence, Sq / Sk = max_seqlen). */
  void *ds_scratch;
  int32_t window, window_left, window_right; /* as in rfa_fwd_args (a bounded window_left is not eligible for ds_scratch) */
  /* dK/dV launch plan (ABI 4: part of the call instead of process environment, so that the COMPUTE and the
   * REDUCE phase of one backward — and rfa_bwd_workspace_bytes() — can never disagree).
   *   dkdv_form   RFA_DKDV_AUTO: chosen from the shapes; RFA_DKDV_128: a workgroup owns 128 keys;
   *               RFA_DKDV_256: 256 keys (head dim 128 without a window only, otherwise ignored)
   *               RFA_DKDV_BAL (ABI 6): 256 keys in the balanced causal schedule — every workgroup of a dense causal
   *               self-attention block (Sq == Sk, a multiple of 512 rows, head dim 128 or 64, single-phase call that writes
   *               dk / dv or overwrites dk_acc / dv_acc) does the same amount of work, key blocks of the lower half are
   *               shared by two workgroups that add their partials between themselves: no reduction pass.  Where the
   *               call is not eligible the field is read as RFA_DKDV_AUTO.  RFA_DKDV_256 with dkdv_nsplit > 0 names the
   *               shared-range plan instead.
   *   dkdv_nsplit 0: chosen from the shapes; 1..8: workgroups sharing the query range of a key block
   *               (256-key form only)
   * A zero-initialised struct means "auto".  rfa_bwd_plan() reports what a call will run. */
  int32_t dkdv_form, dkdv_nsplit;
  /* Measurement aid (NULL = off): 4 caller-owned hipEvent_t handles, recorded on `stream` before the first
   * launch of the call and after its first kernel, its second kernel and the reduction pass (launches a call
   * does not make record their event right behind the previous one).  Kernel order: dK/dV then dQ when the call
   * runs the dS-spill form (rfa_bwd_plan: five_gemm), dQ then dK/dV otherwise.  This is how bench.py times the
   * kernels INSIDE the real step instead of in isolation. */
  void **prof_events;
  /* dropout: as in rfa_fwd_args, with the forward's values (a call with dropout runs the 7-GEMM form) */
  float dropout_p;
  uint64_t dropout_seed;
  int64_t q_pos_offset, k_pos_offset;
  /* position map of the dropout mask: as in rfa_fwd_args, with the forward's values */
  int32_t q_pos_stride, k_pos_stride;
  int32_t q_pos_split, k_pos_split;
  int64_t q_pos_offset2, k_pos_offset2;
  int32_t head_offset;
  /* ABI 5: size of the buffer `ds_scratch` points to.  0 = at least rfa_bwd_ds_scratch_bytes().  A SMALLER buffer does
   * not switch the 5-GEMM form off: the call then runs it in HEAD-GROUP CHUNKS that reuse the one buffer — chunks of
   * whole K/V heads (with their query heads) or, where even one K/V head's query heads do not fit, fractions of ONE
   * K/V head's query heads, whose dK/dV shares are accumulated in the fp32 partials — each chunk one dK/dV launch and
   * one dQ launch, in stream order.  Peak scratch is then independent of the head count and the long-context cases
   * (S = 32768, 32 heads: 34 GB of dS) keep the 5-GEMM form (rfa_bwd_ds_chunks() reports the chunking; head dim 128
   * only; a buffer below one query head's share, rfa_bwd_ds_scratch_min_bytes(), falls back to the 7-GEMM form). */
  int64_t ds_scratch_bytes;
  /* ABI 5, varlen: number of packed q rows addressed (Tq); 0 = total_k.  Sizes the packed layout of ds_scratch:
   * H * (total_q / 32 + B) * ceil(max_seqlen_k / 32) blocks of 2 KiB — bounded by the packed row count, not by
   * B x the longest sequence. */
  int64_t total_q;
  /* ABI 7: as in rfa_fwd_args, with the forward's value */
  int64_t mask_shift;
  /* ABI 8: as in rfa_fwd_args, with the forward's value */
  int32_t mask_shift_lens;
} rfa_bwd_args;

enum { RFA_DKDV_AUTO = 0, RFA_DKDV_128 = 1, RFA_DKDV_256 = 2, RFA_DKDV_BAL = 3 };

enum {
  RFA_BWD_ALL = 0,
  RFA_BWD_COMPUTE = 1,
  RFA_BWD_REDUCE = 2,
  /* measurement aids, valid together with RFA_BWD_COMPUTE: launch only one of the two kernels */
  RFA_BWD_SKIP_DKDV = 4,
  RFA_BWD_SKIP_DQ = 8,
  /* dk_acc / dv_acc are OVERWRITTEN with this block's dK/dV (fp32) while dq_acc still follows
   * acc_init — for schedules in which every dK/dV accumulator slot receives exactly one block
   * (all-gather / reduce-scatter exchange).  In a single-phase call the dK/dV kernel then stores
   * fp32 straight into dk_acc / dv_acc: no workspace, no reduction pass (unless the launch is split,
   * see `workspace`). */
  RFA_BWD_KV_OVERWRITE = 16
};

typedef struct {
  float *out_acc;          /* (B,S,H,D) fp32, updated in place */
  rfa_strides out_acc_st;
  float *lse_acc;          /* (B,H,S) fp32, updated in place   */
  int64_t lse_acc_batch, lse_acc_head;
  const void *block_out;   /* io dtype */
  rfa_strides block_out_st;
  const float *block_lse;  /* (B,H,S) */
  int64_t block_lse_batch, block_lse_head;
  int32_t B, H, D, S;      /* S rows are merged (pass slice pointers for a row range) */
  int32_t acc_init;
  int32_t dtype;
  /* element stride between consecutive rows of lse_acc / block_lse; 0 means 1.  The
   * reference keeps its running lse as (B,S,H,1) (utils.py:41,64): batch=S*H, head=1, row=H. */
  int64_t lse_acc_row, block_lse_row;
} rfa_merge_args;

int rfa_abi_version(void);
/* Revision of the structs WITHIN one RFA_ABI_VERSION (fields added in the middle of a struct leave the version number
 * alone): 1 = the dropout position map.  A binding must find this symbol and this value, or refuse the library. */
#define RFA_ABI_REVISION 1
int rfa_abi_revision(void);
/* identity of this build: the first 16 hex digits of the sha256 over the library's sources, compiled into the binary by
 * the build recipe (ring-flash-attention_amd/build.py).  Measurement files (profiles/r*_traffic.json) record the id of
 * the library they were collected on; bench.py only quotes them for a library with the same id. */
const char *rfa_build_id(void);
const char *rfa_strerror(int status);

int rfa_fwd(const rfa_fwd_args *args, void *stream);

/* Extension arguments: per-call features that arrive after the structs above were frozen (ABI 8 revision 1 stays — no
 * existing struct changes) ride on this struct and the two *_ex entry points instead of new fields there.
 *   rfa_fwd(a, s) IS rfa_fwd_ex(a, NULL, s), rfa_bwd likewise; a NULL `ext`, or one whose features are all off, runs the
 *   instance, plan and bits of the plain call.
 *   struct_bytes: sizeof(rfa_ext_args) as the CALLER compiled it.  Smaller than the library's: the missing tail reads as
 *   zero.  Larger: accepted while the tail the library does not know is zero.  RFA_ERR_ARGS: a larger struct with a
 *   non-zero tail, struct_bytes below the fixed head (struct_bytes + reserved), a non-zero `reserved`.  The extension is
 *   validated before any pointer of the base struct is looked at; rfa_ext_args_bytes() is the library's sizeof.
 * ALiBi (Conventions, above): alibi_slopes — fp32, DEVICE, one slope per query head (GQA changes nothing): (H,) with
 *   alibi_batch_stride = 0, or (B, H) with the element stride between batch entries (packed input: between sequences); a
 *   head-group slice is a pointer offset made by the caller.  NULL: off (stride and shift are then not read).
 *   alibi_shift: where the block sits in a longer sequence, with mask_shift's meaning for blocks of equal length — global
 *   position of q row 0 minus that of k row 0, in rows — but a field of its own: it is independent of the mask, is read
 *   without a band and is never rewritten by the band normalisation.  A ring rank that has the K/V of the rank t places in
 *   front on hand passes t * S.
 *   The distance is formed in integers per row and only the per-element part in fp32: exact up to 2^24 rows; beyond that
 *   it carries a relative rounding of 6e-8 (the forward and the backward kernels may round it differently there).
 *   The slopes enter the kernels in score units (slope / softmax_scale: their row max runs on unscaled scores).
 *   RFA_ERR_ARGS with a bias: a bounded window that survives the band normalisation; dropout_p > 0; head_dim > 128;
 *   a non-zero alibi_shift with cu_seqlens; |alibi_shift| + Sq + Sk >= 2^31; softmax_scale <= 0; a negative
 *   alibi_batch_stride.  (A block whose band is empty has nothing to bias: it runs as the call without the extension.)
 *   Forward: one kernel form, 8 waves x 32 rows; fwd_form values that do not exist for a bias (RFA_FWD_4x32,
 *   RFA_FWD_P8x32) and split-KV read as RFA_FWD_AUTO / never split, as for dropout; `workspace` is ignored.
 *   Backward: the plain 128-key dK/dV kernel and the 7-GEMM dQ kernel, as for dropout.  rfa_bwd_workspace_bytes and
 *   rfa_bwd_plan do not see the extension, so rfa_bwd_ex returns RFA_ERR_ARGS unless the BASE arguments already plan to
 *   exactly that — dkdv_form = RFA_DKDV_128, ds_scratch = NULL — and the three can never disagree.
 * Logit soft-capping (flash_attn's softcap): with softcap > 0 every score becomes
 *         s' = softcap * tanh(softmax_scale * q.k / softcap)
 *   before masking and softmax; the mask (causal, window, mask_shift, mask_shift_lens, halves) is applied to s'.  lse is
 *   the log-sum-exp of s', so blocks of a ring merge as before.  Backward, with t = tanh(...) recomputed by the forward's
 *   expression: P = exp(s' - lse), dS = P (dP - delta) (1 - t^2), dQ = softmax_scale dS K, dK = softmax_scale dS^T Q; dV and
 *   delta are unchanged.  softcap == 0: off — the instance, plan and bits of the plain call; a caller's struct that ends
 *   in front of the field reads it as 0 (struct_bytes).  softcap_pad: explicit padding, must be 0.
 *   tanh(x) = 1 - 2 / (1 + exp2(2 log2(e) x)) on the hardware exp2 and reciprocal, ONE expression for the three kernels:
 *   no branch, finite at +-inf, absolute error a few 2^-23 — times softcap about 3e-6 in a capped score at softcap = 50.
 *   RFA_ERR_ARGS, before any base pointer is looked at: a negative, NaN or infinite softcap; a non-zero softcap_pad;
 *   softcap > 0 together with dropout_p > 0, a non-NULL alibi_slopes, head_dim > 128 or softmax_scale <= 0; softcap > 0
 *   with a bounded window that survives the band normalisation at head dims 65 .. 127 (the zero-padded 128-wide windowed
 *   dK/dV instance with a cap does not fit the register file: not built; refused by rfa_fwd_ex and rfa_bwd_ex alike).
 *   Everything else combines with a cap: bounded windows, mask_shift, mask_shift_lens, q_half / k_half, cu_seqlens,
 *   accumulate mode, two-phase backwards, RFA_BWD_KV_OVERWRITE.  (A block whose band is empty runs as the call without the
 *   extension.)  Forward: the 8 waves x 32 rows form; RFA_FWD_4x32, RFA_FWD_P8x32 and split-KV read as RFA_FWD_AUTO / never
 *   split, as for the bias; `workspace` is ignored.  Backward: the 128-key dK/dV kernel and the 7-GEMM dQ kernel;
 *   rfa_bwd_ex returns RFA_ERR_ARGS unless the base arguments name dkdv_form = RFA_DKDV_128 and ds_scratch = NULL — the
 *   same rule and reason as for the bias. */
typedef struct {
  uint32_t struct_bytes;        /* sizeof as the caller compiled it */
  uint32_t reserved;            /* 0 */
  const float *alibi_slopes;    /* NULL: off */
  int64_t alibi_batch_stride;   /* 0: one (H,) row for every batch entry */
  int64_t alibi_shift;
  float softcap;                /* 0: off */
  uint32_t softcap_pad;         /* 0 */
} rfa_ext_args;
int rfa_fwd_ex(const rfa_fwd_args *args, const rfa_ext_args *ext, void *stream);
int64_t rfa_ext_args_bytes(void);
/* bytes of rfa_fwd_args.workspace the call can use (0: the call is never split); *nsplit (may be NULL) = the number of
 * key-range shares the call runs with when given that workspace.  Pure function of the arguments. */
int64_t rfa_fwd_workspace_bytes(const rfa_fwd_args *args, int32_t *nsplit);
int rfa_bwd_preprocess(const rfa_bwd_preprocess_args *args, void *stream);
int64_t rfa_bwd_workspace_bytes(const rfa_bwd_args *args);
/* the launch plan of a call: *form = RFA_DKDV_128 / RFA_DKDV_256 / RFA_DKDV_BAL, *nsplit >= 1, *five_gemm = 1 when the call
 * (with its ds_scratch) runs the dS-spill form.  Pure function of the arguments. */
int rfa_bwd_plan(const rfa_bwd_args *args, int32_t *form, int32_t *nsplit, int32_t *five_gemm);
/* bytes of ds_scratch the whole hand-off of the call uses — dense: B*H*ceil(Sq/32)*ceil(Sk/32)*2048 (dense causal: the
 * visited triangle only); packed input: H*(total_q/32 + B)*ceil(max_seqlen_k/32)*2048; with q_half / k_half: ceil(S/2)
 * instead of S — or 0 if it is not eligible */
int64_t rfa_bwd_ds_scratch_bytes(const rfa_bwd_args *args);
/* the smallest ds_scratch with which the call still runs the 5-GEMM form (one query head's dS; 0: not eligible) */
int64_t rfa_bwd_ds_scratch_min_bytes(const rfa_bwd_args *args);
/* the chunking of the call's dS hand-off for its (ds_scratch, ds_scratch_bytes): *nchunks = launches pairs (0: the
 * call runs the 7-GEMM form, 1: one pair over all heads), *kv_heads / *q_heads = K/V heads and query heads PER K/V HEAD
 * of one chunk, *chunk_bytes = scratch bytes one chunk uses.  Pure function of the arguments. */
int rfa_bwd_ds_chunks(const rfa_bwd_args *args, int32_t *nchunks, int32_t *kv_heads, int32_t *q_heads, int64_t *chunk_bytes);
int rfa_bwd(const rfa_bwd_args *args, void *stream);
int rfa_bwd_ex(const rfa_bwd_args *args, const rfa_ext_args *ext, void *stream);
int rfa_merge(const rfa_merge_args *args, void *stream);

/* dst(io dtype) = (io)src(fp32), n elements, both contiguous */
int rfa_cast(void *dst, const float *src, int64_t n, int32_t dtype, void *stream);

/* dst[b, row, h, :] = sum over s < nslots of src[s][b, row, h, :]: io dtype in, summed in fp32, io dtype out.
 * The owner-side sum of the per-rank dK/dV contributions of the all-to-all exchange form — the reference's
 * `dk = dk_comm_buffer + block_dk` accumulation (zigzag_ring_flash_attn.py:164-187) after the blocks have
 * travelled in the io dtype instead of fp32 accumulators — written straight into the (possibly strided:
 * a slice of a packed kv gradient) destination, instead of a sum + cast + copy triple. */
typedef struct {
  const void *src;         /* slot 0; slot s starts slot_stride elements further */
  int64_t slot_stride;
  int32_t nslots;
  void *dst;
  rfa_strides src_st, dst_st;   /* element strides (batch, row, head) inside one slot / of dst; D contiguous */
  int32_t B, S, H, D;
  int32_t dtype;
} rfa_sum_slots_args;
int rfa_sum_slots(const rfa_sum_slots_args *args, void *stream);

/* LSE re-layout, fp32 (triton_utils.py:39-67,103-137).  The padded tensor is a contiguous
 * (B, H, max_seqlen); the packed tensor has element (h, t) at h*head_stride + t*row_stride, so
 * it covers both the (H, T) result of flatten and the (T, H, 1) input of unflatten.
 * Padding positions of the unflatten destination are left untouched (as the reference does). */
int rfa_lse_flatten(float *dst_packed, const float *src_padded, const int32_t *cu_seqlens,
                    int32_t B, int32_t H, int32_t max_seqlen, int64_t dst_head_stride,
                    int64_t dst_row_stride, void *stream);
int rfa_lse_unflatten(float *dst_padded, const float *src_packed, const int32_t *cu_seqlens,
                      int32_t B, int32_t H, int32_t max_seqlen, int64_t src_head_stride,
                      int64_t src_row_stride, void *stream);

/* Attention sinks (GPT-OSS, the streaming-LLM family; flash_attn's / Hugging Face's `s_aux`): one logit per query head that
 * joins the softmax as an extra column whose value vector is zero,
 *     p_ij = exp(s_ij - lse'_i),   lse'_i = log(sum_j exp(s_ij) + exp(sink_h)),   out'_i = sum_j p_ij v_j .
 * No attention kernel knows about it, and no existing struct changes (ABI 8 revision 1 stays; rfa_ext_args stays): the sink is
 * applied ONCE, to the (out, lse) of the attention without it, merged over all blocks and ranks —
 *     rfa_sink_apply:  lse' = logaddexp(lse, sink_h),  out' = out * exp(lse - lse')    (io dtype out, rounded once more)
 * and rfa_bwd_preprocess / rfa_bwd handed (out', lse') in place of (out, lse) return the exact dq / dk / dv: the sink
 * column's dP is 0, so delta' = rowsum(dO * out'), P' = exp(s - lse'), dS = P' (dP - delta') is the existing formula.
 *     rfa_sink_grad:   dsink_h = - sum over the B x S rows i of exp(sink_h - lse'_i) * rowsum(dO_i * out'_i)
 * in fp32, summed in a fixed order (no atomics): a pure function of its inputs, the same bits on every run.
 * Layout: B x S rows of H heads — dense out (B, S, H, D) with lse (B, H, S); packed out (T, H, D) with lse (H, T) is
 * B = 1, S = T (batch strides unused); no cu_seqlens, the operation is per row.  lse row stride is 1.  sinks, dsink: (H,)
 * fp32, contiguous.  out_dst may be out_src and lse_dst may be lse_src (then with the same strides).
 * Rows without a visible key (lse = +inf; -inf is read the same way) get lse' = sink_h and out' = 0.  A sink so low that
 * exp(sink_h - lse) underflows returns the input bits: out' == out, lse' == lse.
 * Checks, in this order and before any launch: NULL struct RFA_ERR_NULL; dtype, head_dim (a multiple of 8, <= 256), H <= 0,
 * B < 0 as everywhere; S < 0, B or H above 65535, S * H above 16 * (2^31 - 1) RFA_ERR_SHAPE; B == 0 or S == 0: RFA_OK, nothing is launched
 * (rfa_sink_grad then needs dsink alone and sets it to zero); NULL tensors RFA_ERR_NULL; pointers or strides off the 16-byte
 * contract RFA_ERR_ALIGN; rfa_sink_grad: workspace_bytes below rfa_sink_grad_workspace_bytes() RFA_ERR_ARGS. */
typedef struct {
  const void *out_src;     /* io dtype */
  rfa_strides out_src_st;
  void *out_dst;
  rfa_strides out_dst_st;
  const float *lse_src;
  int64_t lse_src_batch, lse_src_head; /* element strides; row stride is 1 */
  float *lse_dst;
  int64_t lse_dst_batch, lse_dst_head;
  const float *sinks;      /* (H,) fp32 */
  int32_t B, S, H, D;
  int32_t dtype;           /* rfa_dtype */
  int32_t reserved;        /* 0 */
} rfa_sink_apply_args;
int rfa_sink_apply(const rfa_sink_apply_args *args, void *stream);

typedef struct {
  const void *dout;        /* io dtype; any (batch, row, head) strides that keep rows 16-byte aligned */
  rfa_strides dout_st;
  const void *out;         /* out' as rfa_sink_apply wrote it */
  rfa_strides out_st;
  const float *lse;        /* lse' */
  int64_t lse_batch, lse_head;
  const float *sinks;      /* (H,) fp32 */
  float *dsink;            /* (H,) fp32, overwritten */
  void *workspace;         /* rfa_sink_grad_workspace_bytes() bytes, 16-byte aligned; contents do not matter */
  int64_t workspace_bytes;
  int32_t B, S, H, D;
  int32_t dtype;
  int32_t reserved;        /* 0 */
} rfa_sink_grad_args;
/* bytes of workspace the call needs: one fp32 partial per (batch entry, chunk of 256 rows, head); 0 for a call without rows
 * and for arguments the call would refuse.  Pure function of B, S and H. */
int64_t rfa_sink_grad_workspace_bytes(const rfa_sink_grad_args *args);
int rfa_sink_grad(const rfa_sink_grad_args *args, void *stream);

/* Sequence/head exchange copies (DeepSpeed-Ulysses in front of a ring: ring_flash_attn.with_ulysses).  Inside a group of U
 * ranks every rank trades heads for rows with ONE all-to-all per direction; this entry point is the layout change on either
 * side of it, for up to three tensors of one call in one launch.  No attention kernel knows about it and no existing struct
 * changes (ABI 8 revision 1 stays).  Three views of a tensor, rank at index p of the group, Hs = H / U:
 *     local    (B, S, P, H, D)        this rank's rows, all heads; P parts (1: q, k, v, out; 2: packed kv; 3: qkv)
 *     merged   (B, U*S, P, Hs, D)     the U ranks' rows, head slice p
 *     slots    U x { for each tensor of the call: [B][S][P][Hs][D] }    the all-to-all buffer, contiguous; slot j is what is
 *                                     sent to rank j, or what arrived from rank j
 * local and merged take any (batch, row, part, head) element strides with last stride 1 and 16-byte aligned rows.  Slot j pairs
 * with head slice j of the local view and, row i of it, with row m(j, i) of the merged view:
 *     RFA_SEQHEAD_CONTIGUOUS  m = j S + i                                                     (the ring schedule's rows)
 *     RFA_SEQHEAD_ZIGZAG      m = i < S/2 ? j S/2 + i : U S/2 + (U-1-j) S/2 + (i - S/2)       (S even)
 *     RFA_SEQHEAD_STRIPE      m = i U + j
 * so that the merged tensor is the schedule's own layout at 1/U of the ranks.  Ops (t[k].ptr is the local or the merged view, whichever the op names;
 * the slot buffer is the other side):
 *     RFA_SEQHEAD_PACK             local  -> slots      (before the all-to-all, towards the attention)
 *     RFA_SEQHEAD_UNPACK           slots  -> merged     (after it)
 *     RFA_SEQHEAD_MERGED_TO_SLOTS  merged -> slots      (inverse of UNPACK: out and the gradients on the way back)
 *     RFA_SEQHEAD_SLOTS_TO_HEADS   slots  -> local      (inverse of PACK)
 * Pure data movement: bytes are copied, never converted.  Every element of the destination inside the map is written exactly
 * once, nothing outside it is touched.  t[k].H is the head count of the LOCAL view (the merged one has H / U).
 * Checks, in this order and before any pointer is read: NULL struct RFA_ERR_NULL; struct_bytes != sizeof, reserved != 0, op or
 * layout unknown, ntensors outside 1..3, a P outside 1..3 RFA_ERR_ARGS; elem_bytes != 2 RFA_ERR_DTYPE; D not a multiple of 8 in
 * 8..256 RFA_ERR_HEAD_DIM; U <= 0, B < 0, S < 0, odd S with ZIGZAG, U*S or U*S*B above 2^31 - 1 RFA_ERR_SHAPE; an H <= 0 or not
 * divisible by U, of any tensor, RFA_ERR_HEADS; then a tensor's 16-byte chunk count (U B S P (H/U) D/8, which needs its H) above
 * 2^31 - 1 RFA_ERR_SHAPE; B == 0 or S == 0: RFA_OK, nothing is launched; NULL tensors or
 * slots RFA_ERR_NULL; pointers or strides off the 16-byte contract RFA_ERR_ALIGN; slots_elems below U times the slot size
 * RFA_ERR_ARGS. */
enum { RFA_SEQHEAD_PACK = 0, RFA_SEQHEAD_UNPACK = 1, RFA_SEQHEAD_MERGED_TO_SLOTS = 2, RFA_SEQHEAD_SLOTS_TO_HEADS = 3 };
enum { RFA_SEQHEAD_CONTIGUOUS = 0, RFA_SEQHEAD_ZIGZAG = 1, RFA_SEQHEAD_STRIPE = 2 };
typedef struct {
  void *ptr;               /* local or merged view (by op); read or written (by op) */
  int64_t batch, row, part, head; /* element strides; `part` unused when P == 1 */
  int32_t P;               /* 1, 2 or 3 */
  int32_t H;               /* heads per part of the LOCAL view */
} rfa_seq_head_tensor;
typedef struct {
  uint32_t struct_bytes;   /* sizeof(rfa_seq_head_args) */
  uint32_t reserved;       /* 0 */
  int32_t op, layout;
  int32_t U, B, S, D;      /* S: rows of the LOCAL view */
  int32_t elem_bytes;      /* 2 */
  int32_t ntensors;        /* 1..3 */
  rfa_seq_head_tensor t[3];
  void *slots;             /* 16-byte aligned */
  int64_t slots_elems;     /* its size in elements: at least U * sum_k B S P_k (H_k / U) D */
} rfa_seq_head_args;
int rfa_seq_head_copy(const rfa_seq_head_args *args, void *stream);

/* Rotary position embedding of q and k at GLOBAL positions (ring_flash_attn.apply_rotary; csrc/rfa_rotary.hip).  Up to two
 * tensors of one call — q (B, S, H, D) and k (B, S, Hk, D), or packed (T, H, D) as B = 1, S = T — share rows, positions and
 * tables and go through one launch.  No attention kernel knows about it and no existing struct changes (ABI 8 revision 1 stays).
 * Of every (row, head) the columns [rot_offset, rot_offset + R) are rotated by the angles of the row's position pos:
 *     interleaved == 0 (GPT-NeoX halves)   x1 = column rot_offset + c,     x2 = column rot_offset + c + R/2,   c < R/2
 *     interleaved == 1 (GPT-J)             x1 = column rot_offset + 2 c,   x2 = column rot_offset + 2 c + 1,   c < R/2
 *     o1 = x1 cos[pos, c] - x2 sin[pos, c],    o2 = x2 cos[pos, c] + x1 sin[pos, c]          (conj != 0: sin -> -sin)
 * in fp32, each result rounded once to the io dtype; the bits of an element depend on its values and its position alone.  The
 * other columns pass through: copied when dst != src, never touched when dst == src (in place).  conj is the inverse rotation
 * and, applied to the incoming gradients, the backward.
 *   cos, sin: (P, R/2), contiguous, table_dtype = the io dtype or RFA_ROTARY_TABLE_F32.
 *   positions != NULL: int32, row i of batch entry b sits at pos_offset + positions[b * pos_batch + i] (pos_batch 0: one row of
 *   positions for every batch entry).  NULL: the position map with the meaning of rfa_fwd_args.q_pos_* —
 *       pos(i) = (pos_split == 0 || i < pos_split) ? pos_offset + i * pos_stride : pos_offset2 + (i - pos_split) * pos_stride
 *   (pos_stride 0 reads as 1).  Where the tables are read the position is clamped to [0, P - 1]: no value of `positions` makes
 *   the kernel read outside them; a map that leaves [0, P - 1] is refused on the host.
 *   Each tensor: src read at the src strides, dst written at the dst strides (element strides, last stride 1, rows 16-byte
 *   aligned); dst == src needs equal strides.  Apart from that a dst must not overlap any src.
 * Checks, in this order and before any pointer is read: NULL struct RFA_ERR_NULL; struct_bytes != sizeof, reserved != 0,
 * ntensors outside 1..2, interleaved or conj outside 0..1, a non-zero pad RFA_ERR_ARGS; dtype, or a table_dtype that is neither
 * dtype nor RFA_ROTARY_TABLE_F32, RFA_ERR_DTYPE; D not a multiple of 8 in 8..256, R not a positive multiple of 16 (interleaved:
 * of 8), rot_offset negative or not a multiple of 8, rot_offset + R > D RFA_ERR_HEAD_DIM; B < 0, S < 0, P < 1, B * S above
 * 2^31 - 1 RFA_ERR_SHAPE; an H <= 0, of any tensor, RFA_ERR_HEADS; then a tensor's unit count (one thread each: B S H times
 * R/16 — interleaved R/8 — plus, out of place, (D - R)/8) above 2^31 - 1 RFA_ERR_SHAPE; B == 0 or S == 0: RFA_OK, nothing is
 * launched; NULL src, dst, cos or sin RFA_ERR_NULL; pointers or strides off the 16-byte contract RFA_ERR_ALIGN; dst == src with
 * differing strides, a negative pos_batch, and with the map a negative pos_stride, a pos_split outside 0..S-1 or a position
 * outside [0, P - 1] RFA_ERR_ARGS. */
#define RFA_ROTARY_TABLE_F32 2
typedef struct {
  const void *src;
  void *dst;               /* == src: in place */
  int64_t src_batch, src_row, src_head; /* element strides */
  int64_t dst_batch, dst_row, dst_head;
  int32_t H;
  int32_t pad;             /* 0 */
} rfa_rotary_tensor;
typedef struct {
  uint32_t struct_bytes;   /* sizeof(rfa_rotary_args) */
  uint32_t reserved;       /* 0 */
  int32_t ntensors;        /* 1..2 */
  int32_t B, S, D;         /* packed input: B = 1, S = T */
  int32_t dtype;           /* rfa_dtype */
  int32_t R, rot_offset;
  int32_t interleaved, conj;
  int32_t table_dtype;     /* dtype, or RFA_ROTARY_TABLE_F32 */
  rfa_rotary_tensor t[2];
  const void *cos, *sin;   /* (P, R/2), 16-byte aligned */
  int64_t P;
  const int32_t *positions; /* (B, S) / (S,) int32, or NULL: the map */
  int64_t pos_batch;       /* elements between two batch entries of positions (0 = shared) */
  int64_t pos_offset;      /* added to positions[], or the map's first offset */
  int32_t pos_stride, pos_split;
  int64_t pos_offset2;
} rfa_rotary_args;
int rfa_rotary(const rfa_rotary_args *args, void *stream);

/* Per-head RMSNorm of q and k fused with the rotary embedding (ring_flash_attn.apply_qk_norm_rotary; csrc/rfa_qknorm.hip) — what
 * Qwen3, Gemma-3 and OLMo-style models run in front of attention: q = rope(rmsnorm_D(q) * w_q), k likewise.  Up to two tensors of
 * one call share rows, positions and tables and go through ONE launch per direction; structs of their own, no existing struct
 * changes (ABI 8 revision 1 stays).  Tensors, tables and positions are rfa_rotary's (t[k].src = the input x, t[k].dst = the
 * output — backward: dx); out of place only.  Of every (row, head), in fp32 with ONE rounding to the io dtype at the end:
 *     rstd = rsqrt(sum_c x_c^2 / D + eps),   a_c = weight_offset + weight[c],   y_c = (x_c * rstd) * a_c
 *     columns [rot_offset, rot_offset + R) of y rotated as rfa_rotary rotates them (the same expression), the others y
 * The norm runs over all D columns.  R == 0 is the norm alone: cos, sin, P and the position fields are not looked at.
 *   weight[k]: (D,), contiguous, 16-byte aligned, weight_dtype = the io dtype or RFA_QK_NORM_WEIGHT_F32.
 * Backward (rfa_qk_norm_rotary_bwd), with g = the conjugate rotation of dout in fp32 (pass-through columns: dout), xh = x rstd
 * (rstd recomputed from x by the forward's own code: nothing but x is kept):
 *     m = (1/D) sum_c g_c a_c xh_c,    dx_c = rstd (g_c a_c - xh_c m)   rounded once
 *     dweight[k][c] = sum over batch, rows and heads of g_c xh_c        fp32 (D,), OVERWRITTEN; NULL: not wanted
 * one launch for dx of both tensors and the per-workgroup partials of dweight, plus one small launch that folds the partials in
 * a fixed order: no atomics, two runs give the same bits.  The bits of an element depend on the row's values, the weight and the
 * position alone — not on the strides, on whether a second tensor rode along, or on how the position was delivered.
 *   workspace: rfa_qk_norm_rotary_bwd_workspace_bytes(args) bytes (a function of ntensors, B, S, D and the H alone; 0 for
 *   arguments the checks below refuse before a pointer is needed), 16-byte aligned, needed where a dweight is asked for; its
 *   contents on entry do not matter.
 * Checks, in this order and before any pointer is read: NULL struct RFA_ERR_NULL; struct_bytes != sizeof, reserved != 0,
 * ntensors outside 1..2, interleaved outside 0..1, a non-zero pad, an eps that is negative or not finite, a weight_offset that
 * is not finite RFA_ERR_ARGS; dtype, a table_dtype that is neither dtype nor RFA_ROTARY_TABLE_F32, a weight_dtype that is
 * neither dtype nor RFA_QK_NORM_WEIGHT_F32 RFA_ERR_DTYPE; D not a multiple of 8 in 8..256, R negative or not a multiple of 16
 * (interleaved: of 8), rot_offset negative or not a multiple of 8, rot_offset + R > D RFA_ERR_HEAD_DIM; B < 0, S < 0, with
 * R > 0 a P < 1, B * S above 2^31 - 1 RFA_ERR_SHAPE; an H <= 0, of any tensor, RFA_ERR_HEADS; then a tensor's B S H above
 * 2^31 - 1 RFA_ERR_SHAPE; B == 0 or S == 0: RFA_OK, nothing is launched or written; NULL src, dst, weight (backward: dout; a
 * dweight without a workspace), with R > 0 a NULL cos or sin RFA_ERR_NULL; pointers or strides off the 16-byte contract (a
 * dweight: 4 bytes) RFA_ERR_ALIGN; dst == src (backward also dst == dout), a negative pos_batch, with R > 0 and the map a
 * negative pos_stride, a pos_split outside 0..S-1 or a position outside [0, P - 1], a workspace_bytes below the stated size
 * RFA_ERR_ARGS. */
#define RFA_QK_NORM_WEIGHT_F32 2
typedef struct {
  uint32_t struct_bytes;   /* sizeof(rfa_qk_norm_rotary_args) */
  uint32_t reserved;       /* 0 */
  int32_t ntensors;        /* 1..2 */
  int32_t B, S, D;         /* packed input: B = 1, S = T */
  int32_t dtype;           /* rfa_dtype */
  int32_t R, rot_offset;   /* R == 0: the norm alone */
  int32_t interleaved;
  int32_t table_dtype;     /* dtype, or RFA_ROTARY_TABLE_F32 */
  int32_t weight_dtype;    /* dtype, or RFA_QK_NORM_WEIGHT_F32 */
  float eps, weight_offset;
  rfa_rotary_tensor t[2];  /* src = x, dst = the output */
  const void *weight[2];   /* (D,) */
  const void *cos, *sin;   /* (P, R/2), 16-byte aligned; R == 0: not looked at */
  int64_t P;
  const int32_t *positions;
  int64_t pos_batch;
  int64_t pos_offset;
  int32_t pos_stride, pos_split;
  int64_t pos_offset2;
} rfa_qk_norm_rotary_args;
typedef struct {
  const void *dout;        /* the gradient of the output, shaped like it */
  int64_t dout_batch, dout_row, dout_head; /* element strides */
} rfa_qk_norm_grad;
typedef struct {
  uint32_t struct_bytes;   /* sizeof(rfa_qk_norm_rotary_bwd_args) */
  uint32_t reserved;       /* 0 */
  int32_t ntensors;
  int32_t B, S, D;
  int32_t dtype;
  int32_t R, rot_offset;
  int32_t interleaved;
  int32_t table_dtype;
  int32_t weight_dtype;
  float eps, weight_offset;
  rfa_rotary_tensor t[2];  /* src = x, dst = dx */
  const void *weight[2];
  const void *cos, *sin;
  int64_t P;
  const int32_t *positions;
  int64_t pos_batch;
  int64_t pos_offset;
  int32_t pos_stride, pos_split;
  int64_t pos_offset2;
  rfa_qk_norm_grad g[2];
  float *dweight[2];       /* fp32 (D,), overwritten; NULL: not wanted */
  void *workspace;
  int64_t workspace_bytes;
} rfa_qk_norm_rotary_bwd_args;
int rfa_qk_norm_rotary_fwd(const rfa_qk_norm_rotary_args *args, void *stream);
int rfa_qk_norm_rotary_bwd(const rfa_qk_norm_rotary_bwd_args *args, void *stream);
int64_t rfa_qk_norm_rotary_bwd_workspace_bytes(const rfa_qk_norm_rotary_bwd_args *args);

/* Per-head max attention logit (QK-Clip / MuonClip; Transformer Engine's and Megatron's `max_logit`): for every query head h
 *     max_logit[h] = max over batch b, query row i and the keys j that row i SEES of  softmax_scale * q[b,i,h,:] . k[b,j,h/G,:]
 * for one block call — the raw scaled dot product (no soft cap, bias, dropout or sink enters it), -inf for a head that sees no
 * pair.  "Sees" is the band of rfa_fwd_args with the same fields and the same meaning: causal, window, mask_shift,
 * mask_shift_lens, q_half / k_half, dense or packed (cu_seqlens) input; dense calls go through the forward's normalisation
 * (mask_shift_lens folded into mask_shift, unreachable bounds dropped, an empty band recognised on the host: it contributes
 * -inf and launches no attention kernel).  No attention kernel and no existing struct changes (ABI 8 revision 1 stays;
 * rfa_ext_args stays): the kernel is the forward's S phase alone (csrc/rfa_maxlogit.hip) — no V, no softmax, no output.
 *   max_logit: (H,) fp32, DEVICE.  accumulate != 0: max_logit[h] = max(max_logit[h], new) — blocks of a ring and calls of a
 *   step fold into one tensor the caller pre-fills with -inf; accumulate == 0: overwritten.
 *   workspace: rfa_max_logit_workspace_bytes() bytes, one fp32 partial per (head, batch entry, block of 256 query rows); may be
 *   NULL when that is 0.  Contents do not matter.  Partials are folded in a fixed order without atomics: the same bits on every
 *   run, and a block cut into block calls accumulates to the bits of the uncut call.
 *   NaN scores are ignored (the hardware max returns its other operand).
 * Checks, in this order and before any tensor pointer is read: NULL struct RFA_ERR_NULL; struct_bytes != sizeof, reserved != 0,
 * a half selector outside 0..2 RFA_ERR_ARGS; dtype RFA_ERR_DTYPE; D not a multiple of 8 in 8..256 RFA_ERR_HEAD_DIM; B, Sq, Sk
 * or total_q negative, or more than 2^31 - 1 workgroups (H * B * ceil(Sq / 256)) RFA_ERR_SHAPE; H or Hk not positive, H not a
 * multiple of Hk RFA_ERR_HEADS; softmax_scale not finite or not positive, only one of cu_seqlens_q / cu_seqlens_k, a non-zero
 * mask_shift with cu_seqlens, |mask_shift_lens| * Sk >= 2^30, workspace_bytes below rfa_max_logit_workspace_bytes()
 * RFA_ERR_ARGS; then NULL max_logit, and — unless the call has nothing to look at — NULL q, k or (where bytes are needed)
 * workspace RFA_ERR_NULL; pointers or strides off the 16-byte contract RFA_ERR_ALIGN. */
typedef struct {
  uint32_t struct_bytes;   /* sizeof(rfa_max_logit_args) */
  uint32_t reserved;       /* 0 */
  const void *q, *k;       /* io dtype: (B,Sq,H,D) / (B,Sk,Hk,D), or packed (Tq,H,D) / (Tk,Hk,D) */
  rfa_strides q_st, k_st;
  const int32_t *cu_seqlens_q, *cu_seqlens_k; /* (B+1,) int32 device, or NULL */
  int32_t B, Sq, Sk, H, Hk, D;                /* packed: Sq / Sk = the longest sequence */
  int64_t total_q;         /* packed: rows of q addressed (kept for symmetry with rfa_fwd_args; not read) */
  int32_t q_half, k_half;
  float softmax_scale;
  int32_t causal;
  int32_t window, window_left, window_right;
  int32_t mask_shift_lens;
  int64_t mask_shift;
  int32_t dtype;           /* rfa_dtype */
  int32_t accumulate;
  float *max_logit;        /* (H,) fp32 */
  void *workspace;
  int64_t workspace_bytes;
} rfa_max_logit_args;
/* bytes of workspace the call needs; 0 for a call without rows or keys and for arguments the call would refuse.  Pure function
 * of H, B, Sq and q_half. */
int64_t rfa_max_logit_workspace_bytes(const rfa_max_logit_args *args);
int rfa_max_logit(const rfa_max_logit_args *args, void *stream);

/* A gradient of lse (ring_flash_attn.with_lse_grad).  lse_i = log sum_j exp(s_ij), so d lse_i / d s_ij = P_ij: a loss that
 * also touches lse, with g_i = dLoss / dlse_i, adds g_i P_ij to dS.  Every backward kernel forms dS = P (dP - delta) — times
 * (1 - t^2) under a soft cap, which multiplies (dP - delta) as a whole; P undropped under dropout, as lse is the undropped
 * softmax's — so handing the UNCHANGED kernels
 *     delta'_i = rowsum(dout_i * out_i) - g_i
 * in place of delta serves it exactly, in every form (7-GEMM dQ, the dS hand-off, the 128-key / 256-key / balanced dK/dV
 * kernels, head dims above 128), with a bias, windows, mask_shift, packed input and GQA.  No attention kernel and no existing
 * struct changes (ABI 8 revision 1 stays; rfa_ext_args stays).
 *   rfa_bwd_preprocess_lse: rfa_bwd_preprocess with `dlse` — fp32, laid out like lse / delta (dense (B, H, Sq), packed (H, Tq),
 *   row stride 1) with batch / head strides of its own, addressed through the same cu_seqlens_q / q_half.  The accumulator is
 *   rfa_bwd_preprocess's; the stored value is ONE fp32 subtraction further: bit for bit delta - dlse.  dlse == NULL: the call IS
 *   rfa_bwd_preprocess (same kernel instance, same bits).  Rows without a visible key (lse = +inf) have P = 0: their dlse is
 *   read and has no effect.
 * Checks, in this order and before any launch: NULL struct RFA_ERR_NULL; dtype, head_dim, H <= 0, B < 0 as rfa_bwd_preprocess;
 * Sq < 0 RFA_ERR_SHAPE; a non-zero `reserved`, a q_half outside 0..2 RFA_ERR_ARGS; B == 0 or Sq == 0: RFA_OK, nothing is
 * launched; NULL dout, out or delta RFA_ERR_NULL; pointers or strides off the 16-byte contract RFA_ERR_ALIGN. */
typedef struct {
  const void *dout, *out;  /* io dtype */
  rfa_strides dout_st, out_st;
  float *delta;            /* same layout contract as lse */
  int64_t delta_batch, delta_head;
  const float *dlse;       /* NULL: rfa_bwd_preprocess */
  int64_t dlse_batch, dlse_head;
  const int32_t *cu_seqlens_q;
  int32_t q_half;
  int32_t B, H, D, Sq;
  int32_t dtype;
  int32_t reserved;        /* 0 */
} rfa_bwd_preprocess_lse_args;
int rfa_bwd_preprocess_lse(const rfa_bwd_preprocess_lse_args *args, void *stream);

/* Pairwise merge of two FINISHED attention results (ring_flash_attn.merge_attn): attention over the union of two key sets is
 *     lse = logaddexp(lse_a, lse_b),   w_x = exp(lse_x - lse),   out = w_a out_a + w_b out_b
 * in fp32, out rounded to the io dtype once.  rfa_merge (the ring's running fp32 accumulator, with the reference's +inf rule)
 * stays as it is.  Backward, from the four forward inputs alone, with x = sum_d dout_d (out_a - out_b)_d:
 *     dout_a = w_a dout,   dout_b = w_b dout,   dlse_a = w_a dlse + w_a w_b x,   dlse_b = w_b dlse - w_a w_b x .
 * x is summed in a fixed order without atomics: the same bits on every run.
 * Empty rows: an infinite lse_x of EITHER sign (+inf: a direct forward; -inf: an accumulate-mode forward) means side x saw no
 * key: its weight is 0, its out is never multiplied and all its gradients are 0.  Both sides empty: out = 0, lse = -inf.
 * Layout: B x S rows of H heads, as rfa_sink_apply — dense out (B, S, H, D) with lse (B, H, S); packed out (T, H, D) with lse
 * (H, T) is B = 1, S = T (batch strides unused).  Every tensor has strides of its own; lse-like tensors have row stride 1.
 * The outputs must not alias the inputs.  rfa_merge_pair_bwd: dlse == NULL reads as zero.
 * Checks, in this order and before any launch: NULL struct RFA_ERR_NULL; dtype, head_dim (a multiple of 8, <= 256), H <= 0,
 * B < 0 as everywhere; S < 0, B or H above 65535, S * H above 16 * (2^31 - 1) RFA_ERR_SHAPE; a non-zero `reserved` RFA_ERR_ARGS;
 * B == 0 or S == 0: RFA_OK, nothing is launched; NULL tensors (all but dlse) RFA_ERR_NULL; pointers or strides of the io-dtype
 * tensors off the 16-byte contract RFA_ERR_ALIGN. */
typedef struct {
  const void *out_a, *out_b;   /* io dtype */
  rfa_strides out_a_st, out_b_st;
  const float *lse_a, *lse_b;
  int64_t lse_a_batch, lse_a_head, lse_b_batch, lse_b_head; /* element strides; row stride is 1 */
  void *out;
  rfa_strides out_st;
  float *lse;
  int64_t lse_batch, lse_head;
  int32_t B, S, H, D;
  int32_t dtype;               /* rfa_dtype */
  int32_t reserved;            /* 0 */
} rfa_merge_pair_args;
int rfa_merge_pair(const rfa_merge_pair_args *args, void *stream);

typedef struct {
  const void *dout;            /* io dtype */
  rfa_strides dout_st;
  const float *dlse;           /* NULL: zero */
  int64_t dlse_batch, dlse_head;
  const void *out_a, *out_b;   /* the forward's inputs */
  rfa_strides out_a_st, out_b_st;
  const float *lse_a, *lse_b;
  int64_t lse_a_batch, lse_a_head, lse_b_batch, lse_b_head;
  void *dout_a, *dout_b;       /* io dtype, overwritten */
  rfa_strides dout_a_st, dout_b_st;
  float *dlse_a, *dlse_b;      /* fp32, overwritten */
  int64_t dlse_a_batch, dlse_a_head, dlse_b_batch, dlse_b_head;
  int32_t B, S, H, D;
  int32_t dtype;
  int32_t reserved;            /* 0 */
} rfa_merge_pair_bwd_args;
int rfa_merge_pair_bwd(const rfa_merge_pair_bwd_args *args, void *stream);

/* A value head dim of its own (multi-head latent attention as DeepSeek-V2/V3 and Kimi K2 train it: QK head dim 192, V head
 * dim 128).  Two entry points with a struct of their own; no existing struct changes (ABI 8 revision 1 stays; rfa_ext_args
 * stays).  The base structs are the existing ones with
 *     D                                                        the QK head dim: q, k, dq, dk (and their accumulators),
 *     v_st, out_st, out_acc_st, dout_st, dv_st, dv_acc_st      rows of head_dim_v elements: v, out, dout, dv,
 * everything else as rfa_fwd / rfa_bwd say.  Served: D a multiple of 8 in 136..192, head_dim_v a multiple of 8 in 8..128,
 * bf16 / fp16, dense and packed input, causal / window / mask_shift / mask_shift_lens, q_half / k_half, plain and accumulate
 * outputs (csrc/rfa_vdim.hip).  No dropout.
 * rfa_bwd_vd runs the BASE arguments' own plan: dkdv_nsplit, phases, RFA_BWD_KV_OVERWRITE, workspace, ds_scratch /
 * ds_scratch_bytes mean what they mean to rfa_bwd, and rfa_bwd_plan, rfa_bwd_workspace_bytes, rfa_bwd_ds_scratch_bytes and
 * rfa_bwd_ds_chunks of the base arguments describe it (the workspace holds D-wide slots for dV too, head_dim_v <= D of them
 * used; the dS scratch does not depend on V: dQ = scale dS K is finished by the same kernel as for rfa_bwd).
 * rfa_bwd_preprocess and rfa_merge serve a head_dim_v-wide out through their own D.
 * Checks, before any pointer of the base struct is looked at: NULL args RFA_ERR_NULL; a NULL vd, struct_bytes below
 * sizeof(rfa_vdim_args) (or above it with a non-zero tail), a non-zero reserved or pad, dropout_p > 0 RFA_ERR_ARGS; head_dim_v
 * not a multiple of 8 in 8..128, D not a multiple of 8 in 136..192 RFA_ERR_HEAD_DIM.  Then the checks of rfa_fwd / rfa_bwd in
 * their order. */
typedef struct {
  uint32_t struct_bytes;       /* sizeof(rfa_vdim_args) as the caller compiled it */
  uint32_t reserved;           /* 0 */
  int32_t head_dim_v;
  int32_t pad;                 /* 0 */
} rfa_vdim_args;
int rfa_fwd_vd(const rfa_fwd_args *args, const rfa_vdim_args *vd, void *stream);
int rfa_bwd_vd(const rfa_bwd_args *args, const rfa_vdim_args *vd, void *stream);

/* Per-row key ranges (interval masks: documents on dense input, prefix-LM, shared prefixes, a window plus global tokens).
 * Two entry points with a struct of their own; no existing struct changes (ABI 8 revision 1 stays).  Query row i of batch
 * entry b sees key row j of the block iff
 *     start[b * batch_stride + i] <= k_pos0 + j < end[b * batch_stride + i]
 * AND the base arguments' own mask (causal, window, mask_shift) allows the pair.  start / end: int32, one entry per query
 * row of the call (row stride 1), GLOBAL key positions; k_pos0: the global position of key row 0 of the block.  Values are
 * clamped to the block, so anything outside it is allowed; start >= end is an empty row (out = 0, lse = +inf; -inf into
 * lse_acc by acc_init; an accumulate call leaves such a row as it was).  All query heads share the ranges; they get no gradient.
 * The kernels are the 8 x 32 forward, the 7-GEMM dQ kernel and the 128-key dK/dV kernel (csrc: the kRng instances), whose
 * tile walks skip the key tiles / query tiles outside every row's range; a call whose rows all miss the block runs as a dark
 * block does.  The backward needs `tile_bounds`: rfa_rowrange_workspace_bytes(args) bytes of device memory, 16-byte aligned,
 * filled and read by rfa_bwd_rr itself (nothing to keep between calls; the forward ignores the field).
 * Served: dense input, head dims 8 .. 128 (multiples of 8), bf16 / fp16, GQA, causal / window / mask_shift, plain and
 * accumulate outputs, the two-phase backward.  rfa_bwd_rr runs the base arguments' plan, which must say what the kernels are:
 * dkdv_form = RFA_DKDV_128 and no ds_scratch — rfa_bwd_plan / rfa_bwd_workspace_bytes of the base arguments then describe it.
 * Checks, in this order, before any tensor pointer of the base struct is looked at: NULL args RFA_ERR_NULL; a NULL rr,
 * struct_bytes below sizeof(rfa_rowrange_args) (or above it with a non-zero tail), a non-zero reserved RFA_ERR_ARGS;
 * dropout_p > 0, cu_seqlens_q / cu_seqlens_k, q_half / k_half, a ds_scratch, (rfa_bwd_rr) dkdv_form other than RFA_DKDV_128
 * RFA_ERR_ARGS; D above 128 RFA_ERR_HEAD_DIM; a negative batch_stride RFA_ERR_ARGS; then the checks of rfa_fwd / rfa_bwd in
 * their order; then, where the call has work to do, a NULL start / end (rfa_bwd_rr: or tile_bounds) RFA_ERR_NULL and a
 * tile_bounds off 16 bytes RFA_ERR_ALIGN. */
typedef struct {
  uint32_t struct_bytes;       /* sizeof(rfa_rowrange_args) as the caller compiled it */
  uint32_t reserved;           /* 0 */
  const int32_t *start;        /* (B, Sq) */
  const int32_t *end;
  int64_t batch_stride;        /* elements between two batch entries of start / end (>= 0) */
  int64_t k_pos0;
  void *tile_bounds;           /* backward only */
} rfa_rowrange_args;
int64_t rfa_rowrange_workspace_bytes(const rfa_bwd_args *args);
int rfa_fwd_rr(const rfa_fwd_args *args, const rfa_rowrange_args *rr, void *stream);
int rfa_bwd_rr(const rfa_bwd_args *args, const rfa_rowrange_args *rr, void *stream);

/* Block-sparse masks (BigBird / Longformer window + global + random blocks, block-selected attention, document masks with
 * shared tokens, a FlexAttention BlockMask's blocks).  Two entry points with a struct of their own; no existing struct changes
 * (ABI 8 revision 1 stays).  The mask has one byte per pair of 128 query rows and 128 keys (RFA_BLOCK_MASK_SIZE), non-zero =
 * lit.  Query row i of head h of batch entry b sees key row j of the block iff
 *     mask[b * batch_stride + h * head_stride + (i / 128) * row_stride + k_blk0 + j / 128] != 0
 * AND the base arguments' own mask (causal, window, mask_shift) allows the pair.  The columns of a mask row are the key blocks
 * of the WHOLE sequence (nk_blocks of them); k_blk0 is the column of the block's key row 0 and may have any sign: a column
 * outside [0, nk_blocks) is dark.  batch_stride / head_stride 0 share the mask between batch entries / query heads (h counts
 * QUERY heads).  The mask must hold ceil(Sq / 128) rows per (batch entry, head).  A row without a visible key: out = 0,
 * lse = +inf (-inf into lse_acc by acc_init; an accumulate call leaves it as it was), zero gradients; a call none of whose pairs
 * is lit runs as a dark block does.  The mask gets no gradient.
 * The kernels are the 8 x 32 forward, the 7-GEMM dQ kernel and the 128-key dK/dV kernel (csrc: the kBlk instances).  Their tile
 * walks are list-driven: a forward / dQ workgroup (256 rows = two query blocks) visits only the 64-key tiles of blocks lit for
 * one of its two query blocks, a dK/dV workgroup (128 keys = one column) only the (64-row Q/dO tile, query head) items lit in
 * its column for that head.  They read the bytes themselves (64 at a time, kept as bits in scalar registers), so no packed
 * form is needed: rfa_blockmask_workspace_bytes() is 0 and `workspace` is not looked at (leave it NULL).
 * Served: dense input, head dims 8 .. 128 (multiples of 8), bf16 / fp16, GQA with at most 64 query heads per K/V head,
 * causal / window / mask_shift, plain and accumulate outputs, the two-phase backward.  rfa_bwd_bm runs the base arguments'
 * plan, which must say what the kernels are: dkdv_form = RFA_DKDV_128 and no ds_scratch — the contract of rfa_bwd_rr.
 * dkdv_nsplit is ignored: that plan has no shares (one workgroup per key block walks all of the column's visited items).
 * Checks, in this order, before any tensor pointer of the base struct is looked at: NULL args RFA_ERR_NULL; a NULL bm,
 * struct_bytes below sizeof(rfa_blockmask_args) (or above it with a non-zero tail), a non-zero reserved RFA_ERR_ARGS;
 * dropout_p > 0, cu_seqlens_q / cu_seqlens_k, q_half / k_half, (rfa_bwd_bm) a ds_scratch or a dkdv_form other than
 * RFA_DKDV_128 RFA_ERR_ARGS; D above 128 RFA_ERR_HEAD_DIM; a negative stride or nk_blocks, nk_blocks above 2^31 - 1, k_blk0
 * outside [-2^30, 2^30], more than 64 query heads per K/V head RFA_ERR_ARGS; then the checks of rfa_fwd / rfa_bwd in their
 * order; then, where the call has work to do, a NULL mask RFA_ERR_NULL. */
#define RFA_BLOCK_MASK_SIZE 128
typedef struct {
  uint32_t struct_bytes;       /* sizeof(rfa_blockmask_args) as the caller compiled it */
  uint32_t reserved;           /* 0 */
  const uint8_t *mask;         /* (Bm, Hm, ceil(Sq / 128), nk_blocks) bytes, non-zero = lit; column stride 1 */
  int64_t batch_stride;        /* bytes between two batch entries (0 = broadcast) */
  int64_t head_stride;         /* bytes between two query heads (0 = broadcast) */
  int64_t row_stride;          /* bytes between two query blocks */
  int64_t nk_blocks;           /* columns of a mask row: key blocks of the whole sequence */
  int64_t k_blk0;              /* column of key row 0 of this block */
  void *workspace;             /* rfa_blockmask_workspace_bytes() bytes (0 today: may be NULL) */
} rfa_blockmask_args;
int64_t rfa_blockmask_workspace_bytes(const rfa_bwd_args *args);
int rfa_fwd_bm(const rfa_fwd_args *args, const rfa_blockmask_args *bm, void *stream);
int rfa_bwd_bm(const rfa_bwd_args *args, const rfa_blockmask_args *bm, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RFA_H_ */
