"""Operator backend: the seam between the ring schedules (Python) and the attention kernels.

`HipBackend` is the product: it translates torch tensors into the plain-pointer C ABI of
librfa_hip.so (include/rfa.h) and launches on torch's current HIP stream.  It is the stand-in
for what the reference imports from the CUDA-only `flash_attn` package
(/root/reference/ring_flash_attn/zigzag_ring_flash_attn.py:3, ring_flash_attn_varlen.py:3-6).

There is deliberately NO CPU implementation here.  The test suite injects the CPU oracle
(oracle/flash_attn_ref.py) through ring_flash_attn._testing.set_backend to exercise the *schedules*
under gloo on a GPU-less machine; the product never selects anything but HipBackend, and HipBackend
raises if the extension is missing or a tensor is not on a HIP device.
"""
import ctypes as C
from typing import Optional

import torch

from . import _C, config

HALF_FULL, HALF_FRONT, HALF_BACK = _C.HALF_FULL, _C.HALF_FRONT, _C.HALF_BACK

_DTYPES = {torch.bfloat16: _C.RFA_BF16, torch.float16: _C.RFA_F16}


def _st3(t: torch.Tensor, varlen: bool) -> _C.Strides:
    """(batch,row,head) element strides of (B,S,H,D) or (T,H,D)."""
    if t.stride(-1) != 1:
        raise ValueError("last (head_dim) stride must be 1")
    if varlen:
        return _C.Strides(0, t.stride(0), t.stride(1))
    return _C.Strides(t.stride(0), t.stride(1), t.stride(2))


def _lse_st(t: torch.Tensor, varlen: bool):
    """(batch, head) strides of a (B,H,S) / (H,T) fp32 tensor; row stride must be 1."""
    if t.dtype != torch.float32:
        raise ValueError("lse/delta tensors must be float32")
    if t.stride(-1) != 1 and t.shape[-1] != 1:
        raise ValueError("lse row stride must be 1")
    if varlen:
        return 0, t.stride(0)
    return t.stride(0), t.stride(1)


_DESC_MAX_ROWS = 256     # csrc/rfa_kernels.hpp: kDescMaxRows — the rows one tile's 32-bit byte offsets have to span


def _row_stride_ok(t: torch.Tensor) -> bool:
    """include/rfa.h, "row strides": 256 * |row stride| * element size + D * element size <= 2^31 - 1 for a (B, S, H, D) /
    (T, H, D) tensor; the batch and head strides are free"""
    if t.dim() < 3:
        return True
    e = t.element_size()
    return _DESC_MAX_ROWS * abs(t.stride(-3)) * e + t.shape[-1] * e <= 2 ** 31 - 1


def _in_contract(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """an INPUT tensor as the library takes it: t, or a contiguous copy of a view whose row stride the kernels' 32-bit tile
    offsets cannot express (the library refuses it: RFA_ERR_ARGS) — a legal torch view stays a legal argument"""
    return t if t is None or _row_stride_ok(t) else t.contiguous()


def _rows16(t: torch.Tensor) -> torch.Tensor:
    """t, or a contiguous copy when a view's rows are off the library's 16-byte contract (last stride 1, 2-byte elements)
    or its row stride beyond the library's bound (_row_stride_ok)"""
    if t.stride(-1) != 1 or any(st % 8 for st in t.stride()[:-1]) or t.data_ptr() % 16 or not _row_stride_ok(t):
        return t.contiguous()
    return t


def _unit_rows(t: torch.Tensor) -> torch.Tensor:
    """an lse-like tensor with row stride 1 (a copy when it has another)"""
    return t.contiguous() if t.stride(-1) != 1 and t.shape[-1] != 1 else t


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class HipBackend:
    """MI355X kernels through the C ABI.  All methods enqueue on the current stream and return
    immediately; outputs are caller-allocated unless stated otherwise."""

    name = "hip"
    serves_mask_shift = True        # fwd / bwd take `mask_shift` (include/rfa.h, ABI 7): what a windowed multi-rank schedule needs
    serves_mask_shift_lens = True   # ... and `mask_shift_lens` (ABI 8), the per-sequence shift the packed (varlen) ring schedules need
    serves_alibi = True             # fwd / bwd take `alibi=(slopes, shift)` (include/rfa.h: rfa_ext_args)
    serves_softcap = True           # ... and `softcap=` (flash_attn's logit soft-capping: rfa_ext_args.softcap)
    serves_sinks = True             # sink_apply / sink_grad (include/rfa.h: rfa_sink_apply, rfa_sink_grad): ring_flash_attn.with_sinks
    serves_seq_head_exchange = True  # seq_head_copy (include/rfa.h: rfa_seq_head_copy): ring_flash_attn.with_ulysses
    serves_max_logit = True          # max_logit (include/rfa.h: rfa_max_logit): ring_flash_attn.with_max_logit
    serves_lse_grad = True           # bwd_preprocess takes `dlse=` (include/rfa.h: rfa_bwd_preprocess_lse): ring_flash_attn.with_lse_grad
    serves_merge_pair = True         # merge_pair / merge_pair_bwd (include/rfa.h: rfa_merge_pair, rfa_merge_pair_bwd): ring_flash_attn.merge_attn
    serves_vdim = True               # fwd / bwd take a `v` whose head dim differs from q's (include/rfa.h: rfa_fwd_vd, rfa_bwd_vd): MLA 192 / 128
    serves_row_ranges = True         # fwd / bwd take `row_ranges=(start, end, k_pos0)` (include/rfa.h: rfa_fwd_rr, rfa_bwd_rr): ring_flash_attn.with_row_ranges
    serves_block_mask = True         # fwd / bwd take `block_mask=(mask_view, k_blk0)` (include/rfa.h: rfa_fwd_bm, rfa_bwd_bm): ring_flash_attn.with_block_mask
    serves_rotary = True             # rotary (include/rfa.h: rfa_rotary): ring_flash_attn.apply_rotary
    serves_qk_norm = True            # qk_norm_rotary_fwd / _bwd (include/rfa.h: rfa_qk_norm_rotary_fwd / _bwd): ring_flash_attn.apply_qk_norm_rotary
    serves_dropout_positions = True  # `dropout=` takes the position maps (q_map, k_map): what dropout over a dense ring, zigzag or stripe schedule needs

    def __init__(self):
        self.lib = _C.load()
        self._ds_pool = {}            # (device index, stream handle) -> the ONE reusable dS scratch of that stream
        self._ds_capped = {}          # same key -> [backwards left until growth of a memory-capped scratch is retried]

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _check_dev(*ts):
        for t in ts:
            if t is not None and not t.is_cuda:
                raise RuntimeError(
                    "ring_flash_attn: tensors must live on a HIP (cuda) device — there is no CPU "
                    "compute path in this package"
                )

    @staticmethod
    def _dtype(t):
        try:
            return _DTYPES[t.dtype]
        except KeyError:
            raise TypeError(f"ring_flash_attn: unsupported dtype {t.dtype} (bf16/fp16 only)") from None

    # ------------------------------------------------------------------ forward
    def fwd(self, q, k, v, *, softmax_scale, causal, cu_seqlens_q=None, cu_seqlens_k=None,
            max_seqlen_q=None, max_seqlen_k=None, q_half=HALF_FULL, k_half=HALF_FULL,
            out=None, lse=None, out_acc=None, lse_acc=None, acc_init=False, window=(-1, -1), dropout=None,
            mask_shift=0, mask_shift_lens=0, alibi=None, softcap=0.0, row_ranges=None, block_mask=None):
        """Block attention.  Plain mode fills (out, lse); accumulate mode merges into the fp32
        (out_acc, lse_acc) pair (fused update_out_and_lse).  Dense: q (B,Sq,H,D); varlen: (T,H,D).
        dropout: (p, seed, q_pos_offset, k_pos_offset, head_offset), the same plus the position maps (q_map, k_map) —
        each (stride, split, offset2), _common.dropout_arg — or None.
        mask_shift: where the block sits in a longer sequence (include/rfa.h; dense input) — for blocks of equal length
        the global position of q row 0 minus that of k row 0; moves the causal diagonal and the window alike.
        mask_shift_lens: the same in units of every sequence's own key length (include/rfa.h, ABI 8): the shift of packed
        (cu_seqlens) input; dense input folds it into mask_shift.
        alibi: (slopes, shift) or None — fp32 slopes (H,) or (B, H) on q's device and the block's alibi_shift
        (include/rfa.h: rfa_ext_args; _common.alibi_arg validates and builds it).
        softcap: scores become softcap * tanh(softmax_scale * q.k / softcap) in front of the mask (include/rfa.h:
        rfa_ext_args.softcap); 0 is off — the plain call.
        row_ranges: (start, end, k_pos0) or None — int32 (B, Sq) tensors on q's device (row stride 1; the batch stride is
        free, so a schedule passes slices) holding GLOBAL key positions, and the global position of k's row 0: row i sees key
        row j iff start[b, i] <= k_pos0 + j < end[b, i] and the call's own mask allows it (include/rfa.h: rfa_rowrange_args).
        Dense input, head dims <= 128, no dropout, bias or cap.
        block_mask: (mask_view, k_blk0) or None — a bool / uint8 (Bm, Hm, ceil(Sq / 128), NK) tensor on q's device (Bm in {1, B},
        Hm in {1, H}; column stride 1, the other strides are free, so a schedule passes slices) and the mask column of k's row 0:
        row i of query head h sees key row j iff mask[b, h, i // 128, k_blk0 + j // 128] (columns outside [0, NK) are dark)
        and the call's own mask allows it (include/rfa.h: rfa_blockmask_args).  The conditions of row_ranges; not with them."""
        self._check_dev(q, k, v, out, lse, out_acc, lse_acc)
        q, k, v = _in_contract(q), _in_contract(k), _in_contract(v)
        varlen = cu_seqlens_q is not None
        a = _C.FwdArgs()
        a.q, a.k, a.v = _ptr(q), _ptr(k), _ptr(v)
        a.q_st, a.k_st, a.v_st = _st3(q, varlen), _st3(k, varlen), _st3(v, varlen)
        if out_acc is not None:
            a.out_acc, a.out_acc_st = _ptr(out_acc), _st3(out_acc, varlen)
            a.lse_acc = _ptr(lse_acc)
            a.lse_acc_batch, a.lse_acc_head = _lse_st(lse_acc, varlen)
            a.acc_init = 1 if acc_init else 0
        else:
            a.out, a.out_st = _ptr(out), _st3(out, varlen)
            a.lse = _ptr(lse)
            a.lse_batch, a.lse_head = _lse_st(lse, varlen)
        if varlen:
            a.cu_seqlens_q, a.cu_seqlens_k = _ptr(cu_seqlens_q), _ptr(cu_seqlens_k)
            a.B = cu_seqlens_q.numel() - 1
            a.H, a.D = q.shape[1], q.shape[2]
            a.Hk = k.shape[1]
            a.Sq, a.Sk = int(max_seqlen_q), int(max_seqlen_k)
            a.total_q = q.shape[0]
        else:
            a.B, a.Sq, a.H, a.D = q.shape
            a.Sk, a.Hk = k.shape[1], k.shape[2]
        a.q_half, a.k_half = q_half, k_half
        a.softmax_scale = float(softmax_scale)
        a.causal = 1 if causal else 0
        if window is not None and (window[0] >= 0 or window[1] >= 0):
            a.window, a.window_left, a.window_right = 1, int(window[0]), int(window[1])
        a.mask_shift = int(mask_shift)
        a.mask_shift_lens = int(mask_shift_lens)
        a.dtype = self._dtype(q)
        _set_dropout(a, dropout)
        a.fwd_form = _fwd_form()
        a.kv_nsplit = config.get().fwd_kv_nsplit
        # split-KV launches (few query rows against many keys on an under-filled grid: include/rfa.h) need a small
        # workspace for the partial (out, lse) pairs: a few tens of MB, only for the calls that split
        vd = _vdim_args(q, v, alibi, softcap, dropout)
        rr = _rowrange_args(row_ranges, q, alibi, softcap, dropout, vd, varlen)
        bm = _blockmask_args(block_mask, q, alibi, softcap, dropout, vd, varlen, rr)
        if rr is not None:                        # per-row key ranges: the kRng instances of the 8 x 32 form, never split
            _C.check(self.lib.rfa_fwd_rr(C.byref(a), C.byref(rr), _stream(q)), "rfa_fwd_rr")
            return
        if bm is not None:                        # a block-sparse mask: the kBlk instances of the same form
            _C.check(self.lib.rfa_fwd_bm(C.byref(a), C.byref(bm), _stream(q)), "rfa_fwd_bm")
            return
        if vd is not None:                        # a value head dim of its own (csrc/rfa_vdim.hip): never split either
            _C.check(self.lib.rfa_fwd_vd(C.byref(a), C.byref(vd), _stream(q)), "rfa_fwd_vd")
            return
        ext = _ext_args(alibi, q, softcap)
        if ext is not None:                       # a bias or a cap is never split: no workspace (include/rfa.h)
            _C.check(self.lib.rfa_fwd_ex(C.byref(a), C.byref(ext), _stream(q)), "rfa_fwd_ex")
            return
        ws = None
        nbytes = self.lib.rfa_fwd_workspace_bytes(C.byref(a), None)
        if nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
            a.workspace = ws.data_ptr()
        _C.check(self.lib.rfa_fwd(C.byref(a), _stream(q)), "rfa_fwd")

    # ------------------------------------------------------------------ backward
    def bwd_preprocess(self, dout, out, delta, *, cu_seqlens_q=None, max_seqlen_q=None, q_half=HALF_FULL, dlse=None):
        """delta[b,h,i] = sum_d dout*out, fp32, laid out like lse.
        dlse: the gradient of lse (ring_flash_attn.with_lse_grad) — fp32, laid out like lse / delta, row stride 1: delta
        becomes sum_d dout*out - dlse, which carries it through every backward kernel (include/rfa.h:
        rfa_bwd_preprocess_lse).  None: the existing call, bit for bit."""
        self._check_dev(dout, out, delta, dlse)
        dout, out = _in_contract(dout), _in_contract(out)
        varlen = cu_seqlens_q is not None
        a = _C.BwdPreArgs() if dlse is None else _C.BwdPreLseArgs()
        a.dout, a.out, a.delta = _ptr(dout), _ptr(out), _ptr(delta)
        a.dout_st, a.out_st = _st3(dout, varlen), _st3(out, varlen)
        a.delta_batch, a.delta_head = _lse_st(delta, varlen)
        if dlse is not None:
            if tuple(dlse.shape) != tuple(delta.shape):
                raise ValueError(f"dlse {tuple(dlse.shape)} must have delta's shape {tuple(delta.shape)}")
            a.dlse = _ptr(dlse)
            a.dlse_batch, a.dlse_head = _lse_st(dlse, varlen)
        if varlen:
            a.cu_seqlens_q = _ptr(cu_seqlens_q)
            a.B = cu_seqlens_q.numel() - 1
            a.H, a.D = dout.shape[1], dout.shape[2]
            a.Sq = int(max_seqlen_q)
        else:
            a.B, a.Sq, a.H, a.D = dout.shape
        a.q_half = q_half
        a.dtype = self._dtype(dout)
        if dlse is not None:
            _C.check(self.lib.rfa_bwd_preprocess_lse(C.byref(a), _stream(dout)), "rfa_bwd_preprocess_lse")
            return
        _C.check(self.lib.rfa_bwd_preprocess(C.byref(a), _stream(dout)), "rfa_bwd_preprocess")

    def bwd(self, dout, q, k, v, lse, delta, *, softmax_scale, causal, cu_seqlens_q=None,
            cu_seqlens_k=None, max_seqlen_q=None, max_seqlen_k=None, q_half=HALF_FULL,
            k_half=HALF_FULL, dq=None, dk=None, dv=None, dq_acc=None, dk_acc=None, dv_acc=None,
            acc_init=False, deterministic=False, phases=_C.BWD_ALL, partials=None, ds_scratch=None,
            window=(-1, -1), prof_events=None, dropout=None, mask_shift=0, mask_shift_lens=0, alibi=None,
            softcap=0.0, row_ranges=None, block_mask=None):
        """dQ/dK/dV of one block.  Plain outputs (io dtype) or `+=` into fp32 accumulators.
        phases=BWD_COMPUTE / BWD_REDUCE splits the call so a ring step can overlap the kernels
        with the arrival of the dk/dv accumulators it adds into: the COMPUTE call RETURNS the buffer
        holding its dK/dV partials and the REDUCE call must be handed exactly that buffer (`partials=`),
        so interleaved backwards (other streams, re-entrant / checkpointed autograd, pipeline
        micro-batches) can never consume each other's partials.  Scratch comes from torch's caching
        allocator on the current stream, per call; the C library itself never allocates.
        alibi, softcap: as in fwd, with the forward's values; such a call names the 128-key dK/dV form and takes no dS scratch —
        what rfa_bwd_ex asks of the base arguments (include/rfa.h).
        row_ranges: as in fwd, with the forward's values; the same two conditions (rfa_bwd_rr), plus a small tile-bounds
        workspace from torch's caching allocator, per call.
        block_mask: as in fwd, with the forward's values; the same two conditions (rfa_bwd_bm); no workspace."""
        self._check_dev(dout, q, k, v, lse, delta, dq, dk, dv, dq_acc, dk_acc, dv_acc)
        dout, q, k, v = _in_contract(dout), _in_contract(q), _in_contract(k), _in_contract(v)
        varlen = cu_seqlens_q is not None
        a = _C.BwdArgs()
        a.dout, a.q, a.k, a.v = _ptr(dout), _ptr(q), _ptr(k), _ptr(v)
        a.dout_st, a.q_st = _st3(dout, varlen), _st3(q, varlen)
        a.k_st, a.v_st = _st3(k, varlen), _st3(v, varlen)
        a.lse = _ptr(lse)
        a.lse_batch, a.lse_head = _lse_st(lse, varlen)
        a.delta = _ptr(delta)
        a.delta_batch, a.delta_head = _lse_st(delta, varlen)
        if dq_acc is not None:
            a.dq_acc, a.dq_acc_st = _ptr(dq_acc), _st3(dq_acc, varlen)
        else:
            a.dq, a.dq_st = _ptr(dq), _st3(dq, varlen)
        if dk_acc is not None:
            a.dk_acc, a.dv_acc = _ptr(dk_acc), _ptr(dv_acc)
            a.dk_acc_st, a.dv_acc_st = _st3(dk_acc, varlen), _st3(dv_acc, varlen)
        else:
            a.dk, a.dv = _ptr(dk), _ptr(dv)
            a.dk_st, a.dv_st = _st3(dk, varlen), _st3(dv, varlen)
        a.acc_init = 1 if acc_init else 0
        if varlen:
            a.cu_seqlens_q, a.cu_seqlens_k = _ptr(cu_seqlens_q), _ptr(cu_seqlens_k)
            a.B = cu_seqlens_q.numel() - 1
            a.H, a.D = q.shape[1], q.shape[2]
            a.Hk = k.shape[1]
            a.Sq, a.Sk = int(max_seqlen_q), int(max_seqlen_k)
            a.total_k, a.total_q = k.shape[0], q.shape[0]
        else:
            a.B, a.Sq, a.H, a.D = q.shape
            a.Sk, a.Hk = k.shape[1], k.shape[2]
            a.total_k = a.B * a.Sk
        a.q_half, a.k_half = q_half, k_half
        a.softmax_scale = float(softmax_scale)
        a.causal = 1 if causal else 0
        a.deterministic = 1 if deterministic else 0
        if window is not None and (window[0] >= 0 or window[1] >= 0):
            a.window, a.window_left, a.window_right = 1, int(window[0]), int(window[1])
        a.mask_shift = int(mask_shift)
        a.mask_shift_lens = int(mask_shift_lens)
        a.dtype = self._dtype(q)
        a.phases = phases
        _set_dropout(a, dropout)
        if prof_events is not None:       # measurement (bench.py): a ctypes array of 4 hipEvent_t, see include/rfa.h
            a.prof_events = prof_events
        reduce_only = bool(phases & _C.BWD_REDUCE) and not (phases & _C.BWD_COMPUTE)
        # dK/dV launch plan: part of the call (ABI 4).  The tuning / test overrides (config.dkdv_wide, config.dkdv_nsplit)
        # are applied HERE, once per backward; a REDUCE call is given the plan its COMPUTE call RESOLVED (it travels with
        # the `partials` token), so the two phases cannot disagree whatever the configuration, or the chunking of the
        # dS hand-off, does in between.
        if reduce_only and partials is not None and hasattr(partials, "_rfa_plan"):
            a.dkdv_form, a.dkdv_nsplit = partials._rfa_plan
        else:
            a.dkdv_form, a.dkdv_nsplit = _plan_overrides()
        # 5-GEMM backward (csrc/rfa_dqs.hip): the dK/dV kernel hands dS to the dQ kernel through a scratch instead of dQ
        # recomputing S and dP, when the call is eligible (D == 128 or 256, whole sequences, dense or packed).  The
        # scratch is ONE reusable buffer per device and stream (bwd_ds_scratch below), at most config.ds_spill_max_bytes
        # large: a hand-off that does not fit runs in head-group chunks over it (include/rfa.h: ds_scratch_bytes).
        # config.bwd_ds_spill = False (RFA_BWD_DS_SPILL=0) keeps the 7-GEMM form.  Callers that split one backward over
        # several calls (measurement: BWD_SKIP_DQ / BWD_SKIP_DKDV) pass the same `ds_scratch` to both.
        vd = _vdim_args(q, v, alibi, softcap, dropout)    # (rfa_bwd_vd runs the base arguments' own plan and scratch)
        ext = _ext_args(alibi, q, softcap)
        rr = _rowrange_args(row_ranges, q, alibi, softcap, dropout, vd, varlen)
        bm = _blockmask_args(block_mask, q, alibi, softcap, dropout, vd, varlen, rr)
        if ext is not None or rr is not None or bm is not None:
            a.dkdv_form, a.dkdv_nsplit, ds_scratch = _C.DKDV_128, 0, None
        if ext is None and rr is None and bm is None and ds_scratch is None and not reduce_only and _spill_enabled():
            ds_scratch = self.bwd_ds_scratch(a, q.device)
        if ds_scratch is not None and not reduce_only:
            a.ds_scratch = ds_scratch.data_ptr()
            a.ds_scratch_bytes = ds_scratch.numel() * ds_scratch.element_size()
        nbytes = self.lib.rfa_bwd_workspace_bytes(C.byref(a))
        ws = None
        if reduce_only:
            if partials is None:
                raise RuntimeError("rfa_bwd: a BWD_REDUCE call needs the `partials` buffer its BWD_COMPUTE call returned")
            if partials.device != q.device or partials.numel() < nbytes:
                raise RuntimeError("rfa_bwd: `partials` does not belong to this call (device / size mismatch)")
            ws = partials
        elif nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
            form, ns, _ = self.bwd_plan(a)           # the RESOLVED plan (with this call's scratch): what a REDUCE call must repeat
            ws._rfa_plan = (form, ns if form == _C.DKDV_256 or a.D > 128 else 0)
        if ws is not None:
            a.workspace = ws.data_ptr()
        if rr is not None:
            nb = self.lib.rfa_rowrange_workspace_bytes(C.byref(a))
            tb = torch.empty(max(nb, 16), dtype=torch.uint8, device=q.device)
            rr.tile_bounds = tb.data_ptr()
            _C.check(self.lib.rfa_bwd_rr(C.byref(a), C.byref(rr), _stream(q)), "rfa_bwd_rr")
        elif bm is not None:
            _C.check(self.lib.rfa_bwd_bm(C.byref(a), C.byref(bm), _stream(q)), "rfa_bwd_bm")
        elif vd is not None:
            _C.check(self.lib.rfa_bwd_vd(C.byref(a), C.byref(vd), _stream(q)), "rfa_bwd_vd")
        elif ext is not None:
            _C.check(self.lib.rfa_bwd_ex(C.byref(a), C.byref(ext), _stream(q)), "rfa_bwd_ex")
        else:
            _C.check(self.lib.rfa_bwd(C.byref(a), _stream(q)), "rfa_bwd")
        return ws if (phases & _C.BWD_COMPUTE) else None

    def bwd_plan(self, a):
        """(form, nsplit, five_gemm) the call described by `a` (a filled BwdArgs) will run"""
        form, ns, five = C.c_int32(), C.c_int32(), C.c_int32()
        _C.check(self.lib.rfa_bwd_plan(C.byref(a), C.byref(form), C.byref(ns), C.byref(five)), "rfa_bwd_plan")
        return form.value, ns.value, five.value

    def bwd_ds_chunks(self, a):
        """(nchunks, kv_heads, q_heads_per_kv_head, chunk_bytes) of the dS hand-off of the call described by `a`
        (nchunks 0: the 7-GEMM form)"""
        n, hc, gc, cb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _C.check(self.lib.rfa_bwd_ds_chunks(C.byref(a), C.byref(n), C.byref(hc), C.byref(gc), C.byref(cb)), "rfa_bwd_ds_chunks")
        return n.value, hc.value, gc.value, cb.value

    def bwd_ds_scratch(self, a, device):
        """The dS scratch for the call described by `a` (a filled BwdArgs), or None: the call then runs the 7-GEMM form.

        ONE buffer per (device, stream), kept and reused by every backward on that stream (kernels of one stream run in
        order, so the next backward's dK/dV kernel cannot start before this one's dQ kernel has read the blocks) —
        no 2 GB allocation per backward, and peak memory independent of the head count and the sequence length: the
        buffer is at most config.ds_spill_max_bytes (default 4.5 GiB; the headline's hand-off is 2.0 GiB and takes just that) and,
        when it is first taken or has to grow, at most config.ds_spill_max_frac (0.5) of the memory free at that moment;
        a hand-off that does not fit runs in head-group chunks over it (include/rfa.h: ds_scratch_bytes; long contexts
        keep the 5-GEMM form — measured at S = 32768, 32 heads, 34 GB of dS: 942 TFLOP/s in 8 chunks of 4 query heads
        against 950 with the whole hand-off resident and 895 for the 7-GEMM form; chunks of 2 query heads — a 2.5 GiB
        limit — give the dQ kernel only one workgroup per CU and fall to 848, which is why the default is not smaller).  A hand-off whose smallest chunk does not fit, or an allocation failure, falls back to
        the 7-GEMM form instead of failing a backward that would have fitted without it (logged once).
        `release_scratch()` returns the buffers."""
        full = self.lib.rfa_bwd_ds_scratch_bytes(C.byref(a))
        if full <= 0:
            return None
        least = self.lib.rfa_bwd_ds_scratch_min_bytes(C.byref(a))
        want = min(full, max(_spill_limit(), 0))
        capped = False
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream) if device.type == "cuda" else ("cpu", 0)
        buf = self._ds_pool.get(key)
        if buf is not None:
            if buf.numel() >= min(want, full):
                return buf                                  # (the steady state: no query, no allocation)
            # a buffer that was CAPPED by the free-memory fraction when it was taken is smaller than `want` for ever:
            # keep using it (the hand-off runs in chunks over it) instead of querying the allocator, dropping and
            # re-making it in every backward; growth is retried once in a while
            retry = self._ds_capped.get(key)
            if retry is not None and buf.numel() >= least:
                retry[0] -= 1
                if retry[0] > 0:
                    return buf
        if want < least:
            _log_once("spill-limit", f"ring_flash_attn: the dS hand-off needs at least {least / 2**30:.2f} GiB per chunk "
                                     f"(limit {want / 2**30:.2f} GiB): this backward runs the 7-GEMM form")
            return None
        if device.type == "cuda" and want > _SPILL_CHECK_ABOVE:
            free, _ = torch.cuda.mem_get_info(device)
            cached = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
            have = buf.numel() if buf is not None else 0
            cap = int(_spill_frac() * (free + cached + have))
            if cap < want:
                want = cap
                capped = True
        if buf is not None and buf.numel() >= least and want <= buf.numel():
            # a growth retry that would not GROW the pooled buffer (memory is as tight as before, or tighter): keep what
            # works — never trade a usable scratch for a smaller one or for the 7-GEMM form — and try again later
            self._ds_capped[key] = [_SPILL_GROW_RETRY]
            return buf
        if want < least:
            _log_once("spill-mem", f"ring_flash_attn: not enough free memory for a dS hand-off chunk ({least / 2**30:.2f} GiB): "
                                   "this backward runs the 7-GEMM form")
            return None
        self._ds_pool.pop(key, None)
        buf = None
        try:
            buf = torch.empty(want, dtype=torch.uint8, device=device)
        except torch.OutOfMemoryError:
            _log_once("spill-oom", f"ring_flash_attn: a dS hand-off scratch of {want / 2**30:.2f} GiB could not be allocated: "
                                   "this backward runs the 7-GEMM form")
            return None
        self._ds_pool[key] = buf
        if capped:
            self._ds_capped[key] = [_SPILL_GROW_RETRY]
        else:
            self._ds_capped.pop(key, None)
        return buf

    def zero_outside(self, shape, dtype, device, lo, hi, slot=0, dim=0):
        """A reusable buffer of `shape` whose rows OUTSIDE [lo, hi) along `dim` are zero — the dK/dV contribution buffer of
        the llama3 backward, whose rows inside the range the dK/dV kernel overwrites completely on every call (key blocks
        without a visible query store zeros) and whose rows outside must read as zero in the reduce-scatter.  Rounds 2-5
        allocated it per backward and zero-filled the outside rows with torch fills (7 us launches on a
        0.5 ms step); now ONE buffer per (device, stream, shape, slot) is zeroed when it is made and only the rows that LEAVE
        the range between two calls are zeroed again (a packed batch whose local key slice shrinks).  Safe to reuse: every
        caller waits for the collective that reads the buffer before it returns."""
        cuda = device.type == "cuda"
        key = ("zero", (device.index if device.index is not None else torch.cuda.current_device()) if cuda else -1,
               torch.cuda.current_stream(device).cuda_stream if cuda else 0, tuple(shape), dtype, slot, dim)
        ent = self._ds_pool.get(key)
        if ent is None:
            buf = torch.zeros(shape, dtype=dtype, device=device)
            self._ds_pool[key] = [buf, lo, hi]
            return buf
        buf, plo, phi = ent
        if lo > plo:                                   # rows [plo, lo) were inside, now outside
            buf.narrow(dim, plo, min(lo, phi) - plo).zero_()
        if hi < phi:
            start = max(hi, plo)
            buf.narrow(dim, start, phi - start).zero_()
        ent[1], ent[2] = lo, hi
        return buf

    def release_scratch(self):
        """drop the reusable dS scratch buffers (they are re-made on demand): up to config.ds_spill_max_bytes per device
        and stream that the pool otherwise holds for the life of the process — call it before a phase that needs the
        memory (evaluation with long sequences, checkpoint loading), or from an out-of-memory handler"""
        self._ds_pool.clear()
        self._ds_capped.clear()

    # ------------------------------------------------------------------ side kernels
    def merge(self, out_acc, lse_acc, block_out, block_lse, *, acc_init=False):
        """Stand-alone (out, lse) merge.  out_acc/block_out: (B,S,H,D) views; lse_acc/block_lse:
        (B,H,S) views of ANY strides (so the reference's (B,S,H,1) running lse works too)."""
        self._check_dev(out_acc, lse_acc, block_out, block_lse)
        if lse_acc.dtype != torch.float32 or block_lse.dtype != torch.float32:
            raise ValueError("lse tensors must be float32")
        a = _C.MergeArgs()
        a.out_acc, a.out_acc_st = _ptr(out_acc), _st3(out_acc, False)
        a.lse_acc = _ptr(lse_acc)
        a.lse_acc_batch, a.lse_acc_head, a.lse_acc_row = lse_acc.stride()
        a.block_out, a.block_out_st = _ptr(block_out), _st3(block_out, False)
        a.block_lse = _ptr(block_lse)
        a.block_lse_batch, a.block_lse_head, a.block_lse_row = block_lse.stride()
        a.B, a.S, a.H, a.D = block_out.shape
        a.acc_init = 1 if acc_init else 0
        a.dtype = self._dtype(block_out)
        _C.check(self.lib.rfa_merge(C.byref(a), _stream(block_out)), "rfa_merge")

    # ------------------------------------------------------------------ pairwise merge (ring_flash_attn.merge_attn)
    def merge_pair(self, out_a, lse_a, out_b, lse_b):
        """(out, lse) of attention over the union of two key sets from the two parts' finished results: lse =
        logaddexp(lse_a, lse_b), out = exp(lse_a - lse) out_a + exp(lse_b - lse) out_b in fp32, rounded once (include/rfa.h:
        rfa_merge_pair).  out_x (B,S,H,D) with lse_x (B,H,S), or packed (T,H,D) with (H,T); an infinite lse_x of either sign
        marks an empty side.  New tensors."""
        self._check_dev(out_a, lse_a, out_b, lse_b)
        varlen = out_a.dim() == 3
        out_a, out_b = (_rows16(t) for t in (out_a, out_b))
        lse_a, lse_b = (_unit_rows(t) for t in (lse_a, lse_b))
        out = torch.empty(out_a.shape, dtype=out_a.dtype, device=out_a.device)
        lse = torch.empty(lse_a.shape, dtype=torch.float32, device=out_a.device)
        a = _C.MergePairArgs()
        a.out_a, a.out_b, a.out = _ptr(out_a), _ptr(out_b), _ptr(out)
        a.out_a_st, a.out_b_st, a.out_st = _st3(out_a, varlen), _st3(out_b, varlen), _st3(out, varlen)
        a.lse_a, a.lse_b, a.lse = _ptr(lse_a), _ptr(lse_b), _ptr(lse)
        a.lse_a_batch, a.lse_a_head = _lse_st(lse_a, varlen)
        a.lse_b_batch, a.lse_b_head = _lse_st(lse_b, varlen)
        a.lse_batch, a.lse_head = _lse_st(lse, varlen)
        a.B, (a.S, a.H, a.D) = (1, out.shape) if varlen else (out.shape[0], out.shape[1:])
        a.dtype = self._dtype(out)
        _C.check(self.lib.rfa_merge_pair(C.byref(a), _stream(out)), "rfa_merge_pair")
        return out, lse

    def merge_pair_bwd(self, dout, dlse, out_a, lse_a, out_b, lse_b):
        """(dout_a, dlse_a, dout_b, dlse_b) of merge_pair from the gradients of its outputs and its four inputs (include/rfa.h:
        rfa_merge_pair_bwd); dlse None: zero.  Summed in a fixed order: the same bits on every run."""
        self._check_dev(dout, dlse, out_a, lse_a, out_b, lse_b)
        varlen = out_a.dim() == 3
        dout, out_a, out_b = (_rows16(t) for t in (dout, out_a, out_b))
        lse_a, lse_b = (_unit_rows(t) for t in (lse_a, lse_b))
        dlse = None if dlse is None else _unit_rows(dlse)
        dout_a, dout_b = torch.empty_like(dout, memory_format=torch.contiguous_format), torch.empty_like(dout, memory_format=torch.contiguous_format)
        dlse_a = torch.empty(lse_a.shape, dtype=torch.float32, device=dout.device)
        dlse_b = torch.empty(lse_a.shape, dtype=torch.float32, device=dout.device)
        a = _C.MergePairBwdArgs()
        a.dout, a.dout_st = _ptr(dout), _st3(dout, varlen)
        if dlse is not None:
            a.dlse = _ptr(dlse)
            a.dlse_batch, a.dlse_head = _lse_st(dlse, varlen)
        a.out_a, a.out_b = _ptr(out_a), _ptr(out_b)
        a.out_a_st, a.out_b_st = _st3(out_a, varlen), _st3(out_b, varlen)
        a.lse_a, a.lse_b = _ptr(lse_a), _ptr(lse_b)
        a.lse_a_batch, a.lse_a_head = _lse_st(lse_a, varlen)
        a.lse_b_batch, a.lse_b_head = _lse_st(lse_b, varlen)
        a.dout_a, a.dout_b = _ptr(dout_a), _ptr(dout_b)
        a.dout_a_st, a.dout_b_st = _st3(dout_a, varlen), _st3(dout_b, varlen)
        a.dlse_a, a.dlse_b = _ptr(dlse_a), _ptr(dlse_b)
        a.dlse_a_batch, a.dlse_a_head = _lse_st(dlse_a, varlen)
        a.dlse_b_batch, a.dlse_b_head = _lse_st(dlse_b, varlen)
        a.B, (a.S, a.H, a.D) = (1, dout.shape) if varlen else (dout.shape[0], dout.shape[1:])
        a.dtype = self._dtype(dout)
        _C.check(self.lib.rfa_merge_pair_bwd(C.byref(a), _stream(dout)), "rfa_merge_pair_bwd")
        return dout_a, dlse_a, dout_b, dlse_b

    # ------------------------------------------------------------------ attention sinks
    def sink_apply(self, out, lse, sinks, *, varlen, inplace=False):
        """(out', lse') of the attention with one sink logit per query head, from the merged (out, lse) of the attention
        without it: lse' = logaddexp(lse, sinks[h]), out' = out * exp(lse - lse') (include/rfa.h: rfa_sink_apply).
        out (B,S,H,D) with lse (B,H,S), or varlen: (T,H,D) with (H,T); sinks (H,), any floating dtype.  New tensors unless
        `inplace` (then `out` and `lse` are overwritten and returned)."""
        self._check_dev(out, lse, sinks)
        if lse.stride(-1) != 1 and lse.shape[-1] != 1:
            lse, inplace_lse = lse.contiguous(), True
        else:
            inplace_lse = inplace
        out_dst = out if inplace else torch.empty_like(out)
        lse_dst = lse if inplace_lse else torch.empty_like(lse)
        s32 = _sinks_f32(sinks, out)
        a = _C.SinkApplyArgs()
        a.out_src, a.out_src_st = _ptr(out), _st3(out, varlen)
        a.out_dst, a.out_dst_st = _ptr(out_dst), _st3(out_dst, varlen)
        a.lse_src, a.lse_dst = _ptr(lse), _ptr(lse_dst)
        a.lse_src_batch, a.lse_src_head = _lse_st(lse, varlen)
        a.lse_dst_batch, a.lse_dst_head = _lse_st(lse_dst, varlen)
        a.sinks = _ptr(s32)
        a.B, (a.S, a.H, a.D) = (1, out.shape) if varlen else (out.shape[0], out.shape[1:])
        a.dtype = self._dtype(out)
        _C.check(self.lib.rfa_sink_apply(C.byref(a), _stream(out)), "rfa_sink_apply")
        return out_dst, lse_dst

    def sink_grad(self, dout, out, lse, sinks, *, varlen):
        """(H,) fp32: dsink[h] = - sum over rows of exp(sinks[h] - lse') * rowsum(dout * out'), with the (out', lse') that
        sink_apply returned (include/rfa.h: rfa_sink_grad) — summed in a fixed order, the same bits on every run.  dout may
        be any strided view whose rows stay 16-byte aligned (anything else is copied)."""
        self._check_dev(dout, out, lse, sinks)
        dout = _rows16(dout)
        if lse.stride(-1) != 1 and lse.shape[-1] != 1:
            lse = lse.contiguous()
        s32 = _sinks_f32(sinks, out)
        dsink = torch.empty(s32.shape, dtype=torch.float32, device=out.device)
        a = _C.SinkGradArgs()
        a.dout, a.dout_st = _ptr(dout), _st3(dout, varlen)
        a.out, a.out_st = _ptr(out), _st3(out, varlen)
        a.lse = _ptr(lse)
        a.lse_batch, a.lse_head = _lse_st(lse, varlen)
        a.sinks, a.dsink = _ptr(s32), _ptr(dsink)
        a.B, (a.S, a.H, a.D) = (1, out.shape) if varlen else (out.shape[0], out.shape[1:])
        a.dtype = self._dtype(out)
        nbytes = self.lib.rfa_sink_grad_workspace_bytes(C.byref(a))
        if nbytes:
            ws = self._sink_scratch(nbytes, out.device)
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        _C.check(self.lib.rfa_sink_grad(C.byref(a), _stream(out)), "rfa_sink_grad")
        return dsink

    def _sink_scratch(self, nbytes, device):
        """the partial sums of sink_grad: ONE reusable buffer per (device, stream) in the scratch pool (kernels of one stream
        run in order, so the next call cannot overwrite partials that are still to be read); release_scratch() drops it"""
        key = ("sink", device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream)
        buf = self._ds_pool.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._ds_pool[key] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
        return buf

    # ------------------------------------------------------------------ per-head max attention logit (with_max_logit)
    def max_logit(self, q, k, dst, *, softmax_scale, causal, cu_seqlens_q=None, cu_seqlens_k=None, max_seqlen_q=None,
                  max_seqlen_k=None, q_half=HALF_FULL, k_half=HALF_FULL, window=(-1, -1), mask_shift=0, mask_shift_lens=0,
                  accumulate=True, head0=0):
        """dst[head0 + h] = max(dst[head0 + h], m_h) (accumulate) or m_h, for the H query heads of q: m_h = the largest
        softmax_scale * q.k over the (query row, key) pairs the block call `fwd(q, k, ...)` with the same geometry keywords
        looks at, -inf when it looks at none (include/rfa.h: rfa_max_logit).  dst: fp32, contiguous, 1-d, on q's device.  The
        raw scaled dot product: a soft cap, a bias, dropout and sinks do not enter it.  Same bits on every run."""
        self._check_dev(q, k, dst)
        q, k = _in_contract(q), _in_contract(k)
        varlen = cu_seqlens_q is not None
        a = _C.MaxLogitArgs()
        a.q, a.k = _ptr(q), _ptr(k)
        a.q_st, a.k_st = _st3(q, varlen), _st3(k, varlen)
        if varlen:
            a.cu_seqlens_q, a.cu_seqlens_k = _ptr(cu_seqlens_q), _ptr(cu_seqlens_k)
            a.B = cu_seqlens_q.numel() - 1
            a.H, a.D = q.shape[1], q.shape[2]
            a.Hk = k.shape[1]
            a.Sq, a.Sk = int(max_seqlen_q), int(max_seqlen_k)
            a.total_q = q.shape[0]
        else:
            a.B, a.Sq, a.H, a.D = q.shape
            a.Sk, a.Hk = k.shape[1], k.shape[2]
        head0 = int(head0)
        if (dst.dtype != torch.float32 or dst.dim() != 1 or not dst.is_contiguous() or dst.device != q.device
                or head0 < 0 or head0 + a.H > dst.numel()):
            raise ValueError(f"ring_flash_attn: max_logit needs a contiguous float32 (H,) tensor on {q.device} with room for "
                             f"heads [{head0}, {head0 + a.H}); got {tuple(dst.shape)} {dst.dtype} on {dst.device}")
        a.q_half, a.k_half = q_half, k_half
        a.softmax_scale = float(softmax_scale)
        a.causal = 1 if causal else 0
        if window is not None and (window[0] >= 0 or window[1] >= 0):
            a.window, a.window_left, a.window_right = 1, int(window[0]), int(window[1])
        a.mask_shift = int(mask_shift)
        a.mask_shift_lens = int(mask_shift_lens)
        a.dtype = self._dtype(q)
        a.accumulate = 1 if accumulate else 0
        a.max_logit = dst.data_ptr() + 4 * head0
        nbytes = self.lib.rfa_max_logit_workspace_bytes(C.byref(a))
        if nbytes:
            ws = self._max_logit_scratch(nbytes, q.device)
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        _C.check(self.lib.rfa_max_logit(C.byref(a), _stream(q)), "rfa_max_logit")

    def _max_logit_scratch(self, nbytes, device):
        """the per-workgroup partials of max_logit: ONE reusable buffer per (device, stream) in the scratch pool, kept like
        _sink_scratch (kernels of one stream run in order); release_scratch() drops it"""
        key = ("maxlogit", device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream)
        buf = self._ds_pool.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._ds_pool[key] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
        return buf

    # ------------------------------------------------------------------ sequence/head exchange (with_ulysses)
    def seq_head_copy(self, op, layout, U, tensors, slots):
        """one launch of the layout change on either side of the Ulysses all-to-all (include/rfa.h: rfa_seq_head_copy) for
        up to three tensors.  op / layout: _C.SEQHEAD_*.  tensors: the LOCAL views (B,S,[P,]H,D) for PACK (read) and
        SLOTS_TO_HEADS (written), the MERGED views (B,U*S,[P,]H/U,D) for UNPACK (written) and MERGED_TO_SLOTS (read); any
        strides with last stride 1 and 16-byte aligned rows.  slots: the contiguous all-to-all buffer, U slots of
        [tensor 0 | tensor 1 | ...], same dtype."""
        self._check_dev(slots, *tensors)
        local = op in (_C.SEQHEAD_PACK, _C.SEQHEAD_SLOTS_TO_HEADS)
        a = _C.SeqHeadArgs()
        a.op, a.layout, a.U = op, layout, U
        t0 = tensors[0]
        a.B, a.S, a.D = t0.shape[0], t0.shape[1] if local else t0.shape[1] // U, t0.shape[-1]
        a.elem_bytes, a.ntensors = t0.element_size(), len(tensors)
        for d, t in zip(a.t, tensors):
            if t.dtype != slots.dtype or t.stride(-1) != 1:
                raise ValueError("seq_head_copy: tensors and slots share one dtype; last (head_dim) stride must be 1")
            d.ptr = t.data_ptr()
            # (the stride of a dimension of length 1 is never used: 0, whatever torch reports for it)
            st = [s_ if n > 1 else 0 for n, s_ in zip(t.shape, t.stride())]
            d.batch, d.row, d.head = st[0], st[1], st[-2]
            d.P, d.part = (t.shape[2], st[2]) if t.dim() == 5 else (1, 0)
            d.H = t.shape[-2] if local else t.shape[-2] * U
        a.slots, a.slots_elems = slots.data_ptr(), slots.numel()
        if not slots.is_contiguous():
            raise ValueError("seq_head_copy: the slot buffer must be contiguous")
        _C.check(self.lib.rfa_seq_head_copy(C.byref(a), _stream(slots)), "rfa_seq_head_copy")

    # ------------------------------------------------------------------ rotary embedding (apply_rotary)
    def rotary(self, srcs, dsts, cos, sin, *, positions=None, pos_map=None, interleaved=False, rot_offset=0, conj=False):
        """one launch of the rotary embedding (include/rfa.h: rfa_rotary) for one or two tensors that share rows and positions.
        srcs / dsts: (B,S,H,D) or packed (T,H,D), io dtype, any strides with last stride 1 and 16-byte aligned rows; dsts[k] is
        srcs[k] for in place.  cos / sin: (P, R/2) contiguous, fp32 or the io dtype.  positions: int32 (S,) / (B,S) / (T,),
        row stride 1, to which pos_map's offset is added — or None: the rows sit at pos_map = (offset, (stride, split,
        offset2)) (_common.pos_map).  conj: the inverse rotation (the backward)."""
        self._check_dev(cos, sin, positions, *srcs, *dsts)
        t0 = srcs[0]
        packed = t0.dim() == 3
        a = _C.RotaryArgs()
        a.ntensors = len(srcs)
        a.B, a.S = (1, t0.shape[0]) if packed else (t0.shape[0], t0.shape[1])
        a.D, a.dtype = t0.shape[-1], self._dtype(t0)
        a.R, a.rot_offset = 2 * cos.shape[1], int(rot_offset)
        a.interleaved, a.conj = int(bool(interleaved)), int(bool(conj))
        a.table_dtype = _C.ROTARY_TABLE_F32 if cos.dtype == torch.float32 else self._dtype(cos)
        if not cos.is_contiguous() or not sin.is_contiguous() or cos.shape != sin.shape or cos.dtype != sin.dtype:
            raise ValueError("rotary: cos and sin are contiguous (P, R/2) tensors of one shape and dtype")
        for d, s, o in zip(a.t, srcs, dsts):
            if s.dtype != t0.dtype or o.dtype != t0.dtype or s.shape != o.shape or s.stride(-1) != 1 or o.stride(-1) != 1:
                raise ValueError("rotary: sources and destinations share one dtype and shape; last (head_dim) stride must be 1")
            d.src, d.dst, d.H = s.data_ptr(), o.data_ptr(), s.shape[-2]
            # (the stride of a dimension of length 1 is never used: 0, whatever torch reports for it)
            ss, os_ = ([st if n > 1 else 0 for n, st in zip(t.shape, t.stride())] for t in (s, o))
            d.src_batch, d.src_row, d.src_head = (0 if packed else ss[0]), ss[-3], ss[-2]
            d.dst_batch, d.dst_row, d.dst_head = (0 if packed else os_[0]), os_[-3], os_[-2]
        a.cos, a.sin, a.P = cos.data_ptr(), sin.data_ptr(), cos.shape[0]
        off, (stride, split, off2) = pos_map if pos_map is not None else (0, (1, 0, 0))
        a.pos_offset = int(off)
        if positions is not None:
            if positions.dtype != torch.int32 or (positions.stride(-1) != 1 and positions.shape[-1] != 1):
                raise ValueError("rotary: positions are int32 with row stride 1")
            a.positions = positions.data_ptr()
            a.pos_batch = positions.stride(0) if positions.dim() == 2 and positions.shape[0] > 1 else 0
        else:
            a.pos_stride, a.pos_split, a.pos_offset2 = int(stride), int(split), int(off2)
        _C.check(self.lib.rfa_rotary(C.byref(a), _stream(t0)), "rfa_rotary")

    # ------------------------------------------------------------------ QK RMSNorm + rotary (apply_qk_norm_rotary)
    def _qk_norm_args(self, a, xs, outs, weights, cos, sin, positions, pos_map, interleaved, rot_offset, eps, weight_offset):
        """the fields rfa_qk_norm_rotary_args and rfa_qk_norm_rotary_bwd_args share"""
        self._check_dev(cos, sin, positions, *xs, *outs, *weights)
        t0 = xs[0]
        packed = t0.dim() == 3
        a.ntensors = len(xs)
        a.B, a.S = (1, t0.shape[0]) if packed else (t0.shape[0], t0.shape[1])
        a.D, a.dtype = t0.shape[-1], self._dtype(t0)
        a.rot_offset, a.interleaved = int(rot_offset), int(bool(interleaved))
        a.eps, a.weight_offset = float(eps), float(weight_offset)
        if (cos is None) != (sin is None):
            raise ValueError("qk_norm_rotary: cos and sin come together (both None: the norm alone)")
        if cos is not None:
            if not cos.is_contiguous() or not sin.is_contiguous() or cos.shape != sin.shape or cos.dtype != sin.dtype:
                raise ValueError("qk_norm_rotary: cos and sin are contiguous (P, R/2) tensors of one shape and dtype")
            a.R, a.P = 2 * cos.shape[1], cos.shape[0]
            a.cos, a.sin = cos.data_ptr(), sin.data_ptr()
            a.table_dtype = _C.ROTARY_TABLE_F32 if cos.dtype == torch.float32 else self._dtype(cos)
        else:
            a.table_dtype = a.dtype
        w0 = weights[0]
        a.weight_dtype = _C.QK_NORM_WEIGHT_F32 if w0.dtype == torch.float32 else self._dtype(w0)
        for k, (d, s, o, w) in enumerate(zip(a.t, xs, outs, weights)):
            if s.dtype != t0.dtype or o.dtype != t0.dtype or s.shape != o.shape or s.stride(-1) != 1 or o.stride(-1) != 1:
                raise ValueError("qk_norm_rotary: inputs and outputs share one dtype and shape; last (head_dim) stride must be 1")
            if w.dtype != w0.dtype or tuple(w.shape) != (a.D,) or not w.is_contiguous():
                raise ValueError("qk_norm_rotary: the weights are contiguous (D,) tensors of one dtype")
            d.src, d.dst, d.H = s.data_ptr(), o.data_ptr(), s.shape[-2]
            a.weight[k] = w.data_ptr()
            ss, os_ = ([st if n > 1 else 0 for n, st in zip(t.shape, t.stride())] for t in (s, o))
            d.src_batch, d.src_row, d.src_head = (0 if packed else ss[0]), ss[-3], ss[-2]
            d.dst_batch, d.dst_row, d.dst_head = (0 if packed else os_[0]), os_[-3], os_[-2]
        off, (stride, split, off2) = pos_map if pos_map is not None else (0, (1, 0, 0))
        a.pos_offset = int(off)
        if positions is not None:
            if positions.dtype != torch.int32 or (positions.stride(-1) != 1 and positions.shape[-1] != 1):
                raise ValueError("qk_norm_rotary: positions are int32 with row stride 1")
            a.positions = positions.data_ptr()
            a.pos_batch = positions.stride(0) if positions.dim() == 2 and positions.shape[0] > 1 else 0
        else:
            a.pos_stride, a.pos_split, a.pos_offset2 = int(stride), int(split), int(off2)
        return packed

    def qk_norm_rotary_fwd(self, xs, outs, weights, cos, sin, *, positions=None, pos_map=None, interleaved=False, rot_offset=0,
                           eps=1e-6, weight_offset=0.0):
        """one launch of the per-head RMSNorm + rotary (include/rfa.h: rfa_qk_norm_rotary_fwd) for one or two tensors that share
        rows and positions: outs[k] = rope((xs[k] rstd) (weight_offset + weights[k])).  xs / outs as in `rotary` (out of place);
        weights: (D,) contiguous, fp32 or the io dtype; cos = sin = None: the norm alone."""
        a = _C.QkNormRotaryArgs()
        self._qk_norm_args(a, xs, outs, weights, cos, sin, positions, pos_map, interleaved, rot_offset, eps, weight_offset)
        _C.check(self.lib.rfa_qk_norm_rotary_fwd(C.byref(a), _stream(xs[0])), "rfa_qk_norm_rotary_fwd")

    def qk_norm_rotary_bwd(self, xs, douts, dxs, weights, dweights, cos, sin, *, positions=None, pos_map=None, interleaved=False,
                           rot_offset=0, eps=1e-6, weight_offset=0.0):
        """the backward (include/rfa.h: rfa_qk_norm_rotary_bwd): dxs[k] from xs[k] and douts[k] in one launch; dweights[k] an
        fp32 (D,) tensor that is overwritten with this call's weight gradient, or None.  The workspace is allocated here."""
        a = _C.QkNormRotaryBwdArgs()
        packed = self._qk_norm_args(a, xs, dxs, weights, cos, sin, positions, pos_map, interleaved, rot_offset, eps, weight_offset)
        self._check_dev(*douts, *[d for d in dweights if d is not None])
        for k, (g, x, dw) in enumerate(zip(douts, xs, dweights)):
            if g.dtype != x.dtype or g.shape != x.shape or g.stride(-1) != 1:
                raise ValueError("qk_norm_rotary: a gradient has its tensor's dtype and shape; last (head_dim) stride must be 1")
            gs = [st if n > 1 else 0 for n, st in zip(g.shape, g.stride())]
            a.g[k].dout = g.data_ptr()
            a.g[k].dout_batch, a.g[k].dout_row, a.g[k].dout_head = (0 if packed else gs[0]), gs[-3], gs[-2]
            if dw is not None:
                if dw.dtype != torch.float32 or tuple(dw.shape) != (a.D,) or not dw.is_contiguous():
                    raise ValueError("qk_norm_rotary: dweight is a contiguous fp32 (D,) tensor")
                a.dweight[k] = dw.data_ptr()
        ws = None
        if any(d is not None for d in dweights):
            need = int(self.lib.rfa_qk_norm_rotary_bwd_workspace_bytes(C.byref(a)))
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=xs[0].device)
            a.workspace, a.workspace_bytes = ws.data_ptr(), need
        _C.check(self.lib.rfa_qk_norm_rotary_bwd(C.byref(a), _stream(xs[0])), "rfa_qk_norm_rotary_bwd")
        if a.B == 0 or a.S == 0:                                   # (nothing was launched: an empty sum)
            for dw in dweights:
                if dw is not None:
                    dw.zero_()

    def sum_slots(self, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        """dst[...] = sum over dim 0 of src (io dtype, summed in fp32).  src: (W, B, S, H, D) or (W, T, H, D), each slot
        laid out like dst up to strides; dst may be a strided view (a slice of a packed gradient)."""
        self._check_dev(src, dst)
        varlen = dst.dim() == 3
        a = _C.SumSlotsArgs()
        a.src, a.dst = _ptr(src), _ptr(dst)
        a.nslots, a.slot_stride = src.shape[0], src.stride(0)
        a.src_st, a.dst_st = _st3(src[0], varlen), _st3(dst, varlen)
        if varlen:
            a.B, (a.S, a.H, a.D) = 1, dst.shape
        else:
            a.B, a.S, a.H, a.D = dst.shape
        a.dtype = self._dtype(dst)
        _C.check(self.lib.rfa_sum_slots(C.byref(a), _stream(dst)), "rfa_sum_slots")
        return dst

    def cast(self, src: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """fp32 accumulator -> io dtype (new contiguous tensor)."""
        self._check_dev(src)
        if not src.is_contiguous():
            src = src.contiguous()
        dst = torch.empty(src.shape, dtype=dtype, device=src.device)
        _C.check(self.lib.rfa_cast(dst.data_ptr(), src.data_ptr(), src.numel(), _DTYPES[dtype], _stream(src)),
                 "rfa_cast")
        return dst

    def lse_flatten(self, lse_padded, cu_seqlens):
        """(B,H,max_seqlen) -> (H,T)   (triton_utils.flatten_varlen_lse)."""
        self._check_dev(lse_padded, cu_seqlens)
        B, H, M = lse_padded.shape
        T = int(cu_seqlens[-1].item())
        src = lse_padded.contiguous()
        dst = torch.empty((H, T), dtype=torch.float32, device=src.device)
        _C.check(self.lib.rfa_lse_flatten(dst.data_ptr(), src.data_ptr(), cu_seqlens.data_ptr(), B, H, M,
                                          dst.stride(0), dst.stride(1), _stream(src)), "rfa_lse_flatten")
        return dst

    def lse_unflatten(self, lse_packed, cu_seqlens, max_seqlen):
        """(T,H,1)/(T,H) -> (B,H,max_seqlen)   (triton_utils.unflatten_varlen_lse)."""
        self._check_dev(lse_packed, cu_seqlens)
        if lse_packed.dim() == 3:
            lse_packed = lse_packed.squeeze(-1)
        T, H = lse_packed.shape
        B = cu_seqlens.numel() - 1
        dst = torch.empty((B, H, max_seqlen), dtype=torch.float32, device=lse_packed.device)
        _C.check(self.lib.rfa_lse_unflatten(dst.data_ptr(), lse_packed.data_ptr(), cu_seqlens.data_ptr(), B, H,
                                            int(max_seqlen), lse_packed.stride(1), lse_packed.stride(0),
                                            _stream(lse_packed)), "rfa_lse_unflatten")
        return dst


def _set_dropout(a, dropout):
    """dropout = (p, seed, q_pos_offset, k_pos_offset, head_offset) or None (include/rfa.h: rfa_fwd_args.dropout_p), or
    the 7-tuple that adds the position maps (q_map, k_map) of tensors whose rows are not one contiguous run of the
    sequence: each (stride, split, offset2) — include/rfa.h: q_pos_stride ... (_common.dropout_arg builds both)"""
    if dropout is None or not dropout[0] > 0:
        return
    p, seed, q0, k0, h0 = dropout[:5]
    a.dropout_p, a.dropout_seed = float(p), int(seed) & 0xFFFFFFFFFFFFFFFF
    a.q_pos_offset, a.k_pos_offset, a.head_offset = int(q0), int(k0), int(h0)
    if len(dropout) > 5:
        (a.q_pos_stride, a.q_pos_split, a.q_pos_offset2), (a.k_pos_stride, a.k_pos_split, a.k_pos_offset2) = (
            tuple(int(x) for x in m) for m in dropout[5:7])


def _sinks_f32(sinks, like):
    """the sinks as the kernels read them: (H,) fp32, contiguous, on `like`'s device (a copy only when they are not)"""
    if sinks.dim() != 1 or sinks.shape[0] != like.shape[-2] or sinks.device != like.device or not sinks.is_floating_point():
        raise ValueError(f"ring_flash_attn: sinks must be a floating tensor of shape ({like.shape[-2]},) on {like.device}; "
                         f"got {tuple(sinks.shape)} {sinks.dtype} on {sinks.device}")
    return sinks.detach().to(torch.float32).contiguous()


def _ext_args(alibi, q, softcap=0.0):
    """rfa_ext_args of a call with `alibi=(slopes, shift)` and / or `softcap`, or None: the call without the extension"""
    softcap = check_softcap(softcap)
    if alibi is None or alibi[0] is None:
        if not softcap:
            return None
        ext = _C.ExtArgs()
        ext.softcap = softcap
        return ext
    slopes, shift = alibi
    if slopes.dtype != torch.float32 or slopes.device != q.device or slopes.dim() not in (1, 2) or slopes.stride(-1) != 1:
        raise ValueError("alibi slopes must be a float32 tensor of shape (H,) or (B, H), innermost stride 1, on q's device")
    ext = _C.ExtArgs()
    ext.alibi_slopes = slopes.data_ptr()
    ext.alibi_batch_stride = slopes.stride(0) if slopes.dim() == 2 else 0
    ext.alibi_shift = int(shift)
    ext.softcap = softcap
    return ext


def _rowrange_args(row_ranges, q, alibi, softcap, dropout, vd, varlen):
    """rfa_rowrange_args of a call with `row_ranges=(start, end, k_pos0)`, or None: the call without them.  What the ranged
    kernels do not have is refused here, before the library is called."""
    if row_ranges is None:
        return None
    start, end, k_pos0 = row_ranges
    if (alibi is not None and alibi[0] is not None) or check_softcap(softcap) or (dropout is not None and dropout[0] > 0):
        raise NotImplementedError("ring_flash_attn: row ranges together with alibi, softcap or dropout are not served")
    if vd is not None or varlen or q.shape[-1] > 128:
        raise NotImplementedError("ring_flash_attn: row ranges are served for dense input with one head dim up to 128")
    want = tuple(q.shape[:2])
    for nm, t in (("start", start), ("end", end)):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != want or t.device != q.device
                or (t.stride(1) != 1 and t.shape[1] != 1)):
            raise ValueError(f"row_ranges: {nm} must be an int32 tensor of shape {want} on {q.device} with row stride 1")
    if start.stride(0) != end.stride(0) and start.shape[0] > 1:
        end = end.contiguous()
        start = start.contiguous()
    rr = _C.RowRangeArgs()
    rr.start, rr.end = start.data_ptr(), end.data_ptr()
    rr.batch_stride = start.stride(0) if start.shape[0] > 1 else 0
    rr.k_pos0 = int(k_pos0)
    rr._keep = (start, end)                       # (the tensors live as long as the struct does)
    return rr


def _blockmask_args(block_mask, q, alibi, softcap, dropout, vd, varlen, rr=None):
    """rfa_blockmask_args of a call with `block_mask=(mask_view, k_blk0)`, or None: the call without one.  What the masked
    kernels do not have is refused here, before the library is called.  Strides of broadcast dims are 0."""
    if block_mask is None:
        return None
    mask, k_blk0 = block_mask
    if (alibi is not None and alibi[0] is not None) or check_softcap(softcap) or (dropout is not None and dropout[0] > 0):
        raise NotImplementedError("ring_flash_attn: a block mask together with alibi, softcap or dropout is not served")
    if rr is not None:
        raise NotImplementedError("ring_flash_attn: a block mask together with row ranges is not served")
    if vd is not None or varlen or q.shape[-1] > 128:
        raise NotImplementedError("ring_flash_attn: block masks are served for dense input with one head dim up to 128")
    B, Sq, H = q.shape[0], q.shape[1], q.shape[2]
    nq = (Sq + _C.BLOCK_MASK_SIZE - 1) // _C.BLOCK_MASK_SIZE
    if (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 4
            or mask.device != q.device or mask.shape[0] not in (1, B) or mask.shape[1] not in (1, H) or mask.shape[2] != nq
            or (mask.shape[3] > 1 and mask.stride(3) != 1)):
        got = f"{tuple(mask.shape)} {mask.dtype} on {mask.device}" if isinstance(mask, torch.Tensor) else repr(mask)
        raise ValueError(f"block_mask: the mask must be a bool / uint8 tensor of shape ({{1, {B}}}, {{1, {H}}}, {nq}, NK) on "
                         f"{q.device} with column stride 1; got {got}")
    bm = _C.BlockMaskArgs()
    bm.mask = mask.data_ptr()                     # (bool and uint8 are both one byte per element, non-zero = True)
    bm.batch_stride = mask.stride(0) if mask.shape[0] > 1 else 0
    bm.head_stride = mask.stride(1) if mask.shape[1] > 1 else 0
    bm.row_stride = mask.stride(2) if mask.shape[2] > 1 else 0
    bm.nk_blocks = mask.shape[3]
    bm.k_blk0 = int(k_blk0)
    bm._keep = mask                               # (the tensor lives as long as the struct does)
    return bm


def _vdim_args(q, v, alibi, softcap, dropout):
    """rfa_vdim_args of a call whose `v` has a head dim of its own, or None: equal widths — the call as it always was.
    What the kernels of such a call do not have (a bias, a soft cap, dropout) is refused here, before the library is called."""
    if v.shape[-1] == q.shape[-1]:
        return None
    if (alibi is not None and alibi[0] is not None) or check_softcap(softcap):
        raise NotImplementedError("ring_flash_attn: alibi / softcap with a value head dim that differs from q's is not served "
                                  "(both stop at head dim 128)")
    if dropout is not None and dropout[0] > 0:
        raise NotImplementedError("ring_flash_attn: dropout with a value head dim that differs from q's is not served")
    vd = _C.VdimArgs()
    vd.head_dim_v = v.shape[-1]
    return vd


def check_softcap(softcap):
    """flash_attn's softcap as a float: None and 0 are off (0.0); a negative or non-finite value is a ValueError"""
    import math

    cap = 0.0 if softcap is None else float(softcap)
    if not math.isfinite(cap) or cap < 0.0:
        raise ValueError(f"ring_flash_attn: softcap must be a finite number >= 0 (0: off); got {softcap!r}")
    return cap


_FWD_FORMS = {"auto": _C.FWD_AUTO, "8x32": _C.FWD_8x32, "4x32": _C.FWD_4x32, "p8x32": _C.FWD_P8x32}


def _fwd_form() -> int:
    """config.fwd_form (RFA_FWD_FORM = 8x32 | 4x32, tuning / tests); auto: the library's choice"""
    return _FWD_FORMS[config.get().fwd_form]


def _spill_enabled() -> bool:
    return config.get().bwd_ds_spill


def _spill_limit() -> int:
    return config.get().ds_spill_max_bytes


def _spill_frac() -> float:
    return config.get().ds_spill_max_frac


def _plan_overrides():
    """(dkdv_form, dkdv_nsplit) from the tuning / test switches config.dkdv_wide (RFA_DKDV_WIDE=0|1|2; 2 = the balanced causal schedule) and
    config.dkdv_nsplit (RFA_DKDV_NSPLIT=n; n > 0 also forces the 256-key form); (AUTO, 0) when unset"""
    c = config.get()
    form = _C.DKDV_AUTO
    if c.dkdv_wide == 0:
        form = _C.DKDV_128
    elif c.dkdv_wide == 2 and c.dkdv_nsplit <= 0:
        form = _C.DKDV_BAL               # (the balanced causal schedule where the call is eligible, else the library's choice)
    elif c.dkdv_nsplit > 0 or c.dkdv_wide >= 1:
        form = _C.DKDV_256               # (forced: the C plan takes form == 256 as given; nsplit 0 = its own choice)
    return form, c.dkdv_nsplit


_SPILL_CHECK_ABOVE = 256 << 20      # bytes: scratch requests up to this size are simply attempted
_SPILL_GROW_RETRY = 64               # backwards between two attempts to grow a scratch that free memory had capped

_LOGGED = set()


def _log_once(key, msg):
    if key not in _LOGGED:
        _LOGGED.add(key)
        import sys
        sys.stderr.write(msg + "\n")


_backend = None


def get_backend():
    """the operator backend of this process: the HIP library (raises if librfa_hip.so is missing — there is no CPU
    path).  Tests and bench.py's in-step timer replace it through ring_flash_attn._testing.set_backend.
    Inside `softcap_scope(cap)` with cap > 0 — the forward or the backward of ONE capped autograd node — the backend comes
    wrapped so that every block call carries `softcap=cap`.  Inside a call bound by `with_max_logit` it comes wrapped — outside
    a cap wrapper — so that every forward block call is followed by the backend's `max_logit` of the same block."""
    global _backend
    if _backend is None:
        _backend = HipBackend()
    cap = _softcap.get()
    be = _CappedBackend(_backend, cap) if cap else _backend
    dst = _max_logit.get()
    return be if dst is None else _MaxLogitBackend(be, dst)


# ---- logit soft-capping (ring_flash_attn.with_softcap) ------------------------------------------------------------------
# The cap is a pointwise function of one score: unlike a window, dropout or a bias it needs nothing about where a block sits,
# so no schedule computes anything for it — every block call of a capped forward or backward simply carries the one value.
# That is done HERE, once, instead of at each of the schedules' call sites: a schedule asks get_backend() for its backend at
# the start of its forward and of its backward, and gets this wrapper while its autograd node runs under softcap_scope.  The
# scope is private and is entered by the autograd Functions only (forward: the value with_softcap bound to the call;
# backward: the value kept on the node) — nothing ambient is read in a backward.
import contextvars

_softcap = contextvars.ContextVar("ring_flash_attn_softcap", default=0.0)


class softcap_scope:
    """`with softcap_scope(cap):` — block calls made inside carry softcap=cap (0: none; an enclosing scope is masked)"""

    def __init__(self, cap):
        self.cap = check_softcap(cap)

    def __enter__(self):
        self.token = _softcap.set(self.cap)
        return self

    def __exit__(self, *exc):
        _softcap.reset(self.token)
        return False


def pending_softcap():
    """the cap bound to the public call that is running (with_softcap), 0.0 without one"""
    return _softcap.get()


class _CappedBackend:
    """a backend whose fwd / bwd carry `softcap=`; everything else — attributes, scratch, the other operators — is the
    wrapped backend's own.  A backend that does not serve a cap is refused when the wrapper is made, i.e. before the
    schedule exchanges anything, on every rank alike."""

    def __init__(self, be, cap):
        if not getattr(be, "serves_softcap", False):
            raise NotImplementedError(f"ring_flash_attn: softcap needs a backend that serves `softcap`; "
                                      f"{getattr(be, 'name', type(be).__name__)!r} does not (it would ignore the cap)")
        object.__setattr__(self, "_be", be)
        object.__setattr__(self, "_cap", cap)

    def __getattr__(self, name):
        return getattr(self._be, name)

    def __setattr__(self, name, value):
        setattr(self._be, name, value)

    def fwd(self, *args, **kw):
        return self._be.fwd(*args, softcap=self._cap, **kw)

    def bwd(self, *args, **kw):
        return self._be.bwd(*args, softcap=self._cap, **kw)


# ---- per-head max attention logit (ring_flash_attn.with_max_logit) --------------------------------------------------------
# The largest softmax_scale * q.k over the pairs an attention looks at is the max over the block calls its schedule makes: every
# block call already names its q, its k and its visibility (causal, window, halves, packed lengths, where the block sits).  So
# no schedule computes anything for it either: inside a call bound by with_max_logit, get_backend() hands out this wrapper,
# which follows every `fwd` with the backend's `max_logit` of the same q, k and geometry keywords, max-accumulated into the
# caller's tensor.  No new keyword reaches a backend's fwd.  The scope is entered by with_max_logit's callable only, around the
# public call: a backward (which runs outside it) never touches the tensor, a checkpointed re-run accumulates the same values.
_max_logit = contextvars.ContextVar("ring_flash_attn_max_logit", default=None)

_MAX_LOGIT_GEOMETRY = ("softmax_scale", "causal", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "q_half",
                       "k_half", "window", "mask_shift", "mask_shift_lens")


class max_logit_scope:
    """`with max_logit_scope(t):` — forward block calls made inside max-accumulate their per-head max logit into t (None: none)"""

    def __init__(self, dst):
        self.dst = dst

    def __enter__(self):
        self.token = _max_logit.set(self.dst)
        return self

    def __exit__(self, *exc):
        _max_logit.reset(self.token)
        return False


def require_max_logit(what):
    """NotImplementedError unless the process's backend serves `max_logit` — asked at the public entry, before anything is
    exchanged, on every rank alike"""
    global _backend
    if _backend is None:
        _backend = HipBackend()
    if not getattr(_backend, "serves_max_logit", False):
        raise NotImplementedError(f"ring_flash_attn: {what} needs a backend that serves `max_logit`; "
                                  f"{getattr(_backend, 'name', type(_backend).__name__)!r} does not")


class _MaxLogitBackend:
    """a backend whose every `fwd` is followed by `max_logit` of the same block into dst[head0 : head0 + q's heads]; everything
    else is the wrapped backend's own (which may be a cap wrapper: the max is of the RAW logit and carries no cap)"""

    def __init__(self, be, dst, head0=0):
        object.__setattr__(self, "_be", be)
        object.__setattr__(self, "_dst", dst)
        object.__setattr__(self, "_head0", head0)

    def __getattr__(self, name):
        return getattr(self._be, name)

    def __setattr__(self, name, value):
        setattr(self._be, name, value)

    def fwd(self, q, k, v, **kw):
        res = self._be.fwd(q, k, v, **kw)
        self._be.max_logit(q, k, self._dst, accumulate=True, head0=self._head0,
                           **{n: kw[n] for n in _MAX_LOGIT_GEOMETRY if n in kw})
        return res

    def heads_from(self, head0):
        return _MaxLogitBackend(self._be, self._dst, head0)


def heads_from(be, head0):
    """the backend for block calls whose q is the slice of query heads that starts at `head0` (llama3's head groups): the
    max-logit wrapper then writes that slice of the caller's tensor; any other backend is returned as it is"""
    return be.heads_from(head0) if isinstance(be, _MaxLogitBackend) else be
