"""Basic ring attention over packed (varlen) sequences.

Same public surface and step semantics as
/root/reference/ring_flash_attn/ring_flash_attn_varlen.py (forward :25-100, backward :103-192,
autograd :195-265, wrappers :268-358).  Every packed sequence is sharded contiguously over the
ring, so the local `cu_seqlens` are identical for q and k at every step.  lse is produced
natively as (nheads, total) — the layout of flash_attn >= 2.7 — so the reference's
flatten/unflatten shims (triton_utils.py) are never needed on this path.

Sliding windows over several ranks (no counterpart in the reference): the K/V on hand at step d belong to rank
r - d, which holds the l_b rows in front of this rank's l_b rows of EVERY packed sequence b — d times the sequence's own
local length, a different number of rows for every sequence.  The kernels are told so in those units
(`mask_shift_lens`, include/rfa.h ABI 8) and band every sequence as its part of one window over its full length.
The exchange stays a full rotation: the host does not know the shortest sequence, so it cannot prove a hop dark for
all of them — the COMPUTE follows the window inside the kernels (dark sequences and tiles are skipped there), the
traffic does not.  A window that covers the whole of the longest sequence is dropped on the host and takes the
unwindowed path unchanged.
"""
import torch

from . import _C
from .backend import get_backend
from .utils import RingComm, single_rank
from ._common import alibi_kw, dlse_kw, out_shape, dropout_arg, global_window, require_mask_shift_lens
from ._api import ScheduleSpec, make_autograd_function, make_api, _grad_buffers


def _band(causal, win, step, rank, world):
    """band keywords of the block call of ring step `step`: unwindowed, only the diagonal block is masked; windowed, every
    block is told how many ranks (= local sequence lengths) its keys lie in front of its queries"""
    if win is None:
        return {"causal": causal and step == 0}
    t = step if step <= rank else step - world
    kw = {"causal": causal, "window": win}
    if t:
        kw["mask_shift_lens"] = t
    return kw


def ring_flash_attn_varlen_forward(
    process_group,
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens,
    max_seqlen,
    softmax_scale,
    dropout_p=0,
    causal=True,
    window_size=(-1, -1),
    alibi_slopes=None,
    deterministic=False,
    dropout_seed=None,
):
    be = get_backend()
    comm = RingComm(process_group)
    T, H, D = q.shape
    vl = dict(cu_seqlens_q=cu_seqlens, cu_seqlens_k=cu_seqlens, max_seqlen_q=max_seqlen, max_seqlen_k=max_seqlen)

    if single_rank(comm.world_size):
        out = torch.empty(out_shape(q, v), dtype=q.dtype, device=q.device)
        lse = torch.empty((H, T), dtype=torch.float32, device=q.device)
        be.fwd(q, k, v, softmax_scale=softmax_scale, causal=causal, out=out, lse=lse, window=window_size, dropout=dropout_arg(dropout_p, dropout_seed), **alibi_kw(alibi_slopes), **vl)
        return out, lse
    assert not dropout_p, "dropout over a multi-rank ring is not supported (as in the reference)"
    win = global_window(window_size, causal, comm.world_size * int(max_seqlen))
    if win is not None:
        require_mask_shift_lens(be, "ring_flash_attn_varlen")

    out_acc = torch.empty(out_shape(q, v), dtype=torch.float32, device=q.device)
    lse_acc = torch.empty((H, T), dtype=torch.float32, device=q.device)
    first = True
    next_k, next_v = None, None
    for step in range(comm.world_size):
        if step + 1 != comm.world_size:
            next_k, next_v = comm.send_recv_kv(k, v)
        if not causal or step <= comm.rank:
            be.fwd(q, k, v, softmax_scale=softmax_scale, out_acc=out_acc, lse_acc=lse_acc, acc_init=first,
                   **_band(causal, win, step, comm.rank, comm.world_size), **vl)
            first = False
        if step + 1 != comm.world_size:
            comm.wait()
            k, v = next_k, next_v

    return be.cast(out_acc, q.dtype), lse_acc


def ring_flash_attn_varlen_backward(
    process_group,
    dout,
    q,
    k,
    v,
    out,
    softmax_lse,
    cu_seqlens,
    max_seqlen,
    softmax_scale,
    dropout_p=0,
    causal=True,
    window_size=(-1, -1),
    alibi_slopes=None,
    deterministic=False,
    dropout_seed=None,
    out_grads=None,
    dlse=None,
):
    be = get_backend()
    kv_comm = RingComm(process_group)
    d_kv_comm = RingComm(process_group)
    T, H, D = q.shape
    vl = dict(cu_seqlens_q=cu_seqlens, cu_seqlens_k=cu_seqlens, max_seqlen_q=max_seqlen, max_seqlen_k=max_seqlen)
    if not softmax_lse.is_contiguous():
        softmax_lse = softmax_lse.contiguous()
    if dout.stride(-1) != 1:
        dout = dout.contiguous()

    delta = torch.empty((H, T), dtype=torch.float32, device=q.device)
    be.bwd_preprocess(dout, out, delta, cu_seqlens_q=cu_seqlens, max_seqlen_q=max_seqlen, **dlse_kw(dlse))

    if single_rank(kv_comm.world_size):
        dq, dk, dv = _grad_buffers(out_grads, q, k, v)
        be.bwd(dout, q, k, v, softmax_lse, delta, softmax_scale=softmax_scale, causal=causal,
               dq=dq, dk=dk, dv=dv, deterministic=deterministic, window=window_size, dropout=dropout_arg(dropout_p, dropout_seed), **alibi_kw(alibi_slopes), **vl)
        return dq, dk, dv
    assert not dropout_p, "dropout over a multi-rank ring is not supported (as in the reference)"
    win = global_window(window_size, causal, kv_comm.world_size * int(max_seqlen))
    if win is not None:
        require_mask_shift_lens(be, "ring_flash_attn_varlen")

    dq = None
    dk = torch.empty(k.shape, dtype=torch.float32, device=q.device)
    dv = torch.empty(v.shape, dtype=torch.float32, device=q.device)
    next_dk, next_dv = None, None
    next_k, next_v = None, None
    for step in range(kv_comm.world_size):
        if step + 1 != kv_comm.world_size:
            next_k, next_v = kv_comm.send_recv_kv(k, v)

        if step <= kv_comm.rank or not causal:
            common = dict(softmax_scale=softmax_scale, deterministic=deterministic,
                          **_band(causal, win, step, kv_comm.rank, kv_comm.world_size), **vl)
            if dq is None:
                dq = torch.empty((T, H, D), dtype=torch.float32, device=q.device)
                be.bwd(dout, q, k, v, softmax_lse, delta, dq_acc=dq, dk_acc=dk, dv_acc=dv, acc_init=True, **common)
            else:
                part = be.bwd(dout, q, k, v, softmax_lse, delta, dq_acc=dq, dk_acc=dk, dv_acc=dv,
                              phases=_C.BWD_COMPUTE, **common)
                d_kv_comm.wait()
                dk, dv = next_dk, next_dv
                be.bwd(dout, q, k, v, softmax_lse, delta, dq_acc=dq, dk_acc=dk, dv_acc=dv,
                       phases=_C.BWD_REDUCE, partials=part, **common)
        elif step != 0:
            d_kv_comm.wait()
            dk, dv = next_dk, next_dv

        if step + 1 != kv_comm.world_size:
            kv_comm.wait()
            k, v = next_k, next_v

        next_dk, next_dv = d_kv_comm.send_recv_kv(dk, dv)

    d_kv_comm.wait()

    return be.cast(dq, q.dtype), be.cast(next_dk, q.dtype), be.cast(next_dv, q.dtype)


SPEC = ScheduleSpec("RingFlashAttnVarlenFunc", "ring_flash_attn_varlen", n_lead=2, pack_dim=1, window_ring=True, vdim=True)
RingFlashAttnVarlenFunc = make_autograd_function(SPEC, ring_flash_attn_varlen_forward, ring_flash_attn_varlen_backward)
(
    ring_flash_attn_varlen_func,
    ring_flash_attn_varlen_kvpacked_func,
    ring_flash_attn_varlen_qkvpacked_func,
) = make_api(SPEC, RingFlashAttnVarlenFunc, ring_flash_attn_varlen_forward, ring_flash_attn_varlen_backward)
