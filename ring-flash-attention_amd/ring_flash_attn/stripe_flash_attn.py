"""Striped attention (token t lives on rank t mod W; Brandon et al. 2023).

Same public surface and step semantics as /root/reference/ring_flash_attn/stripe_flash_attn.py
(forward :7-101, backward :104-231, wrappers :300-378): always causal; at step s <= rank the block is
an ordinary causal block; at step s > rank the incoming keys are "one token ahead", so the block is
causal on the SHIFTED views q[:, 1:] x k[:, :-1] (:63-93), merged into rows [1:].
Built from the same kernels as the zigzag path: the shifted views are pointer offsets into the same
tensors (no copies), merged by the fused fp32 epilogue; dQ / dK / dV accumulate in fp32 in place.

Sliding windows over several ranks (no counterpart in the reference): token i of rank r is global token i W + r, so for
the queries of rank rq against the keys of rank rk (a = rq - rk) a causal window (wl, 0) of the global sequence is, in
LOCAL rows, the band  i + ceil((a - wl) / W) <= j <= i + floor(a / W)  — an ordinary dense shifted block
(`stripe_window_band`: mask_shift = floor(a / W), 0 or -1, causal, and a local left bound).  A block whose local left
bound comes out negative holds no visible element and is skipped — on every rank alike, it depends on (a, wl, W)
only.  The exchange stays a full rotation: a token's neighbours are strided over ALL ranks, so the compute follows the
window and the traffic does not.  The unwindowed code, with its sliced views, is untouched; a window that covers the
whole sequence (wl >= W S - 1) is dropped on the host and takes it.
"""
import torch

from . import _C
from .backend import get_backend
from .utils import RingComm, single_rank
from ._common import alibi_kw, dlse_kw, out_shape, dropout_arg, global_window, require_dropout_positions, require_mask_shift, stripe_map
from ._api import ScheduleSpec, make_autograd_function, make_api, _grad_buffers


def stripe_window_band(rank, src, world, window_left):
    """(mask_shift, local window_left) of the block of rank `rank`'s queries against rank `src`'s keys under a causal
    window of `window_left` global tokens, or None where no element of the block is visible"""
    a = rank - src
    hi = a // world                                  # floor(a / W): 0 (keys of a rank in front or this one) or -1
    lo = -((window_left - a) // world)               # ceil((a - wl) / W)
    return None if hi - lo < 0 else (hi, hi - lo)


def _stripe_window_forward(be, comm, q, k, v, softmax_scale, wl):
    B, S, H, D = q.shape
    W, rank = comm.world_size, comm.rank
    out_acc = torch.empty(out_shape(q, v), dtype=torch.float32, device=q.device)
    lse_acc = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    next_k, next_v = None, None
    for step in range(W):
        if step + 1 != W:
            next_k, next_v = comm.send_recv_kv(k, v)
        band = stripe_window_band(rank, (rank - step) % W, W, wl)
        if band is not None:                         # (step 0, a = 0, is always visible: it initialises the accumulators)
            shift = {"mask_shift": band[0]} if band[0] else {}
            be.fwd(q, k, v, softmax_scale=softmax_scale, causal=True, window=(band[1], -1),
                   out_acc=out_acc, lse_acc=lse_acc, acc_init=(step == 0), **shift)
        if step + 1 != W:
            comm.wait()
            k, v = next_k, next_v
    return be.cast(out_acc, q.dtype), lse_acc


def _stripe_window_backward(be, kv_comm, d_kv_comm, dout, q, k, v, softmax_lse, delta, softmax_scale, wl, deterministic):
    B, S, H, D = q.shape
    W, rank = kv_comm.world_size, kv_comm.rank
    dq = torch.empty((B, S, H, D), dtype=torch.float32, device=q.device)
    dk = torch.empty(k.shape, dtype=torch.float32, device=q.device)
    dv = torch.empty(v.shape, dtype=torch.float32, device=q.device)
    next_dk, next_dv = None, None
    next_k, next_v = None, None
    for step in range(W):
        if step + 1 != W:
            next_k, next_v = kv_comm.send_recv_kv(k, v)
        band = stripe_window_band(rank, (rank - step) % W, W, wl)
        if band is not None:
            common = dict(softmax_scale=softmax_scale, causal=True, window=(band[1], -1), deterministic=deterministic)
            if band[0]:
                common["mask_shift"] = band[0]
            if step == 0:
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
        if step + 1 != W:
            kv_comm.wait()
            k, v = next_k, next_v
        next_dk, next_dv = d_kv_comm.send_recv_kv(dk, dv)
    d_kv_comm.wait()
    return be.cast(dq, q.dtype), be.cast(next_dk, q.dtype), be.cast(next_dv, q.dtype)


def _stripe_dropout(be, rank, world, dropout_p, dropout_seed):
    """(src, shifted) -> the `dropout=` keyword of a block call against the K/V of rank `src` (nothing without dropout).
    The mask is a function of GLOBAL positions (include/rfa.h); local row i of rank x is global token i W + x — a
    position map with stride W (_common.stripe_map).  shifted: the `q[:, 1:]` x `k[:, :-1]` views of a step whose keys
    are one token ahead — the queries then start one stride later, the keys where they always start.
    The backward passes the forward's map with the forward's seed.  (Dropout with a window: _api._check_unsupported.)"""
    if not dropout_p or not dropout_p > 0:
        return lambda src, shifted: {}
    require_dropout_positions(be, "stripe_flash_attn")
    return lambda src, shifted: {"dropout": dropout_arg(dropout_p, dropout_seed,
                                                        q_map=stripe_map(rank, world, skip=1 if shifted else 0),
                                                        k_map=stripe_map(src, world))}


def stripe_flash_attn_forward(
    process_group,
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    softmax_scale,
    dropout_p=0,
    causal=True,
    window_size=(-1, -1),
    alibi_slopes=None,
    deterministic=False,
    dropout_seed=None,
):
    assert (
        causal
    ), "stripe flash attn only supports causal attention, if not causal, use ring flash attn instead"
    be = get_backend()
    comm = RingComm(process_group)
    B, S, H, D = q.shape

    if single_rank(comm.world_size):
        out = torch.empty(out_shape(q, v), dtype=q.dtype, device=q.device)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
        be.fwd(q, k, v, softmax_scale=softmax_scale, causal=True, out=out, lse=lse, window=window_size, dropout=dropout_arg(dropout_p, dropout_seed), **alibi_kw(alibi_slopes))
        return out, lse
    drop = _stripe_dropout(be, comm.rank, comm.world_size, dropout_p, dropout_seed)
    win = global_window(window_size, True, comm.world_size * S)
    if win is not None:
        require_mask_shift(be, "stripe_flash_attn")
        return _stripe_window_forward(be, comm, q, k, v, softmax_scale, win[0])

    out_acc = torch.empty(out_shape(q, v), dtype=torch.float32, device=q.device)
    lse_acc = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    next_k, next_v = None, None
    for step in range(comm.world_size):
        if step + 1 != comm.world_size:
            next_k, next_v = comm.send_recv_kv(k, v)

        src = (comm.rank - step) % comm.world_size                     # whose K/V are on hand
        if step <= comm.rank:
            be.fwd(q, k, v, softmax_scale=softmax_scale, causal=True,
                   out_acc=out_acc, lse_acc=lse_acc, acc_init=(step == 0), **drop(src, False))
        else:
            be.fwd(q[:, 1:], k[:, :-1], v[:, :-1], softmax_scale=softmax_scale, causal=True,
                   out_acc=out_acc[:, 1:], lse_acc=lse_acc[:, :, 1:], **drop(src, True))

        if step + 1 != comm.world_size:
            comm.wait()
            k, v = next_k, next_v

    return be.cast(out_acc, q.dtype), lse_acc


def stripe_flash_attn_backward(
    process_group,
    dout,
    q,
    k,
    v,
    out,
    softmax_lse,
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
    assert (
        causal
    ), "stripe flash attn only supports causal attention, if not causal, ring flash attn instead"
    be = get_backend()
    kv_comm = RingComm(process_group)
    d_kv_comm = RingComm(process_group)
    B, S, H, D = q.shape
    if not softmax_lse.is_contiguous():
        softmax_lse = softmax_lse.contiguous()
    if dout.stride(-1) != 1:
        dout = dout.contiguous()

    delta = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    be.bwd_preprocess(dout, out, delta, **dlse_kw(dlse))

    if single_rank(kv_comm.world_size):
        dq, dk, dv = _grad_buffers(out_grads, q, k, v)
        be.bwd(dout, q, k, v, softmax_lse, delta, softmax_scale=softmax_scale, causal=True,
               dq=dq, dk=dk, dv=dv, deterministic=deterministic, window=window_size, dropout=dropout_arg(dropout_p, dropout_seed), **alibi_kw(alibi_slopes))
        return dq, dk, dv
    drop = _stripe_dropout(be, kv_comm.rank, kv_comm.world_size, dropout_p, dropout_seed)
    win = global_window(window_size, True, kv_comm.world_size * S)
    if win is not None:
        require_mask_shift(be, "stripe_flash_attn")
        return _stripe_window_backward(be, kv_comm, d_kv_comm, dout, q, k, v, softmax_lse, delta, softmax_scale, win[0],
                                       deterministic)

    dq = torch.empty((B, S, H, D), dtype=torch.float32, device=q.device)
    dk = torch.empty(k.shape, dtype=torch.float32, device=q.device)
    dv = torch.empty(v.shape, dtype=torch.float32, device=q.device)
    next_dk, next_dv = None, None
    next_k, next_v = None, None
    dk_comm_buffer, dv_comm_buffer = None, None

    for step in range(kv_comm.world_size):
        if step + 1 != kv_comm.world_size:
            next_k, next_v = kv_comm.send_recv_kv(k, v)

        shift_causal = step > kv_comm.rank
        if shift_causal:
            args = (dout[:, 1:], q[:, 1:], k[:, :-1], v[:, :-1], softmax_lse[:, :, 1:], delta[:, :, 1:])
            dq_view = dq[:, 1:]
        else:
            args = (dout, q, k, v, softmax_lse, delta)
            dq_view = dq
        common = dict(softmax_scale=softmax_scale, causal=True, deterministic=deterministic,
                      **drop((kv_comm.rank - step) % kv_comm.world_size, shift_causal))

        if step == 0:
            be.bwd(*args, dq_acc=dq, dk_acc=dk, dv_acc=dv, acc_init=True, **common)
        else:
            # dQ (+= fp32) and per-head dK/dV partials while the dk/dv accumulators are in flight
            part = be.bwd(*args, dq_acc=dq_view, dk_acc=dk, dv_acc=dv, phases=_C.BWD_COMPUTE, **common)
            d_kv_comm.wait()
            dk_comm_buffer, dv_comm_buffer = dk, dv
            dk, dv = next_dk, next_dv
            if shift_causal:
                be.bwd(*args, dq_acc=dq_view, dk_acc=dk[:, :-1], dv_acc=dv[:, :-1], phases=_C.BWD_REDUCE,
                       partials=part, **common)
            else:
                be.bwd(*args, dq_acc=dq_view, dk_acc=dk, dv_acc=dv, phases=_C.BWD_REDUCE, partials=part, **common)

        if step + 1 != kv_comm.world_size:
            kv_comm.wait()
            k, v = next_k, next_v

        next_dk, next_dv = d_kv_comm.send_recv_kv(dk, dv, dk_comm_buffer, dv_comm_buffer)

    d_kv_comm.wait()

    return be.cast(dq, q.dtype), be.cast(next_dk, q.dtype), be.cast(next_dv, q.dtype)


SPEC = ScheduleSpec("StripeFlashAttnFunc", "stripe_flash_attn", vdim=True, window_ring=True, dropout_ring=True, must_be_causal=True)
StripeFlashAttnFunc = make_autograd_function(SPEC, stripe_flash_attn_forward, stripe_flash_attn_backward)
(
    stripe_flash_attn_func,
    stripe_flash_attn_kvpacked_func,
    stripe_flash_attn_qkvpacked_func,
) = make_api(SPEC, StripeFlashAttnFunc, stripe_flash_attn_forward, stripe_flash_attn_backward)
