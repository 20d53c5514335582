"""Basic ring attention (contiguous sequence shard per rank).

Same public surface and step semantics as /root/reference/ring_flash_attn/ring_flash_attn.py
(forward :7-67, backward :70-154, autograd :157-220, wrappers :223-301): at step s rank r holds
the K/V of rank (r-s) mod W; with `causal` only steps s <= r compute and only step 0 is masked.
See zigzag_ring_flash_attn.py for the MI355X-first changes (fused fp32 merge / accumulate,
strided views, two-phase backward, world_size==1 short-circuit).  One deliberate fix: dq is
returned in q.dtype (the reference hard-codes bfloat16 at ring_flash_attn.py:154).

Sliding windows over several ranks (no counterpart in the reference): the K/V on hand at step d belong to rank
r - d, i.e. they lie d * S rows in front of this rank's queries — the kernels are told so (`mask_shift`, include/rfa.h)
and band every block as ONE window over the whole sequence.  With a causal window of w rows only the
d_max = (w - 1) // S + 1 ranks in front of a query hold visible keys, whatever the rank: every rank stops
exchanging K/V after d_max hops and the dK/dV accumulators, d_max ranks from home by then, return in one direct
transfer (`ring_window_plan`).  Calls without a window that cuts the global sequence take the unwindowed code, unchanged.

ALiBi over several ranks rides on the same bookkeeping: the bias is a function of the global distance i - j, so the block
at signed rank distance t is told alibi_shift = t * S (include/rfa.h: rfa_ext_args) — `ring_window_plan` with both sides
unbounded walks all W steps, and the causal diagonal moves with the same t * S as a windowed call's.

Per-row key ranges (ring_flash_attn.with_row_ranges) take that route as well: the block at signed rank distance t holds the
keys of rank r - t, so its key row 0 sits at global position k_pos0 = (r - t) S; every block call gets this rank's
(start, end) and that one number (`row_ranges=`, include/rfa.h: rfa_rowrange_args), and the kernels skip what no row sees.

Block-sparse masks (ring_flash_attn.with_block_mask) travel the same way: every block call gets this rank's rows of the mask
(all of them) and the mask column of its key row 0, k_blk0 = (r - t) S / 128 (`block_mask=`, include/rfa.h: rfa_blockmask_args).
"""
import torch

from . import _C
from .backend import get_backend
from .utils import RingComm, single_rank
from ._common import alibi_kw, block_mask_kw, dlse_kw, out_shape, row_ranges_kw, dropout_arg, global_window, pos_map, require_dropout_positions, require_mask_shift
from ._api import ScheduleSpec, make_autograd_function, make_api, _grad_buffers


def ring_window_plan(rank, world_size, S, causal, window):
    """The steps of a windowed ring: (n_steps, dists) — the ring runs steps 0 .. n_steps - 1 (n_steps - 1 K/V hops) and
    dists[d] is the signed distance in RANKS between this rank's queries and the K/V on hand at step d (positive: keys
    in front), or None where the step computes nothing.  `window` = (left, right) of the GLOBAL sequence, a side < 0
    unbounded.  The block at distance t >= 1 has its nearest (query, key) pair (t - 1) S + 1 rows apart, so it holds a
    visible key iff left < 0 or left >= (t - 1) S + 1 — the same for every rank, which is what lets a causal ring stop
    early on all ranks at once; likewise the right side of keys behind the queries (never visible when causal)."""
    wl, wr = window

    def visible(t):
        if t == 0:
            return True
        if t > 0:
            return wl < 0 or wl >= (t - 1) * S + 1
        return not causal and (wr < 0 or wr >= (-t - 1) * S + 1)

    n_steps = world_size
    if causal:
        n_steps = world_size if wl < 0 else min(world_size, (wl - 1) // S + 2)
    dists = []
    for d in range(n_steps):
        t = d if d <= rank else d - world_size
        dists.append(t if visible(t) else None)
    return n_steps, dists


def _band(causal, window, t, S, alibi_slopes=None, row_ranges=None, rank=0, block_mask=None):
    """keywords of a block call t ranks off the diagonal (the shift only where it is not zero: backends that predate
    it serve the diagonal block unchanged; the bias only where there is one; the ranges only where there are some, with the
    global position of the block's key row 0)"""
    kw = {"causal": causal, "window": window}
    if t:
        kw["mask_shift"] = t * S
    kw.update(alibi_kw(alibi_slopes, t * S))
    if row_ranges is not None:
        kw["row_ranges"] = (row_ranges[0], row_ranges[1], (rank - t) * S)
    kw.update(block_mask_kw(block_mask, (rank - t) * S // 128))
    return kw


def _ring_window_forward(be, comm, q, k, v, softmax_scale, causal, window, alibi_slopes=None, row_ranges=None, block_mask=None):
    B, S, H, D = q.shape
    n_steps, dists = ring_window_plan(comm.rank, comm.world_size, S, causal, window)
    out_acc = torch.empty(out_shape(q, v), dtype=torch.float32, device=q.device)
    lse_acc = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    first = True
    next_k, next_v = None, None
    for step in range(n_steps):
        if step + 1 != n_steps:
            next_k, next_v = comm.send_recv_kv(k, v)
        if dists[step] is not None:
            be.fwd(q, k, v, softmax_scale=softmax_scale, out_acc=out_acc, lse_acc=lse_acc, acc_init=first,
                   **_band(causal, window, dists[step], S, alibi_slopes, row_ranges, comm.rank, block_mask))
            first = False
        if step + 1 != n_steps:
            comm.wait()
            k, v = next_k, next_v
    return be.cast(out_acc, q.dtype), lse_acc


def _ring_window_backward(be, process_group, kv_comm, d_kv_comm, dout, q, k, v, softmax_lse, delta, softmax_scale,
                          causal, window, deterministic, alibi_slopes=None, row_ranges=None, block_mask=None):
    B, S, H, D = q.shape
    world = kv_comm.world_size
    n_steps, dists = ring_window_plan(kv_comm.rank, world, S, causal, window)
    dq = None
    dk = torch.empty(k.shape, dtype=torch.float32, device=q.device)
    dv = torch.empty(v.shape, dtype=torch.float32, device=q.device)
    next_dk, next_dv = None, None
    next_k, next_v = None, None
    for step in range(n_steps):
        if step + 1 != n_steps:
            next_k, next_v = kv_comm.send_recv_kv(k, v)
        if dists[step] is not None:
            band = _band(causal, window, dists[step], S, alibi_slopes, row_ranges, kv_comm.rank, block_mask)
            if dq is None:                       # step 0: the diagonal block always computes
                dq = torch.empty((B, S, H, D), dtype=torch.float32, device=q.device)
                be.bwd(dout, q, k, v, softmax_lse, delta, softmax_scale=softmax_scale,
                       dq_acc=dq, dk_acc=dk, dv_acc=dv, acc_init=True, deterministic=deterministic, **band)
            else:
                part = be.bwd(dout, q, k, v, softmax_lse, delta, softmax_scale=softmax_scale,
                              dq_acc=dq, dk_acc=dk, dv_acc=dv, deterministic=deterministic,
                              phases=_C.BWD_COMPUTE, **band)
                d_kv_comm.wait()
                dk, dv = next_dk, next_dv
                be.bwd(dout, q, k, v, softmax_lse, delta, softmax_scale=softmax_scale,
                       dq_acc=dq, dk_acc=dk, dv_acc=dv, deterministic=deterministic,
                       phases=_C.BWD_REDUCE, partials=part, **band)
        elif step != 0:
            d_kv_comm.wait()
            dk, dv = next_dk, next_dv
        if step + 1 != n_steps:
            kv_comm.wait()
            k, v = next_k, next_v
            next_dk, next_dv = d_kv_comm.send_recv_kv(dk, dv)
    # the accumulators are n_steps - 1 ranks in front of their owners: home in ONE transfer (a full rotation: the
    # ring's own last hop, distance 1)
    back = (n_steps - 1) % world
    if back:
        home = RingComm(process_group, distance=-back)
        dk, dv = home.send_recv_kv(dk, dv)
        home.wait()
    return be.cast(dq, q.dtype), be.cast(dk, q.dtype), be.cast(dv, q.dtype)


def _ring_dropout(be, comm, S, dropout_p, dropout_seed):
    """step -> the `dropout=` keyword of that step's block call (nothing without dropout).  The mask is a function of
    GLOBAL positions (include/rfa.h): this rank's queries are rows rank * S ..., the K/V on hand at step d those of rank
    rank - d — every block draws the bits the unsharded call draws there, and the backward, which walks the same steps
    with the forward's seed, the forward's.  (Dropout together with a window never gets here: _api._check_unsupported.)"""
    if not dropout_p or not dropout_p > 0:
        return lambda step: {}
    require_dropout_positions(be, "ring_flash_attn")
    rank, world = comm.rank, comm.world_size
    return lambda step: {"dropout": dropout_arg(dropout_p, dropout_seed, q_map=pos_map(rank * S),
                                                k_map=pos_map(((rank - step) % world) * S))}


def ring_flash_attn_forward(
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
    row_ranges=None,
    block_mask=None,
):
    """row_ranges: (start, end) of a call bound by with_row_ranges — this rank's rows, global key positions — or None;
    block_mask: the (Bm, Hm, NQ, NK) mask of a call bound by with_block_mask — this rank's query blocks, all key blocks — or None"""
    be = get_backend()
    comm = RingComm(process_group)
    B, S, H, D = q.shape

    if single_rank(comm.world_size):
        out = torch.empty(out_shape(q, v), dtype=q.dtype, device=q.device)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
        be.fwd(q, k, v, softmax_scale=softmax_scale, causal=causal, out=out, lse=lse, window=window_size, dropout=dropout_arg(dropout_p, dropout_seed),
               **alibi_kw(alibi_slopes), **row_ranges_kw(row_ranges, 0), **block_mask_kw(block_mask, 0))
        return out, lse
    drop = _ring_dropout(be, comm, S, dropout_p, dropout_seed)

    win = global_window(window_size, causal, comm.world_size * S)
    if alibi_slopes is not None:                 # (never together with a window: _api._check_unsupported)
        win = (-1, -1)
    if (row_ranges is not None or block_mask is not None) and win is None:   # (ranges and block masks ride on the windowed route's bookkeeping, with or without a window)
        win = (-1, -1)
    if win is not None:
        require_mask_shift(be, "ring_flash_attn")
        return _ring_window_forward(be, comm, q, k, v, softmax_scale, causal, win, alibi_slopes, row_ranges, block_mask)

    out_acc = torch.empty(out_shape(q, v), dtype=torch.float32, device=q.device)
    lse_acc = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    first = True
    next_k, next_v = None, None

    for step in range(comm.world_size):
        if step + 1 != comm.world_size:
            next_k, next_v = comm.send_recv_kv(k, v)

        if not causal or step <= comm.rank:
            be.fwd(q, k, v, softmax_scale=softmax_scale, causal=causal and step == 0,
                   out_acc=out_acc, lse_acc=lse_acc, acc_init=first, **drop(step))
            first = False

        if step + 1 != comm.world_size:
            comm.wait()
            k, v = next_k, next_v

    out = be.cast(out_acc, q.dtype)
    return out, lse_acc


def ring_flash_attn_backward(
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
    row_ranges=None,
    block_mask=None,
):
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
        be.bwd(dout, q, k, v, softmax_lse, delta, softmax_scale=softmax_scale, causal=causal,
               dq=dq, dk=dk, dv=dv, deterministic=deterministic, window=window_size, dropout=dropout_arg(dropout_p, dropout_seed),
               **alibi_kw(alibi_slopes), **row_ranges_kw(row_ranges, 0), **block_mask_kw(block_mask, 0))
        return dq, dk, dv
    drop = _ring_dropout(be, kv_comm, S, dropout_p, dropout_seed)

    win = global_window(window_size, causal, kv_comm.world_size * S)
    if alibi_slopes is not None:
        win = (-1, -1)
    if (row_ranges is not None or block_mask is not None) and win is None:
        win = (-1, -1)
    if win is not None:
        return _ring_window_backward(be, process_group, kv_comm, d_kv_comm, dout, q, k, v, softmax_lse, delta,
                                     softmax_scale, causal, win, deterministic, alibi_slopes, row_ranges, block_mask)

    dq = None
    dk = torch.empty(k.shape, dtype=torch.float32, device=q.device)
    dv = torch.empty(v.shape, dtype=torch.float32, device=q.device)
    next_dk, next_dv = None, None
    next_k, next_v = None, None

    for step in range(kv_comm.world_size):
        if step + 1 != kv_comm.world_size:
            next_k, next_v = kv_comm.send_recv_kv(k, v)

        if step <= kv_comm.rank or not causal:
            bwd_causal = causal and step == 0
            if dq is None:
                dq = torch.empty((B, S, H, D), dtype=torch.float32, device=q.device)
                be.bwd(dout, q, k, v, softmax_lse, delta, softmax_scale=softmax_scale, causal=bwd_causal,
                       dq_acc=dq, dk_acc=dk, dv_acc=dv, acc_init=True, deterministic=deterministic, **drop(step))
            else:
                part = be.bwd(dout, q, k, v, softmax_lse, delta, softmax_scale=softmax_scale, causal=bwd_causal,
                              dq_acc=dq, dk_acc=dk, dv_acc=dv, deterministic=deterministic,
                              phases=_C.BWD_COMPUTE, **drop(step))
                d_kv_comm.wait()
                dk, dv = next_dk, next_dv
                be.bwd(dout, q, k, v, softmax_lse, delta, softmax_scale=softmax_scale, causal=bwd_causal,
                       dq_acc=dq, dk_acc=dk, dv_acc=dv, deterministic=deterministic,
                       phases=_C.BWD_REDUCE, partials=part, **drop(step))
        elif step != 0:
            d_kv_comm.wait()
            dk, dv = next_dk, next_dv

        if step + 1 != kv_comm.world_size:
            kv_comm.wait()
            k, v = next_k, next_v

        next_dk, next_dv = d_kv_comm.send_recv_kv(dk, dv)

    d_kv_comm.wait()

    return be.cast(dq, q.dtype), be.cast(next_dk, q.dtype), be.cast(next_dv, q.dtype)


SPEC = ScheduleSpec("RingFlashAttnFunc", "ring_flash_attn", vdim=True, window_ring=True, dropout_ring=True, alibi_ring=True)
RingFlashAttnFunc = make_autograd_function(SPEC, ring_flash_attn_forward, ring_flash_attn_backward)
(
    ring_flash_attn_func,
    ring_flash_attn_kvpacked_func,
    ring_flash_attn_qkvpacked_func,
) = make_api(SPEC, RingFlashAttnFunc, ring_flash_attn_forward, ring_flash_attn_backward)
